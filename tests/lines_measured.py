# Recorded results of the zebra line smoother along Z.  Data only; tests/test_lines_oracle.py re-measures every row.
# iterations to eps 1e-8 at 33 x 47 x 61, FP64, the seeded problem, pcg mgrb with the coefficient hierarchy -- (field, state):
# (zebra Z-lines at coef 1.0, point colour sweeps at coef 1.2)
COUNTS = {
    ("anisoz100", "dirichlet"): (5, 46),
    ("anisoz100", "inflow"): (8, 68),
    ("anisoz100", "closed"): (6, 68),
    ("stretch30", "dirichlet"): (7, 25),
    ("stretch30", "inflow"): (8, 62),
    ("stretch30", "closed"): (7, 58),
    ("random", "dirichlet"): (9, 9),
    ("random", "inflow"): (10, 10),
    ("random", "closed"): (8, 8),
}
# `ones`, Dirichlet faces, lines at coef 1.0
ONES = 9
