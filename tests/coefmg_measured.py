"""Recorded results of tests/coefmg_parity.py (data only; tests/test_coefmg_oracle.py re-measures every row)."""
# iterations to eps 1e-8 at 33 x 47 x 61, FP64, Dirichlet faces, the seeded problem, with the coefficient cycle (cz_set_coef_mg) -- (field, run)
COUNTS = {
    ('random', 'mgrb'): 9,
    ('random', 'mg'): 15,
    ('smooth4', 'mgrb'): 9,
    ('smooth4', 'mg'): 16,
    ('smooth10', 'mgrb'): 10,
    ('smooth10', 'mg'): 16,
    ('bubble10', 'mgrb'): 11,
    ('bubble10', 'mg'): 18,
    ('bubble100', 'mgrb'): 13,
    ('bubble100', 'mg'): 22,
    ('bubble1000', 'mgrb'): 15,
    ('bubble1000', 'mg'): 27,
    ('aniso4', 'mgrb'): 11,
    ('aniso4', 'mg'): 23,
    ('ones', 'mgrb'): 9,
    ('ones', 'mg'): 15,
}
# the scaled preconditioner (flag off) on the fields that coef_measured.COUNTS does not hold
SCALED = {
    ('random', 'mgrb'): 21,
    ('random', 'mg'): 26,
}
