// cz_solvers.h -- the solvers and preconditioners of the command line: one row per name, stated once.
//
// Everything the driver and the command line know about a name -- how it is spelled and printed, where it is accepted, whether it is a
// MAF form, which loop runs it, what CZ::Preconditioner does with it, what a line solver's iteration is made of -- is a row of `table`.
// Plain C++17, no HIP: cz_main.cpp includes it for the usage text.
//
// Adding a solver: one enumerator, one row.  A loop in cz_driver.cpp (and a case in CZ::run) only if its family is new.
#ifndef CZ_SOLVERS_H_
#define CZ_SOLVERS_H_

#include <strings.h>

#include <string>

// cz_Define.h:68-89: the reference's values (LS_PCG, LS_MG, LS_MGRB: beyond the reference).  Nothing compares them by order.
enum LinearSolver { LS_NONE = 0, LS_PSOR = 1, LS_SOR2SMA, LS_BICGSTAB, LS_JACOBI, LS_PCR = 5, LS_PCR_EDA, LS_PCR_ESA, LS_PCR_RB, LS_PCR_RB_ESA, LS_PCR_J_ESA, LS_PSOR_MAF = 11, LS_SOR2SMA_MAF, LS_BICGSTAB_MAF, LS_JACOBI_MAF, LS_PCR_MAF, LS_PCR_EDA_MAF, LS_PCR_ESA_MAF, LS_PCR_RB_MAF, LS_PCR_RB_ESA_MAF, LS_PCG, LS_MG, LS_MGRB };

namespace cz_solvers {

// where a name is accepted: as linear_solver; as precond of pbicgstab[_maf]; as precond of pcg
enum Role : unsigned { SOLVER = 1, PRE_BICG = 2, PRE_PCG = 4 };
// the loop of cz_driver.cpp that runs it (NO_LOOP: none, and the V-cycles, which only pcg applies)
enum Family { NO_LOOP, JACOBI, RBSOR, PSOR, LINE, BICGSTAB, PCG };
enum LineKernel { NO_LINE, PCR_RB, PCR_VARIANT, PCR_MAF };  // pcr_rb_async / pcr_variant_async / pcr_maf_async

// One iteration of a line solver (CZ::LSOR).  order: 0 two colours, 1 lexicographic, 2 Jacobi order through WRK.  final4: the reduction ends
// in 4x4 systems (pcr_variant_async).  fin: flops of one final system in the kernel family's flop formula (CZ::line_flop).
struct Line {
  LineKernel kernel;
  int order, final4;
  double fin;
};

struct Row {
  int id;
  const char* name;     // on the command line (matched without regard to case); the history file is name + ".txt"
  const char* printed;  // "Iterative Mehtod = ", "Preconditioner = ", profiling.txt
  unsigned roles;
  bool maf;             // sets SW_maf, as solver and as preconditioner
  Family family;
  bool precond_runs;    // CZ::Preconditioner runs the family's loop; false: it copies (PBiCGSTAB then takes the right-hand side itself)
  Line line;
};

constexpr Line no_line{NO_LINE, 0, 0, 0.0};
constexpr unsigned S = SOLVER, SB = SOLVER | PRE_BICG;

// The rows stand in the order the usage text and the refusals list the names (not the enum's): look a row up by id, never index by it.
//   pcr_esa, pcr_esa_maf: solvers only.  pcr_j_esa: accepted as a preconditioner, but CZ::Preconditioner has no loop for it (nor has the
//   reference, cz_Poisson.cpp:282-321): it copies -- and still counts as a line solver where MSK is allocated.
constexpr Row table[] = {
    {LS_NONE, "none", "NONE", PRE_BICG | PRE_PCG, false, NO_LOOP, false, no_line},
    {LS_JACOBI, "jacobi", "JACOBI", SB | PRE_PCG, false, JACOBI, true, no_line},
    {LS_PSOR, "psor", "PSOR", SB, false, PSOR, true, no_line},
    {LS_SOR2SMA, "sor2sma", "SOR2SMA", SB, false, RBSOR, true, no_line},
    {LS_BICGSTAB, "pbicgstab", "PBiCGSTAB", S, false, BICGSTAB, false, no_line},
    {LS_PCR, "pcr", "PCR", SB, false, LINE, true, {PCR_VARIANT, 1, 1, 74.0}},
    {LS_PCR_EDA, "pcr_eda", "PCR_EDA", SB, false, LINE, true, {PCR_VARIANT, 1, 0, 9.0}},
    {LS_PCR_ESA, "pcr_esa", "PCR_ESA", S, false, LINE, false, {PCR_VARIANT, 1, 1, 78.0}},
    {LS_PCR_RB, "pcr_rb", "PCR_RB", SB, false, LINE, true, {PCR_RB, 0, 0, 0.0}},
    {LS_PCR_RB_ESA, "pcr_rb_esa", "PCR_RB_ESA", SB, false, LINE, true, {PCR_VARIANT, 0, 1, 78.0}},
    {LS_PCR_J_ESA, "pcr_j_esa", "PCR_J_ESA", SB, false, LINE, false, {PCR_VARIANT, 2, 0, 9.0}},
    {LS_JACOBI_MAF, "jacobi_maf", "JACOBI_MAF", SB, true, JACOBI, true, no_line},
    {LS_PSOR_MAF, "psor_maf", "PSOR_MAF", SB, true, PSOR, true, no_line},
    {LS_SOR2SMA_MAF, "sor2sma_maf", "SOR2SMA_MAF", SB, true, RBSOR, true, no_line},
    {LS_BICGSTAB_MAF, "pbicgstab_maf", "PBiCGSTAB_MAF", S, true, BICGSTAB, false, no_line},
    {LS_PCR_MAF, "pcr_maf", "PCR_MAF", SB, true, LINE, true, {PCR_MAF, 1, 0, 11.0}},
    {LS_PCR_EDA_MAF, "pcr_eda_maf", "PCR_EDA_MAF", SB, true, LINE, true, {PCR_MAF, 1, 0, 9.0}},
    {LS_PCR_ESA_MAF, "pcr_esa_maf", "PCR_ESA_MAF", S, true, LINE, false, {PCR_MAF, 1, 0, 9.0}},
    {LS_PCR_RB_MAF, "pcr_rb_maf", "PCR_RB_MAF", SB, true, LINE, true, {PCR_MAF, 0, 0, 11.0}},
    {LS_PCR_RB_ESA_MAF, "pcr_rb_esa_maf", "PCR_RB_ESA_MAF", SB, true, LINE, true, {PCR_MAF, 0, 0, 11.0}},
    {LS_PCG, "pcg", "PCG", S, false, PCG, false, no_line},
    {LS_MG, "mg", "MG", PRE_PCG, false, NO_LOOP, false, no_line},
    {LS_MGRB, "mgrb", "MGRB", PRE_PCG, false, NO_LOOP, false, no_line},
};

// the row of an id (an id without a row reads as none)
inline const Row& row(int id) {
  for (const Row& r : table)
    if (r.id == id) return r;
  return table[0];
}

// the row a name selects in a role; nullptr: not accepted there
inline const Row* find(const char* name, unsigned role) {
  for (const Row& r : table)
    if ((r.roles & role) && !strcasecmp(name, r.name)) return &r;
  return nullptr;
}

// "a | b | c": the names of a role, in table order
inline std::string list(unsigned role) {
  std::string s;
  for (const Row& r : table)
    if (r.roles & role) s += (s.empty() ? "" : " | ") + std::string(r.name);
  return s;
}

inline bool krylov(const Row& r) { return r.family == BICGSTAB || r.family == PCG; }

}  // namespace cz_solvers

#endif
