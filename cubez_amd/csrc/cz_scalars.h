// cz_scalars.h -- the one layout of the driver's device scalars (CZ::d_res) and of their pinned host mirror (CZ::h_scal), and of the device
// convergence words (CZ::d_flag).  A host field mirrors the device field of the same name (CZ::fetch); DESIGN.md §5.21 has the table.
// Every member is scratch of one call of the driver -- nothing reads it after the call that wrote it returned -- except `rhs_mean`.
// How a member is written is noted beside it: "stored" = the workgroup that arrives last stores a fixed-order sum (or one thread a scalar),
// so the member needs no zeroing and no other user's store.  A run of members that a kernel or a copy takes as neighbours is an array or a
// sub-struct that names the consumer, and is pinned by a static_assert below.
#ifndef CZ_SCALARS_H_
#define CZ_SCALARS_H_

#include <cstddef>

#include "cz_internal.h"

struct CzScalars {
  // the residual sums of the sweeps of one pass: a fused pass stores up to four (jac4_k), the colour and line kernels take (pass, slot),
  // check2 reads two.  Stored; the SPLIT pass then folds its slabs' sums into what its interior launch stored (pair_shell_fold_async)
  double pass[4];
  double rerun[4];      // ... of the re-run of a converged first iteration (fused_end): up to three sweeps.  Stored, never read
  double lagged[2][2];  // ... of pass p of the lagged split, in lagged[p & 1]: two sweeps (check2).  Stored, then folded into, like `pass`
  double fdot;          // Fdot1 / Fdot2.  Stored
  // BiCGSTAB's three pairs of dots; they live across a whole Preconditioner() solve, which writes `pass`.  Each pair is one launch's
  // out[0], out[1] (calc_ax_dots, triad_dots) and one all-reduce / copy of two.  Stored
  struct Bicg {
    double q_r0[2];     // q.r0 (and q.q)
    double t_s[2];      // t.s, t.t
    double r_r[2];      // r.r, r.r0
  } bicg;
  // PCG's dots.  rho .. rr: read back in ONE copy of four (the one wait of an iteration); pq, qq: out[0], out[1] of calc_ax_dots / coef_ax;
  // rr, rsum: the closed update stores sum r^2 and sum r side by side (one all-reduce of two).  Stored
  struct Cg {
    double rho, pq, qq, rr, rsum;
  } cg;
  double cg_r0[2];      // out[0], out[1] of coef_ax's r = b - A x at PCG's start (not read).  Stored
  double comm_sum;      // Comm_SUM_1: a host value in, its all-reduced sum out.  Copied in
  double field_sumsq[2];  // [0] sum r^2 of cz_get_residual, sum div^2 of cz_set_rhs_div ([1]: the second sum of coef_ax's out[0], out[1], not read).  Stored
  double project[2];    // project(): this rank's sum A', sum A'^2 of the pass that shifts (before it: sum A in [0]).  Stored
  // the bad-value count of the face coefficients: counted atomically by coef_prep_k, zeroed by coef_prepare's own memset before
  alignas(8) unsigned coef_bad;
  // the scalars made on the device (czhip_internal::ScCg / ScBicg, written by one thread of cg_scal_k / bicg_scal_k) and, behind them as
  // the closed update reads it (sc[SC_LAG_MEAN]), the lagged mean of the residual (mean_scal_k)
  alignas(8) CZ_REAL sc[5];
  alignas(8) CZ_REAL closed_mean[2];  // the means of the closed box's steps 1 and 3 as cz_closed_mean reports them: read back in one copy (mean_scal_k)
  // LIVES ACROSS CALLS: the mean cz_set_rhs removed on a closed box, until cz_closed_mean(0) fetches it (CZ::closed_m0_on_device).  mean_scal_k
  alignas(8) CZ_REAL rhs_mean;
};

// the device convergence words: what the check kernels set and the passes skip on
struct CzFlags {
  int converged;  // set by the test of the iteration that met eps: launches queued behind it are no-ops
  int iteration;  // ... that iteration
  int snap[2];    // the lagged split: `converged` as the test of pass p - 2 left it, in snap[p & 1] (split_pass)
};

static_assert(sizeof(CzScalars) % 8 == 0 && sizeof(CzScalars) <= 48 * sizeof(double), "the block is a few dozen doubles");
static_assert(offsetof(CzScalars, cg.rr) - offsetof(CzScalars, cg.rho) == 3 * sizeof(double), "PCG reads rho .. rr back in one copy of four");
static_assert(offsetof(CzScalars, cg.qq) - offsetof(CzScalars, cg.pq) == sizeof(double), "calc_ax_dots / coef_ax store out[0], out[1]");
static_assert(offsetof(CzScalars, cg.rsum) - offsetof(CzScalars, cg.rr) == sizeof(double), "the closed update stores r.r and sum r side by side");
static_assert(sizeof(CzScalars::Bicg) == 6 * sizeof(double), "BiCGSTAB's pairs");
static_assert(czhip_internal::SC_LAG_MEAN == 4 && sizeof(CzScalars::sc) == 5 * sizeof(CZ_REAL), "cg_update_k<CLOSED> reads the mean at sc[4]");
static_assert(offsetof(CzScalars, sc) % 8 == 0 && offsetof(CzScalars, closed_mean) % 8 == 0 && offsetof(CzScalars, rhs_mean) % 8 == 0, "REAL members on 8 bytes");
static_assert(offsetof(CzScalars, rhs_mean) >= offsetof(CzScalars, closed_mean) + sizeof(CzScalars::closed_mean), "the one member that lives across calls is in no scratch group");
static_assert(offsetof(CzFlags, iteration) == sizeof(int) && offsetof(CzFlags, snap) == 2 * sizeof(int) && sizeof(CzFlags) == 4 * sizeof(int), "flag, iteration: one copy of two; four words in all");

#endif
