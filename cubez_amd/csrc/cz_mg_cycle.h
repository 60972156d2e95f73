// cz_mg_cycle.h -- the V-cycle of pcg ... mg and pcg ... mgrb as far as the single-domain hierarchy (cz_h_mg.h) and the distributed one
// (cz_mg_dist.cpp) share it: which levels there are, and the order of a cycle.  The order is stated here and nowhere else on the host
// (mg_tail_k states it once more on the device, for the levels it runs from LDS).
#ifndef CZ_MG_CYCLE_H_
#define CZ_MG_CYCLE_H_

#include <algorithm>

constexpr int MG_MAXLEV = 32;  // levels of a hierarchy at most (ceil(log2 n) + 1 for any int extent)

// the levels below a level of n points per direction: ceil(n / 2) per direction until the largest extent is <= 4 (the coarsest level).
// dims[0] = n; returns the number of levels, 0 if there are more than max
inline int mg_level_dims(const int* n, int (*dims)[3], int max) {
  for (int d = 0; d < 3; d++) dims[0][d] = n[d];
  for (int l = 0; l < max; l++) {
    if (std::max(dims[l][0], std::max(dims[l][1], dims[l][2])) <= 4) return l + 1;
    if (l + 1 < max)
      for (int d = 0; d < 3; d++) dims[l + 1][d] = (dims[l][d] + 1) / 2;
  }
  return 0;
}

// x_l = V_l(b_l).  Ops names the arrays and launches (and, decomposed, exchanges):
//   whole(l)          true if it ran levels l .. coarsest in one go (the tail kernel; the gathered levels of a decomposed run)
//   pair(l, zero, post)  x_l <- two smoothing iterations from x_l (zero: from zero).  mg: relaxed Jacobi sweeps, post is not looked at.
//                     mgrb: red-black iterations, forward (colour 0, 1) before the coarse correction and backward (colour 1, 0: post) after it,
//                     which makes the post-smoother the adjoint of the pre-smoother
//   restrict_down(l)  b_{l+1} <- the residual of x_l summed over the children
//   prolong_up(l)     x_l <- x_l + alpha x_{l+1}(parent)
template <class Ops>
void mg_walk(Ops& ops, int l, int coarsest) {
  if (ops.whole(l)) return;
  if (l == coarsest) {  // eight iterations from zero: four as before a correction, four as after one
    ops.pair(l, true, false);
    ops.pair(l, false, false);
    for (int s = 0; s < 2; s++) ops.pair(l, false, true);
    return;
  }
  ops.pair(l, true, false);
  ops.restrict_down(l);
  mg_walk(ops, l + 1, coarsest);
  ops.prolong_up(l);
  ops.pair(l, false, true);
}

#endif
