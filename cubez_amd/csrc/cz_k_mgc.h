// cz_k_mgc.h -- part of cz_kernels.hip (ONE translation unit per precision; this file is included inside its anonymous
// namespace and is not a stand-alone header): the V-cycle of pcg ... mg | mgrb with the face coefficients of cz_set_face_coef inside the
// hierarchy (cz_set_coef_mg).
//
// The levels, the walk, the per-point functions, the level kernels and the tail are those of cz_k_mg.h, instantiated with the weights
// policies MgArr / MgArrG / MgcTail there; only the weights change, and this file holds what is the arrays' own: level 0's row kernels and
// the build.  Level l keeps three
// face-weight arrays X, Y, Z and a diagonal D with the geometry of the level's own arrays (MgLev): X(I, J, K) is the link between points I
// and I + 1, I = -1 .. n - 1; -1 and n - 1 are the box's two faces, and the -1 entry lives in the array's shell.  Level 0's X, Y, Z are the
// handle's own padded coefficient arrays (face 0 of a periodic direction already holds the copy of face n - 2, coef_prep_k).  Level l + 1's
// weights are the sums of the fine face weights that cross the aggregate's face (mgc_coarsen_k), the exact Galerkin product for
// piecewise-constant aggregation; with unit coefficients they are the integers of mg_weights, and every kernel then gives the bits
// of the constant cycle.  A face that carries no link -- a Neumann face of the box, the seam of a periodic direction on a level of one
// point -- is stored as a zero weight from level 1 on, so these levels need neither mask nor mirror.
//   ss = X(I) u(I+1) + X(I-1) u(I-1) + Y(J) u(J+1) + Y(J-1) u(J-1) + Z(K) u(K+1) + Z(K-1) u(K-1), left to right
//   sweep pn = pp + ((ss - bb) / D - pp) omg (IEEE division), residual b - (ss - D x), D = ((X(I) + X(I-1)) + (Y(J) + Y(J-1))) + (Z(K) + Z(K-1))
// every operation rounded once in REAL.  No kernel here reduces anything: the cycle is deterministic, bit for bit.

// ---- level 0, the hot path: the row form of ax_coef_k.  k across the lanes, a row cut into the 16-byte vectors of the array written, stored
// aligned; every operand loaded with REAL-aligned 16-byte loads (the rows i - 1, i + 1, j - 1, j + 1 of u and i - 1, j - 1 of X, Y are the
// rows neighbouring threads ask for at the same time: L2 / MALL); a vector that the box cuts goes cell by cell through the per-point
// functions of cz_k_mg.h.  The same operations in the same order: the bits of mg_smooth_k / mg_rb_k with MgArr.
// the relaxed update of the V cells at element e (pc: their own values; not read where ZPP)
template <int V, bool ZERO, bool ZPP>
__device__ __forceinline__ Vec<V> mgc0_vec(const REAL* u, const REAL* __restrict__ b, const MgcW& W, long long e, long long si, long long sj, REAL omg,
                                           const Vec<V>& pc) {
  const Vec<V> bb = ldve<V>(b, e), dd = ldve<V>(W.d, e);
  Vec<V> q;
  if (ZERO) {
#pragma unroll
    for (int cc = 0; cc < V; cc++) {
      const REAL pp = (REAL)0;
      const REAL dp = (((REAL)0 - bb.v[cc]) / dd.v[cc] - pp) * omg;
      q.v[cc] = pp + dp;
    }
    return q;
  }
  const Vec<V> pim = ldve<V>(u, e - si), pip = ldve<V>(u, e + si), pjm = ldve<V>(u, e - sj), pjp = ldve<V>(u, e + sj);
  const Vec<V> xc = ldve<V>(W.x, e), xm = ldve<V>(W.x, e - si), yc = ldve<V>(W.y, e), ym = ldve<V>(W.y, e - sj), zc = ldve<V>(W.z, e);
  const REAL kl = u[e - 1], kr = u[e + V], zl = W.z[e - 1];
#pragma unroll
  for (int cc = 0; cc < V; cc++) {
    const REAL km1 = cc == 0 ? kl : pc.v[cc > 0 ? cc - 1 : 0];
    const REAL kp1 = cc == V - 1 ? kr : pc.v[cc < V - 1 ? cc + 1 : V - 1];
    const REAL zm = cc == 0 ? zl : zc.v[cc > 0 ? cc - 1 : 0];
    const REAL ss = xc.v[cc] * pip.v[cc] + xm.v[cc] * pim.v[cc] + yc.v[cc] * pjp.v[cc] + ym.v[cc] * pjm.v[cc] + zc.v[cc] * kp1 + zm * km1;
    const REAL pp = ZPP ? (REAL)0 : pc.v[cc];
    const REAL dp = ((ss - bb.v[cc]) / dd.v[cc] - pp) * omg;
    q.v[cc] = pp + dp;
  }
  return q;
}

// grid (x: vectors of the rows of a plane, y: planes), both strided; slots: the vectors a row can touch, whatever its phase
template <int V, bool ZERO>
__global__ void __launch_bounds__(256) mgc0_smooth_k(const REAL* __restrict__ u, REAL* __restrict__ w, const REAL* __restrict__ b, const MgLev L, const MgcW W,
                                                     const REAL omg, const int slots) {
  const int per_plane = L.ni * slots;
  const long long si = L.nkp, sj = (long long)L.nkp * L.nip;
  for (int J = blockIdx.y; J < L.nj; J += gridDim.y) {
    for (int it = blockIdx.x * 256 + threadIdx.x; it < per_plane; it += gridDim.x * 256) {
      const int I = it / slots, s = it - I * slots;
      const long long a = mg_at(L, I, J, 0);
      const int ph = (int)((reinterpret_cast<uintptr_t>(w + a) / sizeof(REAL)) & (uintptr_t)(V - 1));
      const int e0 = s * V - ph;
      if (e0 > L.nk - 1 || e0 + V - 1 < 0) continue;
      if (e0 >= 0 && e0 + V - 1 <= L.nk - 1) {
        const long long e = a + e0;
        Vec<V> pc = zerov<V>();
        if (!ZERO) pc = ldve<V>(u, e);
        stv<V>(w + e, 0, mgc0_vec<V, ZERO, ZERO>(u, b, W, e, si, sj, omg, pc));
      } else {  // a vector that the box cuts
        const int c1 = e0 + V - 1 < L.nk - 1 ? e0 + V - 1 : L.nk - 1;
        for (int K = e0 > 0 ? e0 : 0; K <= c1; K++) w[a + K] = mg_sweep_pt<ZERO>(u, b, L, MgArr{W}, I, J, K, omg);
      }
    }
  }
}

// one colour sweep of level 0 IN PLACE: the vector is read, its cells of colour c ((I + J + K) & 1) take the update, and it is stored whole --
// the cells of the other colour, which the neighbouring threads read, are written back with the bytes they hold.  Z as mg_rb_pt
template <int V, int Z>
__global__ void __launch_bounds__(256) mgc0_rb_k(REAL* x, const REAL* __restrict__ b, const MgLev L, const MgcW W, const REAL omg, const int c, const int slots) {
  const int per_plane = L.ni * slots;
  const long long si = L.nkp, sj = (long long)L.nkp * L.nip;
  for (int J = blockIdx.y; J < L.nj; J += gridDim.y) {
    for (int it = blockIdx.x * 256 + threadIdx.x; it < per_plane; it += gridDim.x * 256) {
      const int I = it / slots, s = it - I * slots;
      const long long a = mg_at(L, I, J, 0);
      const int ph = (int)((reinterpret_cast<uintptr_t>(x + a) / sizeof(REAL)) & (uintptr_t)(V - 1));
      const int e0 = s * V - ph;
      if (e0 > L.nk - 1 || e0 + V - 1 < 0) continue;
      if (e0 >= 0 && e0 + V - 1 <= L.nk - 1) {
        const long long e = a + e0;
        const Vec<V> pc = ldv<V>(x + e, 0);
        const Vec<V> q = mgc0_vec<V, Z == 1, Z != 0>(x, b, W, e, si, sj, omg, pc);
        Vec<V> out;
#pragma unroll
        for (int cc = 0; cc < V; cc++) out.v[cc] = ((I + J + e0 + cc + c) & 1) == 0 ? q.v[cc] : pc.v[cc];
        stv<V>(x + e, 0, out);
      } else {  // a vector that the box cuts
        const int c1 = e0 + V - 1 < L.nk - 1 ? e0 + V - 1 : L.nk - 1;
        for (int K = e0 > 0 ? e0 : 0; K <= c1; K++)
          if (((I + J + K + c) & 1) == 0) x[a + K] = mg_rb_pt<Z>(x, b, L, MgArr{W}, I, J, K, omg);
      }
    }
  }
}

// bc = the children's residual tree under the arrays, every level: mg_restrict_k<false, .>'s work (the shared mg_restrict_pt) in a frame of
// its own.  Through mg_restrict_k's frame the compiler forms the eight children's addresses one by one: 586 instructions for 479, and
// the launch measured 3 % (FP32) and 30 % (FP64) slower at 512^3 (profiles/r29/mg_one_cycle_rate.txt); the weights addressed through
// MgArrG with the level's own geometry, in this frame, give the shorter form
__global__ void __launch_bounds__(256) mgc_restrict_k(REAL* __restrict__ bc, const REAL* __restrict__ x, const REAL* __restrict__ b, MgLev F, MgLev C, MgcW W) {
  const int K = blockIdx.x * 64 + threadIdx.x, I = blockIdx.y * 4 + threadIdx.y, J = blockIdx.z;
  if (K >= C.nk || I >= C.ni) return;
  bc[mg_at(C, I, J, K)] = mg_restrict_pt(x, b, F, MgArrG{W, F}, I, J, K);
}

// ---- the build: level C's weights from level F's ("Coarsening").  The coarse face (f; s, t) of one direction sums the fine
// faces (f'; 2s + sb, 2t + tb) that exist, the faster-running tangential direction t paired first: (w00 + w01) + (w10 + w11).
// at(sb, tb): the fine element
template <class A>
__device__ __forceinline__ REAL mgc_face_sum(const REAL* __restrict__ W, bool hs, bool ht, A at) {
  REAL a = W[at(0, 0)];
  if (ht) a = a + W[at(0, 1)];
  if (hs) {
    REAL c = W[at(1, 0)];
    if (ht) c = c + W[at(1, 1)];
    a = a + c;
  }
  return a;
}
// the fine normal index of coarse face I: -1 is the box's - face, else the last fine point of the aggregate
__device__ __forceinline__ int mgc_fine_face(int I, int nf) { return I < 0 ? -1 : (2 * I + 1 < nf - 1 ? 2 * I + 1 : nf - 1); }

// thread (a, b, c) of [0, ni] x [0, nj] x [0, nk] is the coarse index (a - 1, b - 1, c - 1): it writes X where J, K >= 0, Y where I, K >= 0, Z where
// I, J >= 0.  A box face whose bit of C.nm is set carries no link: a zero, the fine faces are not read.  bad: += the weights written that
// are not finite and positive (such a zero is not one of them)
__global__ void __launch_bounds__(256) mgc_coarsen_k(REAL* __restrict__ XC, REAL* __restrict__ YC, REAL* __restrict__ ZC, const REAL* __restrict__ XF,
                                                     const REAL* __restrict__ YF, const REAL* __restrict__ ZF, MgLev F, MgLev C, unsigned* bad) {
  const int K = (int)(blockIdx.x * 64 + threadIdx.x) - 1, I = (int)(blockIdx.y * 4 + threadIdx.y) - 1, J = (int)blockIdx.z - 1;
  if (K >= C.nk || I >= C.ni) return;
  const bool hi = 2 * I + 1 < F.ni, hj = 2 * J + 1 < F.nj, hk = 2 * K + 1 < F.nk;
  const long long q = mg_at(C, I, J, K);
  unsigned nbad = 0u;
  if (J >= 0 && K >= 0) {
    const bool cut = (I < 0 && (C.nm & 1)) || (I == C.ni - 1 && (C.nm & 2));
    const int f = mgc_fine_face(I, F.ni);
    const REAL w = cut ? (REAL)0 : mgc_face_sum(XF, hj, hk, [&](int sb, int tb) { return mg_at(F, f, 2 * J + sb, 2 * K + tb); });
    XC[q] = w;
    nbad += !cut && !coef_ok(w);
  }
  if (I >= 0 && K >= 0) {
    const bool cut = (J < 0 && (C.nm & 4)) || (J == C.nj - 1 && (C.nm & 8));
    const int f = mgc_fine_face(J, F.nj);
    const REAL w = cut ? (REAL)0 : mgc_face_sum(YF, hi, hk, [&](int sb, int tb) { return mg_at(F, 2 * I + sb, f, 2 * K + tb); });
    YC[q] = w;
    nbad += !cut && !coef_ok(w);
  }
  if (I >= 0 && J >= 0) {
    const bool cut = (K < 0 && (C.nm & 16)) || (K == C.nk - 1 && (C.nm & 32));
    const int f = mgc_fine_face(K, F.nk);
    const REAL w = cut ? (REAL)0 : mgc_face_sum(ZF, hj, hi, [&](int sb, int tb) { return mg_at(F, 2 * I + tb, 2 * J + sb, f); });
    ZC[q] = w;
    nbad += !cut && !coef_ok(w);
  }
  if (nbad) atomicAdd(bad, nbad);
}

// D of every point of the level from its stored weights; bad (nullptr: level 0, whose faces coef_prep_k has checked): += the D that are not
// finite and positive
__global__ void __launch_bounds__(256) mgc_diag_k(REAL* __restrict__ D, const REAL* __restrict__ X, const REAL* __restrict__ Y, const REAL* __restrict__ Z,
                                                  MgLev L, unsigned* bad) {
  const int K = blockIdx.x * 64 + threadIdx.x, I = blockIdx.y * 4 + threadIdx.y, J = blockIdx.z;
  if (K >= L.nk || I >= L.ni) return;
  const long long q = mg_at(L, I, J, K), ti = L.nkp, tj = (long long)L.nkp * L.nip;
  const REAL d = ((X[q] + X[q - ti]) + (Y[q] + Y[q - tj])) + (Z[q] + Z[q - 1]);
  D[q] = d;
  if (bad && !coef_ok(d)) atomicAdd(bad, 1u);
}
