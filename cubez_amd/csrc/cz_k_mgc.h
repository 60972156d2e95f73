// cz_k_mgc.h -- part of cz_kernels.hip (ONE translation unit per precision; this file is included inside its anonymous
// namespace and is not a stand-alone header): the V-cycle of pcg ... mg | mgrb with the face coefficients of cz_set_face_coef inside the
// hierarchy (cz_set_coef_mg).
//
// The levels, the walk, the restriction tree and the prolongation are those of cz_k_mg.h; only the weights change.  Level l keeps three
// face-weight arrays X, Y, Z and a diagonal D with the geometry of the level's own arrays (MgLev): X(I, J, K) is the link between points I
// and I + 1, I = -1 .. n - 1; -1 and n - 1 are the box's two faces, and the -1 entry lives in the array's shell.  Level 0's X, Y, Z are the
// handle's own padded coefficient arrays (face 0 of a periodic direction already holds the copy of face n - 2, coef_prep_k).  Level l + 1's
// weights are the sums of the fine face weights that cross the aggregate's face (mgc_coarsen_k), the exact Galerkin product for
// piecewise-constant aggregation; with unit coefficients they are the integers of mg_weights, and every kernel below then gives the bits
// of its twin in cz_k_mg.h.  A face that carries no link -- a Neumann face of the box, the seam of a periodic direction on a level of one
// point -- is stored as a zero weight from level 1 on, so these levels need neither mask nor mirror.
//   ss = X(I) u(I+1) + X(I-1) u(I-1) + Y(J) u(J+1) + Y(J-1) u(J-1) + Z(K) u(K+1) + Z(K-1) u(K-1), left to right
//   sweep pn = pp + ((ss - bb) / D - pp) omg (IEEE division), residual b - (ss - D x), D = ((X(I) + X(I-1)) + (Y(J) + Y(J-1))) + (Z(K) + Z(K-1))
// every operation rounded once in REAL.  No kernel here reduces anything: the cycle is deterministic, bit for bit.
struct MgcW {
  const REAL *x, *y, *z, *d;  // the level's face weights and diagonal
};

// u lives in an array of geometry L at element p (a global array, or the tail's LDS copy), the weights in global arrays of geometry G at
// element q.  ZERO: u is identically zero -- every product is a weight (finite, not negative) times a literal zero, and the sum is +0
template <bool ZERO>
__device__ __forceinline__ REAL mgc_ss(const REAL* u, const MgLev& L, long long p, const MgcW& w, const MgLev& G, long long q) {
  if (ZERO) return (REAL)0;
  const long long si = L.nkp, sj = (long long)L.nkp * L.nip;
  const long long ti = G.nkp, tj = (long long)G.nkp * G.nip;
  return w.x[q] * u[p + si] + w.x[q - ti] * u[p - si] + w.y[q] * u[p + sj] + w.y[q - tj] * u[p - sj] + w.z[q] * u[p + 1] + w.z[q - 1] * u[p - 1];
}

// mg_sweep_pt with the level's weight arrays (ZPP: the point's own value is a literal zero although its neighbours are read)
template <bool ZERO, bool ZPP = ZERO>
__device__ __forceinline__ REAL mgc_sweep_pt(const REAL* u, const REAL* b, const MgLev& L, const MgcW& w, const MgLev& G, int I, int J, int K, REAL omg) {
  const long long p = mg_at(L, I, J, K), q = mg_at(G, I, J, K);
  const REAL pp = ZPP ? (REAL)0 : u[p];
  const REAL ss = mgc_ss<ZERO>(u, L, p, w, G, q);
  const REAL dp = ((ss - b[p]) / w.d[q] - pp) * omg;
  return pp + dp;
}

// mg_res_pt with the level's weight arrays
__device__ __forceinline__ REAL mgc_res_pt(const REAL* x, const REAL* b, const MgLev& L, const MgcW& w, const MgLev& G, int I, int J, int K) {
  const long long p = mg_at(L, I, J, K), q = mg_at(G, I, J, K);
  const REAL ss = mgc_ss<false>(x, L, p, w, G, q);
  return b[p] - (ss - w.d[q] * x[p]);
}

__device__ __forceinline__ REAL mgc_restrict_pt(const REAL* x, const REAL* b, const MgLev& F, const MgcW& w, const MgLev& G, int I, int J, int K) {
  const int i0 = 2 * I, j0 = 2 * J, k0 = 2 * K;
  const bool hi = i0 + 1 < F.ni, hj = j0 + 1 < F.nj, hk = k0 + 1 < F.nk;
  return mg_tree(hi, hj, hk, [&](int ib, int jb, int kb) { return mgc_res_pt(x, b, F, w, G, i0 + ib, j0 + jb, k0 + kb); });
}

// Z as mg_rb_pt: 0 from the iterate, 1 the first colour of an iteration from zero, 2 its second colour
template <int Z>
__device__ __forceinline__ REAL mgc_rb_pt(const REAL* x, const REAL* b, const MgLev& L, const MgcW& w, const MgLev& G, int I, int J, int K, REAL omg) {
  return mgc_sweep_pt<Z == 1, Z != 0>(x, b, L, w, G, I, J, K, omg);
}

// ---- the level kernels: one thread per point written, block (64, 4), grid (k, i, j), as cz_k_mg.h.  Single domain: the array is the whole level
template <bool ZERO>
__global__ void __launch_bounds__(256) mgc_smooth_k(const REAL* __restrict__ u, REAL* __restrict__ w, const REAL* __restrict__ b, MgLev L, MgcW W, REAL omg) {
  const int K = blockIdx.x * 64 + threadIdx.x, I = blockIdx.y * 4 + threadIdx.y, J = blockIdx.z;
  if (K >= L.nk || I >= L.ni) return;
  w[mg_at(L, I, J, K)] = mgc_sweep_pt<ZERO>(u, b, L, W, L, I, J, K, omg);
}

// one colour sweep IN PLACE, thread kk of row (I, J) owns K = 2 kk + ((I + J + c) & 1) (mg_rb_k)
template <int Z>
__global__ void __launch_bounds__(256) mgc_rb_k(REAL* x, const REAL* __restrict__ b, MgLev L, MgcW W, REAL omg, int c) {
  const int I = blockIdx.y * 4 + threadIdx.y, J = blockIdx.z;
  const int K = 2 * (blockIdx.x * 64 + threadIdx.x) + ((I + J + c) & 1);
  if (K >= L.nk || I >= L.ni) return;
  x[mg_at(L, I, J, K)] = mgc_rb_pt<Z>(x, b, L, W, L, I, J, K, omg);
}

// bc = the children's residual tree: residual and restriction in one pass, only the coarse right-hand side is written
__global__ void __launch_bounds__(256) mgc_restrict_k(REAL* __restrict__ bc, const REAL* __restrict__ x, const REAL* __restrict__ b, MgLev F, MgLev C, MgcW W) {
  const int K = blockIdx.x * 64 + threadIdx.x, I = blockIdx.y * 4 + threadIdx.y, J = blockIdx.z;
  if (K >= C.nk || I >= C.ni) return;
  bc[mg_at(C, I, J, K)] = mgc_restrict_pt(x, b, F, W, F, I, J, K);
}

// ---- level 0, the hot path: the row form of ax_coef_k.  k across the lanes, a row cut into the 16-byte vectors of the array written, stored
// aligned; every operand loaded with REAL-aligned 16-byte loads (the rows i - 1, i + 1, j - 1, j + 1 of u and i - 1, j - 1 of X, Y are the
// rows neighbouring threads ask for at the same time: L2 / MALL); a vector that the box cuts goes cell by cell through the per-point
// functions above.  The same operations in the same order: the bits of mgc_smooth_k / mgc_rb_k.
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
        for (int K = e0 > 0 ? e0 : 0; K <= c1; K++) w[a + K] = mgc_sweep_pt<ZERO>(u, b, L, W, L, I, J, K, omg);
      }
    }
  }
}

// one colour sweep of level 0 IN PLACE: the vector is read, its cells of colour c ((I + J + K) & 1) take the update, and it is stored whole --
// the cells of the other colour, which the neighbouring threads read, are written back with the bytes they hold.  Z as mgc_rb_pt
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
          if (((I + J + K + c) & 1) == 0) x[a + K] = mgc_rb_pt<Z>(x, b, L, W, L, I, J, K, omg);
      }
    }
  }
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

// ---- the tail: mg_tail_k's structure, every level's b, x and t in LDS exactly as there (mg_tail_plan); the weights of tail level m are read
// from their global arrays (geometry g[m]): read-only, a few KiB, resident in L2
struct MgcTail {
  MgLev g[MG_TAIL_MAXLEV];
  MgcW w[MG_TAIL_MAXLEV];
};

template <bool RB, bool PER>
__device__ __forceinline__ void mgc_tail_pair(const MgLev& L, const MgcW& w, const MgLev& G, const REAL* b, REAL* x, REAL* t, bool zero, bool post, REAL omg) {
  if (RB) {
    const int c0 = post ? 1 : 0;
    if (zero) {
      mg_each_colour(L, c0, [&](int I, int J, int K) { x[mg_at(L, I, J, K)] = mgc_rb_pt<1>(x, b, L, w, G, I, J, K, omg); });
      __syncthreads();
      if (PER) mg_tail_wrap(L, x);
      mg_each_colour(L, 1 - c0, [&](int I, int J, int K) { x[mg_at(L, I, J, K)] = mgc_rb_pt<2>(x, b, L, w, G, I, J, K, omg); });
      __syncthreads();
      if (PER) mg_tail_wrap(L, x);
    }
    for (int s = zero ? 2 : 0; s < 4; s++) {
      mg_each_colour(L, (c0 + s) & 1, [&](int I, int J, int K) { x[mg_at(L, I, J, K)] = mgc_rb_pt<0>(x, b, L, w, G, I, J, K, omg); });
      __syncthreads();
      if (PER) mg_tail_wrap(L, x);
    }
    return;
  }
  if (zero) mg_each(L, [&](int I, int J, int K) { t[mg_at(L, I, J, K)] = mgc_sweep_pt<true>(t, b, L, w, G, I, J, K, omg); });
  else mg_each(L, [&](int I, int J, int K) { t[mg_at(L, I, J, K)] = mgc_sweep_pt<false>(x, b, L, w, G, I, J, K, omg); });
  __syncthreads();
  if (PER) mg_tail_wrap(L, t);
  mg_each(L, [&](int I, int J, int K) { x[mg_at(L, I, J, K)] = mgc_sweep_pt<false>(t, b, L, w, G, I, J, K, omg); });
  __syncthreads();
  if (PER) mg_tail_wrap(L, x);
}

template <bool RB, bool PER>
__global__ void __launch_bounds__(MG_TAIL_THREADS) mgc_tail_k(REAL* __restrict__ xg, const REAL* __restrict__ bg, MgTail T, MgcTail W) {
  extern __shared__ __align__(16) unsigned char mg_lds_raw[];
  REAL* const lds = reinterpret_cast<REAL*>(mg_lds_raw);
  for (int q = threadIdx.x; q < T.total; q += blockDim.x) lds[q] = (REAL)0;  // the zero shells (and a defined start)
  __syncthreads();
  {
    REAL* b0 = lds + T.off[0];
    mg_each(T.s[0], [&](int I, int J, int K) { b0[mg_at(T.s[0], I, J, K)] = bg[mg_at(T.gl, I, J, K)]; });
  }
  __syncthreads();
  const REAL omg = T.omg;
  for (int m = 0; m + 1 < T.nlev; m++) {  // down
    const MgLev& L = T.s[m];
    REAL *b = lds + T.off[m], *x = b + T.len[m], *t = x + T.len[m];
    mgc_tail_pair<RB, PER>(L, W.w[m], W.g[m], b, x, t, true, false, omg);
    const MgLev& Cl = T.s[m + 1];
    REAL* bc = lds + T.off[m + 1];
    mg_each(Cl, [&](int I, int J, int K) { bc[mg_at(Cl, I, J, K)] = mgc_restrict_pt(x, b, L, W.w[m], W.g[m], I, J, K); });
    __syncthreads();
  }
  {  // the coarsest level: four pairs from zero, the last two post
    const int m = T.nlev - 1;
    REAL *b = lds + T.off[m], *x = b + T.len[m], *t = x + T.len[m];
    for (int s = 0; s < 4; s++) mgc_tail_pair<RB, PER>(T.s[m], W.w[m], W.g[m], b, x, t, s == 0, s >= 2, omg);
  }
  for (int m = T.nlev - 2; m >= 0; m--) {  // up
    const MgLev& L = T.s[m];
    const MgLev& Cl = T.s[m + 1];
    REAL *b = lds + T.off[m], *x = b + T.len[m], *t = x + T.len[m];
    const REAL* xc = lds + T.off[m + 1] + T.len[m + 1];
    mg_each(L, [&](int I, int J, int K) {
      const long long p = mg_at(L, I, J, K);
      x[p] = mg_prolong_pt(x, xc, L, Cl, I, J, K);
    });
    __syncthreads();
    if (PER) mg_tail_wrap(L, x);
    mgc_tail_pair<RB, PER>(L, W.w[m], W.g[m], b, x, t, false, true, omg);
  }
  {
    const REAL* x0 = lds + T.off[0] + T.len[0];
    mg_each(T.s[0], [&](int I, int J, int K) { xg[mg_at(T.gl, I, J, K)] = x0[mg_at(T.s[0], I, J, K)]; });
  }
}
