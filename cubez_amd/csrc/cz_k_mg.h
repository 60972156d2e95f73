// cz_k_mg.h -- part of cz_kernels.hip (ONE translation unit per precision; this file is included inside its anonymous
// namespace and is not a stand-alone header): the level kernels of the multigrid V-cycle preconditioner of PCG.
//
// Aggregation multigrid with the exact Galerkin operator: level l+1 has ceil(n/2) points per direction, coarse point I covers the
// level-0 points [I 2^l, min((I+1) 2^l, n)), so its extent in fine points is E(I) = min(2^l, n - I 2^l).  The level-l operator (the
// correction is zero outside the box) is
//   A_l u = Wx u(i+1) + Wx u(i-1) + Wy u(j+1) + Wy u(j-1) + Wz u(k+1) + Wz u(k-1) - D u,  Wx = Ey Ez, Wy = Ex Ez, Wz = Ex Ey, D = 2 (Wx+Wy+Wz)
// summed in that order (c1 .. c6 of the reference).  The weights are small integers computed from (I, J, K, l, n0): exact in either
// precision, no coefficient arrays.  At level 0 they are 1 and 6: the fine operator itself, whose sweep w * 1 = w gives the bits of jacobi_.
// Every kernel is pointwise-independent and contains no reduction: the cycle is deterministic, bit for bit.
// With face coefficients inside the hierarchy (cz_k_mgc.h) the weights are arrays instead; the cycle below is stated once
// for both, over a weights policy.
//
// Geometry of one level's array (MgLev): padded extents and the padded 0-based index of the first inner point.  The global arrays use the
// S3D layout with guide g; the tail kernel's LDS arrays the same description with one zero shell (nip = ni + 2, first point at 1).
constexpr int MG_TAIL_MAXLEV = 8;   // levels of the tail at most (its LDS holds far fewer)
constexpr int MG_TAIL_THREADS = 1024;
constexpr int MG_GUIDE = 2;         // the guide of the hierarchy's arrays (S3D arrays)

struct MgLev {
  int nip, nkp;        // padded rows per plane, elements per row
  int i0, j0, k0;      // padded 0-based index of the first inner point
  int ni, nj, nk;      // points of the level per direction
  int l;               // level
  int n0i, n0j, n0k;   // level-0 points per direction (the extents E)
  int nm;              // zero-flux (Neumann) physical faces of the box, bit f = face X-, X+, Y-, Y+, Z-, Z+; level 0: always 0
                       // (the LDS levels of the tail also carry bits 6 .. 8: the level wraps direction X, Y, Z -- mg_tail_wrap)
};

// global index of a level array's local point (0, 0, 0): zero on a single domain, the brick's first owned point of the level in the
// distributed cycle (the weights depend on the global index, addresses on the local one)
struct MgG {
  int i, j, k;
};

__device__ __forceinline__ long long mg_at(const MgLev& L, int I, int J, int K) {
  return (long long)(L.k0 + K) + (long long)(L.i0 + I) * L.nkp + (long long)(L.j0 + J) * L.nkp * L.nip;
}
__device__ __forceinline__ int mg_ext(int I, int l, int n0) {
  const int s = 1 << l, e = n0 - (I << l);
  return e < s ? e : s;
}

struct MgW {
  REAL wx, wy, wz, d;
};
// the links of global point I in one direction that exist: 2, less the one across a Neumann face (nm: bit 0 the - face, bit 1 the + face) at
// the level's first / last point -- there the Galerkin operator has no link, the correction being zero outside the box either way
__device__ __forceinline__ int mg_links(int I, int l, int n0, int nm) {
  return 2 - ((nm & 1) && I == 0 ? 1 : 0) - ((nm & 2) && ((I + 1) << l) >= n0 ? 1 : 0);
}
// (I, J, K): the GLOBAL index.  NM: the level has Neumann faces (L.nm != 0), D = Wx cx + Wy cy + Wz cz; else 2 (Wx + Wy + Wz), which is the
// same integer for a mask of zero.  A template parameter, chosen by the launcher from L.nm, as DIST is: the instantiations without a mask are
// the text and the code from before there was one (the one-workgroup tail measured 2-3 us slower with the test inside, profiles/r16/neumann.txt)
template <bool NM>
__device__ __forceinline__ MgW mg_weights(const MgLev& L, int I, int J, int K) {
  const int ex = mg_ext(I, L.l, L.n0i), ey = mg_ext(J, L.l, L.n0j), ez = mg_ext(K, L.l, L.n0k);
  const int wx = ey * ez, wy = ex * ez, wz = ex * ey;
  const int d = NM ? wx * mg_links(I, L.l, L.n0i, L.nm) + wy * mg_links(J, L.l, L.n0j, L.nm >> 2) + wz * mg_links(K, L.l, L.n0k, L.nm >> 4)
                   : 2 * (wx + wy + wz);
  return MgW{(REAL)wx, (REAL)wy, (REAL)wz, (REAL)d};
}

// ---- the weights of a level: a policy W.  W.at(L, I, J, K) is the point's weights (L: the geometry of the array u that is read, (I, J, K)
// the local index); what it returns gives ss<ZERO>(u, L, p), the six weighted neighbours of element p = mg_at(L, I, J, K) summed left to
// right in the reference's c1 .. c6 order, and d(), the diagonal.  W.from(o) is the policy for an array whose local point (0, 0, 0) is the
// global point o (a kernel argument carries none; the arrays have the array's own index).  Everything below that touches the operator takes
// a policy and is stated once; a new level operator supplies a policy.

// the integers of mg_weights at the global index
template <bool NM>
struct MgConst {
  MgG o;
  struct At {
    MgW w;
    // ZERO: u is identically zero (literal zeros, the same arithmetic)
    template <bool ZERO>
    __device__ __forceinline__ REAL ss(const REAL* u, const MgLev& L, long long p) const {
      const long long si = L.nkp, sj = (long long)L.nkp * L.nip;
      const REAL z = (REAL)0;
      const REAL ip = ZERO ? z : u[p + si], im = ZERO ? z : u[p - si], jp = ZERO ? z : u[p + sj], jm = ZERO ? z : u[p - sj];
      const REAL kp = ZERO ? z : u[p + 1], km = ZERO ? z : u[p - 1];
      return w.wx * ip + w.wx * im + w.wy * jp + w.wy * jm + w.wz * kp + w.wz * km;
    }
    __device__ __forceinline__ REAL d() const { return w.d; }
  };
  __device__ __forceinline__ At at(const MgLev& L, int I, int J, int K) const { return At{mg_weights<NM>(L, I + o.i, J + o.j, K + o.k)}; }
  __device__ __forceinline__ MgConst from(MgG g) const { return MgConst{g}; }
};

// face-weight arrays X, Y, Z and a diagonal D (cz_k_mgc.h): X(I, J, K) is the link between points I and I + 1
struct MgcW {
  const REAL *x, *y, *z, *d;
};
// the weights at element q of arrays with row stride ti and plane stride tj.  ZERO: u is identically zero -- every product is a weight
// (finite, not negative) times a literal zero, and the sum is +0: nothing is read
struct MgArrAt {
  const MgcW& w;
  long long q, ti, tj;
  template <bool ZERO>
  __device__ __forceinline__ REAL ss(const REAL* u, const MgLev& L, long long p) const {
    if (ZERO) return (REAL)0;
    const long long si = L.nkp, sj = (long long)L.nkp * L.nip;
    return w.x[q] * u[p + si] + w.x[q - ti] * u[p - si] + w.y[q] * u[p + sj] + w.y[q - tj] * u[p - sj] + w.z[q] * u[p + 1] + w.z[q - 1] * u[p - 1];
  }
  __device__ __forceinline__ REAL d() const { return w.d[q]; }
};
// weight arrays with the geometry of the array read (the level kernels)
struct MgArr {
  MgcW w;
  __device__ __forceinline__ MgArrAt at(const MgLev& L, int I, int J, int K) const {
    return MgArrAt{w, mg_at(L, I, J, K), L.nkp, (long long)L.nkp * L.nip};
  }
  __device__ __forceinline__ const MgArr& from(MgG) const { return *this; }
};
// weight arrays of geometry G while u lives elsewhere (the tail: u in LDS, the weights in their global arrays)
struct MgArrG {
  const MgcW& w;
  const MgLev& G;
  __device__ __forceinline__ MgArrAt at(const MgLev&, int I, int J, int K) const {
    return MgArrAt{w, mg_at(G, I, J, K), G.nkp, (long long)G.nkp * G.nip};
  }
};

// one relaxed Jacobi sweep at a point (cz_solver.f90:334-351 with the level's weights): pn = pp + ((ss - bb)/D - pp) omg, IEEE division
// (ZPP: the point's own value is a literal zero although its neighbours are read -- the second colour of a red-black iteration from zero)
template <bool ZERO, bool ZPP = ZERO, class W>
__device__ __forceinline__ REAL mg_sweep_pt(const REAL* u, const REAL* b, const MgLev& L, const W& wt, int I, int J, int K, REAL omg) {
  const auto w = wt.at(L, I, J, K);
  const long long p = mg_at(L, I, J, K);
  const REAL pp = ZPP ? (REAL)0 : u[p];
  const REAL ss = w.template ss<ZERO>(u, L, p);
  const REAL dp = ((ss - b[p]) / w.d() - pp) * omg;
  return pp + dp;
}

// residual at a point, written like blas_calc_rk_ (cz_blas.f90:705-711): b - (ss - D x)
template <class W>
__device__ __forceinline__ REAL mg_res_pt(const REAL* x, const REAL* b, const MgLev& L, const W& wt, int I, int J, int K) {
  const auto w = wt.at(L, I, J, K);
  const long long p = mg_at(L, I, J, K);
  const REAL ss = w.template ss<false>(x, L, p);
  return b[p] - (ss - w.d() * x[p]);
}

// b_{l+1}(I, J, K) = the residual summed over the <= 8 children (j, i, k; k innermost) as the tree
// ((r000 + r001) + (r010 + r011)) + ((r100 + r101) + (r110 + r111)); absent children drop out of it.  res(ib, jb, kb) is child
// (2I + ib, 2J + jb, 2K + kb)'s residual; hi, hj, hk: the second child exists in that direction
template <class R>
__device__ __forceinline__ REAL mg_tree(bool hi, bool hj, bool hk, R res) {
  REAL t[2];
#pragma unroll
  for (int jb = 0; jb < 2; jb++) {
    if (jb && !hj) break;
    REAL s[2];
#pragma unroll
    for (int ib = 0; ib < 2; ib++) {
      if (ib && !hi) break;
      s[ib] = res(ib, jb, 0);
      if (hk) s[ib] = s[ib] + res(ib, jb, 1);
    }
    t[jb] = hi ? s[0] + s[1] : s[0];
  }
  return hj ? t[0] + t[1] : t[0];
}

template <class W>
__device__ __forceinline__ REAL mg_restrict_pt(const REAL* x, const REAL* b, const MgLev& F, const W& wt, int I, int J, int K) {
  const int i0 = 2 * I, j0 = 2 * J, k0 = 2 * K;
  const bool hi = i0 + 1 < F.ni, hj = j0 + 1 < F.nj, hk = k0 + 1 < F.nk;
  return mg_tree(hi, hj, hk, [&](int ib, int jb, int kb) { return mg_res_pt(x, b, F, wt, i0 + ib, j0 + jb, k0 + kb); });
}

// u = x + R(alpha xc(parent)), alpha = R(1.8): one rounding per operation (no contraction: the build has -ffp-contract=off)
// (fo, co: global index of the local point (0, 0, 0) of the fine and the coarse array; the parent may then be a ghost cell)
__device__ __forceinline__ REAL mg_prolong_pt(const REAL* x, const REAL* xc, const MgLev& F, const MgLev& Cl, int I, int J, int K, MgG fo = MgG{0, 0, 0},
                                              MgG co = MgG{0, 0, 0}) {
  const REAL alpha = (REAL)1.8;
  const REAL c = alpha * xc[mg_at(Cl, ((I + fo.i) >> 1) - co.i, ((J + fo.j) >> 1) - co.j, ((K + fo.k) >> 1) - co.k)];
  return x[mg_at(F, I, J, K)] + c;
}

// ---- the level kernels: one thread per point of the level written; block (64, 4), grid (k, i, j).  One array of a level is what a domain
// owns of it ("Decomposed runs"): MgLev's ni, nj, nk are the OWNED points in the fine brick's inner-range convention, l and
// n0 the global ones; o is the global index of the first owned point, gn the level's global points per direction.  Ghost cells hold the
// neighbours' values after an exchange.  A single domain owns every point: o = 0, gn = (ni, nj, nk).
struct MgDLev {
  MgLev L;
  MgG o;
  int gni, gnj, gnk;
};

// (W: the weights as a kernel argument, MgConst<NM> or MgArr; wt.from(o) the policy of the array at hand)
template <bool ZERO, class W>
__global__ void __launch_bounds__(256) mg_smooth_k(const REAL* __restrict__ u, REAL* __restrict__ w, const REAL* __restrict__ b, MgDLev D, REAL omg, W wt) {
  const int K = blockIdx.x * 64 + threadIdx.x, I = blockIdx.y * 4 + threadIdx.y, J = blockIdx.z;
  if (K >= D.L.nk || I >= D.L.ni) return;
  w[mg_at(D.L, I, J, K)] = mg_sweep_pt<ZERO>(u, b, D.L, wt.from(D.o), I, J, K, omg);
}

// ---- pcg ... mgrb: one colour sweep of a level >= 1, IN PLACE.  The colour of a point is (I + J + K) & 1; the points of
// one colour read only points of the other one (and their own value), so the sweep is deterministic in place.  One thread per UPDATED point:
// thread kk of row (I, J) owns K = 2 kk + ((I + J + c) & 1).  A workgroup is (64, 4) with one row per wave, so that offset is wave-uniform and
// the colour c a launch argument: no lane selects operands.  Z: 0 = from the iterate; 1 = the first colour of an iteration from zero (x is not
// read); 2 = its second colour (reads the freshly written colour, its own value is a literal zero).  The same bits as a sweep from a cleared x.
template <int Z, class W>
__device__ __forceinline__ REAL mg_rb_pt(const REAL* x, const REAL* b, const MgLev& L, const W& wt, int I, int J, int K, REAL omg) {
  return mg_sweep_pt<Z == 1, Z != 0>(x, b, L, wt, I, J, K, omg);
}

// (the array is the whole level: global index = local index)
template <int Z, class W>
__global__ void __launch_bounds__(256) mg_rb_k(REAL* x, const REAL* __restrict__ b, MgLev L, REAL omg, int c, W wt) {
  const int I = blockIdx.y * 4 + threadIdx.y, J = blockIdx.z;
  const int K = 2 * (blockIdx.x * 64 + threadIdx.x) + ((I + J + c) & 1);
  if (K >= L.nk || I >= L.ni) return;
  x[mg_at(L, I, J, K)] = mg_rb_pt<Z>(x, b, L, wt.from(MgG{0, 0, 0}), I, J, K, omg);
}

// bc (owned coarse points) = the children's residual tree; owned children computed here, children on the + neighbours (the brick's
// ghost layer) read from rt after its exchange.  C.L may be a dense block (no shell): the gathered level's send buffer.  DIST = false: the
// domain owns the whole level (offsets 0, global extents = the local ones, rt not read) -- the same text with those constants folded in,
// kept as an instantiation of its own because the FP32 launch measured 1-2 % slower without it (profiles/r11/mg_one_cycle.txt)
template <bool DIST, class W>
__global__ void __launch_bounds__(256) mg_restrict_k(REAL* __restrict__ bc, const REAL* __restrict__ x, const REAL* __restrict__ b, const REAL* __restrict__ rt,
                                                     MgDLev F, MgDLev C, W wt) {
  const int K = blockIdx.x * 64 + threadIdx.x, I = blockIdx.y * 4 + threadIdx.y, J = blockIdx.z;
  if (K >= C.L.nk || I >= C.L.ni) return;
  const MgG fo = DIST ? F.o : MgG{0, 0, 0}, co = DIST ? C.o : MgG{0, 0, 0};
  const int gni = DIST ? F.gni : F.L.ni, gnj = DIST ? F.gnj : F.L.nj, gnk = DIST ? F.gnk : F.L.nk;
  // global first child, then local (fine array) index
  const int gi = 2 * (I + co.i), gj = 2 * (J + co.j), gk = 2 * (K + co.k);
  const bool hi = gi + 1 < gni, hj = gj + 1 < gnj, hk = gk + 1 < gnk;
  const int li = gi - fo.i, lj = gj - fo.j, lk = gk - fo.k;
  const auto wf = wt.from(fo);  // (the children's residual takes the FINE level's weights)
  bc[mg_at(C.L, I, J, K)] = mg_tree(hi, hj, hk, [&](int ib, int jb, int kb) {
    const int ci = li + ib, cj = lj + jb, ck = lk + kb;
    if (!DIST || (ci < F.L.ni && cj < F.L.nj && ck < F.L.nk)) return mg_res_pt(x, b, F.L, wf, ci, cj, ck);
    return rt[mg_at(F.L, ci, cj, ck)];
  });
}

// u = x + R(alpha xc(parent)) on the owned points (u may be x: every point reads its own x and its parent only); the parent is a ghost cell
// of xc where it lies on a - neighbour, or a point of the gathered global array (C.o = 0)
__global__ void __launch_bounds__(256) mg_prolong_k(REAL* u, const REAL* x, const REAL* __restrict__ xc, MgDLev F, MgDLev C) {
  const int K = blockIdx.x * 64 + threadIdx.x, I = blockIdx.y * 4 + threadIdx.y, J = blockIdx.z;
  if (K >= F.L.nk || I >= F.L.ni) return;
  u[mg_at(F.L, I, J, K)] = mg_prolong_pt(x, xc, F.L, C.L, I, J, K, F.o, C.o);
}

// rt = the residual of the first owned layer on the rank-internal - faces (d = 0, 1, 2: I, J, K face; edges and corners belong to the
// face of the lowest d among the internal ones).  grid: (64-wide blocks along the face's faster free direction, the slower one)
template <bool NM>
__global__ void __launch_bounds__(64) mgd_resface_k(REAL* __restrict__ rt, const REAL* __restrict__ x, const REAL* __restrict__ b, MgDLev D, int d,
                                                    int mi, int mj) {
  const int a = blockIdx.x * 64 + threadIdx.x, c = blockIdx.y;
  int I, J, K;
  if (d == 0) I = 0, K = a, J = c;
  else if (d == 1) J = 0, K = a, I = c;
  else K = 0, I = a, J = c;
  if (I >= D.L.ni || J >= D.L.nj || K >= D.L.nk) return;
  if ((d >= 1 && mi && I == 0) || (d == 2 && mj && J == 0)) return;  // written by the I (J) face launch
  rt[mg_at(D.L, I, J, K)] = mg_res_pt(x, b, D.L, MgConst<NM>{D.o}, I, J, K);
}

// one rank's dense block (ni, nj, nk; K fastest) into the gathered global array at global offset o: an exact copy
__global__ void __launch_bounds__(256) mgd_unpack_k(REAL* __restrict__ X, const REAL* __restrict__ blk, MgLev G, MgG o, int ni, int nj, int nk) {
  const long long n = (long long)ni * nj * nk;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < n; q += (long long)gridDim.x * 256) {
    const int K = (int)(q % nk);
    const long long r = q / nk;
    const int I = (int)(r % ni), J = (int)(r / ni);
    X[mg_at(G, I + o.i, J + o.j, K + o.k)] = blk[q];
  }
}

// ---- the tail: x = V_t(b) from level t down to the coarsest and back, in ONE workgroup with every level's b, x and t in LDS
struct MgTail {
  int nlev;                // levels t .. t + nlev - 1 (the last is the coarsest)
  MgLev gl;                // the global arrays of level t (b read, x written)
  MgLev s[MG_TAIL_MAXLEV];      // the LDS arrays of every tail level (one zero shell)
  int off[MG_TAIL_MAXLEV];      // REAL offset of level m's b in LDS; x and t follow at + len[m], + 2 len[m] (mgrb: no t)
  int len[MG_TAIL_MAXLEV];      // REALs per LDS array of level m
  int total;               // REALs of LDS in all
  REAL omg;
};
// the weights of the tail's levels (WT of mg_tail_k): lev(m) is level m's policy.  The integers need nothing from the host; the arrays of
// tail level m are read from their global arrays (geometry g[m]): read-only, a few KiB, resident in L2
template <bool NM>
struct MgConstTail {
  __device__ __forceinline__ MgConst<NM> lev(int) const { return MgConst<NM>{MgG{0, 0, 0}}; }
};
struct MgcTail {
  MgLev g[MG_TAIL_MAXLEV];
  MgcW w[MG_TAIL_MAXLEV];
  __device__ __forceinline__ MgArrG lev(int m) const { return MgArrG{w[m], g[m]}; }
};

// every point of level L, by the workgroup
template <class F>
__device__ __forceinline__ void mg_each(const MgLev& L, F f) {
  const int n = L.ni * L.nj * L.nk;
  for (int q = threadIdx.x; q < n; q += blockDim.x) {
    const int K = q % L.nk, r = q / L.nk, I = r % L.ni, J = r / L.ni;
    f(I, J, K);
  }
}

// the points of colour c of level L, by the workgroup (K = 2 kk + the row's offset)
template <class F>
__device__ __forceinline__ void mg_each_colour(const MgLev& L, int c, F f) {
  const int nh = (L.nk + 1) / 2, n = L.ni * L.nj * nh;
  for (int q = threadIdx.x; q < n; q += blockDim.x) {
    const int kk = q % nh, r = q / nh, I = r % L.ni, J = r / L.ni;
    const int K = 2 * kk + ((I + J + c) & 1);
    if (K < L.nk) f(I, J, K);
  }
}

// Periodic directions in the tail: the wrap of array a of level L into its own one-cell shell, a(-1) = a(n - 1) and a(n) = a(0)
// in every direction whose wrap bit (6 + d of L.nm) is set, over the level's points of the other two directions (edges stay zero: no kernel
// reads them).  A workgroup loop over the seam faces; the caller's threads are in step before it, and it ends with them in step
__device__ __forceinline__ void mg_tail_wrap(const MgLev& L, REAL* a) {
  const int per = L.nm >> 6;
  if (!per) return;
  if (per & 1)
    for (int q = threadIdx.x; q < L.nj * L.nk; q += blockDim.x) {
      const int K = q % L.nk, J = q / L.nk;
      a[mg_at(L, -1, J, K)] = a[mg_at(L, L.ni - 1, J, K)];
      a[mg_at(L, L.ni, J, K)] = a[mg_at(L, 0, J, K)];
    }
  if (per & 2)
    for (int q = threadIdx.x; q < L.ni * L.nk; q += blockDim.x) {
      const int K = q % L.nk, I = q / L.nk;
      a[mg_at(L, I, -1, K)] = a[mg_at(L, I, L.nj - 1, K)];
      a[mg_at(L, I, L.nj, K)] = a[mg_at(L, I, 0, K)];
    }
  if (per & 4)
    for (int q = threadIdx.x; q < L.ni * L.nj; q += blockDim.x) {
      const int I = q % L.ni, J = q / L.ni;
      a[mg_at(L, I, J, -1)] = a[mg_at(L, I, J, L.nk - 1)];
      a[mg_at(L, I, J, L.nk)] = a[mg_at(L, I, J, 0)];
    }
  __syncthreads();
}

// x <- two smoothing iterations of the level (zero: from zero); RB: red-black in place, backward (colours 1, 0) where post; else relaxed
// Jacobi through t.  Ends with the workgroup in step.  PER: a wrap follows every sweep and colour sweep (x is wrapped on return; on an odd
// periodic extent the seam points share a colour and the shell holds the value from before the sweep -- from zero that is the cleared LDS)
template <bool RB, bool PER, class W>
__device__ __forceinline__ void mg_tail_pair(const MgLev& L, const W& wt, const REAL* b, REAL* x, REAL* t, bool zero, bool post, REAL omg) {
  if (RB) {
    const int c0 = post ? 1 : 0;
    if (zero) {
      mg_each_colour(L, c0, [&](int I, int J, int K) { x[mg_at(L, I, J, K)] = mg_rb_pt<1>(x, b, L, wt, I, J, K, omg); });
      __syncthreads();
      if (PER) mg_tail_wrap(L, x);
      mg_each_colour(L, 1 - c0, [&](int I, int J, int K) { x[mg_at(L, I, J, K)] = mg_rb_pt<2>(x, b, L, wt, I, J, K, omg); });
      __syncthreads();
      if (PER) mg_tail_wrap(L, x);
    }
    for (int s = zero ? 2 : 0; s < 4; s++) {
      mg_each_colour(L, (c0 + s) & 1, [&](int I, int J, int K) { x[mg_at(L, I, J, K)] = mg_rb_pt<0>(x, b, L, wt, I, J, K, omg); });
      __syncthreads();
      if (PER) mg_tail_wrap(L, x);
    }
    return;
  }
  if (zero) mg_each(L, [&](int I, int J, int K) { t[mg_at(L, I, J, K)] = mg_sweep_pt<true>(t, b, L, wt, I, J, K, omg); });
  else mg_each(L, [&](int I, int J, int K) { t[mg_at(L, I, J, K)] = mg_sweep_pt<false>(x, b, L, wt, I, J, K, omg); });
  __syncthreads();
  if (PER) mg_tail_wrap(L, t);
  mg_each(L, [&](int I, int J, int K) { x[mg_at(L, I, J, K)] = mg_sweep_pt<false>(t, b, L, wt, I, J, K, omg); });
  __syncthreads();
  if (PER) mg_tail_wrap(L, x);
}

// RB: the cycle of pcg ... mgrb (its levels keep b and x only: T.len[m] apart, no t).  PER: some level of the tail wraps (T.s[m].nm bits 6 .. 8;
// without it, the code from before there were periodic directions).  WT: the levels' weights, MgConstTail<NM> or MgcTail
template <bool RB, bool PER, class WT>
__global__ void __launch_bounds__(MG_TAIL_THREADS) mg_tail_k(REAL* __restrict__ xg, const REAL* __restrict__ bg, MgTail T, WT W) {
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
  // down: pre-smoothing pair from zero, residual restricted into the next level's b
  for (int m = 0; m + 1 < T.nlev; m++) {
    const MgLev& L = T.s[m];
    REAL *b = lds + T.off[m], *x = b + T.len[m], *t = x + T.len[m];
    mg_tail_pair<RB, PER>(L, W.lev(m), b, x, t, true, false, omg);
    const MgLev& Cl = T.s[m + 1];
    REAL* bc = lds + T.off[m + 1];
    mg_each(Cl, [&](int I, int J, int K) { bc[mg_at(Cl, I, J, K)] = mg_restrict_pt(x, b, L, W.lev(m), I, J, K); });
    __syncthreads();
  }
  {  // the coarsest level: four pairs from zero, the last two post (mg_walk's order)
    const int m = T.nlev - 1;
    REAL *b = lds + T.off[m], *x = b + T.len[m], *t = x + T.len[m];
    for (int s = 0; s < 4; s++) mg_tail_pair<RB, PER>(T.s[m], W.lev(m), b, x, t, s == 0, s >= 2, omg);
  }
  // up: x += R(alpha x_c(parent)) in place, post-smoothing pair
  for (int m = T.nlev - 2; m >= 0; m--) {
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
    mg_tail_pair<RB, PER>(L, W.lev(m), b, x, t, false, true, omg);
  }
  {
    const REAL* x0 = lds + T.off[0] + T.len[0];
    mg_each(T.s[0], [&](int I, int J, int K) { xg[mg_at(T.gl, I, J, K)] = x0[mg_at(T.s[0], I, J, K)]; });
  }
}
