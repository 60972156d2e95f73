// cz_k_pair.h -- part of cz_kernels.hip (ONE translation unit per precision; this file is included inside its anonymous
// namespace after cz_k_pass.h and is not a stand-alone header): pair_shell_k, the shell slabs of a decomposed brick's two-stage pass, and
// shell_fold_k.  The pass itself is jacobi2p_k (cz_k_pair2.h); geometry, per-point update and finalisation are the frame's (cz_k_pass.h).
// ------------------------------------------------------------------------------------------------------------
// The same two-stage update on thin boxes: the cells a decomposed brick owes its neighbours (two layers behind every
// rank-internal face).  The driver runs this first, starts the halo exchange on a second stream and lets jacobi2p_k
// work on the interior meanwhile.  A slab two cells thick has no plane to march along, so it is cut into
// small 3-D tiles instead: a workgroup stages the tile of u with two halo layers in LDS, applies stage 1 to the tile
// plus one layer (LDS), then stage 2 to the tile.  Tile shapes follow the slab's orientation (long in k wherever k is
// not the thin axis, so that global accesses stay coalesced).  Same scalar operation sequence as relax_vec<1> => the
// fields are bit-identical to an unsplit jacobi2p_k launch.
// ------------------------------------------------------------------------------------------------------------
struct ShellBox {
  int i0, j0, k0, ni, nj, nk;  // padded 0-based start, extent
  int kind;                    // tile shape: 0 = 64x4x2 (k,i,j; J slabs), 1 = 64x2x4 (I slabs), 2 = 2x16x16 (K slabs), 3 = 32x4x4
  int ntk, nti, ntj;           // tiles per axis
};
struct ShellTab {
  int n;
  ShellBox b[6];
  int ii0a, ii1a, jj0a, jj1a, kk0a, kk1a;  // stage-1 box of the brick (inner box grown across rank-internal faces)
  int nkp, nip, njp;
  int par;
};

// all tiles of one box that this workgroup takes; the tile shape is a compile-time constant (index arithmetic without divisions)
// MAF = 1: the weights of every point from the 1-D coordinate arrays (cz_maf.f90:193-225; padded index == index into xc / yc / zc for g = 2),
// through relax_vec_maf<1> like the pass itself.
template <int RB, int TK, int TI, int TJ, int MAF>
__device__ __forceinline__ void shell_tiles(const REAL* __restrict__ U, const REAL* __restrict__ B, REAL* __restrict__ W, const Coef& c,
                                            const ShellTab& s, const ShellBox& d, REAL* lu, double& acc1, double& acc2, const MafArgs& ma) {
  // metric terms of padded index x of a 1-D grid: XG-like first difference and XGG-like second difference
  auto met1 = [](const REAL* __restrict__ xc, int x) { return (REAL)0.5 * (xc[x + 1] - xc[x - 1]); };
  auto met2 = [](const REAL* __restrict__ xc, int x) { return xc[x + 1] - (REAL)2.0 * xc[x] + xc[x - 1]; };
  constexpr int UK = TK + 4, UI = TI + 4, UJ = TJ + 4;  // u tile: two halo layers
  constexpr int VK = TK + 2, VI = TI + 2, VJ = TJ + 2;  // v tile: one halo layer
  REAL* lv = lu + UK * UI * UJ;
  const int t = threadIdx.x;
  const int si = s.nkp, sj = s.nkp * s.nip;  // a halo'd tile spans < 2^31 elements: 32-bit offsets from the tile origin
  const int ntiles = d.ntk * d.nti * d.ntj;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int tkx = tile % d.ntk, tr = tile / d.ntk;
    const int K0 = d.k0 + tkx * TK, I0 = d.i0 + (tr % d.nti) * TI, J0 = d.j0 + (tr / d.nti) * TJ;
    const int ck = min(TK, d.k0 + d.nk - K0), ci = min(TI, d.i0 + d.ni - I0), cj = min(TJ, d.j0 + d.nj - J0);  // clipped core
    const size_t org = (size_t)(K0 - 2) + (size_t)(I0 - 2) * s.nkp + (size_t)(J0 - 2) * s.nkp * s.nip;  // first cell of the u tile
    const REAL* __restrict__ Ut = U + org;
    const REAL* __restrict__ Bt = B + org;
    REAL* __restrict__ Wt = W + org;
    // ---- every global read of the tile is issued before the first use (one memory latency per tile, not one per element)
    constexpr int NU = (UK * UI * UJ + 255) / 256, NV = (VK * VI * VJ + 255) / 256, NO = (TK * TI * TJ + 255) / 256;
    REAL ru[NU], rb1[NV], rb2[NO];
#pragma unroll
    for (int n = 0; n < NU; n++) {
      const int e = t + n * 256;
      const int k = e % UK, r = e / UK, i = r % UI, j = r / UI;
      const int gk = K0 - 2 + k, gi = I0 - 2 + i, gj = J0 - 2 + j;
      ru[n] = (e < UK * UI * UJ && gk < s.nkp && gi < s.nip && gj < s.njp) ? Ut[k + i * si + j * sj] : (REAL)0;
    }
    unsigned in1 = 0;  // bit n: stage 1 applies to this thread's n-th point of the v tile
#pragma unroll
    for (int n = 0; n < NV; n++) {
      const int e = t + n * 256;
      const int k = e % VK, r = e / VK, i = r % VI, j = r / VI;
      const int gk = K0 - 1 + k, gi = I0 - 1 + i, gj = J0 - 1 + j;
      const bool inside = e < VK * VI * VJ && gi >= s.ii0a && gi <= s.ii1a && gj >= s.jj0a && gj <= s.jj1a && gk >= s.kk0a && gk <= s.kk1a &&
                          !(RB && ((gk + gi + gj + s.par) & 1));
      rb1[n] = inside ? Bt[(k + 1) + (i + 1) * si + (j + 1) * sj] : (REAL)0;
      if (inside) in1 |= 1u << n;
    }
#pragma unroll
    for (int n = 0; n < NO; n++) {
      const int e = t + n * 256;
      const int k = e % TK, r = e / TK, i = r % TI, j = r / TI;
      const bool live = e < TK * TI * TJ && k < ck && i < ci && j < cj;
      rb2[n] = live ? Bt[(k + 2) + (i + 2) * si + (j + 2) * sj] : (REAL)0;
    }
#pragma unroll
    for (int n = 0; n < NU; n++)
      if (t + n * 256 < UK * UI * UJ) lu[t + n * 256] = ru[n];
    __syncthreads();
    // ---- stage 1 on the core plus one layer
#pragma unroll
    for (int n = 0; n < NV; n++) {
      const int e = t + n * 256;
      if (e >= VK * VI * VJ) continue;
      const int k = e % VK, r = e / VK, i = r % VI, j = r / VI;
      const int cu = (k + 1) + UK * ((i + 1) + UI * (j + 1));
      REAL v = lu[cu];
      if (in1 & (1u << n)) {
        const bool core = k >= 1 && k <= ck && i >= 1 && i <= ci && j >= 1 && j <= cj;
        Vec<1> pc, im, ip, pm, pn, bb;
        pc.v[0] = v, im.v[0] = lu[cu - UK], ip.v[0] = lu[cu + UK], pm.v[0] = lu[cu - UK * UI], pn.v[0] = lu[cu + UK * UI];
        bb.v[0] = rb1[n];
        if (MAF) {
          const int gk = K0 - 1 + k, gi = I0 - 1 + i, gj = J0 - 1 + j;
          Vec<1> zt, ztt;
          zt.v[0] = met1(ma.zc, gk), ztt.v[0] = met2(ma.zc, gk);
          v = relax_vec_maf<1>(pc, im, ip, pm, pn, lu[cu - 1], lu[cu + 1], bb, met1(ma.xc, gi), met2(ma.xc, gi), met1(ma.yc, gj), met2(ma.yc, gj), zt, ztt,
                               c.omg, 1u, core ? 1u : 0u, acc1).v[0];
        } else {
          v = relax_vec<1>(pc, im, ip, pm, pn, lu[cu - 1], lu[cu + 1], bb, c, PlainDiv{c.dd}, 1u, core ? 1u : 0u, acc1).v[0];
        }
      }
      lv[e] = v;
    }
    __syncthreads();
    // ---- stage 2 on the core
#pragma unroll
    for (int n = 0; n < NO; n++) {
      const int e = t + n * 256;
      const int k = e % TK, r = e / TK, i = r % TI, j = r / TI;
      if (e >= TK * TI * TJ || k >= ck || i >= ci || j >= cj) continue;
      const int gk = K0 + k, gi = I0 + i, gj = J0 + j;
      const int cv = (k + 1) + VK * ((i + 1) + VI * (j + 1));
      REAL o = lv[cv];
      if (!(RB && !((gk + gi + gj + s.par) & 1))) {  // RB: colour 0 passes through stage 2
        Vec<1> pc, im, ip, pm, pn, bb;
        pc.v[0] = o, im.v[0] = lv[cv - VK], ip.v[0] = lv[cv + VK], pm.v[0] = lv[cv - VK * VI], pn.v[0] = lv[cv + VK * VI];
        bb.v[0] = rb2[n];
        if (MAF) {
          Vec<1> zt, ztt;
          zt.v[0] = met1(ma.zc, gk), ztt.v[0] = met2(ma.zc, gk);
          o = relax_vec_maf<1>(pc, im, ip, pm, pn, lv[cv - 1], lv[cv + 1], bb, met1(ma.xc, gi), met2(ma.xc, gi), met1(ma.yc, gj), met2(ma.yc, gj), zt, ztt,
                               c.omg, 1u, 1u, acc2).v[0];
        } else {
          o = relax_vec<1>(pc, im, ip, pm, pn, lv[cv - 1], lv[cv + 1], bb, c, PlainDiv{c.dd}, 1u, 1u, acc2).v[0];
        }
      }
      Wt[(k + 2) + (i + 2) * si + (j + 2) * sj] = o;
    }
    __syncthreads();
  }
}

template <int RB, int MAF = 0>
__global__ void __launch_bounds__(256)
pair_shell_k(const REAL* __restrict__ U, const REAL* __restrict__ B, REAL* __restrict__ W, Coef c, ShellTab s, double* partials,
             const int* __restrict__ skip, MafArgs ma) {
  if (skip != nullptr && *skip != 0) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ double wsum[8];
  const int t = threadIdx.x;
  const ShellBox d = s.b[blockIdx.y];
  REAL* lu = reinterpret_cast<REAL*>(smem);
  double acc1 = 0.0, acc2 = 0.0;
  switch (d.kind) {  // uniform per workgroup
    case 0: shell_tiles<RB, 64, 4, 2, MAF>(U, B, W, c, s, d, lu, acc1, acc2, ma); break;
    case 1: shell_tiles<RB, 64, 2, 4, MAF>(U, B, W, c, s, d, lu, acc1, acc2, ma); break;
    case 2: shell_tiles<RB, 2, 16, 16, MAF>(U, B, W, c, s, d, lu, acc1, acc2, ma); break;
    default: shell_tiles<RB, 32, 4, 4, MAF>(U, B, W, c, s, d, lu, acc1, acc2, ma); break;
  }
  // residuals: one pair of sums per workgroup; the interior launch that follows on the stream adds them to its own
  const int nblk = gridDim.x * gridDim.y;
  const int lb = blockIdx.y * gridDim.x + blockIdx.x;
  const double s1 = block_sum<256>(acc1, wsum);
  __syncthreads();
  const double s2 = block_sum<256>(acc2, wsum);
  if (t == 0) {
    partials[lb] = s1;
    partials[nblk + lb] = s2;
  }
}

// The sums of a pair_shell_k launch added to the sums of the interior launch of the same pass (the driver runs the two concurrently on
// two streams and folds afterwards): res[0] += first-stage sums, res[1] += second-stage sums (single: both into res[0]).  One
// workgroup, fixed order.
__global__ void __launch_bounds__(256)
shell_fold_k(const double* __restrict__ partials, int n, double* __restrict__ res, int single, const int* __restrict__ skip) {
  if (skip != nullptr && *skip != 0) return;
  __shared__ double wsum[8];
  double x1 = 0.0, x2 = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) x1 += partials[i], x2 += partials[n + i];
  const double s1 = block_sum<256>(x1, wsum);
  __syncthreads();
  const double s2 = block_sum<256>(x2, wsum);
  if (threadIdx.x == 0) {
    if (single) {
      res[0] += s1 + s2;
    } else {
      res[0] += s1;
      res[1] += s2;
    }
  }
}
