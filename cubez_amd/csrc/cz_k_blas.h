// cz_k_blas.h -- part of cz_kernels.hip (ONE translation unit per precision; this file is included inside its anonymous
// namespace and is not a stand-alone header): reductions, convergence bookkeeping, BLAS-like element-wise kernels, dots, pivot, shell copy, boundary faces.
// sum of n partials in a fixed order -> dst[0] (= or +=).  One workgroup: deterministic.
__global__ void __launch_bounds__(1024)
reduce_partials_k(const double* __restrict__ partials, int n, double* __restrict__ dst, int accumulate,
                  const int* __restrict__ skip) {
  if (skip != nullptr && *skip != 0) return;
  __shared__ double wsum[16];
  double x = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) x += partials[i];
  const double s = block_sum<1024>(x, wsum);
  if (threadIdx.x == 0) dst[0] = accumulate ? dst[0] + s : s;
}

// cz_Poisson.cpp:67-77 on the device.  snap (optional) receives the flag as it stands after this test: the lagged loops of
// CZ::JACOBI / CZ::RBSOR hand that copy -- which no later test can change -- to the pass two passes further on, so that every
// workgroup of a pass sees the same value (the flag itself may be rewritten by the next test while the pass is running).
__global__ void check_k(const double* res_dev, double res_normal, double eps, int itr, double* hist, int* flag,
                        int* conv_itr, int* snap) {
  if (*flag == 0) {
    double r = res_dev[0];
    r *= res_normal;
    r = sqrt(r);
    hist[itr] = r;
    if (r < eps) {
      *flag = 1;
      *conv_itr = itr;
    }
  }
  if (snap) *snap = *flag;
}

// the same bookkeeping for a fused pair (iterations itr, itr+1) whose two sums were all-reduced first
__global__ void check2_k(const double* res_dev, double res_normal, double eps, int itr, double* hist, int* flag,
                         int* conv_itr, int* snap) {
  if (*flag == 0) {
    double r = sqrt(res_dev[0] * res_normal);
    hist[itr] = r;
    if (r < eps) {
      *flag = 1;
      *conv_itr = itr;
    } else {
      r = sqrt(res_dev[1] * res_normal);
      hist[itr + 1] = r;
      if (r < eps) {
        *flag = 1;
        *conv_itr = itr + 1;
      }
    }
  }
  if (snap) *snap = *flag;
}

// ------------------------------------------------------------------------------------------------------------
// element-wise kernels on the inner box (cz_blas.f90): one vector per thread, blockIdx.y = plane
// ------------------------------------------------------------------------------------------------------------
enum { OP_TRIAD = 0, OP_BICG1 = 1, OP_BICG2 = 2, OP_COPY = 3 };

struct EGeom {
  int R;
  long long PSV;
  int kk0, kk1, jj0;
  long long F0, Fend;
  // rows as R vectors from a vector boundary each; in memory a row is nkp elements and a plane PSE elements (Geom2, cz_k_pair.h)
  int nkp = 0;
  long long PSE = 0;
  // scalars of the update kept on the device (BiCGSTAB's alpha / omega, made by bicg_scal_k from the dot products of the launch before):
  // where set they replace the by-value arguments a / b of ewise_k and triad_dots_k -- the host need not read the dot products back first
  const REAL* pa = nullptr;
  const REAL* pb = nullptr;
  // PCG's breakdown guard (cg_update_k): where set and |*pg| < FLT_MIN (rho, cg_scal_k's sc[3]) the launch stores nothing and its sums are 0
  const REAL* pg = nullptr;
};
// element offset of vector f of the row view inside a plane in memory
template <int V>
__device__ __forceinline__ long long egeom_eo(const EGeom& g, long long f) {
  const long long r = f / g.R;
  return r * g.nkp + (f - r * g.R) * V;
}

// The streaming row frame of the kernels below: a thread owns vector f = erow_f of the row view in every plane it visits; erow_mask = the
// components of that vector with k inside the box; egeom_eo = its element offset inside a plane.
__device__ __forceinline__ long long erow_f(const EGeom& g) { return g.F0 + (long long)blockIdx.x * 256 + threadIdx.x; }
template <int V>
__device__ __forceinline__ unsigned erow_mask(const EGeom& g, long long f) {
  const int kv = (int)(f % g.R);
  unsigned mk = 0;
#pragma unroll
  for (int cc = 0; cc < V; cc++) {
    const int kk = kv * V + cc;
    if (kk >= g.kk0 && kk <= g.kk1) mk |= 1u << cc;
  }
  return mk;
}
// body(pe, mk) at the thread's vector of the planes blockIdx.y, blockIdx.y + gridDim.y, ... below nplanes; pe = its element offset in the
// array.  Not entered by a thread beyond the update range, nor -- unless EMPTY_TOO -- by one without a component inside the box.
template <int V, bool EMPTY_TOO = false, class BODY>
__device__ __forceinline__ void erow_planes(const EGeom& g, int nplanes, BODY body) {
  const long long f = erow_f(g);
  if (f >= g.Fend) return;
  const unsigned mk = erow_mask<V>(g, f);
  if (!EMPTY_TOO && mk == 0) return;
  const long long eo = egeom_eo<V>(g, f);
  for (int pl = blockIdx.y; pl < nplanes; pl += gridDim.y) body((long long)(g.jj0 + pl) * g.PSE + eo, mk);
}

template <int V, int OP>
__global__ void __launch_bounds__(256)
ewise_k(REAL* Z, const REAL* X, const REAL* Y, REAL a, REAL b, EGeom g) {
  const long long f = erow_f(g);
  if (f >= g.Fend) return;
  if (g.pa) a = *g.pa;
  if (g.pb) b = *g.pb;
  const long long pe = (long long)(g.jj0 + blockIdx.y) * g.PSE + egeom_eo<V>(g, f);
  const unsigned mk = erow_mask<V>(g, f);
  if (mk == 0) return;
  Vec<V> x = ldve<V>(X, pe), y, z, o;
  if (OP != OP_COPY) y = ldve<V>(Y, pe);
  if (OP == OP_BICG1 || OP == OP_BICG2) z = ldve<V>(Z, pe);
#pragma unroll
  for (int cc = 0; cc < V; cc++) {
    if (OP == OP_TRIAD) o.v[cc] = a * x.v[cc] + y.v[cc];                              // cz_blas.f90:297
    if (OP == OP_BICG1) o.v[cc] = x.v[cc] + a * (z.v[cc] - b * y.v[cc]);              // :490  p = r + beta*(p - omg*q)
    if (OP == OP_BICG2) o.v[cc] = a * x.v[cc] + b * y.v[cc] + z.v[cc];                // :554
    if (OP == OP_COPY) o.v[cc] = x.v[cc];
  }
  stve_masked<V>(Z, pe, o, mk);
}

// BiCGSTAB's scalars on the device (cz_Poisson.cpp:427, 464), from the dot products the launch before left in `dots` (all-reduced in a
// decomposed run), with the host's own operations -- the double sums rounded to REAL, then one REAL division: the same bits as the host path.
//   STEP 1: alpha = rho / (q . r0)              sc[0] = alpha, sc[2] = -alpha      (the indices: enum ScBicg, cz_internal.h)
//   STEP 2: omega = (t . s) / (t . t)           sc[1] = omega, sc[3] = -omega
template <int STEP>
__global__ void bicg_scal_k(const double* __restrict__ dots, REAL rho, REAL* __restrict__ sc) {
  if (STEP == 1) {
    const REAL q_r0 = (REAL)dots[0];
    const REAL alpha = rho / q_r0;
    sc[0] = alpha, sc[2] = -alpha;
  } else {
    const REAL ts = (REAL)dots[0], tt = (REAL)dots[1];
    const REAL omega = ts / tt;
    sc[1] = omega, sc[3] = -omega;
  }
}

// search_pivot (cz_blas.f90:947-1039): pvt = 1 / max(|row entries|) on the inner box
template <int V>
__global__ void __launch_bounds__(256)
pivot_k(REAL* PVT, EGeom g, MafArgs ma, int nkp, int nip) {
  const long long f = g.F0 + (long long)blockIdx.x * 256 + threadIdx.x;
  if (f >= g.Fend) return;
  const int jj = g.jj0 + blockIdx.y;
  const long long row = f / g.R;
  const int kv = (int)(f - row * g.R);
  const long long pe = (long long)jj * g.PSE + row * g.nkp + (long long)kv * V;
  const int ii = (int)row;
  const REAL xm = ma.xc[ii - 1], x0 = ma.xc[ii], xp = ma.xc[ii + 1];
  const REAL ym = ma.yc[jj - 1], y0 = ma.yc[jj], yp = ma.yc[jj + 1];
  const REAL XG = (REAL)0.5 * (xp - xm), XGG = xp - (REAL)2.0 * x0 + xm;
  const REAL YE = (REAL)0.5 * (yp - ym), YEE = yp - (REAL)2.0 * y0 + ym;
#pragma unroll
  for (int cc = 0; cc < V; cc++) {
    const int kk = kv * V + cc;
    if (kk < g.kk0 || kk > g.kk1) continue;
    const REAL zm = ma.zc[kk - 1], z0 = ma.zc[kk], zp = ma.zc[kk + 1];
    const MafW w = maf_weights(XG, XGG, YE, YEE, (REAL)0.5 * (zp - zm), zp - (REAL)2.0 * z0 + zm);
    REAL ss = fmax(fabs(w.w1), fabs(w.w2));  // max(s1..s7), left to right (cz_blas.f90:1024)
    ss = fmax(ss, fabs(w.w3));
    ss = fmax(ss, fabs(w.w4));
    ss = fmax(ss, fabs(w.w5));
    ss = fmax(ss, fabs(w.w6));
    ss = fmax(ss, fabs(w.dd));
    PVT[pe + cc] = (REAL)1.0 / ss;
  }
  (void)nkp;
  (void)nip;
}

// dot products (cz_blas.f90:361-362, :426): per-point product in REAL, accumulated in double.  A workgroup strides over
// the planes (few thousand workgroups in all); the last one to finish sums the partials in fixed order into dst[0]
// (sums_finish, cz_k_sums.h: no second launch).
template <int V, int TWO>
__global__ void __launch_bounds__(256)
dot_k(const REAL* X, const REAL* Y, EGeom g, int nplanes, double* partials, double* dst, unsigned* counter) {
  __shared__ double wsum[5];  // cz_k_sums.h
  double acc[1] = {0.0};
  // (a thread whose vector lies outside the box in k walks its planes all the same and adds nothing: one division for mask and offset.
  // Skipping it as the kernels below do costs dot_k<4, 1> 155 instructions and nine scalar registers, profiles/r32/sums_kernel_text.txt)
  erow_planes<V, true>(g, nplanes, [&](long long pe, unsigned mk) {
    const Vec<V> x = ldve<V>(X, pe);
    Vec<V> y = x;
    if (TWO) y = ldve<V>(Y, pe);
#pragma unroll
    for (int cc = 0; cc < V; cc++) {
      const REAL tt = x.v[cc] * y.v[cc];
      if (mk & (1u << cc)) acc[0] += (double)tt;
    }
  });
  sums_finish<256>(acc, partials, counter, wsum, [&](const double (&tot)[1]) { dst[0] = tot[0]; });
}

// z = a*x + y on the inner box (blas_triad, cz_blas.f90:297) with the two dot products that follow it in BiCGSTAB folded
// in: dst[0] = sum z*z (cz_Poisson.cpp:481), dst[1] = sum z*w (the next iteration's rho, :376).  Same structure as dot_k.
template <int V>
__global__ void __launch_bounds__(256)
triad_dots_k(REAL* Z, const REAL* X, const REAL* Y, const REAL* W, REAL a, EGeom g, int nplanes, double* partials, double* dst,
             unsigned* counter) {
  __shared__ double wsum[5];  // cz_k_sums.h
  if (g.pa) a = *g.pa;
  double acc[2] = {0.0, 0.0};
  erow_planes<V>(g, nplanes, [&](long long pe, unsigned mk) {
    const Vec<V> x = ldve<V>(X, pe), y = ldve<V>(Y, pe), w = ldve<V>(W, pe);
    Vec<V> o;
#pragma unroll
    for (int cc = 0; cc < V; cc++) {
      o.v[cc] = a * x.v[cc] + y.v[cc];
      const REAL zz = o.v[cc] * o.v[cc];
      const REAL zw = o.v[cc] * w.v[cc];
      if (mk & (1u << cc)) {
        acc[0] += (double)zz;
        acc[1] += (double)zw;
      }
    }
    stve_masked<V>(Z, pe, o, mk);
  });
  sums_finish<256>(acc, partials, counter, wsum, [&](const double (&tot)[2]) { dst[0] = tot[0], dst[1] = tot[1]; });
}

// PCG's update (beyond the reference): x = alpha*p + x, r = (-alpha)*q + r (blas_triad twice) and dst[0] = sum r*r, one pass over the four
// arrays.  alpha and -alpha come from the device (g.pa / g.pb, made by cg_scal_k); same structure and launch shape as triad_dots_k.
// CLOSED (the closed box): r = ((-alpha)*q + r) - m, m = g.pa[4] the mean of the residual as the update before left it
// (mean_scal_k), and dst[1] = sum r of the values written, through a second row of partials; false: the code from before there was a closed box.
// g.pg (CZ::PCG sets it to rho): a rho under the breakdown threshold makes alpha = rho / p.q meaningless (0 / 0 from an exact start), and the
// host learns rho only after this launch -- so the launch itself leaves x and r alone there, every thread alike, and returns sums of 0.
template <int V, bool CLOSED>
__global__ void __launch_bounds__(256)
cg_update_k(REAL* X, REAL* Rr, const REAL* Pd, const REAL* Q, EGeom g, int nplanes, double* partials, double* dst, unsigned* counter) {
  __shared__ double wsum[5];  // cz_k_sums.h
  constexpr int N = CLOSED ? 2 : 1;  // sum r*r; CLOSED: and sum r
  const REAL a = *g.pa, na = *g.pb;
  const REAL m = CLOSED ? g.pa[4] : (REAL)0;
  const bool live = !(g.pg && fabs(*g.pg) < (REAL)FLT_MIN);  // (the host's test, CZ::PCG)
  double acc[N] = {};
  if (live) {
    erow_planes<V>(g, nplanes, [&](long long pe, unsigned mk) {
      const Vec<V> p = ldve<V>(Pd, pe), q = ldve<V>(Q, pe), x = ldve<V>(X, pe), r = ldve<V>(Rr, pe);
      Vec<V> xo, ro;
#pragma unroll
      for (int cc = 0; cc < V; cc++) {
        xo.v[cc] = a * p.v[cc] + x.v[cc];
        ro.v[cc] = na * q.v[cc] + r.v[cc];
        if (CLOSED) ro.v[cc] = ro.v[cc] - m;
        const REAL rr = ro.v[cc] * ro.v[cc];
        if (mk & (1u << cc)) {
          acc[0] += (double)rr;
          if (CLOSED) acc[N - 1] += (double)ro.v[cc];
        }
      }
      stve_masked<V>(X, pe, xo, mk);
      stve_masked<V>(Rr, pe, ro, mk);
    });
  }
  sums_finish<256>(acc, partials, counter, wsum, [&](const double (&tot)[N]) {
    dst[0] = tot[0];
    if (CLOSED) dst[1] = tot[N - 1];
  });
}

// The closed box: a <- a - *m over the inner box (SHIFT; false: a is only read, m is not), with dst[0] = sum a' and
// dst[1] = sum a'^2 of the values a holds afterwards -- the squares as REAL products widened, like every dot here.  It projects the
// right-hand side, the initial residual and the answer of a closed-box solve.  Row frame and hand-off are those of triad_dots_k.
template <int V, bool SHIFT>
__global__ void __launch_bounds__(256)
shift_sums_k(REAL* A, const REAL* mp, EGeom g, int nplanes, double* partials, double* dst, unsigned* counter) {
  __shared__ double wsum[5];  // cz_k_sums.h
  const REAL m = SHIFT ? *mp : (REAL)0;
  double acc[2] = {0.0, 0.0};
  erow_planes<V>(g, nplanes, [&](long long pe, unsigned mk) {
    Vec<V> o = ldve<V>(A, pe);
#pragma unroll
    for (int cc = 0; cc < V; cc++) {
      if (SHIFT) o.v[cc] = o.v[cc] - m;
      const REAL aa = o.v[cc] * o.v[cc];
      if (mk & (1u << cc)) {
        acc[0] += (double)o.v[cc];
        acc[1] += (double)aa;
      }
    }
    if (SHIFT) stve_masked<V>(A, pe, o, mk);
  });
  sums_finish<256>(acc, partials, counter, wsum, [&](const double (&tot)[2]) { dst[0] = tot[0], dst[1] = tot[1]; });
}

// the mean of a closed-box projection on the device: double division, then the one rounding to REAL; keep (optional) receives a copy that
// no later launch overwrites (cz_closed_mean reads it after the solve)
__global__ void mean_scal_k(const double* __restrict__ sum, double npts, REAL* __restrict__ m, REAL* __restrict__ keep) {
  const REAL v = (REAL)(sum[0] / npts);
  *m = v;
  if (keep) *keep = v;
}

// PCG's scalars on the device, with the host's operations (REAL division of REAL-rounded double sums), like bicg_scal_k.
// (enum ScCg, cz_internal.h) sc[0] = alpha, sc[1] = -alpha, sc[2] = beta, sc[3] = rho (the REAL of the current iteration; the previous one until STEP 0 replaces it).
//   STEP 0: rho = (REAL)dot[0];  beta = rho / rho_old unless `first`;  rho_old <- rho
//   STEP 1: alpha = rho / (REAL)dot[0]   (dot = p . A p)
template <int STEP>
__global__ void cg_scal_k(const double* __restrict__ dot, int first, REAL* __restrict__ sc) {
  if (STEP == 0) {
    const REAL rho = (REAL)dot[0];
    if (!first) sc[2] = rho / sc[3];
    sc[3] = rho;
  } else {
    const REAL pq = (REAL)dot[0];
    const REAL alpha = sc[3] / pq;
    sc[0] = alpha, sc[1] = -alpha;
  }
}

// ------------------------------------------------------------------------------------------------------------
// bc_k (cz_solver.f90:22-191): the sin*sin table is evaluated on the HOST with the host libm -- the same sinf/sin
// the reference's Fortran calls -- so the Dirichlet data are bit-identical to the reference's; the kernels only
// scatter it.  Three launches in the reference's order: K faces, then I faces, then J faces (edges end up 0).
// ------------------------------------------------------------------------------------------------------------
__global__ void bc_kface_k(REAL* p, const REAL* __restrict__ tab, int ix, int jx, int kface, int g, int nkp, int nip) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x + 1, j = blockIdx.y + 1;
  if (i > ix) return;
  p[(size_t)(kface + g - 1) + (size_t)(i + g - 1) * nkp + (size_t)(j + g - 1) * nkp * nip] = tab[(size_t)(j - 1) * ix + (i - 1)];
}
__global__ void bc_iface_k(REAL* p, int jx, int kx, int iface, int g, int nkp, int nip) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x + 1, j = blockIdx.y + 1;
  if (k > kx) return;
  p[(size_t)(k + g - 1) + (size_t)(iface + g - 1) * nkp + (size_t)(j + g - 1) * nkp * nip] = (REAL)0;
}
__global__ void bc_jface_k(REAL* p, int ix, int kx, int jface, int g, int nkp, int nip) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x + 1, i = blockIdx.y + 1;
  if (k > kx) return;
  p[(size_t)(k + g - 1) + (size_t)(i + g - 1) * nkp + (size_t)(jface + g - 1) * nkp * nip] = (REAL)0;
}

// Zero-flux (Neumann) faces: the face layer of a physical face is the mirror of the first inner layer, p(1, j, k) = p(2, j, k)
// on a - side and p(size, j, k) = p(size-1, j, k) on a + side, j and k over the inner box (edges and corners are neither read by a 7-point
// kernel nor written here).  One launch fills every face listed: blockIdx.y picks the face (0 .. 5: X-, X+, Y-, Y+, Z-, Z+), one wave per row.
// X and Y faces copy k-rows with the lanes along k; a Z face has one element per k-row, so its lanes run along i.  Padded 0-based indices.
struct MirrorFaces {
  int nkp, nip;
  int ii0, ii1, jj0, jj1, kk0, kk1;  // the inner box (inclusive)
  int n, face[6];                    // the faces to fill
};
__global__ void __launch_bounds__(256) mirror_faces_k(REAL* p, MirrorFaces m) {
  const int f = m.face[blockIdx.y], d = f >> 1, plus = f & 1;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const long long si = m.nkp, sj = (long long)m.nkp * m.nip;
  if (d == 0) {  // row = j; from layer ii0 (ii1) to ii0 - 1 (ii1 + 1)
    const int jj = m.jj0 + row, is = plus ? m.ii1 : m.ii0;
    if (jj > m.jj1) return;
    const long long src = jj * sj + is * si, dst = src + (plus ? si : -si);
    for (int kk = m.kk0 + lane; kk <= m.kk1; kk += 64) p[dst + kk] = p[src + kk];
  } else if (d == 1) {  // row = i
    const int ii = m.ii0 + row, js = plus ? m.jj1 : m.jj0;
    if (ii > m.ii1) return;
    const long long src = js * sj + ii * si, dst = src + (plus ? sj : -sj);
    for (int kk = m.kk0 + lane; kk <= m.kk1; kk += 64) p[dst + kk] = p[src + kk];
  } else {  // row = j, lanes along i
    const int jj = m.jj0 + row, ks = plus ? m.kk1 : m.kk0;
    if (jj > m.jj1) return;
    const long long src = jj * sj + ks, dst = src + (plus ? 1 : -1);
    for (int ii = m.ii0 + lane; ii <= m.ii1; ii += 64) p[dst + ii * si] = p[src + ii * si];
  }
}

// Periodic directions: mirror_faces_k's shape with the source layer as a parameter.  Entry q fills layer dst[q] of direction
// dir[q] from layer src[q], both over the inner box of the other two directions: a mirror takes the first inner layer next to the face, a wrap
// the last inner layer for the - face (p(1) = p(size-1)) and the first one for the + face (p(size) = p(2)).  Every source is an inner layer and
// every destination a face layer, so the entries of one launch do not read what another writes.  A Z entry touches one element per k-row; a Z
// wrap is ONE entry whose thread serves both faces of its row (dst2 / src2 >= 0), so that a short row's two accesses share its cache lines.
struct FillFaces {
  int nkp, nip;
  int ii0, ii1, jj0, jj1, kk0, kk1;  // the inner box (inclusive)
  int n, dir[6], dst[6], src[6];     // the entries: padded 0-based layer indices
  int dst2, src2;                    // the second face of a Z wrap entry (-1: none)
};
__global__ void __launch_bounds__(256) fill_faces_k(REAL* p, FillFaces m) {
  const int q = blockIdx.y, d = m.dir[q];
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const long long si = m.nkp, sj = (long long)m.nkp * m.nip;
  if (d == 0) {  // row = j
    const int jj = m.jj0 + row;
    if (jj > m.jj1) return;
    const long long src = jj * sj + m.src[q] * si, dst = jj * sj + m.dst[q] * si;
    for (int kk = m.kk0 + lane; kk <= m.kk1; kk += 64) p[dst + kk] = p[src + kk];
  } else if (d == 1) {  // row = i
    const int ii = m.ii0 + row;
    if (ii > m.ii1) return;
    const long long src = m.src[q] * sj + ii * si, dst = m.dst[q] * sj + ii * si;
    for (int kk = m.kk0 + lane; kk <= m.kk1; kk += 64) p[dst + kk] = p[src + kk];
  } else {  // row = j, lanes along i
    const int jj = m.jj0 + row;
    if (jj > m.jj1) return;
    const long long at = jj * sj;
    for (int ii = m.ii0 + lane; ii <= m.ii1; ii += 64) {
      REAL* const r = p + at + ii * si;
      const REAL a = r[m.src[q]];
      if (m.dst2 >= 0) {
        const REAL b = r[m.src2];
        r[m.dst2] = b;
      }
      r[m.dst[q]] = a;
    }
  }
}

// copy every element OUTSIDE the inner box (guide cells, Dirichlet faces) from src to dst: one wave per k-row.
// Used to give the ping-pong partner buffer of a Jacobi solve the same boundary data as the solution array.
__global__ void __launch_bounds__(256)
copy_shell_k(REAL* __restrict__ dst, const REAL* __restrict__ src, int nkp, int nip, int njp, int kk0, int kk1, int ii0, int ii1,
             int jj0, int jj1) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (long long)nip * njp) return;
  const int lane = threadIdx.x & 63;
  const int jj = (int)(row / nip), ii = (int)(row - (long long)jj * nip);
  const bool inner_row = ii >= ii0 && ii <= ii1 && jj >= jj0 && jj <= jj1;
  const size_t base = (size_t)row * nkp;
  if (inner_row) {
    for (int kk = lane; kk < kk0; kk += 64) dst[base + kk] = src[base + kk];
    for (int kk = kk1 + 1 + lane; kk < nkp; kk += 64) dst[base + kk] = src[base + kk];
  } else {
    for (int kk = lane; kk < nkp; kk += 64) dst[base + kk] = src[base + kk];
  }
}
