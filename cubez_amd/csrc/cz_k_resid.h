// cz_k_resid.h -- part of cz_kernels.hip (ONE translation unit per precision; this file is included inside its anonymous
// namespace and is not a stand-alone header): the row forms of cz_get_residual and cz_add_field (the caller's k is its unit
// stride).  Geometry and indices are those of cz_k_field.h; the caller's side has element type T (float | double), whatever REAL is.
//
// resid_row_k   r = b - (ss - dd p) (blas_calc_rk_, cz_blas.f90:705-711: the same operations in the same order, in REAL) from P and RHS, the
//               caller's array U = (T)(r scale) and sum r^2 in one pass: no padded residual array.  A thread has two roles for run s of four
//               cells of a row:
//                 sum    cells 4 s .. 4 s + 3 -- a partition that depends on the brick alone, so that the sum has the same bits whatever the
//                        destination is (its type, its strides, none at all); squares and sums in double, block_sum, then the fixed-order sum
//                        of the workgroups' partials by the workgroup that arrives last (cz_k_sums.h);
//                 store  cells 4 s - ph .. 4 s - ph + 3, ph = the phase of the destination row against a 16-byte boundary: whole 16-byte
//                        vectors of the DESTINATION stored aligned (one of four floats, two of two doubles), the cells before the first and
//                        after the last whole vector of a row one by one.  ph = 0 (aligned rows of a multiple of the vector width -- any
//                        dense tensor whose nk is one): the two roles have the same cells and the residual is computed once; otherwise the
//                        store role computes its own four cells, from rows the sum role has just brought into the cache.
//               The k neighbours of a run come from the run's own vector and one element either side; the i and j neighbours are four more
//               vector loads per run, served by L2 / MALL for all but one of the five rows (the planes j - 1, j, j + 1 of a workgroup's
//               neighbours in the grid are in flight at the same time).  Cells outside the box (Dirichlet faces) give 0 and add nothing.
// addf_row_k    P = P + (REAL)U scale at the cells of the box: 16-byte vectors of P read, updated and stored aligned where a whole vector lies
//               inside the box, one by one elsewhere; P's other cells are not written.
template <class T, int N>
__device__ __forceinline__ void ldt(const T* base, long long elem, T (&o)[N]) {  // N elements from an offset that is only T-aligned
  constexpr int LV = (N * sizeof(T) > 16) ? (int)(16 / sizeof(T)) : N;
  typedef T nv __attribute__((ext_vector_type(LV)));
  typedef nv unv __attribute__((aligned(sizeof(T))));
#pragma unroll
  for (int q = 0; q < N / LV; q++) {
    const nv x = *reinterpret_cast<const unv*>(base + elem + q * LV);
    __builtin_memcpy(&o[q * LV], &x, sizeof(x));
  }
}

// the residual of cells c0 .. c0 + 3 of the k row whose cell 0 is element `a` of the padded arrays (any c0 >= -3: the guide cells are there)
__device__ __forceinline__ void resid4(const REAL* __restrict__ P, const REAL* __restrict__ B, long long a, int c0, const FieldGeom& g, const Coef& c,
                                       REAL (&r)[4]) {
  const long long e = a + c0;
  REAL pp[4], im[4], ip[4], pm[4], pn[4], bb[4];
  ldt<REAL, 4>(P, e, pp);
  ldt<REAL, 4>(P, e - g.nkp, im);
  ldt<REAL, 4>(P, e + g.nkp, ip);
  ldt<REAL, 4>(P, e - g.PSE, pm);
  ldt<REAL, 4>(P, e + g.PSE, pn);
  ldt<REAL, 4>(B, e, bb);
  const REAL kl = P[e - 1], kr = P[e + 4];
#pragma unroll
  for (int cc = 0; cc < 4; cc++) {
    const REAL km1 = cc == 0 ? kl : pp[cc > 0 ? cc - 1 : 0];
    const REAL kp1 = cc == 3 ? kr : pp[cc < 3 ? cc + 1 : 3];
    const REAL ss = offdiag_sum<0>(c, ip[cc], im[cc], pn[cc], pm[cc], kp1, km1);
    r[cc] = bb[cc] - (ss - c.dd * pp[cc]);
  }
}

template <class T, int DST>
__global__ __launch_bounds__(256) void resid_row_k(T* __restrict__ dst, const REAL* __restrict__ P, const REAL* __restrict__ B, const FieldGeom g,
                                                   const FieldBox bx, const Coef c, const REAL scale, const int slots, double* partials,
                                                   double* out, unsigned* counter) {
  constexpr int VT = 16 / sizeof(T);
  typedef T nvt __attribute__((ext_vector_type(VT)));
  __shared__ double wsum[5];  // cz_k_sums.h
  const int per_plane = g.ni * slots;
  double acc = 0.0;
  for (int j = blockIdx.y; j < g.nj; j += gridDim.y) {
    for (int it = blockIdx.x * 256 + threadIdx.x; it < per_plane; it += gridDim.x * 256) {
      const int i = it / slots, s = it - i * slots;
      const long long a = (long long)(j + g.g) * g.PSE + (long long)(i + g.g) * g.nkp + g.g;
      const bool in_ij = i >= bx.lo0 && i <= bx.hi0 && j >= bx.lo1 && j <= bx.hi1;
      const int k0 = 4 * s;
      REAL r[4] = {(REAL)0, (REAL)0, (REAL)0, (REAL)0};
      if (k0 < g.nk && in_ij) {
        resid4(P, B, a, k0, g, c, r);
#pragma unroll
        for (int cc = 0; cc < 4; cc++) {
          if (k0 + cc < bx.lo2 || k0 + cc > bx.hi2) r[cc] = (REAL)0;
          acc += (double)r[cc] * (double)r[cc];
        }
      }
      if (DST) {
        const long long u = (long long)i * g.s0 + (long long)j * g.s1;
        const int ph = (int)((reinterpret_cast<uintptr_t>(dst + u) / sizeof(T)) & (uintptr_t)(VT - 1));
        const int e0 = k0 - ph;
        if (e0 >= g.nk) continue;
        if (ph != 0 && in_ij) {
          resid4(P, B, a, e0, g, c, r);
#pragma unroll
          for (int cc = 0; cc < 4; cc++)
            if (e0 + cc < bx.lo2 || e0 + cc > bx.hi2) r[cc] = (REAL)0;
        }
        T v[4];
#pragma unroll
        for (int cc = 0; cc < 4; cc++) v[cc] = (T)(r[cc] * scale);
#pragma unroll
        for (int q = 0; q < 4 / VT; q++) {
          const int f = e0 + q * VT;  // the first cell of this vector
          if (f >= 0 && f + VT <= g.nk) {
            nvt y;
            __builtin_memcpy(&y, &v[q * VT], sizeof(y));
            *reinterpret_cast<nvt*>(dst + u + f) = y;
          } else {  // the row's head or tail
#pragma unroll
            for (int cc = 0; cc < VT; cc++)
              if (f + cc >= 0 && f + cc < g.nk) dst[u + f + cc] = v[q * VT + cc];
          }
        }
      }
    }
  }
  const double a1[1] = {acc};
  sums_finish<256>(a1, partials, counter, wsum, [&](const double (&tot)[1]) { out[0] = tot[0]; });
}

template <class T>
__global__ __launch_bounds__(256) void addf_row_k(REAL* __restrict__ Pd, const T* __restrict__ src, const FieldGeom g, const FieldBox bx, const REAL scale,
                                                  const int slots) {
  constexpr int V = 16 / sizeof(REAL);
  const int per_plane = g.ni * slots;
  for (int j = blockIdx.y + bx.lo1; j <= bx.hi1; j += gridDim.y) {
    for (int it = blockIdx.x * 256 + threadIdx.x; it < per_plane; it += gridDim.x * 256) {
      const int i = it / slots, s = it - i * slots;
      if (i < bx.lo0 || i > bx.hi0) continue;
      const long long a = (long long)(j + g.g) * g.PSE + (long long)(i + g.g) * g.nkp + g.g;
      const long long u = (long long)i * g.s0 + (long long)j * g.s1;
      // vector s of the row, counted from the 16-byte boundary at or before P's cell 0 of the row
      const int ph = (int)((reinterpret_cast<uintptr_t>(Pd + a) / sizeof(REAL)) & (uintptr_t)(V - 1));
      const int e0 = s * V - ph;
      if (e0 > bx.hi2) continue;
      if (e0 >= bx.lo2 && e0 + V - 1 <= bx.hi2) {
        Vec<V> p = ldv<V>(Pd + a + e0, 0);
        T x[V];
        ldt<T, V>(src, u + e0, x);
#pragma unroll
        for (int cc = 0; cc < V; cc++) p.v[cc] = p.v[cc] + (REAL)x[cc] * scale;
        stv<V>(Pd + a + e0, 0, p);
      } else {  // a vector that the box cuts
        const int c1 = e0 + V - 1 < bx.hi2 ? e0 + V - 1 : bx.hi2;
        for (int cc = e0 > bx.lo2 ? e0 : bx.lo2; cc <= c1; cc++) Pd[a + cc] = Pd[a + cc] + (REAL)src[u + cc] * scale;
      }
    }
  }
}
