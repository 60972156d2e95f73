// cz_k_project.h -- part of cz_kernels.hip (ONE translation unit per precision; this file is included inside its anonymous
// namespace and is not a stand-alone header): the projection step on a staggered velocity (cz_set_rhs_div, cz_sub_grad).
//
// The velocity is three arrays U, V, W of the brick's shape with ONE stride triple (cz_k_field.h's U side: cell (i, j, k) 0-based at
// i s0 + j s1 + k s2); U(i, j, k) is the normal velocity on the face between cells i and i + 1, faces 0 .. ni - 2 (entry ni - 1 is never
// touched), V and W the same along j and k.  In a periodic direction (bit d of `per`) face 0 is an alias of face n - 2: ignored on input
// (face n - 2 is read in its place), on output it receives the value of face n - 2 from the thread that owns that face.  The padded arrays
// (RHS, P) are cz_k_field.h's A side.
//   div   at every inner cell  d = ((U(i) - U(i-1)) + (V(j) - V(j-1))) + (W(k) - W(k-1)),  RHS = d scale, each operation rounded once; 0 at the
//         brick's other cells; sum d^2 (double squares, double sums) through the workgroups' partials, summed in a fixed order by the
//         workgroup that arrives last (cz_k_sums.h).  3 reads + 1 write per cell: the rows i - 1 and j - 1 and the element k - 1 are
//         the rows and elements that neighbouring threads of the grid ask for at the same time, served by L2 / MALL.
//   grad  U(i, j, k) = U(i, j, k) - (P(i+1, j, k) - P(i, j, k)) scale for faces 0 .. ni - 2 at inner j, k; V and W likewise.  P's face layers
//         are the handle's (mirror, wrap or Dirichlet value).  A thread reads only elements of the velocity that it writes itself, and no
//         element is written by two threads: face 0 of a periodic direction has no owner and is only written.  1 read (P, its neighbour
//         rows from cache) + 3 read-modify-writes.
// Two forms each, chosen on the host (field_div_async, field_grad_async):
//   *_row_k  s2 == 1: k across the lanes, the row cut into the 16-byte vectors of the DESTINATION (the padded RHS; each of U, V, W -- their
//            phases differ, so a thread serves run s of the row once per component), stored aligned, everything else loaded with
//            REAL-aligned 16-byte loads, the cells before the first and after the last whole vector one by one (field_row_k's scheme).
//   *_any_k  any strides: one cell per thread.  Correct; no performance claim.
// Offsets are long long throughout.
__device__ __forceinline__ REAL div_cell(const REAL* __restrict__ U, const REAL* __restrict__ Vv, const REAL* __restrict__ W, long long u, long long um,
                                         long long vm, long long wm) {
  const REAL dx = U[u] - U[um], dy = Vv[u] - Vv[vm], dz = W[u] - W[wm];
  return (dx + dy) + dz;
}

template <int V>
__global__ __launch_bounds__(256) void div_row_k(REAL* __restrict__ B, const REAL* __restrict__ U, const REAL* __restrict__ Vv, const REAL* __restrict__ W,
                                                 const FieldGeom g, const int per, const REAL scale, const int slots, double* partials, double* out,
                                                 unsigned* counter) {
  __shared__ double wsum[5];  // cz_k_sums.h
  const int per_plane = g.ni * slots;
  double acc = 0.0;
  for (int j = blockIdx.y; j < g.nj; j += gridDim.y) {
    for (int it = blockIdx.x * 256 + threadIdx.x; it < per_plane; it += gridDim.x * 256) {
      const int i = it / slots, s = it - i * slots;
      const long long a = (long long)(j + g.g) * g.PSE + (long long)(i + g.g) * g.nkp + g.g;
      // vector s of the row, counted from the 16-byte boundary at or before the row's first cell in RHS
      const int ph = (int)((reinterpret_cast<uintptr_t>(B + a) / sizeof(REAL)) & (uintptr_t)(V - 1));
      const int e0 = s * V - ph;
      if (e0 >= g.nk) continue;
      const bool in_ij = i >= 1 && i <= g.ni - 2 && j >= 1 && j <= g.nj - 2;
      const long long u = (long long)i * g.s0 + (long long)j * g.s1;
      // (the rows behind: face n - 2 for face 0 in a periodic direction)
      const long long um = (long long)(((per & 1) && i == 1) ? g.ni - 2 : i - 1) * g.s0 + (long long)j * g.s1;
      const long long vm = (long long)i * g.s0 + (long long)(((per & 2) && j == 1) ? g.nj - 2 : j - 1) * g.s1;
      if (e0 >= 0 && e0 + V <= g.nk) {
        Vec<V> r = zerov<V>();
        if (in_ij) {
          const Vec<V> ua = ldve<V>(U, u + e0), ub = ldve<V>(U, um + e0), va = ldve<V>(Vv, u + e0), vb = ldve<V>(Vv, vm + e0);
          const Vec<V> wa = ldve<V>(W, u + e0);
          const REAL wl = e0 >= 1 ? W[u + e0 - 1] : (REAL)0;
          const REAL wp = ((per & 4) && e0 <= 1 && e0 + V > 1) ? W[u + g.nk - 2] : (REAL)0;  // (W(k - 1) of cell 1 across the seam)
#pragma unroll
          for (int cc = 0; cc < V; cc++) {
            const int k = e0 + cc;
            REAL wb = cc == 0 ? wl : wa.v[cc > 0 ? cc - 1 : 0];
            if ((per & 4) && k == 1) wb = wp;
            const REAL dx = ua.v[cc] - ub.v[cc], dy = va.v[cc] - vb.v[cc], dz = wa.v[cc] - wb;
            const REAL d = (dx + dy) + dz;
            if (k >= 1 && k <= g.nk - 2) {
              r.v[cc] = d * scale;
              acc += (double)d * (double)d;
            }
          }
        }
        stv<V>(B + a + e0, 0, r);
      } else {  // the row's head or tail
        const int c1 = e0 + V < g.nk ? e0 + V : g.nk;
        for (int k = e0 > 0 ? e0 : 0; k < c1; k++) {
          REAL r = (REAL)0;
          if (in_ij && k >= 1 && k <= g.nk - 2) {
            const REAL d = div_cell(U, Vv, W, u + k, um + k, vm + k, u + (((per & 4) && k == 1) ? g.nk - 2 : k - 1));
            r = d * scale;
            acc += (double)d * (double)d;
          }
          B[a + k] = r;
        }
      }
    }
  }
  const double a1[1] = {acc};
  sums_finish<256>(a1, partials, counter, wsum, [&](const double (&tot)[1]) { out[0] = tot[0]; });
}

__global__ __launch_bounds__(256) void div_any_k(REAL* __restrict__ B, const REAL* __restrict__ U, const REAL* __restrict__ Vv, const REAL* __restrict__ W,
                                                 const FieldGeom g, const int per, const REAL scale, double* partials, double* out, unsigned* counter) {
  __shared__ double wsum[5];  // cz_k_sums.h
  const long long per_plane = (long long)g.ni * g.nk;
  double acc = 0.0;
  for (int j = blockIdx.y; j < g.nj; j += gridDim.y) {
    for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < per_plane; it += (long long)gridDim.x * 256) {
      const int i = (int)(it / g.nk), k = (int)(it - (long long)i * g.nk);
      const long long a = (long long)(j + g.g) * g.PSE + (long long)(i + g.g) * g.nkp + (k + g.g);
      REAL r = (REAL)0;
      if (i >= 1 && i <= g.ni - 2 && j >= 1 && j <= g.nj - 2 && k >= 1 && k <= g.nk - 2) {
        const int im = ((per & 1) && i == 1) ? g.ni - 2 : i - 1, jm = ((per & 2) && j == 1) ? g.nj - 2 : j - 1;
        const int km = ((per & 4) && k == 1) ? g.nk - 2 : k - 1;
        const long long ij = (long long)i * g.s0 + (long long)j * g.s1;
        const REAL d = div_cell(U, Vv, W, ij + (long long)k * g.s2, (long long)im * g.s0 + (long long)j * g.s1 + (long long)k * g.s2,
                                (long long)i * g.s0 + (long long)jm * g.s1 + (long long)k * g.s2, ij + (long long)km * g.s2);
        r = d * scale;
        acc += (double)d * (double)d;
      }
      B[a] = r;
    }
  }
  const double a1[1] = {acc};
  sums_finish<256>(a1, partials, counter, wsum, [&](const double (&tot)[1]) { out[0] = tot[0]; });
}

// run s of the k row whose cell 0 is element u of X and element a of P: X = X - (P(+pstep) - P) scale at the cells klo .. khi.  alias != 0:
// the same values also go to the row at u + alias (face 0 of a periodic i or j; that row's phase is its own: REAL-aligned stores).  wrap_k:
// the value of cell khi also goes to cell 0 of the row (face 0 of a periodic k)
template <int V>
__device__ __forceinline__ void grad_row_part(REAL* __restrict__ X, const REAL* __restrict__ P, long long u, long long a, long long pstep, int s, int klo,
                                              int khi, long long alias, bool wrap_k, REAL scale) {
  const int ph = (int)((reinterpret_cast<uintptr_t>(X + u) / sizeof(REAL)) & (uintptr_t)(V - 1));
  const int e0 = s * V - ph;
  if (e0 > khi || e0 + V - 1 < klo) return;
  if (e0 >= klo && e0 + V - 1 <= khi) {
    Vec<V> x = ldv<V>(X + u + e0, 0);
    const Vec<V> p0 = ldve<V>(P, a + e0), p1 = ldve<V>(P, a + e0 + pstep);
#pragma unroll
    for (int cc = 0; cc < V; cc++) x.v[cc] = x.v[cc] - (p1.v[cc] - p0.v[cc]) * scale;
    stv<V>(X + u + e0, 0, x);
    if (alias) stve<V>(X, u + alias + e0, x);
    if (wrap_k) {
#pragma unroll
      for (int cc = 0; cc < V; cc++)
        if (e0 + cc == khi) X[u] = x.v[cc];
    }
  } else {  // a vector that the range cuts
    const int c1 = e0 + V - 1 < khi ? e0 + V - 1 : khi;
    for (int k = e0 > klo ? e0 : klo; k <= c1; k++) {
      const REAL x = X[u + k] - (P[a + k + pstep] - P[a + k]) * scale;
      X[u + k] = x;
      if (alias) X[u + alias + k] = x;
      if (wrap_k && k == khi) X[u] = x;
    }
  }
}

template <int V>
__global__ __launch_bounds__(256) void grad_row_k(REAL* __restrict__ U, REAL* __restrict__ Vv, REAL* __restrict__ W, const REAL* __restrict__ P,
                                                  const FieldGeom g, const int per, const REAL scale, const int slots) {
  const int per_plane = g.ni * slots;
  for (int j = blockIdx.y; j < g.nj; j += gridDim.y) {
    for (int it = blockIdx.x * 256 + threadIdx.x; it < per_plane; it += gridDim.x * 256) {
      const int i = it / slots, s = it - i * slots;
      const long long a = (long long)(j + g.g) * g.PSE + (long long)(i + g.g) * g.nkp + g.g;
      const long long u = (long long)i * g.s0 + (long long)j * g.s1;
      const bool in_i = i >= 1 && i <= g.ni - 2, in_j = j >= 1 && j <= g.nj - 2;
      // face 0 of a periodic direction has no owner: the owner of face n - 2 writes it
      if (in_j && i <= g.ni - 2 && !((per & 1) && i == 0))
        grad_row_part<V>(U, P, u, a, (long long)g.nkp, s, 1, g.nk - 2, ((per & 1) && i == g.ni - 2) ? -(long long)(g.ni - 2) * g.s0 : 0LL, false, scale);
      if (in_i && j <= g.nj - 2 && !((per & 2) && j == 0))
        grad_row_part<V>(Vv, P, u, a, g.PSE, s, 1, g.nk - 2, ((per & 2) && j == g.nj - 2) ? -(long long)(g.nj - 2) * g.s1 : 0LL, false, scale);
      if (in_i && in_j) grad_row_part<V>(W, P, u, a, 1LL, s, (per & 4) ? 1 : 0, g.nk - 2, 0LL, (per & 4) != 0, scale);
    }
  }
}

__global__ __launch_bounds__(256) void grad_any_k(REAL* __restrict__ U, REAL* __restrict__ Vv, REAL* __restrict__ W, const REAL* __restrict__ P,
                                                  const FieldGeom g, const int per, const REAL scale) {
  const long long per_plane = (long long)g.ni * g.nk;
  for (int j = blockIdx.y; j < g.nj; j += gridDim.y) {
    for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < per_plane; it += (long long)gridDim.x * 256) {
      const int i = (int)(it / g.nk), k = (int)(it - (long long)i * g.nk);
      const long long a = (long long)(j + g.g) * g.PSE + (long long)(i + g.g) * g.nkp + (k + g.g);
      const long long u = (long long)i * g.s0 + (long long)j * g.s1 + (long long)k * g.s2;
      const bool in_i = i >= 1 && i <= g.ni - 2, in_j = j >= 1 && j <= g.nj - 2, in_k = k >= 1 && k <= g.nk - 2;
      const REAL pc = P[a];
      if (in_j && in_k && i <= g.ni - 2 && !((per & 1) && i == 0)) {
        const REAL x = U[u] - (P[a + g.nkp] - pc) * scale;
        U[u] = x;
        if ((per & 1) && i == g.ni - 2) U[u - (long long)(g.ni - 2) * g.s0] = x;
      }
      if (in_i && in_k && j <= g.nj - 2 && !((per & 2) && j == 0)) {
        const REAL x = Vv[u] - (P[a + g.PSE] - pc) * scale;
        Vv[u] = x;
        if ((per & 2) && j == g.nj - 2) Vv[u - (long long)(g.nj - 2) * g.s1] = x;
      }
      if (in_i && in_j && k <= g.nk - 2 && !((per & 4) && k == 0)) {
        const REAL x = W[u] - (P[a + 1] - pc) * scale;
        W[u] = x;
        if ((per & 4) && k == g.nk - 2) W[u - (long long)(g.nk - 2) * g.s2] = x;
      }
    }
  }
}
