// cz_k_coef.h -- part of cz_kernels.hip (ONE translation unit per precision; this file is included inside its anonymous
// namespace and is not a stand-alone header): face coefficients for pcg (cz_set_face_coef).
//
// BX, BY, BZ are padded arrays of the handle (cz_k_field.h's A side): BX at cell c is the coefficient on the face between c and c + e_x,
// faces 0 .. ni - 2 at inner tangential cells; in a periodic direction face 0 holds a copy of face n - 2 (coef_prep_k writes it), so no
// kernel below carries a wrap branch.  P's face layers are what the handle's state made them (Dirichlet value, mirror, wrap).
//   per direction  t_d = B_d(c) (p(c + e_d) - p(c)) - B_d(c - e_d) (p(c) - p(c - e_d)),   A p = (t_x + t_y) + t_z,   r = b - A p
// every operation rounded once in REAL (the translation unit is built without contraction).
//   coef_prep_k   after the import, and again when the periodic directions change: the alias faces, the count of faces the operator reads
//                 that are not finite and positive (and of cells whose scaling is not), and S = sqrt(6 / D) at the cells of the box, D = ((bx+ + bx-) + (by+ + by-)) + (bz+ + bz-), 0 at the brick's
//                 other cells.  One cell per thread: it runs once per set of coefficients.
//   ax_coef_k     MODE 0: Q = A p at the cells of the box, sums p.q and q.q (REAL products, double sums: blas_dot2's terms);
//                 MODE 1: Q = b - A p there, sum r^2 (double squares, as resid_row_k).  Q's other cells are not written.  k across the lanes, a
//                 row cut into the 16-byte vectors of Q, stored aligned; every operand loaded with REAL-aligned 16-byte loads (the rows i - 1,
//                 i + 1, j - 1, j + 1 of P and i - 1, j - 1 of BX, BY are the rows neighbouring threads ask for at the same time: L2 / MALL);
//                 a vector that the box cuts goes cell by cell.  The sums go through the workgroups' partials and are added in index order by
//                 the workgroup that arrives last (sums_finish, cz_k_sums.h; MODE 1 has one sum).
//   coef_scale_k  out = S in where S is not zero, 0 elsewhere, over whole padded arrays (S is zero outside the box): the diagonal scaling
//                 either side of the preconditioner.  out may be in.
//   grad_coef_*   cz_sub_grad's coefficient form: U(i) = U(i) - (BX(i) (P(i+1) - P(i))) scale, V and W likewise -- grad_row_k / grad_any_k with
//                 one more operand; kernels of their own so that those two keep their code.
// Offsets are long long throughout.
__device__ __forceinline__ bool coef_ok(REAL b) { return b > (REAL)0 && b <= std::numeric_limits<REAL>::max(); }

// face 0 (element a, the direction's step `st`, n cells): now = the direction is periodic, was = face 0 holds the copy already
__device__ __forceinline__ void coef_alias(REAL* __restrict__ C, long long a, long long st, int n, int now, int was) {
  if (now && !was) {
    C[a - st] = C[a];
    C[a] = C[a + (long long)(n - 2) * st];
  } else if (!now && was) {
    C[a] = C[a - st];
  }
}

__global__ __launch_bounds__(256) void coef_prep_k(REAL* __restrict__ BX, REAL* __restrict__ BY, REAL* __restrict__ BZ, REAL* __restrict__ S,
                                                   const FieldGeom g, const FieldBox bx, const int per, const int per_old, unsigned* bad) {
  const long long per_plane = (long long)g.ni * g.nk;
  unsigned nbad = 0u;
  for (int j = blockIdx.y; j < g.nj; j += gridDim.y) {
    for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < per_plane; it += (long long)gridDim.x * 256) {
      const int i = (int)(it / g.nk), k = (int)(it - (long long)i * g.nk);
      const long long a = (long long)(j + g.g) * g.PSE + (long long)(i + g.g) * g.nkp + (k + g.g);
      const bool in_i = i >= 1 && i <= g.ni - 2, in_j = j >= 1 && j <= g.nj - 2, in_k = k >= 1 && k <= g.nk - 2;
      // face 0 of a periodic direction: the copy of face n - 2 (nobody reads face 0 in this launch); the caller's own value waits in the
      // guide layer behind it for the day the direction stops being periodic (per_old: the directions that hold a copy already)
      if (i == 0 && in_j && in_k) coef_alias(BX, a, (long long)g.nkp, g.ni, per & 1, per_old & 1);
      if (j == 0 && in_i && in_k) coef_alias(BY, a, g.PSE, g.nj, per & 2, per_old & 2);
      if (k == 0 && in_i && in_j) coef_alias(BZ, a, 1LL, g.nk, per & 4, per_old & 4);
      REAL s = (REAL)0;
      if (field_in(bx, i, j, k)) {
        // (the face behind cell 1: face n - 2 in a periodic direction; the guide layer where face 0 is being restored in this launch)
        const long long im = i != 1 ? -(long long)g.nkp : (per & 1) ? (long long)(g.ni - 3) * g.nkp : (per_old & 1) ? -2LL * g.nkp : -(long long)g.nkp;
        const long long jm = j != 1 ? -g.PSE : (per & 2) ? (long long)(g.nj - 3) * g.PSE : (per_old & 2) ? -2LL * g.PSE : -g.PSE;
        const long long km = k != 1 ? -1LL : (per & 4) ? (long long)(g.nk - 3) : (per_old & 4) ? -2LL : -1LL;
        const REAL xp = BX[a], xm = BX[a + im], yp = BY[a], ym = BY[a + jm], zp = BZ[a], zm = BZ[a + km];
        const REAL d = ((xp + xm) + (yp + ym)) + (zp + zm);
        s = sqrt((REAL)6 / d);
        if (!(coef_ok(xp) && coef_ok(xm) && coef_ok(yp) && coef_ok(ym) && coef_ok(zp) && coef_ok(zm) && coef_ok(s))) nbad++;
      }
      S[a] = s;
    }
  }
  if (nbad) atomicAdd(bad, nbad);
}

// A p at the cell at element e of the padded arrays
__device__ __forceinline__ REAL coef_ax_cell(const REAL* __restrict__ P, const REAL* __restrict__ BX, const REAL* __restrict__ BY, const REAL* __restrict__ BZ,
                                             long long e, long long nkp, long long PSE) {
  const REAL pc = P[e];
  const REAL tx = BX[e] * (P[e + nkp] - pc) - BX[e - nkp] * (pc - P[e - nkp]);
  const REAL ty = BY[e] * (P[e + PSE] - pc) - BY[e - PSE] * (pc - P[e - PSE]);
  const REAL tz = BZ[e] * (P[e + 1] - pc) - BZ[e - 1] * (pc - P[e - 1]);
  return (tx + ty) + tz;
}

template <int V, int MODE>
__global__ __launch_bounds__(256) void ax_coef_k(REAL* __restrict__ Q, const REAL* __restrict__ P, const REAL* __restrict__ B, const REAL* __restrict__ BX,
                                                 const REAL* __restrict__ BY, const REAL* __restrict__ BZ, const FieldGeom g, const FieldBox bx,
                                                 const int slots, double* partials, double* out, unsigned* counter) {
  __shared__ double wsum[5];  // cz_k_sums.h
  const int per_plane = (bx.hi0 - bx.lo0 + 1) * slots;
  const long long nkp = g.nkp;
  double acc0 = 0.0, acc1 = 0.0;
  for (int j = bx.lo1 + blockIdx.y; j <= bx.hi1; j += gridDim.y) {
    for (int it = blockIdx.x * 256 + threadIdx.x; it < per_plane; it += gridDim.x * 256) {
      const int ii = it / slots, s = it - ii * slots;
      const int i = bx.lo0 + ii;
      const long long a = (long long)(j + g.g) * g.PSE + (long long)(i + g.g) * nkp + g.g;
      // vector s of the row, counted from the 16-byte boundary at or before the row's first cell in Q
      const int ph = (int)((reinterpret_cast<uintptr_t>(Q + a) / sizeof(REAL)) & (uintptr_t)(V - 1));
      const int e0 = s * V - ph;
      if (e0 > bx.hi2 || e0 + V - 1 < bx.lo2) continue;
      if (e0 >= bx.lo2 && e0 + V - 1 <= bx.hi2) {
        const long long e = a + e0;
        const Vec<V> pc = ldve<V>(P, e), pim = ldve<V>(P, e - nkp), pip = ldve<V>(P, e + nkp), pjm = ldve<V>(P, e - g.PSE), pjp = ldve<V>(P, e + g.PSE);
        const Vec<V> xc = ldve<V>(BX, e), xm = ldve<V>(BX, e - nkp), yc = ldve<V>(BY, e), ym = ldve<V>(BY, e - g.PSE), zc = ldve<V>(BZ, e);
        const REAL kl = P[e - 1], kr = P[e + V], zl = BZ[e - 1];
        Vec<V> bb = zerov<V>();
        if (MODE == 1) bb = ldve<V>(B, e);
        Vec<V> q;
#pragma unroll
        for (int cc = 0; cc < V; cc++) {
          const REAL km1 = cc == 0 ? kl : pc.v[cc > 0 ? cc - 1 : 0];
          const REAL kp1 = cc == V - 1 ? kr : pc.v[cc < V - 1 ? cc + 1 : V - 1];
          const REAL zm = cc == 0 ? zl : zc.v[cc > 0 ? cc - 1 : 0];
          const REAL c = pc.v[cc];
          const REAL tx = xc.v[cc] * (pip.v[cc] - c) - xm.v[cc] * (c - pim.v[cc]);
          const REAL ty = yc.v[cc] * (pjp.v[cc] - c) - ym.v[cc] * (c - pjm.v[cc]);
          const REAL tz = zc.v[cc] * (kp1 - c) - zm * (c - km1);
          const REAL ap = (tx + ty) + tz;
          if (MODE == 1) {
            const REAL r = bb.v[cc] - ap;
            q.v[cc] = r;
            acc0 += (double)r * (double)r;
          } else {
            q.v[cc] = ap;
            acc0 += (double)(ap * c);
            acc1 += (double)(ap * ap);
          }
        }
        stv<V>(Q + e, 0, q);
      } else {  // a vector that the box cuts
        const int c1 = e0 + V - 1 < bx.hi2 ? e0 + V - 1 : bx.hi2;
        for (int k = e0 > bx.lo2 ? e0 : bx.lo2; k <= c1; k++) {
          const REAL ap = coef_ax_cell(P, BX, BY, BZ, a + k, nkp, g.PSE);
          if (MODE == 1) {
            const REAL r = B[a + k] - ap;
            Q[a + k] = r;
            acc0 += (double)r * (double)r;
          } else {
            Q[a + k] = ap;
            acc0 += (double)(ap * P[a + k]);
            acc1 += (double)(ap * ap);
          }
        }
      }
    }
  }
  const double acc[2] = {acc0, acc1};
  sums_finish<256>(acc, partials, counter, wsum, [&](const double (&tot)[2]) { out[0] = tot[0], out[1] = tot[1]; });
}

// (no __restrict__: the scaling after the preconditioner runs in place)
template <int V>
__global__ __launch_bounds__(256) void coef_scale_k(REAL* out, const REAL* in, const REAL* __restrict__ S, const long long nvec, const long long n) {
  for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < nvec; v += (long long)gridDim.x * 256) {
    if ((v + 1) * V <= n) {
      const Vec<V> s = ldv<V>(S, v), x = ldv<V>(in, v);
      Vec<V> y;
#pragma unroll
      for (int cc = 0; cc < V; cc++) y.v[cc] = s.v[cc] != (REAL)0 ? s.v[cc] * x.v[cc] : (REAL)0;
      stv<V>(out, v, y);
    } else {
      for (long long c = v * V; c < n; c++) out[c] = S[c] != (REAL)0 ? S[c] * in[c] : (REAL)0;
    }
  }
}

// grad_row_part with the coefficient: X = X - (C (P(+pstep) - P)) scale, C the padded coefficient array of X's direction
template <int V>
__device__ __forceinline__ void grad_coef_row_part(REAL* __restrict__ X, const REAL* __restrict__ P, const REAL* __restrict__ C, long long u, long long a,
                                                   long long pstep, int s, int klo, int khi, long long alias, bool wrap_k, REAL scale) {
  const int ph = (int)((reinterpret_cast<uintptr_t>(X + u) / sizeof(REAL)) & (uintptr_t)(V - 1));
  const int e0 = s * V - ph;
  if (e0 > khi || e0 + V - 1 < klo) return;
  if (e0 >= klo && e0 + V - 1 <= khi) {
    Vec<V> x = ldv<V>(X + u + e0, 0);
    const Vec<V> p0 = ldve<V>(P, a + e0), p1 = ldve<V>(P, a + e0 + pstep), c = ldve<V>(C, a + e0);
#pragma unroll
    for (int cc = 0; cc < V; cc++) x.v[cc] = x.v[cc] - (c.v[cc] * (p1.v[cc] - p0.v[cc])) * scale;
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
      const REAL x = X[u + k] - (C[a + k] * (P[a + k + pstep] - P[a + k])) * scale;
      X[u + k] = x;
      if (alias) X[u + alias + k] = x;
      if (wrap_k && k == khi) X[u] = x;
    }
  }
}

template <int V>
__global__ __launch_bounds__(256) void grad_coef_row_k(REAL* __restrict__ U, REAL* __restrict__ Vv, REAL* __restrict__ W, const REAL* __restrict__ P,
                                                       const REAL* __restrict__ BX, const REAL* __restrict__ BY, const REAL* __restrict__ BZ,
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
        grad_coef_row_part<V>(U, P, BX, u, a, (long long)g.nkp, s, 1, g.nk - 2, ((per & 1) && i == g.ni - 2) ? -(long long)(g.ni - 2) * g.s0 : 0LL, false, scale);
      if (in_i && j <= g.nj - 2 && !((per & 2) && j == 0))
        grad_coef_row_part<V>(Vv, P, BY, u, a, g.PSE, s, 1, g.nk - 2, ((per & 2) && j == g.nj - 2) ? -(long long)(g.nj - 2) * g.s1 : 0LL, false, scale);
      if (in_i && in_j) grad_coef_row_part<V>(W, P, BZ, u, a, 1LL, s, (per & 4) ? 1 : 0, g.nk - 2, 0LL, (per & 4) != 0, scale);
    }
  }
}

__global__ __launch_bounds__(256) void grad_coef_any_k(REAL* __restrict__ U, REAL* __restrict__ Vv, REAL* __restrict__ W, const REAL* __restrict__ P,
                                                       const REAL* __restrict__ BX, const REAL* __restrict__ BY, const REAL* __restrict__ BZ,
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
        const REAL x = U[u] - (BX[a] * (P[a + g.nkp] - pc)) * scale;
        U[u] = x;
        if ((per & 1) && i == g.ni - 2) U[u - (long long)(g.ni - 2) * g.s0] = x;
      }
      if (in_i && in_k && j <= g.nj - 2 && !((per & 2) && j == 0)) {
        const REAL x = Vv[u] - (BY[a] * (P[a + g.PSE] - pc)) * scale;
        Vv[u] = x;
        if ((per & 2) && j == g.nj - 2) Vv[u - (long long)(g.nj - 2) * g.s1] = x;
      }
      if (in_i && in_j && k <= g.nk - 2 && !((per & 4) && k == 0)) {
        const REAL x = W[u] - (BZ[a] * (P[a + 1] - pc)) * scale;
        W[u] = x;
        if ((per & 4) && k == g.nk - 2) W[u - (long long)(g.nk - 2) * g.s2] = x;
      }
    }
  }
}
