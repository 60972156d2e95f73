// cz_k_mgline.h -- part of cz_kernels.hip (ONE translation unit per precision; this file is included inside its anonymous
// namespace and is not a stand-alone header): the zebra line smoother along Z of pcg ... mgrb under the coefficient hierarchy
// (cz_set_mg_lines).
//
// One sweep of colour c solves every row (I, J) with (I + J) & 1 == c exactly along K, IN PLACE, and relaxes; the four X / Y neighbour rows of
// a row have the other colour, so the sweep has no race.  Per row, n = nk, every operation rounded once in REAL (IEEE division):
//   f_K = b_K - (((X(I) u(I+1) + X(I-1) u(I-1)) + Y(J) u(J+1)) + Y(J-1) u(J-1))      a_K = Z(K-1)   c_K = Z(K)   d_K = -D_K
//   end K = 0   : folded ?  d_0 = d_0 + Z(-1)          :  f_0 = f_0 - Z(-1) u(-1)
//   end K = n-1 : folded ?  d_{n-1} = d_{n-1} + Z(n-1) :  f_{n-1} = f_{n-1} - Z(n-1) u(n)
//   forward :  cp_0 = c_0 / d_0,  dp_0 = f_0 / d_0;   m = d_K - a_K cp_{K-1},  cp_K = c_K / m,  dp_K = (f_K - a_K dp_{K-1}) / m
//   backward:  y_{n-1} = dp_{n-1};   y_K = dp_K - cp_K y_{K+1}
//   update  :  x_K = u_K + (y_K - u_K) omega
//
// A workgroup owns MGL_ROWS rows of the colour and marches them in chunks of MGL_CHUNK cells.  Global memory is only ever touched with k
// across the lanes: four lanes share a row's chunk, one 16-byte vector each (REAL-aligned loads, the rows' pitch is odd), and write f, d
// and Z into LDS tiles of MGL_ROWS x MGL_CHUNK.  The recurrences then run one row per lane out of the tiles, read transposed: the tile row
// is padded to MGL_CHUNK + 1 REALs, an odd number, so the 32 lanes that one ds_read_b32 / ds_read_b64 serves together fall on distinct
// banks.  cp and dp carry across chunks in registers and go to global scratch (coalesced, rows of this colour only) for the backward
// march, which comes back chunk by chunk through the same tiles and writes x coalesced.  The last chunk of the forward march stays in LDS.
constexpr int MGL_ROWS = 256;               // rows per workgroup = threads per workgroup
constexpr int MGL_SLOTS = 4;                // 16-byte vectors per row and chunk
constexpr int MGL_CHUNK = MGL_SLOTS * VW;   // C: cells per row and chunk (FP32 16, FP64 8)
constexpr int MGL_PITCH = MGL_CHUNK + 1;    // REALs per tile row
// (a thread moves vector `slot` of MGL_SLOTS rows per chunk: the workgroup's rows in MGL_SLOTS groups of MGL_ROWS / MGL_SLOTS)

struct MgLine {
  int c;             // the colour swept
  int fold;          // bit 0: the end K = 0 is folded, bit 1: the end K = n - 1
  int mh;            // rows of one colour per plane J at most: ceil(ni / 2)
  int rows;          // nj * mh
  long long pitch;   // REALs per row of the scratch tables (a multiple of the vector width)
};

// f, d, Z of the V cells at element e (row (I, J), cells K .. K + V - 1), before the ends.  ZMODE 1: every u a literal +0 -- the products
// are weights (finite, not negative) times +0 and f = b - (+0) = b: only b, D, Z are read
template <int V, int ZMODE>
__device__ __forceinline__ void mgl_vec(const REAL* x, const REAL* __restrict__ b, const MgcW& W, long long e, long long si, long long sj, Vec<V>& f, Vec<V>& d,
                                        Vec<V>& z) {
  const Vec<V> bb = ldve<V>(b, e), dd = ldve<V>(W.d, e);
  z = ldve<V>(W.z, e);
  if (ZMODE == 1) {
#pragma unroll
    for (int cc = 0; cc < V; cc++) f.v[cc] = bb.v[cc], d.v[cc] = -dd.v[cc];
    return;
  }
  const Vec<V> pim = ldve<V>(x, e - si), pip = ldve<V>(x, e + si), pjm = ldve<V>(x, e - sj), pjp = ldve<V>(x, e + sj);
  const Vec<V> xc = ldve<V>(W.x, e), xm = ldve<V>(W.x, e - si), yc = ldve<V>(W.y, e), ym = ldve<V>(W.y, e - sj);
#pragma unroll
  for (int cc = 0; cc < V; cc++) {
    f.v[cc] = bb.v[cc] - (((xc.v[cc] * pip.v[cc] + xm.v[cc] * pim.v[cc]) + yc.v[cc] * pjp.v[cc]) + ym.v[cc] * pjm.v[cc]);
    d.v[cc] = -dd.v[cc];
  }
}
// one cell (a vector that the row's end cuts)
template <int ZMODE>
__device__ __forceinline__ void mgl_cell(const REAL* x, const REAL* __restrict__ b, const MgcW& W, long long e, long long si, long long sj, REAL& f, REAL& d, REAL& z) {
  z = W.z[e];
  d = -W.d[e];
  if (ZMODE == 1) f = b[e];
  else f = b[e] - (((W.x[e] * x[e + si] + W.x[e - si] * x[e - si]) + W.y[e] * x[e + sj]) + W.y[e - sj] * x[e - sj]);
}
// the two ends of a row on cell K at element e.  ZMODE != 0: the Z ghosts are literal zeros, f - Z (+0) = f
template <int ZMODE>
__device__ __forceinline__ void mgl_ends(const REAL* x, const MgcW& W, long long e, int K, int nk, int fold, REAL& f, REAL& d, REAL z) {
  if (K == 0) {
    if (fold & 1) d = d + W.z[e - 1];
    else if (ZMODE == 0) f = f - W.z[e - 1] * x[e - 1];
  }
  if (K == nk - 1) {
    if (fold & 2) d = d + z;
    else if (ZMODE == 0) f = f - z * x[e + 1];
  }
}

// ZMODE as mg_rb_k's Z: 0 from the iterate; 1 the first colour from zero (x is not read); 2 the second colour (its own row and its Z ghosts
// are literal zeros, the other colour is read).  grid: ceil(rows / MGL_ROWS) workgroups of MGL_ROWS threads
template <int V, int ZMODE>
__global__ void __launch_bounds__(MGL_ROWS) mg_line_k(REAL* x, const REAL* __restrict__ b, const MgLev L, const MgcW W, const REAL omg, const MgLine P,
                                                      REAL* __restrict__ scp, REAL* __restrict__ sdp) {
  __shared__ REAL tf[MGL_ROWS * MGL_PITCH], td[MGL_ROWS * MGL_PITCH], tz[MGL_ROWS * MGL_PITCH];
  constexpr int C = MGL_CHUNK, G = MGL_ROWS / MGL_SLOTS;
  const int t = threadIdx.x, slot = t & (MGL_SLOTS - 1), g = t / MGL_SLOTS;
  const long long si = L.nkp, sj = (long long)L.nkp * L.nip;
  const int nk = L.nk;
  // the rows this thread moves (row g + G p of the workgroup, vector `slot` of every chunk), and the row it solves (row t)
  long long ea[MGL_SLOTS];  // element of the row's cell K = 0; -1: no such row
#pragma unroll
  for (int p = 0; p < MGL_SLOTS; p++) {
    const int q = blockIdx.x * MGL_ROWS + g + G * p;
    const int J = q / P.mh, I = 2 * (q - J * P.mh) + ((J + P.c) & 1);
    ea[p] = q < P.rows && I < L.ni ? mg_at(L, I, J, 0) : -1;
  }
  bool mine;
  {
    const int q = blockIdx.x * MGL_ROWS + t;
    const int J = q / P.mh, I = 2 * (q - J * P.mh) + ((J + P.c) & 1);
    mine = q < P.rows && I < L.ni;
  }
  const int nchunk = (nk + C - 1) / C;
  REAL cp = (REAL)0, dp = (REAL)0, a = (REAL)0;
  // ---- forward: f, d, Z of a chunk into the tiles, the elimination out of them, cp and dp to the scratch
  for (int ch = 0; ch < nchunk; ch++) {
    const int k0 = ch * C, K = k0 + slot * V;
#pragma unroll
    for (int p = 0; p < MGL_SLOTS; p++) {
      if (ea[p] < 0 || K >= nk) continue;
      const long long e = ea[p] + K;
      const int o = (g + G * p) * MGL_PITCH + slot * V;
      Vec<V> f, d, z;
      const int nv = nk - K < V ? nk - K : V;
      if (nv == V) {
        mgl_vec<V, ZMODE>(x, b, W, e, si, sj, f, d, z);
      } else {
#pragma unroll
        for (int cc = 0; cc < V; cc++)
          if (cc < nv) mgl_cell<ZMODE>(x, b, W, e + cc, si, sj, f.v[cc], d.v[cc], z.v[cc]);
      }
      if (K == 0) mgl_ends<ZMODE>(x, W, e, 0, nk, P.fold, f.v[0], d.v[0], z.v[0]);  // (a one-cell row: both ends, K = 0 first)
      if (nk > 1 && K <= nk - 1 && nk - 1 < K + V) {
#pragma unroll
        for (int cc = 0; cc < V; cc++)
          if (K + cc == nk - 1) mgl_ends<ZMODE>(x, W, e + cc, nk - 1, nk, P.fold, f.v[cc], d.v[cc], z.v[cc]);
      }
#pragma unroll
      for (int cc = 0; cc < V; cc++)
        if (cc < nv) tf[o + cc] = f.v[cc], td[o + cc] = d.v[cc], tz[o + cc] = z.v[cc];
    }
    __syncthreads();
    if (mine) {
      const int cn = nk - k0 < C ? nk - k0 : C;
      for (int kk = 0; kk < cn; kk++) {
        const int o = t * MGL_PITCH + kk;
        const REAL f = tf[o], d = td[o], z = tz[o];
        if (k0 + kk == 0) {
          cp = z / d;
          dp = f / d;
        } else {
          const REAL m = d - a * cp;
          cp = z / m;
          dp = (f - a * dp) / m;
        }
        a = z;
        td[o] = cp, tf[o] = dp;
      }
    }
    __syncthreads();
    if (ch + 1 < nchunk) {  // (every vector of this chunk is whole: only the last chunk is cut)
#pragma unroll
      for (int p = 0; p < MGL_SLOTS; p++) {
        if (ea[p] < 0) continue;
        const int o = (g + G * p) * MGL_PITCH + slot * V;
        const long long s = (long long)(blockIdx.x * MGL_ROWS + g + G * p) * P.pitch + K;
        Vec<V> vc, vd;
#pragma unroll
        for (int cc = 0; cc < V; cc++) vc.v[cc] = td[o + cc], vd.v[cc] = tf[o + cc];
        stv<V>(scp + s, 0, vc);
        stv<V>(sdp + s, 0, vd);
      }
      __syncthreads();
    }
  }
  // ---- backward: cp and dp of a chunk back into the tiles (the last chunk is still there), the substitution, the relaxed update
  REAL y = (REAL)0;
  for (int ch = nchunk - 1; ch >= 0; ch--) {
    const int k0 = ch * C, K = k0 + slot * V;
    if (ch + 1 < nchunk) {
#pragma unroll
      for (int p = 0; p < MGL_SLOTS; p++) {
        if (ea[p] < 0) continue;
        const int o = (g + G * p) * MGL_PITCH + slot * V;
        const long long s = (long long)(blockIdx.x * MGL_ROWS + g + G * p) * P.pitch + K;
        const Vec<V> vc = ldv<V>(scp + s, 0), vd = ldv<V>(sdp + s, 0);
#pragma unroll
        for (int cc = 0; cc < V; cc++) td[o + cc] = vc.v[cc], tf[o + cc] = vd.v[cc];
      }
      __syncthreads();
    }
    if (mine) {
      const int cn = nk - k0 < C ? nk - k0 : C;
      for (int kk = cn - 1; kk >= 0; kk--) {
        const int o = t * MGL_PITCH + kk;
        y = k0 + kk == nk - 1 ? tf[o] : tf[o] - td[o] * y;
        tf[o] = y;
      }
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < MGL_SLOTS; p++) {
      if (ea[p] < 0 || K >= nk) continue;
      const long long e = ea[p] + K;
      const int o = (g + G * p) * MGL_PITCH + slot * V;
      const int nv = nk - K < V ? nk - K : V;
      if (nv == V) {
        Vec<V> u = zerov<V>(), out;
        if (ZMODE == 0) u = ldve<V>(x, e);
#pragma unroll
        for (int cc = 0; cc < V; cc++) out.v[cc] = u.v[cc] + (tf[o + cc] - u.v[cc]) * omg;
        stve<V>(x, e, out);
      } else {
#pragma unroll
        for (int cc = 0; cc < V; cc++)
          if (cc < nv) {
            const REAL u = ZMODE == 0 ? x[e + cc] : (REAL)0;
            x[e + cc] = u + (tf[o + cc] - u) * omg;
          }
      }
    }
    if (ch > 0) __syncthreads();
  }
}
