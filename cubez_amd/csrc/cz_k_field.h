// cz_k_field.h -- part of cz_kernels.hip (ONE translation unit per precision; this file is included inside its anonymous
// namespace and is not a stand-alone header): a caller's brick <-> the padded array (cz_set_rhs, cz_set_field, cz_get_field).
//
// The caller's array U holds the brick's ni x nj x nk cells without guide cells, cell (i, j, k) 0-based at U[i s0 + j s1 + k s2] (strides in
// elements, any positive values); the padded array A holds it at A[(j + g) PSE + (i + g) nkp + (k + g)].  DIR 0: U -> A (import), DIR 1: A -> U
// (export).  Only the brick's cells are written on either side.  Three forms, chosen on the host from the strides (field_copy_async):
//   field_row_k   s2 == 1: both sides have k rows.  A row is cut into 16-byte vectors of the DESTINATION (its rows start anywhere: k offset g, odd
//                 pitches, a caller's slice), stored aligned; the source is read with REAL-aligned 16-byte loads; the cells before the first and
//                 after the last whole vector of a row go one by one.
//   field_tr_k    s0 == 1 or s1 == 1: the unit stride of U is i (or j), that of A is k.  A 64 x 64 tile goes through LDS, read along one side's
//                 unit stride and written along the other's, so both sides move runs of 64 elements (256 / 512 bytes).  The tile's pitch is
//                 65 elements: the transposed access has lane stride 65 REALs, which is one bank (FP32) or two (FP64, whose 8-byte accesses
//                 take two banks each) further per lane -- no two lanes of a 32-lane group share a bank.
//   field_any_k   every other stride triple: one cell per thread, k fastest on A's side.  Correct; no performance claim.
// Offsets are long long throughout (1024^3 and beyond).
// The transpose and generic forms also serve cz_get_residual and cz_add_field (their row forms are cz_k_resid.h): the caller's
// side has element type T (float | double, whatever REAL is), and OP 1 is the scaled, boxed form of the copy -- DIR 1: U = (T)(A scale) at
// the cells of the box and 0 at the brick's other cells (the residual in WRK out to the caller); DIR 0: A = A + (REAL)U scale at the cells of
// the box, A's other cells untouched (the correction into P).  The product is one REAL multiplication, the conversion comes after it.
// OP 0 is the plain copy, T = REAL.
struct FieldBox {  // the cells every sweep updates, 0-based in the brick, inclusive
  int lo0, hi0, lo1, hi1, lo2, hi2;
};
__device__ __forceinline__ bool field_in(const FieldBox& b, int c0, int c1, int c2) {
  return c0 >= b.lo0 && c0 <= b.hi0 && c1 >= b.lo1 && c1 <= b.hi1 && c2 >= b.lo2 && c2 <= b.hi2;
}
template <int DIR, class T>
struct FieldSides {  // element types of the destination and the source
  typedef REAL D;
  typedef T S;
};
template <class T>
struct FieldSides<1, T> {
  typedef T D;
  typedef REAL S;
};
struct FieldGeom {
  int ni, nj, nk, g;
  int nkp;               // elements per k row of A
  long long PSE;         // elements per j plane of A
  long long s0, s1, s2;  // U's strides in elements
};

template <int V, int DIR>
__global__ __launch_bounds__(256) void field_row_k(REAL* __restrict__ dst, const REAL* __restrict__ src, const FieldGeom g, const int slots) {
  const int per_plane = g.ni * slots;
  for (int j = blockIdx.y; j < g.nj; j += gridDim.y) {
    for (int it = blockIdx.x * 256 + threadIdx.x; it < per_plane; it += gridDim.x * 256) {
      const int i = it / slots, s = it - i * slots;
      const long long a = (long long)(j + g.g) * g.PSE + (long long)(i + g.g) * g.nkp + g.g;
      const long long u = (long long)i * g.s0 + (long long)j * g.s1;
      const long long d0 = DIR ? u : a, r0 = DIR ? a : u;
      // vector s of the row, counted from the 16-byte boundary at or before the destination row's first cell
      const int ph = (int)((reinterpret_cast<uintptr_t>(dst + d0) / sizeof(REAL)) & (uintptr_t)(V - 1));
      const int e0 = s * V - ph;
      if (e0 >= g.nk) continue;
      if (e0 >= 0 && e0 + V <= g.nk) {
        stv<V>(dst + d0 + e0, 0, ldve<V>(src, r0 + e0));
      } else {  // the row's head or tail
        const int c1 = e0 + V < g.nk ? e0 + V : g.nk;
        for (int c = e0 > 0 ? e0 : 0; c < c1; c++) dst[d0 + c] = src[r0 + c];
      }
    }
  }
}

// the tile: cells (u0 .. u0+63, k0 .. k0+63) of line w.  A: a0 + u a_us + w a_ws + k;  U: u + w u_ws + k u_ks
struct FieldTGeom {
  int nu, nw, nk;
  long long a0, a_us, a_ws;
  long long u_ws, u_ks;
};
constexpr int FIELD_TS = 64, FIELD_TP = FIELD_TS + 1;

// bx (OP 1): the box in the tile's directions (u, w, k)
template <int DIR, class T = REAL, int OP = 0>
__global__ __launch_bounds__(256) void field_tr_k(typename FieldSides<DIR, T>::D* __restrict__ dst, const typename FieldSides<DIR, T>::S* __restrict__ src,
                                                  const FieldTGeom g, const FieldBox bx, const REAL scale) {
  __shared__ REAL tile[FIELD_TS * FIELD_TP];  // tile[kk * FIELD_TP + uu]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int u0 = blockIdx.x * FIELD_TS, k0 = blockIdx.y * FIELD_TS;
  for (int w = blockIdx.z; w < g.nw; w += gridDim.z) {
    if (DIR == 0) {  // U's rows run along u
      if (u0 + lane < g.nu) {
        const long long ub = (long long)(u0 + lane) + (long long)w * g.u_ws;
        for (int kk = wave; kk < FIELD_TS && k0 + kk < g.nk; kk += 4) tile[kk * FIELD_TP + lane] = (REAL)src[ub + (long long)(k0 + kk) * g.u_ks];
      }
    } else {  // A's rows run along k
      if (k0 + lane < g.nk) {
        const long long ab = g.a0 + (long long)w * g.a_ws + (k0 + lane);
        for (int uu = wave; uu < FIELD_TS && u0 + uu < g.nu; uu += 4) tile[lane * FIELD_TP + uu] = src[ab + (long long)(u0 + uu) * g.a_us];
      }
    }
    __syncthreads();
    if (DIR == 0) {
      if (k0 + lane < g.nk) {
        const long long ab = g.a0 + (long long)w * g.a_ws + (k0 + lane);
        for (int uu = wave; uu < FIELD_TS && u0 + uu < g.nu; uu += 4) {
          const long long d = ab + (long long)(u0 + uu) * g.a_us;
          if (!OP) dst[d] = tile[lane * FIELD_TP + uu];
          else if (field_in(bx, u0 + uu, w, k0 + lane)) dst[d] = dst[d] + tile[lane * FIELD_TP + uu] * scale;
        }
      }
    } else {
      if (u0 + lane < g.nu) {
        const long long ub = (long long)(u0 + lane) + (long long)w * g.u_ws;
        for (int kk = wave; kk < FIELD_TS && k0 + kk < g.nk; kk += 4) {
          const long long d = ub + (long long)(k0 + kk) * g.u_ks;
          if (!OP) dst[d] = (T)tile[kk * FIELD_TP + lane];
          else dst[d] = field_in(bx, u0 + lane, w, k0 + kk) ? (T)(tile[kk * FIELD_TP + lane] * scale) : (T)0;
        }
      }
    }
    __syncthreads();  // (the next line's tile)
  }
}

template <int DIR, class T = REAL, int OP = 0>
__global__ __launch_bounds__(256) void field_any_k(typename FieldSides<DIR, T>::D* __restrict__ dst, const typename FieldSides<DIR, T>::S* __restrict__ src,
                                                   const FieldGeom g, const FieldBox bx, const REAL scale) {
  const long long per_plane = (long long)g.ni * g.nk;
  for (int j = blockIdx.y; j < g.nj; j += gridDim.y) {
    for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < per_plane; it += (long long)gridDim.x * 256) {
      const int i = (int)(it / g.nk), k = (int)(it - (long long)i * g.nk);
      const long long a = (long long)(j + g.g) * g.PSE + (long long)(i + g.g) * g.nkp + (k + g.g);
      const long long u = (long long)i * g.s0 + (long long)j * g.s1 + (long long)k * g.s2;
      if (!OP) {
        if (DIR) dst[u] = (T)src[a];
        else dst[a] = (REAL)src[u];
      } else if (DIR) {
        dst[u] = field_in(bx, i, j, k) ? (T)(src[a] * scale) : (T)0;
      } else if (field_in(bx, i, j, k)) {
        dst[a] = dst[a] + (REAL)src[u] * scale;
      }
    }
  }
}
