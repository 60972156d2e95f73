// cz_k_jac3.h -- part of cz_kernels.hip (ONE translation unit per precision; included inside its anonymous namespace after cz_k_rb4.h):
// jac3_k, THREE relaxed-Jacobi sweeps (cz_solver.f90:334-351 three times) per pass over memory.  Single-domain runs, constant coefficients.
// ------------------------------------------------------------------------------------------------------------
// Why: the two-sweep pass (jacobi2p_k) moves 1.11 x the bytes of one fused pass at 0.88 of the copy ceiling (profiles/hbm_traffic.json), so
// the only lever left on a large Jacobi solve is fewer bytes per sweep.  The arrangement is rb4_k's (cz_k_rb4.h) one stage shorter:
//     fields      u on E3 = own segment +- 3 rows, f1 (after sweep n+1) on E2, f2 (after sweep n+2) on E1, f3 = output on the segment
//     threads     one per vector of E2 (TB = LV = S + 4R), dealt in order (x = t): a Jacobi stage has no colour, so rows need no dealing by parity
//     stages      1 on all of E2; 2 on the waves that hold a vector of E1; 3 on the waves that own a vector (wave-uniform branches: the waves at
//                 the ends of E2 skip what no valid point reads)
//     LDS         u: 2 x (LV + 2R), f1, f2: 2 x LV each (by plane parity; the j-1 operand of a vector is read by the thread that wrote it)
//     k windows   KT vectors + hv halo vectors per side; three stages reach 3 elements beyond a window: hv = 1 (FP32), 2 (FP64)
//     planes      stage s at step q works on plane q - s + 1: f1(q) from u(q-1..q+1), f2(q-1) from f1, f3(q-2) -> W
// Per point: relax_vec<V, UNIT> with the hoisted IEEE division (or its checked shorter form, MED), the operations of jacobi2p_k on the same
// values => the same bits as three single sweeps.  The three residuals (sum dp^2 of sweeps n+1, n+2, n+3) are produced and finalised in the kernel; if the first or the second
// converges, the driver re-runs one sweep or one pair from the untouched input (out of place, like the pair).
// ------------------------------------------------------------------------------------------------------------

// the three-sum form of pair_finalize: the bookkeeping of cz_Poisson.cpp:67-77 for iterations itr, itr+1, itr+2 in order
template <int TB>
__device__ __forceinline__ void jac3_finalize(const double* partials, int nblk, const Fin2& fin, double* wsum) {
  const int t = threadIdx.x;
  double x[3] = {0.0, 0.0, 0.0};
  for (int i = t; i < nblk; i += TB) {
#pragma unroll
    for (int s = 0; s < 3; s++) x[s] += __hip_atomic_load(&partials[s * nblk + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  double tot[3];
#pragma unroll
  for (int s = 0; s < 3; s++) {
    __syncthreads();
    tot[s] = block_sum<TB>(x[s], wsum);
  }
  if (t == 0) {
#pragma unroll
    for (int s = 0; s < 3; s++) fin.dst[s] = tot[s];
    if (fin.do_check) {
      for (int s = 0; s < 3; s++) {
        const double r = sqrt(tot[s] * fin.res_normal);
        fin.hist[fin.itr + s] = r;
        if (r < fin.eps) {
          *fin.flag = 1;
          *fin.conv_itr = fin.itr + s;
          break;
        }
      }
    }
    *fin.counter = 0u;
  }
}

// MED = 1 (FP32): the division with one correction step (mediumdiv, cz_k_fastdiv.h), taken only for a divisor that passed the exhaustive
// comparison with `n / d` on this context (jac3_medium, cz_h_launch.h)
template <int V, int TB, int UNIT, int MED>
__global__ void __launch_bounds__(TB, 1)
jac3_k(const REAL* __restrict__ U, const REAL* __restrict__ B, REAL* __restrict__ W, Coef c, Geom2 g, double* partials,
       const int* __restrict__ skip, Fin2 fin) {
  if (skip != nullptr && *skip != 0) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int t = threadIdx.x;
  const int R = g.R;
  constexpr int LV = TB;      // E2: own segment +- two rows (S = LV - 4R); one vector per thread
  const int LU = LV + 2 * R;  // E3
  // (R vectors of padding in front of the u buffers and behind the last field buffer: stages 1 and 2 are evaluated on whole waves and the
  // lanes beyond their sets read +-R outside them -- inside the allocation, never used)
  Vec<V>* ldsU = reinterpret_cast<Vec<V>*>(smem) + R;  // 2 buffers of LU vectors: plane p in buffer p & 1
  Vec<V>* ldsF = ldsU + (size_t)2 * LU;                 // f1, f2: [field][plane & 1][LV]
  double* wsum = reinterpret_cast<double*>(ldsF + (size_t)4 * LV + R);

  // ---- workgroup -> (window, segment, chunk): as jacobi2p_k
  const int lb = blockIdx.x;
  const int nblk = gridDim.x;
  int seg, chunk;
  if (g.map != nullptr) {
    seg = g.map[2 * lb];
    chunk = g.map[2 * lb + 1];
  } else {
    const int xc = lb & 7, r = lb >> 3;
    const int base = g.nseg >> 3, rem = g.nseg & 7, bmax = base + (rem ? 1 : 0);
    const int blen = base + (xc < rem ? 1 : 0);
    const int sl = r % bmax;
    chunk = r / bmax;
    seg = (sl < blen) ? xc * base + min(xc, rem) + sl : g.nseg;  // nseg = no work
  }
  int win = 0;
  if (seg < g.nseg) {
    win = seg / g.nsegw;
    seg -= win * g.nsegw;
  } else {
    seg = g.nsegw;
  }
  const int kw0 = win * g.KW - g.hv * V;
  const long long fb = (seg < g.nsegw) ? g.F0 + (long long)seg * g.S : g.Fend;
  const int ja = g.jj0 + chunk * g.TJ;
  int jb = ja + g.TJ - 1;
  if (jb > g.jj1) jb = g.jj1;

  double acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
  const typename std::conditional<MED != 0, MediumDiv, HoistedDiv>::type dv{fastdiv_init(c.dd)};

  if (ja <= jb && fb < g.Fend) {
    const long long e2_0 = fb - 2 * (long long)R;  // first vector of E2
    const long long vlast = g.PSV - 1;
    const size_t PB = (size_t)g.PSB;
    auto off_of = [&](long long f) -> unsigned {  // (see jacobi2p_k: clamped below the plane, not beyond it; `lim` for the array's last plane)
      if (f < 0) f = 0;
      if (f > vlast) f = vlast;
      const long long r = f / R;
      long long el = r * g.nkp + kw0 + (f - r * R) * V;
      el = el < 0 ? 0 : el;
      return (unsigned)(el * (long long)sizeof(REAL));
    };
    auto lim = [&](unsigned off, int plane) -> unsigned { return plane == g.jlast ? (off < g.last_off ? off : g.last_off) : off; };
    auto pl = [&](int p) -> int { return p < 0 ? 0 : (p > g.jlast ? g.jlast : p); };  // planes beyond the array are never used: clamped
    const int x = t;  // this thread's vector: index in E2
    const long long f = e2_0 + x;
    const unsigned bo = off_of(f);
    unsigned inbox = 0;  // components inside the inner box (every stage updates only those)
    unsigned own = 0;    // ... of a vector this workgroup owns (stores, residual counts)
    {
      const long long fc = f < 0 ? 0 : f;
      const long long row = fc / R;
      const int kv = (int)(fc - row * R);
      const int kb = kw0 + kv * V;
      unsigned bits = 0;
#pragma unroll
      for (int cc = 0; cc < V; cc++) {
        const int kk = kb + cc;
        if (kk >= g.kk0 && kk <= g.kk1) bits |= 1u << cc;
      }
      const bool rows_in = f >= g.F0 && f < g.Fend;
      inbox = rows_in ? bits : 0u;
      const bool kown = kv >= g.hv && kv < g.hv + g.KT;
      own = (x >= 2 * R && x < LV - 2 * R && rows_in && kown) ? bits : 0u;
    }
    // wave-uniform: does this wave hold a vector of E1 (stage 2) / an owned vector (stage 3)?
    const bool wave2 = __builtin_amdgcn_ballot_w64(x >= R && x < LV - R) != 0ull;
    const bool wave3 = __builtin_amdgcn_ballot_w64(own != 0) != 0ull;
    // the outer rows of E3: the first R threads stage the lower one, the last R threads the upper one
    const bool has_halo = (t < R) || (t >= TB - R);
    const int hl = (t < R) ? t : (LV + R + (t - (TB - R)));  // index inside an LDS u buffer (E3 coordinates)
    const unsigned hbo = off_of(has_halo ? (fb - 3 * (long long)R + hl) : f);
    const char* Ub = reinterpret_cast<const char*>(U);
    const char* Bb = reinterpret_cast<const char*>(B);
    char* Wb = reinterpret_cast<char*>(W);

    // ---- prologue: the first step is q0 = ja - 2 (stage 1 on plane ja - 2): LDS u(q0 - 1) own, u(q0) on E3; in flight u(q0 + 1), b(q0)
    const int q0 = ja - 2;
    Vec<V> uA, uB, bA, bB, hx;
    {
      const Vec<V> t2 = ld16<V>(Ub + (size_t)pl(q0 - 1) * PB, lim(bo, pl(q0 - 1)));
      const Vec<V> t1 = ld16<V>(Ub + (size_t)pl(q0) * PB, lim(bo, pl(q0)));
      const Vec<V> h1 = ld16<V>(Ub + (size_t)pl(q0) * PB, lim(hbo, pl(q0)));
      uA = ld16<V>(Ub + (size_t)pl(q0 + 1) * PB, lim(bo, pl(q0 + 1)));
      bA = ld16<V>(Bb + (size_t)pl(q0) * PB, lim(bo, pl(q0)));
      ldsU[(size_t)((q0 - 1) & 1) * LU + R + x] = t2;
      ldsU[(size_t)(q0 & 1) * LU + R + x] = t1;
      if (has_halo) ldsU[(size_t)(q0 & 1) * LU + hl] = h1;
    }
    Vec<V> bq1 = zerov<V>(), bq2 = zerov<V>();  // b of the planes of stages 2, 3
    __syncthreads();

    // the k neighbours beyond the wave's first and last vector come from LDS (one element each, the same address in all lanes)
    const int x_first = __builtin_amdgcn_readfirstlane(x), x_last = __builtin_amdgcn_readlane(x, 63);
    auto stage = [&](const Vec<V>* cur, const Vec<V>* prv, const Vec<V>& nxt, const Vec<V>& bb, unsigned msk, unsigned cnt,
                     double& acc) __attribute__((always_inline)) -> Vec<V> {
      const Vec<V> pc = lds_ld<V>(cur + x);
      const Vec<V> im = lds_ld<V>(cur + x - R);
      const Vec<V> ip = lds_ld<V>(cur + x + R);
      const Vec<V> pm = lds_ld<V>(prv + x);
      const REAL elo = reinterpret_cast<const REAL*>(cur)[(long long)x_first * V - 1];
      const REAL ehi = reinterpret_cast<const REAL*>(cur)[(long long)(x_last + 1) * V];
      const REAL kl = lane_shr1(elo, pc.v[V - 1]);
      const REAL kr = lane_shl1(ehi, pc.v[0]);
      return relax_vec<V, UNIT>(pc, im, ip, pm, nxt, kl, kr, bb, c, dv, msk, cnt, acc);
    };

    // One plane step q.  uc = u(q+1) and b1 = b(q) were requested one step ago; un / bn receive this step's requests.
    auto step = [&](const int q, Vec<V>& uc, Vec<V>& un, Vec<V>& b1, Vec<V>& bn) __attribute__((always_inline)) {
      {
        const int qu = pl(q + 2 <= jb + 3 ? q + 2 : jb + 3), qb = pl(q + 1 <= jb + 2 ? q + 1 : jb + 2);
        hx = ld16<V>(Ub + (size_t)pl(q + 1) * PB, lim(hbo, pl(q + 1)));
        un = ld16<V>(Ub + (size_t)qu * PB, lim(bo, qu));
        bn = ld16<V>(Bb + (size_t)qb * PB, lim(bo, qb));
      }
      // planes of the three stages; masks: inside the inner box a stage updates, inside the chunk the owner counts the residual
      const int p1 = q, p2 = q - 1, p3 = q - 2;
      auto upd = [&](int p) -> unsigned { return (p >= g.jj0 && p <= g.jj1) ? inbox : 0u; };
      auto cnt = [&](int p) -> unsigned { return (p >= ja && p <= jb) ? own : 0u; };
      const Vec<V>* cU = ldsU + (size_t)(p1 & 1) * LU + R;  // u(p1) in E2 coordinates (index x)
      const Vec<V>* pU = ldsU + (size_t)((p1 - 1) & 1) * LU + R;
      Vec<V>* F1 = ldsF;
      Vec<V>* F2 = ldsF + (size_t)2 * LV;
      // ---- stage 1: f1(p1) on every vector of E2
      const Vec<V> v1 = stage(cU, pU, uc, b1, upd(p1), cnt(p1), acc1);
      // ---- stage 2: f2(p2) from f1(p2 - 1) [LDS], f1(p2) [LDS], f1(p1) [v1]
      Vec<V> v2 = v1;  // (a wave outside E1 publishes a value no valid point reads)
      if (wave2) v2 = stage(F1 + (size_t)(p2 & 1) * LV, F1 + (size_t)((p2 - 1) & 1) * LV, v1, bq1, upd(p2), cnt(p2), acc2);
      // ---- stage 3: f3(p3) = the output, owned vectors of the chunk's planes.  Whole waves: the k neighbours travel by lane shifts, and the
      // lane next to the first owned vector of a window holds a halo vector -- it owns nothing but must take part.
      if (p3 >= ja && wave3) {
        const Vec<V> o = stage(F2 + (size_t)(p3 & 1) * LV, F2 + (size_t)((p3 - 1) & 1) * LV, v2, bq2, own, own, acc3);
        char* Wq = Wb + (size_t)p3 * PB;
        if (own == (1u << V) - 1) {
          st16<V>(Wq, bo, o);
        } else if (own != 0) {
          REAL* wp = reinterpret_cast<REAL*>(Wq + bo);
#pragma unroll
          for (int cc = 0; cc < V; cc++)
            if (own & (1u << cc)) wp[cc] = o.v[cc];
        }
      }
      // ---- publish: f1(p1), f2(p2) and the next u centre plane u(q+1) with its outer rows
      F1[(size_t)(p1 & 1) * LV + x] = v1;
      F2[(size_t)(p2 & 1) * LV + x] = v2;
      Vec<V>* nU = ldsU + (size_t)((p1 + 1) & 1) * LU;
      nU[R + x] = uc;
      if (has_halo) nU[hl] = hx;
      bq2 = bq1, bq1 = b1;  // (b1 is complete: stage 1 used it)
      __syncthreads();
    };
    // (stage s first matters at plane ja - (3 - s), which it reaches at step ja - 2 + (s - 1): every field buffer a valid point reads was
    // written by a step of this loop)
    for (int q = q0;; q += 2) {
      step(q, uA, uB, bA, bB);
      if (q + 1 > jb + 2) break;
      step(q + 1, uB, uA, bB, bA);
      if (q + 2 > jb + 2) break;
    }
  }

  // ---- residuals of the three sweeps: per-workgroup partials, finalised by the last workgroup (see jacobi2p_k)
  __syncthreads();
  const double s1 = block_sum<TB>(acc1, wsum);
  __syncthreads();
  const double s2 = block_sum<TB>(acc2, wsum);
  __syncthreads();
  const double s3 = block_sum<TB>(acc3, wsum);
  int* last_flag = reinterpret_cast<int*>(wsum + 16);
  if (t == 0) {
    __hip_atomic_store(&partials[lb], s1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&partials[nblk + lb], s2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&partials[2 * nblk + lb], s3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *last_flag = arrive_and_test_last(fin.counter, nblk);
  }
  __syncthreads();
  if (*last_flag) jac3_finalize<TB>(partials, nblk, fin, wsum);
}
