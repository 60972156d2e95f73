// cz_k_sums.h -- part of cz_kernels.hip (ONE translation unit per precision; included inside its anonymous namespace after cz_k_common.h):
// the ONE statement of how a launch turns per-thread double sums into a result on the device without a second launch.  Every kernel that
// returns a sum ends through these pieces; the two-launch folds (stencil_k with fin.dst == nullptr, pair_shell_k /
// shell_fold_k, psor_tile_k with reduce_partials_k) hand over at the launch boundary and need none of it.
//
// Hand-off of the per-workgroup partial sums to the workgroup that arrives last (in-kernel finalisation; no extra launch per sweep).
// Why it is sound (MI355X_MICROARCH.md, "Workgroup dispatch, XCD placement & inter-workgroup visibility"; cdna_hip_programming.md G16):
//   producer  lane 0 of every workgroup stores its partials with agent-scope relaxed atomic stores = `global_store ... sc1`: write-through,
//             the bytes leave the XCD's L2 for memory.  `s_waitcnt vmcnt(0)` (inline asm, so that no compiler pass can drop or move it)
//             holds the lane until those stores are acknowledged -- on gfx9 stores are counted in vmcnt -- and only then the lane adds to
//             the agent-scope ticket.  One lane signals for all of its workgroup's handed-off bytes because that lane stored all of them.
//   consumer  the workgroup whose add returned nblk-1 knows every other add, hence every other drain, came before its own.  Its lane 0
//             then executes ONE agent-scope acquire (`buffer_inv sc1`: no line of this CU's L1 survives) and waits for it; the
//             workgroup barrier that follows releases the other waves; all of them read the partials with agent-scope relaxed loads
//             (`sc1`: served from L2 / memory, never from L1).  The acquire costs about 1.7 us once per launch (one workgroup); a
//             release fence in every producer instead cost 27 % of a whole sweep (it writes back the XCD's dirty output lines).
//   The ticket is reset by the finishing workgroup and again at the start of every solve (reset_ticket).
// Called by lane 0 after its partial stores; returns true in the workgroup that must finalise.
__device__ __forceinline__ bool arrive_and_test_last(unsigned* counter, int nblk) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const unsigned ticket = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const bool last = (ticket == (unsigned)nblk - 1u);
  if (last) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  return last;
}

// block_sum for a thread count known only at run time (pcr_lex_wg_k): the same tree, the waves in index order
__device__ __forceinline__ double block_sum_rt(double x, double* wsum, int nwaves) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) wsum[wave] = x;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < nwaves; w++) s += wsum[w];
  return s;  // valid on thread 0
}

// The pieces.  LDS: the caller hands over ONE array `lds` of threads / 64 + 1 doubles: the wave sums of block_sum, and behind them the word
// in which "I am last" travels from thread 0 to the others.  Nothing here declares a __shared__ object (a second object beside a kernel's LDS
// can change how the compiler waits, a static one shifts a dynamic region off its alignment: cdna_hip_programming.md).
// TB: the workgroup's thread count; 0 = known at run time only and passed as `nthreads`.
// ORDER OF THE ADDITIONS, which is part of every caller's contract (the results are compared bit for bit): a thread's own accumulation;
// the wave shuffle tree and the waves in index order (block_sum); in the last workgroup a thread's partials i = t, t + threads, ... of
// every row; what `more` adds; block_sum per row, the rows in index order; what `finish` does with the totals.
template <int TB, int N>
__device__ __forceinline__ void sums_block(const double (&x)[N], double* lds, double (&s)[N], int nthreads = TB) {
#pragma unroll
  for (int n = 0; n < N; n++) {
    if (n > 0) __syncthreads();  // thread 0 has read the wave sums of row n - 1
    if constexpr (TB != 0) s[n] = block_sum<TB>(x[n], lds);
    else s[n] = block_sum_rt(x[n], lds, nthreads >> 6);
  }
}

// one partial, by the lane that will arrive for it (sums_arrive): agent-scope relaxed = write-through
__device__ __forceinline__ void sums_put(double* slot, double v) { __hip_atomic_store(slot, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// All threads: thread 0 puts this workgroup's partials -- row n of the partials starts at partials[n * stride], `me` is this workgroup's
// place in a row, s is valid on thread 0 -- and draws the ticket; true in every thread of the workgroup that arrived last.
__device__ __forceinline__ int* sums_flag(double* lds, int nthreads) { return reinterpret_cast<int*>(lds + (nthreads >> 6)); }
template <int TB, int N>
__device__ __forceinline__ bool sums_arrive(const double (&s)[N], double* partials, int stride, int me, unsigned* counter, int nblk, double* lds) {
  int* last = sums_flag(lds, TB);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int n = 0; n < N; n++) sums_put(&partials[n * stride + me], s[n]);
    *last = arrive_and_test_last(counter, nblk);
  }
  __syncthreads();
  return *last != 0;
}
// ... for a workgroup whose thread 0 has put its partials already, one per column or strip it worked on (psor_col_k, pcr_lex_wg_k)
template <int TB>
__device__ __forceinline__ bool sums_arrive(unsigned* counter, int nblk, double* lds, int nthreads = TB) {
  int* last = sums_flag(lds, nthreads);
  if (threadIdx.x == 0) *last = arrive_and_test_last(counter, nblk);
  __syncthreads();
  return *last != 0;
}

// All threads of the last workgroup: `count` partials per row (one per workgroup, column or strip) in index order, every one an agent-scope
// load; more(x) may add to a thread's sums (SumsNoMore: nothing); the N totals go to finish(tot) on thread 0, and the ticket is reset behind it.
struct SumsNoMore {
  template <int N>
  __device__ __forceinline__ void operator()(double (&)[N]) const {}
};
template <int TB, int N, class MORE, class FINISH>
__device__ __forceinline__ void sums_last(const double* partials, int stride, int count, unsigned* counter, double* lds, MORE more, FINISH finish,
                                          int nthreads = TB) {
  double x[N], tot[N];
#pragma unroll
  for (int n = 0; n < N; n++) x[n] = 0.0;
  for (int i = threadIdx.x; i < count; i += nthreads) {
#pragma unroll
    for (int n = 0; n < N; n++) x[n] += __hip_atomic_load(&partials[n * stride + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  more(x);
  __syncthreads();  // thread 0 has read the wave sums of this workgroup's own partials
  sums_block<TB, N>(x, lds, tot, nthreads);
  if (threadIdx.x == 0) {
    finish(tot);
    *counter = 0u;
  }
}

// All threads of a launch whose every workgroup has one partial per row: block sums, puts and ticket, and in the last workgroup sums_last.
// WHERE says which place of how many the workgroup takes in a row of the partials.
struct SumsGrid1 {  // a one-dimensional grid
  __device__ __forceinline__ int n() const { return gridDim.x; }
  __device__ __forceinline__ int me() const { return blockIdx.x; }
};
struct SumsGrid2 {  // a two-dimensional grid, x fastest
  __device__ __forceinline__ int n() const { return gridDim.x * gridDim.y; }
  __device__ __forceinline__ int me() const { return blockIdx.y * gridDim.x + blockIdx.x; }
};
struct SumsAt {  // a place the caller has worked out
  int me_, n_;
  __device__ __forceinline__ int n() const { return n_; }
  __device__ __forceinline__ int me() const { return me_; }
};
template <int TB, int N, class WHERE, class MORE, class FINISH>
__device__ __forceinline__ void sums_finish(const double (&acc)[N], double* partials, WHERE where, unsigned* counter, double* lds, MORE more, FINISH finish) {
  double s[N];
  sums_block<TB, N>(acc, lds, s);
  const int nblk = where.n();
  const int me = where.me();
  if (sums_arrive<TB>(s, partials, nblk, me, counter, nblk, lds)) sums_last<TB, N>(partials, nblk, nblk, counter, lds, more, finish);
}
// ... the regular case: a two-dimensional grid, nothing more
template <int TB, int N, class FINISH>
__device__ __forceinline__ void sums_finish(const double (&acc)[N], double* partials, unsigned* counter, double* lds, FINISH finish) {
  sums_finish<TB>(acc, partials, SumsGrid2{}, counter, lds, SumsNoMore{}, finish);
}
