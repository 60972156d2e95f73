// cz_k_jac3.h -- part of cz_kernels.hip (ONE translation unit per precision; included inside its anonymous namespace after cz_k_rb4.h):
// jac3_k, THREE relaxed-Jacobi sweeps (cz_solver.f90:334-351 three times) per pass over memory.  Single-domain runs, constant coefficients.
// ------------------------------------------------------------------------------------------------------------
// Why: the two-sweep pass (jacobi2p_k) moves 1.11 x the bytes of one fused pass at 0.88 of the copy ceiling (profiles/hbm_traffic.json), so
// the only lever left on a large Jacobi solve is fewer bytes per sweep.  On the frame of cz_k_pass.h (work item, addresses, masks, outer rows, masked
// store, epilogue); the arrangement is rb4_k's (cz_k_rb4.h) one stage shorter:
//     fields      u on E3 = own segment +- 3 rows, f1 (after sweep n+1) on E2, f2 (after sweep n+2) on E1, f3 = output on the segment
//     threads     one per vector of E2 (TB = LV = S + 4R), dealt in order (x = t): a Jacobi stage has no colour, so rows need no dealing by parity
//     stages      1 on all of E2; 2 on the waves that hold a vector of E1; 3 on the waves that own a vector (wave-uniform branches: the waves at
//                 the ends of E2 skip what no valid point reads)
//     LDS         u: 2 x (LV + 2R), f1, f2: 2 x LV each (by plane parity; the j-1 operand of a vector is read by the thread that wrote it)
//     k windows   KT vectors + hv halo vectors per side; three stages reach 3 elements beyond a window: hv = 1 (FP32), 2 (FP64)
//     planes      stage s at step q works on plane q - s + 1: f1(q) from u(q-1..q+1), f2(q-1) from f1, f3(q-2) -> W
//     in flight   step q requests u(q+2) and b(q+1) of its own vector first of all, and -- only the waves that hold a thread of the outer
//                 rows, after stage 1 -- the outer rows of u(q+2).  Nothing in step q waits for them: all three are first used in step
//                 q+1, behind barrier q (u(q+2) as the j+1 operand and b(q+1) in stage 1; the outer rows are written to LDS after stage 1,
//                 into the outer slots [0, R) and [LV + R, LV + 2R) of the buffer of u(q+2).  That buffer is step q+1's `prv` buffer, read
//                 at [R, R + LV) only; its outer slots were last read in step q and are next read in step q+2).  The prologue primes the
//                 outer rows of two planes.  The store of W(q-2) is younger than the requests of step q: the wait for b(q+1) in step q+1
//                 retires it as well (gfx9 counts loads and stores in one counter, in order).  profiles/r20/jac3_requests_in_flight.txt
//     LDS in flight  a stage is `fetch` (its six LDS reads: centre, j-1, j+1, the plane before, the two k edges) and `relax` (lane shifts and
//                 relax_vec).  Behind barrier q - 1 a step issues stage 1's six reads and then stage 2's six (f1 of earlier planes: published
//                 before that barrier), then computes stage 1; behind the outer-row block it issues stage 3's six (f2 of earlier planes) and
//                 then computes stages 2 and 3.  So the round trip of stage s + 1's operands runs under stage s's arithmetic instead of in
//                 front of its own.  The ORDER matters: LDS returns in order and lgkmcnt counts in order, so a stage's wait for its last
//                 operand retires everything issued before that operand.  All six reads of a stage, the edge reads included, therefore
//                 stand in front of every read of the next (reads_stay_in_order: the compiler put stage 1's edge reads behind stage 2's
//                 vector reads otherwise), and the fetches are unconditional: behind a wave-uniform `if (wave2)` the compiler counts the
//                 waits of stage 1 for the path with the fewer reads outstanding, which retires stage 2's reads on the other.  A wave
//                 that skips stage 2 or 3 thus requests operands it never uses, from addresses no stage that runs would read in its lanes:
//                 F1 + x +- R for x outside [R, LV - R) and F2 + x +- R for x outside the owned range reach at most R vectors below a
//                 field buffer -- into the u buffers or f1 -- or R vectors beyond the last one, the padding deep_lds puts behind it (and in
//                 front of the first u buffer): inside the allocation.  Buffers, parities, the publish and the barrier are unchanged; the
//                 second set of operands costs 15-16 VGPRs (122-123 FP32, 127-128 FP64, no scratch).  profiles/r25/jac3_operands_ahead.txt
// Per point: relax_vec<V, UNIT> with the hoisted IEEE division (or its checked shorter form, MED), the operations of jacobi2p_k on the same
// values => the same bits as three single sweeps.  The three residuals (sum dp^2 of sweeps n+1, n+2, n+3) are produced and finalised in the kernel; if the first or the second
// converges, the driver re-runs one sweep or one pair from the untouched input (out of place, like the pair).
// ------------------------------------------------------------------------------------------------------------

// The three helpers below are empty asm statements that pin what the compiler makes of the inner step (scalar-base requests, no wait on a
// step's requests before its barrier); reads_stay_in_order further down pins the order of the LDS reads.  They change no value.  What they
// achieve depends on the compiler: the listing of the inner step in profiles/r25/jac3_operands_ahead.txt (global requests, LDS reads and
// writes, vmcnt and lgkmcnt waits, gate branches, barriers, registers) is the contract to compare against after a change of the toolchain;
// tests cannot see it.
// A plane pointer the compiler must take as it stands: global memory, in a scalar register pair.
template <class T>
__device__ __forceinline__ T* uniform_global(T* p) {
  auto g = (__attribute__((address_space(1))) T*)p;
  asm("" : "+s"(g));
  return (T*)g;
}

// ... and the 32-bit lane offset that goes with it, widened where it is used and not once in front of the loop.
__device__ __forceinline__ unsigned lane_offset(unsigned o) {
  asm("" : "+v"(o));
  return o;
}

// A value that has to be complete at this place of the code: what is computed from it comes after, what it is computed from before.
template <int V>
__device__ __forceinline__ void complete_here(Vec<V>& x) {
  static_assert(V == 2 || V == 4, "one constraint per component");
  if constexpr (V == 4) asm volatile("" : "+v"(x.v[0]), "+v"(x.v[1]), "+v"(x.v[2]), "+v"(x.v[3]));
  else asm volatile("" : "+v"(x.v[0]), "+v"(x.v[1]));
}

// A stage's six LDS operands between their request and their use.  lds_request is the read alone, lds_whole the constraint of lds_ld
// (cz_k_pass.h) on the value that came back: together they are lds_ld, apart they let other work stand between the two.
template <int V>
struct LdsOperands {
  typename NatVec<V>::type pc, im, ip, pm;  // centre, j-1 row, j+1 row of the current plane; centre of the plane before
  REAL elo, ehi;                            // the k neighbours beyond the wave's first and last vector
};
template <int V>
__device__ __forceinline__ typename NatVec<V>::type lds_request(const Vec<V>* p) {
  return *reinterpret_cast<const typename NatVec<V>::type*>(p);
}
template <int V>
__device__ __forceinline__ Vec<V> lds_whole(typename NatVec<V>::type x) {
  asm("" : "+v"(x));  // (as in lds_ld: whole, in consecutive registers -- one ds_read_b128)
  Vec<V> r;
  __builtin_memcpy(&r, &x, sizeof(r));
  return r;
}

// Nothing is scheduled across this place: the LDS reads in front of it are issued before the ones behind it.  LDS returns in order and
// lgkmcnt counts in order, so a stage's wait for its own last operand retires every read issued before that operand -- it must not be a
// read of the next stage.
__device__ __forceinline__ void reads_stay_in_order() { __builtin_amdgcn_sched_barrier(0); }

// A stage of jac3_k and jac4_k in two parts.  jac_fetch requests its six LDS operands -- centre, j-1, j+1, the plane before, and the k
// neighbours beyond the wave's first and last vector (x_first, x_last: one element each, the same address in all lanes) -- and uses none of
// them; jac_relax takes them whole (lds_whole) and does the arithmetic.  What a step puts between the two is what the round trip hides behind.
template <int V>
__device__ __forceinline__ LdsOperands<V> jac_fetch(const Vec<V>* cur, const Vec<V>* prv, int x, int R, int x_first, int x_last) {
  LdsOperands<V> o;
  o.pc = lds_request<V>(cur + x);
  o.im = lds_request<V>(cur + x - R);
  o.ip = lds_request<V>(cur + x + R);
  o.pm = lds_request<V>(prv + x);
  o.elo = reinterpret_cast<const REAL*>(cur)[(long long)x_first * V - 1];
  o.ehi = reinterpret_cast<const REAL*>(cur)[(long long)(x_last + 1) * V];
  return o;
}
template <int V, int UNIT, class DIV>
__device__ __forceinline__ Vec<V> jac_relax(const LdsOperands<V>& o, const Vec<V>& nxt, const Vec<V>& bb, const Coef& c, const DIV& dv,
                                            unsigned msk, unsigned cnt, double& acc) {
  const Vec<V> pc = lds_whole<V>(o.pc);
  const Vec<V> im = lds_whole<V>(o.im);
  const Vec<V> ip = lds_whole<V>(o.ip);
  const Vec<V> pm = lds_whole<V>(o.pm);
  const REAL kl = lane_shr1(o.elo, pc.v[V - 1]);
  const REAL kr = lane_shl1(o.ehi, pc.v[0]);
  return relax_vec<V, UNIT>(pc, im, ip, pm, nxt, kl, kr, bb, c, dv, msk, cnt, acc);
}

// The division policy of both kernels:
// MED = 1 (FP32): the division with one correction step (mediumdiv, cz_k_fastdiv.h), taken only for a divisor that passed the exhaustive
// comparison with `n / d` on this context (jac3_medium, cz_h_launch.h)
// GATE = 1: that division (medium or hoisted, by MED) in its gated form (GatedDiv, cz_k_pass.h): whether a numerator is huge is tested once per
// vector and wave instead of at every point.  Taken only for a divisor that passed its comparison on this context (jac3_gated, cz_h_launch.h).
// What the compiler has to make of it -- the tail without den_s a block of its own in the inner step -- is part of the listing in
// profiles/r23/jac3_gated_division.txt.
template <int MED, int GATE>
using JacDiv = typename std::conditional<GATE != 0, GatedDiv<MED>, typename std::conditional<MED != 0, MediumDiv, HoistedDiv>::type>::type;

template <int V, int TB, int UNIT, int MED, int GATE = 0>
__global__ void __launch_bounds__(TB, 1)
jac3_k(const REAL* __restrict__ U, const REAL* __restrict__ B, REAL* __restrict__ W, Coef c, Geom2 g, double* partials,
       const int* __restrict__ skip, Fin2 fin) {
  if (skip != nullptr && *skip != 0) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int t = threadIdx.x;
  const int R = g.R;
  constexpr int LV = TB;  // E2: own segment +- two rows (S = LV - 4R); one vector per thread; u on E3
  const DeepLds<V> lds = deep_lds<V, LV, 3>(smem, R);
  const int LU = lds.LU;
  Vec<V>* ldsU = lds.U;
  Vec<V>* ldsF = lds.F;
  double* wsum = lds.wsum;

  const PassItem it = pass_item<V>(g);
  const int ja = it.ja, jb = it.jb;

  double acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
  const JacDiv<MED, GATE> dv{fastdiv_init(c.dd)};

  if (it.work) {
    const long long e2_0 = it.fb - 2 * (long long)R;  // first vector of E2
    const size_t PB = (size_t)g.PSB;
    const RowView<V> rv = row_view<V>(g, it);
    const int x = t;  // this thread's vector: index in E2
    const long long f = e2_0 + x;
    unsigned bo = rv.off_of(f);  // (not const: the inner steps pass it through `lane_offset`)
    const VecMask mk = vec_mask<V>(g, it, f);
    const unsigned inbox = mk.rows ? mk.bits : 0u;                                                     // components inside the inner box (every stage updates only those)
    const unsigned own = (x >= 2 * R && x < LV - 2 * R && mk.rows && mk.kown) ? mk.bits : 0u;  // ... of a vector this workgroup owns (stores, residual counts)
    // wave-uniform: does this wave hold a vector of E1 (stage 2) / an owned vector (stage 3)?
    const bool wave2 = __builtin_amdgcn_ballot_w64(x >= R && x < LV - R) != 0ull;
    const bool wave3 = __builtin_amdgcn_ballot_w64(own != 0) != 0ull;
    OuterRow h = outer_row<V, TB>(rv, LV, it.fb - 3 * (long long)R, f);  // the outer rows of E3
    const bool waveh = __builtin_amdgcn_ballot_w64(h.has) != 0ull;                // wave-uniform: does this wave stage a vector of them?
    const char* Ub = reinterpret_cast<const char*>(U);
    const char* Bb = reinterpret_cast<const char*>(B);
    char* Wb = reinterpret_cast<char*>(W);

    // ---- prologue: the first step is q0 = ja - 2 (stage 1 on plane ja - 2): LDS u(q0 - 1) own, u(q0) on E3; in flight u(q0 + 1) with its
    // outer rows (hx), b(q0)
    const int q0 = ja - 2;
    Vec<V> uA, uB, bA, bB, hx = zerov<V>();
    {
      const Vec<V> t2 = ld16<V>(Ub + (size_t)rv.pl(q0 - 1) * PB, rv.lim(bo, rv.pl(q0 - 1)));
      const Vec<V> t1 = ld16<V>(Ub + (size_t)rv.pl(q0) * PB, rv.lim(bo, rv.pl(q0)));
      Vec<V> h1 = zerov<V>();
      if (waveh) {
        h1 = ld16<V>(Ub + (size_t)rv.pl(q0) * PB, rv.lim(h.bo, rv.pl(q0)));
        hx = ld16<V>(Ub + (size_t)rv.pl(q0 + 1) * PB, rv.lim(h.bo, rv.pl(q0 + 1)));
      }
      uA = ld16<V>(Ub + (size_t)rv.pl(q0 + 1) * PB, rv.lim(bo, rv.pl(q0 + 1)));
      bA = ld16<V>(Bb + (size_t)rv.pl(q0) * PB, rv.lim(bo, rv.pl(q0)));
      ldsU[(size_t)((q0 - 1) & 1) * LU + R + x] = t2;
      ldsU[(size_t)(q0 & 1) * LU + R + x] = t1;
      if (h.has) ldsU[(size_t)(q0 & 1) * LU + h.hl] = h1;
    }
    Vec<V> bq1 = zerov<V>(), bq2 = zerov<V>();  // b of the planes of stages 2, 3
    __syncthreads();

    // the k neighbours beyond the wave's first and last vector come from LDS (one element each, the same address in all lanes)
    const int x_first = __builtin_amdgcn_readfirstlane(x), x_last = __builtin_amdgcn_readlane(x, 63);
    // a stage in two parts (jac_fetch, jac_relax) with this thread's vector, row length, coefficients and division
    auto fetch = [&](const Vec<V>* cur, const Vec<V>* prv) __attribute__((always_inline)) { return jac_fetch<V>(cur, prv, x, R, x_first, x_last); };
    auto relax = [&](const LdsOperands<V>& o, const Vec<V>& nxt, const Vec<V>& bb, unsigned msk, unsigned cnt, double& acc)
                     __attribute__((always_inline)) { return jac_relax<V, UNIT>(o, nxt, bb, c, dv, msk, cnt, acc); };

    // One plane step q.  uc = u(q+1), its outer rows hx and b1 = b(q) were requested one step ago; un / bn / hx receive this step's requests
    // (u(q+2), b(q+1), the outer rows of u(q+2)).  b2 = b(q-1), b3 = b(q-2): the right-hand sides of stages 2 and 3.
    // Two forms.  The general one clamps every requested plane, tests it for the array's last plane and gates every stage by its plane.  The
    // INNER one is for the steps on which none of that acts -- q - 2 >= ja and q <= jb, so all three stages work on planes of the chunk, and
    // q + 2 <= jlast - 1, so no request is clamped or touches the last plane: the plane addresses are pointers carried from step to step
    // (uN = u(q+2), bN = b(q+1), wN = w(q-2)), the masks are `inbox` and `own` as they stand.  Same loads from the same addresses, same
    // masks => the same bits; what goes is the scalar work per request (clamps, a 64-bit product, the last-plane test and its selects on the
    // load offsets) and per stage (plane gates): 5-6 % of the kernel at 512^3, profiles/r19/jac3_step_instructions.txt.
    const char* uN = Ub;
    const char* bN = Bb;
    char* wN = Wb;
    auto step = [&](auto inner, const int q, Vec<V>& uc, Vec<V>& un, Vec<V>& b1, Vec<V>& bn, Vec<V>& b2, Vec<V>& b3) __attribute__((always_inline)) {
      constexpr bool INNER = decltype(inner)::value;
      const char *up, *bp;  // the planes u(q+2) and b(q+1) of this step's requests, and the lane offsets into them
      unsigned uo, bo1, ho;
      if constexpr (INNER) {
        uN = uniform_global(uN), bN = uniform_global(bN), wN = uniform_global(wN);
        bo = lane_offset(bo), h.bo = lane_offset(h.bo);
        up = uN, bp = bN, uo = bo, bo1 = bo, ho = h.bo;
      } else {
        const int qu = rv.pl(q + 2 <= jb + 3 ? q + 2 : jb + 3), qb = rv.pl(q + 1 <= jb + 2 ? q + 1 : jb + 2);
        up = Ub + (size_t)qu * PB, bp = Bb + (size_t)qb * PB;
        uo = rv.lim(bo, qu), bo1 = rv.lim(bo, qb), ho = rv.lim(h.bo, qu);
      }
      un = ld16<V>(up, uo);
      bn = ld16<V>(bp, bo1);
      // planes of the three stages; masks: inside the inner box a stage updates, inside the chunk the owner counts the residual
      const int p1 = q, p2 = q - 1, p3 = q - 2;
      auto upd = [&](int p) -> unsigned { return (INNER || (p >= g.jj0 && p <= g.jj1)) ? inbox : 0u; };
      auto cnt = [&](int p) -> unsigned { return (INNER || (p >= ja && p <= jb)) ? own : 0u; };
      const Vec<V>* cU = ldsU + (size_t)(p1 & 1) * LU + R;  // u(p1) in E2 coordinates (index x)
      const Vec<V>* pU = ldsU + (size_t)((p1 - 1) & 1) * LU + R;
      Vec<V>* F1 = ldsF;
      Vec<V>* F2 = ldsF + (size_t)2 * LV;
      const bool run3 = (INNER || p3 >= ja) && wave3;
      // ---- the LDS operands of stage 1 and, behind ALL six of them, those of stage 2 (f1 of earlier planes: published before barrier q - 1)
      const LdsOperands<V> o1 = fetch(cU, pU);
      reads_stay_in_order();
      // Every wave requests them, also one that skips the stage (see "LDS in flight" above): a branch here would merge two counts of
      // outstanding reads in front of stage 1's waits, and the compiler waits for the smaller one -- which retires these reads.
      const LdsOperands<V> o2 = fetch(F1 + (size_t)(p2 & 1) * LV, F1 + (size_t)((p2 - 1) & 1) * LV);
      reads_stay_in_order();
      // ---- stage 1: f1(p1) on every vector of E2
      Vec<V> v1 = relax(o1, uc, b1, upd(p1), cnt(p1), acc1);
      complete_here<V>(v1);
      // ---- the outer rows of u(q+1), requested one step ago (they landed with uc): into the buffer of u(q+1), this step's `prv` buffer, which
      // is read at [R, R + LV) only; then the request of those of u(q+2)
      if (waveh) {
        if (h.has) ldsU[(size_t)((p1 + 1) & 1) * LU + h.hl] = hx;
        hx = ld16<V>(up, ho);
      }
      // ---- the LDS operands of stage 3 (f2 of earlier planes), in front of stage 2's arithmetic
      const LdsOperands<V> o3 = fetch(F2 + (size_t)(p3 & 1) * LV, F2 + (size_t)((p3 - 1) & 1) * LV);
      reads_stay_in_order();
      // ---- stage 2: f2(p2) from f1(p2 - 1) [LDS], f1(p2) [LDS], f1(p1) [v1]
      Vec<V> v2 = v1;  // (a wave outside E1 publishes a value no valid point reads)
      if (wave2) v2 = relax(o2, v1, b2, upd(p2), cnt(p2), acc2);
      // ---- stage 3: f3(p3) = the output, owned vectors of the chunk's planes.  Whole waves: the k neighbours travel by lane shifts, and the
      // lane next to the first owned vector of a window holds a halo vector -- it owns nothing but must take part.
      if (run3) {
        const Vec<V> o = relax(o3, v2, b3, own, own, acc3);
        store_owned<V>(INNER ? wN : Wb + (size_t)p3 * PB, bo, own, o);
      }
      // ---- publish: f1(p1), f2(p2) and the next u centre plane u(q+1) (its outer rows were written behind stage 1)
      F1[(size_t)(p1 & 1) * LV + x] = v1;
      F2[(size_t)(p2 & 1) * LV + x] = v2;
      Vec<V>* nU = ldsU + (size_t)((p1 + 1) & 1) * LU;
      nU[R + x] = uc;
      if constexpr (!INNER) b3 = b2, b2 = b1;  // (b1 is complete: stage 1 used it; the inner steps rotate the four sets by name)
      if constexpr (INNER) uN += PB, bN += PB, wN += PB;
      __syncthreads();
    };
    // (stage s first matters at plane ja - (3 - s), which it reaches at step ja - 2 + (s - 1): every field buffer a valid point reads was
    // written by a step of this loop)
    // The march, steps q0 = ja - 2 .. jb + 2, in three parts:
    //   phase 0   q0 .. ja + 1: the four steps that fill the pipeline, general form.  Always four (ja <= jb, so ja + 1 < jb + 2): two A/B pairs,
    //             so uA / bA hold the pending requests again when it ends, at q = ja + 2
    //   inner     q = ja + 2 .. qi in groups of four, while a whole group fits (q + 3 <= qi); none for chunks of fewer than six planes.  Four,
    //             because b lives for three steps (stages 1, 2, 3) plus the step that requests it: the four register sets bA, bB, bq1, bq2
    //             rotate BY NAME and are back in place after four steps, the two u sets after every two.  (In A/B pairs the b sets rotated
    //             by copies, which the compiler put at the loop head, in front of a wait for everything outstanding.)
    //   phase 1   from where the inner steps stopped to jb + 2, general form (it rotates b by copies): at least jb + 1 and jb + 2, and in front
    //             of them the steps up to jb that no whole group of four took -- up to three.  Where the chunk ends at the array's last inner
    //             plane (jb = jlast - 2) the inner form ends one step earlier, qi = jlast - 3 = jb - 1: step jb requests the array's last
    //             plane and takes the general form in any case, and the up to three left-over steps lie in front of it
    // The general loop is ONE copy in the code, run once per phase (nounroll: two copies would cost code size for nothing).
    const int qi = jb < g.jlast - 3 ? jb : g.jlast - 3;  // the last step that may take the inner form: q <= jb and q + 2 <= jlast - 1
    int q = q0;
#pragma nounroll
    for (int phase = 0; phase < 2; phase++) {
      const int qg = phase == 0 ? ja + 1 : jb + 2;
      for (;;) {
        step(std::false_type{}, q, uA, uB, bA, bB, bq1, bq2);
        if (++q > qg) break;
        step(std::false_type{}, q, uB, uA, bB, bA, bq1, bq2);
        if (++q > qg) break;
      }
      if (phase == 0) {  // (q = ja + 2: an even number of steps lies behind, uA / bA hold the requests again, bq1 / bq2 = b(q-1), b(q-2))
        uN = Ub + (size_t)(q + 2) * PB, bN = Bb + (size_t)(q + 1) * PB, wN = Wb + (size_t)(q - 2) * PB;  // (q - 2 = ja: inside the array)
        for (; q + 3 <= qi; q += 4) {
          step(std::true_type{}, q, uA, uB, bA, bB, bq1, bq2);
          step(std::true_type{}, q + 1, uB, uA, bB, bq2, bA, bq1);
          step(std::true_type{}, q + 2, uA, uB, bq2, bq1, bB, bA);
          step(std::true_type{}, q + 3, uB, uA, bq1, bA, bq2, bB);
        }
      }
    }
  }

  // ---- residuals of the three sweeps: per-workgroup partials, finalised by the last workgroup
  const double acc[3] = {acc1, acc2, acc3};
  pass_epilogue<TB, 3>(acc, partials, fin, wsum);
}
