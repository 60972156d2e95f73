// cz_k_jac4.h -- part of cz_kernels.hip (ONE translation unit per precision; included inside its anonymous namespace after cz_k_jac3.h):
// jac4_k, FOUR relaxed-Jacobi sweeps (cz_solver.f90:334-351 four times) per pass over memory.  Single-domain runs, constant coefficients.
// ------------------------------------------------------------------------------------------------------------
// Why: jac3_k (cz_k_jac3.h) runs at the streaming ceiling of this project's kernels, so the argument of its head applies one stage further:
// fewer bytes per sweep.  On the frame of cz_k_pass.h; the arrangement is jac3_k's one stage deeper (rb4_k's frame, cz_k_rb4.h):
//     fields      u on E4 = own segment +- 4 rows, f1 on E3, f2 on E2, f3 on E1, f4 = output on the segment
//     threads     one per vector of E3 (TB = LV = S + 6R), dealt in order (x = t)
//     stages      1 on all of E3; 2, 3 on the waves that hold a vector of E2, E1; 4 on the waves that own a vector (wave-uniform branches)
//     LDS         u: 2 x (LV + 2R), f1, f2, f3: 2 x LV each (by plane parity)          = 134 KB for R = 28
//     k windows   KT vectors + hv halo vectors per side; four stages reach 4 elements beyond a window: hv = 1 (FP32), 2 (FP64)
//     planes      stage s at step q works on plane q - s + 1: f1(q) from u(q-1..q+1), f2(q-1) from f1, f3(q-2) from f2, f4(q-3) -> W
//     in flight   as in jac3_k: step q requests u(q+2), b(q+1) and (behind stage 1, the waves of the outer rows) the outer rows of u(q+2);
//                 nothing in step q waits for them
//     LDS reads   a stage is `fetch` (its six LDS reads) and `relax`, as in jac3_k, but a stage's reads stand directly in front of its own
//                 arithmetic: requesting the next stage's operands one stage early (jac3_k's "LDS in flight") needs 72-136 bytes of
//                 scratch per lane here and is NOT built (profiles/r26/jac4_four_sweeps_per_pass.txt).  Every fetch is unconditional --
//                 a wave that skips a stage reads addresses inside the allocation that it never uses, as in jac3_k.
// Per point: relax_vec<V, UNIT> with the division policies of jac3_k => the same bits as four single sweeps.  The four residuals are produced
// and finalised in the kernel, in order, with a stop at the first that converged; the input is never modified, so the driver can re-run one,
// two or three sweeps from it.
// ------------------------------------------------------------------------------------------------------------
template <int V, int TB, int UNIT, int MED, int GATE = 0>
__global__ void __launch_bounds__(TB, 1)
jac4_k(const REAL* __restrict__ U, const REAL* __restrict__ B, REAL* __restrict__ W, Coef c, Geom2 g, double* partials,
       const int* __restrict__ skip, Fin2 fin) {
  if (skip != nullptr && *skip != 0) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int t = threadIdx.x;
  const int R = g.R;
  constexpr int LV = TB;  // E3: own segment +- three rows (S = LV - 6R); one vector per thread; u on E4
  const DeepLds<V> lds = deep_lds<V, LV, 4>(smem, R);
  const int LU = lds.LU;
  Vec<V>* ldsU = lds.U;
  Vec<V>* ldsF = lds.F;
  double* wsum = lds.wsum;

  const PassItem it = pass_item<V>(g);
  const int ja = it.ja, jb = it.jb;

  double acc1 = 0.0, acc2 = 0.0, acc3 = 0.0, acc4 = 0.0;
  const JacDiv<MED, GATE> dv{fastdiv_init(c.dd)};

  if (it.work) {
    const long long e3_0 = it.fb - 3 * (long long)R;  // first vector of E3
    const size_t PB = (size_t)g.PSB;
    const RowView<V> rv = row_view<V>(g, it);
    const int x = t;  // this thread's vector: index in E3
    const long long f = e3_0 + x;
    unsigned bo = rv.off_of(f);  // (not const: the inner steps pass it through `lane_offset`)
    const VecMask mk = vec_mask<V>(g, it, f);
    const unsigned inbox = mk.rows ? mk.bits : 0u;                                             // components inside the inner box (every stage updates only those)
    const unsigned own = (x >= 3 * R && x < LV - 3 * R && mk.rows && mk.kown) ? mk.bits : 0u;  // ... of a vector this workgroup owns (stores, residual counts)
    // wave-uniform: does this wave hold a vector of E2 (stage 2) / of E1 (stage 3) / an owned vector (stage 4)?
    const bool wave2 = __builtin_amdgcn_ballot_w64(x >= R && x < LV - R) != 0ull;
    const bool wave3 = __builtin_amdgcn_ballot_w64(x >= 2 * R && x < LV - 2 * R) != 0ull;
    const bool wave4 = __builtin_amdgcn_ballot_w64(own != 0) != 0ull;
    OuterRow h = outer_row<V, TB>(rv, LV, it.fb - 4 * (long long)R, f);  // the outer rows of E4
    const bool waveh = __builtin_amdgcn_ballot_w64(h.has) != 0ull;      // wave-uniform: does this wave stage a vector of them?
    const char* Ub = reinterpret_cast<const char*>(U);
    const char* Bb = reinterpret_cast<const char*>(B);
    char* Wb = reinterpret_cast<char*>(W);

    // ---- prologue: the first step is q0 = ja - 3 (stage 1 on plane ja - 3): LDS u(q0 - 1) own, u(q0) on E4; in flight u(q0 + 1) with its
    // outer rows (hx), b(q0)
    const int q0 = ja - 3;
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
    Vec<V> bq1 = zerov<V>(), bq2 = zerov<V>(), bq3 = zerov<V>();  // b of the planes of stages 2, 3, 4
    __syncthreads();

    // the k neighbours beyond the wave's first and last vector come from LDS (one element each, the same address in all lanes)
    const int x_first = __builtin_amdgcn_readfirstlane(x), x_last = __builtin_amdgcn_readlane(x, 63);
    auto fetch = [&](const Vec<V>* cur, const Vec<V>* prv) __attribute__((always_inline)) { return jac_fetch<V>(cur, prv, x, R, x_first, x_last); };
    auto relax = [&](const LdsOperands<V>& o, const Vec<V>& nxt, const Vec<V>& bb, unsigned msk, unsigned cnt, double& acc)
                     __attribute__((always_inline)) { return jac_relax<V, UNIT>(o, nxt, bb, c, dv, msk, cnt, acc); };

    // One plane step q.  uc = u(q+1), its outer rows hx and b1 = b(q) were requested one step ago; un / bn / hx receive this step's requests
    // (u(q+2), b(q+1), the outer rows of u(q+2)).  b2 = b(q-1), b3 = b(q-2), b4 = b(q-3): the right-hand sides of stages 2, 3 and 4.
    // Two forms, as in jac3_k: the general one clamps every requested plane and gates every stage by its plane; the INNER one is for the steps
    // with q - 3 >= ja, q <= jb and q + 2 <= jlast - 1, where none of that acts: carried plane pointers (uN = u(q+2), bN = b(q+1),
    // wN = w(q-3)), the masks `inbox` and `own` as they stand.
    const char* uN = Ub;
    const char* bN = Bb;
    char* wN = Wb;
    auto step = [&](auto inner, const int q, Vec<V>& uc, Vec<V>& un, Vec<V>& b1, Vec<V>& bn, Vec<V>& b2, Vec<V>& b3, Vec<V>& b4) __attribute__((always_inline)) {
      constexpr int PAR = decltype(inner)::value;  // the parity of q where the step is an inner one, -1 for the general form
      constexpr bool INNER = PAR >= 0;
      const char *up, *bp;
      unsigned uo, bo1, ho;
      if constexpr (INNER) {
        uN = uniform_global(uN), bN = uniform_global(bN), wN = uniform_global(wN);
        bo = lane_offset(bo), h.bo = lane_offset(h.bo);
        up = uN, bp = bN, uo = bo, bo1 = bo, ho = h.bo;
      } else {
        const int qu = rv.pl(q + 2 <= jb + 4 ? q + 2 : jb + 4), qb = rv.pl(q + 1 <= jb + 3 ? q + 1 : jb + 3);
        up = Ub + (size_t)qu * PB, bp = Bb + (size_t)qb * PB;
        uo = rv.lim(bo, qu), bo1 = rv.lim(bo, qb), ho = rv.lim(h.bo, qu);
      }
      un = ld16<V>(up, uo);
      bn = ld16<V>(bp, bo1);
      // planes of the four stages; masks: inside the inner box a stage updates, inside the chunk the owner counts the residual
      const int p1 = q, p2 = q - 1, p3 = q - 2, p4 = q - 3;
      // LDS buffer (plane parity) of p1 and p3, and of p2 and p4: constants in the inner steps, which start at an even q -- the operand
      // addresses are then a few bases with constant offsets instead of one register per stage, operand and parity
      const int ev = INNER ? PAR : (q & 1), od = ev ^ 1;
      auto upd = [&](int p) -> unsigned { return (INNER || (p >= g.jj0 && p <= g.jj1)) ? inbox : 0u; };
      auto cnt = [&](int p) -> unsigned { return (INNER || (p >= ja && p <= jb)) ? own : 0u; };
      const Vec<V>* cU = ldsU + (size_t)ev * LU + R;  // u(p1) in E3 coordinates (index x)
      const Vec<V>* pU = ldsU + (size_t)od * LU + R;
      Vec<V>* F1 = ldsF;
      Vec<V>* F2 = ldsF + (size_t)2 * LV;
      Vec<V>* F3 = ldsF + (size_t)4 * LV;
      const bool run4 = (INNER || p4 >= ja) && wave4;
      auto fetch2 = [&]() __attribute__((always_inline)) { return fetch(F1 + (size_t)od * LV, F1 + (size_t)ev * LV); };
      auto fetch3 = [&]() __attribute__((always_inline)) { return fetch(F2 + (size_t)ev * LV, F2 + (size_t)od * LV); };
      auto fetch4 = [&]() __attribute__((always_inline)) { return fetch(F3 + (size_t)od * LV, F3 + (size_t)ev * LV); };
      // ---- the LDS operands of stage 1
      const LdsOperands<V> o1 = fetch(cU, pU);
      reads_stay_in_order();
      // ---- stage 1: f1(p1) on every vector of E3
      Vec<V> v1 = relax(o1, uc, b1, upd(p1), cnt(p1), acc1);
      complete_here<V>(v1);
      // ---- publish the next u centre plane u(q+1): its buffer is this step's `prv` buffer of stage 1, read at a thread's own vector only,
      // and stage 1 is done with it.  Then its outer rows, requested one step ago, and the request of those of u(q+2).
      // (Every value is published as soon as its last reader in this thread is through -- uc behind stage 1, f(s) behind stage s + 1 --
      // and not at the end of the step: at most one stage value is live beside a stage's operands, which is what lets four stages fit
      // into 128 registers.  The buffer a value goes to is the `prv` buffer of the stage just computed: other threads read a `prv`
      // buffer nowhere, this thread's own read of it has been consumed.)
      Vec<V>* nU = ldsU + (size_t)od * LU;
      nU[R + x] = uc;
      if (waveh) {
        if (h.has) nU[h.hl] = hx;
        hx = ld16<V>(up, ho);
      }
      const LdsOperands<V> o2 = fetch2();  // (every wave requests them, also one that skips the stage)
      reads_stay_in_order();
      // ---- stage 2: f2(p2) from f1(p2 - 1) [LDS], f1(p2) [LDS], f1(p1) [v1]
      Vec<V> v2 = v1;  // (a wave outside E2 publishes a value no valid point reads)
      if (wave2) v2 = relax(o2, v1, b2, upd(p2), cnt(p2), acc2);
      complete_here<V>(v2);
      F1[(size_t)ev * LV + x] = v1;
      const LdsOperands<V> o3 = fetch3();
      reads_stay_in_order();
      // ---- stage 3: f3(p3) from f2
      Vec<V> v3 = v2;
      if (wave3) v3 = relax(o3, v2, b3, upd(p3), cnt(p3), acc3);
      complete_here<V>(v3);
      F2[(size_t)od * LV + x] = v2;
      const LdsOperands<V> o4 = fetch4();
      reads_stay_in_order();
      // ---- stage 4: f4(p4) = the output, owned vectors of the chunk's planes.  Whole waves: the k neighbours travel by lane shifts, and the
      // lane next to the first owned vector of a window holds a halo vector -- it owns nothing but must take part.
      if (run4) {
        const Vec<V> o = relax(o4, v3, b4, own, own, acc4);
        store_owned<V>(INNER ? wN : Wb + (size_t)p4 * PB, bo, own, o);
      }
      F3[(size_t)ev * LV + x] = v3;
      if constexpr (!INNER) b4 = b3, b3 = b2, b2 = b1;  // (b1 is complete: stage 1 used it; the inner steps rotate the five sets by name)
      if constexpr (INNER) uN += PB, bN += PB, wN += PB;
      __syncthreads();
    };
    // (stage s first matters at plane ja - (4 - s), which it reaches at step ja - 3 + (s - 1): every field buffer a valid point reads was
    // written by a step of this loop)
    // The march, steps q0 = ja - 3 .. jb + 3, in three parts:
    //   phase 0   q0 .. ja + 2: the six steps that fill the pipeline, general form (ja <= jb, so ja + 2 < jb + 3): three A/B pairs, so uA / bA
    //             hold the pending requests again when it ends, at q = ja + 3; a seventh where that q is odd
    //   inner     from the first even q >= ja + 3 to qi in groups of ten, while a whole group fits: b lives for four steps plus the step that requests it, so five
    //             register sets rotate BY NAME and are back in place after five steps, the two u sets after every two -- ten for both
    //   phase 1   from where the inner steps stopped to jb + 3, general form
    // The general loop is ONE copy in the code, run once per phase.
    const int qi = jb < g.jlast - 3 ? jb : g.jlast - 3;  // the last step that may take the inner form: q <= jb and q + 2 <= jlast - 1
    int q = q0;
    auto five = [&](auto even, auto odd, const int q5, Vec<V>& ua, Vec<V>& ub) __attribute__((always_inline)) {
      step(even, q5, ua, ub, bA, bB, bq1, bq2, bq3);
      step(odd, q5 + 1, ub, ua, bB, bq3, bA, bq1, bq2);
      step(even, q5 + 2, ua, ub, bq3, bq2, bB, bA, bq1);
      step(odd, q5 + 3, ub, ua, bq2, bq1, bq3, bB, bA);
      step(even, q5 + 4, ua, ub, bq1, bA, bq2, bq3, bB);
    };
    const std::integral_constant<int, -1> general;
    const std::integral_constant<int, 0> even;
    const std::integral_constant<int, 1> odd;
#pragma nounroll
    for (int phase = 0; phase < 2; phase++) {
      // (phase 0 takes a seventh step where ja + 3 is odd, so that the inner steps start at an even q and know their LDS buffers; the
      // pending requests are then in uB / bB and move to uA / bA, one wait per chunk)
      const int qg = phase == 0 ? ja + 2 + ((ja + 3) & 1) : jb + 3;
      for (;;) {
        step(general, q, uA, uB, bA, bB, bq1, bq2, bq3);
        if (++q > qg) break;
        step(general, q, uB, uA, bB, bA, bq1, bq2, bq3);
        if (++q > qg) break;
      }
      if (phase == 0) {  // (q = ja + 3 or ja + 4, even; bq1 .. bq3 = b(q-1) .. b(q-3))
        if ((ja + 3) & 1) uA = uB, bA = bB;
        uN = Ub + (size_t)(q + 2) * PB, bN = Bb + (size_t)(q + 1) * PB, wN = Wb + (size_t)(q - 3) * PB;  // (q - 3 >= ja: inside the array)
        for (; q + 9 <= qi; q += 10) {
          five(even, odd, q, uA, uB);
          five(odd, even, q + 5, uB, uA);
        }
        if (q > jb + 3) break;  // (a chunk of one plane whose ja + 3 is odd: the seventh step was the last)
      }
    }
  }

  // ---- residuals of the four sweeps: per-workgroup partials, finalised by the last workgroup
  const double acc[4] = {acc1, acc2, acc3, acc4};
  pass_epilogue<TB, 4>(acc, partials, fin, wsum);
}
