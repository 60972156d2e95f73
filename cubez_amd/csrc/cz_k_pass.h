// cz_k_pass.h -- part of cz_kernels.hip (ONE translation unit per precision; included inside its anonymous namespace after cz_k_fastdiv.h):
// the FRAME of the temporally blocked passes -- jacobi2p_k (cz_k_pair2.h), rb4_k (cz_k_rb4.h), jac3_k (cz_k_jac3.h), jac4_k (cz_k_jac4.h) and
// the shell kernel of a split pass (cz_k_pair.h).  What they share is stated here once: the geometry (Geom2) and the finalisation record
// (Fin2), the per-point update (relax_vec*), the map from a workgroup id to its work item (pass_item), the addresses of the windowed row
// view (RowView), the masks of a vector (vec_mask), the staging of the outer rows (outer_row), the masked store (store_owned) and the
// residual epilogue (pass_epilogue, on cz_k_sums.h).  For rb4_k, jac3_k and jac4_k also the LDS carve-up (deep_lds) and its size, which their
// launcher takes from here (deep_lds_bytes).  jac3_k and jac4_k further share a stage's two halves and the division policy (jac_fetch,
// jac_relax, JacDiv; cz_k_jac3.h).  What a kernel writes itself: how its threads are dealt to the vectors, which vectors it owns, its
// prologue, its per-lane set-up and the plane step with its requests.  Those differ between rb4_k, jac3_k and jac4_k in little but the depth,
// and stay copies for a reason that was checked each time, by the code the compiler makes of them:
//   r14  prologue, requests, operand fetch and A/B loop of rb4_k and jac3_k stated once as helpers: other register allocation and instruction
//        sequence in the plane steps of both (jac3_k 95 -> 86, rb4_k 128 -> 123 VGPRs), the Jacobi and RB-SOR bench lines at 512^3 1.6-1.8 %
//        slower (profiles/r14/pass_frame.txt)
//   r27  jac3_k and jac4_k, every kernel's instruction text against the parent's (profiles/r27/deep_pass_one_launcher.txt).  jac_fetch,
//        jac_relax as free functions and JacDiv: all 365 FP32 and 352 FP64 kernels identical, register names included -- taken.  The same
//        and the prologue block as a free function (outputs by reference): jac3_k identical, all 8 jac4_k differ, 4 in register names only, 4
//        in the opcode sequence (+4 instructions) -- not taken.  The same and the per-lane set-up (f, bo, masks, outer_row, waveh) returned
//        in a struct: all 8 jac3_k and all 8 jac4_k differ in the opcode sequence -- not taken.
// DESIGN 5.2.
// ------------------------------------------------------------------------------------------------------------
// SEVERAL relaxation stages per pass over memory (temporal blocking).
//
// Each sweep of cz_solver.f90:334-351 is HBM bound at 12 B per update and stencil_k already moves within 5 % of the ideal bytes
// (profiles/r01), so the only way past the streaming ceiling is to apply sweep n+1, n+2 (, n+3) while the data are on chip.  Same 2.5-D march
// as stencil_k, D stages deep -- stage s at step q works on plane q - s + 1:
//     stage 1 at plane q   : f1(q)   = relax(u(q-1), u(q), u(q+1))        on the own segment +- (D-1) k-rows (R vectors each)
//     stage 2 at plane q-1 : f2(q-1) = relax(f1(q-2), f1(q-1), f1(q))     on the own segment +- (D-2) rows ... stage D on the own segment -> W
// u = input field, f1 .. f(D-1) never leave the CU (registers + LDS), fD = output.  LDS holds the centre planes of u (own segment +- D rows)
// and of every intermediate field for the i+-1 / k+-1 neighbours, double-buffered, one barrier per plane step; the j-1 operand of a vector is
// re-read from the buffer its own thread wrote, the j+1 operand is the value just made.  The halo rows and the first/last planes of a chunk
// are recomputed by the neighbouring workgroups (redundant arithmetic) instead of being exchanged.  Points outside the inner box pass through
// unchanged, exactly what separate sweeps would have left in memory, and the per-point arithmetic is the same un-fused float sequence, so the
// result is bit-identical to D launches of stencil_k.  One residual (sum dp^2) per sweep or iteration is produced; each point is counted by
// the one workgroup that owns it.
// ------------------------------------------------------------------------------------------------------------
struct Geom2 {
  // Rows of the (k, i) plane as the pass sees them: R vectors each, row i starting at a vector boundary.  In memory a row is nkp elements
  // long and rows follow one another without padding: where nkp is not a multiple of the vector width the last vector of a row is partial
  // (its tail belongs to the next row and is masked like every k outside the box) and a vector is only REAL-aligned in memory -- the global
  // accesses of the pass are dword-aligned dwordx4, which this hardware takes.  (Rounds 1-2 required nkp % V == 0 and sent every other
  // size to the one-sweep scalar kernel: 220 000 against 740 000 MLUPS at 511^3, profiles/r03/unaligned_k_extent.txt.)
  //
  // K WINDOWS (round 4).  The segment of a workgroup is a run of whole rows with one (stage 1) and two (u) halo rows on either side in LDS, so
  // its useful share is (TB MV - 2R) / (TB MV): rows beyond 2 044 (FP32) / 1 020 (FP64) elements did not fit at all (single sweeps at half
  // the rate until round 3), and from 700 elements up a segment was two or three rows of five to seven.  Now the k axis may be cut into
  // `nwin` windows of KT vectors: a workgroup sees its window as a plane of its own whose rows are R = KT + 2 vectors long -- the window plus
  // ONE halo vector on either side (a stage-2 point at the window's edge reads the stage-1 value next to it, which this workgroup computes
  // itself from the u values of that halo vector: V >= 2 elements reach far enough).  Nothing else changes in the kernel: +-R is still the i
  // neighbour, +-1 element the k neighbour, the lane next door holds it; only the map from (row, vector of the row) to memory gains the
  // window's origin `kw0`, and a vector is owned by the workgroup whose window holds it.  Same per-point arithmetic on the same values =>
  // the same bits (test_two_fused_sweeps_equal_two_oracle_sweeps with forced windows; k = 1 100 FP64 and k = 2 100 FP32 boxes).
  int R;
  long long PSV;               // R * nip: vectors per plane in that view
  int nkp = 0;                 // elements per row in memory
  long long PSB = 0;           // bytes per plane in memory
  int jlast = 0;               // index of the array's last plane, whose last vectors must not be read beyond the array:
  unsigned last_off = 0;       // ... offsets into that plane are clamped to this (the values clamped away are never used)
  int nwin = 1;                // k windows per row
  int hv = 0;                  // halo vectors on either side of a window (1 when nwin > 1)
  int KT = 1 << 30;            // vectors a window owns: vector kv of a virtual row is owned when hv <= kv < hv + KT
  int KW = 0;                  // elements from one window's origin to the next (= KT * V)
  int nsegw = 0;               // segments per window (nseg = nwin * nsegw; segment s of window w has the id w * nsegw + s)
  int kk0, kk1, jj0, jj1;      // output box = the inner box
  long long F0, Fend;
  // stage-1 box: the inner box, grown by one layer across rank-internal faces of a decomposed run (the first sweep
  // must also be applied to the ghost layer the second sweep reads; two ghost layers are exchanged per pair)
  int kk0a, kk1a, jj0a, jj1a;
  long long F0a, Fenda;
  int nseg, TJ, S;  // S = vectors a workgroup holds - halo rows * R
  int par;          // RB: colour 0 = points with (kk + ii + jj + par) even
  int zero_u;       // the input field is identically zero (a freshly cleared preconditioner vector): u is not read
  int band;         // workgroup id -> (segment, chunk) by XCD bands (see pass_item)
  const int* map;   // or by a table: map[2 * id] = segment (nseg: no work), map[2 * id + 1] = chunk (pair_xcd_map, cz_h_launch.h)
};

// jacobi2p_k<..., BS>: the right-hand side made on the fly (see there).  x, y, z: operands; out: where the owner of a vector stores it.
struct BSrc {
  const REAL* x = nullptr;
  const REAL* y = nullptr;
  const REAL* z = nullptr;
  REAL* out = nullptr;
  REAL a = 0, b = 0;
  const REAL* pa = nullptr;  // where set: a is read from the device (bicg_scal_k)
};

struct Fin2 {
  double* dst = nullptr;   // [s] <- sum of sweep n+1+s
  int do_check = 0, itr = 0;  // itr = iteration number of sweep n+1
  int single = 0;             // RB, two stages: both belong to ONE iteration: dst[0] = sum1 + sum2, one bookkeeping step
  const double* extra = nullptr;  // per-workgroup sums of the shell launch of a split pass (pair_shell_k): n_extra first-stage
  int n_extra = 0;                // sums followed by n_extra second-stage sums, added to this launch's own
  double res_normal = 0.0, eps = 0.0;
  double* hist = nullptr;
  int* flag = nullptr;
  int* conv_itr = nullptr;
  unsigned* counter = nullptr;
};

// bit cc set when (base + cc) is even
template <int V>
__device__ __forceinline__ unsigned colour_bits(int base) {
  const unsigned even = (V == 4) ? 0x5u : (V == 2) ? 0x1u : 0x1u;   // components 0,2 / 0 / 0
  const unsigned odd = (V == 4) ? 0xAu : (V == 2) ? 0x2u : 0x0u;    // components 1,3 / 1 / -
  return (base & 1) ? odd : even;
}

// the ordinary division (the compiler's IEEE expansion at every point); see cz_k_fastdiv.h for the hoisted form
struct PlainDiv {
  REAL d;
  __device__ __forceinline__ REAL operator()(REAL n) const { return n / d; }
};
struct HoistedDiv {
  FastDiv<REAL> f;
  __device__ __forceinline__ REAL operator()(REAL n) const { return fastdiv(n, f); }
};

struct ShortDiv {  // cz_k_fastdiv.h: only for divisors that passed the exhaustive comparison
  FastDiv<REAL> f;
  __device__ __forceinline__ REAL operator()(REAL n) const { return shortdiv(n, f); }
};

struct MediumDiv {
  FastDiv<REAL> f;
  __device__ __forceinline__ REAL operator()(REAL n) const { return mediumdiv(n, f); }
};

// The medium (MED = 1) or hoisted (MED = 0) form, GATED (cz_k_fastdiv.h): one test per vector and wave whether any numerator is huge, and
// where none is -- every wave of a real field -- the tail without den_s, compare and select.  A policy with a vector-level entry: relax_vec
// hands it the V numerators of a vector at once.  Only for divisors that passed fastdiv_check_k<3 | 4> on this context (jac3_gated, cz_h_launch.h).
__device__ __forceinline__ float uniform_real(float x) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, x))); }
__device__ __forceinline__ double uniform_real(double x) {
  const unsigned long long b = __builtin_bit_cast(unsigned long long, x);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
template <int MED>
struct GatedDiv {
  FastDiv<REAL> f;
  REAL T;  // f.T, the same in every lane (a scalar register)
  __device__ __forceinline__ explicit GatedDiv(const FastDiv<REAL>& f_) : f(f_), T(uniform_real(f_.T)) {}
  template <int V>
  __device__ __forceinline__ void vec(const REAL (&n)[V], REAL (&q)[V]) const {
    if (__builtin_expect(gated_none_huge<V>(n, T), 1)) {  // (expected: the gated tail is the fall-through path)
#pragma unroll
      for (int cc = 0; cc < V; cc++) q[cc] = gated_tail<MED>(n[cc], f);
    } else {
#pragma unroll
      for (int cc = 0; cc < V; cc++) q[cc] = general_tail<MED>(n[cc], f);
    }
  }
};
template <class DIV>
struct has_vec_entry : std::false_type {};
template <int MED>
struct has_vec_entry<GatedDiv<MED>> : std::true_type {};

template <int V, int UNIT = 0, class DIV>
__device__ __forceinline__ Vec<V> relax_vec(const Vec<V>& pc, const Vec<V>& im, const Vec<V>& ip, const Vec<V>& pm,
                                            const Vec<V>& pn, REAL kl, REAL kr, const Vec<V>& bb, const Coef& c, const DIV& dv,
                                            unsigned mask, unsigned count_mask, double& acc) {
  Vec<V> o;
#if defined(CZ_P2_RES_GROUP)  // tools/pair_lab A/B only: the vector's dp^2 summed in REAL, one conversion and one double add per vector
  REAL grp = (REAL)0;
#endif
  constexpr bool BY_VECTOR = has_vec_entry<DIV>::value;  // the policy divides the V numerators of the vector at once
  REAL nv[V], qv[V];
  if constexpr (BY_VECTOR) {
#pragma unroll
    for (int cc = 0; cc < V; cc++) {
      const REAL km1 = (cc == 0) ? kl : pc.v[cc > 0 ? cc - 1 : 0];
      const REAL kp1 = (cc == V - 1) ? kr : pc.v[cc < V - 1 ? cc + 1 : V - 1];
      nv[cc] = offdiag_sum<UNIT>(c, ip.v[cc], im.v[cc], pn.v[cc], pm.v[cc], kp1, km1) - bb.v[cc];
    }
    dv.template vec<V>(nv, qv);
  }
#pragma unroll
  for (int cc = 0; cc < V; cc++) {
    const REAL pp = pc.v[cc];
    REAL qd;
    if constexpr (BY_VECTOR) {
      qd = qv[cc];
    } else {
      const REAL km1 = (cc == 0) ? kl : pc.v[cc > 0 ? cc - 1 : 0];
      const REAL kp1 = (cc == V - 1) ? kr : pc.v[cc < V - 1 ? cc + 1 : V - 1];
      const REAL ss = offdiag_sum<UNIT>(c, ip.v[cc], im.v[cc], pn.v[cc], pm.v[cc], kp1, km1);
      qd = dv(ss - bb.v[cc]);
    }
    const REAL dp = (qd - pp) * c.omg;
    const REAL d2 = dp * dp;
    o.v[cc] = (mask & (1u << cc)) ? pp + dp : pp;
#if defined(CZ_P2_NO_RES)  // tools/pair_lab A/B only: no residual at all (what the accumulation costs at most)
    (void)d2, (void)count_mask, (void)acc;
#elif defined(CZ_P2_RES_GROUP)
    grp += (count_mask & (1u << cc)) ? d2 : (REAL)0;
#else
    acc += (double)((count_mask & (1u << cc)) ? d2 : (REAL)0);  // (+0.0 leaves the sum as it is)
#endif
  }
#if defined(CZ_P2_RES_GROUP)
  acc += (double)grp;
#endif
  return o;
}

// The MAF flavour of the per-point update (cz_maf.f90:193-225, operation for operation as in stencil_k<..., MAF = 1>): the six weights and
// the diagonal are recomputed at every point from the metric terms of the 1-D grids -- XG, XGG of the row, YE, YEE of the plane, ZT, ZTT of
// the component.
template <int V>
__device__ __forceinline__ Vec<V> relax_vec_maf(const Vec<V>& pc, const Vec<V>& im, const Vec<V>& ip, const Vec<V>& pm, const Vec<V>& pn,
                                                REAL kl, REAL kr, const Vec<V>& bb, REAL XG, REAL XGG, REAL YE, REAL YEE, const Vec<V>& ZT,
                                                const Vec<V>& ZTT, REAL omg, unsigned mask, unsigned count_mask, double& acc) {
  Vec<V> o;
#pragma unroll
  for (int cc = 0; cc < V; cc++) {
    const REAL pp = pc.v[cc];
    const REAL km1 = (cc == 0) ? kl : pc.v[cc > 0 ? cc - 1 : 0];
    const REAL kp1 = (cc == V - 1) ? kr : pc.v[cc < V - 1 ? cc + 1 : V - 1];
    const MafW w = maf_weights(XG, XGG, YE, YEE, ZT.v[cc], ZTT.v[cc]);
    const REAL rp = w.w1 * ip.v[cc] + w.w2 * im.v[cc] + w.w3 * pn.v[cc] + w.w4 * pm.v[cc] + w.w5 * kp1 + w.w6 * km1 + bb.v[cc];  // :219-225
    const REAL dp = (rp / w.dd - pp) * omg;
    const REAL d2 = dp * dp;
    o.v[cc] = (mask & (1u << cc)) ? pp + dp : pp;
    acc += (double)((count_mask & (1u << cc)) ? d2 : (REAL)0);
  }
  return o;
}

// global accesses of the pass: a vector is REAL-aligned in memory (16-byte aligned where the row length is a multiple of the vector width)
template <int V>
__device__ __forceinline__ Vec<V> ld16(const char* plane, unsigned byte_off) {
  typedef typename NatVec<V>::type nv;
  typedef nv unv __attribute__((aligned(sizeof(REAL))));
  const nv x = *reinterpret_cast<const unv*>(plane + byte_off);
  Vec<V> r;
  __builtin_memcpy(&r, &x, sizeof(r));
  return r;
}
template <int V>
__device__ __forceinline__ void st16(char* plane, unsigned byte_off, const Vec<V>& x) {
  typedef typename NatVec<V>::type nv;
  typedef nv unv __attribute__((aligned(sizeof(REAL))));
  nv y;
  __builtin_memcpy(&y, &x, sizeof(y));
  *reinterpret_cast<unv*>(plane + byte_off) = y;
}

// one ds_read_b128 per vector: left to itself the compiler re-reads overlapping pieces of a vector with ds_read_b32 / ds_read2_b32
// (operand pairs for packed FP32 math) -- stride-16-byte scalar reads, i.e. 4-way bank conflicts
template <int V>
__device__ __forceinline__ Vec<V> lds_ld(const Vec<V>* p) {
  typedef typename NatVec<V>::type nv;
  nv x = *reinterpret_cast<const nv*>(p);
  asm("" : "+v"(x));  // the value is needed whole, in consecutive registers: keeps the read one ds_read_b128
  Vec<V> r;
  __builtin_memcpy(&r, &x, sizeof(r));
  return r;
}

// ------------------------------------------------------------------------------------------------------------
// Workgroup id -> work item: the k window, the row segment inside it (first vector fb of the window's row view) and the chunk of planes
// ja .. jb.  `work` is false for the ids that pad the launch to whole XCD rounds.
struct PassItem {
  int win, seg, chunk;
  int kw0;       // element of the row that vector 0 of the window's view starts at (-hv * V: the left halo of window 0)
  long long fb;  // first own vector of the segment
  int ja, jb;
  bool work;
};
template <int V>
__device__ __forceinline__ PassItem pass_item(const Geom2& g) {
  PassItem it;
  const int lb = blockIdx.x;
  int seg, chunk;
  if (g.map != nullptr) {
    // balanced shares: the (segment, chunk) items in segment-major order are cut into eight equal runs, one per XCD (the hardware deals
    // workgroup ids round-robin over the XCDs), each walked chunk by chunk -- see pair_xcd_map
    seg = g.map[2 * lb];
    chunk = g.map[2 * lb + 1];
  } else {
    // XCD bands: XCD x owns a contiguous band of whole segments of every chunk (row-adjacent segments share their halo rows in one L2)
    // and walks it chunk by chunk
    const int x = lb & 7, r = lb >> 3;
    const int base = g.nseg >> 3, rem = g.nseg & 7, bmax = base + (rem ? 1 : 0);
    const int blen = base + (x < rem ? 1 : 0);
    const int sl = r % bmax;
    chunk = r / bmax;
    seg = (sl < blen) ? x * base + min(x, rem) + sl : g.nseg;  // nseg = no work
  }
  // k window of this segment (Geom2): ids are window-major, so the band / run of an XCD is a set of row-adjacent segments of ONE window.
  // (The nwin > 1 guards stay: plan_pass fills nsegw for whole rows too, a geometry made by hand -- tools/pair_lab -- may leave it 0.)
  int win = 0;
  if (g.nwin > 1 && seg < g.nseg) {
    win = seg / g.nsegw;
    seg -= win * g.nsegw;
  } else if (g.nwin > 1) {
    seg = g.nsegw;  // no work
  }
  const int nseg_w = (g.nwin > 1) ? g.nsegw : g.nseg;
  it.win = win, it.seg = seg, it.chunk = chunk;
  it.kw0 = win * g.KW - g.hv * V;
  it.fb = (seg < nseg_w) ? g.F0 + (long long)seg * g.S : g.Fend;
  it.ja = g.jj0 + chunk * g.TJ;
  it.jb = it.ja + g.TJ - 1;
  if (it.jb > g.jj1) it.jb = g.jj1;
  it.work = it.ja <= it.jb && it.fb < g.Fend;
  return it;
}

// Addresses of the (window's) row view: vector f = row * R + kv of the view is element row * nkp + kw0 + kv * V of a plane in memory.
template <int V>
struct RowView {
  int R, nkp, kw0, jlast;
  unsigned last_off;
  long long vlast;  // last vector of the view of a plane
  // Byte offset of vector f inside a plane.  f is clamped into the view first (the vectors clamped away belong to lanes that are masked).
  // Then the one subtle rule: the ELEMENT offset is clamped BELOW the plane (row 0's left halo vector of window 0: masked, and no unmasked
  // point reads it) and NOT beyond its end -- the last vector of the last row of a plane whose rows are no multiple of the vector width
  // hangs over by a few elements and IS read by the first stage of a decomposed brick (row nip-1 is the second ghost layer); the elements
  // behind the plane are the next plane's, masked.  Only in the array's last plane must the access stay inside, and there the vector is
  // never used: `lim`, Geom2::last_off.  (Clamping into the plane for EVERY plane shifted that vector: DESIGN 5.2.)
  // (jacobi2p_k used to clamp f only above, at its call sites; rb4_k and jac3_k on both sides, here.  The clamp below never acts in
  // jacobi2p_k: its lowest vector is fb - 2R with fb >= F0 = ii0 * R and ii0 >= 2 -- launch_jacobi2 refuses boxes with less than two layers
  // below -- so f >= 0 in every call and every call gets the offset it got; the same holds for the `fc` of vec_mask.)
  __device__ __forceinline__ unsigned off_of(long long f) const {
    if (f < 0) f = 0;
    if (f > vlast) f = vlast;
    const long long r = f / R;
    long long el = r * nkp + kw0 + (f - r * R) * V;
    el = el < 0 ? 0 : el;
    return (unsigned)(el * (long long)sizeof(REAL));
  }
  __device__ __forceinline__ unsigned lim(unsigned off, int plane) const { return plane == jlast ? (off < last_off ? off : last_off) : off; }
  __device__ __forceinline__ int pl(int p) const { return p < 0 ? 0 : (p > jlast ? jlast : p); }  // planes beyond the array are never used: clamped
};
template <int V>
__device__ __forceinline__ RowView<V> row_view(const Geom2& g, const PassItem& it) {
  return RowView<V>{g.R, g.nkp, it.kw0, g.jlast, g.last_off, g.PSV - 1};
}

// Masks of vector f of the row view: the components whose k lies inside the inner (output) box and inside the stage-1 box, whether its row
// lies inside them, whether the window owns the vector (its halo vectors belong to the windows next door); RB: pbase = (kk + ii + par) of
// component 0 -- component cc on plane jj has colour (pbase + cc + jj) & 1.  A kernel forms its masks from these in one select each
// (`rows ? bits : 0`, `(its own range && rows && kown) ? bits : 0`): the compiler turns such a mask into per-component wave masks that the plane
// steps use directly, and a select of a select is not simplified that way -- it cost rb4_k and jac3_k 50 instructions per pair of steps.
struct VecMask {
  unsigned bits, bits1;  // components with k inside the inner box / the stage-1 box
  bool rows, rows1;      // the vector lies in a row of the inner box / the stage-1 box
  bool kown;
  int pbase;
};
template <int V>
__device__ __forceinline__ VecMask vec_mask(const Geom2& g, const PassItem& it, long long f) {
  const long long fc = f < 0 ? 0 : f;
  const long long row = fc / g.R;
  const int kv = (int)(fc - row * g.R);
  const int kb = it.kw0 + kv * V;  // k of component 0
  VecMask m;
  m.bits = 0, m.bits1 = 0;
#pragma unroll
  for (int cc = 0; cc < V; cc++) {
    const int kk = kb + cc;
    if (kk >= g.kk0a && kk <= g.kk1a) m.bits1 |= 1u << cc;
    if (kk >= g.kk0 && kk <= g.kk1) m.bits |= 1u << cc;
  }
  m.rows = f >= g.F0 && f < g.Fend;
  m.rows1 = f >= g.F0a && f < g.Fenda;
  m.kown = kv >= g.hv && kv < g.hv + g.KT;
  m.pbase = kb + (int)row + g.par;
  return m;
}

// The two outer rows of the u planes in LDS (LV own vectors with R in front and R behind): the first R threads stage the lower one, the last R
// threads the upper one (2R <= TB).  hl = index inside an LDS u buffer, bo = byte offset in a plane; the other threads get the offset of
// their own vector f_own, so that the load is unconditional.  f_outer0 = first vector of the lower outer row.
struct OuterRow {
  bool has;
  int hl;
  unsigned bo;
};
template <int V, int TB>
__device__ __forceinline__ OuterRow outer_row(const RowView<V>& rv, int LV, long long f_outer0, long long f_own) {
  const int t = threadIdx.x, R = rv.R;
  OuterRow h;
  h.has = (t < R) || (t >= TB - R);
  h.hl = (t < R) ? t : (LV + R + (t - (TB - R)));
  h.bo = rv.off_of(h.has ? f_outer0 + h.hl : f_own);
  return h;
}

// the components `own` of a vector to byte offset bo of a plane: one 16-byte store where all are owned
template <int V>
__device__ __forceinline__ void store_owned(char* plane, unsigned bo, unsigned own, const Vec<V>& x) {
  if (own == (1u << V) - 1) {
    st16<V>(plane, bo, x);
  } else if (own != 0) {
    REAL* p = reinterpret_cast<REAL*>(plane + bo);
#pragma unroll
    for (int cc = 0; cc < V; cc++)
      if (own & (1u << cc)) p[cc] = x.v[cc];
  }
}

// ------------------------------------------------------------------------------------------------------------
// The passes of D stages with ONE vector per thread (rb4_k, jac4_k: D = 4, jac3_k: D = 3): u on the own segment +- D rows, the intermediate fields
// f1 .. f(D-1) on E = own segment +- (D-1) rows, LV = TB vectors of which S = LV - 2 (D-1) R are the workgroup's own.
// LDS: u in 2 buffers of LU = LV + 2R vectors, then f1 .. f(D-1) in 2 buffers of LV each -- plane p in buffer p & 1 -- then the 18 doubles of
// the epilogue.  R vectors of padding in front of the u buffers and behind the last field buffer: the stages are evaluated on whole waves
// and the lanes beyond a stage's set read +-R outside it -- inside the allocation, never used.
template <int V>
struct DeepLds {
  int LU;
  Vec<V>* U;  // [plane & 1][LU]
  Vec<V>* F;  // [field][plane & 1][LV]
  double* wsum;
};
// The vectors of that carve-up, i.e. where the epilogue's doubles start, and the dynamic LDS of a launch: the ONE statement of the size, for
// the device (deep_lds) and the host (launch_deep, cz_h_launch.h).
__host__ __device__ constexpr size_t deep_lds_vectors(int LV, int D, int R) {
  return (size_t)R + (size_t)2 * (LV + 2 * R) + (size_t)(2 * (D - 1)) * LV + (size_t)R;
}
template <int V>
__host__ __device__ constexpr size_t deep_lds_bytes(int LV, int D, int R) {
  return deep_lds_vectors(LV, D, R) * sizeof(Vec<V>) + 18 * sizeof(double);
}
template <int V, int LV, int D>
__device__ __forceinline__ DeepLds<V> deep_lds(char* smem, int R) {
  DeepLds<V> l;
  l.LU = LV + 2 * R;
  l.U = reinterpret_cast<Vec<V>*>(smem) + R;
  l.F = l.U + (size_t)2 * l.LU;
  // = smem + deep_lds_vectors(LV, D, R).  Written from F, not from that expression: derived from it the plane steps of rb4_k, jac3_k and
  // jac4_k compiled to other code (FP64 rb4_k with 8 bytes of scratch; profiles/r27/deep_pass_one_launcher.txt).  The assertion ties the two.
  static_assert(deep_lds_vectors(LV, D, 1) == 1 + 2 * (LV + 2) + (2 * (D - 1)) * LV + 1 &&
                    deep_lds_vectors(LV, D, 2) - deep_lds_vectors(LV, D, 1) == 6,
                "deep_lds and deep_lds_vectors carve the same allocation: R + 2 LU + 2 (D - 1) LV + R vectors, linear in R");
  l.wsum = reinterpret_cast<double*>(l.F + (size_t)(2 * (D - 1)) * LV + R);
  return l;
}

// ------------------------------------------------------------------------------------------------------------
// End of a pass kernel, all threads: the workgroup's N residual sums through the hand-off of cz_k_sums.h (partials[s * nblk + id]).  What
// the pass adds to it: a thread of the last workgroup also takes its strided share of the `extra` terms (written by an earlier launch on
// this stream) after its partials, and thread 0 does the bookkeeping of cz_Poisson.cpp:67-77 for the iterations of the pass in order --
// record the residual of iteration itr + s, stop at the first that converged.  N sums are N iterations, or with fin.single (N = 2: the two
// colours of a red-black iteration, cz_Poisson.cpp:205-209 accumulate into one res) ONE: t1 + t2 comes last.  wsum: TB / 64 + 1 doubles of LDS.
template <int TB, int N>
__device__ __forceinline__ void pass_epilogue(const double (&acc)[N], double* partials, const Fin2& fin, double* wsum) {
  const SumsAt at{(int)blockIdx.x, (int)gridDim.x};
  __syncthreads();
  sums_finish<TB>(
      acc, partials, at, fin.counter, wsum,
      [&](double (&x)[N]) {
        for (int i = threadIdx.x; i < fin.n_extra; i += TB) {
#pragma unroll
          for (int q = 0; q < N; q++) x[q] += fin.extra[q * fin.n_extra + i];
        }
      },
      [&](double (&tot)[N]) {
        const bool single = N == 2 && fin.single;
        if (single) tot[0] = tot[0] + tot[1];
        const int nit = single ? 1 : N;
        for (int q = 0; q < nit; q++) fin.dst[q] = tot[q];
        if (fin.do_check) {
          for (int q = 0; q < nit; q++) {
            const double r = sqrt(tot[q] * fin.res_normal);
            fin.hist[fin.itr + q] = r;
            if (r < fin.eps) {
              *fin.flag = 1;
              *fin.conv_itr = fin.itr + q;
              break;
            }
          }
        }
      });
}
