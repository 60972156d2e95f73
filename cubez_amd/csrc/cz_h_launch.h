// cz_h_launch.h -- part of cz_kernels.hip (ONE translation unit per precision; this file is included inside its anonymous
// namespace and is not a stand-alone header): host side: launch geometry of the sweep, pair, shell, element-wise and dot kernels.
template <int V, int TB, int M, int PF, int MODE, int MAF = 0>
void launch_stencil_inst(const REAL* P, const REAL* B, REAL* OUT, const Coef& c, const Box& b, int par, int tj_req,
                         const int* skip, int* nblk_out, const Fin& fin, const MafArgs& ma = MafArgs()) {
  Geom g;
  g.nip = b.nip;
  g.R = (b.nkp + V - 1) / V;  // rows from a vector boundary each; the last vector of a row partial where nkp % V != 0 (Geom)
  g.PSV = (long long)g.R * b.nip;
  g.nkp = b.nkp;
  g.PSE = (long long)b.nkp * b.nip;
  g.jlast = b.njp - 1;
  g.last_eo = g.PSE - V;
  g.kk0 = b.kk0, g.kk1 = b.kk1, g.jj0 = b.jj0, g.jj1 = b.jj1;
  g.F0 = (long long)b.ii0 * g.R;
  g.Fend = (long long)(b.ii1 + 1) * g.R;
  g.S = TB * M;
  const long long nf = g.Fend - g.F0;
  g.nseg = (int)((nf + g.S - 1) / g.S);
  const int nplanes = b.jj1 - b.jj0 + 1;
  int tj = tj_req;
  if (tj <= 0) {
    // auto: enough workgroups to fill the chip a few times over, chunk count a multiple of 8 (XCD remap)
    const int waves_per_wg = TB / 64;
    const long long want = (long long)ctx.num_cu * 32 / waves_per_wg;  // one full residency of waves
    int nchunk = (int)((want + g.nseg - 1) / g.nseg);
    nchunk = ((nchunk + 7) / 8) * 8;
    if (nchunk > nplanes) nchunk = nplanes;
    if (nchunk < 1) nchunk = 1;
    tj = (nplanes + nchunk - 1) / nchunk;
  }
  if (tj > nplanes) tj = nplanes;
  g.TJ = tj;
  int nchunk = (nplanes + tj - 1) / tj;
  // pad the chunk count to a multiple of 8 when that costs nothing but empty workgroups (keeps the remap on)
  if (((long long)nchunk * g.nseg) % 8 != 0 && nchunk >= 8) nchunk = ((nchunk + 7) / 8) * 8;
  const long long nblk = (long long)nchunk * g.nseg;
  const size_t lds = (size_t)2 * (g.S + 2 * g.R) * sizeof(Vec<V>) + 18 * sizeof(double);
  if (lds > 160 * 1024) {
    cz_fatal(1, "czhip: k-row of %d elements needs %zu bytes of LDS (>160 KiB)\n", b.nkp, lds);
  }
  if (MODE == MODE_JACOBI || MODE == MODE_RB || MODE == MODE_AX || MODE == MODE_DIRAX) ensure_partials((size_t)2 * nblk);
  allow_dynamic_lds(&stencil_k<V, TB, M, PF, MODE, MAF>, 160 * 1024);
  {
    ScopedTimer tm(MODE == MODE_JACOBI ? LBL_JACOBI : MODE == MODE_RB ? LBL_RBSOR : (MODE == MODE_AX || MODE == MODE_DIRAX) ? LBL_AX : LBL_RK);
    hipLaunchKernelGGL((stencil_k<V, TB, M, PF, MODE, MAF>), dim3((unsigned)nblk), dim3(TB), lds, ctx.stream, P, B, OUT, c, g, par,
                       ctx.partials, skip, fin, ma);
  }
  HIP_CHECK(hipGetLastError());
  if (nblk_out) *nblk_out = (int)nblk;
}

template <int MODE>
void launch_stencil(const REAL* P, const REAL* B, REAL* OUT, const Coef& c, const Box& b, int par, const int* skip,
                    int* nblk_out, const Fin& fin = Fin()) {
  const Tuning& tu = ctx.tune;
  if (!rows_ok(b, {P, B, OUT})) {
    launch_stencil_inst<1, 256, 2, 0, MODE>(P, B, OUT, c, b, par, tu.tj, skip, nblk_out, fin);
    return;
  }
#define CZ_INST(TB_, M_, PF_)                                                                      \
  if (tu.threads == TB_ && tu.m == M_ && tu.pf == PF_) {                                           \
    launch_stencil_inst<VW, TB_, M_, PF_, MODE>(P, B, OUT, c, b, par, tu.tj, skip, nblk_out, fin); \
    return;                                                                                        \
  }
  if (MODE == MODE_JACOBI || MODE == MODE_RB) {
    CZ_INST(256, 1, 0) CZ_INST(256, 1, 1) CZ_INST(256, 2, 0) CZ_INST(256, 2, 1) CZ_INST(256, 4, 0) CZ_INST(256, 4, 1)
    CZ_INST(512, 1, 0) CZ_INST(512, 1, 1) CZ_INST(512, 2, 0) CZ_INST(512, 2, 1) CZ_INST(512, 4, 0) CZ_INST(512, 4, 1)
    CZ_INST(1024, 1, 0) CZ_INST(1024, 1, 1) CZ_INST(1024, 2, 0) CZ_INST(1024, 2, 1)
  }
#undef CZ_INST
  launch_stencil_inst<VW, 512, 2, 0, MODE>(P, B, OUT, c, b, par, tu.tj, skip, nblk_out, fin);
}

// the coefficients of the MAF kernels, which compute their weights per point: only omg
Coef make_coef_omg(REAL omg) {
  Coef c;
  c.c1 = c.c2 = c.c3 = c.c4 = c.c5 = c.c6 = c.dd = (REAL)0;
  c.omg = omg;
  return c;
}

// MAF flavour: one tuned shape (and the scalar fallback); coordinates / pvt are device pointers
template <int MODE>
void launch_stencil_maf(const REAL* P, const REAL* B, REAL* OUT, REAL omg, const Box& b, int par, const int* skip, int* nblk_out,
                        const Fin& fin, const MafArgs& ma) {
  if (b.g != 2) {
    cz_fatal(1, "czhip: the MAF kernels assume GUIDE = 2 (X(-1:sz+2), cz_maf.f90:146-148)\n");
  }
  const Coef c = make_coef_omg(omg);
  if (rows_ok(b, {P, B, OUT, ma.pvt}))
    launch_stencil_inst<VW, 512, 2, 0, MODE, 1>(P, B, OUT, c, b, par, ctx.tune.tj, skip, nblk_out, fin, ma);
  else
    launch_stencil_inst<1, 256, 2, 0, MODE, 1>(P, B, OUT, c, b, par, ctx.tune.tj, skip, nblk_out, fin, ma);
}

void reduce_partials(int n, double* dst, int accumulate, const int* skip) {
  ScopedTimer tm(LBL_REDUCE);
  hipLaunchKernelGGL(reduce_partials_k, dim3(1), dim3(1024), 0, ctx.stream, ctx.partials, n, dst, accumulate, skip);
  HIP_CHECK(hipGetLastError());
}


// Planes per chunk of the two-stage pass.  A workgroup of chunk length tj costs about tj + 3.5 plane steps (two redundant planes and
// the un-overlapped prologue); each XCD serves its band of segments with num_cu/8 * wg_per_cu resident workgroups, so a launch takes
// ceil(band * nchunk / slots) rounds of that (tools/pair_lab sweeps, profiles/r02/pair_lab_sweep_*.txt: the model ranks the measured
// times of both shapes and both precisions).  Returns the cost in units of plane steps; *tj_out the best chunk length.
inline double pair_tj_model(int nseg, int nplanes, int wg_per_cu, bool balanced, int* tj_out, double extra = 3.5, bool long_chunks = false) {
  // (decomposed runs: cu_reserved CUs of every XCD stay free for the exchange stream; reserve_comm_cus)
  const int slots = std::max(1, ctx.num_cu / 8 - ctx.cu_reserved) * wg_per_cu;
  double best = 1e300;
  int best_tj = std::min(16, nplanes);
  // (chunks from two planes up: on small grids, where one round of short chunks holds every item, the chain of plane steps of a workgroup is
  // the whole launch -- 64^3 FP64: 16 us per pass with chunks of 2 planes against 32 us with 12, the floor of rounds 1-2;
  // profiles/r03/small_grids_chunk_length.txt)
  // (chunks of more than 128 planes only with long_chunks, and only where the whole launch is then ONE round: jac3_k at 512^3 FP32 takes
  // 3 chunks of 171 planes, 240 workgroups at once, against 16 chunks of 32 in five rounds -- fewer re-read halo planes and redundant
  // plane steps per point; profiles/r10/pass_planner.txt.  Plans of several rounds keep the cap the other passes were tuned with.)
  for (int tj = std::min(2, nplanes); tj <= nplanes; tj++) {
    const int nchunk = (nplanes + tj - 1) / tj;
    if (tj > 2 && (nplanes + tj - 2) / (tj - 1) == nchunk) continue;  // a shorter chunk gives the same count: not a candidate
    // items of the busiest XCD: a band of whole segments, or an eighth of all items with the balanced table (pair_xcd_map)
    const long long items = balanced ? ((long long)nseg * nchunk + 7) / 8 : (long long)((nseg + 7) / 8) * nchunk;
    if (tj > 128 && !(long_chunks && items <= slots)) continue;
    const double cost = (double)((items + slots - 1) / slots) * (tj + extra);
    if (cost < best) best = cost, best_tj = tj;
  }
  *tj_out = best_tj;
  return best;
}

// Workgroup id -> (segment, chunk) table with equal shares per XCD.  With whole-segment bands an XCD serves ceil(nseg/8) or floor(nseg/8)
// segments: 5 against 4 at 512^3 with the 1024-thread shape, i.e. three XCDs idle for a fifth of the launch.  Here the nseg*nchunk items,
// taken in segment-major order, are cut into eight runs of equal length; an XCD's run covers whole segments except at its two ends, where
// a segment is shared with the neighbouring XCD by plane range.  Inside its run an XCD walks chunk by chunk (row-adjacent segments are then
// in the same planes at the same time and share their halo rows in the XCD's L2).  Cached per (nseg, nchunk); 8 bytes per workgroup.
// Measured (profiles/r02/ab_xcd_map.txt): +6 % at 256^3 and 384^3, where the bands are 3 against 2 segments; -1 % at 512^3 and -4 % at
// 640^3, where an XCD that finishes early only hands its share of the HBM bandwidth to the others and shared segments cost L2 hits.  So
// the table is used where the bands would leave more than a tenth of the XCD slots idle (pair_use_map).
//
// ROW BANDS (k-windowed passes, nwin > 1; pair_row_bands).  Segment ids are window-major (Geom2::nsegw), so a run of ids puts ONE window of a
// set of rows on an XCD and the neighbouring windows of the same rows on others -- and those read the same lines: a window row is not a whole
// number of 128-byte lines, so the lines at every window boundary were fetched into two L2s.  Here the items are taken in (row segment,
// window, chunk) order before the cut: an XCD's run is every window of a band of row segments, walked chunk by chunk and inside a chunk by
// (row segment, window), so that the windows of the same rows start in the same round and share boundary lines and halo rows in one L2.
// The ids in the table stay window-major; nwin = 1 is the table above.  Cached per (nsegw, nwin, nchunk).
inline const int* pair_xcd_map(int nsegw, int nchunk, long long* nblk_out, int nwin = 1) {
  const long long key = ((long long)nwin << 48) | ((long long)nsegw << 24) | (unsigned)nchunk;
  auto it = ctx.pair_maps.find(key);
  if (it == ctx.pair_maps.end()) {
    const long long nseg = (long long)nsegw * nwin, T = nseg * nchunk;
    std::vector<std::vector<long long>> own(8);  // chunk << 42 | row segment << 21 | window, for the sort
    for (long long e = 0; e < T; e++) {
      const long long q = e / nchunk;  // row segment * nwin + window
      own[(size_t)(e * 8 / T)].push_back((e % nchunk) << 42 | (q / nwin) << 21 | (q % nwin));
    }
    size_t most = 0;
    for (auto& v : own) {
      std::sort(v.begin(), v.end());
      most = std::max(most, v.size());
    }
    std::vector<int> tab(2 * 8 * most);
    for (size_t r = 0; r < most; r++)
      for (int x = 0; x < 8; x++) {
        const bool has = r < own[x].size();
        const long long it3 = has ? own[x][r] : 0;
        tab[2 * (8 * r + x)] = has ? (int)((it3 & 0x1fffff) * nsegw + ((it3 >> 21) & 0x1fffff)) : (int)nseg;
        tab[2 * (8 * r + x) + 1] = (int)(it3 >> 42);
      }
    Ctx::PairMap pm;
    pm.nblk = (long long)(8 * most);
    HIP_CHECK(hipMalloc(&pm.dev, tab.size() * sizeof(int)));
    HIP_CHECK(hipMemcpy(pm.dev, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice));
    it = ctx.pair_maps.emplace(key, pm).first;
  }
  *nblk_out = it->second.nblk;
  return it->second.dev;
}

// (fewer than eight segments -- small planes, boxes long in j -- leave whole XCDs without a band: 40 x 2000 x 40 ran on ONE XCD, at 0.6 of the
// single-sweep rate, until round 3; profiles/r03/non_cubic_boxes.txt)
inline bool pair_use_map(int nseg) { return ctx.tune.t2_map && 10 * nseg < 9 * 8 * ((nseg + 7) / 8); }
// k-windowed passes take the row-band table whatever the balance of the bands (CZHIP_T2_MAP / t2_map: 1 = this, the default; 2 = the
// window-major order before it, where bands idle, for A/B measurements; 0 = whole-segment bands everywhere; profiles/r10/pass_planner.txt)
inline bool pair_row_bands(const Geom2& g) { return ctx.tune.t2_map == 1 && g.nwin > 1; }

// k windows of the two-stage pass (Geom2).  A window of KT vectors costs a workgroup (KT + 2) / KT in loads and first-stage work and leaves it
// rows of R = KT + 2 vectors, i.e. a useful share of (LV - 2R) / LV of its LV = TB MV vectors.  That product peaks near KT = sqrt(LV) = 45 --
// and the measurements say otherwise (profiles/r04/k_windows_sweep.txt): pieces of rows shorter than about 100 vectors (1.6 KB) cost more in
// memory efficiency than they save in redundant work (512^3 FP32, R = 129: two windows of 65 are 8 % SLOWER than whole rows), pieces of 129 to
// 176 vectors are the best everywhere they were tried: 512^3 FP64 (R = 258) 0.80 -> 0.655 ms per pass with two windows, 1024^3 FP32 (R = 257)
// 598 000 -> 820 000 MLUPS, rows of 2 104 FP32 / 1 104 FP64 elements (which took single sweeps until round 3) 790 000 / 410 000 MLUPS.  Rule:
// whole rows up to 192 vectors, else the fewest windows of at most 176.
constexpr int kPairWin = 176;
inline bool pair_whole_rows_ok(int Rfull, int /*LV*/) { return Rfull <= 192; }

// c1 .. c6 all exactly 1: the kernels may leave the six multiplications out (offdiag_sum<UNIT>, cz_k_common.h)
inline bool coef_is_unit(const Coef& c) {
  return c.c1 == (REAL)1 && c.c2 == (REAL)1 && c.c3 == (REAL)1 && c.c4 == (REAL)1 && c.c5 == (REAL)1 && c.c6 == (REAL)1;
}

// A multi-stage pass (jacobi2p_k, rb4_k, jac3_k, jac4_k, all on Geom2): what its launcher chooses, and what plan_pass makes of it
struct PassPlan {
  int TB = 0;             // threads per workgroup
  int own = 0;            // vectors a workgroup holds; S = own - halo_rows * R of them are its own
  int halo_rows = 2;
  int max_R = 0;          // longest row (window and halo vectors) a workgroup takes
  int kwin = 0;           // vectors per k window; 0: whole rows
  int hv = 1;             // halo vectors on either side of a window
  int wg_per_cu = 0;      // resident workgroups per CU for the chunk model; 0: as many as LDS and threads allow
  double extra = 3.5;     // plane steps a chunk costs beyond its own (pair_tj_model)
  int tj = 0;             // planes per chunk; 0: the model's choice
  bool long_chunks = false;  // the model may take chunks of more than 128 planes where that makes the launch one round (pair_tj_model)
  int nres = 2;           // residual slots per workgroup in ctx.partials
  int par = 0, zero_u = 0;
  // filled in by plan_pass
  Geom2 g;
  size_t lds = 0;
  int nchunk = 0;
};

// Geometry of a multi-stage pass over the output box b with the stage-1 box ba; lds_bytes(R, S) is the kernel's dynamic LDS.  Returns false
// where the geometry does not suit the kernel.  model_cost: the launch's cost by pair_tj_model, in plane steps x work per CU and step.
template <class LdsBytes>
bool plan_pass(PassPlan& p, const Box& b, const Box& ba, LdsBytes lds_bytes, double* model_cost = nullptr) {
  constexpr int V = VW;
  Geom2& g = p.g;
  g.R = (b.nkp + V - 1) / V;  // rows as vectors from a vector boundary each; the last one partial where nkp % V != 0 (Geom2)
  if (p.kwin > 0) {
    g.nwin = (g.R + p.kwin - 1) / p.kwin;
    g.KT = (g.R + g.nwin - 1) / g.nwin;
    g.hv = p.hv, g.KW = g.KT * V, g.R = g.KT + 2 * p.hv;
  }
  if (g.R > p.max_R) return false;
  g.PSV = (long long)g.R * b.nip;
  g.nkp = b.nkp;
  g.PSB = (long long)b.nkp * b.nip * (long long)sizeof(REAL);
  if (g.PSB >= (1LL << 32)) return false;  // 32-bit byte offsets inside a plane
  g.jlast = b.njp - 1;
  g.last_off = (unsigned)(g.PSB - (long long)sizeof(Vec<V>));
  g.kk0 = b.kk0, g.kk1 = b.kk1, g.jj0 = b.jj0, g.jj1 = b.jj1;
  g.F0 = (long long)b.ii0 * g.R;
  g.Fend = (long long)(b.ii1 + 1) * g.R;
  g.kk0a = ba.kk0, g.kk1a = ba.kk1, g.jj0a = ba.jj0, g.jj1a = ba.jj1;
  g.F0a = (long long)ba.ii0 * g.R;
  g.Fenda = (long long)(ba.ii1 + 1) * g.R;
  g.S = p.own - p.halo_rows * g.R;
  g.par = p.par, g.zero_u = p.zero_u;
  g.nsegw = (int)((g.Fend - g.F0 + g.S - 1) / g.S);
  g.nseg = g.nwin * g.nsegw;
  g.band = 1, g.map = nullptr;
  p.lds = lds_bytes(g.R, g.S);
  if (p.lds > 160 * 1024) return false;
  const int nplanes = b.jj1 - b.jj0 + 1;
  const int wg_per_cu = p.wg_per_cu > 0 ? p.wg_per_cu : std::max(1, std::min((int)(160 * 1024 / p.lds), 2048 / p.TB));
  int tj = p.tj;
  if (tj <= 0 || model_cost) {
    int best = 0;
    const double cost = pair_tj_model(g.nseg, nplanes, wg_per_cu, pair_row_bands(g) || pair_use_map(g.nseg), &best, p.extra, p.long_chunks);
    if (model_cost) *model_cost = cost * wg_per_cu * (double)(p.own + g.S);
    if (tj <= 0) tj = best;
  }
  g.TJ = std::min(tj, nplanes);
  p.nchunk = (nplanes + g.TJ - 1) / g.TJ;
  return true;
}

// Launch of a planned pass: workgroup order, partials, arrival counter; the kernel takes (U, B, W, c, g, partials, skip, fin, extra...)
template <typename... P, typename... A>
void launch_pass(void (*kernel)(P...), int label, PassPlan& p, const REAL* U, const REAL* B, REAL* W, const Coef& c, const int* skip, Fin2 fin,
                 const A&... extra) {
  long long nblk = 8LL * ((p.g.nseg + 7) / 8) * p.nchunk;
  if (pair_row_bands(p.g)) p.g.map = pair_xcd_map(p.g.nsegw, p.nchunk, &nblk, p.g.nwin);
  else if (pair_use_map(p.g.nseg)) p.g.map = pair_xcd_map(p.g.nseg, p.nchunk, &nblk);
  ensure_partials((size_t)p.nres * nblk);
  allow_dynamic_lds(kernel, 160 * 1024);
  fin.counter = ctx.counter;
  {
    ScopedTimer tm(label);
    hipLaunchKernelGGL(kernel, dim3((unsigned)nblk), dim3(p.TB), p.lds, ctx.stream, U, B, W, c, p.g, ctx.partials, skip, fin, extra...);
  }
  HIP_CHECK(hipGetLastError());
}

// two fused sweeps (jacobi2p_k); returns false when the geometry does not suit the kernel (caller falls back to two stencil_k launches)
template <int TB, int MV, int RB, int ZU, int MAF = 0, int BS = 0, int PRE = 0, int UNIT = 0>
bool launch_jacobi2_inst(const REAL* U, const REAL* B, REAL* W, const Coef& c, const Box& b, const Box& ba, int tj_req,
                         const int* skip, const Fin2& fin, int par, bool probe, double* model_cost, const MafArgs& ma = MafArgs(),
                         const BSrc& bs = BSrc()) {
  PassPlan p;
  p.TB = TB, p.own = TB * MV, p.par = par, p.zero_u = ZU;
  p.max_R = std::min(TB / 2, (TB * MV - 1) / 4);  // 2R <= TB: the outer rows are staged by 2R threads; 4R < TB MV: halo rows would dominate
  p.wg_per_cu = (MAF && TB == 512) ? 1 : 0;  // (MAF: a 512-thread workgroup of up to 256 registers per thread fills a CU's register file)
  p.tj = PRE ? PRE : tj_req;  // (the preloaded form, jacobi2p_k<PRE>: chunks of PRE planes)
  // k windows (Geom2): whole rows where a segment of them is a decent share of the workgroup's vectors, else windows of about kPairWin vectors;
  // CZHIP_T2_KWIN / ctx.tune.t2_kwin: > 0 = vectors per window, 0 = whole rows wherever they fit, -1 = this rule
  const int Rfull = (b.nkp + VW - 1) / VW;
  const bool whole_fits = Rfull <= p.max_R;
  int want = ctx.tune.t2_kwin;
  if (want < 0) want = (whole_fits && (pair_whole_rows_ok(Rfull, TB * MV) || BS)) ? 0 : kPairWin;  // (BS: the pass that makes its right-hand side reads
                                                                                                     // three or four arrays; the halo vectors of two windows cost it 6-8 % at 512^3 FP64)
  if (want == 0 && !whole_fits) want = kPairWin;
  if (want > 0 && want < Rfull) p.kwin = want;
  const auto lds_bytes = [](int R, int S) {
    return (size_t)2 * ((S + 4 * R) + (S + 2 * R)) * sizeof(Vec<VW>) + 18 * sizeof(double) +
           (MAF ? (size_t)2 * R * VW * sizeof(REAL) : 0);  // MAF: the table of the k metric terms
  };
  if (!plan_pass(p, b, ba, lds_bytes, model_cost)) return false;
  if (PRE) {
    // the preloaded form only where every workgroup of the pass is resident at once -- one workgroup per CU (its operands live in ~190
    // registers per thread) less the CUs left to the exchange stream of a decomposed run
    const long long slots = (long long)std::max(1, ctx.num_cu / 8 - ctx.cu_reserved) * 8;  // (one per CU also for the 256 x 1 shape: measured, profiles/r04/small_grids_preloaded_shapes.txt)
    if ((long long)p.g.nseg * p.nchunk > slots) return false;
  }
  if (probe) return true;
  launch_pass(&jacobi2p_k<VW, TB, MV, RB, ZU, MAF, BS, PRE, UNIT>, RB ? LBL_RBSOR2 : LBL_JACOBI2, p, U, B, W, c, skip, fin, ma, bs);
  return true;
}

template <int RB>
bool launch_jacobi2(const REAL* U, const REAL* B, REAL* W, const Coef& c, const Box& b, const Box& ba, const int* skip,
                    const Fin2& fin, int par = 0, int zero_u = 0, bool probe = false, const MafArgs* ma = nullptr, const BSrc* bs = nullptr, int bs_op = 0) {
  if (!rows_ok(b, {U, B, W})) return false;
  if (!ma && !fastdiv_ok(c.dd)) return false;  // jacobi2p_k divides by dd with the hoisted form (cz_k_fastdiv.h); odd magnitudes take single sweeps
  if (ma && b.g != 2) return false;             // the MAF kernels index the coordinate arrays with the padded index (GUIDE = 2)
  // the stage-1 box may exceed the output box by at most one layer per side
  if (ba.ii0 < b.ii0 - 1 || ba.ii0 > b.ii0 || ba.ii1 > b.ii1 + 1 || ba.ii1 < b.ii1 || ba.jj0 < b.jj0 - 1 || ba.jj0 > b.jj0 ||
      ba.jj1 > b.jj1 + 1 || ba.jj1 < b.jj1 || ba.kk0 < b.kk0 - 1 || ba.kk0 > b.kk0 || ba.kk1 > b.kk1 + 1 || ba.kk1 < b.kk1)
    return false;
  // the two-stage march reads two layers around the box
  if (b.ii0 < 2 || b.jj0 < 2 || b.ii1 > b.nip - 3 || b.jj1 > b.njp - 3) return false;
  const Tuning& tu = ctx.tune;
  // shape: 512 threads (two workgroups per CU) or 1024 threads (one, less redundant first-stage work); fixed by CZHIP_T2 or chosen by the
  // cost model of pair_tj_model
  int tb = tu.t2_threads;
  if (tb == 0) {
    double c512 = 0.0, c1024 = 0.0;
    const bool ok512 = launch_jacobi2_inst<512, 2, RB, 0>(U, B, W, c, b, ba, tu.t2_tj, skip, fin, par, true, &c512);
    const bool ok1024 = launch_jacobi2_inst<1024, 2, RB, 0>(U, B, W, c, b, ba, tu.t2_tj, skip, fin, par, true, &c1024);
    if (!ok512 && !ok1024) return false;
    tb = (ok512 && (!ok1024 || c512 <= c1024)) ? 512 : 1024;
  }
  if (ma) {  // MAF flavour (cz_maf.f90): weights recomputed per point from the 1-D grids.  Shape by measurement (profiles/r04/
             // register_spills_priced.txt; 512^3): the 512-thread form may use 256 registers per thread and spills nothing, the 1024-thread
             // form keeps 6-28 registers in scratch.  FP64 and the red-black pass: 512 threads (FP64 Jacobi 197 000 against 176 500 MLUPS,
             // red-black 115 600 against 93 200; FP32 red-black 181 800 / 182 500); FP32 Jacobi: 1024 threads, 6 registers in scratch and
             // all the same 352 600 against 273 900 MLUPS -- the spill is priced, the shape without it is slower.
    const bool first512 = tu.t2_threads == 512 || (tu.t2_threads == 0 && (sizeof(REAL) == 8 || RB));
    if (first512 && launch_jacobi2_inst<512, 2, RB, 0, 1>(U, B, W, c, b, ba, tu.t2_tj, skip, fin, par, probe, nullptr, *ma)) return true;
    return launch_jacobi2_inst<1024, 2, RB, 0, 1>(U, B, W, c, b, ba, tu.t2_tj, skip, fin, par, probe, nullptr, *ma);
  }
  if (zero_u && bs_op != 0) {  // the right-hand side made from the operands of the vector update before the solve (jacobi2p_k<BS>)
    if (!bs || !rows_ok(b, {bs->x, bs->y, bs->z, bs->out})) return false;
    if (bs_op == 1) {
      if (tb == 512) return launch_jacobi2_inst<512, 2, RB, 1, 0, 1>(U, B, W, c, b, ba, tu.t2_tj, skip, fin, par, probe, nullptr, MafArgs(), *bs);
      return launch_jacobi2_inst<1024, 2, RB, 1, 0, 1>(U, B, W, c, b, ba, tu.t2_tj, skip, fin, par, probe, nullptr, MafArgs(), *bs);
    }
    if (tb == 512) return launch_jacobi2_inst<512, 2, RB, 1, 0, 2>(U, B, W, c, b, ba, tu.t2_tj, skip, fin, par, probe, nullptr, MafArgs(), *bs);
    return launch_jacobi2_inst<1024, 2, RB, 1, 0, 2>(U, B, W, c, b, ba, tu.t2_tj, skip, fin, par, probe, nullptr, MafArgs(), *bs);
  }
  if (zero_u) {
    if (tb == 512) return launch_jacobi2_inst<512, 2, RB, 1>(U, B, W, c, b, ba, tu.t2_tj, skip, fin, par, probe, nullptr);
    return launch_jacobi2_inst<1024, 2, RB, 1>(U, B, W, c, b, ba, tu.t2_tj, skip, fin, par, probe, nullptr);
  }
  // small grids: the preloaded form (jacobi2p_k<PRE>) where the pass is at most one workgroup per CU.  Two shapes: 256 threads x 1 vector -- a
  // 64^3 pass cut into 512 x 2 pieces is 62 workgroups, three quarters of the CUs idle while the others grind through 2.4 us plane steps --
  // and 512 x 2 with its smaller share of halo rows for the grids that fill the chip either way; the first form of the list that fits is
  // the fastest at every size measured (32^3 .. 128^3, FP32 and FP64: 1.5x at 32^3 .. 64^3, 1.05-1.1x at 96^3 and 128^3; beyond that no form
  // fits and the pipelined one stays).  t2_pre: 1 = this rule,
  // 0 = never, TB * 10 + PRE = that form or none (measurements).  A fixed shape (CZHIP_T2=1,threads,2,tj with tj > 0) keeps the pipelined form.
  if (!probe && tu.t2_pre && tu.t2_tj == 0 && tu.t2_threads != 1024) {
#define CZ_PRE(TB_, MV_, PRE_) \
  if ((tu.t2_pre == 1 || tu.t2_pre == TB_ * 10 + PRE_) && launch_jacobi2_inst<TB_, MV_, RB, 0, 0, 0, PRE_>(U, B, W, c, b, ba, 0, skip, fin, par, false, nullptr)) return true;
    CZ_PRE(256, 1, 2) CZ_PRE(256, 1, 4) CZ_PRE(512, 2, 2) CZ_PRE(512, 2, 3) CZ_PRE(512, 2, 4)
#undef CZ_PRE
  }
  // unit coefficients (what CZ sets: cz.h:169-172): the Jacobi pair without the six multiplications per point -- 2-3 % at 512^3 FP32, where the
  // vector ALU is 77 % busy; the red-black pair is bound by memory and keeps one form (profiles/r04/unit_coefficients.txt)
  if (RB == 0 && tu.unit_coef && coef_is_unit(c)) {
    if (tb == 512) return launch_jacobi2_inst<512, 2, RB, 0, 0, 0, 0, 1>(U, B, W, c, b, ba, tu.t2_tj, skip, fin, par, probe, nullptr);
    return launch_jacobi2_inst<1024, 2, RB, 0, 0, 0, 0, 1>(U, B, W, c, b, ba, tu.t2_tj, skip, fin, par, probe, nullptr);
  }
  if (tb == 512) return launch_jacobi2_inst<512, 2, RB, 0>(U, B, W, c, b, ba, tu.t2_tj, skip, fin, par, probe, nullptr);
  return launch_jacobi2_inst<1024, 2, RB, 0>(U, B, W, c, b, ba, tu.t2_tj, skip, fin, par, probe, nullptr);
}

// rb4_k's two forms (launch_deep).  Named here, ahead of the division checks and UNIT = 0 first: the kernels keep their place in the code object.
// (unit coefficients: rb4_k is an arithmetic kernel -- vector ALU 93 % busy -- and the six multiplications are a fifth of a point's
// instructions: 6-7 % at 512^3 FP32, profiles/r04/unit_coefficients.txt)
constexpr int kDeepTB = 1024;
inline auto rb4_form(bool unit) { return !unit ? &rb4_k<VW, kDeepTB, 0> : &rb4_k<VW, kDeepTB, 1>; }

// numerators (of 2^32; see fastdiv_check_k) whose quotient by d in division form FORM (0 hoisted, 1 short, 2 medium, 3 / 4 the gated tail of the
// hoisted / medium form) differs from `n / d`; *compared = how many were compared (all of them but for the gated tails, which skip the huge ones)
template <int FORM>
long long div_check_count(REAL d, long long* compared = nullptr) {
  unsigned long long* out = nullptr;
  HIP_CHECK(hipMalloc(&out, 2 * sizeof(*out)));
  HIP_CHECK(hipMemsetAsync(out, 0, 2 * sizeof(*out), ctx.stream));
  hipLaunchKernelGGL(fastdiv_check_k<FORM>, dim3(4096), dim3(256), 0, ctx.stream, d, out);
  HIP_CHECK(hipGetLastError());
  unsigned long long h[2] = {0, 0};
  HIP_CHECK(hipMemcpyAsync(h, out, sizeof(h), hipMemcpyDeviceToHost, ctx.stream));
  HIP_CHECK(hipStreamSynchronize(ctx.stream));
  HIP_CHECK(hipFree(out));
  if (compared) *compared = (long long)h[1];
  return (long long)h[0];
}
// Does jac3_k divide by d with mediumdiv (cz_k_fastdiv.h: 8 instructions against 10)?  FP32 only, ctx.tune.jac3_medium.  Only a divisor whose
// quotients agree with `n / d` in every bit for all 2^32 numerators: the comparison runs once per context and divisor (a few ms, synchronous),
// at the first launch that needs it -- never inside a timed loop that has warmed up.
inline bool jac3_medium(REAL d) {
  if (sizeof(REAL) != 4 || !ctx.tune.jac3_medium || !fastdiv_ok(d)) return false;
  unsigned long long key = 0;
  memcpy(&key, &d, sizeof(REAL));
  auto it = ctx.medium_div.find(key);
  if (it == ctx.medium_div.end()) {
    long long bad = -1;
    if constexpr (sizeof(REAL) == 4) bad = div_check_count<2>(d);
    it = ctx.medium_div.emplace(key, bad == 0).first;
  }
  return it->second;
}

// the gated tail of the form jac3_k takes (medium: FP32 only) against `n / d`
inline long long gated_check(REAL d, bool med, long long* compared) {
  if constexpr (sizeof(REAL) == 4) {
    if (med) return div_check_count<4>(d, compared);
  }
  return div_check_count<3>(d, compared);
}
// Does jac3_k divide by d in the gated form (GatedDiv, cz_k_pass.h) of the division it takes, medium or hoisted?  ctx.tune.jac3_gate, and only
// a divisor whose gated tail agreed with `n / d` in every bit for all numerators below the threshold (FP32: all 2^32 floats; FP64: the 2^32
// sampled doubles the hoisted form rests on): once per context, divisor and form, synchronous, at the first launch that needs it.
inline bool jac3_gated(REAL d, bool med) {
  if (!ctx.tune.jac3_gate || !fastdiv_ok(d)) return false;
  unsigned long long key = 0;
  memcpy(&key, &d, sizeof(REAL));
  auto& verdicts = ctx.gated_div[med ? 1 : 0];
  auto it = verdicts.find(key);
  if (it == verdicts.end()) it = verdicts.emplace(key, gated_check(d, med, nullptr) == 0).first;
  return it->second;
}

// ------------------------------------------------------------------------------------------------------------
// The DEEP passes -- rb4_k (two red-black iterations), jac3_k, jac4_k (three, four Jacobi sweeps) per pass over memory: single-domain boxes,
// constant coefficients, 1 024 threads with one vector each (deep_lds, cz_k_pass.h).  One launcher (launch_deep); what differs between the
// passes is a row of kDeepPass, and the measurements that justify a row's constants stand above it.
// do the 256-thread preloaded forms of the one-iteration pass (launch_jacobi2: small grids) take this box?  Where they do they beat rb4_k
// (32^3 .. 80^3: rb4_k 0.67-0.85 x; from 96^3 on, where they no longer fit, 1.00-1.16 x: profiles/r04/rb4_two_iterations_per_pass.txt)
inline bool pair_small_form_fits(const Box& b) {
  if (!ctx.tune.t2_pre || ctx.tune.t2_tj != 0 || ctx.tune.t2_threads == 1024) return false;
  const int R = (b.nkp + VW - 1) / VW;
  if (4 * R >= 256) return false;
  const long long S = 256 - 2 * R, nf = (long long)(b.ii1 - b.ii0 + 1) * R, nseg = (nf + S - 1) / S;
  const int nplanes = b.jj1 - b.jj0 + 1;
  const long long slots = (long long)std::max(1, ctx.num_cu / 8 - ctx.cu_reserved) * 8;
  return nseg * ((nplanes + 1) / 2) <= slots || nseg * ((nplanes + 3) / 4) <= slots;
}
inline int rb4_window(int Rfull) { return VW == 4 ? (Rfull < 115 ? 26 : 48) : 28; }
inline int jac3_window(int) { return VW == 4 ? 26 : 36; }
inline int jac4_window(int) { return 26; }
constexpr int kRb4Win = 48;
// size gate of jac3 = 1: inner points of the box (256^3: no gain worth the switch; 384^3: 1.11 x)
constexpr long long kJac3MinPoints = 300LL * 300 * 300;
constexpr long long kJac4MinPoints = kJac3MinPoints;

enum DeepKind { DEEP_RB4 = 0, DEEP_JAC3 = 1, DEEP_JAC4 = 2 };
struct DeepPass {
  int label;                  // timing label
  int halo_rows;              // 2 (D - 1) for a pass of D stages: S = TB - halo_rows * R vectors of a workgroup are its own
  int max_R;                  // longest row of a workgroup's view: the halo rows must stay a small share of its 1 024 vectors
  int hv;                     // halo vectors on either side of a k window: D stages reach D - 1 (red-black: 3) elements beyond it
  double extra;               // plane steps a chunk costs beyond its own: the redundant planes and the prologue (pair_tj_model)
  int nres;                   // residual sums per workgroup
  bool long_chunks;           // pair_tj_model may take chunks of more than 128 planes where the launch is then one round
  int (*window)(int Rfull);   // vectors per k window where the switch forces none
  int whole_rows;             // ... and rows up to this many vectors (and the halo) then stay whole; 0: up to the window itself
  long long min_points;       // size gate of switch = 1: inner points of the box
  bool needs_t2;              // only where the driver may fuse Jacobi sweeps at all (use_t2)
  bool fp64;                  // built for FP64 as well
  DeepSwitch Tuning::*sw;     // its switches
  DeepSwitch Tuning::*needs;  // the pass that has to be switched on as well (or null)
};
const DeepPass kDeepPass[3] = {
    // rb4_k (cz_k_rb4.h); refused: the caller runs two fused iterations, jacobi2p_k<RB = 1>.  The k axis is cut into windows of about kRb4Win
    // vectors whatever the row length: the six halo rows of a segment must stay a small share of the 1 024 vectors a workgroup holds (max_R:
    // at least a quarter of them must be its own).  extra: six redundant planes and a longer prologue per chunk.
    // Window length by measurement (profiles/r04/rb4_two_iterations_per_pass.txt; 128^3 .. 1024^3): FP32 rows up to 50 vectors whole (128^3,
    // 192^3: 1.12 x / 1.25 x the one-iteration pass), rows of 65 / 97 vectors in windows of 22 / 25 (1.14 x / 1.28 x; windows of 33 give 1.02 x /
    // 1.09 x), rows of 129 / 257 in windows of 43 (1.15-1.19 x; 26 and 33 give 1.10 x); FP64 anything from 20 to 33 (1.25-1.32 x).
    {LBL_RBSOR4, 6, kDeepTB / 8, VW == 4 ? 1 : 2, 7.5, 2, false, rb4_window, kRb4Win, 0, false, true, &Tuning::rb4, nullptr},
    // jac3_k (cz_k_jac3.h); refused, or below the size gate: the caller runs the two-sweep pass.  Four halo rows (max_R: at least half of the
    // workgroup's vectors must be its own); extra: four redundant planes and a longer prologue per chunk.
    // By measurement (profiles/r06/jac3_three_sweeps_per_pass.txt), per sweep against the pair: FP32 windows of 26 vectors 1.09 x at 512^3 (43:
    // 1.01 x, 20: 0.98 x), 1.11 x at 384^3, 1.07 x at 1024^3, 1.01 x at 256^3; FP64 512^3 windows of 36 1.22 x (28: 1.19 x, 20: 1.11 x).
    // Re-swept with the shorter FP32 division (profiles/r08/jac3_fetch_split_and_medium_division.txt): no window or gate beats these beyond noise.
    {LBL_JACOBI3, 4, kDeepTB / 8, VW == 4 ? 1 : 2, 5.5, 3, true, jac3_window, 0, kJac3MinPoints, true, true, &Tuning::jac3, nullptr},
    // jac4_k (cz_k_jac4.h): the boxes jac3_k takes, under the same gates; refused: the caller runs the three-sweep pass.  FP32 only: the FP64
    // instantiations need 12-16 bytes of scratch per lane at 128 registers, so FP64 keeps jac3_k (profiles/r26).  Six halo rows (max_R: at
    // least half of the vectors its own); four stages reach four elements beyond a window: one FP32 vector.
    // By measurement (profiles/r26/jac4_four_sweeps_per_pass.txt; FP32, ms per sweep against jac3_k under its own rule):
    //   window   512^3: 26 vectors 0.1156 (1.088 x jac3_k), 20: 0.1164, 32: 0.1157, 43: 0.1292 (0.974 x: S = 754, 18 row segments, two rounds);
    //            384^3: 26: 0.0543 (1.099 x), 32: 0.0545; 1024^3: 26: 0.9671 (1.075 x), 32: 0.9826.  Rule: 26, jac3_k's window.
    //   chunks   512^3: the one-round plan of pair_tj_model with long_chunks (3 chunks of 170 planes, 255 workgroups) 0.1156, chunks of 64: 0.1294,
    //            of 32: 0.1482; 1024^3: the model's choice 0.9671, chunks of 128: 0.9792.  Rule: the model, with extra = 7.5 plane steps per chunk
    //            (six redundant planes and the prologue, rb4_k's figure for the same depth; not swept on its own -- the model's choices above
    //            were the fastest chunk lengths tried at every size).
    //   size     256^3: 0.0210 against 0.0204 (0.97 x); 384^3: 1.105 x; 512^3: 1.088 x; 1024^3: 1.075 x.  Nothing was measured between 256^3 and
    //            384^3, so the gate is jac3_k's (below which the issue allows none): 300^3 inner points.
    {LBL_JACOBI4, 6, kDeepTB / 12, 1, 7.5, 4, true, jac4_window, 0, kJac4MinPoints, true, false, &Tuning::jac4, &Tuning::jac3},
};

// The eight forms of a Jacobi kernel K by unit coefficients, division (MED: FP32 only) and its gated form.  The ungated instantiations are
// named first, UNIT = 0 before UNIT = 1: they keep their place in the code object.
#define CZ_JAC_FORMS(K)                                                                \
  kernel = !unit ? &K<VW, TB, 0, 0> : &K<VW, TB, 1, 0>;                                \
  if constexpr (sizeof(REAL) == 4) {                                                   \
    if (med) kernel = !unit ? &K<VW, TB, 0, 1> : &K<VW, TB, 1, 1>;                     \
  }                                                                                    \
  if (gate) {                                                                          \
    kernel = !unit ? &K<VW, TB, 0, 0, 1> : &K<VW, TB, 1, 0, 1>;                        \
    if constexpr (sizeof(REAL) == 4) {                                                 \
      if (med) kernel = !unit ? &K<VW, TB, 0, 1, 1> : &K<VW, TB, 1, 1, 1>;             \
    }                                                                                  \
  }

// Plans and launches the deep pass `kind` u -> w over the box b (par: the colour parity of rb4_k).  Returns false where the pass is switched
// off, the box lies below its gates or the geometry does not suit the kernel.  probe: plan only; plan_out receives the plan.
bool launch_deep(DeepKind kind, const REAL* U, const REAL* B, REAL* W, const Coef& c, const Box& b, const int* skip, Fin2 fin, int par, bool probe,
                 PassPlan* plan_out = nullptr) {
  constexpr int TB = kDeepTB;
  const DeepPass& d = kDeepPass[kind];
  const Tuning& tu = ctx.tune;
  const DeepSwitch& sw = tu.*d.sw;
  if ((sizeof(REAL) == 8 && !d.fp64) || !sw.on || (d.needs && !(tu.*d.needs).on) || !tu.fuse_fin || (d.needs_t2 && !tu.use_t2)) return false;
  // arrays of any REAL alignment, a dd that takes the hoisted division, and two layers between the box and the array's i, j edges
  if (!rows_ok(b, {U, B, W}) || !fastdiv_ok(c.dd) || b.ii0 < 2 || b.jj0 < 2 || b.ii1 > b.nip - 3 || b.jj1 > b.njp - 3) return false;
  const long long npts = (long long)(b.ii1 - b.ii0 + 1) * (b.jj1 - b.jj0 + 1) * (b.kk1 - b.kk0 + 1);
  if (sw.on == 1 && (npts < d.min_points || pair_small_form_fits(b))) return false;  // (2: also there -- measurements and tests)
  PassPlan p;
  p.TB = TB, p.own = TB, p.halo_rows = d.halo_rows, p.max_R = d.max_R, p.hv = d.hv;
  p.wg_per_cu = 1, p.extra = d.extra, p.tj = sw.tj, p.nres = d.nres, p.long_chunks = d.long_chunks, p.par = par;
  const int Rfull = (b.nkp + VW - 1) / VW;
  const int want = sw.kwin > 0 ? sw.kwin : d.window(Rfull);
  if (Rfull > ((sw.kwin > 0 || !d.whole_rows) ? want : d.whole_rows) + 2 * p.hv) p.kwin = want;
  const int depth = d.halo_rows / 2 + 1;
  if (!plan_pass(p, b, b, [depth](int R, int) { return deep_lds_bytes<VW>(TB, depth, R); })) return false;
  if (plan_out) *plan_out = p;
  if (probe) return true;
  fin.single = 0;
  const bool unit = tu.unit_coef && coef_is_unit(c);
  auto kernel = rb4_form(unit);
  if (kind != DEEP_RB4) {
    const bool med = jac3_medium(c.dd), gate = jac3_gated(c.dd, med);
    CZ_JAC_FORMS(jac3_k)
    if constexpr (sizeof(REAL) == 4) {
      if (kind == DEEP_JAC4) { CZ_JAC_FORMS(jac4_k) }
    }
  }
  launch_pass(kernel, d.label, p, U, B, W, c, skip, fin);
  return true;
}
#undef CZ_JAC_FORMS

// the shell boxes of a decomposed brick, all in one launch (pair_shell_k); boxes: n x (ist,ied,jst,jed,kst,ked), 1-based
template <int RB, int MAF = 0>
void launch_pair_shell(const REAL* U, const REAL* B, REAL* W, const Coef& c, const int* sz, int g, const Box& ba, const int* boxes, int n,
                       int par, const int* skip, hipStream_t st, const MafArgs& ma = MafArgs()) {
  ShellTab s;
  s.n = n;
  int most_tiles = 0;
  size_t lds = 0;
  for (int m = 0; m < n; m++) {
    const Box b = make_box(sz, boxes + 6 * m, g);
    if (b.empty || b.ii0 < 2 || b.jj0 < 2 || b.kk0 < 2 || b.ii1 > b.nip - 3 || b.jj1 > b.njp - 3 || b.kk1 > b.nkp - 3) {
      cz_fatal(1, "czhip: pair_shell: box %d is empty or closer than two cells to the array edge\n", m);
    }
    ShellBox& d = s.b[m];
    d.i0 = b.ii0, d.j0 = b.jj0, d.k0 = b.kk0;
    d.ni = b.ii1 - b.ii0 + 1, d.nj = b.jj1 - b.jj0 + 1, d.nk = b.kk1 - b.kk0 + 1;
    // tile shape by orientation: long in k (coalesced rows) unless k is the thin axis
    int tk, ti, tj;
    if (d.nk == 2) d.kind = 2, tk = 2, ti = 16, tj = 16;
    else if (d.nj == 2) d.kind = 0, tk = 64, ti = 4, tj = 2;
    else if (d.ni == 2) d.kind = 1, tk = 64, ti = 2, tj = 4;
    else d.kind = 3, tk = 32, ti = 4, tj = 4;
    d.ntk = (d.nk + tk - 1) / tk, d.nti = (d.ni + ti - 1) / ti, d.ntj = (d.nj + tj - 1) / tj;
    most_tiles = std::max(most_tiles, d.ntk * d.nti * d.ntj);
    lds = std::max(lds, sizeof(REAL) * ((size_t)(tk + 4) * (ti + 4) * (tj + 4) + (size_t)(tk + 2) * (ti + 2) * (tj + 2)));
  }
  s.ii0a = ba.ii0, s.ii1a = ba.ii1, s.jj0a = ba.jj0, s.jj1a = ba.jj1, s.kk0a = ba.kk0, s.kk1a = ba.kk1;
  s.nkp = ba.nkp, s.nip = ba.nip, s.njp = ba.njp;
  s.par = par;
  const unsigned gx = (unsigned)std::min(most_tiles, 2048);
  {
    ScopedTimer tm(LBL_SHELL, st);
    hipLaunchKernelGGL((pair_shell_k<RB, MAF>), dim3(gx, (unsigned)n), dim3(256), lds, st, U, B, W, c, s, ctx.shell_partials, skip, ma);
  }
  HIP_CHECK(hipGetLastError());
  ctx.shell_pending = (int)(gx * n);
}

Coef make_coef(const REAL* cf, REAL omg) {
  Coef c;
  c.c1 = cf[0], c.c2 = cf[1], c.c3 = cf[2], c.c4 = cf[3], c.c5 = cf[4], c.c6 = cf[5], c.dd = cf[6], c.omg = omg;
  return c;
}

template <int V, int OP>
void launch_ewise_inst(REAL* Z, const REAL* X, const REAL* Y, REAL a, REAL bcoef, const Box& b, const REAL* a_dev, const REAL* b_dev) {
  EGeom e = make_egeom<V>(b);
  e.pa = a_dev, e.pb = b_dev;
  dim3 grid((unsigned)((e.Fend - e.F0 + 255) / 256), (unsigned)(b.jj1 - b.jj0 + 1));
  hipLaunchKernelGGL((ewise_k<V, OP>), grid, dim3(256), 0, ctx.stream, Z, X, Y, a, bcoef, e);
}

template <int OP>
void launch_ewise(REAL* Z, const REAL* X, const REAL* Y, REAL a, REAL bcoef, const Box& b, const REAL* a_dev = nullptr, const REAL* b_dev = nullptr) {
  if (b.empty) return;
  ScopedTimer tm(LBL_EWISE);
  if (rows_ok(b, {Z, X, Y})) launch_ewise_inst<VW, OP>(Z, X, Y, a, bcoef, b, a_dev, b_dev);
  else launch_ewise_inst<1, OP>(Z, X, Y, a, bcoef, b, a_dev, b_dev);
  HIP_CHECK(hipGetLastError());
}

template <int V, int TWO>
void launch_dot_inst(const REAL* X, const REAL* Y, const Box& b, double* dst) {
  const int nplanes = b.jj1 - b.jj0 + 1;
  EGeom e = make_egeom<V>(b);
  const unsigned gx = (unsigned)((e.Fend - e.F0 + 255) / 256);
  const unsigned gy = (unsigned)std::max(1, std::min(nplanes, (int)(4096 / gx)));
  ensure_partials((size_t)gx * gy);
  hipLaunchKernelGGL((dot_k<V, TWO>), dim3(gx, gy), dim3(256), 0, ctx.stream, X, Y, e, nplanes, ctx.partials, dst, ctx.counter);
}

// dot -> device double dst[0]
template <int TWO>
void launch_dot(const REAL* X, const REAL* Y, const Box& b, double* dst) {
  if (b.empty) {
    HIP_CHECK(hipMemsetAsync(dst, 0, sizeof(double), ctx.stream));
    return;
  }
  ScopedTimer tm(LBL_DOT);
  if (rows_ok(b, {X, Y})) launch_dot_inst<VW, TWO>(X, Y, b, dst);
  else launch_dot_inst<1, TWO>(X, Y, b, dst);
  HIP_CHECK(hipGetLastError());
}

double read_scalar(int slot) {
  HIP_CHECK(hipMemcpyAsync(ctx.scal_host + slot, ctx.scal_dev + slot, sizeof(double), hipMemcpyDeviceToHost, ctx.stream));
  HIP_CHECK(hipStreamSynchronize(ctx.stream));
  return ctx.scal_host[slot];
}

inline double npts(const int* idx) {
  return (double)(idx[1] - idx[0] + 1) * (double)(idx[3] - idx[2] + 1) * (double)(idx[5] - idx[4] + 1);
}

// Host evaluation of the Dirichlet table sin(pi*x)*sin(pi*y), cz_solver.f90:36,52-58.
// ioff/joff: brick offset in global cells (head-1).  The reference evaluates x = org + dh*real(i-1) with the BRICK
// origin org = G_origin + (head-1)*dh (cz_Evaluate.cpp:136-138), which rounds differently from the single-domain
// x = G_origin + dh*real(i_global-1); the driver passes the global origin plus an integer offset instead so that a
// decomposed run carries bit-identical Dirichlet data (ioff = joff = 0 reproduces the reference expression exactly).
REAL* bc_table(int ix, int jx, REAL dh, const REAL* org, int ioff = 0, int joff = 0) {
  std::vector<double> key = {(double)ix, (double)jx, (double)dh, (double)org[0], (double)org[1], (double)ioff, (double)joff};
  auto it = ctx.bc_tabs.find(key);
  if (it != ctx.bc_tabs.end()) return it->second;
  std::vector<REAL> tab((size_t)ix * jx);
  volatile REAL one = (REAL)1.0;  // keep asin() a run-time libm call like the rest
#ifdef CZ_REAL_IS_DOUBLE
  const REAL pi = 2.0 * asin(one);
#else
  const REAL pi = 2.0f * asinf(one);
#endif
  for (int j = 1; j <= jx; j++)
    for (int i = 1; i <= ix; i++) {
      const REAL x = org[0] + dh * (REAL)(ioff + i - 1);
      const REAL y = org[1] + dh * (REAL)(joff + j - 1);
#ifdef CZ_REAL_IS_DOUBLE
      tab[(size_t)(j - 1) * ix + (i - 1)] = sin(pi * x) * sin(pi * y);
#else
      tab[(size_t)(j - 1) * ix + (i - 1)] = sinf(pi * x) * sinf(pi * y);
#endif
    }
  REAL* d = nullptr;
  HIP_CHECK(hipMalloc(&d, tab.size() * sizeof(REAL)));
  HIP_CHECK(hipMemcpy(d, tab.data(), tab.size() * sizeof(REAL), hipMemcpyHostToDevice));
  ctx.bc_tabs[key] = d;
  return d;
}
