// cz_h_mg.h -- part of cz_kernels.hip (ONE translation unit per precision; this file is included at its end, at file scope, and is
// not a stand-alone header): host side of the multigrid V-cycle preconditioner of PCG: the launches of the level kernels
// (cz_k_mg.h), the hierarchy handle cz_mg and its operations for the order of a cycle (cz_mg_cycle.h).
using czhip_internal::MgdLevel;

namespace {
// f(std::bool_constant...) for the flags given: the launches below name a kernel's instantiation once, with the flags as template arguments
template <class F>
void with_flags(F&& f) {
  f();
}
template <class F, class... Rest>
void with_flags(F&& f, bool flag, Rest... rest) {
  if (flag) with_flags([&](auto... c) { f(std::true_type(), c...); }, rest...);
  else with_flags([&](auto... c) { f(std::false_type(), c...); }, rest...);
}

// the device description of a level from the host one; false if it does not describe level M.level of a grid of M.n0 points
bool mg_lev(MgDLev& D, const MgdLevel& M) {
  MgLev& L = D.L;
  if (M.dense) {
    L.nip = M.sz[0], L.nkp = M.sz[2], L.i0 = L.j0 = L.k0 = 0;
    L.ni = M.sz[0], L.nj = M.sz[1], L.nk = M.sz[2];
  } else {
    const Box b = make_box(M.sz, M.idx, M.g);
    if (b.empty) return false;
    L.nip = b.nip, L.nkp = b.nkp, L.i0 = b.ii0, L.j0 = b.jj0, L.k0 = b.kk0;
    L.ni = b.ii1 - b.ii0 + 1, L.nj = b.jj1 - b.jj0 + 1, L.nk = b.kk1 - b.kk0 + 1;
  }
  if (M.level < 0 || M.level >= MG_MAXLEV - 1) return false;
  L.l = M.level, L.n0i = M.n0[0], L.n0j = M.n0[1], L.n0k = M.n0[2];
  L.nm = M.level >= 1 ? M.nm & 63 : 0;  // (level 0 keeps 1 and 6: there the mirrored face layer carries the condition)
  D.o = MgG{M.o[0], M.o[1], M.o[2]};
  D.gni = M.gn[0], D.gnj = M.gn[1], D.gnk = M.gn[2];
  const int n[3] = {L.ni, L.nj, L.nk};
  const long long s = 1LL << M.level;
  for (int d = 0; d < 3; d++)
    if (M.n0[d] < 1 || (M.n0[d] + s - 1) / s != M.gn[d] || M.o[d] < 0 || n[d] < 0 || M.o[d] + n[d] > M.gn[d]) return false;
  return true;
}
bool mg_none(const MgDLev& D) { return D.L.ni < 1 || D.L.nj < 1 || D.L.nk < 1; }
bool mg_whole(const MgDLev& D) { return !(D.o.i | D.o.j | D.o.k) && D.L.ni == D.gni && D.L.nj == D.gnj && D.L.nk == D.gnk; }
bool mg_coarse_of(const MgdLevel& F, const MgdLevel& C) { return C.level == F.level + 1 && std::equal(F.n0, F.n0 + 3, C.n0); }

// a whole level in one array: the inner box of (sz, idx, g) is the level
MgdLevel mg_array_level(const int* sz, const int* idx, int g, int level, const int* n0) {
  MgdLevel M = MgdLevel();
  std::copy(sz, sz + 3, M.sz);
  std::copy(idx, idx + 6, M.idx);
  M.g = g, M.level = level;
  for (int d = 0; d < 3; d++) M.n0[d] = n0[d], M.gn[d] = idx[2 * d + 1] - idx[2 * d] + 1;
  return M;
}

// the LDS layout of the levels from fine (level l) down to the coarsest: one zero shell per array, b, x, t per level (rb: b and x, the
// red-black iterations run in place)
// (bc: level `fine`'s value of MgdLevel::nm, wrap bits included -- every level of the tail takes its own from it, mg_level_bc; -1: fine.nm)
bool mg_tail_plan(MgTail& T, const MgLev& fine, REAL omg, bool rb = false, int bc = -1) {
  T = MgTail();
  T.gl = fine, T.omg = omg;
  const int n[3] = {fine.ni, fine.nj, fine.nk};
  int dims[MG_TAIL_MAXLEV][3];
  T.nlev = mg_level_dims(n, dims, MG_TAIL_MAXLEV);
  if (!T.nlev) return false;
  for (int m = 0; m < T.nlev; m++) {
    MgLev& s = T.s[m] = fine;
    s.ni = dims[m][0], s.nj = dims[m][1], s.nk = dims[m][2], s.l = fine.l + m;
    s.nm = czhip_internal::mg_level_bc((bc < 0 ? fine.nm : bc) & 63, bc < 0 ? 0 : bc >> 6, dims[m]);
    s.nip = s.ni + 2, s.nkp = s.nk + 2, s.i0 = s.j0 = s.k0 = 1;
    T.len[m] = (s.ni + 2) * (s.nj + 2) * (s.nk + 2);
    T.off[m] = T.total;
    T.total += (rb ? 2 : 3) * T.len[m];
    if ((long long)T.total * (long long)sizeof(REAL) > 160 * 1024) return false;
  }
  return true;
}

// (NM: the level kernels' instantiation for a level with Neumann faces, chosen here from the level's mask -- cz_k_mg.h, mg_weights)
// (PER: some level of the tail wraps a periodic direction, DESIGN.md §5.15.  A level of one point in such a direction carries mask bits that
// the finer levels do not, so both flags are taken over every level of the tail; without a periodic direction that is T.gl.nm)
// (the weight arrays keep their zero faces: no mask, so no NM)
template <bool RB, bool PER, class WT>
void mg_tail_launch(REAL* x, const REAL* b, const MgTail& T, const WT& W) {
  ScopedTimer tm(LBL_MG_TAIL);
  const int bytes = T.total * (int)sizeof(REAL);
  if (bytes > 64 * 1024) allow_dynamic_lds(&mg_tail_k<RB, PER, WT>, 160 * 1024);
  hipLaunchKernelGGL((mg_tail_k<RB, PER, WT>), dim3(1), dim3(MG_TAIL_THREADS), bytes, ctx.stream, x, b, T, W);
  HIP_CHECK(hipGetLastError());
}
// W: the weight arrays of the tail's levels; nullptr: the integers
void mg_tail_launch(REAL* x, const REAL* b, const MgTail& T, bool rb, const MgcTail* W = nullptr) {
  int any = 0;
  for (int m = 0; m < T.nlev; m++) any |= T.s[m].nm;
  with_flags([&](auto RB, auto PER, auto NM) {  // (PER: one instantiation per smoother, a mask of zero gives the unmasked bits)
    if (W) mg_tail_launch<RB(), PER()>(x, b, T, *W);
    else mg_tail_launch<RB(), PER()>(x, b, T, MgConstTail<NM() || PER()>());
  }, rb, (any >> 6) != 0, (any & 63) != 0);
}

dim3 mg_grid(const MgLev& L) { return dim3((unsigned)((L.nk + 63) / 64), (unsigned)((L.ni + 3) / 4), (unsigned)L.nj); }
// level 0's row kernels under coefficients: a streaming grid of about 2048 workgroups (8 per CU), strided over the planes and the vectors of
// a plane's rows; slots: the vectors a row can touch, whatever its phase
int mgc0_slots(const MgLev& L) { return (L.nk + 2 * VW - 2) / VW; }
bool mgc0_rows(const MgLev& L) { return L.l == 0 && (long long)L.ni * mgc0_slots(L) < 0x7ff00000LL; }
dim3 mgc0_grid(const MgLev& L) {
  const unsigned gy = (unsigned)std::min(L.nj, 2048);
  const long long per_plane = ((long long)L.ni * mgc0_slots(L) + 255) / 256;
  return dim3((unsigned)std::max<long long>(1, std::min<long long>(per_plane, 2048 / gy)), gy);
}
// f(the weights of a level as the level kernels take them): the arrays cw where given (cw.d), else the integers, masked where the level
// has Neumann faces (NM: cz_k_mg.h, mg_weights)
template <class F>
void with_weights(const MgcW& cw, const MgLev& L, F&& f) {
  if (cw.d) f(MgArr{cw});
  else with_flags([&](auto NM) { f(MgConst<NM()>()); }, L.nm != 0);
}
// f(std::integral_constant<int, z>) for the from-zero form z = 0, 1, 2 of a colour sweep
template <class F>
void with_zero_form(int z, F&& f) {
  if (z == 0) f(std::integral_constant<int, 0>());
  else if (z == 1) f(std::integral_constant<int, 1>());
  else f(std::integral_constant<int, 2>());
}

// ---- the launches of the level kernels: 0 = refused (nothing launched).  cw: the level's weight arrays; cw.d == nullptr:
// the integers.  Under the arrays level 0 is a level like the others, swept by its row kernels (cz_k_mgc.h) under the labels of the constant
// cycle's level 0 (jacobi, rbsor)
int mg_smooth_launch(const REAL* u, REAL* w, const REAL* b, const MgdLevel& M, REAL omg, const MgcW& cw) {
  MgDLev D;
  if (!w || !b || u == w || !mg_lev(D, M) || M.dense) return 0;
  if (mg_none(D)) return 1;
  ScopedTimer tm(cw.d && M.level == 0 ? LBL_JACOBI : LBL_MG_SMOOTH);
  with_flags([&](auto ZERO) {
    if (cw.d && mgc0_rows(D.L))
      hipLaunchKernelGGL((mgc0_smooth_k<VW, ZERO()>), mgc0_grid(D.L), dim3(256), 0, ctx.stream, u ? u : w, w, b, D.L, cw, omg, mgc0_slots(D.L));
    else
      with_weights(cw, D.L, [&](auto W) {
        hipLaunchKernelGGL((mg_smooth_k<ZERO(), decltype(W)>), mg_grid(D.L), dim3(64, 4), 0, ctx.stream, u ? u : w, w, b, D, omg, W);
      });
  }, !u);
  HIP_CHECK(hipGetLastError());
  return 1;
}

// (a whole level only: the colour is that of the global index, and a cut would need an exchange per colour.  Level 0: under the arrays only)
int mg_rb_launch(REAL* x, const REAL* b, const MgdLevel& M, REAL omg, int colour, int zero, const MgcW& cw) {
  MgDLev D;
  if (!x || !b || x == b || !mg_lev(D, M) || M.dense || !mg_whole(D) || (M.level < 1 && !cw.d) || (colour | 1) != 1 || zero < 0 || zero > 2) return 0;
  if (mg_none(D)) return 1;
  ScopedTimer tm(cw.d && M.level == 0 ? LBL_RBSOR : LBL_MG_RB);
  const dim3 grid((unsigned)(((D.L.nk + 1) / 2 + 63) / 64), (unsigned)((D.L.ni + 3) / 4), (unsigned)D.L.nj);
  with_zero_form(zero, [&](auto Z) {
    if (cw.d && mgc0_rows(D.L))
      hipLaunchKernelGGL((mgc0_rb_k<VW, Z()>), mgc0_grid(D.L), dim3(256), 0, ctx.stream, x, b, D.L, cw, omg, colour, mgc0_slots(D.L));
    else
      with_weights(cw, D.L, [&](auto W) { hipLaunchKernelGGL((mg_rb_k<Z(), decltype(W)>), grid, dim3(64, 4), 0, ctx.stream, x, b, D.L, omg, colour, W); });
  });
  HIP_CHECK(hipGetLastError());
  return 1;
}

// rt = nullptr: every child is a point of F's own array, which then is the whole level (the weight arrays: that case only)
int mg_restrict_launch(REAL* bc, const MgdLevel& MC, const REAL* x, const REAL* b, const REAL* rt, const MgdLevel& MF, const MgcW& cw) {
  MgDLev F, C;
  if (!bc || !x || !b || bc == x || bc == b || !mg_lev(F, MF) || !mg_lev(C, MC) || MF.dense || !mg_coarse_of(MF, MC) || (!rt && !(mg_whole(F) && mg_whole(C))) || (rt && cw.d)) return 0;
  if (mg_none(C)) return 1;
  ScopedTimer tm(LBL_MG_RESTRICT);
  // (the children's residual takes the FINE level's weights: its mask)
  if (cw.d) hipLaunchKernelGGL(mgc_restrict_k, mg_grid(C.L), dim3(64, 4), 0, ctx.stream, bc, x, b, F.L, C.L, cw);  // (its own frame: cz_k_mgc.h)
  else
    with_flags([&](auto RT, auto NM) { hipLaunchKernelGGL((mg_restrict_k<RT(), MgConst<NM()>>), mg_grid(C.L), dim3(64, 4), 0, ctx.stream, bc, x, b, rt, F, C, MgConst<NM()>()); },
               rt != nullptr, F.L.nm != 0);
  HIP_CHECK(hipGetLastError());
  return 1;
}
}  // namespace

namespace czhip_internal {
int mg_smooth_async(const REAL* u, REAL* w, const REAL* b, const MgdLevel& M, REAL omg) { return mg_smooth_launch(u, w, b, M, omg, MgcW()); }
int mg_rb_async(REAL* x, const REAL* b, const MgdLevel& M, REAL omg, int colour, int zero) { return mg_rb_launch(x, b, M, omg, colour, zero, MgcW()); }
int mg_restrict_async(REAL* bc, const MgdLevel& MC, const REAL* x, const REAL* b, const REAL* rt, const MgdLevel& MF) {
  return mg_restrict_launch(bc, MC, x, b, rt, MF, MgcW());
}

int mgd_resface_async(REAL* rt, const REAL* x, const REAL* b, const MgdLevel& M, const int* minus) {
  MgDLev D;
  if (!rt || !x || !b || rt == x || !mg_lev(D, M) || M.dense) return 0;
  if (mg_none(D)) return 1;
  ScopedTimer tm(LBL_MG_RESTRICT);
  for (int d = 0; d < 3; d++) {
    if (!minus[d]) continue;
    const int fast = d == 2 ? D.L.ni : D.L.nk, slow = d == 0 ? D.L.nj : d == 1 ? D.L.ni : D.L.nj;
    const dim3 grid((unsigned)((fast + 63) / 64), (unsigned)slow);
    with_flags([&](auto NM) { hipLaunchKernelGGL(mgd_resface_k<NM()>, grid, dim3(64), 0, ctx.stream, rt, x, b, D, d, minus[0], minus[1]); }, D.L.nm != 0);
    HIP_CHECK(hipGetLastError());
  }
  return 1;
}

int mg_prolong_async(REAL* u, const REAL* x, const REAL* xc, const MgdLevel& MC, const MgdLevel& MF) {
  MgDLev F, C;
  if (!u || !x || !xc || u == xc || !mg_lev(F, MF) || !mg_lev(C, MC) || MF.dense || MC.dense || !mg_coarse_of(MF, MC)) return 0;
  if (mg_none(F)) return 1;
  ScopedTimer tm(LBL_MG_PROLONG);
  hipLaunchKernelGGL(mg_prolong_k, mg_grid(F.L), dim3(64, 4), 0, ctx.stream, u, x, xc, F, C);
  HIP_CHECK(hipGetLastError());
  return 1;
}

int mgd_unpack_async(REAL* X, const MgdLevel& MG, const REAL* blk, const int* o, const int* cnt) {
  MgDLev G;
  if (!X || !blk || !mg_lev(G, MG) || MG.dense) return 0;
  for (int d = 0; d < 3; d++)
    if (o[d] < 0 || cnt[d] < 0 || o[d] + cnt[d] > MG.gn[d]) return 0;
  const long long n = (long long)cnt[0] * cnt[1] * cnt[2];
  if (n == 0) return 1;
  hipLaunchKernelGGL(mgd_unpack_k, dim3((unsigned)std::min<long long>((n + 255) / 256, 1024)), dim3(256), 0, ctx.stream, X, blk, G.L,
                     MgG{o[0], o[1], o[2]}, cnt[0], cnt[1], cnt[2]);
  HIP_CHECK(hipGetLastError());
  return 1;
}
}  // namespace czhip_internal

extern "C" {
int czhip_mg_smooth_async(const CZ_REAL* u, CZ_REAL* w, const CZ_REAL* b, const int* sz, const int* idx, int g, int level, const int* n0, CZ_REAL omg) {
  ensure_init();
  return czhip_internal::mg_smooth_async(u, w, b, mg_array_level(sz, idx, g, level, n0), omg);
}

int czhip_mg_restrict_async(CZ_REAL* bc, const int* szc, const int* idxc, const CZ_REAL* x, const CZ_REAL* b, const int* sz, const int* idx, int g, int level,
                            const int* n0) {
  ensure_init();
  return czhip_internal::mg_restrict_async(bc, mg_array_level(szc, idxc, g, level + 1, n0), x, b, nullptr, mg_array_level(sz, idx, g, level, n0));
}

int czhip_mg_prolong_async(CZ_REAL* u, const CZ_REAL* x, const CZ_REAL* xc, const int* szc, const int* idxc, const int* sz, const int* idx, int g, int level,
                           const int* n0) {
  ensure_init();
  return czhip_internal::mg_prolong_async(u, x, xc, mg_array_level(szc, idxc, g, level + 1, n0), mg_array_level(sz, idx, g, level, n0));
}

int czhip_mg_tail_async(CZ_REAL* x, const CZ_REAL* b, const int* sz, const int* idx, int g, int level, const int* n0, CZ_REAL omg) {
  ensure_init();
  MgDLev D;
  MgTail T;
  if (!x || !b || x == b || !mg_lev(D, mg_array_level(sz, idx, g, level, n0)) || !mg_tail_plan(T, D.L, omg)) return 0;
  mg_tail_launch(x, b, T, false);
  return 1;
}

int czhip_mg_rb_async(CZ_REAL* x, const CZ_REAL* b, const int* sz, const int* idx, int g, int level, const int* n0, CZ_REAL omg, int colour, int zero) {
  ensure_init();
  return czhip_internal::mg_rb_async(x, b, mg_array_level(sz, idx, g, level, n0), omg, colour, zero);
}

int czhip_mg_tail_rb_async(CZ_REAL* x, const CZ_REAL* b, const int* sz, const int* idx, int g, int level, const int* n0, CZ_REAL omg) {
  ensure_init();
  MgDLev D;
  MgTail T;
  if (!x || !b || x == b || level < 1 || !mg_lev(D, mg_array_level(sz, idx, g, level, n0)) || !mg_tail_plan(T, D.L, omg, true)) return 0;
  mg_tail_launch(x, b, T, true);
  return 1;
}
}  // extern "C"

// ---- the hierarchy
namespace czhip_internal {
cz_mg* mg_create(const int* n0, int l0, bool tail, const int* sz0, const int* idx0, bool rb) {
  cz_mg* h = new cz_mg();
  h->rb = rb;
  int dims[MG_MAXLEV][3];
  h->first = l0, h->nlev = mg_level_dims(n0, dims, MG_MAXLEV - 1);
  bool ok = std::min(n0[0], std::min(n0[1], n0[2])) >= 1 && l0 >= 0 && l0 < h->nlev;
  for (int l = l0; ok && l < h->nlev; l++) {  // ceil(n / 2) points per direction, inner box 2 .. n + 1 inside zero faces at 1 and n + 2
    const int* n = dims[l];
    const int sz[3] = {n[0] + 2, n[1] + 2, n[2] + 2}, idx[6] = {2, n[0] + 1, 2, n[1] + 1, 2, n[2] + 1};
    h->lev[l] = l ? mg_array_level(sz, idx, MG_GUIDE, l, n0) : mg_array_level(sz0, idx0, MG_GUIDE, 0, n0);
    MgDLev D;
    ok = mg_lev(D, h->lev[l]);
    if (ok && l) h->b[l] = czhip_alloc_s3d(sz), h->x[l] = czhip_alloc_s3d(sz);
    if (ok && l && !rb) h->t[l] = czhip_alloc_s3d(sz);
  }
  if (!ok) {
    czhip_mg_destroy(h);
    return nullptr;
  }
  if (l0 == 0) {
    h->fine_tmp = czhip_alloc_s3d(sz0);
    HIP_CHECK(hipMalloc(&h->res, 4 * sizeof(double)));
  }
  // the tail starts at the first level >= 1 whose levels down to the coarsest fit one workgroup's LDS (tail off: none)
  h->tail_from = h->nlev;
  for (int l = std::max(l0, 1); tail && l < h->nlev; l++) {
    MgDLev D;
    MgTail T;
    mg_lev(D, h->lev[l]);
    if (mg_tail_plan(T, D.L, (REAL)1, rb)) {
      h->tail_from = l;
      break;
    }
  }
  return h;
}
}  // namespace czhip_internal

namespace {
cz_mg* mg_create_public(const int* sz, const int* idx, int g, const CZ_REAL* cf, bool rb) {
  ensure_init();
  if (g != MG_GUIDE) return nullptr;  // (the coarse arrays and the temporary are S3D arrays: guide 2)
  for (int c = 0; c < 6; c++)
    if (cf[c] != (REAL)1) return nullptr;
  if (cf[6] != (REAL)6) return nullptr;
  const int n0[3] = {idx[1] - idx[0] + 1, idx[3] - idx[2] + 1, idx[5] - idx[4] + 1};
  const CzConfig cfg = CzConfig::from_env();
  cz_mg* h = czhip_internal::mg_create(n0, 0, cfg.on(CZV_MG_TAIL, true), sz, idx, rb);
  if (h) h->zero4 = cfg.on(CZV_MGRB_ZERO4, true);  // (measured: profiles/r12/mgrb.txt)
  return h;
}
}  // namespace
extern "C" {
cz_mg* czhip_mg_create(const int* sz, const int* idx, int g, const CZ_REAL* cf) { return mg_create_public(sz, idx, g, cf, false); }
cz_mg* czhip_mg_create_rb(const int* sz, const int* idx, int g, const CZ_REAL* cf) { return mg_create_public(sz, idx, g, cf, true); }

int czhip_mg_levels(const cz_mg* h) { return h ? h->nlev : 0; }
}  // extern "C"

// ---- face coefficients inside the hierarchy (cz_k_mgc.h): the weights of a level for the launches above, and the build
namespace {
// (the constant hierarchy: no arrays -- the launches take the integers)
MgcW mgc_w(const cz_mg* h, int l) { return h->coef ? MgcW{h->cw[0][l], h->cw[1][l], h->cw[2][l], h->cd[l]} : MgcW(); }
MgLev mgc_lev(const cz_mg* h, int l) {
  MgDLev D;
  if (!mg_lev(D, h->lev[l])) cz_fatal(1, "czhip: V-cycle: level %d has no description\n", l);
  return D.L;
}
void mgc_free(cz_mg* h) {
  for (int l = 0; l < MG_MAXLEV; l++) {
    for (int d = 0; d < 3; d++) {
      if (l && h->cw[d][l]) czhip_free(const_cast<REAL*>(h->cw[d][l]));
      h->cw[d][l] = nullptr;
    }
    if (h->cd[l]) czhip_free(h->cd[l]);
    h->cd[l] = nullptr;
  }
  if (h->cbad) (void)hipFree(h->cbad);
  h->cbad = nullptr;
  h->coef = h->coef_bad = 0;
}

// every level's weights and diagonal under the hierarchy's boundary state, from level 0's weights; one host wait for the count.  false: some
// coarse weight or diagonal is not finite and positive (h->coef_bad)
bool mgc_build(cz_mg* h) {
  HIP_CHECK(hipMemsetAsync(h->cbad, 0, sizeof(unsigned), ctx.stream));
  for (int l = 0; l < h->nlev; l++) {
    const MgLev L = mgc_lev(h, l);
    if (l) {
      const MgLev F = mgc_lev(h, l - 1);
      const dim3 grid((unsigned)((L.nk + 1 + 63) / 64), (unsigned)((L.ni + 1 + 3) / 4), (unsigned)(L.nj + 1));
      hipLaunchKernelGGL(mgc_coarsen_k, grid, dim3(64, 4), 0, ctx.stream, const_cast<REAL*>(h->cw[0][l]), const_cast<REAL*>(h->cw[1][l]),
                         const_cast<REAL*>(h->cw[2][l]), h->cw[0][l - 1], h->cw[1][l - 1], h->cw[2][l - 1], F, L, h->cbad);
      HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(mgc_diag_k, mg_grid(L), dim3(64, 4), 0, ctx.stream, h->cd[l], h->cw[0][l], h->cw[1][l], h->cw[2][l], L, l ? h->cbad : nullptr);
    HIP_CHECK(hipGetLastError());
  }
  unsigned bad = 0u;
  HIP_CHECK(hipMemcpyAsync(&bad, h->cbad, sizeof(unsigned), hipMemcpyDeviceToHost, ctx.stream));
  HIP_CHECK(hipStreamSynchronize(ctx.stream));
  h->coef_bad = bad != 0u;
  return bad == 0u;
}

// ---- zebra line iterations along Z (cz_k_mgline.h)
// a level takes them where it has X or Y links: a level of one row is its own line and keeps the point sweeps (in the closed box that line
// is the whole singular operator)
bool mg_line_level(const cz_mg* h, int l) { return (long long)h->lev[l].gn[0] * h->lev[l].gn[1] > 1; }
// the rows of one colour as mg_line_k numbers them, and the REALs of one scratch table
MgLine mg_line_plan(const MgLev& L) {
  MgLine P = MgLine();
  P.mh = (L.ni + 1) / 2, P.rows = L.nj * P.mh;
  P.pitch = (long long)((L.nk + VW - 1) / VW) * VW;
  return P;
}
unsigned mg_line_blocks(const MgLine& P) { return (unsigned)((P.rows + MGL_ROWS - 1) / MGL_ROWS); }
size_t mg_line_table(const cz_mg* h) {
  size_t n = 0;
  for (int l = h->first; l < h->nlev; l++) {
    if (!mg_line_level(h, l)) continue;
    const MgLine P = mg_line_plan(mgc_lev(h, l));
    n = std::max(n, (size_t)mg_line_blocks(P) * MGL_ROWS * (size_t)P.pitch);
  }
  return n;
}
// one sweep of colour `colour` of level l in place; zero as mg_rb_launch's.  An end is folded at level 0 on a zero-flux Z face (the level's
// word has no such bit while Z is periodic)
int mg_line_launch(cz_mg* h, REAL* x, const REAL* b, int l, REAL omg, int colour, int zero, const MgcW& cw) {
  MgDLev D;
  const MgdLevel& M = h->lev[l];
  if (!x || !b || x == b || !cw.d || !h->line_s[0] || !mg_lev(D, M) || M.dense || !mg_whole(D) || (colour | 1) != 1 || zero < 0 || zero > 2) return 0;
  if (mg_none(D)) return 1;
  if ((long long)D.L.nj * ((D.L.ni + 1) / 2) > 0x7fffff00LL) return 0;
  ScopedTimer tm(M.level == 0 ? LBL_RBSOR : LBL_MG_RB);
  MgLine P = mg_line_plan(D.L);
  P.c = colour;
  P.fold = M.level == 0 ? (M.nm >> 4) & 3 : 0;
  with_zero_form(zero, [&](auto Z) {
    hipLaunchKernelGGL((mg_line_k<VW, Z()>), dim3(mg_line_blocks(P)), dim3(MGL_ROWS), 0, ctx.stream, x, b, D.L, cw, omg, P, h->line_s[0], h->line_s[1]);
  });
  HIP_CHECK(hipGetLastError());
  return 1;
}
void mg_line_free(cz_mg* h) {
  for (REAL*& a : h->line_s) {
    if (a) (void)hipFree(a);
    a = nullptr;
  }
  h->lines = 0;
}
}  // namespace

extern "C" {
int czhip_mg_line_chunk(void) { return MGL_CHUNK; }

int czhip_mg_set_lines(cz_mg* h, int on) {
  if (!h || !h->rb || (on | 1) != 1) return 0;
  ensure_init();
  if (!on) {
    if (h->lines) czhip_sync();
    mg_line_free(h);
    return 1;
  }
  if (h->lines) return 1;
  const size_t n = std::max<size_t>(mg_line_table(h), 1);
  for (REAL*& a : h->line_s) HIP_CHECK(hipMalloc(&a, n * sizeof(REAL)));
  h->lines = 1;
  return 1;
}
}  // extern "C"

namespace czhip_internal {
// every level's word from the state (mg_level_bc; without a periodic direction: the Neumann flags at every level, as before there were
// any).  The arrays whose ghost layers carried the mirrors or wraps of an earlier state are zeros again, as the unmasked passes read them
void mg_set_bc(cz_mg* h, CzBc bc) {
  int wraps = bc.per;
  for (int l = h->first; l < h->nlev; l++) wraps |= h->lev[l].nm >> 6;
  h->bc = bc;
  for (int l = h->first; l < h->nlev; l++) h->lev[l].nm = mg_level_bc(bc, h->lev[l].gn);
  if (h->fine_tmp) {
    const int* sz = h->lev[0].sz;
    HIP_CHECK(hipMemsetAsync(h->fine_tmp, 0, (size_t)(sz[0] + 4) * (sz[1] + 4) * (sz[2] + 4) * sizeof(REAL), ctx.stream));
  }
  for (int l = std::max(h->first, 1); wraps && l < h->nlev; l++)  // (levels >= 1 have ghost layers other than zero only under a wrap)
    for (REAL* a : {h->x[l], h->t[l]})
      if (a) HIP_CHECK(hipMemsetAsync(a, 0, (size_t)(h->lev[l].sz[0] + 4) * (h->lev[l].sz[1] + 4) * (h->lev[l].sz[2] + 4) * sizeof(REAL), ctx.stream));
  if (h->coef && !mgc_build(h)) {  // (the zeroed faces follow the state.  A bad coarse value: the constant hierarchy again, and the
    mgc_free(h);                   // verdict waits in h->coef_bad for whoever set the coefficients)
    h->coef_bad = 1;
  }
}
}  // namespace czhip_internal

extern "C" {

// zero-flux (Neumann) faces for the hierarchy's cycles from now on (faces[6]: X-, X+, Y-, Y+, Z-, Z+; all zero: none); 0 = refused (NULL).
// All six are accepted: D = Wx cx + Wy cy + Wz cz vanishes only at a point that is first and last in all three directions, and the coarsest
// level keeps at least 3 points along its longest direction
int czhip_mg_set_neumann(cz_mg* h, const int* faces) {
  if (!h || !faces) return 0;
  czhip_internal::mg_set_bc(h, h->bc.with_faces(faces));
  return 1;
}

// periodic directions for the hierarchy's cycles from now on (dirs[3]: X, Y, Z; all zero: none); 0 = refused (NULL).  The Neumann
// flags of a periodic direction are ignored while it is periodic
int czhip_mg_set_periodic(cz_mg* h, const int* dirs) {
  if (!h || !dirs) return 0;
  czhip_internal::mg_set_bc(h, h->bc.with_dirs(dirs));
  return 1;
}
int czhip_mg_kind(const cz_mg* h) { return h ? 1 + h->rb : 0; }

// face coefficients inside the hierarchy: bx, by, bz are level 0's face weights, device arrays in the layout of the
// level-0 arrays that stay the caller's; all three NULL: the constant hierarchy again.  1, or 0: refused (a NULL handle, some but not all
// three, a hierarchy without level 0), or a coarse weight or diagonal that is not finite and positive -- the constant hierarchy again
int czhip_mg_set_coef(cz_mg* h, const CZ_REAL* bx, const CZ_REAL* by, const CZ_REAL* bz) {
  ensure_init();
  const int given = (bx != nullptr) + (by != nullptr) + (bz != nullptr);
  if (!h || (given != 0 && given != 3) || h->first != 0) return 0;
  if (given == 0) {
    if (h->coef || h->cd[0]) {
      czhip_sync();
      mgc_free(h);
    }
    return 1;
  }
  h->cw[0][0] = bx, h->cw[1][0] = by, h->cw[2][0] = bz;
  if (!h->cbad) HIP_CHECK(hipMalloc(&h->cbad, sizeof(unsigned)));
  for (int l = 0; l < h->nlev; l++) {
    if (!h->cd[l]) h->cd[l] = czhip_alloc_s3d(h->lev[l].sz);
    for (int d = 0; l && d < 3; d++)
      if (!h->cw[d][l]) h->cw[d][l] = czhip_alloc_s3d(h->lev[l].sz);
  }
  h->coef = 1;
  if (mgc_build(h)) return 1;
  mgc_free(h);
  return 0;
}

void czhip_mg_destroy(cz_mg* h) {
  if (!h) return;
  czhip_sync();
  mgc_free(h);
  mg_line_free(h);
  for (int l = 0; l < MG_MAXLEV; l++)
    for (REAL* a : {h->b[l], h->x[l], h->t[l]})
      if (a) czhip_free(a);
  if (h->fine_tmp) czhip_free(h->fine_tmp);
  if (h->res) (void)hipFree(h->res);
  delete h;
}
}  // extern "C"

namespace {
// the face layers of a level-0 array: the mirror of the first inner layer on its Neumann faces, the wrap in its periodic
// directions, in one launch
void mg_mirror(cz_mg* h, REAL* x) {
  if (!czhip_internal::fill_bc_async(x, h->lev[0].sz, h->lev[0].idx, MG_GUIDE, h->lev[0].nm, true)) cz_fatal(1, "czhip: V-cycle: the mirror of the Neumann faces was refused\n");
}
// the wrap of a level >= 1 array's ghost layers in the level's periodic directions (nothing without one): before every kernel that reads
// the array's neighbours.  The masked diagonal needs no mirror there
bool mg_wraps(const cz_mg* h, int l) { return (h->lev[l].nm >> 6) != 0; }
void mg_wrap(cz_mg* h, int l, REAL* x) {
  if (!czhip_internal::fill_bc_async(x, h->lev[l].sz, h->lev[l].idx, MG_GUIDE, h->lev[l].nm, false)) cz_fatal(1, "czhip: V-cycle: the wrap of a periodic level was refused\n");
}

// level 0's pairs of sweeps with the unit coefficients, u -> w (u = nullptr: from zero): the fused pass, or where it is not taken two single
// sweeps through o (an array other than w; it may be u) and a copy back to w
// (Neumann faces: two single sweeps, the face layers mirrored before each sweep that reads its input -- DESIGN.md §5.13)
void mg_fine_pair(cz_mg* h, REAL* u, REAL* w, REAL* o, const REAL* b, REAL omg) {
  const int* sz = h->lev[0].sz;
  const int* idx = h->lev[0].idx;
  REAL cf[7] = {1, 1, 1, 1, 1, 1, 6};
  if (!h->lev[0].nm && (u ? czhip_jacobi2_async(u, w, b, sz, idx, nullptr, MG_GUIDE, cf, omg, h->res, 0.0, 0.0, 0, nullptr, nullptr, nullptr, nullptr)
                   : czhip_jacobi2_from_zero_async(w, w, b, sz, idx, nullptr, MG_GUIDE, cf, omg, h->res)))
    return;
  const size_t nbytes = (size_t)(sz[0] + 4) * (sz[1] + 4) * (sz[2] + 4) * sizeof(REAL);
  if (!u) {
    HIP_CHECK(hipMemsetAsync(o, 0, nbytes, ctx.stream));
    u = o;
  } else if (h->lev[0].nm) {
    mg_mirror(h, u);
  }
  czhip_jacobi_async(u, w, b, sz, idx, MG_GUIDE, cf, omg, h->res, 0, nullptr);
  if (h->lev[0].nm) mg_mirror(h, w);
  czhip_jacobi_async(w, o, b, sz, idx, MG_GUIDE, cf, omg, h->res, 0, nullptr);
  HIP_CHECK(hipMemcpyAsync(w, o, nbytes, hipMemcpyDeviceToDevice, ctx.stream));
}

// the operations of mg_walk on one domain, for the constant hierarchy and for the one with face coefficients inside (the
// same order, fills and from-zero forms; mgc_w gives a level's weight arrays, or none).  A level keeps b, x and a temporary t of its own
// (mgrb: no t); level 0's are r, x0 and o0.  Every level >= 1, and level 0 under coefficients, is swept by the level kernels, and its
// iterate never changes array: mg's sweeps go through the temporary and come back, mgrb's colour sweeps and the prolongation run in place.
// The constant cycle's level 0 (fine) takes the solvers' fused passes instead, which cannot run in place: its iterate is in x0, or not yet
// anywhere, and the next one goes to o0 -- its pair and its prolongation hand the iterate over
struct MgOps {
  cz_mg* h;
  REAL omg;
  const REAL* r;
  REAL *x0, *o0;

  bool fine(int l) const { return l == 0 && !h->coef; }
  REAL* x(int l) { return l ? h->x[l] : x0; }
  REAL* t(int l) { return l ? h->t[l] : o0; }
  const REAL* b(int l) { return l ? h->b[l] : r; }
  // what an array of the level needs before a kernel reads its neighbours: level 0 the mirrors and wraps of its face layers, levels >= 1 the wraps
  bool fills(int l) const { return l ? mg_wraps(h, l) : h->lev[0].nm != 0; }
  void fill(int l, REAL* a) {
    if (l) mg_wrap(h, l, a);
    else if (h->lev[0].nm) mg_mirror(h, a);
  }
  void mirror(REAL* X) { mg_mirror(h, X); }
  static void must(int launched) {
    if (!launched) cz_fatal(1, "czhip: V-cycle: a level kernel refused its level\n");
  }
  // line iterations are in force under the coefficients only; the tail kernel has no line form
  bool lines() const { return h->lines && h->coef && h->rb; }
  bool whole(int l) {
    if (l < h->tail_from || lines()) return false;
    MgTail T;
    MgcTail W = MgcTail();
    mg_tail_plan(T, mgc_lev(h, l), omg, h->rb, h->lev[l].nm);
    for (int m = 0; h->coef && m < T.nlev; m++) W.g[m] = mgc_lev(h, l + m), W.w[m] = mgc_w(h, l + m);
    mg_tail_launch(h->x[l], h->b[l], T, h->rb, h->coef ? &W : nullptr);
    return true;
  }
  // ---- mgrb.  Level 0 takes the red-black passes that exist (two iterations per pass where the planner takes the box, else one per pass, else
  // the colour sweeps in place); ofst 0 runs colour 0 first, ofst 1 colour 1.  moves: how often such a pair hands the iterate to the other array
  int fine_rb_moves(bool zero) const {
    const int* sz = h->lev[0].sz;
    const int* idx = h->lev[0].idx;
    const REAL cf[7] = {1, 1, 1, 1, 1, 1, 6};
    if (h->lev[0].nm) return 0;  // (Neumann faces: the colour sweeps in place, a mirror after each)
    if ((!zero || h->zero4) && czhip_rbsor4_async(x0, o0, r, sz, idx, MG_GUIDE, cf, 0, omg, h->res, 0.0, 0.0, 0, nullptr, nullptr, nullptr, nullptr, 1)) return 1;
    return czhip_internal::pair_probe(x0, o0, r, sz, idx, idx, MG_GUIDE, (REAL)6, 0) ? 2 : 0;
  }
  void fine_rb_pair(bool zero, bool post) {
    const int* sz = h->lev[0].sz;
    const int* idx = h->lev[0].idx;
    const REAL cf[7] = {1, 1, 1, 1, 1, 1, 6};
    const int ofst = post ? 1 : 0, moves = fine_rb_moves(zero);
    if (zero && moves != 2) HIP_CHECK(hipMemsetAsync(x0, 0, (size_t)(sz[0] + 4) * (sz[1] + 4) * (sz[2] + 4) * sizeof(REAL), ctx.stream));
    if (moves == 1) {
      must(czhip_rbsor4_async(x0, o0, r, sz, idx, MG_GUIDE, cf, ofst, omg, h->res, 0.0, 0.0, 0, nullptr, nullptr, nullptr, nullptr, 0));
      std::swap(x0, o0);
    } else if (moves == 2) {
      for (int it = 0; it < 2; it++) {
        must(zero && it == 0 ? czhip_jacobi2_from_zero_made_async(x0, o0, const_cast<REAL*>(r), 0, nullptr, nullptr, nullptr, (REAL)0, (REAL)0, sz, idx, nullptr, MG_GUIDE, cf,
                                                                  omg, ofst, h->res, 0)
                             : czhip_rbsor2_async(x0, o0, r, sz, idx, nullptr, MG_GUIDE, cf, ofst, omg, h->res, 0.0, 0.0, 0, nullptr, nullptr, nullptr, nullptr));
        std::swap(x0, o0);
      }
    } else {
      // (Neumann faces: the ghost of a cell is read by that cell alone, so one mirror after every colour sweep serves the next one; the
      // prolongation moved the iterate to an array whose face layers are stale)
      if (h->lev[0].nm && !zero) mirror(x0);
      for (int s = 0; s < 4; s++) {
        czhip_rbsor_async(x0, r, sz, idx, MG_GUIDE, cf, ofst, s & 1, omg, h->res, 0, nullptr);
        if (h->lev[0].nm) mirror(x0);
      }
    }
  }
  // level 0's iterate must end in z: how many times the walk moves it
  int fine_moves() const {
    if (!h->rb) return h->nlev == 1 ? 4 : 3;
    return h->nlev == 1 ? fine_rb_moves(true) + 3 * fine_rb_moves(false) : fine_rb_moves(true) + 1 + fine_rb_moves(false);
  }

  void fine_pair(bool zero, bool post) {
    if (h->rb) return fine_rb_pair(zero, post);
    mg_fine_pair(h, zero ? nullptr : x0, o0, x0, r, omg);
    std::swap(x0, o0);
  }

  void pair(int l, bool zero, bool post) {
    if (fine(l)) return fine_pair(zero, post);
    const MgcW cw = mgc_w(h, l);
    if (h->rb) {
      // (a level that is filled: a fill after every colour sweep serves the next one, and the first one after the prolongation.  On an odd
      // periodic extent the seam points share a colour and the ghost holds the value from before the sweep; from zero that value is a zero,
      // so the array is cleared and swept as an iterate -- the bits of the literal zeros)
      const int c0 = post ? 1 : 0;
      const bool f = fills(l);
      if (f && zero) {
        const int* sz = h->lev[l].sz;
        HIP_CHECK(hipMemsetAsync(x(l), 0, (size_t)(sz[0] + 4) * (sz[1] + 4) * (sz[2] + 4) * sizeof(REAL), ctx.stream));
      } else if (f) {
        fill(l, x(l));
      }
      const bool line = lines() && cw.d && mg_line_level(h, l);  // (zebra lines along Z: the same order, fills and from-zero forms)
      for (int s = 0; s < 4; s++) {
        const int colour = (c0 + s) & 1, form = zero && s < 2 && !f ? s + 1 : 0;
        must(line ? mg_line_launch(h, x(l), b(l), l, omg, colour, form, cw) : mg_rb_launch(x(l), b(l), h->lev[l], omg, colour, form, cw));
        fill(l, x(l));
      }
      return;
    }
    if (!zero) fill(l, x(l));
    must(mg_smooth_launch(zero ? nullptr : x(l), t(l), b(l), h->lev[l], omg, cw));
    fill(l, t(l));
    must(mg_smooth_launch(t(l), x(l), b(l), h->lev[l], omg, cw));
  }
  void restrict_down(int l) {
    if (!h->rb) fill(l, x(l));  // (mgrb: filled after its last colour sweep)
    must(mg_restrict_launch(h->b[l + 1], h->lev[l + 1], x(l), b(l), nullptr, h->lev[l], mgc_w(h, l)));
  }
  void prolong_up(int l) {
    must(czhip_internal::mg_prolong_async(fine(l) ? o0 : x(l), x(l), h->x[l + 1], h->lev[l + 1], h->lev[l]));
    if (fine(l)) std::swap(x0, o0);
  }
};
}  // namespace

namespace czhip_internal {
int mg_cycle_async(cz_mg* h, REAL omg) {
  if (!h || h->first < 1) return 0;  // (level 0 needs the arrays of czhip_mg_apply_async)
  MgOps ops{h, omg, nullptr, nullptr, nullptr};
  mg_walk(ops, h->first, h->nlev - 1);
  return 1;
}
}  // namespace czhip_internal

extern "C" {
int czhip_mg_apply_async(cz_mg* h, CZ_REAL* z, const CZ_REAL* r, CZ_REAL omg) {
  ensure_init();
  if (!h || h->first != 0 || !z || !r || z == r || z == h->fine_tmp) return 0;
  // the constant cycle's level 0 changes array with every step: pair, prolongation, pair, or the coarsest level's four pairs (mgrb: a pair
  // moves it once, twice or not at all).  The last step writes z.  Under coefficients the iterate stays in z
  MgOps ops{h, omg, r, z, h->fine_tmp};
  if (!h->coef && (ops.fine_moves() & 1)) std::swap(ops.x0, ops.o0);
  mg_walk(ops, 0, h->nlev - 1);
  return 1;
}
}  // extern "C"
