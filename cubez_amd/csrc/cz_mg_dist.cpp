// cz_mg_dist.cpp -- the V-cycle of pcg ... mg on a decomposed domain ("Decomposed runs"): bit for bit the single-domain
// cycle of czhip_mg_apply_async.
//
// Aggregation stays global; a brick owns coarse point I of level l when it owns the aggregate's first level-0 point (comm_mg_own).
//   level 0        the brick's fine arrays, decomposed Jacobi sweeps (czhip_jacobi_async, one face exchange before every sweep that reads
//                  its input)
//   1 .. G-1       distributed: each brick holds its owned points in an array with the fine brick's inner-range convention and its own
//                  CommCtx; a face exchange before every sweep that reads its input, the residual of the first owned layer on the - faces
//                  exchanged over faces, edges and corners for the children on the + neighbours, the coarse iterate exchanged the same way
//                  for the parents on the - neighbours
//   G .. coarsest  the owned blocks of b_G all-gathered (an exact copy) into a global level-G array on every rank; the single-domain level
//                  kernels and mg_tail_k run there redundantly, and the prolongation from G reads its parents from that copy.
// G = the first level at which some brick owns no point in some direction, the coarsest level, or the first level of at most CZ_MG_GATHER
// global points, whichever comes first (never below 1).  Every G gives the same bits.
#include <algorithm>
#include <vector>

#include "cz_comm.h"
#include "cz_driver.h"

using namespace czhip_internal;

struct MgDist {
  int nlev = 0, G = 0, nproc = 1;
  int n0[3] = {0, 0, 0};
  int gn[MG_DIST_MAXLEV][3];
  MgdLevel lev[MG_DIST_MAXLEV];    // distributed levels 0 .. G-1 (level 0: the driver's arrays)
  MgdLevel blk;                    // this brick's owned block of level G (dense: the all-gather's send buffer)
  MgdLevel glev[MG_DIST_MAXLEV];   // the global levels G .. nlev-1
  CommCtx* comm[MG_DIST_MAXLEV] = {};  // level 0: the driver's; 1 .. G-1 own ones
  int minus[MG_DIST_MAXLEV][3];    // rank-internal - faces (the same at every level)
  REAL_TYPE *b[MG_DIST_MAXLEV] = {}, *x[MG_DIST_MAXLEV] = {}, *t[MG_DIST_MAXLEV] = {}, *rt[MG_DIST_MAXLEV] = {};
  REAL_TYPE *gb[MG_DIST_MAXLEV] = {}, *gx[MG_DIST_MAXLEV] = {}, *gt[MG_DIST_MAXLEV] = {};
  REAL_TYPE* tmp0 = nullptr;       // level 0: the second fine array of the sweeps
  REAL_TYPE *send = nullptr, *recv = nullptr;
  size_t blk_max = 0;              // elements per rank in the all-gather (the largest block)
  std::vector<int> bo, bc;         // every rank's level-G block: global offset and points, 3 per rank
  double* res = nullptr;           // the sums the level-0 sweeps write (unused)
  int exchanges = 0;               // halo exchanges + all-gathers of the last cycle
  bool tail = true;
};

namespace {
// one brick's global 0-based level-0 points [h, h+m) per direction and its neighbour table
bool brick_range(const CZ& cz, int rank, int h[3], int m[3], int nid[6]) {
  int sz[3], hd[3];
  if (!comm_decompose(cz.G_size, cz.G_div, cz.numProc, rank, sz, hd, nid)) return false;
  for (int d = 0; d < 3; d++) {
    const int ist = nid[2 * d] < 0 ? 2 : 1, ied = nid[2 * d + 1] < 0 ? sz[d] - 1 : sz[d];
    h[d] = hd[d] - 1 + ist - 2, m[d] = ied - ist + 1;
  }
  return true;
}

void global_level(MgdLevel& L, const int* n, int level, const int* n0) {
  L = MgdLevel();
  for (int d = 0; d < 3; d++) {
    L.sz[d] = n[d] + 2, L.idx[2 * d] = 2, L.idx[2 * d + 1] = n[d] + 1;
    L.n0[d] = n0[d], L.o[d] = 0, L.gn[d] = n[d];
  }
  L.level = level, L.dense = 0;
}

void fatal_if(bool bad, const char* what) {
  if (bad) cz_fatal(1, "czhip: distributed V-cycle: %s failed\n", what);
}
}  // namespace

MgDist* mgd_create(const CZ& cz, CommCtx* comm0, int gather_points, bool tail) {
  if (cz.numProc < 2 || !comm0) return nullptr;
  MgDist* h = new MgDist();
  h->nproc = cz.numProc;
  h->tail = tail;
  for (int d = 0; d < 3; d++) h->n0[d] = cz.G_size[d] - 2, h->gn[0][d] = h->n0[d];
  // the levels: those of the single-domain hierarchy (coarsening stops at the first level whose largest extent is <= 4)
  for (int l = 0;; l++) {
    if (l >= MG_DIST_MAXLEV) {
      delete h;
      return nullptr;
    }
    h->nlev = l + 1;
    if (std::max(h->gn[l][0], std::max(h->gn[l][1], h->gn[l][2])) <= 4) break;
    for (int d = 0; d < 3; d++) h->gn[l + 1][d] = (h->gn[l][d] + 1) / 2;
  }
  // the gather level
  std::vector<int> H(3 * h->nproc), M(3 * h->nproc), NID(6 * h->nproc);
  for (int r = 0; r < h->nproc; r++)
    if (!brick_range(cz, r, &H[3 * r], &M[3 * r], &NID[6 * r])) {
      delete h;
      return nullptr;
    }
  int G = h->nlev > 1 ? h->nlev - 1 : 0;
  for (int l = 1; l < G; l++) {
    bool empty = false;
    for (int r = 0; r < h->nproc; r++)
      for (int d = 0; d < 3; d++) {
        int f, c;
        comm_mg_own(H[3 * r + d], M[3 * r + d], l, &f, &c);
        if (c < 1) empty = true;
      }
    const double pts = (double)h->gn[l][0] * h->gn[l][1] * h->gn[l][2];
    if (empty || pts <= (double)gather_points) {
      G = l;
      break;
    }
  }
  h->G = G;
  const int me = cz.myRank;
  const int* hm = &H[3 * me];
  const int* mm = &M[3 * me];
  // the distributed levels 0 .. G-1
  for (int l = 0; l < std::max(G, 1); l++) {
    MgdLevel& L = h->lev[l];
    L = MgdLevel();
    L.level = l, L.dense = 0;
    for (int d = 0; d < 3; d++) {
      int f, c;
      comm_mg_own(hm[d], mm[d], l, &f, &c);
      const bool pm = cz.nID[2 * d] < 0, pp = cz.nID[2 * d + 1] < 0;
      L.n0[d] = h->n0[d], L.o[d] = f, L.gn[d] = h->gn[l][d];
      if (l == 0) {
        L.sz[d] = cz.size[d], L.idx[2 * d] = cz.innerFidx[2 * d], L.idx[2 * d + 1] = cz.innerFidx[2 * d + 1];
      } else {
        L.sz[d] = c + (pm ? 1 : 0) + (pp ? 1 : 0), L.idx[2 * d] = pm ? 2 : 1, L.idx[2 * d + 1] = L.idx[2 * d] + c - 1;
      }
      h->minus[l][d] = pm ? 0 : 1;
    }
    if (l == 0) {
      h->comm[0] = comm0;
      h->tmp0 = czhip_alloc_s3d(L.sz);
    } else {
      h->comm[l] = comm_create(me, h->nproc, L.sz, cz.nID, sizeof(REAL_TYPE), cz.G_div);
      fatal_if(!h->comm[l], "comm_create of a coarse level");
      h->b[l] = czhip_alloc_s3d(L.sz), h->x[l] = czhip_alloc_s3d(L.sz), h->t[l] = czhip_alloc_s3d(L.sz);
    }
    if (l < G) h->rt[l] = czhip_alloc_s3d(L.sz);
  }
  if (G > 0) {
    // level G: every rank's block, the padded send / receive buffers, the global arrays of G .. coarsest
    h->bo.resize(3 * h->nproc), h->bc.resize(3 * h->nproc);
    for (int r = 0; r < h->nproc; r++) {
      size_t n = 1;
      for (int d = 0; d < 3; d++) {
        comm_mg_own(H[3 * r + d], M[3 * r + d], G, &h->bo[3 * r + d], &h->bc[3 * r + d]);
        n *= (size_t)h->bc[3 * r + d];
      }
      h->blk_max = std::max(h->blk_max, n);
    }
    MgdLevel& B = h->blk;
    B = MgdLevel();
    B.level = G, B.dense = 1;
    for (int d = 0; d < 3; d++) B.sz[d] = h->bc[3 * me + d], B.o[d] = h->bo[3 * me + d], B.n0[d] = h->n0[d], B.gn[d] = h->gn[G][d];
    HIP_CHECK(hipMalloc(&h->send, h->blk_max * sizeof(REAL_TYPE)));
    HIP_CHECK(hipMalloc(&h->recv, h->blk_max * h->nproc * sizeof(REAL_TYPE)));
    HIP_CHECK(hipMemset(h->send, 0, h->blk_max * sizeof(REAL_TYPE)));
    for (int l = G; l < h->nlev; l++) {
      global_level(h->glev[l], h->gn[l], l, h->n0);
      h->gb[l] = czhip_alloc_s3d(h->glev[l].sz), h->gx[l] = czhip_alloc_s3d(h->glev[l].sz), h->gt[l] = czhip_alloc_s3d(h->glev[l].sz);
    }
  }
  HIP_CHECK(hipMalloc(&h->res, 4 * sizeof(double)));
  return h;
}

void mgd_destroy(MgDist* h) {
  if (!h) return;
  czhip_sync();
  for (int l = 1; l < MG_DIST_MAXLEV; l++)
    if (h->comm[l]) comm_destroy(h->comm[l]);
  for (int l = 0; l < MG_DIST_MAXLEV; l++)
    for (REAL_TYPE* a : {h->b[l], h->x[l], h->t[l], h->rt[l], h->gb[l], h->gx[l], h->gt[l]})
      if (a) czhip_free(a);
  if (h->tmp0) czhip_free(h->tmp0);
  if (h->send) (void)hipFree(h->send);
  if (h->recv) (void)hipFree(h->recv);
  if (h->res) (void)hipFree(h->res);
  delete h;
}

int mgd_levels(const MgDist* h) { return h ? h->nlev : 0; }
int mgd_gather_level(const MgDist* h) { return h ? h->G : 0; }
int mgd_exchanges(const MgDist* h) { return h ? h->exchanges : 0; }

namespace {
void halo(MgDist* h, int l, REAL_TYPE* X) {
  fatal_if(!comm_halo(h->comm[l], X, nullptr, stream()), "face exchange");
  h->exchanges++;
}
void halo_full(MgDist* h, int l, REAL_TYPE* X) {
  fatal_if(!comm_halo_full(h->comm[l], X, stream()), "face + edge + corner exchange");
  h->exchanges++;
}

// level 0's sweep u -> w with the unit coefficients (the decomposed Jacobi sweep of pcg ... jacobi)
void sweep0(MgDist* h, const REAL_TYPE* u, REAL_TYPE* w, const REAL_TYPE* b, REAL_TYPE omg) {
  REAL_TYPE cf[7] = {1, 1, 1, 1, 1, 1, 6};
  czhip_jacobi_async(u, w, b, h->lev[0].sz, h->lev[0].idx, GUIDE, cf, omg, h->res, 0, nullptr);
}

// x_l = V_l(b_l) on the global copy, l >= G: the single-domain level kernels (czhip_mg_apply_async's mg_cycle)
void cycle_global(MgDist* h, int l, REAL_TYPE omg) {
  const MgdLevel& L = h->glev[l];
  REAL_TYPE *b = h->gb[l], *x = h->gx[l], *t = h->gt[l];
  if (h->tail && czhip_mg_tail_async(x, b, L.sz, L.idx, GUIDE, l, h->n0, omg)) return;
  auto smooth = [&](const REAL_TYPE* u, REAL_TYPE* w) { fatal_if(!czhip_mg_smooth_async(u, w, b, L.sz, L.idx, GUIDE, l, h->n0, omg), "smooth"); };
  if (l == h->nlev - 1) {  // the coarsest level: 8 sweeps from zero
    smooth(nullptr, t);
    for (int s = 1; s < 8; s++) smooth((s & 1) ? t : x, (s & 1) ? x : t);
    return;
  }
  const MgdLevel& C = h->glev[l + 1];
  smooth(nullptr, t);
  smooth(t, x);
  fatal_if(!czhip_mg_restrict_async(h->gb[l + 1], C.sz, C.idx, x, b, L.sz, L.idx, GUIDE, l, h->n0), "restrict");
  cycle_global(h, l + 1, omg);
  fatal_if(!czhip_mg_prolong_async(x, x, h->gx[l + 1], C.sz, C.idx, L.sz, L.idx, GUIDE, l, h->n0), "prolong");
  smooth(x, t);
  smooth(t, x);
}

// b_G from the restriction (in the send buffer) -> every rank's global copy -> x_G
void gather_and_cycle(MgDist* h, REAL_TYPE omg) {
  const int G = h->G;
  fatal_if(!comm_allgather(h->comm[0], h->send, h->recv, h->blk_max, stream()), "all-gather");
  h->exchanges++;
  for (int r = 0; r < h->nproc; r++)
    fatal_if(!mgd_unpack_async(h->gb[G], h->glev[G], h->recv + (size_t)r * h->blk_max, &h->bo[3 * r], &h->bc[3 * r]), "unpack");
  cycle_global(h, G, omg);
}

// the coarse iterate of level l+1 (distributed or gathered) and its geometry, for the prolongation to level l
void coarse_of(MgDist* h, int l, const REAL_TYPE** xc, const MgdLevel** C) {
  if (l + 1 < h->G) {
    halo_full(h, l + 1, h->x[l + 1]);  // parents on the - neighbours
    *xc = h->x[l + 1], *C = &h->lev[l + 1];
  } else {
    *xc = h->gx[h->G], *C = &h->glev[h->G];
  }
}

// b_{l+1} (distributed, or level G's block) = restricted residual of x_l; x's faces are current
void restrict_down(MgDist* h, int l, const REAL_TYPE* x, const REAL_TYPE* b) {
  const MgdLevel& F = h->lev[l];
  fatal_if(!mgd_resface_async(h->rt[l], x, b, F, h->minus[l]), "residual of the - faces");
  halo_full(h, l, h->rt[l]);  // children on the + neighbours
  if (l + 1 < h->G) fatal_if(!mgd_restrict_async(h->b[l + 1], h->lev[l + 1], x, b, h->rt[l], F), "restrict");
  else fatal_if(!mgd_restrict_async(h->send, h->blk, x, b, h->rt[l], F), "restrict into the gathered level");
}

// x_l = V_l(b_l), 1 <= l < G
void cycle_dist(MgDist* h, int l, REAL_TYPE omg) {
  const MgdLevel& L = h->lev[l];
  REAL_TYPE *b = h->b[l], *x = h->x[l], *t = h->t[l];
  auto smooth = [&](const REAL_TYPE* u, REAL_TYPE* w) { fatal_if(!mgd_smooth_async(u, w, b, L, omg), "smooth"); };
  smooth(nullptr, t);
  halo(h, l, t);
  smooth(t, x);
  halo(h, l, x);
  restrict_down(h, l, x, b);
  if (l + 1 < h->G) cycle_dist(h, l + 1, omg);
  else gather_and_cycle(h, omg);
  const REAL_TYPE* xc;
  const MgdLevel* C;
  coarse_of(h, l, &xc, &C);
  fatal_if(!mgd_prolong_async(x, x, xc, *C, L), "prolong");
  halo(h, l, x);
  smooth(x, t);
  halo(h, l, t);
  smooth(t, x);
}
}  // namespace

// z = V_0(r) on this rank's brick; collective.  r's ghost cells are not read.
int mgd_apply(MgDist* h, REAL_TYPE* z, const REAL_TYPE* r, REAL_TYPE omg) {
  if (!h || !z || !r || z == r) return 0;
  h->exchanges = 0;
  REAL_TYPE* const tmp = h->tmp0;
  const MgdLevel& F = h->lev[0];
  const size_t nbytes = (size_t)(F.sz[0] + 2 * GUIDE) * (F.sz[1] + 2 * GUIDE) * (F.sz[2] + 2 * GUIDE) * sizeof(REAL_TYPE);
  HIP_CHECK(hipMemsetAsync(tmp, 0, nbytes, stream()));
  if (h->nlev == 1) {  // level 0 is already the coarsest: 8 sweeps from zero
    sweep0(h, tmp, z, r, omg);
    for (int s = 1; s < 8; s++) {
      REAL_TYPE* u = (s & 1) ? z : tmp;
      halo(h, 0, u);
      sweep0(h, u, (s & 1) ? tmp : z, r, omg);
    }
    HIP_CHECK(hipMemcpyAsync(z, tmp, nbytes, hipMemcpyDeviceToDevice, stream()));  // (the eighth sweep wrote tmp)
    return 1;
  }
  sweep0(h, tmp, z, r, omg);  // x = 2 sweeps from zero (in tmp)
  halo(h, 0, z);
  sweep0(h, z, tmp, r, omg);
  halo(h, 0, tmp);
  restrict_down(h, 0, tmp, r);
  if (h->G > 1) cycle_dist(h, 1, omg);
  else gather_and_cycle(h, omg);
  const REAL_TYPE* xc;
  const MgdLevel* C;
  coarse_of(h, 0, &xc, &C);
  fatal_if(!mgd_prolong_async(z, tmp, xc, *C, F), "prolong");  // u = x + R(alpha x_1(parent)), in z
  halo(h, 0, z);
  sweep0(h, z, tmp, r, omg);  // x = 2 sweeps from u
  halo(h, 0, tmp);
  sweep0(h, tmp, z, r, omg);
  return 1;
}
