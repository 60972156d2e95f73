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
//   G .. coarsest  the owned blocks of b_G all-gathered (an exact copy) into level G of a single-domain hierarchy (cz_mg) that every rank
//                  keeps for the levels from G on; its own cycle runs there redundantly, and the prolongation from G reads its parents
//                  from that copy.
// The order of the cycle is mg_walk's (cz_mg_cycle.h), the one the single-domain cycle takes; MgdOps below are its operations here, the
// level kernels those of the single domain (cz_k_mg.h).
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
  MgdLevel lev[MG_MAXLEV];         // distributed levels 0 .. G-1 (level 0: the driver's arrays); nm: the level's word of the state (mgd_set_bc)
  MgdLevel blk;                    // this brick's owned block of level G (dense: the all-gather's send buffer)
  cz_mg* g = nullptr;              // levels G .. coarsest: a single-domain hierarchy on every rank
  CommCtx* comm[MG_MAXLEV] = {};   // level 0: the driver's; 1 .. G-1 own ones
  int minus[3];                    // rank-internal - faces (the same at every level)
  REAL_TYPE *b[MG_MAXLEV] = {}, *x[MG_MAXLEV] = {}, *t[MG_MAXLEV] = {}, *rt[MG_MAXLEV] = {};  // levels >= 1 (rt: 0 too)
  REAL_TYPE* tmp0 = nullptr;       // level 0: the second fine array of the sweeps
  REAL_TYPE *send = nullptr, *recv = nullptr;
  size_t blk_max = 0;              // elements per rank in the all-gather (the largest block)
  std::vector<int> bo, bc;         // every rank's level-G block: global offset and points, 3 per rank
  double* res = nullptr;           // the sums the level-0 sweeps write (unused)
  int exchanges = 0;               // halo exchanges + all-gathers of the last cycle
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

void fatal_if(bool bad, const char* what) {
  if (bad) cz_fatal(1, "czhip: distributed V-cycle: %s failed\n", what);
}

size_t padded(const MgdLevel& L) { return (size_t)(L.sz[0] + 2 * GUIDE) * (L.sz[1] + 2 * GUIDE) * (L.sz[2] + 2 * GUIDE); }

}  // namespace

// The state of the global box, the same on every rank; its periodic directions are not cut by the decomposition (the driver checks), so every
// brick holds both faces of such a direction at every level and the wrap is the single domain's fill beside the exchange.  Every distributed
// level, the gathered block and the hierarchy of the gathered levels learn it (mg_level_bc: without a periodic direction the six flags at
// every level); the arrays whose ghost layers carried an earlier state's mirrors or wraps are zeros again
void mgd_set_bc(MgDist* h, CzBc bc) {
  if (h->g) mg_set_bc(h->g, bc);
  const int dist = std::max(h->G, 1);
  int wraps = bc.per;
  for (int l = 0; l < dist; l++) wraps |= h->lev[l].nm >> 6;
  for (int l = 0; l < dist; l++) h->lev[l].nm = mg_level_bc(bc, h->lev[l].gn);
  h->blk.nm = mg_level_bc(bc, h->blk.gn);  // (G = 0: there is no block)
  HIP_CHECK(hipMemsetAsync(h->tmp0, 0, padded(h->lev[0]) * sizeof(REAL_TYPE), stream()));
  for (int l = 1; wraps && l < h->G; l++)
    for (REAL_TYPE* a : {h->x[l], h->t[l]})
      if (a) HIP_CHECK(hipMemsetAsync(a, 0, padded(h->lev[l]) * sizeof(REAL_TYPE), stream()));
}

MgDist* mgd_create(const CZ& cz, CommCtx* comm0, int gather_points, bool tail) {
  if (cz.numProc < 2 || !comm0) return nullptr;
  MgDist* h = new MgDist();
  h->nproc = cz.numProc;
  int gn[MG_MAXLEV][3];
  for (int d = 0; d < 3; d++) h->n0[d] = cz.G_size[d] - 2;
  h->nlev = mg_level_dims(h->n0, gn, MG_MAXLEV - 1);  // the levels of the single-domain hierarchy
  if (!h->nlev) {
    delete h;
    return nullptr;
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
    const double pts = (double)gn[l][0] * gn[l][1] * gn[l][2];
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
    L.level = l, L.g = GUIDE;
    for (int d = 0; d < 3; d++) {
      int f, c;
      comm_mg_own(hm[d], mm[d], l, &f, &c);
      const bool pm = cz.nID[2 * d] < 0, pp = cz.nID[2 * d + 1] < 0;
      L.n0[d] = h->n0[d], L.o[d] = f, L.gn[d] = gn[l][d];
      if (l == 0) {
        L.sz[d] = cz.size[d], L.idx[2 * d] = cz.innerFidx[2 * d], L.idx[2 * d + 1] = cz.innerFidx[2 * d + 1];
      } else {
        L.sz[d] = c + (pm ? 1 : 0) + (pp ? 1 : 0), L.idx[2 * d] = pm ? 2 : 1, L.idx[2 * d + 1] = L.idx[2 * d] + c - 1;
      }
      h->minus[d] = pm ? 0 : 1;
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
    // level G: every rank's block, the padded send / receive buffers, the hierarchy of G .. coarsest
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
    for (int d = 0; d < 3; d++) B.sz[d] = h->bc[3 * me + d], B.o[d] = h->bo[3 * me + d], B.n0[d] = h->n0[d], B.gn[d] = gn[G][d];
    HIP_CHECK(hipMalloc(&h->send, h->blk_max * sizeof(REAL_TYPE)));
    HIP_CHECK(hipMalloc(&h->recv, h->blk_max * h->nproc * sizeof(REAL_TYPE)));
    HIP_CHECK(hipMemset(h->send, 0, h->blk_max * sizeof(REAL_TYPE)));
    h->g = mg_create(h->n0, G, tail);
    fatal_if(!h->g, "the hierarchy of the gathered levels");
  }
  HIP_CHECK(hipMalloc(&h->res, 4 * sizeof(double)));
  return h;
}

void mgd_destroy(MgDist* h) {
  if (!h) return;
  czhip_sync();
  for (int l = 1; l < MG_MAXLEV; l++)
    if (h->comm[l]) comm_destroy(h->comm[l]);
  for (int l = 0; l < MG_MAXLEV; l++)
    for (REAL_TYPE* a : {h->b[l], h->x[l], h->t[l], h->rt[l]})
      if (a) czhip_free(a);
  czhip_mg_destroy(h->g);
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
// the operations of mg_walk on the distributed levels 0 .. G-1 (G = 0: level 0 alone).  Levels >= 1 keep b, x and a temporary t of their own;
// level 0's b is r and its iterate is in x0, with o0 as the temporary, until the prolongation moves it to o0
struct MgdOps {
  MgDist* h;
  REAL_TYPE omg;
  const REAL_TYPE* r;
  REAL_TYPE *x0, *o0;

  REAL_TYPE* x(int l) { return l ? h->x[l] : x0; }
  const REAL_TYPE* b(int l) { return l ? h->b[l] : r; }
  // (the fill of the brick's physical faces stands beside the exchange; it is not one: level 0 mirrors its Neumann faces, every level wraps
  // its periodic directions -- DESIGN.md §5.13, §5.15)
  void halo(int l, REAL_TYPE* X) {
    fatal_if(!comm_halo(h->comm[l], X, nullptr, stream()), "face exchange");
    h->exchanges++;
    fatal_if(!fill_bc_async(X, h->lev[l].sz, h->lev[l].idx, GUIDE, h->lev[l].nm, l == 0), "fill of the periodic and Neumann faces");
  }
  void halo_full(int l, REAL_TYPE* X) {
    fatal_if(!comm_halo_full(h->comm[l], X, stream()), "face + edge + corner exchange");
    h->exchanges++;
  }
  // w = one sweep from u, after a face exchange of u (zero: u is zero, nothing to exchange).  Level 0: the decomposed Jacobi sweep of
  // pcg ... jacobi with the unit coefficients, which reads the zeros from u
  void sweep(int l, REAL_TYPE* u, REAL_TYPE* w, bool zero) {
    if (!zero) halo(l, u);
    REAL_TYPE cf[7] = {1, 1, 1, 1, 1, 1, 6};
    if (l == 0) czhip_jacobi_async(u, w, r, h->lev[0].sz, h->lev[0].idx, GUIDE, cf, omg, h->res, 0, nullptr);
    else fatal_if(!mg_smooth_async(zero ? nullptr : u, w, h->b[l], h->lev[l], omg), "smooth");
  }

  // level G: b_G from the restriction (in the send buffer) -> every rank's copy of the whole level -> x_G by the single-domain cycle
  bool whole(int l) {
    if (!h->g || l < h->G) return false;
    fatal_if(!comm_allgather(h->comm[0], h->send, h->recv, h->blk_max, stream()), "all-gather");
    h->exchanges++;
    for (int q = 0; q < h->nproc; q++)
      fatal_if(!mgd_unpack_async(h->g->b[l], h->g->lev[l], h->recv + (size_t)q * h->blk_max, &h->bo[3 * q], &h->bc[3 * q]), "unpack");
    fatal_if(!mg_cycle_async(h->g, omg), "the cycle of the gathered levels");
    return true;
  }
  void pair(int l, bool zero, bool /*post: Jacobi sweeps are the same before and after the correction*/) {
    REAL_TYPE* const t = l ? h->t[l] : o0;
    sweep(l, x(l), t, zero);
    sweep(l, t, x(l), false);
  }
  // b_{l+1} (distributed, or level G's block) = the restricted residual of x_l; the children on the + neighbours come from rt
  void restrict_down(int l) {
    halo(l, x(l));
    fatal_if(!mgd_resface_async(h->rt[l], x(l), b(l), h->lev[l], h->minus), "residual of the - faces");
    halo_full(l, h->rt[l]);
    const bool dist = l + 1 < h->G;
    fatal_if(!mg_restrict_async(dist ? h->b[l + 1] : h->send, dist ? h->lev[l + 1] : h->blk, x(l), b(l), h->rt[l], h->lev[l]), "restrict");
  }
  // the parents: level l+1's iterate after its exchange (parents on the - neighbours), or the gathered level
  void prolong_up(int l) {
    const bool dist = l + 1 < h->G;
    if (dist) halo_full(l + 1, h->x[l + 1]);
    REAL_TYPE* const u = l ? h->x[l] : o0;
    fatal_if(!mg_prolong_async(u, x(l), dist ? h->x[l + 1] : h->g->x[l + 1], dist ? h->lev[l + 1] : h->g->lev[l + 1], h->lev[l]), "prolong");
    if (l == 0) std::swap(x0, o0);
  }
};
}  // namespace

// z = V_0(r) on this rank's brick; collective.  r's ghost cells are not read.
int mgd_apply(MgDist* h, REAL_TYPE* z, const REAL_TYPE* r, REAL_TYPE omg) {
  if (!h || !z || !r || z == r) return 0;
  h->exchanges = 0;
  // level 0's iterate ends in z: it starts there where nothing moves it (level 0 the coarsest), else in the temporary.  The array it starts
  // in is cleared for the sweep from zero; the other one is written on its owned points and rank-internal ghost cells only, so tmp0's
  // physical faces keep the zeros of its allocation, as z's do by the caller's contract
  const bool stays = h->nlev == 1;
  MgdOps ops{h, omg, r, stays ? z : h->tmp0, stays ? h->tmp0 : z};
  const MgdLevel& F = h->lev[0];
  HIP_CHECK(hipMemsetAsync(ops.x0, 0, (size_t)(F.sz[0] + 2 * GUIDE) * (F.sz[1] + 2 * GUIDE) * (F.sz[2] + 2 * GUIDE) * sizeof(REAL_TYPE), stream()));
  mg_walk(ops, 0, h->nlev - 1);
  return 1;
}
