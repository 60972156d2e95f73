// cz_driver.cpp -- restatement of the reference's host driver for a GPU-resident solve.
//
//   CZ::Setup / Solve / Evaluate   <- src/cz_cpp/cz_Evaluate.cpp:21-567   (argv parsing, solver select, allocation,
//                                      boundary conditions, dispatch, "Iter = .. Res = .." print, history file)
//   CZ::JACOBI / RBSOR / PBiCGSTAB <- src/cz_cpp/cz_Poisson.cpp:30-82, 159-235, 332-504
//   CZ::Fdot1/2, Preconditioner    <- cz_Poisson.cpp:239-270, 273-322
//   CZ::range_inner_index          <- src/cz_cpp/cz_miscel.cpp:20-52
//
// What is different from the reference, and why (details in DESIGN.md):
//   * all 3-D arrays live in HBM; the Fortran kernels are the HIP kernels of cz_kernels.hip.
//   * JACOBI ping-pongs between X and WRK instead of sweeping into WRK and copying back (12 instead of 20 B/LUP).
//   * the per-iteration "all-reduce, sqrt, history line, eps test" of cz_Poisson.cpp:67-77 runs on the device
//     (czhip_check_async); sweeps queued after convergence turn into no-ops through a device flag, so the host never
//     waits for the GPU inside the loop yet the iteration count, history and final field are exactly those of the
//     sequential loop.
//   * bc_k_ after each checked iteration (cz_Poisson.cpp:74) is skipped: sweeps write the inner box only, the
//     Dirichlet faces set at start-up are never touched, so the call is an identity.
//   * the CBrick/MPI domain decomposition is replaced by cell-ownership decomposition + RCCL (cz_comm.cpp).
//
// What a solver or preconditioner name means is stated once, as a row of cz_solvers.h: spelling, printed name, where it is accepted, MAF
// flag, loop family, what Preconditioner does with it, a line solver's iteration.  setLS / setStrPre look the name up, CZ::run turns the
// family into the loop (for Solve, Sweeps and Preconditioner alike).  A new solver is one enumerator and one row; it needs a loop here and
// a case in CZ::run only if its family is new.  Conditions that belong to one loop's own reasoning (the literal zero start, pcg's
// coefficient ranges) stay with that loop.
#include "cz_driver.h"

#include <unistd.h>

#include <cfloat>
#include <chrono>
#include <cstdint>
#include <cmath>
#include <cstring>
#include <ctime>
#include <algorithm>
#include <vector>

#include "cz_comm.h"

using namespace czhip_internal;

#define Hostonly_ if (myRank == 0)

namespace {
const char* printMethod(int t) { return cz_solvers::row(t).printed; }
double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
constexpr int POLL_EVERY = 32;   // iterations between convergence polls of the host
constexpr int POLL_SLOTS = 4;
}  // namespace

CZ::CZ() {
  czhip_init(-1);
  HIP_CHECK(hipMalloc(&d_res, sizeof(CzScalars)));
  HIP_CHECK(hipMemset(d_res, 0, sizeof(CzScalars)));
  HIP_CHECK(hipMalloc(&d_flag, sizeof(CzFlags)));
  HIP_CHECK(hipMemset(d_flag, 0, sizeof(CzFlags)));
  HIP_CHECK(hipHostMalloc(&h_scal, sizeof(CzScalars), hipHostMallocDefault));
  HIP_CHECK(hipHostMalloc(&h_flag, 2 * POLL_SLOTS * sizeof(int), hipHostMallocDefault));
  cfg = CzConfig::from_env();  // the environment as this driver was created in (cz_config.h); nothing below asks it again
  overlap = cfg.num(CZV_OVERLAP, overlap);
  lag_reduce = cfg.num(CZV_LAG_REDUCE, lag_reduce);
  field_form = cfg.num(CZV_FIELD_FORM, field_form);
  if (const char* sk = cfg.str(CZV_TEST_SKEW)) sscanf(sk, "%d,%d", &skew_rank, &skew_ms);  // tests: "rank,milliseconds"
}

CZ::~CZ() {
  czhip_sync();
  if (comm_cus > 0) reserve_comm_cus(0);  // the library context outlives this object
  REAL_TYPE* arrs[] = {WRK, WRK2, P, RHS, pcg_p, pcg_p_, pcg_r, pcg_r0, pcg_q, pcg_s, pcg_s_, pcg_t_, cg_r, cg_z, cg_p[0], cg_p[1], cg_q, pvt, MSK};
  if (mg) czhip_mg_destroy(mg);
  mg = nullptr;  // (coef_clear below detaches the coefficients from a hierarchy that is still there)
  if (mgd) mgd_destroy(mgd);
  if (d_xc) (void)hipFree(d_xc);
  if (d_yc) (void)hipFree(d_yc);
  if (d_zc) (void)hipFree(d_zc);
  for (REAL_TYPE* a : arrs)
    if (a) czhip_free(a);
  coef_clear();
  if (d_hist) (void)hipFree(d_hist);
  (void)hipFree(d_res);
  (void)hipFree(d_flag);
  (void)hipHostFree(h_scal);
  (void)hipHostFree(h_flag);
  if (comm) comm_destroy(comm);
  if (ev_shell) (void)hipEventDestroy(ev_shell);
  if (ev_src) (void)hipEventDestroy(ev_src);
  if (ev_comm) (void)hipEventDestroy(ev_comm);
  if (ev_int) (void)hipEventDestroy(ev_int);
  for (hipEvent_t e : ev_chk)
    if (e) (void)hipEventDestroy(e);
  if (comm_stream) (void)hipStreamDestroy(comm_stream);
  if (ev_io) (void)hipEventDestroy(ev_io);
  if (io_stage) (void)hipFree(io_stage);
  if (fph) fclose(fph);
}

size_t CZ::padded_cells() const { return (size_t)(size[0] + 2 * GUIDE) * (size[1] + 2 * GUIDE) * (size[2] + 2 * GUIDE); }

double CZ::npts() const {
  return (double)(innerFidx[I_plus] - innerFidx[I_minus] + 1) * (double)(innerFidx[J_plus] - innerFidx[J_minus] + 1) *
         (double)(innerFidx[K_plus] - innerFidx[K_minus] + 1);
}

// cz_miscel.cpp:20-52.  The reference always starts at 2 because its CBrick "node" bricks share one layer with the
// lower neighbour; this build's bricks own disjoint cells, so a face that borders another rank starts at 1 / ends at
// size, a physical face at 2 / size-1 (identical to the reference when numProc == 1).
double CZ::range_inner_index() {
  int ist = (nID[I_minus] < 0) ? 2 : 1, jst = (nID[J_minus] < 0) ? 2 : 1, kst = (nID[K_minus] < 0) ? 2 : 1;
  int ied = size[0], jed = size[1], ked = size[2];
  if (nID[I_plus] < 0) ied = size[0] - 1;
  if (nID[J_plus] < 0) jed = size[1] - 1;
  if (nID[K_plus] < 0) ked = size[2] - 1;
  innerFidx[I_minus] = ist, innerFidx[I_plus] = ied;
  innerFidx[J_minus] = jst, innerFidx[J_plus] = jed;
  innerFidx[K_minus] = kst, innerFidx[K_plus] = ked;
  for (int f = 0; f < 6; f++) idx1[f] = innerFidx[f] + ((nID[f] >= 0) ? ((f & 1) ? 1 : -1) : 0);
  return (double)(ied - ist + 1) * (double)(jed - jst + 1) * (double)(ked - kst + 1);
}

// cz_Evaluate.cpp:571-681: the preconditioner of pbicgstab[_maf] (a MAF preconditioner alone sets SW_maf as well)
void CZ::setStrPre() {
  const cz_solvers::Row* r = cz_solvers::find(precon.c_str(), cz_solvers::PRE_BICG);
  if (!r) {
    Hostonly_ printf("Invalid preconditioner '%s' (this build: %s)\n", precon.c_str(), cz_solvers::list(cz_solvers::PRE_BICG).c_str());
    exit(0);
  }
  pc_type = r->id;
  if (r->maf) SW_maf = 1;
}

// cz_Evaluate.cpp:684-803 (hot-path solvers only; see DESIGN.md "out of scope").  What a name means is its row in cz_solvers.h; what is
// left here are pcg's rules.
void CZ::setLS(const char* q) {
  const cz_solvers::Row* r = cz_solvers::find(q, cz_solvers::SOLVER);
  if (!r) {
    printf("Invalid solver\n");  // :799-802
    exit(0);
  }
  ls_type = r->id;
  hist_name = std::string(r->name) + ".txt";
  if (r->family == cz_solvers::BICGSTAB) setStrPre();
  if (r->maf) SW_maf = 1;
  if (r->family == cz_solvers::PCG) {  // beyond the reference (DESIGN.md "PCG"): symmetric preconditioners only
    const cz_solvers::Row* pre = cz_solvers::find(precon.c_str(), cz_solvers::PRE_PCG);
    if (!pre) {
      // (a literal, not cz_solvers::list: the text is older than mg and mgrb, and tests/test_gpu_pcg.py pins it)
      Hostonly_ printf("Invalid preconditioner for pcg '%s' (none | jacobi)\n", precon.c_str());
      exit(0);
    }
    pc_type = pre->id;
    // the V-cycle's smoothers are relaxed Jacobi sweeps: the same range keeps it symmetric and definite
    if (pc_type == LS_MG && !(ac1 > (REAL_TYPE)0 && ac1 <= (REAL_TYPE)1)) {
      Hostonly_ printf("Invalid coefficient for pcg with mg '%g' (0 < coef <= 1: a symmetric definite preconditioner)\n", (double)ac1);
      exit(0);
    }
    // the red-black V-cycle is symmetric by its colour order; definite as far as the Ritz estimates of M A were taken
    if (pc_type == LS_MGRB && !(ac1 > (REAL_TYPE)0 && ac1 <= (REAL_TYPE)1.2)) {
      Hostonly_ printf("Invalid coefficient for pcg with mgrb '%g' (0 < coef <= 1.2: a symmetric definite preconditioner)\n", (double)ac1);
      exit(0);
    }
    // under a cut a colour sweep needs an exchange per colour and the two-iteration pass four ghost layers: not built
    if (pc_type == LS_MGRB && numProc > 1) {
      Hostonly_ printf("pcg with mgrb runs on a single domain only (%d ranks); use mg\n", numProc);
      fflush(stdout);
      // ranks may be threads of one process that all arrive here with the GPU open: no exit handlers (as cz_fatal_quick), and the ranks that
      // print nothing leave the process to rank 0 for a moment, so that its line is out before the first of them ends it
      if (myRank != 0) sleep(2);
      _exit(0);
    }
    // k relaxed Jacobi sweeps from zero are a polynomial in A: symmetric, and definite with A's sign for 0 < omega <= 1
    if (pc_type == LS_JACOBI && !(ac1 > (REAL_TYPE)0 && ac1 <= (REAL_TYPE)1)) {
      Hostonly_ printf("Invalid coefficient for pcg with jacobi '%g' (0 < coef <= 1: a symmetric definite preconditioner)\n", (double)ac1);
      exit(0);
    }
  }
}

// Replaces CBrick's SubDomain (cz_Evaluate.cpp:103-159): Cartesian split of the G_size nodes into G_div bricks of
// disjoint cells, rank = ri + div_i*(rj + div_j*rk).
bool CZ::decompose(int div_type) {
  if (numProc == 1) {
    G_div[0] = G_div[1] = G_div[2] = 1;  // :162-176
    for (int a = 0; a < 3; a++) size[a] = G_size[a], head[a] = 1, origin[a] = G_origin[a];
    for (int f = 0; f < 6; f++) nID[f] = -1;
    return true;
  }
  if (div_type == 0) comm_auto_division(numProc, G_size, G_div);
  int sz3[3], hd3[3], nid6[6];
  if (!comm_decompose(G_size, G_div, numProc, myRank, sz3, hd3, nid6)) return false;
  for (int a = 0; a < 3; a++) {
    size[a] = sz3[a], head[a] = hd3[a];
    origin[a] = G_origin[a] + (REAL_TYPE)(head[a] - 1) * pitch[a];  // :136-138
  }
  for (int f = 0; f < 6; f++) nID[f] = nid6[f];
  return true;
}

void CZ::ensure_hist(int n) {
  if (n <= hist_cap) return;
  if (d_hist) {
    czhip_sync();
    HIP_CHECK(hipFree(d_hist));
  }
  hist_cap = n + 1024;
  HIP_CHECK(hipMalloc(&d_hist, (size_t)hist_cap * sizeof(double)));
  HIP_CHECK(hipMemset(d_hist, 0, (size_t)hist_cap * sizeof(double)));
}

// ------------------------------------------------------------------------------------------------------------
int CZ::Setup(int argc, char** argv) {
  int div_type = 0;
  const int gc = GUIDE;
  if (argc != 7 && argc != 8 && argc != 10 && argc != 11) return 0;  // main.cpp:19

  // a set-up starts with Dirichlet faces: the hierarchy it builds knows no mask (cz_set_neumann comes after cz_setup)
  bc = CzBc();
  closed_box = 0;
  coef_clear();  // (and with unit coefficients: cz_set_face_coef comes after cz_setup)
  coef_mg = 0;   // (and without the coefficient hierarchy: cz_set_coef_mg comes after cz_setup)
  mg_lines = 0;  // (and without line iterations: cz_set_mg_lines comes after cz_setup)
  closed_m[0] = closed_m[1] = closed_m[2] = 0.0;
  closed_m0_on_device = false;
  solve_plan = PassPlan();

  comm_world(&myRank, &numProc);  // rank/size from the launcher environment (replaces MPI_Comm_rank/size, :44-50)

  G_size[0] = atoi(argv[1]);
  G_size[1] = atoi(argv[2]);
  G_size[2] = atoi(argv[3]);
  if (G_size[0] < 3 || G_size[1] < 3 || G_size[2] < 3) {
    Hostonly_ printf("command line error : grid size must be >= 3\n");
    return 0;
  }

  const char* q = argv[4];
  const cz_solvers::Row* named = cz_solvers::find(q, cz_solvers::SOLVER);  // (an unknown name is refused by setLS, after the checks in between)
  if (named && named->family == cz_solvers::BICGSTAB) {  // :63-70
    if (argc != 8 && argc != 11) {
      Hostonly_ printf("command line error : pbicgstab\n");
      exit(0);
    }
    precon = argv[7];
  }
  if (named && named->family == cz_solvers::PCG) precon = (argc == 8 || argc == 11) ? argv[7] : "none";
  if (argc == 10) {  // :73-78
    div_type = 1;
    G_div[0] = atoi(argv[7]), G_div[1] = atoi(argv[8]), G_div[2] = atoi(argv[9]);
  }
  if (argc == 11) {  // :80-85
    div_type = 1;
    G_div[0] = atoi(argv[8]), G_div[1] = atoi(argv[9]), G_div[2] = atoi(argv[10]);
  }

  pitch[0] = pitch[1] = pitch[2] = 1.0 / (REAL_TYPE)(G_size[2] - 1);  // :88

  if (div_type == 1 && G_div[0] * G_div[1] * G_div[2] != numProc) {  // :93-96
    printf("\tThe number of proceees does not agree with the division size.\n");
    return 0;
  }
  ac1 = atof(argv[6]);  // :99

  if (!decompose(div_type)) return 0;
  if (numProc > 1) {
    comm = comm_create(myRank, numProc, size, nID, sizeof(REAL_TYPE), G_div);
    if (!comm) return 0;
  }

  setLS(q);
  if (!quiet) Hostonly_ {
    printf("Iterative Mehtod = %s\n", printMethod(ls_type));  // :194 (sic)
    if (cz_solvers::krylov(cz_solvers::row(ls_type))) printf("Preconditioner = %s\n", printMethod(pc_type));
  }

  if (!quiet) Hostonly_ {  // :210-218
    if (!(fph = fopen(hist_name.c_str(), "w"))) {
      printf("\tSorry, can't open file.\n");
      exit(0);
    }
    fprintf(fph, "Itration      Residual\n");
  }

  double sum_r = range_inner_index();  // :222-224
  plan_overlap();
  if (!Comm_SUM_1(&sum_r)) return 0;
  res_normal = 1.0 / (double)sum_r;
  g_npts = (double)sum_r;

  // :239-288 (only the arrays the hot path touches)
  RHS = czhip_alloc_s3d(size);
  P = czhip_alloc_s3d(size);
  WRK = czhip_alloc_s3d(size);
  if (numProc > 1) {
    // The fused pass needs the two-layer exchange, single sweeps the one-layer exchange: all bricks must take the same path.
    // Bricks of an uneven division can differ (k-extent multiple of the vector width or not): agree on the weakest.
    // (the MAF flavour of the pass needs a little more LDS -- the table of the k metric terms -- and is probed as well where it will run)
    const double mine = (pair_probe(P, WRK, RHS, size, innerFidx, idx1, GUIDE, cf[6], 0) && (!SW_maf || pair_probe(P, WRK, RHS, size, innerFidx, idx1, GUIDE, cf[6], 1))) ? 0.0 : 1.0;
    pairs_ok = comm_allreduce_max_host(comm, mine) == 0.0;
    if (cfg.has(CZV_COMM_DEBUG)) {  // one line per rank on stderr: what a multi-GPU run decided
      int dev = -1;
      (void)hipGetDevice(&dev);
      fprintf(stderr,
              "cz rank %d/%d device %d: div %dx%dx%d size %dx%dx%d head %d,%d,%d nID %d %d %d %d %d %d fused_pass=%d shell_slabs=%d overlap=%d "
              "lagged_reduce=%d comm_cus_per_xcd=%d\n",
              myRank, numProc, dev, G_div[0], G_div[1], G_div[2], size[0], size[1], size[2], head[0], head[1], head[2], nID[0], nID[1], nID[2],
              nID[3], nID[4], nID[5], (int)pairs_ok, n_shell, overlap, lag_reduce, comm_cus);
      if (myRank == 0) {  // the switches in force (cz_config.h), once per job
        std::string sw = cfg.describe(true);
        for (char& ch : sw) if (ch == '\n') ch = ' ';
        fprintf(stderr, "cz config: %s\n", sw.c_str());
      }
    }
  }
  const bool bicg = cz_solvers::row(ls_type).family == cz_solvers::BICGSTAB;
  if (bicg) {
    pcg_p = czhip_alloc_s3d(size), pcg_p_ = czhip_alloc_s3d(size), pcg_r = czhip_alloc_s3d(size);
    pcg_r0 = czhip_alloc_s3d(size), pcg_q = czhip_alloc_s3d(size), pcg_s = czhip_alloc_s3d(size);
    pcg_s_ = czhip_alloc_s3d(size), pcg_t_ = czhip_alloc_s3d(size);
  }
  const int narr = bicg ? 11 : ls_type == LS_PCG ? (pc_type == LS_JACOBI ? 8 : pc_type == LS_MG || pc_type == LS_MGRB ? 9 : 7) : 3;
  if (ls_type == LS_PCG) {  // zero-filled; only their inner boxes are ever written (the fused passes read the shells as zeros)
    cg_r = czhip_alloc_s3d(size), cg_q = czhip_alloc_s3d(size), cg_p[0] = czhip_alloc_s3d(size), cg_p[1] = czhip_alloc_s3d(size);
    if (pc_type == LS_JACOBI || pc_type == LS_MG || pc_type == LS_MGRB) cg_z = czhip_alloc_s3d(size);
    // (a decomposed run: the distributed cycle, DESIGN.md §5.10 "Decomposed runs"; the coefficients are the unit ones of the command line)
    if (pc_type == LS_MG && numProc > 1 && !(mgd = mgd_create(*this, comm, cfg.num(CZV_MG_GATHER, 32768), cfg.on(CZV_MG_TAIL, true)))) {
      Hostonly_ printf("pcg with mg: the distributed V-cycle could not be set up\n");
      return 0;
    }
    if (pc_type == LS_MG && numProc == 1 && !(mg = czhip_mg_create(size, innerFidx, GUIDE, cf))) {
      Hostonly_ printf("pcg with mg: unsupported coefficients (c1 .. c6 = 1, dd = 6 only)\n");
      return 0;
    }
    if (pc_type == LS_MGRB && !(mg = czhip_mg_create_rb(size, innerFidx, GUIDE, cf))) {
      Hostonly_ printf("pcg with mgrb: unsupported coefficients (c1 .. c6 = 1, dd = 6 only)\n");
      return 0;
    }
  }
  if (!quiet) Hostonly_ {
    const double arr = (double)padded_cells() * sizeof(REAL_TYPE);
    printf("\n----------\n\n\tDevice memory per rank : %.1f MiB in %d arrays of (%d+4)x(%d+4)x(%d+4) %s\n", arr *
           narr / 1048576.0, narr, size[0], size[1], size[2],
           sizeof(REAL_TYPE) == 4 ? "float" : "double");
    if (mg) printf("\tMultigrid levels       : %d (coarse arrays about %s of one array more)\n", czhip_mg_levels(mg), pc_type == LS_MGRB ? "2/7" : "3/7");
    if (mgd) printf("\tMultigrid levels       : %d, gathered from level %d on\n", mgd_levels(mgd), mgd_gather_level(mgd));
  }

  ItrMax = atoi(argv[5]);  // :330

  auto is_line = [](int t) { return cz_solvers::row(t).family == cz_solvers::LINE; };
  if (is_line(ls_type) || is_line(pc_type)) {
    // Decomposed line SOR.  The colour and Jacobi orders exchange ghost columns after each colour / iteration: with whole k-lines per
    // brick (gdv_z = 1) they reproduce the single-domain run bit for bit.  What cannot: (a) a cut along k -- every brick then solves ITS
    // piece of a line with the neighbour's last values beyond its ends, exactly what the reference's MPI path does with CBrick bricks;
    // (b) the lexicographic orders (pcr, pcr_eda, pcr_esa, and psor), one wavefront through the whole grid -- every brick sweeps its own
    // cells in that order with the ghost values of the last exchange, one Comm_S per iteration (cz_Poisson.cpp:124, 794).  Both are
    // block-local iterations, NOT the single-domain iterate; tests/test_gpu_decomp.py pins them against the same loops restated with the
    // oracle's kernels (tests/blocklocal.py).
    MSK = czhip_alloc_s3d(size);            // :242
    imask_async(MSK, size, innerFidx, gc);  // :389
  }
  if (SW_maf) {
    // :342-363 one-dimensional grid xc[i] = (i-1)*pitch (local index; the reference adds no brick origin), uploaded once;
    // :369 search_pivot_
    REAL_TYPE** dst[3] = {&d_xc, &d_yc, &d_zc};
    for (int a = 0; a < 3; a++) {
      std::vector<REAL_TYPE> c(size[a] + 2 * gc);
      for (int i = 0; i < size[a] + 2 * gc; i++) c[i] = (REAL_TYPE)(i - 1) * pitch[a];
      HIP_CHECK(hipMalloc(dst[a], c.size() * sizeof(REAL_TYPE)));
      HIP_CHECK(hipMemcpy(*dst[a], c.data(), c.size() * sizeof(REAL_TYPE), hipMemcpyHostToDevice));
    }
    pvt = czhip_alloc_s3d(size);
    search_pivot_async(pvt, size, innerFidx, gc, d_xc, d_yc, d_zc);
  }

  // :375-386  boundary values on P and RHS, ghost layers filled from the neighbours
  // (global origin + integer brick offset instead of the brick origin: bit-identical faces on every decomposition)
  // (two ghost layers incl. edges: what a fused pair of Jacobi sweeps reads; a superset of Comm_S(X, 1))
  bc_async(size, gc, P, pitch[0], G_origin, nID, head[0] - 1, head[1] - 1);
  if (!Comm_S2(P)) return 0;
  bc_async(size, gc, RHS, pitch[0], G_origin, nID, head[0] - 1, head[1] - 1);
  if (!Comm_S2(RHS)) return 0;
  czhip_sync();
  set_up = true;
  sweeps_done = 0;
  wrk_shell_tag = 0;
  return 1;
}

// Zero-flux faces are built for pcg (none | jacobi | mg | mgrb) alone: every other loop would sweep with Dirichlet faces
bool CZ::neumann_refused(const char* who, int s_type) const {
  if ((!bc.any() && !coef_on()) || s_type == LS_PCG) return false;
  if (coef_on()) fprintf(stderr, "%s: face coefficients are set (cz_set_face_coef) and the solver is not pcg\n", who);
  else if (bc.nm) fprintf(stderr, "%s: Neumann faces are set (cz_set_neumann) and the solver is not pcg\n", who);
  else fprintf(stderr, "%s: periodic directions are set (cz_set_periodic) and the solver is not pcg\n", who);
  return true;
}

int CZ::Solve() {
  if (!set_up || neumann_refused("cz_solve", ls_type)) return 0;
  double res = 0.0, flop = 0.0;
  int itr = 0;
  // every solve starts from the current P with the bookkeeping a fresh set-up leaves (the loops clear the device flag and their counters
  // themselves; the lagged tests of an earlier solve were drained by its fused_end)
  history.clear();
  sweeps_done = 0;
  line_error = false;
  pcg_void_start = 0;
  result_itr = 0;
  result_res = 0.0;  // (a solve that returns 0 reports no iteration and no residual, not those of the solve before)
  solve_plan = PassPlan();  // (cz_info 7-9 describe this solve: a solve that plans no pass -- pcg under a mask -- reports a fresh handle's values)
  if (profile) czhip_timing(1);  // restart the section timers (the reference's PM.start/stop around the kernels)
  czhip_sync();
  const double t0 = now_s();
  if (0 == (itr = run(ls_type, res, P, RHS, ItrMax, flop))) return 0;  // :415-488
  czhip_sync();
  solve_seconds = now_s() - t0;
  result_itr = itr;
  result_res = res;

  if (fph) {
    for (size_t i = 0; i < history.size(); i++) fprintf(fph, "%6d, %13.6e\n", (int)i + 1, history[i]);  // cz_Poisson.cpp:71
    fflush(fph);
  }
  if (!quiet) Hostonly_ {  // :492-496
    printf("\n=================================\n");
    printf("Iter = %d  Res = %e\n", itr, res);
    printf("=================================\n");
  }
  return itr;
}

int CZ::Evaluate(int argc, char** argv) {
  if ((bc.any() || coef_on()) && argc > 4) {
    const cz_solvers::Row* named = cz_solvers::find(argv[4], cz_solvers::SOLVER);
    if (neumann_refused("cz_evaluate", named ? named->id : LS_NONE)) return 0;
  }
  if (!Setup(argc, argv)) return 0;
  if (!Solve()) return 0;
  if (!quiet) Hostonly_ {
    const double lups = 1.0 / res_normal * (double)(result_itr > ItrMax ? ItrMax : result_itr);
    if (!cz_solvers::krylov(cz_solvers::row(ls_type)))
      printf("\n\tGPU time = %.6f s   %.1f MLUPS\n", solve_seconds, lups / solve_seconds * 1e-6);
    else
      printf("\n\tGPU time = %.6f s\n", solve_seconds);
  }
  if (profile) {  // :506-545 (PMlib report; rank 0 writes, the others' sections are assumed alike)
    Hostonly_ {
      FILE* fp = fopen("profiling.txt", "w");
      if (!fp) {
        printf("\tSorry, can't open 'profiling.txt' file. Write failed.\n");
        return 0;
      }
      WriteProfile(fp);
      fclose(fp);
    }
  }
  if (debug_mode == 1) {  // :550-563
    int loc[3];
    // fileout_t_ has a body only in the reference's -D_aurora_=1 build (cz_utility.f90:33-44); here CZ_SPH=1 asks for the files
    const bool dump = cfg.on(CZV_SPH, false);
    char fname[32];
    if (dump) {
      snprintf(fname, sizeof(fname), "p_%05d.sph", myRank);  // :553-554
      std::vector<REAL_TYPE> p(padded_cells());
      Field(p.data());
      if (!WriteSph(fname, p.data())) return 0;
    }
    double errmax = ErrorMax(loc);
    if (!quiet) Hostonly_ printf("\nError max = %e at (%d %d %d)\n\n", errmax, loc[0], loc[1], loc[2]);
    if (dump) {
      snprintf(fname, sizeof(fname), "e_%05d.sph", myRank);  // :560-561
      std::vector<REAL_TYPE> e;
      Exact(e);
      if (!WriteSph(fname, e.data())) return 0;
    }
  }
  return 1;
}

// Bench leg: n more iterations of the stationary solver, with the complete per-iteration work of the checked loop
// (sweep, residual reduction, convergence bookkeeping) but eps disabled so that nothing is skipped.
int CZ::Sweeps(int n) {
  const cz_solvers::Family f = cz_solvers::row(ls_type).family;
  if (set_up && neumann_refused("cz_sweeps", ls_type)) return 0;
  if (!set_up || !(f == cz_solvers::JACOBI || f == cz_solvers::RBSOR || f == cz_solvers::PSOR || f == cz_solvers::LINE)) return 0;
  const double keep = eps;
  eps = -1.0;
  double res = 0.0, flop = 0.0;
  history.clear();
  solve_plan = PassPlan();
  run(ls_type, res, P, RHS, n, flop);
  eps = keep;
  sweeps_done += n;
  result_res = res;
  return n;
}

// The one place where a solver's family (cz_solvers.h) becomes the loop that runs it: Solve and Sweeps (checked), Preconditioner (unchecked,
// perhaps from a literal zero and making its right-hand side).  0: failed, as every loop returns it.
int CZ::run(int s_type, double& res, REAL_TYPE* X, REAL_TYPE* B, int itr_max, double& flop, bool converge_check, bool x_is_zero, const BMade* made) {
  switch (cz_solvers::row(s_type).family) {
    case cz_solvers::JACOBI: return JACOBI(res, X, B, itr_max, flop, s_type, converge_check, x_is_zero, made);
    case cz_solvers::RBSOR: return RBSOR(res, X, B, itr_max, flop, s_type, converge_check, x_is_zero, made);
    case cz_solvers::PSOR: return PSOR(res, X, B, itr_max, flop, s_type, converge_check);
    case cz_solvers::LINE: return LSOR(res, X, B, itr_max, flop, s_type, converge_check);
    case cz_solvers::BICGSTAB: return PBiCGSTAB(res, X, B, flop, s_type);  // (the Krylov loops run to ItrMax)
    case cz_solvers::PCG: return PCG(res, X, B, flop);
    case cz_solvers::NO_LOOP: break;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------------------
// communication wrappers (cz_comm.cpp:23-38, 102-120 of the reference)
bool CZ::Comm_S(REAL_TYPE* X, const int* skip_flag) {
  if (numProc == 1) return true;
  return comm_halo(comm, X, skip_flag, stream());
}
bool CZ::Comm_S2(REAL_TYPE* X, const int* skip_flag) {
  if (numProc == 1) return true;
  return comm_halo2(comm, X, skip_flag, stream());
}
bool CZ::Comm_SUM_dev(double* d_val, int count, const int* skip_flag) {
  if (numProc == 1) return true;
  // INVARIANT: collectives are issued unconditionally -- never gated by a device flag the host has not read, never by host timing.
  // What a rank issues depends only on its argv, on the agreed launch count and on `stop` (see CZ::FlagPoll).
  (void)skip_flag;
  return comm_allreduce_sum(comm, d_val, count, stream());
}
bool CZ::Comm_SUM_1(double* host_val) {
  if (numProc == 1) return true;
  HIP_CHECK(hipMemcpyAsync(&d_res->comm_sum, host_val, sizeof(double), hipMemcpyHostToDevice, stream()));
  if (!comm_allreduce_sum(comm, &d_res->comm_sum, 1, stream())) return false;
  *host_val = *fetch(&d_res->comm_sum);
  return true;
}

// The read-back of d_res (cz_driver.h): the mirror of a member is the same member of h_scal
template <class T> const T* CZ::fetch_queued(const T* dev, int n) {
  const void *const block = d_res, *const member = dev;
  const size_t at = (size_t)(static_cast<const char*>(member) - static_cast<const char*>(block));
  if (at + (size_t)n * sizeof(T) > sizeof(CzScalars)) cz_fatal(1, "error : a read-back beyond the device scalars\n");
  T* const host = static_cast<T*>(static_cast<void*>(static_cast<char*>(static_cast<void*>(h_scal)) + at));
  HIP_CHECK(hipMemcpyAsync(host, dev, (size_t)n * sizeof(T), hipMemcpyDeviceToHost, stream()));
  return host;
}
template <class T> const T* CZ::fetch(const T* dev, int n) {
  const T* const host = fetch_queued(dev, n);
  HIP_CHECK(hipStreamSynchronize(stream()));
  return host;
}

// WRK must carry the guide cells / faces of the array it ping-pongs with.  Single-domain runs know two kinds of shells that never change
// after set-up -- P's Dirichlet faces and the all-zero shell of the preconditioner's work vectors -- so the copy is made only when the
// kind changes (8 preconditioner solves per BiCGSTAB iteration otherwise pay 76 us each at 512^3).  Decomposed runs always copy: ghost
// cells change with every exchange.
void CZ::sync_wrk_shell(const REAL_TYPE* X) {
  const int tag = (numProc == 1) ? (X == P ? 1 : xx_shell_is_zero(X) ? 2 : 0) : 0;
  if (tag == 0 || tag != wrk_shell_tag) copy_shell_async(WRK, X, size, innerFidx, GUIDE);
  wrk_shell_tag = tag;
}

void CZ::skew_wait() const {
  if (skew_ms > 0 && myRank == skew_rank) usleep((useconds_t)skew_ms * 1000u);
}

// Split of the inner box for overlapped exchanges (pair_plan, cz_kernels.hip); n_shell = 0 when there is nothing to overlap.
void CZ::plan_overlap() {
  n_shell = 0;
  comm_cus = 0;
  if (numProc > 1 && overlap) n_shell = pair_plan(innerFidx, nID, shell_boxes, interior, interior1);
  // CUs per XCD the sweeps leave to the exchange stream while an interior launch fills the chip (RCCL's send/recv kernels need CUs of their
  // own for as long as a message is in flight; reserve_comm_cus, cz_kernels.hip): CZ_COMM_CUS, default 2, through the launch geometry --
  // at 512^3 FP32 the interior launch of the two-stage pass uses 30 of an XCD's 32 CUs anyway (profiles/r03/cu_reserve_cost.txt).  Every rank
  // reserves alike (argv and environment are the job's), also a brick without a rank-internal face: the launch geometry depends on it.
  if (numProc > 1 && overlap) {
    comm_cus = reserve_comm_cus(cfg.num(CZV_COMM_CUS, 2));
  } else {
    reserve_comm_cus(0);
  }
  if (n_shell == 0) return;
  if (!comm_stream) {
    // highest priority: pack / send-recv / unpack must get workgroup slots while the interior sweep (thousands of queued
    // workgroups on the compute stream) keeps the GPU full, or the overlap would turn into a tail
    int prio_least = 0, prio_greatest = 0;
    HIP_CHECK(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
    HIP_CHECK(hipStreamCreateWithPriority(&comm_stream, hipStreamNonBlocking, prio_greatest));
    HIP_CHECK(hipEventCreateWithFlags(&ev_shell, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&ev_src, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&ev_comm, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&ev_int, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&ev_chk[0], hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&ev_chk[1], hipEventDisableTiming));
  }
}

// One fused pair of sweeps (rb < 0) or one red-black iteration (rb = colour parity) of a decomposed run, src -> dst, with
// the two-layer exchange of dst hidden behind the interior:
//   stream      : [ev_src] -> interior ------------------------------------------> wait ev_comm -> fold slab sums -> (all-reduce, test)
//   comm_stream : wait ev_src -> shell slabs -> pack, send/recv, unpack -> [ev_comm]
// The slabs and the interior write disjoint cells of dst and read only src; the unpack writes ghost cells of dst.
// Returns false (nothing launched) when the split does not apply; the caller then takes the unsplit path.
bool CZ::pair_overlapped(REAL_TYPE* src, REAL_TYPE* dst, REAL_TYPE* B, int rb, const int* skip, double* res_slot, const MafPtrs* maf) {
  if (n_shell == 0) return false;
  double* rs = res_slot ? res_slot : d_res->pass;
  const int gc = GUIDE;
  hipStream_t st = stream();
  if (!pair_probe(src, dst, B, size, interior, interior1, gc, cf[6], maf ? 1 : 0)) return false;
  // The shell slabs and the interior read src and write disjoint cells of dst: they run side by side (round 2; round 1 ran the slabs first
  // on the compute stream, 49 us per pass of a corner brick during which the GPU was mostly idle).  The slabs go first on the exchange
  // stream, which has the higher priority, so the exchange starts as early as before.
  HIP_CHECK(hipEventRecord(ev_src, st));  // src is complete (and nobody reads dst any more) once everything issued so far on st is done
  HIP_CHECK(hipStreamWaitEvent(comm_stream, ev_src, 0));
  pair_shell_async(src, dst, B, size, idx1, shell_boxes, n_shell, gc, cf, ac1, rb, skip, comm_stream, maf);
  if (!comm_halo2(comm, dst, skip, comm_stream)) return false;
  HIP_CHECK(hipEventRecord(ev_comm, comm_stream));
  if (!pair_box_async(src, dst, B, size, interior, interior1, gc, cf, ac1, rb, rs, 0, skip, maf)) {
    cz_fatal(1, "error : interior launch refused after a successful probe\n");
  }
  HIP_CHECK(hipStreamWaitEvent(st, ev_comm, 0));
  pair_shell_fold_async(rs, rb >= 0 ? 1 : 0, skip, st);  // (behind ev_comm: the slabs have finished)
  return true;
}

// Drain the queue and turn the device-side bookkeeping into the loop's return values.
int CZ::finish_stationary(int itr_max, bool converge_check, double& res) {
  if (!converge_check) {
    // (a preconditioner solve inside BiCGSTAB returns without draining: 20-30 us of idle GPU per solve otherwise, see
    // profiles/r03/bicgstab_iteration_timeline_512_f64.txt)
    if (!in_precond) czhip_sync();
    return itr_max + 1;
  }
  HIP_CHECK(hipMemcpyAsync(h_flag, &d_flag->converged, 2 * sizeof(int), hipMemcpyDeviceToHost, stream()));  // (flag, iteration)
  HIP_CHECK(hipStreamSynchronize(stream()));
  const bool conv = h_flag[0] != 0;
  const int n_exec = conv ? h_flag[1] : itr_max;
  read_history(n_exec, res);
  return conv ? n_exec : itr_max + 1;
}

// the residuals of iterations 1..n_exec of the last checked solve, appended to `history`; res = the last of them
void CZ::read_history(int n_exec, double& res) {
  const size_t base = history.size();
  history.resize(base + n_exec);
  if (n_exec > 0) {
    HIP_CHECK(hipMemcpy(history.data() + base, d_hist + 1, (size_t)n_exec * sizeof(double), hipMemcpyDeviceToHost));
    res = history.back();
  }
}

// :67-77 after a sweep (nres = 1) or a pair of sweeps (nres = 2): all-reduce of the residual(s), then the test on the device
bool CZ::reduce_test(int nres, int itr, const int* skip) {
  if (!Comm_SUM_dev(d_res->pass, nres, skip)) return false;
  if (nres == 2) czhip_check2_async(d_res->pass, res_normal, eps, itr, d_hist, &d_flag->converged, &d_flag->iteration);
  else czhip_check_async(d_res->pass, res_normal, eps, itr, d_hist, &d_flag->converged, &d_flag->iteration);
  return true;
}

// the residual sum of the sweep(s) just issued, read back behind them: NaN = the sweep gave up a wait between its workgroups (pcr_lex_wg_k)
bool CZ::sweep_failed(const char* solver) {
  if (!std::isnan(*fetch(d_res->pass))) return false;
  fprintf(stderr, "cz rank %d: %s: the residual of a sweep is NaN -- a hand-off between the workgroups of the one-launch lexicographic sweep did "
                  "not arrive within its bound (czhip_set_pcr_lex_timeout), or the data hold NaN.  The iterate is void.  CZHIP_PCR_PIPE=0 selects "
                  "the launch-per-diagonal form.\n", myRank, solver);
  line_error = true;
  return true;
}

// ------------------------------------------------------------------------------------------------------------
// How the sweeps of a stationary solve (or of a preconditioner solve) are executed.  Decided ONCE, before the loop, from what is known
// then -- solver flavour, iteration budget, whether convergence is tested, the geometry probes of the two-stage pass, what the ranks
// agreed on at set-up -- and then carried out by the loop without further choices.  (Round 2 chose among five launch paths inside the loop,
// iteration by iteration, with fallbacks from one to the next.)
//   kind     SINGLE  one sweep (one colour) per launch, one-layer exchange after each                         cz_Poisson.cpp:58-63, 205-215
//            WHOLE   two Jacobi sweeps / one red-black iteration per pass over memory (jacobi2p_k), two-layer exchange after the pass
//            SPLIT   the same pass as shell slabs + interior; the exchange runs on the exchange stream beside the interior (decomposed runs)
//   lag      SPLIT + convergence test: residual all-reduce and test one pass behind, on the exchange stream; three rotating buffers
//   zero_start  the start vector is identically zero and the first pass takes it as a literal (first pair of a preconditioner solve)
// What the ranks of a decomposed run must agree on is the sequence of collectives: the exchange depth (SINGLE against the fused kinds --
// `pairs_ok`, all-reduced at set-up) and the iteration at which they stop (the poll below).  WHOLE against SPLIT and lag against no lag may
// differ from brick to brick (a brick too thin to split): the same exchanges and all-reduces in the same order either way.
CZ::PassPlan CZ::plan_pass(REAL_TYPE* X, REAL_TYPE* B, int s_type, int itr_max, bool converge_check, bool x_is_zero, bool rb, bool probe_only) {
  PassPlan p;
  p.maf = cz_solvers::row(s_type).maf ? 1 : 0;
  p.rb = rb ? 1 : 0;
  p.comm_cus = comm_cus;
  bool fused = czhip_use_t2() != 0 && (rb || itr_max >= 2);
  if (fused) {
    const bool mine = pair_probe(X, WRK, B, size, innerFidx, idx1, GUIDE, cf[6], p.maf) != 0;
    if (numProc > 1 && pairs_ok && !mine) {  // (pairs_ok was probed on P / WRK / RHS: same geometry, same alignment)
      cz_fatal(1, "cz rank %d: the fused pass the ranks agreed on at set-up is refused for this solve\n", myRank);
    }
    fused = numProc > 1 ? pairs_ok : mine;
  }
  if (fused) {
    p.kind = PassPlan::WHOLE, p.depth = 2;
    if (numProc > 1 && n_shell > 0 && pair_probe(X, WRK, B, size, interior, interior1, GUIDE, cf[6], p.maf)) p.kind = PassPlan::SPLIT;
    p.lag = (p.kind == PassPlan::SPLIT && converge_check && lag_reduce != 0) ? 1 : 0;
    p.buffers = p.lag ? 3 : 2;
    p.zero_start = (x_is_zero && numProc == 1 && !converge_check && !p.maf && (rb || itr_max >= 2)) ? 1 : 0;
  }
  if (probe_only) return p;  // a question (bicg_fusable), not a solve: cz_info 7..9 and the debug line keep describing solves that ran
  if (cfg.has(CZV_COMM_DEBUG) && numProc > 1 && (p.kind != last_plan.kind || p.lag != last_plan.lag || p.maf != last_plan.maf || p.rb != last_plan.rb || !plan_printed)) {
    static const char* const kinds[] = {"single sweeps", "fused pass, whole box", "fused pass, shell + interior (exchange overlapped)"};
    fprintf(stderr, "cz rank %d: %s plan: %s, exchange depth %d, lagged reduce %d, buffers %d, zero start %d, maf %d, comm CUs per XCD %d\n", myRank,
            rb ? "RBSOR" : "JACOBI", kinds[p.kind], p.depth, p.lag, p.buffers, p.zero_start, p.maf, p.comm_cus);
    plan_printed = true;
  }
  last_plan = p;
  solve_plan = p;
  return p;
}

// ------------------------------------------------------------------------------------------------------------
// The host's lagging, non-blocking view of the device convergence flag.  Each poll issues a stream-ordered copy of d_flag->converged and looks at
// the copy issued two polls earlier; the caller decides when to poll (its cadence).  The events are released with the poller, early returns
// included.
// INVARIANT (rank lock step): the answer decides whether this rank issues further passes, i.e. further collectives.  It is a function of
// the copy two polls back only: a copy of the device flag taken at a fixed position of the stream (lagged mode: behind the tests of all
// passes issued up to that poll, which run on the exchange stream), and the flag is computed from all-reduced sums -- the same bits on every
// rank.  When the host gets to look at the copy (skew_wait: a test delays one rank here) cannot change what it reads.
class CZ::FlagPoll {
 public:
  FlagPoll(CZ& cz, bool lag) : cz_(cz), lag_(lag) {}
  ~FlagPoll() {
    for (int i = 0; i < std::min(npoll_, POLL_SLOTS); i++) HIP_CHECK(hipEventDestroy(ev_[i]));
  }
  FlagPoll(const FlagPoll&) = delete;
  FlagPoll& operator=(const FlagPoll&) = delete;
  // true: the flag was set (the solve has converged) as of two polls ago
  bool stop() {
    const int slot = npoll_ % POLL_SLOTS;
    if (npoll_ >= POLL_SLOTS) HIP_CHECK(hipEventDestroy(ev_[slot]));
    if (lag_) cz_.wait_lagged_tests();  // every rank must read the same flag: the copy follows the tests of all passes issued so far
    HIP_CHECK(hipMemcpyAsync(cz_.h_flag + 2 * slot, &cz_.d_flag->converged, sizeof(int), hipMemcpyDeviceToHost, stream()));
    HIP_CHECK(hipEventCreateWithFlags(&ev_[slot], hipEventDisableTiming));
    HIP_CHECK(hipEventRecord(ev_[slot], stream()));
    if (++npoll_ < 3) return false;
    const int old = (npoll_ - 3) % POLL_SLOTS;
    cz_.skew_wait();
    HIP_CHECK(hipEventSynchronize(ev_[old]));
    return cz_.h_flag[2 * old] != 0;
  }

 private:
  CZ& cz_;
  const bool lag_;
  hipEvent_t ev_[POLL_SLOTS];
  int npoll_ = 0;
};

// lagged mode: the compute stream waits for the convergence tests still in flight on the exchange stream
void CZ::wait_lagged_tests() {
  HIP_CHECK(hipStreamWaitEvent(stream(), ev_chk[0], 0));
  HIP_CHECK(hipStreamWaitEvent(stream(), ev_chk[1], 0));
}

// What JACOBI and RBSOR share around their choice of kernels.  The field rotates through buf[0 .. nbuf) -- X, WRK and, lagged, WRK2 -- and
// every launch of a fused plan is recorded (first iteration, iterations, source buffer) so that the state at the converged iteration can be
// produced exactly (fused_end).
class CZ::FusedLoop {
 public:
  FusedLoop(CZ& cz, const PassPlan& p, REAL_TYPE* b, bool check) : plan(p), B(b), converge_check(check), nbuf(p.buffers), poll(cz, p.lag != 0) {}
  const PassPlan& plan;
  REAL_TYPE* const B;
  const bool converge_check;
  const int* skip = nullptr;  // checked solves: d_flag->converged (launches queued after convergence are no-ops)
  REAL_TYPE* buf[3] = {nullptr, nullptr, nullptr};
  const int nbuf;
  int cur = 0;
  std::vector<Launch> launches;
  FlagPoll poll;
  REAL_TYPE* src() const { return buf[cur]; }
  REAL_TYPE* dst() const { return buf[(cur + 1) % nbuf]; }
  void record(int itr, int n) {
    launches.push_back({itr, n, cur});
    cur = (cur + 1) % nbuf;
  }
};

// The start of a JACOBI / RBSOR solve, after its plan.  Every ping-pong reads X's shell and ghost cells from WRK (and WRK2) as well.
bool CZ::fused_begin(FusedLoop& L, REAL_TYPE* X, int itr_max, bool x_is_zero, const BMade* made) {
  const PassPlan& plan = L.plan;
  if (made && !(plan.kind == PassPlan::WHOLE && plan.zero_start)) {  // (bicg_fusable asked the same questions before the update was withheld)
    cz_fatal(1, "error : the solve that was to make its right-hand side does not start with a whole fused pass from zero\n");
  }
  exact_reruns = 0;
  if (x_is_zero && !plan.zero_start) {
    // the caller skipped its blas_clear_ (cz_Poisson.cpp:405, 441) and this solve does not take the zero as a literal: clear now
    // (guide cells / faces are zero already)
    HIP_CHECK(hipMemsetAsync(X, 0, padded_cells() * sizeof(REAL_TYPE), stream()));
  }
  reset_ticket();
  if (L.converge_check) {
    ensure_hist(itr_max + 3);
    HIP_CHECK(hipMemsetAsync(d_flag, 0, sizeof(CzFlags), stream()));  // flag, iteration, the two snapshots of the lagged mode
    L.skip = &d_flag->converged;
  }
  // the fused pass reads two ghost layers (and the edge cells) of X and one of B
  if (plan.depth == 2 && numProc > 1 && (!Comm_S2(X) || !Comm_S2(L.B))) return false;
  L.buf[0] = X, L.buf[1] = WRK;
  if (!plan.rb || plan.kind != PassPlan::SINGLE) sync_wrk_shell(X);  // ping-pong partner (the red-black SINGLE plan sweeps in place)
  // Lagged mode (decomposed, checked runs): the residual all-reduce and the convergence test of pass n run on the exchange stream while
  // pass n+1 is being swept (pass n+2 waits for the test of pass n).  A pass may therefore run beyond convergence once; with THREE rotating
  // buffers it cannot touch the source or the destination of the converged pass, so the exact-iteration fix-up (fused_end) still finds both.
  if (plan.lag) {
    if (!WRK2) WRK2 = czhip_alloc_s3d(size);
    copy_shell_async(WRK2, X, size, innerFidx, GUIDE);
    L.buf[2] = WRK2;
  }
  return true;
}

// One SPLIT pass src -> dst (pair_overlapped) with its all-reduce and test: rb < 0 two Jacobi sweeps (nres = 2 residuals), else one
// red-black iteration of colour parity rb (nres = 1).  Pass p is the p-th launch of the solve.
bool CZ::split_pass(FusedLoop& L, int rb, int nres, int itr, const MafPtrs* mpp) {
  if (!L.plan.lag) {
    if (!pair_overlapped(L.src(), L.dst(), L.B, rb, L.skip, nullptr, mpp)) return false;  // :58 (:205-209), :63 (:215) behind the interior
    return !L.converge_check || reduce_test(nres, itr, L.skip);                          // :67-77
  }
  hipStream_t st = stream();
  const int p = (int)L.launches.size();
  if (p >= 2) HIP_CHECK(hipStreamWaitEvent(st, ev_chk[p & 1], 0));  // the test of pass p-2
  double* rs = d_res->lagged[p & 1];
  // Pass p looks at the flag as the test of pass p-2 left it (d_flag->snap[p & 1], written by that test and by nothing else until
  // pass p is over): every workgroup of the pass, its pack and its unpack take the same decision.  The live flag d_flag->converged may be
  // set by the test of pass p-1 while pass p is running.
  int* snap = &d_flag->snap[p & 1];
  if (!pair_overlapped(L.src(), L.dst(), L.B, rb, snap, rs, mpp)) return false;
  HIP_CHECK(hipEventRecord(ev_int, st));
  HIP_CHECK(hipStreamWaitEvent(comm_stream, ev_int, 0));
  if (!comm_allreduce_sum(comm, rs, nres, comm_stream)) return false;  // :67, all the pass's residuals
  if (nres == 2) check2_on_stream(comm_stream, rs, res_normal, eps, itr, d_hist, &d_flag->converged, &d_flag->iteration, snap);  // :69-77
  else check_on_stream(comm_stream, rs, res_normal, eps, itr, d_hist, &d_flag->converged, &d_flag->iteration, snap);
  HIP_CHECK(hipEventRecord(ev_chk[p & 1], comm_stream));
  return true;
}

// After a WHOLE pass of a decomposed run: the two layers of its destination once per pass (:63, :215), one all-reduce of all the pass's
// residuals and the test (:67-77)
bool CZ::whole_exchange_test(FusedLoop& L, int nres, int itr) {
  if (numProc == 1) return true;
  if (!Comm_S2(L.dst(), L.skip)) return false;
  return !L.converge_check || reduce_test(nres, itr, L.skip);
}

// The first pass of a preconditioner solve whose start vector is identically zero: neither cleared in memory nor read; with `made` the
// right-hand side is made on the way (BiCGSTAB's vector update folded in).  rb < 0: two Jacobi sweeps, else one red-black iteration.
int CZ::zero_start_pass(REAL_TYPE* src, REAL_TYPE* dst, REAL_TYPE* B, const BMade* made, int rb) {
  static const BMade read_b{0, nullptr, nullptr, nullptr, (REAL_TYPE)0, (REAL_TYPE)0, nullptr};
  const BMade& m = made ? *made : read_b;
  return pass_from_zero_made(src, dst, B, m.op, m.x, m.y, m.z, m.a, m.a_dev, m.b, size, innerFidx, idx1, GUIDE, cf, ac1, rb, d_res->pass, 0);
}

// The end of a JACOBI / RBSOR solve: drain, read the bookkeeping back, and hand the iterate of the converged (or last) iteration to the
// caller.  Launches after convergence were no-ops or -- lagged mode -- wrote the third buffer.  A launch whose converged iteration is not
// its last wrote later iterates into its destination; its source is untouched, so `rerun(launch, k, src, dst)` -- k = the converged
// iteration's index within the launch -- reproduces the converged iterate from it (exactly what the sequential loop holds).
int CZ::fused_end(FusedLoop& L, REAL_TYPE* X, int itr_max, double& res, const Rerun& rerun) {
  if (L.plan.lag) HIP_CHECK(hipStreamSynchronize(comm_stream));  // the last tests
  last_lag = L.plan.lag;
  const int ret = finish_stationary(itr_max, L.converge_check, res);
  if (L.launches.empty()) return ret;
  const Launch* last = &L.launches.back();
  if (L.converge_check && ret <= itr_max) {  // converged at iteration `ret`: the launch that contains it
    for (const Launch& l : L.launches)
      if (ret >= l.first_itr && ret < l.first_itr + l.n) {
        last = &l;
        break;
      }
    if (ret < last->first_itr + last->n - 1) {
      rerun(*last, ret - last->first_itr, L.buf[last->src], L.buf[(last->src + 1) % L.nbuf]);
      exact_reruns++;
    }
  }
  const int fb = (last->src + 1) % L.nbuf;
  if (fb != 0) {
    // the result is in WRK (or WRK2).  The arrays are ours: swap the roles instead of copying back.
    if (X == P) {
      REAL_TYPE* t = P;
      P = L.buf[fb];
      if (fb == 1) WRK = t;
      else WRK2 = t;
    } else {
      copy_inner_async(X, L.buf[fb], size, innerFidx, GUIDE);
    }
  }
  return ret;
}

// ------------------------------------------------------------------------------------------------------------
// cz_Poisson.cpp:30-82.  Ping-pong X <-> WRK; fused plans apply the sweeps two (or three) at a time per pass over memory (temporal blocking,
// the intermediate field stays on chip).
int CZ::JACOBI(double& res, REAL_TYPE* X, REAL_TYPE* B, const int itr_max, double& flop, int s_type, bool converge_check,
               bool x_is_zero, const BMade* made) {
  const int gc = GUIDE;
  const PassPlan plan = plan_pass(X, B, s_type, itr_max, converge_check, x_is_zero, false);
  const bool maf = plan.maf != 0;  // cz_Poisson.cpp:45-53
  const MafPtrs mp{d_xc, d_yc, d_zc, nullptr};
  const MafPtrs* mpp = maf ? &mp : nullptr;
  FusedLoop L(*this, plan, B, converge_check);
  if (!fused_begin(L, X, itr_max, x_is_zero, made)) return 0;
  const int* skip = L.skip;
  // One Jacobi pass of n sweeps s -> d: n = 3, 4 through the deep entries (jac3_k, jac4_k), n = 2 the pair; the sums go to rs[0 .. n-1].
  // check: with the solve's bookkeeping for iteration it (:58 + :67-77, n times) and its skip flag; else bare, as the probes and re-runs are
  auto jacobi_pass = [&](int n, REAL_TYPE* s, REAL_TYPE* d, double* rs, bool check, int it, int probe) -> int {
    const double rn = check ? res_normal : 0.0, ep = check ? eps : 0.0;
    double* hist = (check && converge_check) ? d_hist : nullptr;
    int* flag = check ? &d_flag->converged : nullptr;
    int* conv = check ? &d_flag->iteration : nullptr;
    const int* sk = check ? skip : nullptr;
    if (n == 4) return czhip_jacobi4_async(s, d, B, size, innerFidx, gc, cf, ac1, rs, rn, ep, it, hist, flag, conv, sk, probe);
    if (n == 3) return czhip_jacobi3_async(s, d, B, size, innerFidx, gc, cf, ac1, rs, rn, ep, it, hist, flag, conv, sk, probe);
    return czhip_jacobi2_async(s, d, B, size, innerFidx, idx1, gc, cf, ac1, rs, rn, ep, it, hist, flag, conv, sk);
  };
  // THREE sweeps per pass (jac3_k) where the whole inner box is one launch of one rank with constant coefficients, outside a preconditioner
  // solve; triples while three sweeps remain, then the pair or the single sweep
  const bool jac3 = plan.kind == PassPlan::WHOLE && numProc == 1 && !maf && !in_precond && itr_max >= 3 && jacobi_pass(3, X, WRK, d_res->pass, false, 0, 1) != 0;
  // FOUR sweeps per pass (jac4_k) where that pass takes the box as well and the solve is long enough (czhip_jac4_min_sweeps: a solve of
  // fewer than eight sweeps keeps the triples it had, the passes cz_info 14 reports): quads while four sweeps remain, then the triple,
  // the pair or the single sweep
  const bool jac4 = jac3 && itr_max >= czhip_jac4_min_sweeps() && jacobi_pass(4, X, WRK, d_res->pass, false, 0, 1) != 0;
  jac3_passes = 0, jac4_passes = 0;
  bool stop = false;
  int itr = 1;
  while (itr <= itr_max && !stop) {
    REAL_TYPE* src = L.src();
    REAL_TYPE* dst = L.dst();
    int done = 2;
    const bool pass = plan.kind != PassPlan::SINGLE && itr + 1 <= itr_max;
    if (pass && plan.kind == PassPlan::SPLIT) {
      if (!split_pass(L, -1, 2, itr, mpp)) return 0;  // :58 twice, :63 hidden behind the interior, :67-77 for both sweeps
    } else if (pass && jac3 && itr + 2 <= itr_max && !(plan.zero_start && itr == 1)) {
      done = (jac4 && itr + 3 <= itr_max) ? 4 : 3;  // :58 + :67-77, `done` times (pass[0 .. done-1]; the re-runs below write `rerun`)
      if (!jacobi_pass(done, src, dst, d_res->pass, true, itr, 0)) {
        cz_fatal(1, "error : the %s-sweep pass refused after a successful probe\n", done == 4 ? "four" : "three");
      }
      (done == 4 ? jac4_passes : jac3_passes)++;
    } else if (pass) {  // the whole inner box in one launch
      const bool in_kernel_check = converge_check && numProc == 1;
      int launched;
      if (plan.zero_start && itr == 1)
        launched = zero_start_pass(src, dst, B, made, -1);
      else if (maf)
        launched = pair_maf_async(src, dst, B, size, innerFidx, idx1, gc, d_xc, d_yc, d_zc, ac1, -1, d_res->pass, res_normal, eps, itr,
                                  in_kernel_check ? d_hist : nullptr, &d_flag->converged, &d_flag->iteration, skip);  // :45-53 twice
      else
        launched = czhip_jacobi2_async(src, dst, B, size, innerFidx, idx1, gc, cf, ac1, d_res->pass, res_normal, eps, itr,
                                       in_kernel_check ? d_hist : nullptr, &d_flag->converged, &d_flag->iteration, skip);  // :58 + :67-77, twice
      if (!launched) {
        cz_fatal(1, "error : fused pass refused after a successful probe\n");
      }
      if (!whole_exchange_test(L, 2, itr)) return 0;
    } else {  // one sweep: the SINGLE plan, or the odd last sweep of a fused one
      if (plan.lag) wait_lagged_tests();  // the tests still in flight on the exchange stream come first
      const bool fused_check = converge_check && numProc == 1;  // no all-reduce between sweep and test: one launch
      if (maf)
        jacobi_maf_async(src, dst, B, size, innerFidx, gc, d_xc, d_yc, d_zc, ac1, d_res->pass, skip, fused_check ? 1 : 0, res_normal, eps,
                         itr, d_hist, &d_flag->converged, &d_flag->iteration);
      else if (fused_check)
        czhip_jacobi_checked_async(src, dst, B, size, innerFidx, gc, cf, ac1, d_res->pass, res_normal, eps, itr, d_hist,
                                   &d_flag->converged, &d_flag->iteration);  // :58 + :67-77
      else
        czhip_jacobi_async(src, dst, B, size, innerFidx, gc, cf, ac1, d_res->pass, 0, skip);  // :58
      if (!Comm_S(dst, skip)) return 0;                                             // :63
      if (converge_check && !fused_check && !reduce_test(1, itr, skip)) return 0;  // :67-77
      done = 1;
    }
    flop += (maf ? 66.0 : 18.0) * npts() * done;
    L.record(itr, done);
    itr += done;
    if (converge_check && L.launches.size() % (POLL_EVERY / 2) == 0 && itr <= itr_max) stop = L.poll.stop();
  }
  return fused_end(L, X, itr_max, res, [&](const Launch& l, int k, REAL_TYPE* s, REAL_TYPE* d) {
    // k + 1 sweeps from the launch's source: a triple, a pair, or one plain sweep
    if (k >= 1) {
      if (!jacobi_pass(k + 1, s, d, d_res->rerun, false, 0, 0)) {
        cz_fatal(1, "error : %s refused after a successful probe\n", k == 2 ? "the three-sweep pass" : "fused pass");
      }
    } else if (maf) {  // the first sweep of a fused pass: one plain sweep
      jacobi_maf_async(s, d, B, size, innerFidx, gc, d_xc, d_yc, d_zc, ac1, d_res->rerun, nullptr, 0, 0.0, 0.0, 0, nullptr, nullptr, nullptr);
    } else {
      czhip_jacobi_async(s, d, B, size, innerFidx, gc, cf, ac1, d_res->rerun, 0, nullptr);
    }
  });
}

// cz_Poisson.cpp:159-235
int CZ::RBSOR(double& res, REAL_TYPE* X, REAL_TYPE* B, const int itr_max, double& flop, int s_type, bool converge_check, bool x_is_zero,
              const BMade* made) {
  const int gc = GUIDE;
  const PassPlan plan = plan_pass(X, B, s_type, itr_max, converge_check, x_is_zero, true);
  const bool maf = plan.maf != 0;  // cz_Poisson.cpp:190-200
  const MafPtrs mp{d_xc, d_yc, d_zc, nullptr};
  const MafPtrs* mpp = maf ? &mp : nullptr;
  FusedLoop L(*this, plan, B, converge_check);
  if (!fused_begin(L, X, itr_max, x_is_zero, made)) return 0;
  const int* skip = L.skip;
  // :178-186.  ip makes colour 0 the points of even GLOBAL i+j+k; the kernel's parity is relative to kst
  // (cz_solver.f90:466), which is 1 instead of 2 on a face that borders another rank.
  int ip = 0;
  if (numProc > 1) ip = (head[0] + head[1] + head[2] + 1 + innerFidx[K_minus]) % 2;

  // Fused plans: the whole iteration (colour 0, then colour 1) in ONE pass over memory, out of place X <-> WRK; decomposed runs then
  // exchange two ghost layers once per iteration.  SINGLE: the reference's two in-place colour launches with an exchange after each colour.
  // Round 4: TWO iterations per pass over memory (rb4_k) where the whole inner box is one launch of one rank with constant coefficients.
  const bool rb4 = plan.kind == PassPlan::WHOLE && numProc == 1 && !maf &&
                   czhip_rbsor4_async(X, WRK, B, size, innerFidx, gc, cf, ip, ac1, d_res->pass, 0.0, 0.0, 0, nullptr, nullptr, nullptr, nullptr, 1) != 0;
  rb4_passes = 0;
  bool stop = false;
  int itr = 1;
  while (itr <= itr_max && !stop) {
    int done = 1;
    const bool in_kernel_check = converge_check && numProc == 1;
    REAL_TYPE* src = L.src();
    REAL_TYPE* dst = L.dst();
    if (plan.kind == PassPlan::SPLIT) {
      if (!split_pass(L, rb_par(gc, innerFidx, ip), 1, itr, mpp)) return 0;
    } else if (plan.kind == PassPlan::WHOLE && rb4 && itr + 1 <= itr_max && !(plan.zero_start && itr == 1)) {
      if (!czhip_rbsor4_async(src, dst, B, size, innerFidx, gc, cf, ip, ac1, d_res->pass, res_normal, eps, itr, in_kernel_check ? d_hist : nullptr,
                              &d_flag->converged, &d_flag->iteration, skip, 0)) {  // :205-209 twice (+ :218-230 for both iterations)
        cz_fatal(1, "error : the two-iteration red-black pass refused after a successful probe\n");
      }
      done = 2;
      rb4_passes++;
    } else if (plan.kind == PassPlan::WHOLE) {
      const int launched = (plan.zero_start && itr == 1) ? zero_start_pass(src, dst, B, made, ip)
                           : maf ? pair_maf_async(src, dst, B, size, innerFidx, idx1, gc, d_xc, d_yc, d_zc, ac1, ip, d_res->pass, res_normal, eps, itr,
                                                in_kernel_check ? d_hist : nullptr, &d_flag->converged, &d_flag->iteration, skip)  // :190-200
                               : czhip_rbsor2_async(src, dst, B, size, innerFidx, idx1, gc, cf, ip, ac1, d_res->pass, res_normal, eps, itr,
                                                    in_kernel_check ? d_hist : nullptr, &d_flag->converged, &d_flag->iteration, skip);  // :205-209 (+ :218-230)
      if (!launched) {
        cz_fatal(1, "error : fused red-black iteration refused after a successful probe\n");
      }
      if (!whole_exchange_test(L, 1, itr)) return 0;
    } else {
      for (int color = 0; color < 2; color++) {  // :205-209
        if (maf)
          rbsor_maf_async(X, B, size, innerFidx, gc, d_xc, d_yc, d_zc, ip, color, ac1, d_res->pass, color, skip,
                          (in_kernel_check && color == 1) ? 1 : 0, res_normal, eps, itr, d_hist, &d_flag->converged, &d_flag->iteration);
        else if (in_kernel_check && color == 1)
          czhip_rbsor_checked_async(X, B, size, innerFidx, gc, cf, ip, color, ac1, d_res->pass, 1, res_normal, eps, itr, d_hist,
                                    &d_flag->converged, &d_flag->iteration);
        else
          czhip_rbsor_async(X, B, size, innerFidx, gc, cf, ip, color, ac1, d_res->pass, color, skip);
        // the reference exchanges once per iteration (:215); exchanging after each colour makes the decomposed run
        // identical to the single-domain one
        if (!Comm_S(X, skip)) return 0;
      }
      if (converge_check && !in_kernel_check && !reduce_test(1, itr, skip)) return 0;
    }
    flop += (maf ? 66.0 : 18.0) * npts() * done;
    if (plan.kind != PassPlan::SINGLE) L.record(itr, done);
    const int last_done = itr + done - 1;
    const bool poll_now = last_done / POLL_EVERY > (itr - 1) / POLL_EVERY;  // a multiple of POLL_EVERY iterations was completed by this launch
    itr += done;
    if (converge_check && poll_now && last_done < itr_max) stop = L.poll.stop();
  }
  // the first iteration of a two-iteration pass converged: one fused iteration
  return fused_end(L, X, itr_max, res, [&](const Launch&, int, REAL_TYPE* s, REAL_TYPE* d) {
    if (!czhip_rbsor2_async(s, d, B, size, innerFidx, idx1, gc, cf, ip, ac1, d_res->rerun, 0.0, 0.0, 0, nullptr, nullptr, nullptr, nullptr)) {
      cz_fatal(1, "error : fused red-black iteration refused after a successful probe\n");
    }
  });
}

// cz_Poisson.cpp:95-146.  Lexicographic point SOR, in place; one sweep = the launches of psor_async (tile hyperplanes).
int CZ::PSOR(double& res, REAL_TYPE* X, REAL_TYPE* B, const int itr_max, double& flop, int s_type, bool converge_check) {
  const bool maf = cz_solvers::row(s_type).maf;  // :108-114
  const int gc = GUIDE;
  reset_ticket();
  const int* skip = nullptr;
  if (converge_check) {
    ensure_hist(itr_max + 2);
    HIP_CHECK(hipMemsetAsync(d_flag, 0, offsetof(CzFlags, snap), stream()));  // flag, iteration
    skip = &d_flag->converged;
  }
  FlagPoll poll(*this, false);
  bool stop = false;
  for (int itr = 1; itr <= itr_max && !stop; itr++) {
    psor_async(X, B, size, innerFidx, gc, cf, maf ? d_xc : nullptr, d_yc, d_zc, ac1, d_res->pass, 0, skip);  // :108-122
    flop += (maf ? 66.0 : 18.0) * npts();
    if (!Comm_S(X, skip)) return 0;  // :124 (decomposed: block-local sweeps, ghosts of the last exchange)
    if (converge_check) {
      if (!reduce_test(1, itr, skip)) return 0;                              // :127-141 on the device
      if (itr % POLL_EVERY == 0 && itr < itr_max) stop = poll.stop();
    }
  }
  const int ret = finish_stationary(itr_max, converge_check, res);
  if (psor_failed()) {  // a column of the one-launch sweep gave up waiting for the columns before it: the iterate is void
    fprintf(stderr, "cz rank %d: %s: a sweep gave up a hand-off between its workgroups (bound: czhip_set_pcr_lex_timeout); the iterate is void.  "
                    "CZHIP_PSOR=0 selects the launch-per-tile-hyperplane form.\n", myRank, printMethod(s_type));
    line_error = true;
    return 0;
  }
  return ret;
}

// ------------------------------------------------------------------------------------------------------------
// The line solvers' shared steps.  pcr_num_stage of the k lines (:535-538): no stage count, no solve.
int CZ::line_stages() {
  const int pn = pcr_num_stage(innerFidx[K_plus] - innerFidx[K_minus] + 1);
  if (pn < 0) {
    printf("error : number of stage\n");
    exit(0);
  }
  return pn;
}

// The test after an iteration (:584-601).  The line solves are long launches: a host round trip per iteration is negligible, so the
// reference's sequential test is kept as is.  1: converged, 0: go on, -1: failed (message printed).
int CZ::line_test(int itr, int s_type) {
  if (!reduce_test(1, itr)) return -1;
  HIP_CHECK(hipMemcpyAsync(h_flag, &d_flag->converged, sizeof(int), hipMemcpyDeviceToHost, stream()));
  if (sweep_failed(printMethod(s_type))) return -1;  // (synchronises)
  return h_flag[0] ? 1 : 0;
}

// The end of a line solve: the history of the iterations executed, or (unchecked) the NaN test of the last sweep.
int CZ::line_finish(int itr, int itr_max, bool converge_check, double& res, int s_type) {
  if (!converge_check) return sweep_failed(printMethod(s_type)) ? 0 : itr;  // (synchronises)
  read_history(itr > itr_max ? itr_max : itr, res);
  return itr;
}

// One iteration of a line solver as its row describes it (cz_solvers.h): the launches of a kernel family in a column order, with the
// exchanges that follow them.  false: an exchange failed.
//   order 0  colour 0 then colour 1, in place (cz_Poisson.cpp:573-578, 685-690).  mod(i+j, 2) == colour is meant in GLOBAL indices: the
//            brick's local rule is shifted by its head (the reference's MPI path ignores this, cz_solver.f90:534 "unused variable"; here
//            decomposed == single domain), and the ghost columns are exchanged after each colour, like the two-colour RB-SOR
//   order 1  one lexicographic sweep (:783-786, :966-969), exchange :794 (decomposed: block-local, see CZ::Setup)
//   order 2  Jacobi order into WRK (:1061-1064), copied back, exchange :1068
bool CZ::line_iteration(const cz_solvers::Line& d, REAL_TYPE* X, REAL_TYPE* B, int pn) {
  const int gc = GUIDE;
  auto launch = [&](int par, int slot) {
    switch (d.kernel) {
      case cz_solvers::PCR_RB: pcr_rb_async(X, MSK, B, size, innerFidx, gc, pn, par, ac1, d_res->pass, slot); break;
      case cz_solvers::PCR_VARIANT: pcr_variant_async(X, d.order == 2 ? WRK : nullptr, MSK, B, size, innerFidx, gc, pn, d.order, par, d.final4, ac1, d_res->pass, slot); break;
      case cz_solvers::PCR_MAF: pcr_maf_async(X, MSK, B, size, innerFidx, gc, pn, d.order, par, d_xc, d_yc, d_zc, ac1, d_res->pass, slot); break;
      case cz_solvers::NO_LINE: break;
    }
  };
  if (d.order == 0) {
    for (int color = 0; color < 2; color++) {
      launch((color + head[0] + head[1]) & 1, color);
      if (!Comm_S(X)) return false;
    }
    return true;
  }
  launch(0, 0);
  if (d.order == 2) copy_inner_async(X, WRK, size, innerFidx, gc);
  return Comm_S(X);
}

// The reference's operation count of one iteration, per kernel family: pcr_rb (cz_Poisson.cpp:580), the variants that end in 4x4 systems
// and / or visit the columns in another order (:692, :788, :971, :1066), the MAF flavour (pn-1 stages + 2x2 systems, :559)
double CZ::line_flop(const cz_solvers::Line& d, int pn) const {
  const int n = innerFidx[K_plus] - innerFidx[K_minus] + 1;
  if (d.kernel == cz_solvers::PCR_RB) return npts() * (12.0 + (pn - 1) * 14.0);
  if (d.kernel == cz_solvers::PCR_MAF)
    return (npts() / n) * ((24.0 + 6.0 + 12.0) + n * 21.0 + (n - 2.0) * 6.0 + n * (double)(pn - 1) * 16.0 + (double)(1 << (pn - 1)) * d.fin + n * 6.0);
  const int stages = d.final4 ? pn - 2 : pn - 1;
  return (npts() / n) * (n * 6.0 + n * (double)stages * 14.0 + (double)(1 << stages) * d.fin + n * 6.0 + 6.0);
}

// cz_Poisson.cpp:518-611 (pcr_rb), :621-742 (pcr_rb_esa), :745-826 (pcr), :829-907 (pcr_eda), :910-1005 (pcr_esa), :1008-1095 (pcr_j_esa) and
// their MAF flavours: line SOR, every (i,j) column solved along k by parallel cyclic reduction.  One loop; the row says what an iteration is.
int CZ::LSOR(double& res, REAL_TYPE* X, REAL_TYPE* B, const int itr_max, double& flop, int s_type, bool converge_check) {
  const cz_solvers::Line& d = cz_solvers::row(s_type).line;
  reset_ticket();
  const int pn = line_stages();
  if (converge_check) {
    ensure_hist(itr_max + 2);
    HIP_CHECK(hipMemsetAsync(d_flag, 0, offsetof(CzFlags, snap), stream()));  // flag, iteration
  }
  int itr;
  for (itr = 1; itr <= itr_max; itr++) {
    if (!line_iteration(d, X, B, pn)) return 0;
    flop += line_flop(d, pn);
    if (converge_check) {
      const int t = line_test(itr, s_type);
      if (t < 0) return 0;
      if (t > 0) break;
    }
  }
  return line_finish(itr, itr_max, converge_check, res, s_type);
}

// cz_Poisson.cpp:239-270.  The reference reduces in REAL on every rank and all-reduces the REAL; here the double
// partial sums are all-reduced and rounded to REAL once.
REAL_TYPE CZ::Fdot1(REAL_TYPE* x, double& flop) {
  dot1_async(x, size, innerFidx, GUIDE, &d_res->fdot);
  return dot_read(flop);
}

REAL_TYPE CZ::Fdot2(REAL_TYPE* x, REAL_TYPE* y, double& flop) {
  dot2_async(x, y, size, innerFidx, GUIDE, &d_res->fdot);
  return dot_read(flop);
}

// the partial sums of the dot product just launched: all-reduced, read back, rounded
REAL_TYPE CZ::dot_read(double& flop) {
  flop += 2.0 * npts();
  if (!Comm_SUM_dev(&d_res->fdot, 1)) exit(0);
  return (REAL_TYPE)*fetch(&d_res->fdot);
}

// The work vectors the preconditioner solves into are allocated zero-filled and afterwards only written on the inner box,
// so their guide cells and faces are zero for the whole run.
bool CZ::xx_shell_is_zero(const REAL_TYPE* xx) const { return xx == pcg_p_ || xx == pcg_s_ || (xx != nullptr && xx == cg_z); }

// cz_Poisson.cpp:273-322
// May PBiCGSTAB withhold `p = r + beta (p - omega q)` and `s = r - alpha q` and let the first pair of the preconditioner solve that follows
// make them (jacobi2p_k<BS>)?  Plain Jacobi or red-black SOR preconditioner on the whole-box fused pass with the literal zero start, one rank (a decomposed
// solve reads the right-hand side in its ghost layer, where the operands are not valid), and the launcher takes it.  CZ_BICG_FUSE=0: never.
bool CZ::bicg_fusable(int pc_type) {
  if (!cfg.on(CZV_BICG_FUSE, true)) return false;
  if ((pc_type != LS_JACOBI && pc_type != LS_SOR2SMA) || numProc != 1 || czhip_use_t2() == 0) return false;
  const bool rb = pc_type == LS_SOR2SMA;
  const PassPlan plan = plan_pass(pcg_p_, pcg_p, pc_type, 8, false, true, rb, true);
  if (!(plan.kind == PassPlan::WHOLE && plan.zero_start)) return false;
  return czhip_jacobi2_from_zero_made_async(pcg_p_, WRK, pcg_s, 2, pcg_r, pcg_q, pcg_p, (REAL_TYPE)0, (REAL_TYPE)0, size, innerFidx, idx1, GUIDE, cf, ac1,
                                            rb ? 0 : -1, d_res->pass, 1) != 0;
}

void CZ::Preconditioner(REAL_TYPE* xx, REAL_TYPE* bb, double& flop, int s_type, const BMade* made) {
  double res = 0.0;
  const int lc_max = 8;  // :280
  const size_t nbytes = padded_cells() * sizeof(REAL_TYPE);
  // blas_clear_(xx) of the caller (cz_Poisson.cpp:405, 441) is folded in here.  With the plain Jacobi preconditioner on
  // the fused-pair path the clear is not even executed: xx's guide cells / faces are zero from allocation on (sweeps only
  // ever write its inner box) and the first pair takes "u == 0" as a literal instead of reading it.
  // (single-domain only: a decomposed run leaves the neighbours' values in xx's ghost layers)
  const bool zero_start = (s_type == LS_JACOBI || s_type == LS_SOR2SMA) && numProc == 1 && czhip_use_t2() != 0 && xx_shell_is_zero(xx);
  if (!zero_start) HIP_CHECK(hipMemsetAsync(xx, 0, nbytes, stream()));
  struct Scope {
    bool& f;
    explicit Scope(bool& x) : f(x) { f = true; }
    ~Scope() { f = false; }
  } scope(in_precond);
  // (a name without a loop here -- none, and pcr_j_esa as in the reference, cz_Poisson.cpp:282-321 -- is a copy)
  if (cz_solvers::row(s_type).precond_runs) run(s_type, res, xx, bb, lc_max, flop, false, zero_start, made);
  else HIP_CHECK(hipMemcpyAsync(xx, bb, nbytes, hipMemcpyDeviceToDevice, stream()));  // blas_copy_
}

// cz_Poisson.cpp:332-504
int CZ::PBiCGSTAB(double& res, REAL_TYPE* X, REAL_TYPE* B, double& flop, int s_type) {
  const bool maf = cz_solvers::row(s_type).maf;
  const int gc = GUIDE;
  hipStream_t st = stream();
  const size_t nbytes = padded_cells() * sizeof(REAL_TYPE);
  int itr;
  double flop_count = 0.0;
  res = 0.0;

  HIP_CHECK(hipMemsetAsync(pcg_q, 0, nbytes, st));                       // :344 blas_clear_
  if (maf) calc_rk_maf_async(pcg_r, X, B, size, innerFidx, gc, d_xc, d_yc, d_zc, pvt);  // :352
  else calc_rk_async(pcg_r, X, B, size, innerFidx, gc, cf);                             // :356
  flop += (maf ? 63.0 : 14.0) * npts();
  if (!Comm_S(pcg_r)) return 0;                                         // :362
  HIP_CHECK(hipMemcpyAsync(pcg_r0, pcg_r, nbytes, hipMemcpyDeviceToDevice, st));  // :365 blas_copy_

  REAL_TYPE rho_old = 1.0, alpha = 0.0, omega = 1.0, r_omega = -omega;  // :368-371

  // Dot products that directly follow the kernel producing their operand are folded into that kernel (same per-point
  // REAL products, double accumulation, rounded once to REAL like Fdot1/Fdot2): q.r0 into q = A p_, t_.s and t_.t_ into
  // t_ = A s_, r.r and the NEXT iteration's rho = r.r0 into r = s - omega t_.
  MafPtrs mp{d_xc, d_yc, d_zc, pvt};
  auto fetch2 = [&](double* d_two, REAL_TYPE& a, REAL_TYPE& b2) -> bool {  // all-reduce + D2H of two device doubles
    if (!Comm_SUM_dev(d_two, 2)) return false;
    const double* const two = fetch(d_two, 2);
    a = (REAL_TYPE)two[0], b2 = (REAL_TYPE)two[1];
    return true;
  };
  REAL_TYPE rho_next = 0.0;
  // The two vector updates that make the right-hand side of a preconditioner solve (:398, :434) are folded into the first pair of that solve
  // where it is the whole-box fused pass from a literal zero: one launch and one read of an array less per solve.
  const bool fuse = !maf && bicg_fusable(pc_type);
  bicg_fused = 0;
  // alpha / omega on the device between their dot products and their users (bicg_scalar_async): d_res->sc holds alpha, omega, -alpha, -omega
  // as REALs (ScBicg).  CZ_BICG_DEVSC=0: the host computes them from read-back dot products as in rounds 1-2 (and as the reference does).
  REAL_TYPE* const d_bs = d_res->sc;
  CzScalars::Bicg* const dots = &d_res->bicg;  // q.r0, t.s / t.t, r.r / r.r0
  const bool devsc = cfg.on(CZV_BICG_DEVSC, true);
  bool pc_copy = !cz_solvers::row(pc_type).precond_runs;  // Preconditioner() would copy (cz_Poisson.cpp:318-320)
  if (!cfg.on(CZV_BICG_ALIAS, true)) pc_copy = false;  // (the copy is made: A/B and the bit-equality test)

  for (itr = 1; itr < ItrMax; itr++) {  // :373
    REAL_TYPE rho;
    if (itr == 1) {
      flop_count = 0.0;
      rho = Fdot2(pcg_r, pcg_r0, flop_count);  // :376
      flop += flop_count;
    } else {
      rho = rho_next;  // r.r0 was accumulated while r was written (below)
      flop += 2.0 * npts();
    }
    if (fabs(rho) < FLT_MIN) {  // :379-383
      itr = 0;
      break;
    }
    BMade made_p{0, nullptr, nullptr, nullptr, (REAL_TYPE)0, (REAL_TYPE)0, nullptr};
    if (itr == 1) {
      HIP_CHECK(hipMemcpyAsync(pcg_p, pcg_r, nbytes, hipMemcpyDeviceToDevice, st));  // :387
    } else {
      REAL_TYPE beta = rho / rho_old * alpha / omega;  // :394
      if (fuse) {
        // :398 withheld: the first pair of the solve below makes p = r + beta (p - omega q) on its way and writes it to the array of s
        // (dead until :434), which then IS p -- the pass cannot update p in place: neighbouring workgroups read each other's rows
        made_p = BMade{2, pcg_r, pcg_q, pcg_p, beta, omega, nullptr};
        std::swap(pcg_p, pcg_s);
        bicg_fused++;
      } else {
        bicg1_async(pcg_p, pcg_r, pcg_q, beta, omega, size, innerFidx, gc);  // :398
      }
      flop += 4.0 * npts();
    }
    if (!Comm_S(pcg_p)) return 0;                    // :402
    flop_count = 0.0;                                // :405 blas_clear_(pcg_p_) happens inside Preconditioner
    // "no preconditioner" is a copy in the reference (:318-320 blas_copy_ after :405 blas_clear_): p_ IS p then -- nothing writes p before
    // the last reader of p_ (:470) is through -- and three passes over an array per solve are not made (6.0 -> 4.7 ms per iteration at 512^3 FP64)
    REAL_TYPE* const p_ = pc_copy ? pcg_p : pcg_p_;
    if (!pc_copy) Preconditioner(pcg_p_, pcg_p, flop_count, pc_type, made_p.op ? &made_p : nullptr);  // :409
    flop += flop_count;
    if (line_error) return 0;

    // :417/:421 q = A p_  and  :427 q.r0
    calc_ax_dots_async(pcg_q, p_, pcg_r0, size, innerFidx, gc, cf, maf ? &mp : nullptr, dots->q_r0);
    flop += (maf ? 63.0 : 13.0) * npts() + 2.0 * npts();
    REAL_TYPE r_alpha = (REAL_TYPE)0;
    if (devsc) {
      // alpha = rho / (q . r0) (:427) is made on the device and read there by the launches that need it; the host reads it back with omega and
      // the residual at the end of the iteration (one wait instead of three: 2 x 25-35 us of idle GPU per iteration, a fifth of an iteration at 128^3)
      if (!Comm_SUM_dev(dots->q_r0, 2)) return 0;
      bicg_scalar_async(1, dots->q_r0, rho, d_bs);
    } else {
      REAL_TYPE q_r0, q_q;
      if (!fetch2(dots->q_r0, q_r0, q_q)) return 0;
      alpha = rho / q_r0;  // :427
      r_alpha = -alpha;
    }
    BMade made_s{1, pcg_q, pcg_r, nullptr, r_alpha, (REAL_TYPE)0, devsc ? d_bs + SC_B_NALPHA : nullptr};
    if (fuse) bicg_fused++;  // :434 withheld likewise: s = r - alpha q
    else triad_async(pcg_s, pcg_q, pcg_r, r_alpha, size, innerFidx, gc, devsc ? d_bs + SC_B_NALPHA : nullptr);  // :434
    flop += 2.0 * npts();
    if (!Comm_S(pcg_s)) return 0;  // :438

    flop_count = 0.0;  // :441 blas_clear_(pcg_s_) happens inside Preconditioner
    REAL_TYPE* const s_ = pc_copy ? pcg_s : pcg_s_;
    if (!pc_copy) Preconditioner(pcg_s_, pcg_s, flop_count, pc_type, fuse ? &made_s : nullptr);  // :445
    flop += flop_count;
    if (line_error) return 0;

    // :453/:457 t_ = A s_  and  :464 t_.s, t_.t_
    calc_ax_dots_async(pcg_t_, s_, pcg_s, size, innerFidx, gc, cf, maf ? &mp : nullptr, dots->t_s);
    flop += (maf ? 63.0 : 13.0) * npts() + 4.0 * npts();
    if (devsc) {
      if (!Comm_SUM_dev(dots->t_s, 2)) return 0;
      bicg_scalar_async(2, dots->t_s, (REAL_TYPE)0, d_bs);  // omega = (t . s) / (t . t)  :464
    } else {
      REAL_TYPE ts, tt;
      if (!fetch2(dots->t_s, ts, tt)) return 0;
      omega = ts / tt;  // :464
      r_omega = -omega;
    }

    bicg2_async(X, p_, s_, alpha, omega, size, innerFidx, gc, devsc ? d_bs + SC_B_ALPHA : nullptr, devsc ? d_bs + SC_B_OMEGA : nullptr);  // :470
    flop += 4.0 * npts();
    // :476 r = s - omega t_  with  :481 res = r.r  and the next :376 rho = r.r0
    triad_dots_async(pcg_r, pcg_t_, pcg_s, pcg_r0, r_omega, size, innerFidx, gc, dots->r_r, devsc ? d_bs + SC_B_NOMEGA : nullptr);
    flop += 2.0 * npts() + 2.0 * npts();
    REAL_TYPE rr;
    if (devsc) {  // the one wait of the iteration: r.r, r.r0 and the two scalars the next beta needs
      if (!Comm_SUM_dev(dots->r_r, 2)) return 0;
      const double* const two = fetch_queued(dots->r_r, 2);
      const REAL_TYPE* const hs = fetch(d_bs, 2);  // (alpha and omega are neighbours: SC_B_ALPHA, SC_B_OMEGA)
      rr = (REAL_TYPE)two[0], rho_next = (REAL_TYPE)two[1];
      alpha = hs[SC_B_ALPHA], omega = hs[SC_B_OMEGA];
      r_omega = -omega;
    } else if (!fetch2(dots->r_r, rr, rho_next)) {
      return 0;
    }
    res = rr;

    if (!Comm_S(X)) return 0;  // :486
    // :488 all-reduces `res` a second time although Fdot1 already did (an MPI-only double count in the reference,
    // a no-op in its serial build); dropped here.
    res *= res_normal;  // :490
    res = sqrt(res);
    history.push_back(res);  // :492
    // :495 bc_k_(X): identity, X's faces are never written (see file header)
    if (res < eps) break;  // :498
    rho_old = rho;
  }
  return itr;
}

// Preconditioned conjugate gradient (beyond the reference; DESIGN.md "PCG").  The operator is symmetric and definite, and M^-1 is either the
// identity (z IS r: no copy) or the 8 relaxed Jacobi sweeps from zero of PBiCGSTAB's preconditioner -- a polynomial in A, hence symmetric.
//   r = b - A x;  for itr = 1 .. ItrMax:  z = M^-1 r;  rho = r.z;  p = z (itr 1) | z + beta p, beta = rho / rho_old;  q = A p;
//   alpha = rho / p.q;  x = alpha p + x;  r = (-alpha) q + r;  res = sqrt(r.r * res_normal)
// Every scalar is made on the device (cg_scal_k) from REAL-rounded double sums, so the host waits once per iteration, for r.r and rho.
// Breakdown (cg_breakdown): |rho| < FLT_MIN (absolute, in both precisions) ends the solve with itr = 0 BEFORE the iteration's update of x and
// r.  none: the host holds rho before the first launch.  jacobi | mg | mgrb: the host reads rho at the iteration's one wait, after the update
// pass was launched, so that pass carries the test itself (cg_update_guarded_async: it stores nothing under the threshold); the unfused
// update (CZ_CG_FUSE=0) waits for rho before its triads instead.
// The steps below are the lines of that algorithm, each with its operation count beside its launches; CgMode (cz_driver.h): the modes, decided once
// The operator in constant or face-coefficient form: out = A p with p.out, out.out in dots[0], dots[1] (b null), or out = b - A p (the
// coefficient form leaves two sums in dots that nobody reads; the constant form none).  false: the launch was refused
bool CZ::cg_apply_A(REAL_TYPE* out, REAL_TYPE* p, const REAL_TYPE* b, double* dots) {
  if (coef_on()) return coef_ax_async(b ? 1 : 0, out, p, b, coef_b[0], coef_b[1], coef_b[2], size, innerFidx, GUIDE, dots) != 0;
  if (b) calc_rk_async(out, p, b, size, innerFidx, GUIDE, cf);
  else calc_ax_dots_async(out, p, p, size, innerFidx, GUIDE, cf, nullptr, dots);
  return true;
}

// true: the solve ends with itr = 0; pcg_void_start (cz_info 24): the breakdown came at iteration 1 -- x is the caller's
bool CZ::cg_breakdown(REAL_TYPE rho, int itr) {
  if (!(fabs(rho) < FLT_MIN)) return false;
  pcg_void_start = itr == 1;
  return true;
}

// Start: r = b - A x (14 per cell, 23 with coefficients); the closed box's step 1 (4 per cell): the initial residual into the range of the
// operator -- the pass that writes r' returns sum r' (the first lagged mean) and sum r'^2; none: the one r.r that no update made -> rho
bool CZ::cg_start(const CgMode& m, REAL_TYPE* X, const REAL_TYPE* B, REAL_TYPE& rho, double& flop) {
  const double n = npts();
  REAL_TYPE* const sc = d_res->sc;
  mirror(X);
  if (!cg_apply_A(cg_r, X, B, d_res->cg_r0)) return false;
  flop += (m.coef ? 23.0 : 14.0) * n;
  if (m.closed) {
    if (!project(cg_r, sc + SC_LAG_MEAN, &d_res->closed_mean[0]) || !Comm_SUM_dev(d_res->project, 2)) return false;
    mean_scalar_async(d_res->project, g_npts, sc + SC_LAG_MEAN, nullptr);
    flop += 4.0 * n;
  }
  if (!Comm_S(cg_r)) return false;
  if (m.pc) return true;
  if (m.closed) {
    HIP_CHECK(hipMemcpyAsync(&d_res->cg.rr, &d_res->project[1], sizeof(double), hipMemcpyDeviceToDevice, stream()));
  } else {
    dot1_async(cg_r, size, innerFidx, GUIDE, &d_res->cg.rr);
    flop += 2.0 * n;
    if (!Comm_SUM_dev(&d_res->cg.rr, 1)) return false;
  }
  rho = (REAL_TYPE)*fetch(&d_res->cg.rr);
  return true;
}

// z = M^-1 rin, or with the scaling either side z = s M^-1 (s r) (1 per cell each): the single-domain cycle, the distributed cycle, under
// a mask the 8 relaxed sweeps from zero as single sweeps (8 x 18 per cell), or Preconditioner's 8 sweeps (its own count)
bool CZ::cg_apply_M(const CgMode& m, double& flop) {
  const double n = npts();
  REAL_TYPE* const rin = m.scale ? cg_q : cg_r;  // what M^-1 is applied to
  if (m.scale) {
    coef_scale_async(cg_q, cg_r, coef_s, size, GUIDE);
    flop += n;
  }
  if (mg || mgd) {
    if (mg ? !czhip_mg_apply_async(mg, cg_z, rin, ac1) : !mgd_apply(mgd, cg_z, rin, ac1)) return false;  // z = V_0(r)
    mg_cycles++;
  } else if (bc.any()) {
    // between cg_z and cg_p[1] (free: the direction is not fused), the exchange and the mirror before every sweep that reads its input
    HIP_CHECK(hipMemsetAsync(cg_z, 0, padded_cells() * sizeof(REAL_TYPE), stream()));
    REAL_TYPE *src = cg_z, *dst = cg_p[1];
    for (int s = 0; s < 8; s++) {
      if (s) {
        if (!Comm_S(src)) return false;
        mirror(src);
      }
      czhip_jacobi_async(src, dst, rin, size, innerFidx, GUIDE, cf, ac1, d_res->pass, 0, nullptr);
      std::swap(src, dst);
    }
    flop += 8 * 18.0 * n;
  } else {
    double fc = 0.0;
    Preconditioner(cg_z, rin, fc, LS_JACOBI);
    flop += fc;
  }
  if (m.scale) {
    coef_scale_async(cg_z, cg_z, coef_s, size, GUIDE);
    flop += n;
  }
  return true;
}

// Precondition: z = M^-1 r, then rho = r.z (2 per cell)
bool CZ::cg_precondition(const CgMode& m, double& flop) {
  if (!Comm_S(cg_r) || !cg_apply_M(m, flop)) return false;  // (the exchange: a decomposed pass reads the right-hand side in its ghost layer)
  dot2_async(cg_r, cg_z, size, innerFidx, GUIDE, m.d_rho);
  flop += 2.0 * npts();
  return Comm_SUM_dev(m.d_rho, 1);
}

// Direction and SpMV: rho and beta = rho / rho_old on the device; p = z (iteration 1) | beta p + z (2 per cell) and q = A p with p.q (13 + 2
// per cell, 22 + 2 with coefficients) in the fused pass, or as copy / triad, exchange, mirror, operator; then alpha = rho / p.q.  cg_p[cur] is p
bool CZ::cg_direction(const CgMode& m, int itr, int& cur, double& flop) {
  const double n = npts();
  REAL_TYPE* const sc = d_res->sc;
  cg_scalar_async(0, m.d_rho, itr == 1, sc);
  if (m.fuse_dir) {
    czhip_cg_dir_ax_async(cg_p[cur ^ 1], cg_q, m.z, cg_p[cur], itr == 1 ? nullptr : sc + SC_BETA, size, innerFidx, GUIDE, cf, &d_res->cg.pq);
    cur ^= 1;
    cg_fused++;
  } else {
    if (itr == 1) HIP_CHECK(hipMemcpyAsync(cg_p[cur], m.z, padded_cells() * sizeof(REAL_TYPE), hipMemcpyDeviceToDevice, stream()));
    else triad_async(cg_p[cur], cg_p[cur], m.z, (REAL_TYPE)0, size, innerFidx, GUIDE, sc + SC_BETA);
    if (!Comm_S(cg_p[cur])) return false;
    mirror(cg_p[cur]);
    if (!cg_apply_A(cg_q, cg_p[cur], nullptr, &d_res->cg.pq)) return false;  // (the unfused SpMV writes q.q to cg.qq)
  }
  if (itr > 1) flop += 2.0 * n;
  flop += (m.coef ? 22.0 : 13.0) * n + 2.0 * n;
  if (!Comm_SUM_dev(&d_res->cg.pq, 1)) return false;
  cg_scalar_async(1, &d_res->cg.pq, 0, sc);
  return true;
}

// Update: x = alpha p + x, r = (-alpha) q + r, r.r (6 per cell).  Closed: r = ((-alpha) q + r) - the lagged mean, sum r^2 and sum r side by
// side: one all-reduce, then the mean the next update removes.  Fused: one guarded pass.  Unfused: the triads carry no test of their
// own, so the host learns rho before them.  1: launched, 0: failed, -1: breakdown (nothing updated)
int CZ::cg_update(const CgMode& m, REAL_TYPE* X, const REAL_TYPE* p, int itr, double& flop) {
  REAL_TYPE* const sc = d_res->sc;
  double* const d_rr = &d_res->cg.rr;
  if (m.closed || m.fuse) {
    cg_update_guarded_async(m.closed, X, cg_r, p, cg_q, sc, size, innerFidx, GUIDE, d_rr);
  } else {
    if (m.pc && cg_breakdown((REAL_TYPE)*fetch(m.d_rho), itr)) return -1;
    triad_async(X, p, X, (REAL_TYPE)0, size, innerFidx, GUIDE, sc + SC_ALPHA);
    triad_async(cg_r, cg_q, cg_r, (REAL_TYPE)0, size, innerFidx, GUIDE, sc + SC_NALPHA);
    dot1_async(cg_r, size, innerFidx, GUIDE, d_rr);
  }
  flop += 6.0 * npts();
  if (!Comm_SUM_dev(d_rr, m.closed ? 2 : 1)) return 0;
  if (m.closed) mean_scalar_async(&d_res->cg.rsum, g_npts, sc + SC_LAG_MEAN, nullptr);
  return 1;
}

// End: the closed box's step 3 (3 per cell), the answer of zero mean (the sums read owned cells only; the exchange carries the shifted
// values into the ghost layers) and the two means for cz_closed_mean; the ghost layers of the result, as PBiCGSTAB leaves them
bool CZ::cg_end(const CgMode& m, REAL_TYPE* X, double& flop) {
  if (m.closed) {
    if (!project(X, &d_res->closed_mean[1], nullptr)) return false;
    flop += 3.0 * npts();
    const REAL_TYPE* const hm = fetch(d_res->closed_mean, 2);
    closed_m[1] = (double)hm[0], closed_m[2] = (double)hm[1];
  }
  if (!Comm_S(X)) return false;
  mirror(X);
  return true;
}

int CZ::PCG(double& res, REAL_TYPE* X, REAL_TYPE* B, double& flop) {
  CgMode m;
  m.pc = pc_type == LS_JACOBI || pc_type == LS_MG || pc_type == LS_MGRB;
  m.fuse = cfg.on(CZV_CG_FUSE, true);
  m.coef = coef_on();
  m.scale = m.coef && !coef_mg_on();
  m.fuse_dir = m.fuse && numProc == 1 && !bc.any() && !m.coef;
  m.closed = closed_box != 0;
  m.z = m.pc ? cg_z : cg_r;
  m.d_rho = m.pc ? &d_res->cg.rho : &d_res->cg.rr;
  res = 0.0;
  cg_fused = mg_cycles = pcg_void_start = 0;
  REAL_TYPE rho = (REAL_TYPE)0;
  if (!cg_start(m, X, B, rho, flop)) return 0;
  int cur = 0;  // cg_p[cur] is p
  int itr;
  for (itr = 1; itr <= ItrMax; itr++) {
    if (!m.pc && cg_breakdown(rho, itr)) {  // (none: the host holds rho before the first launch; as PBiCGSTAB)
      itr = 0;
      break;
    }
    if (m.pc && !cg_precondition(m, flop)) return 0;
    if (!cg_direction(m, itr, cur, flop)) return 0;
    const int updated = cg_update(m, X, cg_p[cur], itr, flop);
    if (updated == 0) return 0;
    // the one wait of the iteration: r.r (and this iteration's rho), one copy of the four dots
    if (updated > 0) fetch(&d_res->cg.rho, 4);
    // (pc: found after the iteration's launches, whose update pass stored nothing: x is that of the iteration before)
    if (updated < 0 || (m.pc && cg_breakdown((REAL_TYPE)h_scal->cg.rho, itr))) {
      itr = 0;
      break;
    }
    const REAL_TYPE rr = (REAL_TYPE)h_scal->cg.rr;
    res = sqrt((double)rr * res_normal);
    history.push_back(res);
    if (res < eps) break;
    rho = m.pc ? (REAL_TYPE)h_scal->cg.rho : rr;
  }
  if (itr > ItrMax) itr = ItrMax;
  return cg_end(m, X, flop) ? itr : 0;
}

// ------------------------------------------------------------------------------------------------------------
// Zero-flux (Neumann) faces.  The mask is global and the same on every rank; a brick mirrors the faces that are physical on it
// Periodic directions are never cut, so both their faces are physical on every brick: there the one fill launch wraps, and
// mirrors the Neumann faces of the other directions with it
void CZ::mirror(REAL_TYPE* X) {
  const int gn[3] = {G_size[0] - 2, G_size[1] - 2, G_size[2] - 2};
  if (!fill_bc_async(X, size, innerFidx, GUIDE, mg_level_bc(bc, gn), true)) cz_fatal(1, "czhip: the fill of the periodic and Neumann faces was refused\n");
}

// The one rule of solvability, for the three setters on the combined state: with the closed mode off, some face of a direction that is not
// periodic must be a Dirichlet face (else the operator is singular).  nullptr: solvable; else the line
const char* CZ::unsolvable(CzBc next, int closed) {
  if (closed) return nullptr;
  for (int d = 0; d < 3; d++)
    if (!((next.per >> d) & 1) && ((next.nm >> (2 * d)) & 3) != 3) return nullptr;
  if (!next.per) return "at least one face must stay a Dirichlet face (the all-Neumann problem is singular: cz_set_closed_box keeps it solvable)";
  return "no Dirichlet face is left in a direction that is not periodic (the problem is singular: cz_set_closed_box keeps it solvable)";
}

const char* CZ::bc_unready(const void* arg) const {
  if (!set_up) return "no problem is set up (cz_setup first)";
  if (!arg) return "NULL pointer";
  if (SW_maf) return "the handle's operator is a MAF one, not the unit-coefficient operator";
  return nullptr;
}
static int bc_refuse(const char* who, const char* why) {
  fprintf(stderr, "%s: %s\n", who, why);
  return 0;
}

// The next state of the handle, from any of the three setters (`who`, after bc_unready and its own checks): refused with one line and nothing
// changed, or taken by the hierarchy and the driver.  closed: the closed mode from now on; project: cz_set_closed_box(1) alone projects the
// right-hand side here, inside the one synchronisation
int CZ::set_bc(CzBc next, int closed, bool project, const char* who) {
  if (const char* why = unsolvable(next, closed)) return bc_refuse(who, why);
  // face coefficients: the alias faces and the scaling follow the periodic directions; a face that was ignored and is read now may be bad
  // (before the hierarchy takes the state: where it holds the coefficients, cz_set_coef_mg, it rebuilds from the new alias faces)
  if (coef_on() && next.per != coef_per && !coef_prepare(next.per))
    fprintf(stderr, "%s: a face coefficient that the new state reads is not finite and positive: the handle is left without coefficients\n", who);
  if (mg) mg_set_bc(mg, next);
  if (mgd) mgd_set_bc(mgd, next);
  const bool coef_mg_ok = coef_mg_settle(who, true);
  bc = next;
  closed_box = closed;
  // the work vectors whose face layers carried the wraps and mirrors of the state before: zeros again, as the unmasked passes read them
  for (REAL_TYPE* a : {cg_z, cg_p[0], cg_p[1]})
    if (a) HIP_CHECK(hipMemsetAsync(a, 0, padded_cells() * sizeof(REAL_TYPE), stream()));
  if (project && !project_rhs()) return 0;
  mirror(P);
  wrk_shell_tag = 0;
  czhip_sync();
  return coef_mg_ok ? 1 : 0;  // (0: the state is taken, the coefficient hierarchy is not -- its line is printed)
}

// The coefficient hierarchy (cz_set_coef_mg) after a call of `who` made or changed the state it is built under: attached to
// the hierarchy while the flag is on, coefficients are in force and the preconditioner is mg or mgrb on one domain, detached otherwise.
// rebuilt: the hierarchy has just rebuilt what it held (mg_set_bc).  false: a coarse weight or diagonal is not finite and positive -- one
// line, the flag off, the scaled preconditioner from now on
bool CZ::coef_mg_settle(const char* who, bool rebuilt) {
  if (!mg) return true;
  const bool want = coef_mg && coef_on();
  bool ok = true;
  if (mg->coef_bad) ok = false, mg->coef_bad = 0;  // (mg_set_bc's rebuild: the hierarchy is the constant one already)
  else if (want && !(mg->coef && rebuilt)) ok = czhip_mg_set_coef(mg, coef_b[0], coef_b[1], coef_b[2]) == 1;
  else if (!want && mg->coef) czhip_mg_set_coef(mg, nullptr, nullptr, nullptr);
  if (!ok) {
    fprintf(stderr, "%s: a coarse weight of the coefficient hierarchy is not finite and positive: cz_set_coef_mg is off, the scaled preconditioner runs\n", who);
    coef_mg = 0;
  }
  // the line iterations of cz_set_mg_lines follow: the hierarchy holds the flag (and its scratch) while the flag is on
  // and the smoother is mgrb; its cycles take it while they take the coefficients, so a dropped hierarchy leaves the lines idle
  if (pc_type == LS_MGRB && czhip_mg_set_lines(mg, mg_lines) != 1) cz_fatal(1, "%s: the hierarchy refused the line iterations\n", who);
  return ok;
}

int CZ::SetMgLines(int on) {
  const char* const who = "cz_set_mg_lines";
  auto refuse = [&](const char* why) { return bc_refuse(who, why); };
  if (const char* why = bc_unready(this)) return refuse(why);  // (no set-up, a MAF operator)
  if (numProc > 1) return refuse("a decomposed run: the coefficient hierarchy that the lines run under is refused there (single domain only)");
  if ((on | 1) != 1) return refuse("the flag is 0 or 1");
  if (on && !(ac1 <= (REAL_TYPE)1))
    return refuse("the handle's coefficient exceeds 1: line iterations take 0 < coef <= 1 (over-relaxed, the lagged wrap of a periodic Z makes the preconditioner indefinite)");
  mg_lines = on;
  coef_mg_settle(who, true);  // (the coefficient hierarchy stands as it is: only the flag travels)
  czhip_sync();
  return 1;
}

int CZ::SetCoefMg(int on) {
  const char* const who = "cz_set_coef_mg";
  auto refuse = [&](const char* why) { return bc_refuse(who, why); };
  if (const char* why = bc_unready(this)) return refuse(why);  // (no set-up, a MAF operator)
  if (numProc > 1) return refuse("a decomposed run: the face coefficients themselves are refused there (single domain only)");
  coef_mg = on ? 1 : 0;
  const bool ok = coef_mg_settle(who, false);
  czhip_sync();
  return ok ? 1 : 0;
}

int CZ::SetPeriodic(const int* dirs) {
  const char* const who = "cz_set_periodic";
  const char* why = bc_unready(dirs);
  for (int d = 0; !why && d < 3; d++) {
    if (dirs[d] && G_size[d] < 4) why = "a periodic direction needs two inner points at least";
    else if (dirs[d] && G_div[d] > 1) why = "a periodic direction must not be cut by the decomposition";
  }
  return why ? bc_refuse(who, why) : set_bc(bc.with_dirs(dirs), closed_box, false, who);
}

int CZ::SetNeumann(const int* faces) {
  const char* const who = "cz_set_neumann";
  const char* const why = bc_unready(faces);
  return why ? bc_refuse(who, why) : set_bc(bc.with_faces(faces), 0, false, who);
}

// The closed box: all six faces zero-flux, the right-hand side kept compatible, pcg's residual kept in the range of the
// operator and its answer of zero mean.  on = 0: the Dirichlet problem again (the right-hand side stays projected)
int CZ::SetClosedBox(int on) {
  const char* const who = "cz_set_closed_box";
  const char* const why = bc_unready(this);
  return why ? bc_refuse(who, why) : set_bc(CzBc(on ? 63 : 0, bc.per), on ? 1 : 0, on != 0, who);
}

// A <- A - m over the inner box, m = (REAL)(sum A / npts) over the GLOBAL inner box: a pass that sums, one all-reduce, the mean on the device
// (*m_dev, *keep_dev), a pass that subtracts and leaves this rank's sum A' and sum A'^2 in d_res->project (the caller all-reduces what it uses)
bool CZ::project(REAL_TYPE* A, REAL_TYPE* m_dev, REAL_TYPE* keep_dev) {
  double* const d_cl = d_res->project;
  if (!czhip_shift_sums_async(A, nullptr, size, innerFidx, GUIDE, d_cl) || !Comm_SUM_dev(d_cl, 1)) return false;
  mean_scalar_async(d_cl, g_npts, m_dev, keep_dev);
  return czhip_shift_sums_async(A, m_dev, size, innerFidx, GUIDE, d_cl) != 0;
}

// (no host wait here: cz_set_rhs from a device array stays an event hand-over; the mean stays in d_res->rhs_mean until cz_closed_mean asks for it)
bool CZ::project_rhs() {
  if (!project(RHS, &d_res->rhs_mean, nullptr) || !Comm_S2(RHS)) return false;
  closed_m0_on_device = true;
  return true;
}

double CZ::ClosedMean(int which) {
  if (which < 0 || which > 2) return std::nan("");
  if (which == 0 && closed_m0_on_device) {
    closed_m[0] = (double)*fetch(&d_res->rhs_mean);
    closed_m0_on_device = false;
  }
  return closed_m[which];
}

void CZ::Field(REAL_TYPE* host) const {
  czhip_d2h(host, P, padded_cells() * sizeof(REAL_TYPE));
}

// What FieldIO and ProjectIO share.  field_check: NULL, alignment, strides; *span = the elements the strides cover.  nullptr, or the refusal's line
const char* CZ::field_check(const void* a, int abytes, const long long* stride, long long* span) const {
  if (!a || !stride) return "NULL pointer";
  if (reinterpret_cast<uintptr_t>(a) & (uintptr_t)(abytes - 1)) return "the array is not aligned to its element size";
  for (int d = 0; d < 3; d++)
    if (stride[d] < 1) return "strides must be positive (elements)";
  *span = 1;
  for (int d = 0; d < 3; d++) *span += (long long)(size[d] - 1) * stride[d];
  return nullptr;
}
// two cells of a destination must not share an element.  Accepted: ordered by stride, every stride is at least the span of the
// directions below it (dense arrays in any order of the directions, and slices of them); directions of one cell do not count
const char* CZ::field_distinct(const long long* stride) const {
  int o[3] = {0, 1, 2};
  std::sort(o, o + 3, [&](int x, int y) { return stride[x] < stride[y]; });
  long long below = 1;  // span of the directions already passed
  for (int n = 0; n < 3; n++) {
    const int d = o[n];
    if (size[d] == 1) continue;
    if (stride[d] < below) return "two cells of the destination share an element under these strides";
    below += (long long)(size[d] - 1) * stride[d];
  }
  return nullptr;
}
const char* CZ::field_on_device(const void* a) const {
  hipPointerAttribute_t at;
  int cur = -1;
  HIP_CHECK(hipGetDevice(&cur));
  if (hipPointerGetAttributes(&at, a) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != cur) {
    (void)hipGetLastError();
    return "not a pointer to memory of the handle's device";
  }
  return nullptr;
}
// the compute stream waits for what the caller's stream holds (NULL: nothing to wait for)
void CZ::field_wait_for(void* user_stream) {
  if (!user_stream) return;
  if (!ev_io) HIP_CHECK(hipEventCreateWithFlags(&ev_io, hipEventDisableTiming));
  HIP_CHECK(hipEventRecord(ev_io, (hipStream_t)user_stream));
  HIP_CHECK(hipStreamWaitEvent(stream(), ev_io, 0));
}
// the caller's stream waits for the compute stream; NULL, or host_waits (a host value is due on return): the host waits for the compute stream
void CZ::field_hand_back(void* user_stream, bool host_waits) {
  if (user_stream) {
    HIP_CHECK(hipEventRecord(ev_io, stream()));
    HIP_CHECK(hipStreamWaitEvent((hipStream_t)user_stream, ev_io, 0));
  }
  if (!user_stream || host_waits) HIP_CHECK(hipStreamSynchronize(stream()));
}
// the device buffer host arrays go through, of `bytes` at least
void* CZ::field_stage(size_t bytes) {
  if (bytes > io_stage_cap) {
    if (io_stage) {
      HIP_CHECK(hipStreamSynchronize(stream()));
      HIP_CHECK(hipFree(io_stage));
    }
    HIP_CHECK(hipMalloc(&io_stage, bytes));
    io_stage_cap = bytes;
  }
  return io_stage;
}
// the brick's cells and nothing else from a copy `tmp` of the span into the caller's array, the direction of the smallest stride innermost
void CZ::field_copy_cells(void* a, const void* tmp, int abytes, const long long* stride) const {
  int o[3] = {0, 1, 2};
  std::sort(o, o + 3, [&](int x, int y) { return stride[x] > stride[y]; });
  const long long s0 = stride[o[0]], s1 = stride[o[1]], s2 = stride[o[2]];
  unsigned char* out = static_cast<unsigned char*>(a);
  const unsigned char* in = static_cast<const unsigned char*>(tmp);
  for (int x = 0; x < size[o[0]]; x++)
    for (int y = 0; y < size[o[1]]; y++) {
      const long long base = x * s0 + y * s1;
      for (int z = 0; z < size[o[2]]; z++) memcpy(out + (size_t)(base + z * s2) * abytes, in + (size_t)(base + z * s2) * abytes, (size_t)abytes);
    }
}

// The caller's problem: import into RHS / P, export of P (cz_set_rhs, cz_set_field, cz_get_field), and the two operations of
// mixed-precision refinement, the residual of P out and a correction into P (cz_get_residual, cz_add_field), whose caller's
// side holds float or double (abytes).  Device arrays are handed
// over by events (the compute stream waits for what the caller's stream holds, the kernel runs, the caller's stream waits for the kernel): no
// device-wide wait.  user_stream NULL: nothing to wait for before, the host waits for the compute stream after.  Host arrays: the span the
// strides cover goes through a device buffer and the same kernels; of an export only the brick's cells reach the caller's array.
// Every refusal comes before the first launch.
int CZ::FieldIO(int which, void* a, int abytes, const long long* stride, int on_device, void* user_stream, int op, double scale, double* sumsq,
                const char* who) {
  auto refuse = [&](const char* why) { return bc_refuse(who, why); };
  const bool to_user = op == FIO_EXPORT || op == FIO_RESIDUAL;
  const bool refine = op == FIO_RESIDUAL || op == FIO_ADD;
  const bool none = op == FIO_RESIDUAL && !a;  // the norm only
  if (!set_up) return refuse("no problem is set up (cz_setup first)");
  if (refine) {
    if (SW_maf) return refuse("the handle's operator is a MAF one, not the unit-coefficient operator");
    const REAL_TYPE rs = (REAL_TYPE)scale;
    if (!(scale > 0.0) || !std::isfinite(scale) || !(rs > (REAL_TYPE)0) || !std::isfinite(rs)) return refuse("the scale must be finite and positive");
    if (op == FIO_RESIDUAL && !sumsq) return refuse("NULL pointer");
    if (!none && abytes != 4 && abytes != 8) return refuse("the element size must be 4 or 8 bytes");
  }
  long long span = 1;
  if (!none)
    if (const char* why = field_check(a, abytes, stride, &span)) return refuse(why);
  if (to_user && !none)
    if (const char* why = field_distinct(stride)) return refuse(why);
  hipStream_t st = stream();
  REAL_TYPE* arr = which == 0 ? RHS : P;
  void* dev = a;
  const size_t span_bytes = (size_t)span * (size_t)abytes;
  if (none) {
  } else if (on_device) {
    if (const char* why = field_on_device(a)) return refuse(why);
    field_wait_for(user_stream);
  } else {
    dev = field_stage(span_bytes);
    // (an export fills the brick's cells of the device span only; the host copies exactly those cells below -- the other elements of the
    // caller's span are not the library's to touch: they may be another rank's cells of one shared array)
    if (!to_user) HIP_CHECK(hipMemcpyAsync(dev, a, span_bytes, hipMemcpyHostToDevice, st));
  }
  const int form = field_form == 3 ? 3 : 0;
  if (op == FIO_RESIDUAL) {
    // (the stencil reads one ghost layer of P; a solve may have left it one exchange behind)
    if (!Comm_S(P)) return 0;
    mirror(P);
    if (coef_on()) {
      last_field_form = field_residual_coef_async(P, RHS, WRK, dev, abytes, size, innerFidx, GUIDE, stride, coef_b[0], coef_b[1], coef_b[2], scale, form, d_res->field_sumsq);
    } else {
      last_field_form = field_residual_async(P, RHS, WRK, dev, abytes, size, innerFidx, GUIDE, stride, cf, scale, form, d_res->field_sumsq);
    }
  } else if (op == FIO_ADD) {
    last_field_form = field_add_async(P, dev, abytes, size, innerFidx, GUIDE, stride, scale, form);
  } else {
    last_field_form = field_copy_async(arr, static_cast<REAL_TYPE*>(dev), size, GUIDE, stride, to_user ? 1 : 0, form);
  }
  if (!last_field_form) return refuse("no kernel form takes these strides");
  if (!to_user) {
    // the ghost layers as Setup fills them; WRK's copy of P's shell is stale
    if (which == 0 && op == FIO_IMPORT && closed_box) {  // (the closed box keeps the right-hand side compatible; its exchange included)
      if (!project_rhs()) return 0;
    } else if (!Comm_S2(arr)) {
      return 0;
    }
    if (which == 1) {  // (Neumann faces: what the caller passed there is not data)
      mirror(P);
      wrk_shell_tag = 0;
    }
  }
  if (op == FIO_RESIDUAL) {
    if (!Comm_SUM_dev(d_res->field_sumsq, 1)) return 0;
    fetch_queued(d_res->field_sumsq);  // (the wait is the hand-back's below)
  }
  if (none) {
    HIP_CHECK(hipStreamSynchronize(st));
  } else if (!on_device) {
    std::vector<unsigned char> tmp;
    if (to_user) {
      tmp.resize(span_bytes);
      HIP_CHECK(hipMemcpyAsync(tmp.data(), dev, span_bytes, hipMemcpyDeviceToHost, st));
    }
    HIP_CHECK(hipStreamSynchronize(st));
    if (to_user) field_copy_cells(a, tmp.data(), abytes, stride);
  } else {
    field_hand_back(user_stream, op == FIO_RESIDUAL);  // (the one wait with a stream: the sum is a host value on return)
  }
  if (op == FIO_RESIDUAL) *sumsq = h_scal->field_sumsq[0];
  return 1;
}

// The projection step on a staggered velocity (cz_set_rhs_div, cz_sub_grad): vel = the three components, bricks of REAL_TYPE
// with one stride triple.  PRJ_DIV: RHS = div vel scale, then what cz_set_rhs does after its import; *sumsq (may be NULL) = sum div^2.
// PRJ_GRAD: vel = vel - grad P scale in place, P's face layers re-made first.  Checks, hand-over and staging are FieldIO's; every refusal
// comes before the first launch.
int CZ::ProjectIO(int op, REAL_TYPE* const* vel, const long long* stride, int on_device, void* user_stream, double scale, double* sumsq, const char* who) {
  auto refuse = [&](const char* why) { return bc_refuse(who, why); };
  const int abytes = (int)sizeof(REAL_TYPE);
  if (const char* why = bc_unready(this)) return refuse(why);  // (no set-up, a MAF operator)
  if (numProc > 1)
    return refuse("a decomposed run: faces between bricks need an exchange of one velocity layer, which is the follow-up (single domain only)");
  const REAL_TYPE rs = (REAL_TYPE)scale;
  if (!(scale > 0.0) || !std::isfinite(scale) || !(rs > (REAL_TYPE)0) || !std::isfinite(rs)) return refuse("the scale must be finite and positive");
  long long span = 1;
  for (int c = 0; c < 3; c++)
    if (const char* why = field_check(vel[c], abytes, stride, &span)) return refuse(why);
  if (op == PRJ_GRAD) {
    if (const char* why = field_distinct(stride)) return refuse(why);
    if (vel[0] == vel[1] || vel[0] == vel[2] || vel[1] == vel[2]) return refuse("two components of the velocity are the same array");
  }
  if (on_device)
    for (int c = 0; c < 3; c++)
      if (const char* why = field_on_device(vel[c])) return refuse(why);
  hipStream_t st = stream();
  const size_t span_bytes = (size_t)span * (size_t)abytes;
  REAL_TYPE* dev[3] = {vel[0], vel[1], vel[2]};
  if (on_device) {
    field_wait_for(user_stream);
  } else {
    unsigned char* stage = static_cast<unsigned char*>(field_stage(3 * span_bytes));
    for (int c = 0; c < 3; c++) {
      dev[c] = reinterpret_cast<REAL_TYPE*>(stage + (size_t)c * span_bytes);
      HIP_CHECK(hipMemcpyAsync(dev[c], vel[c], span_bytes, hipMemcpyHostToDevice, st));
    }
  }
  const int form = field_form == 3 ? 3 : 0;
  if (op == PRJ_DIV) {
    last_field_form = field_div_async(RHS, dev[0], dev[1], dev[2], size, GUIDE, stride, bc.per, scale, form, d_res->field_sumsq);
  } else {
    mirror(P);
    if (coef_on()) last_field_form = field_grad_coef_async(dev[0], dev[1], dev[2], P, coef_b[0], coef_b[1], coef_b[2], size, GUIDE, stride, bc.per, scale, form);
    else last_field_form = field_grad_async(dev[0], dev[1], dev[2], P, size, GUIDE, stride, bc.per, scale, form);
  }
  if (!last_field_form) return refuse("no kernel form takes these strides");
  if (op == PRJ_DIV) {
    if (closed_box) {  // (as cz_set_rhs: the closed box keeps the right-hand side compatible)
      if (!project_rhs()) return 0;
    } else if (!Comm_S2(RHS)) {
      return 0;
    }
    if (sumsq) fetch_queued(d_res->field_sumsq);  // (the wait is the hand-back's below)
  }
  if (!on_device) {
    std::vector<unsigned char> tmp;
    if (op == PRJ_GRAD) {
      tmp.resize(3 * span_bytes);
      HIP_CHECK(hipMemcpyAsync(tmp.data(), dev[0], 3 * span_bytes, hipMemcpyDeviceToHost, st));
    }
    HIP_CHECK(hipStreamSynchronize(st));
    if (op == PRJ_GRAD)
      for (int c = 0; c < 3; c++) field_copy_cells(vel[c], tmp.data() + (size_t)c * span_bytes, abytes, stride);
  } else {
    field_hand_back(user_stream, op == PRJ_DIV && sumsq);  // (a sum asked for is a host value on return; without one no host wait)
  }
  if (op == PRJ_DIV && sumsq) *sumsq = h_scal->field_sumsq[0];
  return 1;
}

// Face coefficients for pcg (cz_set_face_coef): b = bx, by, bz, three bricks with one stride triple, laid out and handed over as
// the velocity of ProjectIO.  They are copied into padded arrays of the handle (the import kernels of cz_set_field), one more pass writes the
// alias faces of the periodic directions, the scaling s and the count of values that are not finite and positive; the call waits for that
// count.  All three NULL: the state is cleared.  Every refusal but that of a bad value comes before the first launch and changes nothing; a
// bad value leaves the handle without coefficients.
void CZ::coef_clear() {
  if (!coef_on() && !coef_b[0]) return;
  if (mg) czhip_mg_set_coef(mg, nullptr, nullptr, nullptr);  // (a hierarchy that reads the arrays, cz_set_coef_mg: the constant one again)
  HIP_CHECK(hipStreamSynchronize(stream()));
  for (REAL_TYPE*& a : coef_b) {
    if (a) czhip_free(a);
    a = nullptr;
  }
  if (coef_s) czhip_free(coef_s);
  coef_s = nullptr;
  coef_per = 0;
}

bool CZ::coef_prepare(int per) {
  HIP_CHECK(hipMemsetAsync(&d_res->coef_bad, 0, sizeof(unsigned), stream()));  // (the counter's own zeroing: the kernel counts atomically)
  coef_prep_async(coef_b[0], coef_b[1], coef_b[2], coef_s, size, innerFidx, GUIDE, per, coef_per, &d_res->coef_bad);
  const unsigned bad = *fetch(&d_res->coef_bad);
  coef_per = per;
  if (bad) coef_clear();
  return bad == 0u;
}

int CZ::SetFaceCoef(REAL_TYPE* const* b, const long long* stride, int on_device, void* user_stream) {
  const char* const who = "cz_set_face_coef";
  auto refuse = [&](const char* why) { return bc_refuse(who, why); };
  const int abytes = (int)sizeof(REAL_TYPE);
  if (const char* why = bc_unready(this)) return refuse(why);  // (no set-up, a MAF operator)
  const int given = (b[0] != nullptr) + (b[1] != nullptr) + (b[2] != nullptr);
  if (given == 0) {  // back to the unit coefficients: the work vectors as the fused passes read them (set_bc does the same)
    coef_clear();
    for (REAL_TYPE* a : {cg_z, cg_p[0], cg_p[1]})
      if (a) HIP_CHECK(hipMemsetAsync(a, 0, padded_cells() * sizeof(REAL_TYPE), stream()));
    czhip_sync();
    return 1;
  }
  if (given != 3) return refuse("bx, by, bz: all three arrays, or all three NULL (which clears the coefficients)");
  if (numProc > 1)
    return refuse("a decomposed run: the faces in the ghost layers need an exchange of the coefficients, which is the follow-up (single domain only)");
  long long span = 1;
  for (int c = 0; c < 3; c++)
    if (const char* why = field_check(b[c], abytes, stride, &span)) return refuse(why);
  if (on_device)
    for (int c = 0; c < 3; c++)
      if (const char* why = field_on_device(b[c])) return refuse(why);
  hipStream_t st = stream();
  const size_t span_bytes = (size_t)span * (size_t)abytes;
  REAL_TYPE* dev[3] = {b[0], b[1], b[2]};
  if (on_device) {
    field_wait_for(user_stream);
  } else {
    unsigned char* stage = static_cast<unsigned char*>(field_stage(3 * span_bytes));
    for (int c = 0; c < 3; c++) {
      dev[c] = reinterpret_cast<REAL_TYPE*>(stage + (size_t)c * span_bytes);
      HIP_CHECK(hipMemcpyAsync(dev[c], b[c], span_bytes, hipMemcpyHostToDevice, st));
    }
  }
  for (REAL_TYPE*& a : coef_b)
    if (!a) a = czhip_alloc_s3d(size);
  if (!coef_s) coef_s = czhip_alloc_s3d(size);
  const int form = field_form == 3 ? 3 : 0;
  int took = 0;
  for (int c = 0; c < 3; c++) {
    took = field_copy_async(coef_b[c], dev[c], size, GUIDE, stride, 0, form);
    if (!took) break;
  }
  if (took) last_field_form = took;
  if (on_device) field_hand_back(user_stream, false);  // (the caller's arrays are free from here on)
  coef_per = 0;
  if (!took) {
    coef_clear();
    return refuse("no kernel form takes these strides (the handle is left without coefficients)");
  }
  if (!coef_prepare(bc.per))  // (the one host wait)
    return refuse("a coefficient on a face that the operator reads is not finite and positive (the handle is left without coefficients)");
  // the work vectors whose shells the fused passes read as zeros (the unfused direction leaves mirrors and wraps there): as set_bc
  for (REAL_TYPE* a : {cg_z, cg_p[0], cg_p[1]})
    if (a) HIP_CHECK(hipMemsetAsync(a, 0, padded_cells() * sizeof(REAL_TYPE), st));
  const bool coef_mg_ok = coef_mg_settle(who, false);  // (cz_set_coef_mg: the hierarchy is built from the new values)
  czhip_sync();
  return coef_mg_ok ? 1 : 0;
}

// profiling.txt (cz_Evaluate.cpp:506-545).  The reference prints PMlib's "Basic Report" (PMlib 6.4.x is a third-party
// library that is not part of the reference tree); this is the same table -- one line per measured section with call
// count, accumulated time, share, time per call, operation count and rate -- filled from the library's HIP-event timing
// of its launches (czhip_timing), under the reference's section labels (cz_miscel.cpp:177-262) where a launch maps to one.
void CZ::WriteProfile(FILE* fp) const {
  struct Sec {
    const char* label;   // reference label (or the nearest description)
    const char* lib;     // czhip_timing label
    double flop_per_call;
  };
  const double n = npts();
  const bool maf = SW_maf != 0;
  const int kn = innerFidx[K_plus] - innerFidx[K_minus] + 1;
  const int pn = pcr_num_stage(kn);
  const double pcr_flop = (n / kn) * (kn * 6.0 + kn * (pn - 1) * 14.0 + (double)(1 << (pn > 0 ? pn - 1 : 0)) * 9.0 + kn * 6.0 + 6.0) * 0.5;
  const Sec secs[] = {
      {maf ? "JACOBI_MAF_kernel" : "JACOBI_kernel", "jacobi", (maf ? 66.0 : 18.0) * n},
      {"JACOBI_kernel x2 (fused pair)", "jacobi2", 36.0 * n},
      {maf ? "SOR2SMA_MAF_kernel" : "SOR2SMA_kernel", "rbsor", (maf ? 33.0 : 9.0) * n},
      {"SOR2SMA_kernel x2 (both colours)", "rbsor2", 18.0 * n},
      {"Shell slabs of a fused pass", "pair_shell", 0.0},
      {"PCR_RB", "pcr_rb", pcr_flop},
      {maf ? "SOR_MAF_kernel" : "SOR_kernel", "psor", (maf ? 66.0 : 18.0) * n},
      {"Blas_AX", "calc_ax", (maf ? 63.0 : 13.0) * n},
      {"Blas_Residual", "calc_rk", (maf ? 63.0 : 14.0) * n},
      {"Dot1 / Dot2", "dot", 2.0 * n},
      {"Blas_TRIAD / BiCG_1 / BiCG_2", "ewise", 0.0},
      {"Residual reduction", "reduce", 0.0},
      {"MG restriction (residual + sum)", "mg_restrict", 0.0},
      {"MG Jacobi sweep (coarse level)", "mg_smooth", 0.0},
      {"MG prolongation", "mg_prolong", 0.0},
      {"MG tail (coarse levels in LDS)", "mg_tail", 0.0},
      {"MG red-black colour sweep (coarse level)", "mg_rb", 0.0},
  };
  char host[256] = "unknown";
  gethostname(host, sizeof(host) - 1);
  time_t now = time(nullptr);
  char date[64];
  strftime(date, sizeof(date), "%Y/%m/%d : %H:%M:%S", localtime(&now));
  double tot_ms = 0.0;
  struct Row {
    const Sec* s;
    int calls;
    double ms;
  };
  std::vector<Row> rows;
  for (const Sec& s : secs) {
    double ms = 0.0;
    const int c = czhip_timing_read(s.lib, &ms);
    if (c == 0) continue;
    rows.push_back({&s, c, ms});
    tot_ms += ms;
  }
  std::sort(rows.begin(), rows.end(), [](const Row& a, const Row& b) { return a.ms > b.ms; });  // time cost order
  fprintf(fp, "\n# PMlib Basic Report -------------------------------------------------------\n\n");
  fprintf(fp, "\tTiming Statistics Report (PMlib layout; sections timed with HIP events on the GPU stream)\n");
  fprintf(fp, "\tHost name : %s\n\tDate      : %s\n\n\tCubeZ hot path on %s\n\n", host, date, czhip_arch());
  fprintf(fp, "\tParallel Mode:   %d process%s x 1 GPU\n\n", numProc, numProc > 1 ? "es" : "");
  fprintf(fp, "\tTotal execution time            = %e [sec]\n", solve_seconds);
  fprintf(fp, "\tTotal time of measured sections = %e [sec]\n\n", tot_ms * 1e-3);
  fprintf(fp, "\tExclusive sections statistics per process and total job.\n\n");
  fprintf(fp, "\tSection                          |  call  |        accumulated time[sec]           | [flop counts]\n");
  fprintf(fp, "\tLabel                            |        |      avr   avr[%%]     sdv    avr/call  |      avr       sdv   speed\n");
  fprintf(fp, "\t---------------------------------+--------+----------------------------------------+----------------------------\n");
  double tot_flop = 0.0;
  for (const Row& r : rows) {
    const double sec = r.ms * 1e-3, flop = r.s->flop_per_call * r.calls;
    tot_flop += flop;
    fprintf(fp, "\t%-33s: %8d   %9.3e %6.2f  %8.2e  %9.3e    %9.3e  %8.2e  %7.2f %s\n", r.s->label, r.calls, sec,
            tot_ms > 0 ? 100.0 * r.ms / tot_ms : 0.0, 0.0, sec / r.calls, flop, 0.0, sec > 0 ? flop / sec * 1e-12 : 0.0, "Tflops");
  }
  fprintf(fp, "\t---------------------------------+--------+----------------------------------------+----------------------------\n");
  fprintf(fp, "\t%-33s  %8s   %9.3e %37s %9.3e  %8s  %7.2f %s\n", "Sections per process", "", tot_ms * 1e-3, "", tot_flop, "",
          tot_ms > 0 ? tot_flop / (tot_ms * 1e-3) * 1e-12 : 0.0, "Tflops");
  fprintf(fp, "\t---------------------------------+--------+----------------------------------------+----------------------------\n");
  fprintf(fp, "\t%-33s  %8s   %9.3e %37s %9.3e  %8s  %7.2f %s\n\n", "Sections total job", "", tot_ms * 1e-3, "", tot_flop * numProc, "",
          tot_ms > 0 ? tot_flop * numProc / (tot_ms * 1e-3) * 1e-12 : 0.0, "Tflops");
  fprintf(fp, "\tInclusive section: %s  = %e [sec] (host wall clock around the solver loop)\n", printMethod(ls_type), solve_seconds);
}

// fileout_t (cz_utility.f90:17-47, the -D_aurora_=1 body): a Fortran sequential unformatted file -- every record framed
// by its byte length (4-byte integer) -- holding (1,1) | (ix,jx,kx) | org | (dh,dh,dh) | (0, 0.0) | s(1:kx,1:ix,1:jx) with
// i fastest, then j, then k.  `s` is the padded host copy of a field.
bool CZ::WriteSph(const char* fname, const REAL_TYPE* s) const {
  FILE* fp = fopen(fname, "wb");
  if (!fp) {
    printf("\tSorry, can't open '%s' file. Write failed.\n", fname);
    return false;
  }
  const int g = GUIDE, ix = size[0], jx = size[1], kx = size[2];
  const size_t nk = kx + 2 * g, ni = ix + 2 * g;
  auto rec = [&](const void* a, size_t na, const void* b = nullptr, size_t nb = 0) {
    const int32_t len = (int32_t)(na + nb);
    fwrite(&len, 4, 1, fp);
    fwrite(a, 1, na, fp);
    if (b) fwrite(b, 1, nb, fp);
    fwrite(&len, 4, 1, fp);
  };
  const int32_t one[2] = {1, 1}, dims[3] = {ix, jx, kx}, nn = 0;
  const REAL_TYPE dh3[3] = {pitch[0], pitch[0], pitch[0]}, rtime = 0;
  rec(one, sizeof(one));
  rec(dims, sizeof(dims));
  rec(origin, 3 * sizeof(REAL_TYPE));
  rec(dh3, sizeof(dh3));
  rec(&nn, 4, &rtime, sizeof(REAL_TYPE));
  const size_t nbytes = (size_t)ix * jx * kx * sizeof(REAL_TYPE);
  if (nbytes > 0x7ffffff7u) {
    printf("\t'%s': the field record exceeds the 2 GiB a 4-byte record length can frame. Write failed.\n", fname);
    fclose(fp);
    return false;
  }
  const int32_t len = (int32_t)nbytes;
  fwrite(&len, 4, 1, fp);
  std::vector<REAL_TYPE> slab((size_t)ix * jx);
  for (int k = 1; k <= kx; k++) {
    for (int j = 1; j <= jx; j++)
      for (int i = 1; i <= ix; i++)
        slab[(size_t)(j - 1) * ix + (i - 1)] = s[(size_t)(k + g - 1) + (size_t)(i + g - 1) * nk + (size_t)(j + g - 1) * nk * ni];
    fwrite(slab.data(), sizeof(REAL_TYPE), slab.size(), fp);
  }
  fwrite(&len, 4, 1, fp);
  const bool ok = !ferror(fp);
  fclose(fp);
  return ok;
}

// exact_t (cz_utility.f90:52-82) on the host: the analytic solution on the whole brick (1..ix, 1..jx, 1..kx), padded layout
void CZ::Exact(std::vector<REAL_TYPE>& e) const {
  const int g = GUIDE;
  const size_t nk = size[2] + 2 * g, ni = size[0] + 2 * g, nj = size[1] + 2 * g;
  e.assign(nk * ni * nj, (REAL_TYPE)0);
  volatile REAL_TYPE one = 1.0, two = 2.0;
#ifdef CZ_REAL_IS_DOUBLE
  const REAL_TYPE r2 = sqrt(two), pi = 2.0 * asin(one);
#else
  const REAL_TYPE r2 = sqrtf(two), pi = 2.0f * asinf(one);
#endif
  const REAL_TYPE dh = pitch[0];
  for (int j = 1; j <= size[1]; j++)
    for (int i = 1; i <= size[0]; i++)
      for (int k = 1; k <= size[2]; k++) {
        const REAL_TYPE x = G_origin[0] + dh * (REAL_TYPE)(head[0] - 1 + i - 1);
        const REAL_TYPE y = G_origin[1] + dh * (REAL_TYPE)(head[1] - 1 + j - 1);
        const REAL_TYPE z = G_origin[2] + dh * (REAL_TYPE)(head[2] - 1 + k - 1);
#ifdef CZ_REAL_IS_DOUBLE
        e[(size_t)(k + g - 1) + (size_t)(i + g - 1) * nk + (size_t)(j + g - 1) * nk * ni] =
            sin(pi * x) * sin(pi * y) / sinh(r2 * pi) * (sinh(r2 * pi * z) - sinh(r2 * pi * (z - (REAL_TYPE)1.0)));
#else
        e[(size_t)(k + g - 1) + (size_t)(i + g - 1) * nk + (size_t)(j + g - 1) * nk * ni] =
            sinf(pi * x) * sinf(pi * y) / sinhf(r2 * pi) * (sinhf(r2 * pi * z) - sinhf(r2 * pi * (z - (REAL_TYPE)1.0)));
#endif
      }
}

// Debug epilogue (cz_Evaluate.cpp:550-563): exact_t_ + err_t_ of cz_utility.f90:52-129 restated on the host
// (out of the hot path; the field comes back over PCIe once).
double CZ::ErrorMax(int loc[3]) {
  const int g = GUIDE;
  const size_t nk = size[2] + 2 * g, ni = size[0] + 2 * g, nj = size[1] + 2 * g;
  std::vector<REAL_TYPE> p(nk * ni * nj);
  Field(p.data());
  volatile REAL_TYPE one = 1.0, two = 2.0;
#ifdef CZ_REAL_IS_DOUBLE
  const REAL_TYPE r2 = sqrt(two), pi = 2.0 * asin(one);
#define CZ_SIN sin
#define CZ_SINH sinh
#else
  const REAL_TYPE r2 = sqrtf(two), pi = 2.0f * asinf(one);
#define CZ_SIN sinf
#define CZ_SINH sinhf
#endif
  const REAL_TYPE dh = pitch[0];
  double d = 0.0;
  loc[0] = loc[1] = loc[2] = -1;
  for (int j = innerFidx[J_minus]; j <= innerFidx[J_plus]; j++)
    for (int i = innerFidx[I_minus]; i <= innerFidx[I_plus]; i++)
      for (int k = innerFidx[K_minus]; k <= innerFidx[K_plus]; k++) {
        const REAL_TYPE x = G_origin[0] + dh * (REAL_TYPE)(head[0] - 1 + i - 1);
        const REAL_TYPE y = G_origin[1] + dh * (REAL_TYPE)(head[1] - 1 + j - 1);
        const REAL_TYPE z = G_origin[2] + dh * (REAL_TYPE)(head[2] - 1 + k - 1);
        const REAL_TYPE e = CZ_SIN(pi * x) * CZ_SIN(pi * y) / CZ_SINH(r2 * pi) *
                            (CZ_SINH(r2 * pi * z) - CZ_SINH(r2 * pi * (z - (REAL_TYPE)1.0)));  // cz_utility.f90:75
        const REAL_TYPE r = p[(size_t)(k + g - 1) + (size_t)(i + g - 1) * nk + (size_t)(j + g - 1) * nk * ni] - e;
        const double qq = fabs((double)r);
        if (d < qq) {
          d = qq;
          loc[0] = i, loc[1] = j, loc[2] = k;
        }
      }
  if (numProc > 1) {
    // Comm_MAX_1 (cz_Evaluate.cpp:558): the maximum over ranks; location stays the local one as in the reference
    d = comm_allreduce_max_host(comm, d);
  }
  return d;
}

// ============================================================================================================
// Part 4 of include/cz_hip.h
// ============================================================================================================
struct cz_handle {
  CZ cz;
};

extern "C" {
cz_handle* cz_create(void) { return new cz_handle(); }
void cz_destroy(cz_handle* h) { delete h; }
int cz_evaluate(cz_handle* h, int argc, char** argv) { return h->cz.Evaluate(argc, argv); }
int cz_setup(cz_handle* h, int argc, char** argv) { return h->cz.Setup(argc, argv); }
int cz_solve(cz_handle* h) { return h->cz.Solve(); }
int cz_sweeps(cz_handle* h, int n) { return h->cz.Sweeps(n); }
int cz_result_iter(const cz_handle* h) { return h->cz.result_itr; }
double cz_result_res(const cz_handle* h) { return h->cz.result_res; }
int cz_history(const cz_handle* h, double* out, int cap) {
  const int n = (int)h->cz.history.size();
  for (int i = 0; i < n && i < cap; i++) out[i] = h->cz.history[i];
  return n;
}
void cz_field(const cz_handle* h, CZ_REAL* host_out) { h->cz.Field(host_out); }
int cz_set_rhs(cz_handle* h, const CZ_REAL* src, const long long* stride, int on_device, void* ready_stream) {
  return h ? h->cz.FieldIO(0, const_cast<CZ_REAL*>(src), (int)sizeof(CZ_REAL), stride, on_device, ready_stream, CZ::FIO_IMPORT, 1.0, nullptr, "cz_set_rhs") : 0;
}
int cz_set_field(cz_handle* h, const CZ_REAL* src, const long long* stride, int on_device, void* ready_stream) {
  return h ? h->cz.FieldIO(1, const_cast<CZ_REAL*>(src), (int)sizeof(CZ_REAL), stride, on_device, ready_stream, CZ::FIO_IMPORT, 1.0, nullptr, "cz_set_field") : 0;
}
int cz_get_field(cz_handle* h, CZ_REAL* dst, const long long* stride, int on_device, void* done_stream) {
  return h ? h->cz.FieldIO(1, dst, (int)sizeof(CZ_REAL), stride, on_device, done_stream, CZ::FIO_EXPORT, 1.0, nullptr, "cz_get_field") : 0;
}
int cz_get_residual(cz_handle* h, void* dst, int dst_real_bytes, const long long* stride, int on_device, void* done_stream, double scale, double* sumsq) {
  return h ? h->cz.FieldIO(1, dst, dst_real_bytes, stride, on_device, done_stream, CZ::FIO_RESIDUAL, scale, sumsq, "cz_get_residual") : 0;
}
int cz_add_field(cz_handle* h, const void* src, int src_real_bytes, const long long* stride, int on_device, void* ready_stream, double scale) {
  return h ? h->cz.FieldIO(1, const_cast<void*>(src), src_real_bytes, stride, on_device, ready_stream, CZ::FIO_ADD, scale, nullptr, "cz_add_field") : 0;
}
int cz_set_rhs_div(cz_handle* h, const CZ_REAL* u, const CZ_REAL* v, const CZ_REAL* w, const long long* stride, int on_device, void* ready_stream, double scale,
                   double* sumsq) {
  CZ_REAL* const vel[3] = {const_cast<CZ_REAL*>(u), const_cast<CZ_REAL*>(v), const_cast<CZ_REAL*>(w)};
  return h ? h->cz.ProjectIO(CZ::PRJ_DIV, vel, stride, on_device, ready_stream, scale, sumsq, "cz_set_rhs_div") : 0;
}
int cz_sub_grad(cz_handle* h, CZ_REAL* u, CZ_REAL* v, CZ_REAL* w, const long long* stride, int on_device, void* stream, double scale) {
  CZ_REAL* const vel[3] = {u, v, w};
  return h ? h->cz.ProjectIO(CZ::PRJ_GRAD, vel, stride, on_device, stream, scale, nullptr, "cz_sub_grad") : 0;
}
int cz_set_face_coef(cz_handle* h, const CZ_REAL* bx, const CZ_REAL* by, const CZ_REAL* bz, const long long* stride, int on_device, void* ready_stream) {
  CZ_REAL* const b[3] = {const_cast<CZ_REAL*>(bx), const_cast<CZ_REAL*>(by), const_cast<CZ_REAL*>(bz)};
  return h ? h->cz.SetFaceCoef(b, stride, on_device, ready_stream) : 0;
}
int cz_set_coef_mg(cz_handle* h, int on) { return h ? h->cz.SetCoefMg(on) : 0; }
int cz_set_mg_lines(cz_handle* h, int on) { return h ? h->cz.SetMgLines(on) : 0; }
int cz_set_neumann(cz_handle* h, const int* faces) { return h ? h->cz.SetNeumann(faces) : 0; }
int cz_set_closed_box(cz_handle* h, int on) { return h ? h->cz.SetClosedBox(on) : 0; }
int cz_set_periodic(cz_handle* h, const int* dirs) {
  if (!h) fprintf(stderr, "cz_set_periodic: NULL handle\n");
  return h ? h->cz.SetPeriodic(dirs) : 0;
}
double cz_closed_mean(cz_handle* h, int which) { return h ? h->cz.ClosedMean(which) : std::nan(""); }
int cz_set_eps(cz_handle* h, double eps) {
  if (!h || !h->cz.set_up || !(eps > 0.0)) {
    fprintf(stderr, "cz_set_eps: %s\n", h && h->cz.set_up ? "the tolerance must be positive" : "no problem is set up (cz_setup first)");
    return 0;
  }
  h->cz.eps = eps;
  return 1;
}
int cz_set_itr_max(cz_handle* h, int n) {
  if (!h || !h->cz.set_up || n < 1) {
    fprintf(stderr, "cz_set_itr_max: %s\n", h && h->cz.set_up ? "at least one iteration" : "no problem is set up (cz_setup first)");
    return 0;
  }
  h->cz.ItrMax = n;
  return 1;
}
void cz_local_size(const cz_handle* h, int* size3, int* head3, int* nID6, int* inner6) {
  for (int a = 0; a < 3; a++) size3[a] = h->cz.size[a], head3[a] = h->cz.head[a];
  for (int f = 0; f < 6; f++) nID6[f] = h->cz.nID[f], inner6[f] = h->cz.innerFidx[f];
}
double cz_error_max(cz_handle* h, int* loc3) { return h->cz.ErrorMax(loc3); }
void cz_set_quiet(cz_handle* h, int q) { h->cz.quiet = q != 0; }
void cz_set_debug(cz_handle* h, int m) { h->cz.debug_mode = m; }
void cz_set_profile(cz_handle* h, int on) { h->cz.profile = on != 0; }
double cz_last_solve_seconds(const cz_handle* h) { return h->cz.solve_seconds; }
int cz_info(const cz_handle* h, int what) {
  const CZ& c = h->cz;
  switch (what) {
    case 0: return c.numProc;
    case 1: return c.pairs_ok ? 1 : 0;
    case 2: return c.n_shell;
    case 3: return c.overlap;
    case 4: return c.last_lag;
    case 10: return c.bicg_fused;
    case 11: return c.rb4_passes;
    case 12: return c.exact_reruns;
    case 13: return c.cg_fused;
    case 14: return c.jac3_passes;
    case 15: return c.mg ? czhip_mg_levels(c.mg) : c.mgd ? mgd_levels(c.mgd) : 0;
    case 16: return c.mg_cycles;
    case 17: return mgd_gather_level(c.mgd);
    case 18: return mgd_exchanges(c.mgd);
    case 19: return c.mg ? czhip_mg_kind(c.mg) : c.mgd ? 1 : 0;
    case 5: return comm_transport_ranks(c.comm);
    case 6: return c.comm_cus;
    case 7: return c.solve_plan.kind;
    case 8: return c.solve_plan.depth;
    case 9: return c.solve_plan.buffers;
    case 20: return c.last_field_form;
    case 21: return c.bc.nm;
    case 22: return c.closed_box;
    case 23: return c.bc.per;
    case 24: return c.pcg_void_start;
    case 25: return c.coef_on() ? 1 : 0;
    case 26: return c.jac4_passes;
    case 27: return c.coef_mg_on() ? 1 : 0;
    case 28: return c.mg_lines_on() ? 1 : 0;
    default: return -1;
  }
}
// the driver's and its communicator's copies of their own switches, name=value, one per line (the string lives until the next call on this thread)
const char* cz_config_in_force(const cz_handle* h) {
  static thread_local std::string text;
  const CZ& c = h->cz;
  const std::pair<const char*, int> rows[] = {
      {"overlap", c.overlap}, {"lag_reduce", c.lag_reduce}, {"comm_cus", c.numProc > 1 ? c.cfg.num(CZV_COMM_CUS, 2) : 0},
      {"comm_cus_reserved", c.comm_cus}, {"bicg_fuse", c.cfg.on(CZV_BICG_FUSE, true)}, {"bicg_devsc", c.cfg.on(CZV_BICG_DEVSC, true)},
      {"bicg_alias", c.cfg.on(CZV_BICG_ALIAS, true)}, {"cg_fuse", c.cfg.on(CZV_CG_FUSE, true)}, {"mg_tail", c.cfg.on(CZV_MG_TAIL, true)},
      {"mg_gather", c.cfg.num(CZV_MG_GATHER, 32768)}, {"mgrb_zero4", c.cfg.on(CZV_MGRB_ZERO4, true)}, {"field_form", c.field_form},
      {"comm_pack_j", comm_setting(c.comm, 0)}, {"comm_direct_messages", comm_setting(c.comm, 1)}, {"comm_one_comm", comm_setting(c.comm, 2)}};
  text.clear();
  for (const auto& r : rows) text += std::string(r.first) + "=" + std::to_string(r.second) + "\n";
  return text.c_str();
}
int cz_precondition(cz_handle* h, const CZ_REAL* r_dense, CZ_REAL* z_dense) {
  CZ& c = h->cz;
  if (!c.set_up || !(c.mg || c.mgd)) return 0;
  const size_t n = (size_t)(c.size[0] + 2 * GUIDE) * (c.size[1] + 2 * GUIDE) * (c.size[2] + 2 * GUIDE);
  czhip_h2d(c.cg_r, r_dense, n * sizeof(CZ_REAL));
  czhip_sync();
  const int ok = c.mg ? czhip_mg_apply_async(c.mg, c.cg_z, c.cg_r, c.ac1) : mgd_apply(c.mgd, c.cg_z, c.cg_r, c.ac1);
  czhip_sync();
  if (!ok) return -1;
  czhip_d2h(z_dense, c.cg_z, n * sizeof(CZ_REAL));
  return 1;
}
double cz_kernel_ms(const cz_handle* h, const char* label) {
  (void)h;
  double tot = 0.0;
  const int n = czhip_timing_read(label, &tot);
  return n > 0 ? tot / n : 0.0;
}
}  // extern "C"
