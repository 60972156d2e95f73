// cz_driver.h -- the restated host driver: class CZ of the reference (src/cz_cpp/cz.h:84-181, DomainInfo.h:30-49)
// with every 3-D array resident in HBM and the solver loops (cz_Poisson.cpp) rebuilt around asynchronous launches.
#ifndef CZ_DRIVER_H_
#define CZ_DRIVER_H_

#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "cz_config.h"
#include "cz_internal.h"
#include "cz_solvers.h"  // enum LinearSolver (cz_Define.h:68-89) and the table of the names accepted: one row each

typedef CZ_REAL REAL_TYPE;  // cz_Define.h:28-37
#include "cz_scalars.h"     // CzScalars, CzFlags: the layout of d_res / h_scal and of d_flag
#define GUIDE 2             // cz_Define.h:40

// CB_Define_stub.h:64-70 / cz_fparam.fi:10-16
enum { I_minus = 0, I_plus, J_minus, J_plus, K_minus, K_plus };

struct CommCtx;  // cz_comm.cpp (RCCL halo exchange / all-reduce); nullptr when numProc == 1

class CZ {
 public:
  // ---- DomainInfo (DomainInfo.h:30-49)
  int myRank = 0, numProc = 1;
  int nID[6] = {-1, -1, -1, -1, -1, -1};
  int head[3] = {1, 1, 1};
  int G_div[3] = {1, 1, 1};
  REAL_TYPE pitch[3] = {0, 0, 0};
  int size[3] = {0, 0, 0};
  REAL_TYPE origin[3] = {0, 0, 0};
  int G_size[3] = {0, 0, 0};
  REAL_TYPE G_origin[3] = {0, 0, 0};
  int innerFidx[6] = {0, 0, 0, 0, 0, 0};
  int idx1[6] = {0, 0, 0, 0, 0, 0};  // first sweep of a fused pass: innerFidx plus one layer into the ghost cells across rank-internal faces

  // ---- CZ (cz.h:84-133, 154-181)
  int debug_mode = 0;
  int ItrMax = 0;
  int ls_type = LS_NONE, pc_type = LS_NONE;
  double eps = 1.0e-5;
  REAL_TYPE ac1 = 0;
  double res_normal = 0.0;
  REAL_TYPE cf[7] = {1, 1, 1, 1, 1, 1, 6};
  std::string precon;
  FILE* fph = nullptr;
  std::string hist_name;

  REAL_TYPE *WRK = nullptr, *P = nullptr, *RHS = nullptr;
  // MAF flavour (cz.h:113-118, cz_Evaluate.cpp:245-253, 342-369): 1-D grid on the device, pivot array
  int SW_maf = 0;
  REAL_TYPE* MSK = nullptr;  // cz.h:95, cz_Evaluate.cpp:389 (line-SOR solvers)
  REAL_TYPE *d_xc = nullptr, *d_yc = nullptr, *d_zc = nullptr, *pvt = nullptr;
  REAL_TYPE *pcg_p = nullptr, *pcg_p_ = nullptr, *pcg_r = nullptr, *pcg_r0 = nullptr, *pcg_q = nullptr, *pcg_s = nullptr,
            *pcg_s_ = nullptr, *pcg_t_ = nullptr;
  // PCG's work vectors (the pcg_* above are BiCGSTAB's, named as in the reference); allocated only when pcg is selected
  REAL_TYPE *cg_r = nullptr, *cg_z = nullptr, *cg_p[2] = {nullptr, nullptr}, *cg_q = nullptr;
  cz_mg* mg = nullptr;           // the multigrid hierarchy of pcg ... mg | mgrb, allocated only then
  struct MgDist* mgd = nullptr;  // decomposed runs: the distributed V-cycle of pcg ... mg instead (cz_mg_dist.cpp)

  // ---- build-specific state
  bool quiet = false;
  bool profile = false;          // write profiling.txt after the solve (the cz command line turns it on; CZ_PROFILE=0 off)
  bool set_up = false;
  int result_itr = 0;
  double result_res = 0.0;
  std::vector<double> history;   // residual of iteration 1..n (index 0 = iteration 1)
  double solve_seconds = 0.0;
  int sweeps_done = 0;           // stationary-solver iterations executed so far (bench leg)
  CommCtx* comm = nullptr;
  // decomposed runs: the exchange of a fused pair runs on comm_stream while the interior is being swept
  hipStream_t comm_stream = nullptr;
  hipEvent_t ev_shell = nullptr, ev_src = nullptr, ev_comm = nullptr, ev_int = nullptr, ev_chk[2] = {nullptr, nullptr};
  bool pairs_ok = true;          // decomposed runs: EVERY brick can run the fused pass (agreed at set-up; the exchange pattern depends on it)
  int rb4_passes = 0;            // two-iteration red-black passes (rb4_k) of the last RBSOR solve (cz_info 11)
  int jac4_passes = 0;           // four-sweep Jacobi passes (jac4_k) of the last JACOBI solve (cz_info 26)
  int jac3_passes = 0;           // three-sweep Jacobi passes (jac3_k) of the last JACOBI solve (cz_info 14)
  int exact_reruns = 0;          // converged first iterations of a fused pass re-run alone from the pass's input, last JACOBI / RBSOR solve (cz_info 12)
  int mg_cycles = 0;             // V-cycles of the last PCG solve with mg (cz_info 16)
  int pcg_void_start = 0;        // the last solve was a PCG that stopped at a breakdown (|rho| < FLT_MIN) before any update of P: P is the caller's (cz_info 24)
  int cg_fused = 0;              // iterations of the last PCG solve whose direction update was made inside the SpMV pass (cz_info 13)
  int bicg_fused = 0;            // vector updates of the last BiCGSTAB solve that were made inside the first pair of a preconditioner solve (cz_info 10)
  bool in_precond = false;       // inside Preconditioner: an unchecked solve does not drain the queue (the caller's next launch follows in stream order)
  int last_lag = 0;              // the last stationary solve ran its all-reduce + test one pass behind (cz_info)
  CzBc bc;                       // the boundary faces of the global box as set (cz_bc.h; set_bc).  nm (cz_info 21): the zero-flux (Neumann) faces of
                                 // cz_set_neumann, DESIGN.md §5.13 -- P's face layers there hold the mirror of the first inner layer.  per (cz_info 23):
                                 // the periodic directions of cz_set_periodic, DESIGN.md §5.15 -- there P's two face layers hold the wrap and the
                                 // Neumann flags are ignored
  // face coefficients (cz_set_face_coef, cz_info 25): padded copies of the caller's bx, by, bz and the scaling s = sqrt(6 / D);
  // allocated while coefficients are in force, nullptr otherwise -- pcg then applies A_beta where it applies the operator and s M^-1 s where
  // it preconditions; every other solver is refused
  REAL_TYPE *coef_b[3] = {nullptr, nullptr, nullptr}, *coef_s = nullptr;
  bool coef_on() const { return coef_s != nullptr; }
  int coef_per = 0;              // the periodic directions whose face 0 holds the copy of face n - 2 in coef_b
  bool coef_prepare(int per);    // the alias faces for `per`, s, and the check (one host wait); false: a bad value, the arrays are freed
  void coef_clear();             // frees the four arrays (after the compute stream has drained)
  int SetFaceCoef(REAL_TYPE* const* b, const long long* stride, int on_device, void* user_stream);  // cz_set_face_coef: 1 / 0
  // the coefficients inside the multigrid hierarchy (cz_set_coef_mg, cz_info 27): the flag as asked for; in force while the
  // hierarchy holds the coefficients (coef_mg_settle keeps that in step with the flag, the coefficients and the preconditioner)
  int coef_mg = 0;
  bool coef_mg_on() const { return mg && mg->coef; }
  bool coef_mg_settle(const char* who, bool rebuilt);
  int SetCoefMg(int on);         // cz_set_coef_mg: 1 / 0
  // zebra line iterations along Z in mgrb's cycle (cz_set_mg_lines, cz_info 28): the flag as asked for; in force while the
  // coefficient hierarchy is and the preconditioner is mgrb (coef_mg_settle carries the flag to the hierarchy)
  int mg_lines = 0;
  bool mg_lines_on() const { return mg_lines && coef_mg_on() && mg->rb && mg->lines; }
  int SetMgLines(int on);        // cz_set_mg_lines: 1 / 0
  int closed_box = 0;            // the closed box (cz_set_closed_box, cz_info 22): mask 63 and the three projections of pcg
  double closed_m[3] = {0, 0, 0};  // the means last removed: right-hand side, initial residual, answer (cz_closed_mean)
  bool closed_m0_on_device = false;  // closed_m[0] is still d_res->rhs_mean (cz_set_rhs does not wait for it; ClosedMean fetches)
  double g_npts = 0.0;           // cells of the GLOBAL inner box (1 / res_normal)
  int field_form = 0;            // CZ_FIELD_FORM: 3 = the generic import / export kernel whatever the strides
  int last_field_form = 0;       // the kernel form of the last import / export (cz_info 20: 1 k rows, 2 tile transpose, 3 generic)
  hipEvent_t ev_io = nullptr;    // the hand-over between the caller's stream and the compute stream
  void* io_stage = nullptr;      // device copy of a host array's span
  size_t io_stage_cap = 0;       // ... its bytes
  CzConfig cfg;  // the environment as read when this object was created (cz_config.h)
  int skew_rank = -1, skew_ms = 0;  // CZ_TEST_SKEW=rank,ms: that rank sleeps before each look at the convergence flag (tests)
  void skew_wait() const;
  int lag_reduce = 1;            // CZ_LAG_REDUCE=0: residual all-reduce + test on the compute stream after every pass (no lag)
  REAL_TYPE* WRK2 = nullptr;     // third rotation buffer of the lagged mode
  int wrk_shell_tag = 0;         // whose shell WRK carries: 0 unknown, 1 P's (Dirichlet faces), 2 all zero (sync_wrk_shell)
  void sync_wrk_shell(const REAL_TYPE* X);
  int overlap = 1;               // CZ_OVERLAP=0 turns it off (exchange after the whole sweep, same results)
  // how the sweeps of the current / last stationary solve are executed (CZ::plan_pass; cz_info 7-9)
  struct PassPlan {
    enum Kind { SINGLE = 0, WHOLE = 1, SPLIT = 2 };
    int kind = SINGLE;  // SINGLE: one sweep / colour per launch; WHOLE: fused pass over the whole inner box; SPLIT: shell slabs + interior, exchange overlapped
    int depth = 1;      // ghost layers exchanged per pass
    int lag = 0;        // residual all-reduce + test one pass behind, on the exchange stream
    int buffers = 2;    // rotating field buffers
    int zero_start = 0; // the first pass takes the start vector as a literal zero
    int maf = 0, rb = 0;
    int comm_cus = 0;
  };
  PassPlan last_plan;            // the last plan made (the debug line prints a plan when it differs from this one)
  PassPlan solve_plan;           // the plan of the stationary sweeps of the current / last cz_solve or cz_sweeps (cz_info 7-9); a fresh one where it ran none
  bool plan_printed = false;
  int comm_cus = 0;              // CUs per XCD the sweeps leave to the exchange stream (CZ_COMM_CUS; 0 in single-domain runs)
  int n_shell = 0;               // shell boxes (cells within two layers of a rank-internal face), 1-based index ranges
  int shell_boxes[36];
  int interior[6], interior1[6]; // the rest of the inner box / its first-sweep range

  // device-side convergence bookkeeping (cz_Poisson.cpp:67-77 moved to the GPU)
  CzScalars* d_res = nullptr;    // residual sums, dot products and device-made scalars, one named member per user (cz_scalars.h)
  double* d_hist = nullptr;      // residual history, index = iteration
  int hist_cap = 0;
  CzFlags* d_flag = nullptr;     // converged flag, iteration at which it was set, the lagged split's two snapshots
  CzScalars* h_scal = nullptr;   // pinned: the mirror of d_res, member for member (fetch)
  int* h_flag = nullptr;         // pinned: the host's copies of d_flag's first two words, one pair per poll in flight

  CZ();
  ~CZ();

  int Evaluate(int argc, char** argv);  // cz_Evaluate.cpp:21-567
  int Setup(int argc, char** argv);     //   :21-391
  int Solve();                          //   :397-496
  int Sweeps(int n);
  double ErrorMax(int loc[3]);          //   :550-563
  void Field(REAL_TYPE* host) const;
  // the caller's own problem (part 4 of cz_hip.h): this rank's brick, cell (i, j, k) at a[i stride[0] + j stride[1] + k stride[2]],
  // into RHS (which 0) or P (which 1), or P out into it; elements of abytes bytes (REAL_TYPE's for the import and the export); 1 / 0.
  // FIO_RESIDUAL: (T)(r scale) of r = RHS - A P out into it (a NULL: no destination) and *sumsq = sum r^2 over the whole domain;
  // FIO_ADD: P = P + (REAL_TYPE)a scale on the cells every sweep updates
  enum { FIO_IMPORT = 0, FIO_EXPORT = 1, FIO_RESIDUAL = 2, FIO_ADD = 3 };
  int FieldIO(int which, void* a, int abytes, const long long* stride, int on_device, void* user_stream, int op, double scale, double* sumsq,
              const char* who);
  // the projection step on a staggered velocity (cz_set_rhs_div, cz_sub_grad): vel[3] = u, v, w, bricks with one stride triple.
  // PRJ_DIV: RHS = div vel scale, *sumsq (may be NULL) = sum div^2; PRJ_GRAD: vel = vel - grad P scale in place.  Single domain.
  enum { PRJ_DIV = 0, PRJ_GRAD = 1 };
  int ProjectIO(int op, REAL_TYPE* const* vel, const long long* stride, int on_device, void* user_stream, double scale, double* sumsq, const char* who);
  // what the two share: the checks (nullptr, or the refusal's line), the event hand-over, the staging of host arrays
  const char* field_check(const void* a, int abytes, const long long* stride, long long* span) const;
  const char* field_distinct(const long long* stride) const;
  const char* field_on_device(const void* a) const;
  void field_wait_for(void* user_stream);
  void field_hand_back(void* user_stream, bool host_waits);
  void* field_stage(size_t bytes);
  void field_copy_cells(void* a, const void* tmp, int abytes, const long long* stride) const;
  int SetNeumann(const int* faces);  // cz_set_neumann: 1, or 0 with one line on stderr and nothing changed
  int SetClosedBox(int on);          // cz_set_closed_box: likewise
  int SetPeriodic(const int* dirs);  // cz_set_periodic: likewise
  static const char* unsolvable(CzBc next, int closed);  // the setters' one rule on the combined state: nullptr, or the line of the refusal
  const char* bc_unready(const void* arg) const;         // what every setter refuses before it reads its argument: nullptr, or the line
  int set_bc(CzBc next, int closed, bool project, const char* who);  // the one way to a new state: the rule, the hierarchy, the store, the work vectors, P's face layers
  bool project(REAL_TYPE* A, REAL_TYPE* m_dev, REAL_TYPE* keep_dev);  // A <- A - mean(A) over the global inner box; d_res->project = this rank's sum A', sum A'^2
  double ClosedMean(int which);      // cz_closed_mean
  bool project_rhs();                // ... of RHS, ghost layers included; closed_m[0]
  void mirror(REAL_TYPE* X);         // X's face layers of the state: mirrors on the Neumann faces, wraps in the periodic directions (nothing without either)
  void WriteProfile(FILE* fp) const;                                             // cz_Evaluate.cpp:506-545
  bool WriteSph(const char* fname, const REAL_TYPE* padded_host_field) const;  // cz_utility.f90:17-47
  void Exact(std::vector<REAL_TYPE>& e) const;                                   // cz_utility.f90:52-82

 private:
  void setLS(const char* q);                                   // cz_Evaluate.cpp:684-803
  void setStrPre();                                            // :571-681
  double range_inner_index();                                  // cz_miscel.cpp:20-52
  bool decompose(int div_type);                                // replaces CBrick SubDomain (cz_Evaluate.cpp:103-159)
  void ensure_hist(int n);

  // cz_Poisson.cpp
  // the right-hand side of a preconditioner solve as the vector update that makes it (PBiCGSTAB): op 1: B = a*x + y, op 2: B = x + a*(z - b*y);
  // the first pair of the solve then makes B on its way instead of reading it (czhip_jacobi2_from_zero_made_async)
  struct BMade {
    int op;
    const REAL_TYPE* x;
    const REAL_TYPE* y;
    const REAL_TYPE* z;
    REAL_TYPE a, b;
    const REAL_TYPE* a_dev;  // where set: a lives on the device (bicg_scalar_async)
  };
  int JACOBI(double& res, REAL_TYPE* X, REAL_TYPE* B, int itr_max, double& flop, int s_type, bool converge_check = true,
             bool x_is_zero = false, const BMade* made = nullptr);
  bool bicg_fusable(int pc_type);
  bool xx_shell_is_zero(const REAL_TYPE* xx) const;
  int RBSOR(double& res, REAL_TYPE* X, REAL_TYPE* B, int itr_max, double& flop, int s_type, bool converge_check = true, bool x_is_zero = false,
            const BMade* made = nullptr);
  int PSOR(double& res, REAL_TYPE* X, REAL_TYPE* B, int itr_max, double& flop, int s_type, bool converge_check = true);
  int LSOR(double& res, REAL_TYPE* X, REAL_TYPE* B, int itr_max, double& flop, int s_type, bool converge_check = true);
  // the loop of s_type's family (cz_solvers.h): what Solve, Sweeps and Preconditioner call
  int run(int s_type, double& res, REAL_TYPE* X, REAL_TYPE* B, int itr_max, double& flop, bool converge_check = true, bool x_is_zero = false,
          const BMade* made = nullptr);
  // the read-back of d_res: `n` values from the member at `dev` on (n > 1: a group cz_scalars.h states) copied to the same member of h_scal
  // behind what the compute stream holds; the pointer to that mirror.  fetch waits for the copy, fetch_queued leaves the wait to the caller
  template <class T> const T* fetch_queued(const T* dev, int n = 1);
  template <class T> const T* fetch(const T* dev, int n = 1);
  REAL_TYPE dot_read(double& flop);
  REAL_TYPE Fdot1(REAL_TYPE* x, double& flop);
  REAL_TYPE Fdot2(REAL_TYPE* x, REAL_TYPE* y, double& flop);
  void Preconditioner(REAL_TYPE* xx, REAL_TYPE* bb, double& flop, int s_type, const BMade* made = nullptr);
  int PBiCGSTAB(double& res, REAL_TYPE* X, REAL_TYPE* B, double& flop, int s_type);
  int PCG(double& res, REAL_TYPE* X, REAL_TYPE* B, double& flop);  // beyond the reference (DESIGN.md "PCG")
  // ... the modes of one solve, decided once at its start; then the operator, the breakdown test and the steps (cz_driver.cpp, above CZ::PCG)
  struct CgMode {
    bool pc;        // a preconditioner (jacobi | mg | mgrb): z = M^-1 r in cg_z; none: z IS r and rho is the r.r of the update before
    bool fuse;      // CZ_CG_FUSE (default on): x, r and r.r in one guarded pass (czhip_cg_update_async); off: two triads and a dot
    // ... and the direction inside the SpMV pass (czhip_cg_dir_ax_async, ping-pong between cg_p[0] and cg_p[1]); else the update, Comm_S(p),
    // then the SpMV with its dot folded in.  The fused pass reads z's and p's shells as zeros: single domain only, no Neumann face (whose
    // layer of p is the mirror) nor a periodic direction (whose layer is the wrap), and no face coefficients (their SpMV stays unfused)
    bool fuse_dir;
    // face coefficients: A_beta where the operator is applied (cg_apply_A), and the preconditioner z = s M^-1 (s r) with
    // M^-1 the constant-coefficient one (cg_q is free for s r at that point) ...
    bool coef;
    bool scale;     // ... unless the hierarchy holds the coefficients (cz_set_coef_mg): z = M_beta^-1 r, no scaling either side
    bool closed;    // the closed box: the three projections, the lagged mean in sc[SC_LAG_MEAN]
    REAL_TYPE* z;   // cg_z, or cg_r
    double* d_rho;  // where rho is summed: cg.rho, or (none) cg.rr
  };
  bool cg_apply_A(REAL_TYPE* out, REAL_TYPE* p, const REAL_TYPE* b, double* dots);
  bool cg_breakdown(REAL_TYPE rho, int itr);
  bool cg_start(const CgMode& m, REAL_TYPE* X, const REAL_TYPE* B, REAL_TYPE& rho, double& flop);
  bool cg_apply_M(const CgMode& m, double& flop);
  bool cg_precondition(const CgMode& m, double& flop);
  bool cg_direction(const CgMode& m, int itr, int& cur, double& flop);
  int cg_update(const CgMode& m, REAL_TYPE* X, const REAL_TYPE* p, int itr, double& flop);
  bool cg_end(const CgMode& m, REAL_TYPE* X, double& flop);
  bool neumann_refused(const char* who, int s_type) const;          // a mask is set and the solver is not pcg: one line, true

  // cz_comm.cpp replacements (no-ops when numProc == 1, like cz_comm.cpp:25,76,104)
  bool Comm_S(REAL_TYPE* X, const int* skip_flag = nullptr);
  bool Comm_S2(REAL_TYPE* X, const int* skip_flag = nullptr);  // two layers + edges (fused Jacobi pairs)
  bool Comm_SUM_dev(double* d_val, int count, const int* skip_flag = nullptr);
  bool reduce_test(int nres, int itr, const int* skip = nullptr);
  void plan_overlap();
  bool pair_overlapped(REAL_TYPE* src, REAL_TYPE* dst, REAL_TYPE* B, int rb, const int* skip, double* res_slot = nullptr,
                       const czhip_internal::MafPtrs* maf = nullptr);
  PassPlan plan_pass(REAL_TYPE* X, REAL_TYPE* B, int s_type, int itr_max, bool converge_check, bool x_is_zero, bool rb, bool probe_only = false);
  bool Comm_SUM_1(double* host_val);

  // the host's lagging look at the device convergence flag (JACOBI, RBSOR, PSOR) and the skeleton JACOBI and RBSOR share (cz_driver.cpp)
  class FlagPoll;
  void wait_lagged_tests();
  struct Launch {
    int first_itr, n, src;  // first iteration, iterations, index of the source buffer
  };
  class FusedLoop;
  using Rerun = std::function<void(const Launch& l, int k, REAL_TYPE* src, REAL_TYPE* dst)>;
  bool fused_begin(FusedLoop& L, REAL_TYPE* X, int itr_max, bool x_is_zero, const BMade* made);
  bool split_pass(FusedLoop& L, int rb, int nres, int itr, const czhip_internal::MafPtrs* mpp);
  bool whole_exchange_test(FusedLoop& L, int nres, int itr);
  int zero_start_pass(REAL_TYPE* src, REAL_TYPE* dst, REAL_TYPE* B, const BMade* made, int rb);
  int fused_end(FusedLoop& L, REAL_TYPE* X, int itr_max, double& res, const Rerun& rerun);

  int finish_stationary(int itr_max, bool converge_check, double& res);
  void read_history(int n_exec, double& res);
  // line solvers: the stage count of the k lines (exits when there is none), the launches and exchanges of one iteration and its operation
  // count, the test after an iteration, the end of the solve
  int line_stages();
  bool line_iteration(const cz_solvers::Line& d, REAL_TYPE* X, REAL_TYPE* B, int pn);
  double line_flop(const cz_solvers::Line& d, int pn) const;
  int line_test(int itr, int s_type);
  int line_finish(int itr, int itr_max, bool converge_check, double& res, int s_type);
  // line solvers: the one-launch lexicographic sweep reports a lost hand-off between its workgroups as a NaN residual (every wait inside
  // it is bounded); the iterate is then void and the solve ends with "Solver error" instead of sweeping on (true = failed; message printed)
  bool sweep_failed(const char* solver);
  bool line_error = false;       // set by sweep_failed; PBiCGSTAB gives up when a line-solver preconditioner set it
  double npts() const;
  size_t padded_cells() const;   // cells of an array with its guide layers
};

// the distributed V-cycle of pcg ... mg (cz_mg_dist.cpp, DESIGN.md §5.10 "Decomposed runs")
// nullptr on a single domain; gather_points: CZ_MG_GATHER, tail: CZ_MG_TAIL
MgDist* mgd_create(const CZ& cz, CommCtx* comm0, int gather_points, bool tail);
void mgd_destroy(MgDist*);
int mgd_apply(MgDist*, REAL_TYPE* z, const REAL_TYPE* r, REAL_TYPE omg);  // z = V_0(r) on this rank's brick, collective
void mgd_set_bc(MgDist*, CzBc bc);  // the state of the global box, on every rank; periodic directions uncut
int mgd_levels(const MgDist*);
int mgd_gather_level(const MgDist*);
int mgd_exchanges(const MgDist*);  // halo exchanges + all-gathers of the last cycle

#endif
