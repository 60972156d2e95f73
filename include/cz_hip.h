/*
 * cz_hip.h -- C-ABI of the MI355X-native CubeZ hot path (libczhip_f32.so / libczhip_f64.so).
 *
 * Part 1 is the DROP-IN BOUNDARY: the same `extern "C" void name_(...)` symbols, argument order and
 * by-pointer conventions as the reference's Fortran interface, /root/reference/src/cz_cpp/cz_Ffunc.h:16-578
 * (the lines are cited per prototype).  The only change of contract: every 3-D array argument is a
 * DEVICE pointer obtained from czhip_alloc_s3d() (the replacement of czAllocR_S3D, cz.h:209-232);
 * sz/idx/g/cf/nID and all scalars stay HOST pointers, `res`/`flop` stay host in/out accumulators,
 * the dot results stay host outputs.  Every part-1 call is complete (results visible on the host and
 * in device memory) when it returns, like the Fortran it replaces.
 *
 * Part 2 is the runtime the reference does not need on a CPU (device selection, allocation, copies).
 *
 * Part 3 is the asynchronous, device-resident form of the same operations that the restated solver
 * loops (part 4, replacing CZ::JACOBI / RBSOR / PBiCGSTAB of cz_Poisson.cpp) are built from: no host
 * round trip per sweep, residual history and convergence flag kept on the device.
 *
 * Precision is a build-time switch exactly as in the reference (cz_Define.h:28-37,
 * -D_REAL_IS_DOUBLE_): the f32 and f64 libraries export the same symbol names.
 *
 * Memory layout of every 3-D array (cz_solver.f90:29): dense (NK+2g, NI+2g, NJ+2g), K fastest,
 * lower bound 1-g; linear index of 1-based (k,i,j) = (k+g-1) + (i+g-1)*(NK+2g) + (j+g-1)*(NK+2g)*(NI+2g).
 */
#ifndef CZ_HIP_H_
#define CZ_HIP_H_

#include <stddef.h>

#ifdef CZ_REAL_IS_DOUBLE
typedef double CZ_REAL;
#else
typedef float CZ_REAL;
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * Part 1 -- drop-in kernels (replace cz_solver.f90 / cz_blas.f90 behind cz_Ffunc.h)
 * ---------------------------------------------------------------------------------------------- */

/* cz_Ffunc.h:20-25  <- cz_solver.f90:22-191.  Dirichlet faces where nID[face] < 0. */
void bc_k_(int* sz, int* g, CZ_REAL* p, CZ_REAL* dh, CZ_REAL* org, int* nID);

/* cz_Ffunc.h:27-36  <- cz_solver.f90:284-387.  One relaxed-Jacobi sweep; result in p AND wk2 (inner box),
 * *res += sum dp^2, *flop += 18*npts. */
void jacobi_(CZ_REAL* p, int* sz, int* idx, int* g, CZ_REAL* cf, CZ_REAL* omg, CZ_REAL* b, double* res,
             CZ_REAL* wk2, double* flop);

/* cz_Ffunc.h:48-58  <- cz_solver.f90:404-493.  One colour of red-black SOR, in place. */
void psor2sma_core_(CZ_REAL* p, int* sz, int* idx, int* g, CZ_REAL* cf, int* ip, int* color, CZ_REAL* omg,
                    CZ_REAL* b, double* res, double* flop);

/* cz_Ffunc.h:448-450 <- cz_blas.f90:112-149 (whole array incl. guide cells) */
void blas_clear_(CZ_REAL* x, int* sz, int* g);
/* cz_Ffunc.h:452-455 <- cz_blas.f90:159-195 */
void blas_copy_(CZ_REAL* dst, CZ_REAL* src, int* sz, int* g);
/* cz_Ffunc.h:463-470 <- cz_blas.f90:255-308   z = a*x + y */
void blas_triad_(CZ_REAL* z, CZ_REAL* x, CZ_REAL* y, CZ_REAL* a, int* sz, int* idx, int* g, double* flop);
/* cz_Ffunc.h:472-477 <- cz_blas.f90:320-373   *r = sum p*p  (r overwritten) */
void blas_dot1_(CZ_REAL* r, CZ_REAL* p, int* sz, int* idx, int* g, double* flop);
/* cz_Ffunc.h:479-485 <- cz_blas.f90:386-437   *r = sum p*q */
void blas_dot2_(CZ_REAL* r, CZ_REAL* p, CZ_REAL* q, int* sz, int* idx, int* g, double* flop);
/* cz_Ffunc.h:487-495 <- cz_blas.f90:452-502   p = r + beta*(p - omg*q) */
void blas_bicg_1_(CZ_REAL* p, CZ_REAL* r, CZ_REAL* q, CZ_REAL* beta, CZ_REAL* omg, int* sz, int* idx, int* g,
                  double* flop);
/* cz_Ffunc.h:497-505 <- cz_blas.f90:517-566   z = a*x + b*y + z */
void blas_bicg_2_(CZ_REAL* z, CZ_REAL* x, CZ_REAL* y, CZ_REAL* a, CZ_REAL* b, int* sz, int* idx, int* g,
                  double* flop);
/* cz_Ffunc.h:507-513 <- cz_blas.f90:579-644   ap = ss - dd*p */
void blas_calc_ax_(CZ_REAL* ap, CZ_REAL* p, int* sz, int* idx, int* g, CZ_REAL* cf, double* flop);
/* cz_Ffunc.h:515-522 <- cz_blas.f90:658-723   r = b - (ss - dd*p) */
void blas_calc_rk_(CZ_REAL* r, CZ_REAL* p, CZ_REAL* b, int* sz, int* idx, int* g, CZ_REAL* cf, double* flop);

/* MAF flavour: the same solvers on the metric-form Laplacian whose weights are recomputed per
 * point from 1-D coordinate arrays.  X, Y, Z (length N+4, Fortran X(-1:sz+2)) and tmp are HOST arrays exactly as in
 * the reference (cz_Evaluate.cpp:342-363 fills them on the host); p, b, wk2, pvt, r, ap are device arrays. */
/* cz_Ffunc.h:170-182 <- cz_maf.f90:131-285 */
void jacobi_maf_(CZ_REAL* p, int* sz, int* idx, int* g, CZ_REAL* X, CZ_REAL* Y, CZ_REAL* Z, CZ_REAL* omg, CZ_REAL* b, double* res,
                 CZ_REAL* wk2, CZ_REAL* tmp, double* flop);
/* cz_Ffunc.h:196-209 <- cz_maf.f90:301-438 */
void psor2sma_core_maf_(CZ_REAL* p, int* sz, int* idx, int* g, CZ_REAL* X, CZ_REAL* Y, CZ_REAL* Z, int* ip, int* color,
                        CZ_REAL* omg, CZ_REAL* b, double* res, CZ_REAL* tmp, double* flop);
/* cz_Ffunc.h:524-534 <- cz_blas.f90:738-832   r = (b + dd*p - sum w*p_nb) * pvt */
void calc_rk_maf_(CZ_REAL* r, CZ_REAL* p, CZ_REAL* b, int* sz, int* idx, int* g, CZ_REAL* X, CZ_REAL* Y, CZ_REAL* Z,
                  CZ_REAL* pvt, double* flop);
/* cz_Ffunc.h:536-545 <- cz_blas.f90:845-934   ap = (sum w*p_nb - dd*p) * pvt */
void calc_ax_maf_(CZ_REAL* ap, CZ_REAL* p, int* sz, int* idx, int* g, CZ_REAL* X, CZ_REAL* Y, CZ_REAL* Z, CZ_REAL* pvt,
                  double* flop);
/* Lexicographic point SOR.  Semantics = ONE thread of the reference (its PARALLEL DO makes the result
 * depend on the thread count); computed as a two-level hyperplane wavefront, bit-identical to the sequential loop. */
/* cz_Ffunc.h:38-46 <- cz_solver.f90:207-269 */
void psor_(CZ_REAL* p, int* sz, int* idx, int* g, CZ_REAL* cf, CZ_REAL* omg, CZ_REAL* b, double* res, double* flop);
/* cz_Ffunc.h:184-194 <- cz_maf.f90:23-112 */
void psor_maf_(CZ_REAL* p, int* sz, int* idx, int* g, CZ_REAL* X, CZ_REAL* Y, CZ_REAL* Z, CZ_REAL* omg, CZ_REAL* b, double* res,
               double* flop);
/* cz_Ffunc.h:547-553 <- cz_blas.f90:947-1039  pvt = 1 / max |row entries| */
void search_pivot_(CZ_REAL* pvt, int* sz, int* idx, int* g, CZ_REAL* X, CZ_REAL* Y, CZ_REAL* Z);

/* Line SOR by parallel cyclic reduction.  x, msk, rhs are device arrays; the six work arrays are
 * the reference's host scratch and are ignored (the line systems live in LDS).  Semantics = the reference's serial build
 * (its OpenMP form reads uninitialised private work arrays, see oracle/Makefile). */
/* cz_Ffunc.h:60-77 <- cz_solver.f90:497-662 */
void pcr_rb_(int* sz, int* idx, int* g, int* pn, int* ofst, int* color, CZ_REAL* x, CZ_REAL* msk, CZ_REAL* rhs, CZ_REAL* a,
             CZ_REAL* c, CZ_REAL* d, CZ_REAL* a1, CZ_REAL* c1, CZ_REAL* d1, CZ_REAL* omg, double* res, double* flop);
/* The other line-SOR variants: pn-2 PCR stages + 4x4 systems by Cramer's rule (pcr, pcr_esa, pcr_rb_esa) or pn-1 stages + 2x2
 * systems (pcr_j_esa); columns in lexicographic order in place (pcr, pcr_esa: computed diagonal by diagonal, bit-identical to
 * the sequential loop), one colour in place (pcr_rb_esa), or all from the old field through wrk (pcr_j_esa).  The work arrays
 * (a..d1, src) are the reference's scratch and are ignored; entries beyond a line are zeros ("ESA" semantics, also where the
 * reference indexes past its arrays, i.e. when n < 3/4 * 2^pn). */
/* cz_Ffunc.h:99-114 <- cz_solver.f90:666-878 */
void pcr_(int* sz, int* idx, int* g, int* pn, CZ_REAL* x, CZ_REAL* msk, CZ_REAL* rhs, CZ_REAL* a, CZ_REAL* c, CZ_REAL* d, CZ_REAL* a1,
          CZ_REAL* c1, CZ_REAL* d1, CZ_REAL* omg, double* res, double* flop);
/* cz_Ffunc.h:116-128 <- cz_solver.f90:883-1045 (lexicographic, pn-1 stages + 2x2 systems; its un-refreshed a(kst), c(ked) are +-0.0: fresh
 * zeros here, see oracle/cz_oracle.c) */
void pcr_eda_(int* sz, int* idx, int* g, int* pn, CZ_REAL* x, CZ_REAL* msk, CZ_REAL* rhs, CZ_REAL* a1, CZ_REAL* c1, CZ_REAL* d1, CZ_REAL* omg,
              double* res, double* flop);
/* cz_Ffunc.h:130-146 <- cz_solver.f90:1050-1257 */
void pcr_esa_(int* sz, int* idx, int* g, int* pn, int* s, CZ_REAL* x, CZ_REAL* msk, CZ_REAL* rhs, CZ_REAL* a, CZ_REAL* c, CZ_REAL* d,
              CZ_REAL* a1, CZ_REAL* c1, CZ_REAL* d1, CZ_REAL* omg, double* res, double* flop);
/* cz_Ffunc.h:79-97 <- cz_solver.f90:1261-1469 */
void pcr_rb_esa_(int* sz, int* idx, int* g, int* pn, int* ofst, int* color, int* s, CZ_REAL* x, CZ_REAL* msk, CZ_REAL* rhs, CZ_REAL* a,
                 CZ_REAL* c, CZ_REAL* d, CZ_REAL* a1, CZ_REAL* c1, CZ_REAL* d1, CZ_REAL* omg, double* res, double* flop);
/* cz_Ffunc.h:148-166 <- cz_solver.f90:1473-1676 */
void pcr_j_esa_(int* sz, int* idx, int* g, int* pn, int* s, CZ_REAL* x, CZ_REAL* msk, CZ_REAL* rhs, CZ_REAL* a, CZ_REAL* c, CZ_REAL* d,
                CZ_REAL* a1, CZ_REAL* c1, CZ_REAL* d1, CZ_REAL* src, CZ_REAL* wrk, CZ_REAL* omg, double* res, double* flop);
/* The MAF line solvers (cz_Ffunc.h:211-315 <- cz_maf.f90:442-1560): the tridiagonal coefficients come from the metrics of the 1-D
 * grids XX, YY, ZZ (host arrays as in jacobi_maf_), pn-1 PCR stages + 2x2 systems; one colour (pcr_rb_maf_, pcr_rb_esa_maf_) or
 * lexicographic order (pcr_maf_, pcr_eda_maf_, pcr_esa_maf_; computed diagonal by diagonal).  Work arrays and tmp are ignored. */
void pcr_rb_maf_(int* sz, int* idx, int* g, int* pn, int* ofst, int* color, CZ_REAL* x, CZ_REAL* msk, CZ_REAL* rhs, CZ_REAL* XX, CZ_REAL* YY,
                 CZ_REAL* ZZ, CZ_REAL* a, CZ_REAL* c, CZ_REAL* d, CZ_REAL* aw, CZ_REAL* cw, CZ_REAL* dw, CZ_REAL* omg, double* res, CZ_REAL* tmp,
                 double* flop);
void pcr_rb_esa_maf_(int* sz, int* idx, int* g, int* pn, int* ofst, int* color, int* s, CZ_REAL* x, CZ_REAL* msk, CZ_REAL* rhs, CZ_REAL* XX,
                     CZ_REAL* YY, CZ_REAL* ZZ, CZ_REAL* a, CZ_REAL* c, CZ_REAL* d, CZ_REAL* aw, CZ_REAL* cw, CZ_REAL* dw, CZ_REAL* omg, double* res,
                     CZ_REAL* tmp, double* flop);
void pcr_maf_(int* sz, int* idx, int* g, int* pn, CZ_REAL* x, CZ_REAL* msk, CZ_REAL* rhs, CZ_REAL* XX, CZ_REAL* YY, CZ_REAL* ZZ, CZ_REAL* a,
              CZ_REAL* c, CZ_REAL* d, CZ_REAL* aw, CZ_REAL* cw, CZ_REAL* dw, CZ_REAL* omg, double* res, CZ_REAL* tmp, double* flop);
void pcr_eda_maf_(int* sz, int* idx, int* g, int* pn, CZ_REAL* x, CZ_REAL* msk, CZ_REAL* rhs, CZ_REAL* XX, CZ_REAL* YY, CZ_REAL* ZZ, CZ_REAL* aw,
                  CZ_REAL* cw, CZ_REAL* dw, CZ_REAL* omg, double* res, CZ_REAL* tmp, double* flop);
void pcr_esa_maf_(int* sz, int* idx, int* g, int* pn, int* s, CZ_REAL* x, CZ_REAL* msk, CZ_REAL* rhs, CZ_REAL* XX, CZ_REAL* YY, CZ_REAL* ZZ,
                  CZ_REAL* a, CZ_REAL* c, CZ_REAL* d, CZ_REAL* aw, CZ_REAL* cw, CZ_REAL* dw, CZ_REAL* omg, double* res, CZ_REAL* tmp, double* flop);
/* cz_Ffunc.h:440-443 <- cz_blas.f90:24-104 */
void imask_k_(CZ_REAL* x, int* sz, int* idx, int* g);

/* ------------------------------------------------------------------------------------------------
 * Part 2 -- runtime
 * ---------------------------------------------------------------------------------------------- */
int czhip_real_bytes(void);              /* 4 or 8: which precision this library was built for */
const char* czhip_arch(void);            /* "gfx950" */
int czhip_init(int device);              /* bind the calling process to one GPU, create streams/workspace; 0 = ok.
                                            Any HIP failure anywhere prints a message and exit(1)s: the
                                            reference ABI has no error channel. */
void czhip_finalize(void);
CZ_REAL* czhip_alloc_s3d(const int* sz); /* czAllocR_S3D (cz.h:209-232): (NI+4)(NJ+4)(NK+4) zero-filled, on the device */
void czhip_free(void* dptr);
void czhip_h2d(void* dst_dev, const void* src_host, size_t bytes); /* synchronous */
void czhip_d2h(void* dst_host, const void* src_dev, size_t bytes); /* synchronous (drains the compute stream first) */
void czhip_sync(void);                   /* drain all library streams */
void* czhip_stream(void);                /* the hipStream_t every kernel of this library is launched on */

/* Tuning of the stencil kernels (threads per block, vectors per thread, planes per j-chunk, prefetch
 * depth).  0 keeps the current value.  Returns 0 if that instantiation exists. */
int czhip_set_tuning(int threads, int vec_per_thread, int planes_per_chunk, int prefetch);
void czhip_get_tuning(int* threads, int* vec_per_thread, int* planes_per_chunk, int* prefetch);

/* Per-launch HIP-event timing on the library's stream (bench.py's roofline leg): enable(1) starts a fresh
 * collection, enable(0) stops it; czhip_timing_read returns the number of launches recorded under `label`
 * ("jacobi", "rbsor", "calc_ax", "calc_rk", "reduce", "ewise", "dot") and their summed duration in ms. */
void czhip_timing(int enable);
int czhip_timing_read(const char* label, double* total_ms);

/* ------------------------------------------------------------------------------------------------
 * Part 3 -- asynchronous device-resident operations (stream-ordered, no host synchronisation)
 * ---------------------------------------------------------------------------------------------- */

/* One Jacobi sweep p_in -> p_out (ping-pong; p_out's non-inner elements are left untouched), sum dp^2
 * accumulated in double into res_dev[0] (device) when `accumulate` != 0, else stored.  If skip_flag_dev
 * is non-NULL and *skip_flag_dev != 0 on the device the sweep is a no-op (convergence reached earlier). */
void czhip_jacobi_async(const CZ_REAL* p_in, CZ_REAL* p_out, const CZ_REAL* b, const int* sz, const int* idx, int g,
                        const CZ_REAL* cf, CZ_REAL omg, double* res_dev, int accumulate, const int* skip_flag_dev);

/* One colour of RB-SOR in place; parity: points with (i+j+k+ofst+color) even relative to kst as in
 * cz_solver.f90:466. */
void czhip_rbsor_async(CZ_REAL* p, const CZ_REAL* b, const int* sz, const int* idx, int g, const CZ_REAL* cf,
                       int ofst, int color, CZ_REAL omg, double* res_dev, int accumulate, const int* skip_flag_dev);

/* The same sweeps with the convergence bookkeeping of czhip_check_async folded into the sweep kernel (performed by
 * its last workgroup): one launch per Jacobi iteration, two per RB-SOR iteration (pass the check arguments with the
 * second colour, accumulate = 1).  flag_dev doubles as the skip flag. */
void czhip_jacobi_checked_async(const CZ_REAL* p_in, CZ_REAL* p_out, const CZ_REAL* b, const int* sz, const int* idx, int g,
                                const CZ_REAL* cf, CZ_REAL omg, double* res_dev, double res_normal, double eps, int itr,
                                double* hist_dev, int* flag_dev, int* conv_itr_dev);
void czhip_rbsor_checked_async(CZ_REAL* p, const CZ_REAL* b, const int* sz, const int* idx, int g, const CZ_REAL* cf,
                               int ofst, int color, CZ_REAL omg, double* res_dev, int accumulate, double res_normal,
                               double eps, int itr, double* hist_dev, int* flag_dev, int* conv_itr_dev);

/* TWO Jacobi sweeps per pass over memory (temporal blocking; single-domain, g >= 2): u -> w = two applications of
 * cz_solver.f90:334-351, bit-identical to two czhip_jacobi_async calls, the intermediate field never leaves the chip.
 * res_dev[0] / res_dev[1] = sum dp^2 of the first / second sweep.  hist_dev != NULL adds the convergence bookkeeping for
 * iterations itr and itr+1 (in order; flag_dev doubles as skip flag).  If the FIRST sweep converges, flag is set with
 * conv_itr = itr and w holds time n+2: the caller re-runs one single sweep from u (never modified).  Returns 1 when
 * launched, 0 when the geometry is unsupported (caller falls back to single sweeps).
 * idx1 (NULL = idx): index range of the FIRST sweep; a decomposed run grows it by one layer across rank-internal faces
 * (the second sweep reads the first one's result on the ghost layer; two ghost layers are exchanged per pair).
 * skip_flag_dev is used when hist_dev is NULL (multi-rank runs do the bookkeeping after the all-reduce). */
int czhip_jacobi2_async(const CZ_REAL* u, CZ_REAL* w, const CZ_REAL* b, const int* sz, const int* idx, const int* idx1, int g,
                        const CZ_REAL* cf, CZ_REAL omg, double* res_dev, double res_normal, double eps, int itr, double* hist_dev,
                        int* flag_dev, int* conv_itr_dev, const int* skip_flag_dev);
/* One complete red-black SOR iteration (colour 0 then colour 1, cz_Poisson.cpp:205-209) in ONE pass over memory,
 * u -> w out of place (the caller ping-pongs like Jacobi): bit-identical to psor2sma_core_ colour 0 + colour 1.
 * res_dev[0] = the iteration's sum dp^2 over both colours; check arguments as above (one iteration). */
int czhip_rbsor2_async(const CZ_REAL* u, CZ_REAL* w, const CZ_REAL* b, const int* sz, const int* idx, const int* idx1, int g,
                       const CZ_REAL* cf, int ofst, CZ_REAL omg, double* res_dev, double res_normal, double eps, int itr,
                       double* hist_dev, int* flag_dev, int* conv_itr_dev, const int* skip_flag_dev);
/* TWO red-black SOR iterations (colour 0, 1, 0, 1: cz_Poisson.cpp:205-209 twice) in ONE pass over memory, u -> w out of place (single-domain
 * boxes, constant coefficients): bit-identical to four psor2sma_core_ calls.  res_dev[0], res_dev[1] = the sums dp^2 of iteration itr and
 * itr + 1; check arguments as for czhip_jacobi2_async (two iterations; a converged first iteration leaves conv_itr = itr and the caller
 * recomputes that iteration from u).  probe != 0: only says whether the launch would be taken.  Returns 0 when it is not (the caller then runs
 * czhip_rbsor2_async twice). */
int czhip_rbsor4_async(const CZ_REAL* u, CZ_REAL* w, const CZ_REAL* b, const int* sz, const int* idx, int g, const CZ_REAL* cf, int ofst,
                       CZ_REAL omg, double* res_dev, double res_normal, double eps, int itr, double* hist_dev, int* flag_dev,
                       int* conv_itr_dev, const int* skip_flag_dev, int probe);
/* ... its switches (measurements; negative = keep): 0 off / 1 on / 2 on also for small grids (where the preloaded one-iteration pass is faster
 * and 1 leaves the box to it), vectors per k window, planes per chunk (0 = chosen per launch) */
int czhip_set_rb4(int enable, int window, int planes);
/* THREE relaxed-Jacobi sweeps in ONE pass over memory, u -> w out of place (single-domain boxes, constant coefficients): bit-identical to three
 * czhip_jacobi_async sweeps.  res_dev[0..2] = the sums dp^2 of sweeps itr, itr + 1, itr + 2; check arguments as for czhip_jacobi2_async (three
 * sweeps in order; a converged first or second sweep leaves conv_itr = itr or itr + 1 and the caller recomputes that sweep, or that pair, from
 * u).  probe != 0: only says whether the launch would be taken.  Returns 0 when it is not (the caller then runs czhip_jacobi2_async). */
int czhip_jacobi3_async(const CZ_REAL* u, CZ_REAL* w, const CZ_REAL* b, const int* sz, const int* idx, int g, const CZ_REAL* cf, CZ_REAL omg,
                        double* res_dev, double res_normal, double eps, int itr, double* hist_dev, int* flag_dev, int* conv_itr_dev,
                        const int* skip_flag_dev, int probe);
/* ... its switches (measurements; negative = keep): 0 off / 1 on above the size gate / 2 on also for small grids (tests), vectors per k window,
 * planes per chunk (0 = chosen per launch).  czhip_set_tuning2 with enable 0 (single sweeps) turns it off as well. */
int czhip_set_jac3(int enable, int window, int planes);
/* FOUR relaxed-Jacobi sweeps in ONE pass over memory (FP32; the FP64 library answers 0), u -> w out of place, for the boxes czhip_jacobi3_async
 * takes: bit-identical to four czhip_jacobi_async sweeps.  res_dev[0..3] = the sums dp^2 of sweeps itr .. itr + 3; check arguments as for
 * czhip_jacobi3_async (four sweeps in order; a converged first, second or third sweep leaves conv_itr = itr, itr + 1 or itr + 2 and the caller
 * recomputes that sweep, pair or triple from u).  probe != 0: only says whether the launch would be taken.  Returns 0 when it is not (the
 * caller then runs czhip_jacobi3_async). */
int czhip_jacobi4_async(const CZ_REAL* u, CZ_REAL* w, const CZ_REAL* b, const int* sz, const int* idx, int g, const CZ_REAL* cf, CZ_REAL omg,
                        double* res_dev, double res_normal, double eps, int itr, double* hist_dev, int* flag_dev, int* conv_itr_dev,
                        const int* skip_flag_dev, int probe);
/* ... its switches (negative = keep): 0 off / 1 on above the size gate / 2 on also for small grids (tests), vectors per k window, planes per
 * chunk (0 = chosen per launch).  Off whenever czhip_set_jac3 is off. */
int czhip_set_jac4(int enable, int window, int planes);
/* ... and the fewest sweeps of a solve (its ItrMax) for which the driver takes four-sweep passes: 8 at enable = 1 (two quads; a shorter
 * solve keeps its three-sweep passes), 4 at enable = 2 */
int czhip_jac4_min_sweeps(void);
/* ... and the geometry it plans for a box under the switches in force: out[0..7] = vectors per row of a workgroup's view, own vectors per
 * segment, k windows per row, vectors a window owns (whole rows: the row length), row segments per window, planes per chunk, chunks, LDS
 * bytes.  Returns 0 where the pass does not take the box. */
int czhip_jac4_plan(const CZ_REAL* u, CZ_REAL* w, const CZ_REAL* b, const int* sz, const int* idx, int g, const CZ_REAL* cf, CZ_REAL omg, int* out);
/* ... FP32: its division by the diagonal with one correction step instead of two, for a divisor whose quotients were compared with the IEEE
 * division for all 2^32 numerators on this context (once per divisor, at the first launch) and agreed in every bit; others keep the hoisted
 * form.  1 = on (default), 0 = off, negative = keep.  Returns the previous setting.  Results do not depend on it. */
int czhip_set_jac3_medium(int enable);
/* ... its division in the gated form: whether a numerator is so large that the division scales the divisor (|n| >= 2^(exponent(d) + 96), + 768 in
 * FP64) is tested once per vector and wave, and where none is the quotient is formed without that case.  Taken for a divisor whose gated
 * quotients were compared with the IEEE division on this context (once per divisor, at the first launch) and agreed in every bit.  1 = on
 * (default), 0 = off, negative = keep.  Returns the previous setting.  Results do not depend on it, with one exception: a residual sum over a
 * field that holds NaNs of several payloads is NaN either way, but its payload and sign may differ (the two forms are compiled apart, and
 * which NaN an addition hands on depends on its operand order).  Fields keep every bit, NaN payloads included. */
int czhip_set_jac3_gate(int enable);
/* ... whether that pass takes the gated form for divisor d on this context now: 1 yes, 0 no, -1 = the pass does not take d (it runs the
 * comparison where it is due, like the first launch). */
int czhip_jac3_gated(CZ_REAL d);
/* ... the division that pass takes for divisor d on this context: 1 = the shorter form, 0 = the hoisted form, -1 = the pass does not take d
 * (it runs the comparison where it is due, like the first launch). */
int czhip_jac3_division(CZ_REAL d);
/* The fused pass split the way a decomposed brick runs it (replaces the reference's "sweep, then Comm_S",
 * cz_Poisson.cpp:58-63): first the slabs two cells thick behind every face with nID[f] >= 0 (the cells the neighbours
 * receive), then the interior, so that the exchange can start after the first launch.  Same result as the unsplit op.
 * rb_ofst < 0: two Jacobi sweeps, res_dev[0..1]; rb_ofst >= 0: one red-black iteration (ofst), res_dev[0].
 * Returns 0 (nothing launched) when there is no internal face, the box is too thin or the geometry is unsupported. */
int czhip_pair_split_async(const CZ_REAL* u, CZ_REAL* w, const CZ_REAL* b, const int* sz, const int* idx, const int* idx1,
                           const int* nID, int g, const CZ_REAL* cf, CZ_REAL omg, int rb_ofst, double* res_dev);
/* First pair of a preconditioner solve whose start vector is identically zero (blas_clear_ + 8 sweeps, cz_Poisson.cpp:405-409):
 * u is neither cleared in memory nor read; u_shape only provides the array geometry/alignment.  Bit-identical to clearing u and
 * calling czhip_jacobi2_async. */
int czhip_jacobi2_from_zero_async(const CZ_REAL* u_shape, CZ_REAL* w, const CZ_REAL* b, const int* sz, const int* idx, const int* idx1,
                                  int g, const CZ_REAL* cf, CZ_REAL omg, double* res_dev);
/* The same with the right-hand side of the solve MADE on the way from the operands of the vector update that precedes a preconditioner
 * solve in BiCGSTAB -- op 1: b = a*x + y (blas_triad_, cz_blas.f90:297), op 2: b = x + a*(z - bb*y) (blas_bicg_1_, :490) -- and stored
 * to b_out (not one of x, y, z) for the later passes of the solve: update and first pass in one launch, same bits as the two calls.
 * op 0: b_out is read as the right-hand side.  rb_ofst < 0: two Jacobi sweeps (czhip_jacobi2_async); >= 0: one red-black iteration with
 * that colour offset (czhip_rbsor2_async).  probe != 0: only says whether the launch would be taken. */
int czhip_jacobi2_from_zero_made_async(const CZ_REAL* u_shape, CZ_REAL* w, CZ_REAL* b_out, int op, const CZ_REAL* x, const CZ_REAL* y,
                                       const CZ_REAL* z, CZ_REAL a, CZ_REAL bb, const int* sz, const int* idx, const int* idx1, int g,
                                       const CZ_REAL* cf, CZ_REAL omg, int rb_ofst, double* res_dev, int probe);
/* The same bookkeeping for a pair whose two sums were all-reduced first (decomposed runs).  Here and in every checked pass of several
 * iterations the bookkeeping stops at the first converged iteration: hist entries of the later iterations of the pass are not written. */
void czhip_check2_async(const double* res_dev, double res_normal, double eps, int itr, double* hist_dev, int* flag_dev,
                        int* conv_itr_dev);
/* The MAF flavour of the two calls above (cz_maf.f90:131-438): weights recomputed at every point from the host coordinate arrays X, Y, Z
 * (as in jacobi_maf_ / psor2sma_core_maf_).  rb_ofst < 0: two jacobi_maf sweeps, res_dev[0..1]; rb_ofst >= 0: one red-black iteration with
 * that ofst, res_dev[0].  Returns 1 if launched. */
int czhip_pair_maf_async(const CZ_REAL* u, CZ_REAL* w, const CZ_REAL* b, const int* sz, const int* idx, int g, const CZ_REAL* X,
                         const CZ_REAL* Y, const CZ_REAL* Z, CZ_REAL omg, int rb_ofst, double* res_dev);
/* Shape of the two-stage pass: threads per workgroup (512 | 1024; 0 / -1 keep, -2 = chosen per launch by the balance model), vectors per
 * thread (2), planes per chunk (0 = chosen per launch, -1 keep), enable (-1 keep).  Returns 0 if ok.  Every shape gives the same bits. */
int czhip_set_tuning2(int threads, int vec_per_thread, int planes_per_chunk, int enable);
/* line-SOR kernels (pcr*_): form 0 = one wave per line with the reference's arithmetic literally (a, c and d of the line reduced in LDS; every
 * variant but pcr_j_esa_; also the fall-back for lines whose coefficient table does not fit LDS), 1 = coefficient
 * table + right-hand side in LDS, 2 = table + right-hand side in registers (default); variant (form 1 only; form 2 has one measured shape per
 * case since round 3) = waves*10 + lines per wave, 0 = default; negative = keep.  All forms give the same bits. */
int czhip_set_pcr_mode(int form, int variant);
/* the lexicographic line SOR (pcr_, pcr_esa_, pcr_eda_; reference: cz_solver.f90:666-878, one thread walking j, i): one_launch 1 = the whole
 * sweep in one launch, rows of lines handed from workgroup to workgroup (default), 0 = one launch per diagonal i+j; groups of threads per
 * workgroup (0 = chosen per launch); rows per thread (1 | 2).  Negative = keep.  Every shape gives the same bits. */
int czhip_set_pcr_lex(int one_launch, int groups, int rows_per_thread);
/* Bound, in seconds, of every wait of one workgroup for another inside the one-launch sweep (default 2; negative = keep); returns the bound in
 * force.  If a wait runs out, every workgroup leaves and the residual of that sweep is NaN. */
double czhip_set_pcr_lex_timeout(double seconds);
/* the lexicographic point SOR (psor_, psor_maf_; reference: cz_solver.f90:207-269, one thread walking j, i, k): one_launch 1 = the whole sweep
 * in one launch (default), 0 = one launch per tile hyperplane; workgroups per CU of the former (0 = chosen by the launcher).  Negative = keep.
 * Same bits either way; the waits of the one-launch form are bounded by czhip_set_pcr_lex_timeout, a lost hand-off gives a NaN residual. */
int czhip_set_psor(int one_launch, int wg_per_cu);
/* ... and how many steps ahead of their use a column asks for the face values of the columns before it (4 | 8; 0 = chosen per launch).  Returns
 * the previous setting.  Measurement aid; same bits either way. */
int czhip_set_psor_ahead(int steps);
/* Launch limits of the one-launch sweep (test aid; negative = keep, 0 = chosen per launch): workgroups per CU, workgroups in all, lines per
 * hand-off ring between two rows (rounded up to a power of two).  The launcher's own ring size lets the sweep finish however few of its
 * workgroups the device keeps resident; a ring forced small with few workgroups cannot, and the sweep then ends as described above. */
int czhip_set_pcr_lex_limits(int wg_per_cu, int max_wg, int slots);
int czhip_use_t2(void);
/* The two-stage pass cuts long k rows into windows (a workgroup's LDS holds whole rows of its window only; cz_solver.f90:284-387 takes any
 * extent, and so does the pass since round 4): vectors (16 bytes) per window; 0 = whole rows wherever they fit, -1 = chosen per launch (default),
 * <= -2 = keep.  Returns the previous setting.  Results do not depend on it. */
int czhip_set_pair_window(int vectors);
/* Order in which the workgroups of the multi-stage passes (two-sweep, two-iteration red-black and three-sweep) take their (segment, chunk)
 * items, by XCD: 0 = whole-segment bands, 1 = equal shares where bands would idle and row bands of every k window (default), 2 = equal shares
 * where bands would idle, window-major (CZHIP_T2_MAP); negative = keep.  Returns the previous setting.  Results do not depend on it. */
int czhip_set_pair_map(int order);
/* Small grids (every workgroup of a pass resident at once): the pass requests all operands of a chunk before its first plane step instead of one
 * plane ahead; 1 = on (default), 0 = off, negative = keep.  Returns the previous setting.  Results do not depend on it. */
int czhip_set_pair_preload(int enable);
/* The reference's coefficients are c1 .. c6 = 1, dd = 6 (cz.h:169-172): where the six are exactly 1 the Jacobi pass and the two-iteration red-black
 * pass take a form without the six multiplications (x * 1 is x: same sum, same order).  1 = on (default), 0 = always the general form, negative =
 * keep.  Returns the previous setting.  Results do not depend on it. */
int czhip_set_unit_coef(int enable);
/* Every environment variable the library and the cz command line read (one table, cubez_amd/csrc/cz_config.h), one per line: NAME=value where set,
 * NAME (unset; default ...) otherwise; only_set != 0 lists the former only.  The string lives until the next call on the calling thread. */
const char* czhip_config_describe(int only_set);
/* What czhip_init and the setters made of the kernel switches: the calling thread's tuning (threads, m, tj, pf, fuse_fin, use_t2, t2_threads,
 * t2_mv, t2_tj, t2_map, t2_any_rows, t2_kwin, t2_pre, rb4, rb4_kwin, rb4_tj, jac3, jac3_kwin, jac3_tj, jac3_medium, jac3_gate, unit_coef, pcr_fast,
 * pcr_variant, pcr_pipe, pipe_spin_ticks, pcr_rows, pcr_q, pcr_wg_per_cu, pcr_max_wg, pcr_slots, psor_col, psor_wg_per_cu, psor_ahead), num_cu
 * and cu_reserved (the CU reservation of czhip_set_comm_cus), as name=value, one per line.  ready=0: the thread's context has not started,
 * the values are the built-in defaults (the call does not start it).  Read-only; the string lives until the next call on the calling thread. */
const char* czhip_tuning_describe(void);
/* Decomposed runs keep k CUs of every XCD free of the sweeps (CZ_COMM_CUS, default 2) so that RCCL's send/recv kernels run while an interior
 * sweep fills the chip -- through the launch geometry (the launches count those CUs out).  Measurement aid: put that reservation in force by
 * hand (the driver does it itself in decomposed runs and undoes it in single-domain ones at set-up); returns the reservation in force. */
int czhip_set_comm_cus(int k);
/* self-test: numerators (of 2^32) whose quotient by d in the two-stage pass differs from the IEEE division (expected 0); -1 = divisor not eligible */
long long czhip_selftest_fastdiv(CZ_REAL d);
/* the same for the shorter form jac3_k takes where it agrees (FP32; -1 = divisor not eligible, and in FP64, which has no such form) */
long long czhip_selftest_mediumdiv(CZ_REAL d);
/* the same for the gated form of the division jac3_k takes for d now: numerators below the threshold (NaNs included) whose quotient differs
 * (expected 0); *compared = how many were compared; -1 = divisor not eligible */
long long czhip_selftest_gateddiv(CZ_REAL d, long long* compared);

/* PCG (beyond the reference; DESIGN.md "PCG"), the two passes of its iteration:
 * czhip_cg_update_async: x = alpha*p + x, r = (-alpha)*q + r on the inner box (blas_triad_ twice) and dots_dev[0] = r.r (per-point products in
 *   REAL, summed in double), one pass.  alpha_dev[0] = alpha, alpha_dev[1] = -alpha, read on the device.
 * czhip_cg_dir_ax_async: u = z + beta*p_old at every point the 7-point stencil reads, u written to the inner box of p_new, q = A u
 *   (blas_calc_ax_) and dots_dev[0] = u.q, one pass.  beta_dev: beta on the device; nullptr: u = z (p_old is not read).  Single-domain
 *   arrays only: z and p_old must be zero outside the inner box (their faces and guide cells are read as operands); p_new is not p_old. */
void czhip_cg_update_async(CZ_REAL* x, CZ_REAL* r, const CZ_REAL* p, const CZ_REAL* q, const CZ_REAL* alpha_dev, const int* sz, const int* idx, int g,
                           double* dots_dev);
void czhip_cg_dir_ax_async(CZ_REAL* p_new, CZ_REAL* q, const CZ_REAL* z, const CZ_REAL* p_old, const CZ_REAL* beta_dev, const int* sz, const int* idx,
                           int g, const CZ_REAL* cf, double* dots_dev);

/* Multigrid V-cycle preconditioner of PCG (beyond the reference): aggregation multigrid with the exact Galerkin operator.
 * Level l+1 has ceil(n/2) points per direction of level l; level l's array has its points as the inner box idx of an array sz with guide g
 * (the hierarchy's coarse arrays: sz = n + 2, idx = 2 .. n + 1, zero faces), n0 = the level-0 points per direction (the face weights
 * Wx = Ey Ez, Wy = Ex Ez, Wz = Ex Ey, D = 2 (Wx + Wy + Wz), E = min(2^l, n0 - I 2^l)).  Every entry returns 1 when launched, 0 when the
 * arrays do not describe that level (or alias where they must not).
 * czhip_mg_smooth_async: w = one relaxed Jacobi sweep of level l from u (u = NULL: from zero, u not read), pn = pp + ((ss - bb)/D - pp) omg.
 * czhip_mg_restrict_async: bc (level l+1) = the residual b - (ss - D x) of level l summed over the <= 8 children, the fine residual not
 *   stored.
 * czhip_mg_prolong_async: u = x + R(1.8 xc(parent)) on level l (u may be x), xc of level l+1.
 * czhip_mg_tail_async: x = V_l(b) from level l down to the coarsest and back in one workgroup, every level in LDS; 0 if they do not fit. */
int czhip_mg_smooth_async(const CZ_REAL* u, CZ_REAL* w, const CZ_REAL* b, const int* sz, const int* idx, int g, int level, const int* n0, CZ_REAL omg);
int czhip_mg_restrict_async(CZ_REAL* bc, const int* szc, const int* idxc, const CZ_REAL* x, const CZ_REAL* b, const int* sz, const int* idx, int g, int level,
                            const int* n0);
int czhip_mg_prolong_async(CZ_REAL* u, const CZ_REAL* x, const CZ_REAL* xc, const int* szc, const int* idxc, const int* sz, const int* idx, int g, int level,
                           const int* n0);
int czhip_mg_tail_async(CZ_REAL* x, const CZ_REAL* b, const int* sz, const int* idx, int g, int level, const int* n0, CZ_REAL omg);
/* The hierarchy of a single-domain array (sz, idx, g = 2) for the operator cf: levels down to the first whose largest extent is <= 4, the
 * coarse arrays b, x, t of every level >= 1 (about 3/7 of a fine array) and one fine temporary.  NULL (0) for coefficients other than
 * c1 .. c6 = 1, dd = 6.  czhip_mg_apply_async: z = M^-1 r = V_0(r) with relaxation coefficient omg (0 < omg <= 1), z and r arrays of sz
 * whose faces and guide cells are zero (only inner boxes are written); a level-0 box that is already the coarsest gives the 8 relaxed
 * sweeps from zero.  No reduction: the same bits on every run.  CZ_MG_TAIL=0 at create: no tail kernel (the same bits). */
typedef struct cz_mg cz_mg;
cz_mg* czhip_mg_create(const int* sz, const int* idx, int g, const CZ_REAL* cf);
int czhip_mg_levels(const cz_mg* h);
int czhip_mg_apply_async(cz_mg* h, CZ_REAL* z, const CZ_REAL* r, CZ_REAL omg);
void czhip_mg_destroy(cz_mg* h);
/* The same cycle with a symmetric red-black smoother (pcg ... mgrb): the colour of a point is (I + J + K) & 1 of its 0-based
 * indices in the level's inner box, a colour sweep updates the points of one colour in place, a forward iteration is colour 0 then 1, a backward
 * one colour 1 then 0; V_l = 2 forward iterations from zero, restrict, V_{l+1}, prolong, 2 backward iterations (the coarsest level: 4 forward from
 * zero, 4 backward).  Levels, weights, restriction and prolongation are those above.
 * czhip_mg_rb_async: one colour sweep of a whole level >= 1 in place on x; zero: 0 = from the iterate, 1 = the first colour of an iteration from
 *   zero (x is not read), 2 = its second colour (reads the other colour only).  0 at level 0: that level runs czhip_rbsor2_async /
 *   czhip_rbsor4_async / czhip_jacobi2_from_zero_made_async with ofst 0 (forward) and 1 (backward).
 * czhip_mg_tail_rb_async: czhip_mg_tail_async for this cycle (its levels keep two arrays in LDS, not three: it may start one level earlier).
 * czhip_mg_create_rb: the hierarchy of czhip_mg_create with this smoother (no temporaries on the coarse levels); czhip_mg_apply_async,
 *   czhip_mg_levels and czhip_mg_destroy serve both kinds of handle.  0 < omg <= 1.2 (the range the preconditioner was checked to be definite on).
 * czhip_mg_kind: 0 = no handle, 1 = relaxed Jacobi (czhip_mg_create), 2 = red-black (czhip_mg_create_rb). */
int czhip_mg_rb_async(CZ_REAL* x, const CZ_REAL* b, const int* sz, const int* idx, int g, int level, const int* n0, CZ_REAL omg, int colour, int zero);
int czhip_mg_tail_rb_async(CZ_REAL* x, const CZ_REAL* b, const int* sz, const int* idx, int g, int level, const int* n0, CZ_REAL omg);
cz_mg* czhip_mg_create_rb(const int* sz, const int* idx, int g, const CZ_REAL* cf);
int czhip_mg_kind(const cz_mg* h);
/* Zero-flux (Neumann) faces.  faces[6]: X-, X+, Y-, Y+, Z-, Z+, non-zero = Neumann.
 * czhip_mirror_faces_async: czhip_fill_faces_async (below) with kind 1 on every face whose flag is non-zero and kind 0 on the others; no flag
 *   means a wrap, none is refused.  On every flagged face that is a physical face of the brick (idx starts at 2 / ends at size - 1 in that direction,
 *   the inner-range convention of a brick; a rank-internal face is never touched) the face layer becomes the mirror of the first inner
 *   layer, p(1, j, k) = p(2, j, k) resp. p(size, j, k) = p(size-1, j, k), j and k over idx; edges, corners and every other cell keep their
 *   bytes.  One launch (label bc_mirror).  With that layer the kernels' own statement is the zero-flux operator at the cells next to it.
 * czhip_mg_set_neumann: the hierarchy's cycles from now on take these faces as zero-flux faces: level 0 runs single sweeps / colour sweeps with
 *   the mirror before each one that reads its input, levels >= 1 take D = Wx cx + Wy cy + Wz cz, c = 2 less one per Neumann face the point
 *   lies on (the correction is zero outside the box, the absent link needs nothing else).  All zero: the cycle of czhip_mg_create, bit for
 *   bit.  Either returns 1, or 0 when refused (a NULL pointer). */
int czhip_mirror_faces_async(CZ_REAL* p, const int* sz, const int* idx, int g, const int* faces);
int czhip_mg_set_neumann(cz_mg* h, const int* faces);
/* Periodic directions.
 * czhip_fill_faces_async: kinds[6], order X-, X+, Y-, Y+, Z-, Z+: 0 leave the face layer, 1 the mirror described at czhip_mirror_faces_async (skipped on a
 *   face that is not physical on the brick), 2 the wrap, p(1, j, k) = p(size-1, j, k) and p(size, j, k) = p(2, j, k), j and k over idx.  A
 *   wrap needs both faces of its direction to be 2 and both to be physical on the brick.  One launch for every face listed (label bc_mirror);
 *   edges, corners and every other cell keep their bytes.  It serves the level arrays of a hierarchy as well (S3D arrays, sz / idx / g).
 * czhip_mg_set_periodic: dirs[3], X, Y, Z, non-zero = periodic.  The hierarchy's cycles from now on wrap those directions: at level 0 the
 *   fill stands where the mirror stands (and does the mirrors too), at levels >= 1 the ghost layers are wrapped before every kernel that reads
 *   the iterate's neighbours, which carries the ordinary link Wx = Ey Ez across the seam; a level of ONE point in a periodic direction has no
 *   link there (both mask bits, c = 0, ghost layers zero).  The Neumann flags of a periodic direction are ignored.  All zero: the cycle
 *   of before, bit for bit.  Either returns 1, or 0 when refused (a NULL pointer; a kind other than 0, 1, 2; half a wrap; a wrap on a face
 *   that is not physical). */
int czhip_fill_faces_async(CZ_REAL* p, const int* sz, const int* idx, int g, const int* kinds);
int czhip_mg_set_periodic(cz_mg* h, const int* dirs);
/* Face coefficients inside the hierarchy.  bx, by, bz: device arrays in the layout of the hierarchy's level-0 arrays
 * (padded, guide 2), bx at a cell = the coefficient on the face towards the next cell in X, finite and positive on every face a cell of the
 * box touches, face 0 of a periodic direction holding the copy of face n - 2 (what cz_set_face_coef keeps).  The arrays stay the caller's
 * and are read by every cycle from now on: level 0 takes them as its face weights, level l + 1 the sums of the fine weights across each
 * aggregate face (the exact Galerkin product; a Neumann face and the seam of a one-point periodic level carry a zero), every level a stored
 * diagonal.  The call allocates about 1 + 4/7 of a fine array, builds under the hierarchy's boundary state (czhip_mg_set_neumann /
 * czhip_mg_set_periodic rebuild), waits for the count of coarse weights and diagonals that are not finite and positive, and returns 1
 * where there is none; else 0, and the hierarchy is the constant one again.  All three NULL: the constant hierarchy again, the arrays
 * freed, 1.  0 with nothing changed: a NULL handle, some but not all pointers NULL.  With unit coefficients the cycle gives the bits of
 * the constant cycle in every boundary state. */
int czhip_mg_set_coef(cz_mg* h, const CZ_REAL* bx, const CZ_REAL* by, const CZ_REAL* bz);
/* Zebra line iterations along Z inside the hierarchy.  on = 1: while the hierarchy holds face coefficients
 * (czhip_mg_set_coef), every pair of smoothing iterations of a red-black hierarchy runs two zebra line iterations in place of two
 * red-black point iterations: the colour of row (I, J) is (I + J) & 1, one sweep of a colour solves every row of that colour exactly along
 * K (Thomas, IEEE division) and relaxes with the cycle's coefficient, forward iterations sweep colour 0 then 1, backward ones 1 then 0.
 * An end of a row is folded into the diagonal on a zero-flux Z face of level 0; every other end reads the ghost cell, so a periodic Z is a
 * lagged wrap.  A level with one row (ni = nj = 1) keeps the point sweeps, and the one-workgroup tail is not taken.  The flag is idle while
 * the hierarchy has no coefficients.  on = 1 allocates the scratch of the backward march (two tables of the rows of one colour of the
 * largest level: about one fine array), on = 0 frees it; czhip_mg_destroy frees it too.  The cycle's coefficient must lie in (0, 1]: the
 * caller's to keep.  Returns 1, or 0 with nothing changed: a NULL handle, a Jacobi hierarchy (czhip_mg_kind 1), on other than 0 | 1.
 * czhip_mg_line_chunk: the cells of a row that the line kernel marches at a time in this precision (rows longer than that take the scratch). */
int czhip_mg_set_lines(cz_mg* h, int on);
int czhip_mg_line_chunk(void);
/* The closed box (all six faces zero-flux): the projections onto the zero-mean fields and PCG's update with one folded in.
 * czhip_shift_sums_async: a <- a - *m_dev over the inner box (one REAL subtraction per cell), then sums_dev[0] = sum a', sums_dev[1] = sum a'^2
 *   of the values a holds afterwards (REAL products accumulated in double, as czhip_cg_update_async forms r.r).  m_dev NULL: a is only read,
 *   nothing is stored.  Cells outside the inner box keep their bytes.  One launch (label shift_sums); 1, or 0 when refused (a NULL pointer).
 * czhip_cg_update_closed_async: czhip_cg_update_async with r = ((-alpha)*q + r) - sc_dev[4] (sc_dev: alpha, -alpha, -, -, m) and
 *   dots_dev[0] = r.r, dots_dev[1] = sum r of the written values (label cg_update_closed).
 * In czhip_mg_set_neumann all six faces are accepted: D = Wx cx + Wy cy + Wz cz stays positive. */
int czhip_shift_sums_async(CZ_REAL* a, const CZ_REAL* m_dev, const int* sz, const int* idx, int g, double* sums_dev);
void czhip_cg_update_closed_async(CZ_REAL* x, CZ_REAL* r, const CZ_REAL* p, const CZ_REAL* q, const CZ_REAL* sc_dev, const int* sz, const int* idx, int g,
                                  double* dots_dev);

/* Convergence bookkeeping on the device (cz_Poisson.cpp:67-77): res = sqrt(res_dev[0]*res_normal);
 * hist_dev[itr] = res; if (res < eps && !*flag) { *flag = 1; conv_itr_dev[0] = itr; }.  No-op when
 * already converged. */
void czhip_check_async(const double* res_dev, double res_normal, double eps, int itr, double* hist_dev,
                       int* flag_dev, int* conv_itr_dev);

/* ------------------------------------------------------------------------------------------------
 * Part 4 -- the restated driver (class CZ of cz.h / cz_Evaluate.cpp / cz_Poisson.cpp) behind a handle
 * ---------------------------------------------------------------------------------------------- */
typedef struct cz_handle cz_handle;

cz_handle* cz_create(void);
void cz_destroy(cz_handle*);
/* main.cpp:15-60 + CZ::Evaluate (cz_Evaluate.cpp:21-567): same argv as the reference CLI
 *   cz gsz_x gsz_y gsz_z solver ItrMax coef [precond] [gdv_x gdv_y gdv_z]
 * returns 1 on success, 0 on "Solver error" exactly like CZ::Evaluate. */
int cz_evaluate(cz_handle*, int argc, char** argv);
/* Split form used by bench.py / tests: setup (parse + allocate + boundary conditions), then solve. */
int cz_setup(cz_handle*, int argc, char** argv);
int cz_solve(cz_handle*);                      /* runs the selected solver to ItrMax / eps; returns Iter (0 = error).  Repeatable: every call
                                                  starts from the current P with the history and the counters of cz_info a fresh set-up leaves.
                                                  A Krylov breakdown returns 0 too; pcg breaks down before it updates P (cz_info 24) */
/* A caller's own problem (INTEGRATION.md "Level 3").  After cz_setup (sizes, solver, ItrMax, coefficient, preconditioner,
 * division as on the command line) the built-in test case in P and RHS is replaced by the caller's:
 *   cz_set_rhs    the right-hand side b,
 *   cz_set_field  the Dirichlet values and the initial guess,
 *   cz_get_field  the current iterate / the solution, into the caller's array,
 *   cz_set_eps    the tolerance of the residual test (> 0; 1.0e-5 after cz_setup),  cz_set_itr_max  the iteration limit (>= 1).
 * The system solved is the one the kernels state, with the unit coefficients of the command line:
 *   p[i+1] + p[i-1] + p[j+1] + p[j-1] + p[k+1] + p[k-1] - 6 p = b        at every inner cell
 * -- for the Poisson equation on a mesh of width h, b = h^2 f: scaling is the caller's business.  The MAF solvers take the entries too; their
 * grid stays the built-in one.
 * The array covers the calling rank's brick, cells 1 .. size[d] of cz_local_size, without guide cells: cell [i, j, k] (0-based) is element
 * i stride[0] + j stride[1] + k stride[2], strides in elements, any positive values -- a C-order tensor [ni][nj][nk] has strides
 * {nj nk, nk, 1}, the reference's Fortran array p[i,j,k] has {1, ni, ni nj}, a slice of a larger array keeps the larger array's strides.
 * On a physical side of the domain layer 1 / size[d] of the field is the Dirichlet face: no solver writes it.  Every other cell of
 * cz_set_field is the initial guess.  Values of b on physical faces are copied but never read: every pass reads b at the cells it updates
 * (inner cells; in a decomposed run also inner cells of the neighbour, through the ghost layer), so the solution does not depend on them.
 * After an import the ghost layers are filled from the neighbours as cz_setup does: in a decomposed run cz_set_rhs and cz_set_field are
 * collective, every rank calls them with its own brick, and needs to do nothing more.
 * on_device = 1: the pointer is memory of the handle's device, read or written in place by kernels on the library's compute stream (no copy
 * through the host).  stream is the hipStream_t on which the caller produced the data (cz_set_*) or will consume it (cz_get_field): the
 * compute stream waits for an event recorded there, and that stream waits for the kernel, so the caller neither synchronises nor has to keep
 * its hands off the array afterwards.  NULL: the data must be complete at the call, which returns when the kernel has finished.  Nothing on
 * this path waits for the whole device.  on_device = 0: host memory; the elements the strides span go through a device buffer and the same
 * kernels, and the call returns when done.  Either way cz_get_field writes the brick's cells and no other element of dst -- ranks that are
 * threads of one process may export their bricks into one shared array at the same time.
 * Return 1, or 0 with one line on stderr and nothing changed: before cz_setup, a NULL pointer, a stride < 1, a pointer that is not on the
 * handle's device, a destination under whose strides two cells share an element (accepted: ordered by stride, each stride is at least the
 * span of the directions below it -- dense arrays in any order of directions, and their slices).
 * cz_error_max keeps comparing with the analytic solution of the built-in test case. */
int cz_set_rhs(cz_handle*, const CZ_REAL* src, const long long* stride, int on_device, void* ready_stream);
int cz_set_field(cz_handle*, const CZ_REAL* src, const long long* stride, int on_device, void* ready_stream);
int cz_get_field(cz_handle*, CZ_REAL* dst, const long long* stride, int on_device, void* done_stream);
/* Mixed-precision refinement: the true residual of the iterate in the handle, and a correction into it.  The caller's brick is
 * laid out and handed over as for cz_get_field / cz_set_field, but its elements are float or double, chosen by *_real_bytes (4 | 8), whatever
 * the library's precision -- the FP64 library's residual goes out as the FP32 library's right-hand side, and that library's solution comes back.
 *   cz_get_residual  r = b - (ss - 6 p) of the current P and RHS -- the unit-coefficient operator above, with the arithmetic, the operation
 *     order and the type (CZ_REAL) of blas_calc_rk_ -- at the cells every sweep updates and 0 on physical (Dirichlet) faces, written as
 *     (T)(r * (CZ_REAL)scale): one multiplication, then one conversion (FP64 -> FP32 rounds to nearest, FP32 -> FP64 is exact).  *sumsq (a host
 *     pointer, written on return) = the sum of r^2 of the unscaled r, every square and the sum in double, over the whole domain (a decomposed
 *     run all-reduces it: the same value on every rank); its bits do not depend on the destination, and two calls give the same bits.
 *     dst = NULL: the sum only.  Collective in a decomposed run: the ghost layer of P is exchanged first.
 *   cz_add_field     P = P + (CZ_REAL)src * (CZ_REAL)scale at the cells every sweep updates -- one multiplication and one addition, each
 *     rounded once; Dirichlet faces and guide cells are not written.  Afterwards the ghost layers are filled as cz_set_field fills them.
 * Return 1, or 0 with one line on stderr and nothing changed: every case cz_get_field / cz_set_field refuse, a byte size other than 4 or 8,
 * a scale that is not finite and positive (as given and as CZ_REAL), a handle set up with a _maf solver (its operator is not the unit one). */
int cz_get_residual(cz_handle*, void* dst, int dst_real_bytes, const long long* stride, int on_device, void* done_stream, double scale, double* sumsq);
int cz_add_field(cz_handle*, const void* src, int src_real_bytes, const long long* stride, int on_device, void* ready_stream, double scale);
/* The projection step on a staggered velocity: the discrete divergence of a velocity straight into the right-hand side, and
 * the gradient of the field subtracted from the velocity in place.  Single domain only.  With the handle's solver in between,
 *   cz_set_rhs_div(h, u, v, w, ...);  cz_solve(h);  cz_sub_grad(h, u, v, w, ...);          (both at the same scale)
 * leaves a velocity whose discrete divergence is the residual of the solve: div(u - grad p) = div u - (sum of neighbours - 6 p), exactly,
 * with the face layers of cz_set_neumann (the mirror) and cz_set_periodic (the wrap) as they are.
 * The grid: the brick's cells are 1 .. n_d (n_d = size[d]), the inner cells 2 .. n_d - 1.  u, v, w are three arrays of the brick's shape that
 * share ONE stride triple, laid out and handed over as for cz_set_field (three tensors of equal layout, or the three components of one
 * vel[..., 3]).  u(i, j, k) is the normal velocity on the face between cells i and i + 1 in X, i = 1 .. n_0 - 1; entry i = n_0 is never read
 * or written; v and w are the same along j and k.  In a periodic direction cell 1 is cell n - 1 and cell n is cell 2, so face 1 is an alias
 * of face n - 1: on input face 1 is ignored and face n - 1 read in its place, on output face 1 receives the value of face n - 1.  Nothing
 * else depends on the boundary state: on a zero-flux face the wall-normal velocity u(1) or u(n - 1) is the caller's datum (0 for a wall, the
 * inflow for an inflow plane), enters the divergence like any face, and is left alone by the gradient because the mirror makes
 * p(2) - p(1) = 0; on a Dirichlet face p(1) is the given value and the face is corrected like any other.
 *   cz_set_rhs_div  at every inner cell, each operation rounded once in CZ_REAL:  dx = u(i) - u(i-1), dy = v(j) - v(j-1), dz = w(k) - w(k-1),
 *     d = (dx + dy) + dz, RHS = d * (CZ_REAL)scale; the brick's other cells of RHS get 0.  Afterwards exactly what cz_set_rhs does after its
 *     import (in closed-box mode the mean is removed and cz_closed_mean(h, 0) reports it).  *sumsq (a host pointer, written on return) = the
 *     sum of d^2 of the unscaled d over the inner cells, every square and the sum in double, the same bits from run to run.  sumsq = NULL:
 *     no sum is reported, and with a device array and a stream the call is a pure event hand-over without a host wait.
 *   cz_sub_grad     u(i, j, k) = u(i, j, k) - (p(i+1, j, k) - p(i, j, k)) * (CZ_REAL)scale for i = 1 .. n_0 - 1 and inner j, k -- one subtraction,
 *     one multiplication and one subtraction, each rounded once -- v and w the same along their directions; p is the field in the handle, its
 *     face layers re-made first as cz_get_residual does.  Faces whose tangential index lies on a boundary layer, and entry n, are not
 *     written; of a host array no element outside the brick is written.  In a periodic direction face 1 is written with the value of face n - 1.
 * Return 1, or 0 with one line on stderr and nothing changed: before cz_setup, a NULL array or stride, a stride < 1, an array that is not
 * aligned to CZ_REAL, a pointer that is not on the handle's device, a scale that is not finite and positive (as given and as CZ_REAL), a
 * handle set up with a _maf solver, a decomposed run (faces between bricks need an exchange of one velocity layer: the follow-up); for
 * cz_sub_grad also strides under which two cells of one component share an element (the rule of cz_get_field) and two components given the
 * same pointer.  Accepted on a handle of any other solver; cz_solve keeps its own rules about masks and flags. */
int cz_set_rhs_div(cz_handle*, const CZ_REAL* u, const CZ_REAL* v, const CZ_REAL* w, const long long* stride, int on_device, void* ready_stream,
                   double scale, double* sumsq);
int cz_sub_grad(cz_handle*, CZ_REAL* u, CZ_REAL* v, CZ_REAL* w, const long long* stride, int on_device, void* stream, double scale);
/* Face coefficients for pcg: the variable-density pressure solve div(beta grad p) = b, beta = dt / rho given on the faces
 * (constant bx != by != bz: grid spacings that differ by direction).  bx, by, bz are laid out and handed over exactly as u, v, w of
 * cz_set_rhs_div: three arrays of the brick's shape with ONE stride triple, bx(i, j, k) on the face between cells i and i + 1, i = 1 .. n_0 - 1;
 * entry n_0 is never read; in a periodic direction face 1 is ignored and face n - 1 read in its place; only faces at inner tangential
 * indices are read.  The values are copied into padded arrays of the handle (the caller may reuse its arrays at once; with a stream the
 * hand-over is by events), together with a scaling array s = sqrt(6 / D), D = ((bx+ + bx-) + (by+ + by-)) + (bz+ + bz-) over the six faces a
 * cell's row reads -- every operation rounded once in CZ_REAL, IEEE division and square root.  While coefficients are in force (cz_info 25):
 *   the operator is, per direction d, t_d = beta_d(c) (p(c + e_d) - p(c)) - beta_d(c - e_d) (p(c) - p(c - e_d)), A p = (t_x + t_y) + t_z, each
 *     operation rounded once, p's face layers what the handle's state makes them (Dirichlet value, mirror, wrap): a zero-flux face drops
 *     out because the mirror makes its difference 0.  With beta = 1 it is the stated system in exact arithmetic (not bit for bit);
 *   cz_solve (pcg with none | jacobi | mg | mgrb) applies it at the start and once per iteration (the direction is made unfused: cz_info 13
 *     reports 0); every preconditioner application is z = s M^-1 (s r) with M^-1 the constant-coefficient jacobi / mg / mgrb under the handle's
 *     boundary state -- symmetric and positive definite, good for smooth coefficients and moderate jumps, slow (but correct) for large
 *     jumps (DESIGN.md 5.19 has the counts); none stays z = r;
 *   cz_get_residual returns r = b - A p of that operator (kernel forms 2 and 3 of cz_info 20: the residual goes through a work array);
 *   cz_sub_grad subtracts (beta_x(i, j, k) (p(i+1) - p(i))) scale from u, likewise v and w, so that div(u - beta grad p) = div u - A p exactly;
 *   cz_set_rhs_div, cz_add_field and cz_precondition are unchanged (the last applies the constant-coefficient M^-1 without the scaling;
 *     while cz_set_coef_mg is in force, the coefficient cycle M_beta^-1 that cz_solve applies);
 *   cz_solve, cz_sweeps and cz_evaluate of a solver other than pcg return 0 with one line and leave P alone.
 * All three pointers NULL clears the state (the arrays are freed; the handle then runs the code and gives the bytes of a handle that never
 * had coefficients); cz_setup clears it too.  cz_set_periodic / cz_set_closed_box / cz_set_neumann after this call keep the coefficients:
 * the alias faces and s follow the periodic directions (face 1's own value is kept for the day its direction stops being periodic).
 * Return 1, or 0 with one line on stderr and nothing changed: before cz_setup, some but not all pointers NULL, a NULL stride or a stride < 1,
 * an array that is not aligned to CZ_REAL, a pointer that is not on the handle's device, a _maf handle, a decomposed run (the faces in the
 * ghost layers need an exchange: the follow-up).  One more refusal is NOT "nothing changed": some face that the operator reads holds a
 * value that is not finite and positive (or D overflows, or s is not finite and positive).  That is a count made on the device after the
 * import; the call waits for it (its one host wait), returns 0 with a line and leaves the handle WITHOUT coefficients, also where it had
 * some before.  The same holds where a later change of the periodic directions makes the operator read a bad face 1: that setter prints
 * the line, takes the new state and leaves the handle without coefficients (cz_info 25 tells). */
int cz_set_face_coef(cz_handle*, const CZ_REAL* bx, const CZ_REAL* by, const CZ_REAL* bz, const long long* stride, int on_device, void* ready_stream);
/* The face coefficients inside the multigrid hierarchy: on = 1 asks that pcg ... mg | mgrb precondition with the V-cycle of
 * the variable operator itself, z = M_beta^-1 r (czhip_mg_set_coef), in place of the constant cycle inside the diagonal scaling.  The flag
 * is remembered; it is IN FORCE (cz_info 27) while it is on, face coefficients are in force (cz_info 25) and the set-up preconditioner is mg
 * or mgrb; with none or jacobi it is accepted and idle.  The hierarchy is built inside whichever call makes or changes that state: this
 * one, cz_set_face_coef, cz_set_neumann, cz_set_periodic, cz_set_closed_box.  While in force cz_solve applies the cycle without the scaling
 * and cz_precondition applies the same cycle; everything else of cz_set_face_coef is untouched.  A handle on which the flag was never set,
 * or is off again, gives the bytes of before in every state.  cz_setup clears the flag.  Returns 1, or 0 with one line on stderr and
 * nothing changed: before cz_setup, a _maf handle, a decomposed run.  One refusal is NOT "nothing changed": a coarse weight or diagonal
 * -- a sum of up to 4^l fine ones -- is not finite and positive.  The call that built the hierarchy (any of the five) then prints one
 * line, returns 0 and turns the flag off; the face coefficients (and that call's own new state) stay, and the scaled preconditioner runs. */
int cz_set_coef_mg(cz_handle*, int on);
/* Zebra line iterations along Z in the V-cycle of pcg ... mgrb, for grids refined towards a wall: lay the refined direction
 * on Z.  on = 1 asks that the cycle smooths with line iterations (czhip_mg_set_lines) while the coefficient hierarchy is in force.  The flag
 * is remembered; it is IN FORCE (cz_info 28) while it is on, cz_info 27 is 1 and the set-up preconditioner is mgrb; with mg, jacobi or none
 * it is accepted and idle.  Whichever call settles the coefficient hierarchy carries the flag to it; where that hierarchy is dropped for a
 * coarse overflow the lines go idle with it.  While in force cz_solve and cz_precondition apply the line cycle.  A handle on which the
 * flag was never set, or is off again, gives the bytes of before in every state.  cz_setup clears the flag.  Returns 1, or 0 with one line
 * on stderr and nothing changed: before cz_setup, a _maf handle, a decomposed run, on other than 0 | 1, and on = 1 on a handle whose
 * coefficient exceeds 1 -- line iterations take 0 < coef <= 1: over-relaxed, the lagged wrap of a periodic Z makes the preconditioner
 * indefinite. */
int cz_set_mg_lines(cz_handle*, int on);
/* Zero-flux (Neumann) faces for pcg: faces[6], order X-, X+, Y-, Y+, Z-, Z+ of the GLOBAL box (the order of nID), non-zero =
 * the face is a zero-flux face, zero = a Dirichlet face as before; at least one face must stay Dirichlet.  Called after cz_setup; collective,
 * with the same mask on every rank.  On a Neumann face the face layer of the field is not data but the mirror of the first inner layer
 * (p(1, j, k) = p(2, j, k), p(size, j, k) = p(size-1, j, k) over the cells every sweep updates), which makes the stated system
 * `sum of neighbours - 6 p = b` the zero-flux operator (5 neighbours, -5 p) at the cells next to it; a non-zero flux folds into b.  On return
 * of every call that writes P (this one, cz_set_field, cz_add_field, cz_solve) those layers hold the mirror: values passed there are
 * ignored, cz_get_field returns the mirror, cz_get_residual mirrors before its pass.  Returns 1, or 0 with one line on stderr and nothing
 * changed: before cz_setup, all six faces, a _maf handle.  Accepted on a handle of any other solver, but with a non-zero mask cz_solve,
 * cz_sweeps and cz_evaluate of a solver other than pcg (none | jacobi | mg | mgrb) return 0 with one line and leave P alone.  All zero: the
 * Dirichlet problem again (the face layers keep their last values).  cz_setup (and with it cz_evaluate, once it has accepted the solver)
 * clears the mask: a set-up starts with Dirichlet faces. */
int cz_set_neumann(cz_handle*, const int* faces);
/* The closed box for pcg: all six faces zero-flux.  The operator is then singular (its null space: the constants), so the
 * mode keeps the right-hand side compatible, the residual in the range of the operator and the answer of zero mean:
 *   on = 1 (after cz_setup, not a _maf handle): the six faces become Neumann faces (cz_info 21 reports 63, cz_info 22 reports 1), the
 *     hierarchy learns the mask, the right-hand side the handle holds loses its mean over the global inner box -- S = sum b in double, one
 *     all-reduce in a decomposed run, m = (REAL)(S / npts), b <- b - m in REAL -- and so does every right-hand side a later cz_set_rhs
 *     brings; P is mirrored.  cz_solve (pcg with none | jacobi | mg | mgrb) removes the mean of the initial residual, removes in every
 *     update the mean the residual had after the update before (rounding drift: A p has zero sum), and returns a field of zero mean over
 *     the inner box with the mirrors in place -- the same field whichever preconditioner ran, up to the tolerance.
 *   on = 0: mask 0, mode off, the work vectors cleared as cz_set_neumann does.  The right-hand side is NOT restored: it stays projected.
 * Collective, the same value on every rank.  Returns 1, or 0 with one line on stderr and nothing changed: before cz_setup, a _maf handle,
 * the hierarchy's refusal.  Solvers other than pcg are refused while the mode is on, as under cz_set_neumann; an accepted cz_set_neumann
 * leaves the mode (its own refusal of six flags stands: a caller who has not met compatibility is pointed here); cz_setup clears it.
 * cz_closed_mean: the mean last removed, as a double holding the REAL -- which = 0 from the right-hand side, 1 from the initial residual
 * of the last solve, 2 from the answer of the last solve; NaN for another `which`, 0.0 where nothing was removed since cz_setup.  The
 * projection of a right-hand side adds no host wait to cz_set_rhs: its mean stays on the device until cz_closed_mean(h, 0) asks for it,
 * and that call waits for the compute stream. */
int cz_set_closed_box(cz_handle*, int on);
double cz_closed_mean(cz_handle*, int which);
/* Periodic directions for pcg: dirs[3], order X, Y, Z of the GLOBAL box, non-zero = periodic.  Called after cz_setup;
 * collective, with the same flags on every rank.  In a periodic direction the two face layers of the field are not data but the wrap,
 * p(1, j, k) = p(size-1, j, k) and p(size, j, k) = p(2, j, k) over the cells every sweep updates, which makes the stated system
 * `sum of neighbours - 6 p = b` the periodic operator.  On return of every call that writes P (this one, cz_set_neumann, cz_set_closed_box,
 * cz_set_field, cz_add_field, cz_solve) those layers hold the wrap: values passed there are ignored, cz_get_field returns the wrap,
 * cz_get_residual fills before its pass.  The flags are a state of their own beside the mask of cz_set_neumann and the closed mode:
 * cz_setup clears them, the other two setters leave them alone, and in a periodic direction the Neumann flags are ignored (cz_info 21 keeps
 * reporting them).  All three setters apply one rule to the combined state: with the closed mode off, some face of a direction that is not
 * periodic must be a Dirichlet face.  cz_set_closed_box(h, 1) then cz_set_periodic(h, {1,0,1}) is the channel, with {1,1,1} the triply
 * periodic box; {1,0,0} alone is periodic X with Dirichlet Y and Z.  Returns 1, or 0 with one line on stderr and nothing changed: before
 * cz_setup, NULL, a _maf handle, a periodic direction of fewer than two inner points (G_size < 4) or one that the decomposition cuts
 * (G_div > 1), the rule above.  With a flag set, cz_solve, cz_sweeps and cz_evaluate of a solver other than pcg (none | jacobi | mg | mgrb)
 * return 0 with one line and leave P alone. */
int cz_set_periodic(cz_handle*, const int* dirs);
int cz_set_eps(cz_handle*, double eps);
int cz_set_itr_max(cz_handle*, int n);
int cz_sweeps(cz_handle*, int n);              /* bench leg: n more iterations of the selected stationary solver with the
                                                  full per-iteration work (sweep + residual + convergence bookkeeping),
                                                  never stopping early; returns n */
int cz_result_iter(const cz_handle*);
double cz_result_res(const cz_handle*);
int cz_history(const cz_handle*, double* out, int cap); /* copies min(cap, n) residuals, returns n */
void cz_field(const cz_handle*, CZ_REAL* host_out);    /* D2H of the solution P, dense (NK+4,NI+4,NJ+4) */
void cz_local_size(const cz_handle*, int* size3, int* head3, int* nID6, int* inner6);
double cz_error_max(cz_handle*, int* loc3);   /* debug epilogue, cz_Evaluate.cpp:550-563 (host-side restatement) */
void cz_set_quiet(cz_handle*, int quiet);     /* suppress stdout / history file (tests, bench) */
double cz_last_solve_seconds(const cz_handle*);
/* What a (multi-GPU) run decided: what = 0 ranks, 1 every brick takes the fused pass, 2 shell slabs of this brick, 3 overlapped exchange,
 * 4 the last stationary solve ran its residual all-reduce + test one pass behind, 5 ranks of the RCCL communicator (ncclCommCount; 0 = LOCAL
 * test transport or single process), 6 CUs per XCD the sweeps leave to the exchange stream (CZ_COMM_CUS); the plan of the stationary sweeps
 * of the last cz_solve / cz_sweeps (the preconditioner's, for a Krylov solver; 0, 1, 2 as after cz_setup where that call planned none, as pcg
 * does under a mask or a periodic flag): 7 kind of pass (0 single sweeps, 1 fused pass over the whole box, 2 fused pass as shell slabs + interior with the exchange
 * overlapped), 8 ghost layers exchanged per pass, 9 rotating field buffers; 10 vector updates of the last BiCGSTAB solve that were made inside
 * the first pair of the preconditioner solve they feed (czhip_jacobi2_from_zero_made_async); 11 passes of the last red-black SOR solve that made
 * two iterations each (czhip_rbsor4_async); 12 converged iterations of the last Jacobi or red-black SOR solve that were the first of a fused pass
 * (a pair of sweeps, or an rb4 pass of two iterations) and were therefore re-run alone from the pass's untouched input to give the converged iterate;
 * 13 iterations of the last PCG solve whose search direction was made inside the SpMV pass (czhip_cg_dir_ax_async); 14 three-sweep
 * Jacobi passes of the last Jacobi solve (czhip_jacobi3_async); 15 levels of the multigrid hierarchy (pcg ... mg; 0 otherwise); 16 V-cycles
 * of the last PCG solve with mg; 17 the gather level G of a decomposed pcg ... mg (levels >= G run on every rank from an all-gathered copy;
 * 0 on a single domain or where level 0 is the coarsest); 18 halo exchanges and all-gathers of the last V-cycle of a decomposed pcg ... mg;
 * 19 the smoother of the multigrid preconditioner (0 none, 1 relaxed Jacobi: mg, 2 symmetric red-black: mgrb; 15 and 16 count for both);
 * 20 the kernel form of the last cz_set_rhs / cz_set_field / cz_get_field / cz_get_residual / cz_add_field / cz_set_rhs_div / cz_sub_grad (1 k rows,
 * 2 tile transpose, 3 generic; CZ_FIELD_FORM=3 forces 3; the last two have no transpose form);
 * 21 the mask of cz_set_neumann, bit f = face f of X-, X+, Y-, Y+, Z-, Z+ (0: none; 63: the closed box);
 * 22 the closed-box mode of cz_set_closed_box (0 | 1); 23 the periodic directions of cz_set_periodic, bit d = X, Y, Z (0: none);
 * 24 the last cz_solve was a pcg that stopped at a breakdown (|rho| < FLT_MIN, absolute in both precisions) before any update: cz_solve
 * returned 0, P holds the caller's bytes (in the closed box: less its mean), cz_result_iter, cz_result_res and the history are 0 / empty --
 * the start was the answer already, or the problem is scaled below the threshold (1); anything else, a refusal or an error included (0);
 * 25 face coefficients are in force (cz_set_face_coef; 0 | 1); 26 four-sweep Jacobi passes of the last Jacobi solve (czhip_jacobi4_async;
 * 14 counts the three-sweep passes beside them); 27 the coefficient hierarchy of cz_set_coef_mg is in force (0 | 1);
 * 28 the line iterations of cz_set_mg_lines are in force (0 | 1). */
int cz_info(const cz_handle*, int what);
/* The driver's and its communicator's own copies of their switches, as name=value, one per line: overlap, lag_reduce, comm_cus (as asked for;
 * 0 on a single domain), comm_cus_reserved (in force after set-up), bicg_fuse, bicg_devsc, bicg_alias, cg_fuse, mg_tail, mg_gather, mgrb_zero4,
 * field_form; of the communicator (-1 on a single domain): comm_pack_j, comm_direct_messages (messages of the two-layer exchange sent from /
 * received into the array itself: the J faces unless CZ_COMM_PACK_J=1), comm_one_comm.  The string lives until the next call on the thread. */
const char* cz_config_in_force(const cz_handle*);
/* pcg ... mg | mgrb: z = M^-1 r, the set-up solver's V-cycle applied once to host fields of the calling rank's brick in the cz_field layout (the
 * ghost cells of r are not read).  Collective: every rank of a decomposed run calls it.  Returns 1, or 0 where there is no such
 * preconditioner (another solver, or not set up). */
int cz_precondition(cz_handle*, const CZ_REAL* r_dense, CZ_REAL* z_dense);
double cz_kernel_ms(const cz_handle*, const char* label); /* HIP-event time of a labelled section, ms (avg per launch) */

void cz_set_debug(cz_handle*, int mode);      /* main.cpp:38-42: 1 = run the analytic-error epilogue in cz_evaluate */
void cz_set_profile(cz_handle*, int on);      /* cz_Evaluate.cpp:506-545: 1 = cz_evaluate writes profiling.txt (PMlib-style section report) */

/* ------------------------------------------------------------------------------------------------
 * Part 5 -- multi-GPU bootstrap (replaces MPI_Init / CBrick set-up, main.cpp:33-35, cz_Evaluate.cpp:103-159).
 * One process per GPU.  Rank 0 creates the RCCL unique id, the launcher (torch.distributed in bench.py, a shared
 * file for the `cz` binary) hands the bytes to every rank, every rank joins BEFORE cz_setup(); cz_setup then takes
 * rank / size from the communicator and decomposes the cube.  Nothing to call for a single-GPU run.
 * ---------------------------------------------------------------------------------------------- */
int cz_comm_unique_id_bytes(void);
int cz_comm_get_unique_id(char* out_bytes);
int cz_comm_bootstrap(int rank, int nranks, const char* id_bytes);
void cz_comm_shutdown(void);
int cz_comm_selftest(void); /* one-rank RCCL smoke test: init, all-reduce, grouped send/recv to self; 0 = ok */
/* Host-only decomposition helpers (no GPU needed): automatic division and the brick of one rank
 * (local size, 1-based global head index, neighbour table I-,I+,J-,J+,K-,K+ with -1 = physical boundary). */
void cz_comm_auto_division(int nproc, const int* G_size, int* G_div);
int cz_comm_decompose(const int* G_size, const int* G_div, int nproc, int rank, int* size, int* head, int* nID);
/* Test transport: n ranks as n host threads of one process on one GPU (device-to-device copies instead of RCCL). */
void* cz_comm_local_world(int n);
void cz_comm_local_world_free(void* world);
int cz_comm_bootstrap_local(void* world, int rank);

#ifdef __cplusplus
}
#endif
#endif /* CZ_HIP_H_ */
