// cz_h_field.h -- part of cz_kernels.hip (included inside namespace czhip_internal): the launches of cz_k_field.h's and cz_k_resid.h's kernels.
// arr: a padded array of sz with guide g; user: the caller's brick, cell (i, j, k) at user[i stride[0] + j stride[1] + k stride[2]] (elements;
// positive -- the driver checked); to_user: 0 import, 1 export.  form: 0 = from the strides, 1 row / 2 transpose where the strides allow it
// (else refused), 3 = generic.  On the calling thread's compute stream.  Returns the form taken (1 row, 2 transpose, 3 generic), 0 = refused.
static bool field_geom(FieldGeom& fg, const int* sz, int g, const long long* stride) {
  fg.ni = sz[0], fg.nj = sz[1], fg.nk = sz[2], fg.g = g;
  fg.nkp = sz[2] + 2 * g;
  fg.PSE = (long long)fg.nkp * (sz[0] + 2 * g);
  fg.s0 = stride[0], fg.s1 = stride[1], fg.s2 = stride[2];
  return !(fg.ni < 1 || fg.nj < 1 || fg.nk < 1 || fg.s0 < 1 || fg.s1 < 1 || fg.s2 < 1);
}
// the form for these strides (row_fits: the row kernel's index range holds), 0 = the form asked for cannot take them
static int field_form_of(const FieldGeom& fg, int form, bool row_fits) {
  int take = form;
  if (take == 0) take = (fg.s2 == 1 && row_fits) ? 1 : (fg.s0 == 1 || fg.s1 == 1) ? 2 : 3;
  if (take == 1 && !(fg.s2 == 1 && row_fits)) return 0;
  if (take == 2 && !(fg.s0 == 1 || fg.s1 == 1)) return 0;
  return take >= 1 && take <= 3 ? take : 0;
}
// the box idx (1-based, inclusive: the cells every sweep updates) in the brick's 0-based cells
static FieldBox field_box(const int* idx) { return FieldBox{idx[0] - 1, idx[1] - 1, idx[2] - 1, idx[3] - 1, idx[4] - 1, idx[5] - 1}; }

// the transpose (take 2) and generic (take 3) forms; false: the grid does not hold the brick
template <int DIR, class T, int OP>
static bool field_tr_any_launch(int take, typename FieldSides<DIR, T>::D* dst, const typename FieldSides<DIR, T>::S* src, const FieldGeom& fg, const FieldBox& bx,
                                REAL scale) {
  const int g = fg.g;
  if (take == 2) {
    FieldTGeom tg;
    const bool ui = fg.s0 == 1;  // the unit stride is i (else j); w is the other of the two
    tg.nu = ui ? fg.ni : fg.nj, tg.nw = ui ? fg.nj : fg.ni, tg.nk = fg.nk;
    tg.a0 = (long long)g * fg.PSE + (long long)g * fg.nkp + g;
    tg.a_us = ui ? (long long)fg.nkp : fg.PSE, tg.a_ws = ui ? fg.PSE : (long long)fg.nkp;
    tg.u_ws = ui ? fg.s1 : fg.s0, tg.u_ks = fg.s2;
    const FieldBox tb = ui ? bx : FieldBox{bx.lo1, bx.hi1, bx.lo0, bx.hi0, bx.lo2, bx.hi2};
    const dim3 grid((unsigned)((tg.nu + FIELD_TS - 1) / FIELD_TS), (unsigned)((tg.nk + FIELD_TS - 1) / FIELD_TS), (unsigned)std::min(tg.nw, 65535));
    if (grid.y > 65535u) return false;
    hipLaunchKernelGGL((field_tr_k<DIR, T, OP>), grid, dim3(256), 0, ctx.stream, dst, src, tg, tb, scale);
  } else {
    const unsigned gy = (unsigned)std::min(fg.nj, 65535);
    const unsigned gx = (unsigned)std::min<long long>(((long long)fg.ni * fg.nk + 255) / 256, 4096);
    hipLaunchKernelGGL((field_any_k<DIR, T, OP>), dim3(gx, gy), dim3(256), 0, ctx.stream, dst, src, fg, bx, scale);
  }
  return true;
}

int field_copy_async(REAL* arr, REAL* user, const int* sz, int g, const long long* stride, int to_user, int form) {
  ensure_init();
  if (!arr || !user || (reinterpret_cast<uintptr_t>(user) & (sizeof(REAL) - 1))) return 0;
  FieldGeom fg;
  if (!field_geom(fg, sz, g, stride)) return 0;
  const int slots = (fg.nk + 2 * VW - 2) / VW;  // vectors a row can touch, whatever its phase
  const int take = field_form_of(fg, form, (long long)fg.ni * slots <= 0x7fffffffLL);
  if (!take) return 0;
  REAL* dst = to_user ? user : arr;
  const REAL* src = to_user ? arr : user;
  ScopedTimer tm(LBL_FIELD);
  if (take == 1) {
    const unsigned gy = (unsigned)std::min(fg.nj, 65535);
    const unsigned gx = (unsigned)std::min<long long>(((long long)fg.ni * slots + 255) / 256, 4096);
    if (to_user) hipLaunchKernelGGL((field_row_k<VW, 1>), dim3(gx, gy), dim3(256), 0, ctx.stream, dst, src, fg, slots);
    else hipLaunchKernelGGL((field_row_k<VW, 0>), dim3(gx, gy), dim3(256), 0, ctx.stream, dst, src, fg, slots);
  } else if (!(to_user ? field_tr_any_launch<1, REAL, 0>(take, dst, src, fg, FieldBox(), (REAL)0) : field_tr_any_launch<0, REAL, 0>(take, dst, src, fg, FieldBox(), (REAL)0))) {
    return 0;
  }
  HIP_CHECK(hipGetLastError());
  return take;
}

// cz_get_residual: r = rhs - A p at the cells of idx (blas_calc_rk_'s arithmetic with the coefficients cf), 0 at the brick's
// other cells, as (T)(r scale) into the caller's brick `user` of T = float | double (user_bytes 4 | 8; nullptr: no destination), and
// sumsq_dev[0] = sum r^2 (double squares, double sums; the same bits whatever the destination).  Row form: one launch (resid_row_k).  The
// other forms: blas_calc_rk_ into wrk (its inner box is scratch), wrk out through the transpose / generic kernel, and resid_row_k without a
// destination for the sum.  Returns the form taken (norm only: 1), 0 = refused, nothing launched.
template <class T>
static int field_residual_launch(const REAL* p, const REAL* rhs, REAL* wrk, T* user, const int* sz, const int* idx, const FieldGeom& fg, const REAL* cf,
                                 REAL scale, int take, double* sumsq_dev) {
  const int slots = (fg.nk + 6) / 4;  // runs of four cells a row can touch, whatever its phase
  const FieldBox bx = field_box(idx);
  const Coef c = make_coef(cf, (REAL)0);
  const unsigned gy = (unsigned)std::min(fg.nj, 65535);
  const unsigned gx = (unsigned)std::min<long long>(((long long)fg.ni * slots + 255) / 256, 4096);
  ensure_partials((size_t)gx * gy);
  if (user && take != 1) {
    calc_rk_async(wrk, p, rhs, sz, idx, fg.g, cf);
    ScopedTimer tm(LBL_FIELD);
    if (!field_tr_any_launch<1, T, 1>(take, user, wrk, fg, bx, scale)) return 0;
  }
  ScopedTimer tm(LBL_FIELD);
  if (user && take == 1) hipLaunchKernelGGL((resid_row_k<T, 1>), dim3(gx, gy), dim3(256), 0, ctx.stream, user, p, rhs, fg, bx, c, scale, slots, ctx.partials, sumsq_dev, ctx.counter);
  else hipLaunchKernelGGL((resid_row_k<REAL, 0>), dim3(gx, gy), dim3(256), 0, ctx.stream, (REAL*)nullptr, p, rhs, fg, bx, c, scale, slots, ctx.partials, sumsq_dev, ctx.counter);
  HIP_CHECK(hipGetLastError());
  return take;
}
int field_residual_async(const REAL* p, const REAL* rhs, REAL* wrk, void* user, int user_bytes, const int* sz, const int* idx, int g, const long long* stride,
                         const REAL* cf, double scale, int form, double* sumsq_dev) {
  ensure_init();
  static const long long unit[3] = {1, 1, 1};
  FieldGeom fg;
  if (!p || !rhs || !wrk || !sumsq_dev || !field_geom(fg, sz, g, user ? stride : unit)) return 0;
  if ((long long)fg.ni * ((fg.nk + 6) / 4) > 0x7fffffffLL) return 0;
  if (!user) return field_residual_launch<REAL>(p, rhs, wrk, nullptr, sz, idx, fg, cf, (REAL)scale, 1, sumsq_dev);
  if ((user_bytes != 4 && user_bytes != 8) || (reinterpret_cast<uintptr_t>(user) & (uintptr_t)(user_bytes - 1))) return 0;
  const int take = field_form_of(fg, form, true);
  if (!take) return 0;
  if (user_bytes == 4) return field_residual_launch<float>(p, rhs, wrk, static_cast<float*>(user), sz, idx, fg, cf, (REAL)scale, take, sumsq_dev);
  return field_residual_launch<double>(p, rhs, wrk, static_cast<double*>(user), sz, idx, fg, cf, (REAL)scale, take, sumsq_dev);
}

// cz_add_field: p = p + (REAL)user (REAL)scale at the cells of idx, p's other cells untouched; forms and return value as field_copy_async
template <class T>
static int field_add_launch(REAL* p, const T* user, const int* idx, const FieldGeom& fg, REAL scale, int form) {
  const int slots = (fg.nk + 2 * VW - 2) / VW;
  const int take = field_form_of(fg, form, (long long)fg.ni * slots <= 0x7fffffffLL);
  const FieldBox bx = field_box(idx);
  if (!take) return 0;
  if (bx.hi0 < bx.lo0 || bx.hi1 < bx.lo1 || bx.hi2 < bx.lo2) return take;  // (a brick without a cell to update)
  ScopedTimer tm(LBL_FIELD);
  if (take == 1) {
    const unsigned gy = (unsigned)std::min(bx.hi1 - bx.lo1 + 1, 65535);
    const unsigned gx = (unsigned)std::min<long long>(((long long)fg.ni * slots + 255) / 256, 4096);
    hipLaunchKernelGGL((addf_row_k<T>), dim3(gx, gy), dim3(256), 0, ctx.stream, p, user, fg, bx, scale, slots);
  } else if (!field_tr_any_launch<0, T, 1>(take, p, user, fg, bx, scale)) {
    return 0;
  }
  HIP_CHECK(hipGetLastError());
  return take;
}
int field_add_async(REAL* p, const void* user, int user_bytes, const int* sz, const int* idx, int g, const long long* stride, double scale, int form) {
  ensure_init();
  FieldGeom fg;
  if (!p || !user || (user_bytes != 4 && user_bytes != 8) || (reinterpret_cast<uintptr_t>(user) & (uintptr_t)(user_bytes - 1))) return 0;
  if (!field_geom(fg, sz, g, stride)) return 0;
  if (user_bytes == 4) return field_add_launch<float>(p, static_cast<const float*>(user), idx, fg, (REAL)scale, form);
  return field_add_launch<double>(p, static_cast<const double*>(user), idx, fg, (REAL)scale, form);
}

// The projection step (cz_k_project.h).  u, v, w: the staggered velocity, three bricks with one stride triple; per: the
// periodic directions (bit d).  form: 0 = the row form where s2 == 1, else the generic one; 3 = generic.  Returns the form taken, 0 = refused.
// field_div_async: rhs = div (REAL)scale at the inner cells, 0 at the brick's other cells, sumsq_dev[0] = sum div^2 of the unscaled div.
static int proj_form_of(const FieldGeom& fg, int form, int slots) {
  if (form != 0 && form != 3) return 0;
  return (form == 0 && fg.s2 == 1 && (long long)fg.ni * slots <= 0x7ff00000LL) ? 1 : 3;
}
int field_div_async(REAL* rhs, const REAL* u, const REAL* v, const REAL* w, const int* sz, int g, const long long* stride, int per, double scale, int form,
                    double* sumsq_dev) {
  ensure_init();
  FieldGeom fg;
  if (!rhs || !u || !v || !w || !sumsq_dev || !field_geom(fg, sz, g, stride)) return 0;
  const int slots = (fg.nk + 2 * VW - 2) / VW;
  const int take = proj_form_of(fg, form, slots);
  if (!take) return 0;
  // about 4096 workgroups in all, each walking its share of a plane: every workgroup ends with one ticket on one counter, and a workgroup per
  // 256 runs (132 096 of them at 512^3) spent three quarters of the kernel's time queueing there (profiles/r19/project.txt)
  const unsigned gy = (unsigned)std::min(fg.nj, 65535);
  const long long need = (take == 1 ? (long long)fg.ni * slots + 255 : (long long)fg.ni * fg.nk + 255) / 256;
  const unsigned gx = (unsigned)std::max<long long>(1, std::min<long long>(need, 4096 / gy));
  ensure_partials((size_t)gx * gy);
  ScopedTimer tm(LBL_FIELD);
  if (take == 1) hipLaunchKernelGGL((div_row_k<VW>), dim3(gx, gy), dim3(256), 0, ctx.stream, rhs, u, v, w, fg, per, (REAL)scale, slots, ctx.partials, sumsq_dev, ctx.counter);
  else hipLaunchKernelGGL(div_any_k, dim3(gx, gy), dim3(256), 0, ctx.stream, rhs, u, v, w, fg, per, (REAL)scale, ctx.partials, sumsq_dev, ctx.counter);
  HIP_CHECK(hipGetLastError());
  return take;
}
// field_grad_async: u(i) = u(i) - (p(i + 1) - p(i)) (REAL)scale on the faces 0 .. n - 2 at inner tangential cells, v and w likewise; p's face
// layers as the caller left them; face 0 of a periodic direction = face n - 2
int field_grad_async(REAL* u, REAL* v, REAL* w, const REAL* p, const int* sz, int g, const long long* stride, int per, double scale, int form) {
  ensure_init();
  FieldGeom fg;
  if (!p || !u || !v || !w || !field_geom(fg, sz, g, stride)) return 0;
  const int slots = (fg.nk + 2 * VW - 2) / VW;
  const int take = proj_form_of(fg, form, slots);
  if (!take) return 0;
  const unsigned gy = (unsigned)std::min(fg.nj, 65535);
  const unsigned gx = (unsigned)std::min<long long>((take == 1 ? (long long)fg.ni * slots + 255 : (long long)fg.ni * fg.nk + 255) / 256, 4096);
  ScopedTimer tm(LBL_FIELD);
  if (take == 1) hipLaunchKernelGGL((grad_row_k<VW>), dim3(gx, gy), dim3(256), 0, ctx.stream, u, v, w, p, fg, per, (REAL)scale, slots);
  else hipLaunchKernelGGL(grad_any_k, dim3(gx, gy), dim3(256), 0, ctx.stream, u, v, w, p, fg, per, (REAL)scale);
  HIP_CHECK(hipGetLastError());
  return take;
}

// Face coefficients (cz_set_face_coef; cz_k_coef.h).  bx, by, bz, s: padded arrays of the handle.
// coef_prep_async: after the three imports (per_old 0) or a change of the periodic directions (per_old: those in force before) -- the alias
// faces of the periodic directions `per`, s = sqrt(6 / D) at the cells of idx and 0 at
// the brick's other cells, *bad_dev += the faces and cells that are not finite and positive (the caller zeroed it).  Label field_io.
void coef_prep_async(REAL* bx, REAL* by, REAL* bz, REAL* s, const int* sz, const int* idx, int g, int per, int per_old, unsigned* bad_dev) {
  ensure_init();
  static const long long unit[3] = {1, 1, 1};
  FieldGeom fg;
  if (!field_geom(fg, sz, g, unit)) return;
  const unsigned gy = (unsigned)std::min(fg.nj, 65535);
  const unsigned gx = (unsigned)std::min<long long>(((long long)fg.ni * fg.nk + 255) / 256, 4096);
  ScopedTimer tm(LBL_FIELD);
  hipLaunchKernelGGL(coef_prep_k, dim3(gx, gy), dim3(256), 0, ctx.stream, bx, by, bz, s, fg, field_box(idx), per, per_old, bad_dev);
  HIP_CHECK(hipGetLastError());
}
// coef_ax_async: mode 0: q = A p at the cells of idx, out[0] = p.q, out[1] = q.q (the slots of calc_ax_dots_async; label calc_ax); mode 1:
// q = b - A p there, out[0] = sum r^2, out[1] = 0 (label calc_rk).  q's other cells keep their bytes.  About 4096 workgroups at most, each
// with one ticket on the one counter (field_div_async's finding).  0 = refused (the row index does not fit), nothing launched.
int coef_ax_async(int mode, REAL* q, const REAL* p, const REAL* b, const REAL* bx, const REAL* by, const REAL* bz, const int* sz, const int* idx, int g,
                  double* out) {
  ensure_init();
  static const long long unit[3] = {1, 1, 1};
  FieldGeom fg;
  if (!q || !p || !bx || !by || !bz || !out || (mode == 1 && !b) || !field_geom(fg, sz, g, unit)) return 0;
  const FieldBox box = field_box(idx);
  if (box.hi0 < box.lo0 || box.hi1 < box.lo1 || box.hi2 < box.lo2) {
    HIP_CHECK(hipMemsetAsync(out, 0, 2 * sizeof(double), ctx.stream));
    return 1;
  }
  const int slots = (fg.nk + 2 * VW - 2) / VW;  // vectors a row can touch, whatever its phase
  const long long rows = box.hi0 - box.lo0 + 1, planes = box.hi1 - box.lo1 + 1;
  if (rows * slots > 0x7ff00000LL) return 0;
  const unsigned gy = (unsigned)std::min<long long>(planes, 4096);
  const unsigned gx = (unsigned)std::max<long long>(1, std::min<long long>((rows * slots + 255) / 256, 4096 / gy));
  ensure_partials((size_t)2 * gx * gy);
  ScopedTimer tm(mode ? LBL_RK : LBL_AX);
  if (mode) hipLaunchKernelGGL((ax_coef_k<VW, 1>), dim3(gx, gy), dim3(256), 0, ctx.stream, q, p, b, bx, by, bz, fg, box, slots, ctx.partials, out, ctx.counter);
  else hipLaunchKernelGGL((ax_coef_k<VW, 0>), dim3(gx, gy), dim3(256), 0, ctx.stream, q, p, b, bx, by, bz, fg, box, slots, ctx.partials, out, ctx.counter);
  HIP_CHECK(hipGetLastError());
  return 1;
}
// coef_scale_async: out = s in where s is not zero (the cells of the box), 0 at every other cell of the padded array; out may be in.  Label ewise.
void coef_scale_async(REAL* out, const REAL* in, const REAL* s, const int* sz, int g) {
  ensure_init();
  const long long n = (long long)(sz[0] + 2 * g) * (sz[1] + 2 * g) * (sz[2] + 2 * g);
  const long long nvec = (n + VW - 1) / VW;
  const unsigned gx = (unsigned)std::max<long long>(1, std::min<long long>((nvec + 255) / 256, 8192));
  ScopedTimer tm(LBL_EWISE);
  hipLaunchKernelGGL((coef_scale_k<VW>), dim3(gx), dim3(256), 0, ctx.stream, out, in, s, nvec, n);
  HIP_CHECK(hipGetLastError());
}
// cz_get_residual under coefficients: r = rhs - A p into wrk (coef_ax_async mode 1, sumsq_dev[0] = sum r^2), then wrk out as (T)(r scale)
// through the transpose / generic export forms (a k-row destination takes the generic one: the row form of the export is resid_row_k's own
// pass).  Returns the form taken (norm only: 1), 0 = refused, nothing launched.
int field_residual_coef_async(const REAL* p, const REAL* rhs, REAL* wrk, void* user, int user_bytes, const int* sz, const int* idx, int g,
                              const long long* stride, const REAL* bx, const REAL* by, const REAL* bz, double scale, int form, double* sumsq_dev) {
  ensure_init();
  static const long long unit[3] = {1, 1, 1};
  FieldGeom fg;
  if (!p || !rhs || !wrk || !sumsq_dev || !field_geom(fg, sz, g, user ? stride : unit)) return 0;
  int take = 1;
  if (user) {
    if ((user_bytes != 4 && user_bytes != 8) || (reinterpret_cast<uintptr_t>(user) & (uintptr_t)(user_bytes - 1))) return 0;
    take = field_form_of(fg, form, true);
    if (!take) return 0;
    if (take == 1) take = 3;
  }
  if (!coef_ax_async(1, wrk, p, rhs, bx, by, bz, sz, idx, g, sumsq_dev)) return 0;
  if (!user) return take;
  const FieldBox box = field_box(idx);
  ScopedTimer tm(LBL_FIELD);
  const bool ok = user_bytes == 4 ? field_tr_any_launch<1, float, 1>(take, static_cast<float*>(user), wrk, fg, box, (REAL)scale)
                                  : field_tr_any_launch<1, double, 1>(take, static_cast<double*>(user), wrk, fg, box, (REAL)scale);
  HIP_CHECK(hipGetLastError());
  return ok ? take : 0;
}
// field_grad_async's coefficient form: u(i) = u(i) - (bx(i) (p(i + 1) - p(i))) (REAL)scale, v and w likewise
int field_grad_coef_async(REAL* u, REAL* v, REAL* w, const REAL* p, const REAL* bx, const REAL* by, const REAL* bz, const int* sz, int g,
                          const long long* stride, int per, double scale, int form) {
  ensure_init();
  FieldGeom fg;
  if (!p || !u || !v || !w || !bx || !by || !bz || !field_geom(fg, sz, g, stride)) return 0;
  const int slots = (fg.nk + 2 * VW - 2) / VW;
  const int take = proj_form_of(fg, form, slots);
  if (!take) return 0;
  const unsigned gy = (unsigned)std::min(fg.nj, 65535);
  const unsigned gx = (unsigned)std::min<long long>((take == 1 ? (long long)fg.ni * slots + 255 : (long long)fg.ni * fg.nk + 255) / 256, 4096);
  ScopedTimer tm(LBL_FIELD);
  if (take == 1) hipLaunchKernelGGL((grad_coef_row_k<VW>), dim3(gx, gy), dim3(256), 0, ctx.stream, u, v, w, p, bx, by, bz, fg, per, (REAL)scale, slots);
  else hipLaunchKernelGGL(grad_coef_any_k, dim3(gx, gy), dim3(256), 0, ctx.stream, u, v, w, p, bx, by, bz, fg, per, (REAL)scale);
  HIP_CHECK(hipGetLastError());
  return take;
}
