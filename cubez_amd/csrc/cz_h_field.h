// cz_h_field.h -- part of cz_kernels.hip (included inside namespace czhip_internal): the launch of cz_k_field.h's kernels.
// arr: a padded array of sz with guide g; user: the caller's brick, cell (i, j, k) at user[i stride[0] + j stride[1] + k stride[2]] (elements;
// positive -- the driver checked); to_user: 0 import, 1 export.  form: 0 = from the strides, 1 row / 2 transpose where the strides allow it
// (else refused), 3 = generic.  On the calling thread's compute stream.  Returns the form taken (1 row, 2 transpose, 3 generic), 0 = refused.
int field_copy_async(REAL* arr, REAL* user, const int* sz, int g, const long long* stride, int to_user, int form) {
  ensure_init();
  if (!arr || !user || (reinterpret_cast<uintptr_t>(user) & (sizeof(REAL) - 1))) return 0;
  FieldGeom fg;
  fg.ni = sz[0], fg.nj = sz[1], fg.nk = sz[2], fg.g = g;
  fg.nkp = sz[2] + 2 * g;
  fg.PSE = (long long)fg.nkp * (sz[0] + 2 * g);
  fg.s0 = stride[0], fg.s1 = stride[1], fg.s2 = stride[2];
  if (fg.ni < 1 || fg.nj < 1 || fg.nk < 1 || fg.s0 < 1 || fg.s1 < 1 || fg.s2 < 1) return 0;
  const int slots = (fg.nk + 2 * VW - 2) / VW;  // vectors a row can touch, whatever its phase
  const bool row_fits = (long long)fg.ni * slots <= 0x7fffffffLL;
  int take = form;
  if (take == 0) take = (fg.s2 == 1 && row_fits) ? 1 : (fg.s0 == 1 || fg.s1 == 1) ? 2 : 3;
  if (take == 1 && !(fg.s2 == 1 && row_fits)) return 0;
  if (take == 2 && !(fg.s0 == 1 || fg.s1 == 1)) return 0;
  REAL* dst = to_user ? user : arr;
  const REAL* src = to_user ? arr : user;
  const unsigned gy = (unsigned)std::min(fg.nj, 65535);
  ScopedTimer tm(LBL_FIELD);
  if (take == 1) {
    const unsigned gx = (unsigned)std::min<long long>(((long long)fg.ni * slots + 255) / 256, 4096);
    if (to_user) hipLaunchKernelGGL((field_row_k<VW, 1>), dim3(gx, gy), dim3(256), 0, ctx.stream, dst, src, fg, slots);
    else hipLaunchKernelGGL((field_row_k<VW, 0>), dim3(gx, gy), dim3(256), 0, ctx.stream, dst, src, fg, slots);
  } else if (take == 2) {
    FieldTGeom tg;
    const bool ui = fg.s0 == 1;  // the unit stride is i (else j); w is the other of the two
    tg.nu = ui ? fg.ni : fg.nj, tg.nw = ui ? fg.nj : fg.ni, tg.nk = fg.nk;
    tg.a0 = (long long)g * fg.PSE + (long long)g * fg.nkp + g;
    tg.a_us = ui ? (long long)fg.nkp : fg.PSE, tg.a_ws = ui ? fg.PSE : (long long)fg.nkp;
    tg.u_ws = ui ? fg.s1 : fg.s0, tg.u_ks = fg.s2;
    const dim3 grid((unsigned)((tg.nu + FIELD_TS - 1) / FIELD_TS), (unsigned)((tg.nk + FIELD_TS - 1) / FIELD_TS), (unsigned)std::min(tg.nw, 65535));
    if (grid.y > 65535u) return 0;
    if (to_user) hipLaunchKernelGGL((field_tr_k<1>), grid, dim3(256), 0, ctx.stream, dst, src, tg);
    else hipLaunchKernelGGL((field_tr_k<0>), grid, dim3(256), 0, ctx.stream, dst, src, tg);
  } else if (take == 3) {
    const unsigned gx = (unsigned)std::min<long long>(((long long)fg.ni * fg.nk + 255) / 256, 4096);
    if (to_user) hipLaunchKernelGGL((field_any_k<1>), dim3(gx, gy), dim3(256), 0, ctx.stream, dst, src, fg);
    else hipLaunchKernelGGL((field_any_k<0>), dim3(gx, gy), dim3(256), 0, ctx.stream, dst, src, fg);
  } else {
    return 0;
  }
  HIP_CHECK(hipGetLastError());
  return take;
}
