// What v_div_scale_f32 / _f64 hand out for a divisor of ordinary magnitude and numerators of every class: the stand-alone probe behind
// profiles/r21/div_scale_classes.txt (cz_k_fastdiv.h's choice between its two reciprocals rests on that table).  Not part of the library.
//   hipcc --offload-arch=gfx950 -O2 tools/div_scale_probe.hip -o tools/bin/div_scale_probe && tools/bin/div_scale_probe
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cmath>
__global__ void k32(const float* n, float d, int cnt, float* den, float* num, int* vcc) {
  int i = threadIdx.x;
  if (i >= cnt) return;
  bool v, u;
  den[i] = __builtin_amdgcn_div_scalef(n[i], d, false, &u);
  num[i] = __builtin_amdgcn_div_scalef(n[i], d, true, &v);
  vcc[i] = v;
}
__global__ void k64(const double* n, double d, int cnt, double* den, double* num, int* vcc) {
  int i = threadIdx.x;
  if (i >= cnt) return;
  bool v, u;
  den[i] = __builtin_amdgcn_div_scale(n[i], d, false, &u);
  num[i] = __builtin_amdgcn_div_scale(n[i], d, true, &v);
  vcc[i] = v;
}
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s\n", hipGetErrorString(e)); return 2; } } while (0)
int main() {
  const int e32[] = {-149, -140, -130, -126, -124, -123, -120, -110, -104, -103, -102, -100, -50, 0, 50, 97, 98, 99, 110, 120};
  const int e64[] = {-1074, -1050, -1022, -1020, -1019, -1000, -970, -969, -968, -900, 0, 700, 769, 770, 771, 900, 1000};
  const int c32 = sizeof(e32) / 4, c64 = sizeof(e64) / 4;
  float hn[32], *dn, *dd, *dm; double gn[32], *en, *ed, *em; int *dv, hv[32];
  for (int i = 0; i < c32; i++) hn[i] = ldexpf(1.5f, e32[i]);
  for (int i = 0; i < c64; i++) gn[i] = ldexp(1.5, e64[i]);
  CK(hipMalloc(&dn, 128)); CK(hipMalloc(&dd, 128)); CK(hipMalloc(&dm, 128)); CK(hipMalloc(&dv, 128));
  CK(hipMalloc(&en, 256)); CK(hipMalloc(&ed, 256)); CK(hipMalloc(&em, 256));
  CK(hipMemcpy(dn, hn, 128, hipMemcpyHostToDevice)); CK(hipMemcpy(en, gn, 256, hipMemcpyHostToDevice));
  for (float d : {6.0f, 6.2f}) {
    hipLaunchKernelGGL(k32, dim3(1), dim3(64), 0, 0, dn, d, c32, dd, dm, dv);
    float hd[32], hm[32];
    CK(hipMemcpy(hd, dd, 128, hipMemcpyDeviceToHost)); CK(hipMemcpy(hm, dm, 128, hipMemcpyDeviceToHost)); CK(hipMemcpy(hv, dv, 128, hipMemcpyDeviceToHost));
    for (int i = 0; i < c32; i++) printf("f32 d=%g n=1.5*2^%d: den_s/d=2^%g num_s/n=2^%g vcc=%d\n", d, e32[i], log2((double)hd[i] / d), log2((double)hm[i] / hn[i]), hv[i]);
  }
  {
    double d = 6.0;
    hipLaunchKernelGGL(k64, dim3(1), dim3(64), 0, 0, en, d, c64, ed, em, dv);
    double hd[32], hm[32];
    CK(hipMemcpy(hd, ed, 256, hipMemcpyDeviceToHost)); CK(hipMemcpy(hm, em, 256, hipMemcpyDeviceToHost)); CK(hipMemcpy(hv, dv, 128, hipMemcpyDeviceToHost));
    for (int i = 0; i < c64; i++) printf("f64 d=%g n=1.5*2^%d: den_s/d=2^%g num_s/n=2^%Lg vcc=%d\n", d, e64[i], log2(hd[i] / d), log2l((long double)hm[i] / (long double)gn[i]), hv[i]);
  }
  return 0;
}
