"""ctypes binding of include/cz_hip.h (parts 1-3: drop-in kernels, runtime, async operations)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

GUIDE = 2  # /root/reference/src/cz_cpp/cz_Define.h:40
_HERE = os.path.dirname(os.path.abspath(__file__))
_LOADED: dict = {}

# every symbol include/cz_hip.h declares (tests/test_abi.py checks the library exports all of them)
ABI_SYMBOLS = [
    "bc_k_", "jacobi_", "psor2sma_core_", "blas_clear_", "blas_copy_", "blas_triad_", "blas_dot1_", "blas_dot2_",
    "blas_bicg_1_", "blas_bicg_2_", "blas_calc_ax_", "blas_calc_rk_",
    "jacobi_maf_", "psor2sma_core_maf_", "calc_rk_maf_", "calc_ax_maf_", "search_pivot_", "pcr_rb_", "imask_k_",
    "czhip_real_bytes", "czhip_arch", "czhip_init", "czhip_finalize", "czhip_alloc_s3d", "czhip_free", "czhip_h2d",
    "czhip_d2h", "czhip_sync", "czhip_stream", "czhip_set_tuning", "czhip_get_tuning",
    "czhip_jacobi_async", "czhip_rbsor_async", "czhip_check_async", "czhip_jacobi_checked_async",
    "czhip_rbsor_checked_async", "czhip_jacobi2_async", "czhip_set_tuning2", "czhip_set_pcr_mode", "czhip_set_pcr_lex", "czhip_set_pcr_lex_timeout", "czhip_set_pcr_lex_limits", "czhip_set_psor", "czhip_set_psor_ahead", "czhip_use_t2", "czhip_set_pair_window", "czhip_set_pair_map", "czhip_set_pair_preload", "czhip_set_unit_coef", "czhip_config_describe", "czhip_tuning_describe", "czhip_set_comm_cus", "czhip_selftest_fastdiv", "czhip_selftest_mediumdiv", "czhip_selftest_gateddiv", "czhip_pair_maf_async", "czhip_rbsor2_async", "czhip_rbsor4_async", "czhip_set_rb4", "czhip_jacobi3_async", "czhip_set_jac3", "czhip_jacobi4_async", "czhip_set_jac4", "czhip_jac4_plan", "czhip_jac4_min_sweeps", "czhip_set_jac3_medium", "czhip_set_jac3_gate", "czhip_jac3_gated", "czhip_jac3_division", "czhip_jacobi2_from_zero_async", "czhip_jacobi2_from_zero_made_async", "czhip_check2_async", "czhip_pair_split_async", "czhip_cg_update_async", "czhip_cg_dir_ax_async", "czhip_mg_smooth_async", "czhip_mg_restrict_async", "czhip_mg_prolong_async", "czhip_mg_tail_async", "czhip_mg_create", "czhip_mg_levels", "czhip_mg_apply_async", "czhip_mg_destroy", "czhip_mg_rb_async", "czhip_mg_tail_rb_async", "czhip_mg_create_rb", "czhip_mg_kind", "czhip_mirror_faces_async", "czhip_mg_set_neumann", "czhip_fill_faces_async", "czhip_mg_set_periodic", "czhip_mg_set_coef", "czhip_mg_set_lines", "czhip_mg_line_chunk", "czhip_shift_sums_async", "czhip_cg_update_closed_async", "psor_", "psor_maf_", "pcr_", "pcr_eda_", "pcr_esa_", "pcr_rb_esa_", "pcr_j_esa_", "pcr_rb_maf_", "pcr_rb_esa_maf_", "pcr_maf_", "pcr_eda_maf_", "pcr_esa_maf_",
    "cz_create", "cz_destroy", "cz_evaluate", "cz_setup", "cz_solve", "cz_sweeps", "cz_result_iter", "cz_result_res",
    "cz_history", "cz_field", "cz_set_rhs", "cz_set_field", "cz_get_field", "cz_get_residual", "cz_add_field", "cz_set_rhs_div", "cz_sub_grad", "cz_set_face_coef", "cz_set_coef_mg", "cz_set_mg_lines", "cz_set_neumann", "cz_set_periodic", "cz_set_closed_box", "cz_closed_mean", "cz_set_eps", "cz_set_itr_max", "cz_local_size", "cz_error_max", "cz_set_quiet", "cz_last_solve_seconds", "cz_kernel_ms",
    "cz_set_debug", "cz_set_profile", "cz_info", "cz_config_in_force", "cz_precondition", "czhip_timing", "czhip_timing_read",
    "cz_comm_unique_id_bytes", "cz_comm_get_unique_id", "cz_comm_bootstrap", "cz_comm_shutdown", "cz_comm_selftest", "cz_comm_auto_division",
    "cz_comm_decompose", "cz_comm_local_world", "cz_comm_local_world_free", "cz_comm_bootstrap_local",
]


def lib_path(prec: str) -> str:
    return os.path.join(_HERE, f"libczhip_{prec}.so")


def load(prec: str = "f32") -> C.CDLL:
    """dlopen the HIP library of one precision.  Raises if it has not been built: there is no fallback."""
    if prec not in _LOADED:
        path = lib_path(prec)
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing -- build it with `make -C cubez_amd/csrc` "
                               "(or __graft_entry__.build()); cubez_amd has no CPU fallback")
        _LOADED[prec] = C.CDLL(path, mode=C.RTLD_LOCAL)
    return _LOADED[prec]


# the labels czhip_timing_read knows (kLabelNames of cz_h_ctx.h), but for JAC4_LABEL below
LABELS = ("jacobi", "rbsor", "calc_ax", "calc_rk", "reduce", "ewise", "dot", "jacobi2", "rbsor2", "pcr_rb", "pair_shell", "psor", "rbsor4", "jacobi3",
          "mg_restrict", "mg_smooth", "mg_prolong", "mg_tail", "mg_rb", "field_io", "bc_mirror", "shift_sums", "cg_update_closed")
# the four-sweep Jacobi pass (jac4_k) is timed under a label of its own, which czhip_timing_read knows too; it stands beside LABELS, whose
# length the ABI tests of earlier labels pin, and CZ.launches() counts it with the others
JAC4_LABEL = "jacobi4"


def _pairs(text: bytes) -> dict:
    return {k: int(v) for k, v in (line.split("=", 1) for line in text.decode().splitlines() if line)}


def tuning_in_force(lib: C.CDLL) -> dict:
    """czhip_tuning_describe of the calling thread as a dict of ints"""
    lib.czhip_tuning_describe.restype = C.c_char_p
    return _pairs(lib.czhip_tuning_describe())


class DeviceArray:
    """A device-resident S3D array, shape (NJ+4, NI+4, NK+4) K-fastest (czAllocR_S3D, cz.h:209-232)."""

    def __init__(self, hip: "CzHip", sz):
        self.hip, self.sz = hip, tuple(int(v) for v in sz)
        self.shape = (self.sz[1] + 2 * GUIDE, self.sz[0] + 2 * GUIDE, self.sz[2] + 2 * GUIDE)
        self.nbytes = int(np.prod(self.shape)) * hip.real().itemsize
        arr = (C.c_int * 3)(*self.sz)
        self.ptr = hip.lib.czhip_alloc_s3d(arr)

    def put(self, host: np.ndarray):
        assert host.shape == self.shape and host.dtype == self.hip.real
        host = np.ascontiguousarray(host)
        self.hip.lib.czhip_h2d(self.ptr, host.ctypes.data_as(C.c_void_p), self.nbytes)
        return self

    def get(self) -> np.ndarray:
        out = np.empty(self.shape, dtype=self.hip.real)
        self.hip.lib.czhip_d2h(out.ctypes.data_as(C.c_void_p), self.ptr, self.nbytes)
        return out

    def free(self):
        if self.ptr:
            self.hip.lib.czhip_free(self.ptr)
            self.ptr = None


class DeviceBuffer:
    """A small device array of doubles or ints (residual sums, history, convergence flag) for the checked launches of part 3.
    Allocated through czhip_alloc_s3d (zero-filled, on the library's device), so no other allocator or stream is involved."""

    def __init__(self, hip: "CzHip", n: int, dtype):
        self.hip, self.n, self.dtype = hip, int(n), np.dtype(dtype)
        self.nbytes = self.n * self.dtype.itemsize
        k = -(-self.nbytes // (25 * hip.real().itemsize))  # (1+4) x (1+4) x (k+4) REALs hold at least nbytes
        self.ptr = hip.lib.czhip_alloc_s3d((C.c_int * 3)(1, 1, max(k, 1)))

    def put(self, host):
        host = np.ascontiguousarray(host, dtype=self.dtype)
        assert host.size == self.n
        self.hip.lib.czhip_h2d(self.ptr, host.ctypes.data_as(C.c_void_p), self.nbytes)
        return self

    def get(self) -> np.ndarray:
        out = np.empty(self.n, dtype=self.dtype)
        self.hip.lib.czhip_d2h(out.ctypes.data_as(C.c_void_p), self.ptr, self.nbytes)
        return out

    def free(self):
        if self.ptr:
            self.hip.lib.czhip_free(self.ptr)
            self.ptr = None


class CzHip:
    """The drop-in kernels with the reference's argument conventions (everything by pointer)."""

    def __init__(self, prec: str = "f32", device: int = -1):
        self.prec = prec
        self.real = np.float32 if prec == "f32" else np.float64
        self.creal = C.c_float if prec == "f32" else C.c_double
        self.lib = lib = load(prec)
        lib.czhip_alloc_s3d.restype = C.c_void_p
        lib.czhip_alloc_s3d.argtypes = [C.POINTER(C.c_int)]
        lib.czhip_free.argtypes = [C.c_void_p]
        lib.czhip_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        lib.czhip_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        lib.czhip_stream.restype = C.c_void_p
        lib.czhip_arch.restype = C.c_char_p
        assert lib.czhip_real_bytes() == np.dtype(self.real).itemsize
        if lib.czhip_init(int(device)) != 0:
            raise RuntimeError("czhip_init failed")

    # -- helpers
    def alloc(self, sz, host=None) -> DeviceArray:
        a = DeviceArray(self, sz)
        if host is not None:
            a.put(host)
        return a

    @staticmethod
    def _i(v):
        v = np.ascontiguousarray(v, dtype=np.int32)
        return v, v.ctypes.data_as(C.POINTER(C.c_int))

    def _r(self, v):
        v = np.ascontiguousarray(v, dtype=self.real)
        return v, v.ctypes.data_as(C.c_void_p)

    def _s(self, v):
        return C.byref(self.creal(float(v)))

    def set_tuning(self, threads=0, m=0, tj=-1, pf=-1) -> bool:
        return self.lib.czhip_set_tuning(int(threads), int(m), int(tj), int(pf)) == 0

    def sync(self):
        self.lib.czhip_sync()

    # -- part 3 (two fused sweeps)
    def jacobi2(self, u, w, b, sz, idx, cf, omg, idx1=None, read=True):
        """u -> w = two Jacobi sweeps in one launch; returns (launched, res_first, res_second)."""
        (_, szp), (_, idxp), (_, cfp) = self._i(sz), self._i(idx), self._r(cf)
        idx1p = self._i(idx1)[1] if idx1 is not None else None
        if not hasattr(self, "_dres"):
            self._dres = self.lib.czhip_alloc_s3d((C.c_int * 3)(4, 4, 4))
        self.lib.czhip_jacobi2_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                 C.c_void_p, self.creal, C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]
        ok = self.lib.czhip_jacobi2_async(u.ptr, w.ptr, b.ptr, szp, idxp, idx1p, GUIDE, cfp, float(omg), self._dres, 0.0, 0.0, 0,
                                          None, None, None, None)
        if not read:
            return bool(ok), None, None
        out = (C.c_double * 2)()
        self.lib.czhip_d2h(out, self._dres, 16)
        return bool(ok), out[0], out[1]

    def pair_maf(self, u, w, b, sz, idx, x, y, z, omg, rb_ofst=-1):
        """MAF flavour of jacobi2 / rbsor2: u -> w; returns (launched, res_first, res_second) (rb_ofst >= 0: res_first is the iteration's sum)"""
        (_, szp), (_, idxp) = self._i(sz), self._i(idx)
        if not hasattr(self, "_dres"):
            self._dres = self.lib.czhip_alloc_s3d((C.c_int * 3)(4, 4, 4))
        xs = [np.ascontiguousarray(a, dtype=self.real) for a in (x, y, z)]
        self.lib.czhip_pair_maf_async.argtypes = [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 3 + [self.creal, C.c_int, C.c_void_p]
        ok = self.lib.czhip_pair_maf_async(u.ptr, w.ptr, b.ptr, szp, idxp, GUIDE, *[a.ctypes.data_as(C.c_void_p) for a in xs], float(omg), int(rb_ofst),
                                           self._dres)
        out = (C.c_double * 2)()
        self.lib.czhip_d2h(out, self._dres, 16)
        return bool(ok), out[0], out[1]

    def rbsor2(self, u, w, b, sz, idx, cf, ofst, omg, idx1=None):
        """u -> w = one red-black iteration (colour 0 then 1) in one launch; returns (launched, res)."""
        (_, szp), (_, idxp), (_, cfp) = self._i(sz), self._i(idx), self._r(cf)
        idx1p = self._i(idx1)[1] if idx1 is not None else None
        if not hasattr(self, "_dres"):
            self._dres = self.lib.czhip_alloc_s3d((C.c_int * 3)(4, 4, 4))
        self.lib.czhip_rbsor2_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                C.c_void_p, C.c_int, self.creal, C.c_void_p, C.c_double, C.c_double, C.c_int,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        ok = self.lib.czhip_rbsor2_async(u.ptr, w.ptr, b.ptr, szp, idxp, idx1p, GUIDE, cfp, int(ofst), float(omg), self._dres, 0.0,
                                         0.0, 0, None, None, None, None)
        out = (C.c_double * 2)()
        self.lib.czhip_d2h(out, self._dres, 16)
        return bool(ok), out[0]

    def _deep(self, kind, n, u, w, b, sz, idx, cf, omg, probe, ofst=None, ck=None):
        """czhip_<kind>_async (rbsor4 | jacobi3 | jacobi4; ofst: the red-black entry's extra argument).  ck None: a bare launch, returns
        (launched, its n sums); else with ck's bookkeeping or skip flag (pass_checked), returns launched"""
        (_, szp), (_, idxp), (_, cfp) = self._i(sz), self._i(idx), self._r(cf)
        if ck is None and not hasattr(self, "_dres"):
            self._dres = self.lib.czhip_alloc_s3d((C.c_int * 3)(4, 4, 4))
        f = getattr(self.lib, f"czhip_{kind}_async")
        f.argtypes = ([C.c_void_p] * 5 + [C.c_int, C.c_void_p] + ([C.c_int] if ofst is not None else []) + [self.creal, C.c_void_p, C.c_double, C.c_double,
                      C.c_int] + [C.c_void_p] * 4 + [C.c_int])
        tail = (self._dres, 0.0, 0.0, 0, None, None, None, None) if ck is None else (*self._ck(ck), ck["skip"].ptr if ck.get("skip") is not None else None)
        ok = bool(f(u.ptr, w.ptr, b.ptr, szp, idxp, GUIDE, cfp, *([int(ofst)] if ofst is not None else []), float(omg), *tail, int(probe)))
        if ck is not None:
            return ok
        out = (C.c_double * n)()
        self.lib.czhip_d2h(out, self._dres, 8 * n)
        return (ok, *out)

    def rbsor4(self, u, w, b, sz, idx, cf, ofst, omg, probe=0):
        """u -> w = TWO red-black iterations (colour 0, 1, 0, 1) in one launch (rb4_k); returns (launched, res of iteration 1, of iteration 2)."""
        return self._deep("rbsor4", 2, u, w, b, sz, idx, cf, omg, probe, ofst=ofst)

    def jacobi3(self, u, w, b, sz, idx, cf, omg, probe=0):
        """u -> w = THREE Jacobi sweeps in one launch (jac3_k); returns (launched, res of sweep 1, 2, 3)."""
        return self._deep("jacobi3", 3, u, w, b, sz, idx, cf, omg, probe)

    def jacobi4(self, u, w, b, sz, idx, cf, omg, probe=0):
        """u -> w = FOUR Jacobi sweeps in one launch (jac4_k); returns (launched, res of sweep 1, 2, 3, 4)."""
        return self._deep("jacobi4", 4, u, w, b, sz, idx, cf, omg, probe)

    def jac4_plan(self, u, w, b, sz, idx, cf, omg):
        """the geometry jac4_k would run the box with (czhip_jac4_plan), or None where the pass does not take it"""
        (_, szp), (_, idxp), (_, cfp) = self._i(sz), self._i(idx), self._r(cf)
        out = (C.c_int * 8)()
        self.lib.czhip_jac4_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, self.creal, C.c_void_p]
        if not self.lib.czhip_jac4_plan(u.ptr, w.ptr, b.ptr, szp, idxp, GUIDE, cfp, float(omg), out):
            return None
        return dict(zip(("R", "S", "nwin", "KT", "nsegw", "TJ", "nchunk", "lds"), out))

    def pass_from_zero(self, w, b_out, sz, idx, cf, omg, op=0, x=None, y=None, z=None, a=0.0, bb=0.0, rb_ofst=-1):
        """first pass of a preconditioner solve: start vector a literal zero, right-hand side read (op 0) or made from x, y, z (op 1: a*x + y,
        op 2: x + a*(z - bb*y)) and stored to b_out; two Jacobi sweeps (rb_ofst < 0) or one red-black iteration; returns launched"""
        (_, szp), (_, idxp), (_, cfp) = self._i(sz), self._i(idx), self._r(cf)
        if not hasattr(self, "_dres"):
            self._dres = self.lib.czhip_alloc_s3d((C.c_int * 3)(4, 4, 4))
        f = self.lib.czhip_jacobi2_from_zero_made_async
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, self.creal, self.creal, C.c_void_p, C.c_void_p,
                      C.c_void_p, C.c_int, C.c_void_p, self.creal, C.c_int, C.c_void_p, C.c_int]
        ptr = lambda d: d.ptr if d is not None else None  # noqa: E731
        return bool(f(w.ptr, w.ptr, b_out.ptr, int(op), ptr(x), ptr(y), ptr(z), float(a), float(bb), szp, idxp, None, GUIDE, cfp, float(omg), int(rb_ofst),
                      self._dres, 0))

    def pair_split(self, u, w, b, sz, idx, idx1, nID, cf, omg, rb_ofst=-1, read=True):
        """the fused pass as shell slabs + interior (what a decomposed brick runs); returns (launched, res0, res1)."""
        (_, szp), (_, idxp), (_, idx1p), (_, nidp), (_, cfp) = self._i(sz), self._i(idx), self._i(idx1), self._i(nID), self._r(cf)
        if not hasattr(self, "_dres"):
            self._dres = self.lib.czhip_alloc_s3d((C.c_int * 3)(4, 4, 4))
        self.lib.czhip_pair_split_async.argtypes = [C.c_void_p] * 7 + [C.c_int, C.c_void_p, self.creal, C.c_int, C.c_void_p]
        ok = self.lib.czhip_pair_split_async(u.ptr, w.ptr, b.ptr, szp, idxp, idx1p, nidp, GUIDE, cfp, float(omg), int(rb_ofst), self._dres)
        if not read:  # leave the queue running (timing loops)
            return bool(ok), None, None
        out = (C.c_double * 2)()
        self.lib.czhip_d2h(out, self._dres, 16)
        return bool(ok), out[0], out[1]

    # -- part 3 with the convergence bookkeeping.  ck: dict of device state -- res (DeviceBuffer of doubles: the sums), hist (doubles or None),
    # flag, conv (ints), skip (ints or None) -- and the scalars res_normal, eps, itr
    def dbuf(self, n, dtype=np.float64, fill=None) -> DeviceBuffer:
        d = DeviceBuffer(self, n, dtype)
        if fill is not None:
            d.put(np.full(n, fill, dtype=dtype))
        return d

    @staticmethod
    def _ck(ck):
        p = lambda d: d.ptr if d is not None else None  # noqa: E731
        return (ck["res"].ptr, float(ck.get("res_normal", 0.0)), float(ck.get("eps", 0.0)), int(ck.get("itr", 0)), p(ck.get("hist")),
                p(ck.get("flag")), p(ck.get("conv")))

    def jacobi_checked(self, u, w, b, sz, idx, cf, omg, ck):
        """czhip_jacobi_checked_async: one sweep u -> w, its sum in res[0], the bookkeeping of iteration itr; flag doubles as skip flag"""
        (_, szp), (_, idxp), (_, cfp) = self._i(sz), self._i(idx), self._r(cf)
        f = self.lib.czhip_jacobi_checked_async
        f.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_void_p, self.creal, C.c_void_p, C.c_double, C.c_double, C.c_int] + [C.c_void_p] * 3
        f(u.ptr, w.ptr, b.ptr, szp, idxp, GUIDE, cfp, float(omg), *self._ck(ck))

    def rbsor_async(self, p, b, sz, idx, cf, ofst, color, omg, res, accumulate=0, skip=None):
        """czhip_rbsor_async: one colour in place, sum in res[0] (= or +=); skip: DeviceBuffer of ints or None"""
        (_, szp), (_, idxp), (_, cfp) = self._i(sz), self._i(idx), self._r(cf)
        f = self.lib.czhip_rbsor_async
        f.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_int, C.c_int, self.creal, C.c_void_p, C.c_int, C.c_void_p]
        f(p.ptr, b.ptr, szp, idxp, GUIDE, cfp, int(ofst), int(color), float(omg), res.ptr, int(accumulate), skip.ptr if skip is not None else None)

    def rbsor_checked(self, p, b, sz, idx, cf, ofst, color, omg, accumulate, ck):
        """czhip_rbsor_checked_async: one colour in place with the bookkeeping of iteration itr (the driver passes it with colour 1)"""
        (_, szp), (_, idxp), (_, cfp) = self._i(sz), self._i(idx), self._r(cf)
        f = self.lib.czhip_rbsor_checked_async
        f.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_int, C.c_int, self.creal, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_void_p]
        res, rn, eps, itr, hist, flag, conv = self._ck(ck)
        f(p.ptr, b.ptr, szp, idxp, GUIDE, cfp, int(ofst), int(color), float(omg), res, int(accumulate), rn, eps, itr, hist, flag, conv)

    def pass_checked(self, kind, u, w, b, sz, idx, cf, omg, ck, ofst=0) -> bool:
        """one fused pass u -> w with the bookkeeping of its iterations (hist given) or only a skip flag (hist None, skip given):
        kind jacobi2 | rbsor2 | rbsor4 | jacobi3 | jacobi4; returns launched"""
        (_, szp), (_, idxp), (_, cfp) = self._i(sz), self._i(idx), self._r(cf)
        res, rn, eps, itr, hist, flag, conv = self._ck(ck)
        skip = ck["skip"].ptr if ck.get("skip") is not None else None
        tail = [C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        if kind in ("jacobi2", "rbsor2"):
            f = getattr(self.lib, f"czhip_{kind}_async")
            f.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_void_p] + ([C.c_int] if kind == "rbsor2" else []) + [self.creal] + tail
            mid = [int(ofst)] if kind == "rbsor2" else []
            return bool(f(u.ptr, w.ptr, b.ptr, szp, idxp, None, GUIDE, cfp, *mid, float(omg), res, rn, eps, itr, hist, flag, conv, skip))
        return self._deep(kind, 0, u, w, b, sz, idx, cf, omg, 0, ofst=ofst if kind == "rbsor4" else None, ck=ck)

    def check(self, ck, pair=False):
        """czhip_check_async (pair: czhip_check2_async) on the sums in res"""
        f = self.lib.czhip_check2_async if pair else self.lib.czhip_check_async
        f.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        f(*self._ck(ck))

    def tuning(self) -> dict:
        """the calling thread's kernel switches as czhip_init and the setters left them (czhip_tuning_describe)"""
        return tuning_in_force(self.lib)

    def timing(self, enable: bool):
        """HIP-event timing of the library's launches, per label (czhip_timing)."""
        self.lib.czhip_timing(1 if enable else 0)

    def timing_read(self, label: str):
        """(number of launches, total ms) recorded under `label` since timing was enabled."""
        tot = C.c_double(0.0)
        self.lib.czhip_timing_read.argtypes = [C.c_char_p, C.POINTER(C.c_double)]
        n = self.lib.czhip_timing_read(label.encode(), C.byref(tot))
        return n, tot.value

    def set_tuning2(self, threads=0, mv=0, tj=-1, enable=-1) -> bool:
        return self.lib.czhip_set_tuning2(int(threads), int(mv), int(tj), int(enable)) == 0

    # -- part 1: same call shapes as oracle.cz_oracle.Kernels
    def bc_k(self, sz, p: DeviceArray, dh, org, nID):
        (_, szp), (_, nidp), (_, orgp), g = self._i(sz), self._i(nID), self._r(org), C.c_int(GUIDE)
        self.lib.bc_k_(szp, C.byref(g), C.c_void_p(p.ptr), self._s(dh), orgp, nidp)

    def jacobi(self, p, sz, idx, cf, omg, b, wk2, res=0.0):
        (_, szp), (_, idxp), (_, cfp), g = self._i(sz), self._i(idx), self._r(cf), C.c_int(GUIDE)
        r, fl = C.c_double(res), C.c_double(0.0)
        self.lib.jacobi_(C.c_void_p(p.ptr), szp, idxp, C.byref(g), cfp, self._s(omg), C.c_void_p(b.ptr), C.byref(r),
                         C.c_void_p(wk2.ptr), C.byref(fl))
        self.last_flop = fl.value
        return r.value

    def psor2sma_core(self, p, sz, idx, cf, ofst, color, omg, b, res=0.0):
        (_, szp), (_, idxp), (_, cfp), g = self._i(sz), self._i(idx), self._r(cf), C.c_int(GUIDE)
        r, fl, o, c = C.c_double(res), C.c_double(0.0), C.c_int(ofst), C.c_int(color)
        self.lib.psor2sma_core_(C.c_void_p(p.ptr), szp, idxp, C.byref(g), cfp, C.byref(o), C.byref(c), self._s(omg),
                                C.c_void_p(b.ptr), C.byref(r), C.byref(fl))
        self.last_flop = fl.value
        return r.value

    # MAF flavour: x, y, z are host numpy arrays (length N+4), like the reference's xc, yc, zc
    def jacobi_maf(self, p, sz, idx, x, y, z, omg, b, wk2, res=0.0):
        (_, szp), (_, idxp), g = self._i(sz), self._i(idx), C.c_int(GUIDE)
        (xk, xp), (yk, yp), (zk, zp) = self._r(x), self._r(y), self._r(z)
        tmp = np.zeros(sz[2] + 4, dtype=self.real)
        r, fl = C.c_double(res), C.c_double(0.0)
        self.lib.jacobi_maf_(C.c_void_p(p.ptr), szp, idxp, C.byref(g), xp, yp, zp, self._s(omg), C.c_void_p(b.ptr), C.byref(r),
                             C.c_void_p(wk2.ptr), tmp.ctypes.data_as(C.c_void_p), C.byref(fl))
        self.last_flop = fl.value
        return r.value

    def psor(self, p, sz, idx, cf, omg, b, res=0.0):
        (_, szp), (_, idxp), (_, cfp), g = self._i(sz), self._i(idx), self._r(cf), C.c_int(GUIDE)
        r, fl = C.c_double(res), C.c_double(0.0)
        self.lib.psor_(C.c_void_p(p.ptr), szp, idxp, C.byref(g), cfp, self._s(omg), C.c_void_p(b.ptr), C.byref(r), C.byref(fl))
        self.last_flop = fl.value
        return r.value

    def psor_maf(self, p, sz, idx, x, y, z, omg, b, res=0.0):
        (_, szp), (_, idxp), g = self._i(sz), self._i(idx), C.c_int(GUIDE)
        (xk, xp), (yk, yp), (zk, zp) = self._r(x), self._r(y), self._r(z)
        r, fl = C.c_double(res), C.c_double(0.0)
        self.lib.psor_maf_(C.c_void_p(p.ptr), szp, idxp, C.byref(g), xp, yp, zp, self._s(omg), C.c_void_p(b.ptr), C.byref(r), C.byref(fl))
        self.last_flop = fl.value
        return r.value

    def psor2sma_core_maf(self, p, sz, idx, x, y, z, ofst, color, omg, b, res=0.0):
        (_, szp), (_, idxp), g = self._i(sz), self._i(idx), C.c_int(GUIDE)
        (xk, xp), (yk, yp), (zk, zp) = self._r(x), self._r(y), self._r(z)
        tmp = np.zeros(sz[2] + 4, dtype=self.real)
        r, fl, o, c = C.c_double(res), C.c_double(0.0), C.c_int(ofst), C.c_int(color)
        self.lib.psor2sma_core_maf_(C.c_void_p(p.ptr), szp, idxp, C.byref(g), xp, yp, zp, C.byref(o), C.byref(c), self._s(omg),
                                    C.c_void_p(b.ptr), C.byref(r), tmp.ctypes.data_as(C.c_void_p), C.byref(fl))
        self.last_flop = fl.value
        return r.value

    def calc_rk_maf(self, r, p, b, sz, idx, x, y, z, pvt):
        (_, szp), (_, idxp), g, fl = self._i(sz), self._i(idx), C.c_int(GUIDE), C.c_double(0.0)
        (xk, xp), (yk, yp), (zk, zp) = self._r(x), self._r(y), self._r(z)
        self.lib.calc_rk_maf_(C.c_void_p(r.ptr), C.c_void_p(p.ptr), C.c_void_p(b.ptr), szp, idxp, C.byref(g), xp, yp, zp,
                              C.c_void_p(pvt.ptr), C.byref(fl))

    def calc_ax_maf(self, ap, p, sz, idx, x, y, z, pvt):
        (_, szp), (_, idxp), g, fl = self._i(sz), self._i(idx), C.c_int(GUIDE), C.c_double(0.0)
        (xk, xp), (yk, yp), (zk, zp) = self._r(x), self._r(y), self._r(z)
        self.lib.calc_ax_maf_(C.c_void_p(ap.ptr), C.c_void_p(p.ptr), szp, idxp, C.byref(g), xp, yp, zp, C.c_void_p(pvt.ptr),
                              C.byref(fl))

    def search_pivot(self, pvt, sz, idx, x, y, z):
        (_, szp), (_, idxp), g = self._i(sz), self._i(idx), C.c_int(GUIDE)
        (xk, xp), (yk, yp), (zk, zp) = self._r(x), self._r(y), self._r(z)
        self.lib.search_pivot_(C.c_void_p(pvt.ptr), szp, idxp, C.byref(g), xp, yp, zp)

    def imask_k(self, x, sz, idx):
        (_, szp), (_, idxp), g = self._i(sz), self._i(idx), C.c_int(GUIDE)
        self.lib.imask_k_(C.c_void_p(x.ptr), szp, idxp, C.byref(g))

    def pcr_rb(self, sz, idx, pn, ofst, color, x, msk, rhs, omg, res=0.0):
        (_, szp), (_, idxp), g = self._i(sz), self._i(idx), C.c_int(GUIDE)
        w = [np.zeros(sz[2] + 4, dtype=self.real) for _ in range(6)]
        r, fl, pnc, o, c = C.c_double(res), C.c_double(0.0), C.c_int(pn), C.c_int(ofst), C.c_int(color)
        self.lib.pcr_rb_(szp, idxp, C.byref(g), C.byref(pnc), C.byref(o), C.byref(c), C.c_void_p(x.ptr), C.c_void_p(msk.ptr),
                         C.c_void_p(rhs.ptr), *[v.ctypes.data_as(C.c_void_p) for v in w], self._s(omg), C.byref(r), C.byref(fl))
        self.last_flop = fl.value
        return r.value

    def _pcr_call(self, fn, sz, idx, pn, pre, x, msk, rhs, extra, omg, res):
        (_, szp), (_, idxp), g = self._i(sz), self._i(idx), C.c_int(GUIDE)
        w = [np.zeros(sz[2] + 4, dtype=self.real) for _ in range(6)]  # the reference's host scratch: ignored by the library
        r, fl, pnc = C.c_double(res), C.c_double(0.0), C.c_int(pn)
        ints = [C.c_int(v) for v in pre]
        fn(szp, idxp, C.byref(g), C.byref(pnc), *[C.byref(v) for v in ints], C.c_void_p(x.ptr), C.c_void_p(msk.ptr), C.c_void_p(rhs.ptr),
           *[v.ctypes.data_as(C.c_void_p) for v in w], *[C.c_void_p(e.ptr) for e in extra], self._s(omg), C.byref(r), C.byref(fl))
        self.last_flop = fl.value
        return r.value

    def pcr(self, sz, idx, pn, x, msk, rhs, omg, res=0.0):
        return self._pcr_call(self.lib.pcr_, sz, idx, pn, [], x, msk, rhs, [], omg, res)

    def pcr_eda(self, sz, idx, pn, x, msk, rhs, omg, res=0.0):
        (_, szp), (_, idxp), g = self._i(sz), self._i(idx), C.c_int(GUIDE)
        w = [np.zeros(sz[2] + 4, dtype=self.real) for _ in range(3)]
        r, fl, pnc = C.c_double(res), C.c_double(0.0), C.c_int(pn)
        self.lib.pcr_eda_(szp, idxp, C.byref(g), C.byref(pnc), C.c_void_p(x.ptr), C.c_void_p(msk.ptr), C.c_void_p(rhs.ptr),
                          *[v.ctypes.data_as(C.c_void_p) for v in w], self._s(omg), C.byref(r), C.byref(fl))
        self.last_flop = fl.value
        return r.value

    def pcr_esa(self, sz, idx, pn, x, msk, rhs, omg, res=0.0):
        return self._pcr_call(self.lib.pcr_esa_, sz, idx, pn, [(1 << pn) >> 2], x, msk, rhs, [], omg, res)

    def pcr_rb_esa(self, sz, idx, pn, ofst, color, x, msk, rhs, omg, res=0.0):
        return self._pcr_call(self.lib.pcr_rb_esa_, sz, idx, pn, [ofst, color, (1 << pn) >> 2], x, msk, rhs, [], omg, res)

    def pcr_j_esa(self, sz, idx, pn, x, msk, rhs, src, wrk, omg, res=0.0):
        return self._pcr_call(self.lib.pcr_j_esa_, sz, idx, pn, [(1 << pn) >> 2], x, msk, rhs, [src, wrk], omg, res)

    def pcr_maf(self, name, sz, idx, pn, color, x, msk, rhs, xc, yc, zc, omg, res=0.0):
        """the MAF line solvers: name in pcr_rb_maf, pcr_rb_esa_maf, pcr_maf, pcr_eda_maf, pcr_esa_maf (same call shape as the oracle)"""
        (_, szp), (_, idxp), g = self._i(sz), self._i(idx), C.c_int(GUIDE)
        (xk, xp), (yk, yp), (zk, zp) = self._r(xc), self._r(yc), self._r(zc)
        nw = 3 if name == "pcr_eda_maf" else 6
        w = [np.zeros(sz[2] + 4, dtype=self.real) for _ in range(nw)]
        tmp = np.zeros(sz[2] + 4, dtype=self.real)
        r, fl, pnc = C.c_double(res), C.c_double(0.0), C.c_int(pn)
        o, c, ss = C.c_int(0), C.c_int(color), C.c_int((1 << pn) >> 2)
        pre = {"pcr_rb_maf": [o, c], "pcr_rb_esa_maf": [o, c, ss], "pcr_maf": [], "pcr_eda_maf": [], "pcr_esa_maf": [ss]}[name]
        getattr(self.lib, name + "_")(szp, idxp, C.byref(g), C.byref(pnc), *[C.byref(v) for v in pre], C.c_void_p(x.ptr), C.c_void_p(msk.ptr),
                                      C.c_void_p(rhs.ptr), xp, yp, zp, *[v.ctypes.data_as(C.c_void_p) for v in w], self._s(omg), C.byref(r),
                                      tmp.ctypes.data_as(C.c_void_p), C.byref(fl))
        self.last_flop = fl.value
        return r.value

    def blas_clear(self, x, sz):
        (_, szp), g = self._i(sz), C.c_int(GUIDE)
        self.lib.blas_clear_(C.c_void_p(x.ptr), szp, C.byref(g))

    def blas_copy(self, y, x, sz):
        (_, szp), g = self._i(sz), C.c_int(GUIDE)
        self.lib.blas_copy_(C.c_void_p(y.ptr), C.c_void_p(x.ptr), szp, C.byref(g))

    def blas_triad(self, z, x, y, a, sz, idx):
        (_, szp), (_, idxp), g, fl = self._i(sz), self._i(idx), C.c_int(GUIDE), C.c_double(0.0)
        self.lib.blas_triad_(C.c_void_p(z.ptr), C.c_void_p(x.ptr), C.c_void_p(y.ptr), self._s(a), szp, idxp, C.byref(g),
                             C.byref(fl))

    def blas_dot1(self, p, sz, idx):
        (_, szp), (_, idxp), g, fl = self._i(sz), self._i(idx), C.c_int(GUIDE), C.c_double(0.0)
        r = self.creal(0.0)
        self.lib.blas_dot1_(C.byref(r), C.c_void_p(p.ptr), szp, idxp, C.byref(g), C.byref(fl))
        return self.real(r.value)

    def blas_dot2(self, p, q, sz, idx):
        (_, szp), (_, idxp), g, fl = self._i(sz), self._i(idx), C.c_int(GUIDE), C.c_double(0.0)
        r = self.creal(0.0)
        self.lib.blas_dot2_(C.byref(r), C.c_void_p(p.ptr), C.c_void_p(q.ptr), szp, idxp, C.byref(g), C.byref(fl))
        return self.real(r.value)

    def blas_bicg_1(self, p, r, q, beta, omg, sz, idx):
        (_, szp), (_, idxp), g, fl = self._i(sz), self._i(idx), C.c_int(GUIDE), C.c_double(0.0)
        self.lib.blas_bicg_1_(C.c_void_p(p.ptr), C.c_void_p(r.ptr), C.c_void_p(q.ptr), self._s(beta), self._s(omg), szp,
                              idxp, C.byref(g), C.byref(fl))

    def blas_bicg_2(self, z, x, y, a, b, sz, idx):
        (_, szp), (_, idxp), g, fl = self._i(sz), self._i(idx), C.c_int(GUIDE), C.c_double(0.0)
        self.lib.blas_bicg_2_(C.c_void_p(z.ptr), C.c_void_p(x.ptr), C.c_void_p(y.ptr), self._s(a), self._s(b), szp, idxp,
                              C.byref(g), C.byref(fl))

    def blas_calc_ax(self, ap, p, sz, idx, cf):
        (_, szp), (_, idxp), (_, cfp), g, fl = self._i(sz), self._i(idx), self._r(cf), C.c_int(GUIDE), C.c_double(0.0)
        self.lib.blas_calc_ax_(C.c_void_p(ap.ptr), C.c_void_p(p.ptr), szp, idxp, C.byref(g), cfp, C.byref(fl))

    def blas_calc_rk(self, r, p, b, sz, idx, cf):
        (_, szp), (_, idxp), (_, cfp), g, fl = self._i(sz), self._i(idx), self._r(cf), C.c_int(GUIDE), C.c_double(0.0)
        self.lib.blas_calc_rk_(C.c_void_p(r.ptr), C.c_void_p(p.ptr), C.c_void_p(b.ptr), szp, idxp, C.byref(g), cfp,
                               C.byref(fl))

    # -- the multigrid V-cycle of pcg ... mg: level kernels on arrays of guide 2, and the hierarchy handle
    def mg_smooth(self, u, w, b, sz, idx, level, n0, omg) -> bool:
        """w = one level-`level` relaxed Jacobi sweep from u (u None: from zero)"""
        (_, szp), (_, idxp), (_, n0p) = self._i(sz), self._i(idx), self._i(n0)
        f = self.lib.czhip_mg_smooth_async
        f.argtypes = [C.c_void_p] * 3 + [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, self.creal]
        return bool(f(u.ptr if u is not None else None, w.ptr, b.ptr, szp, idxp, GUIDE, int(level), n0p, float(omg)))

    def mg_restrict(self, bc, szc, idxc, x, b, sz, idx, level, n0) -> bool:
        (_, szcp), (_, idxcp), (_, szp), (_, idxp), (_, n0p) = self._i(szc), self._i(idxc), self._i(sz), self._i(idx), self._i(n0)
        f = self.lib.czhip_mg_restrict_async
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        return bool(f(bc.ptr, szcp, idxcp, x.ptr, b.ptr, szp, idxp, GUIDE, int(level), n0p))

    def mg_prolong(self, u, x, xc, szc, idxc, sz, idx, level, n0) -> bool:
        (_, szcp), (_, idxcp), (_, szp), (_, idxp), (_, n0p) = self._i(szc), self._i(idxc), self._i(sz), self._i(idx), self._i(n0)
        f = self.lib.czhip_mg_prolong_async
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        return bool(f(u.ptr, x.ptr, xc.ptr, szcp, idxcp, szp, idxp, GUIDE, int(level), n0p))

    def mg_tail(self, x, b, sz, idx, level, n0, omg) -> bool:
        (_, szp), (_, idxp), (_, n0p) = self._i(sz), self._i(idx), self._i(n0)
        f = self.lib.czhip_mg_tail_async
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, self.creal]
        return bool(f(x.ptr, b.ptr, szp, idxp, GUIDE, int(level), n0p, float(omg)))

    def mg_create(self, sz, idx, cf=(1, 1, 1, 1, 1, 1, 6)):
        """the hierarchy handle (None when refused)"""
        (_, szp), (_, idxp), (_, cfp) = self._i(sz), self._i(idx), self._r(cf)
        self.lib.czhip_mg_create.restype = C.c_void_p
        self.lib.czhip_mg_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        return self.lib.czhip_mg_create(szp, idxp, GUIDE, cfp)

    # -- the same cycle with the symmetric red-black smoother (pcg ... mgrb)
    def mg_rb(self, x, b, sz, idx, level, n0, omg, colour, zero=0) -> bool:
        """one colour sweep of level `level` (>= 1) in place on x; zero: 0 from the iterate, 1 / 2 the first / second colour from zero"""
        (_, szp), (_, idxp), (_, n0p) = self._i(sz), self._i(idx), self._i(n0)
        f = self.lib.czhip_mg_rb_async
        f.argtypes = [C.c_void_p] * 2 + [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, self.creal, C.c_int, C.c_int]
        return bool(f(x.ptr, b.ptr, szp, idxp, GUIDE, int(level), n0p, float(omg), int(colour), int(zero)))

    def mg_tail_rb(self, x, b, sz, idx, level, n0, omg) -> bool:
        (_, szp), (_, idxp), (_, n0p) = self._i(sz), self._i(idx), self._i(n0)
        f = self.lib.czhip_mg_tail_rb_async
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, self.creal]
        return bool(f(x.ptr, b.ptr, szp, idxp, GUIDE, int(level), n0p, float(omg)))

    def mg_create_rb(self, sz, idx, cf=(1, 1, 1, 1, 1, 1, 6)):
        """the hierarchy handle with the red-black smoother (None when refused); mg_levels, mg_apply and mg_destroy serve it too"""
        (_, szp), (_, idxp), (_, cfp) = self._i(sz), self._i(idx), self._r(cf)
        self.lib.czhip_mg_create_rb.restype = C.c_void_p
        self.lib.czhip_mg_create_rb.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        return self.lib.czhip_mg_create_rb(szp, idxp, GUIDE, cfp)

    def mg_kind(self, h) -> int:
        self.lib.czhip_mg_kind.argtypes = [C.c_void_p]
        return self.lib.czhip_mg_kind(h)

    # -- zero-flux (Neumann) faces
    def mirror_faces(self, p, sz, idx, faces) -> bool:
        """the face layers of the flagged physical faces of p (X-, X+, Y-, Y+, Z-, Z+) = the mirror of the first inner layers, one launch"""
        (_, szp), (_, idxp), (_, fp) = self._i(sz), self._i(idx), self._i(faces)
        f = self.lib.czhip_mirror_faces_async
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        return bool(f(p.ptr, szp, idxp, GUIDE, fp))

    # -- the closed box
    def shift_sums(self, a, m_dev, sz, idx, sums_dev) -> bool:
        """a <- a - *m_dev over the inner box (m_dev None: a is only read); sums_dev[0] = sum a', sums_dev[1] = sum a'^2 (doubles)"""
        (_, szp), (_, idxp) = self._i(sz), self._i(idx)
        f = self.lib.czhip_shift_sums_async
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        return bool(f(a.ptr, m_dev.ptr if m_dev is not None else None, szp, idxp, GUIDE, sums_dev.ptr))

    def cg_update_closed(self, x, r, p, q, sc_dev, sz, idx, dots_dev):
        """x = alpha p + x, r = ((-alpha) q + r) - m with sc_dev = (alpha, -alpha, -, -, m) REALs; dots_dev[0] = r.r, dots_dev[1] = sum r"""
        (_, szp), (_, idxp) = self._i(sz), self._i(idx)
        f = self.lib.czhip_cg_update_closed_async
        f.argtypes = [C.c_void_p] * 5 + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        f.restype = None
        f(x.ptr, r.ptr, p.ptr, q.ptr, sc_dev.ptr, szp, idxp, GUIDE, dots_dev.ptr)

    # -- periodic directions
    def fill_faces(self, p, sz, idx, kinds) -> bool:
        """the face layers of p listed in kinds (X-, X+, Y-, Y+, Z-, Z+: 0 leave, 1 mirror, 2 wrap) in one launch; False: refused"""
        (_, szp), (_, idxp), (_, kp) = self._i(sz), self._i(idx), self._i(kinds)
        f = self.lib.czhip_fill_faces_async
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        return bool(f(p.ptr, szp, idxp, GUIDE, kp))

    def mg_set_periodic(self, h, dirs) -> bool:
        """the hierarchy's cycles wrap these directions (X, Y, Z) from now on (all zero: none)"""
        (_, dp) = self._i(dirs)
        f = self.lib.czhip_mg_set_periodic
        f.argtypes = [C.c_void_p, C.c_void_p]
        return bool(f(h, dp))

    def mg_set_neumann(self, h, faces) -> bool:
        """the hierarchy's cycles take these faces as zero-flux faces from now on (all zero: none)"""
        (_, fp) = self._i(faces)
        f = self.lib.czhip_mg_set_neumann
        f.argtypes = [C.c_void_p, C.c_void_p]
        return bool(f(h, fp))

    def mg_levels(self, h) -> int:
        self.lib.czhip_mg_levels.argtypes = [C.c_void_p]
        return self.lib.czhip_mg_levels(h)

    def mg_apply(self, h, z, r, omg) -> bool:
        f = self.lib.czhip_mg_apply_async
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, self.creal]
        return bool(f(h, z.ptr, r.ptr, float(omg)))

    def mg_destroy(self, h):
        self.lib.czhip_mg_destroy.argtypes = [C.c_void_p]
        self.lib.czhip_mg_destroy(h)
