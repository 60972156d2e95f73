"""ctypes binding of parts 4-5 of include/cz_hip.h: the restated CubeZ driver (class CZ) behind a handle.

Mirrors the reference CLI (src/main.cpp:15-60): ``CZ(prec).evaluate(["64","64","64","jacobi","4000","0.8"])``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .lib import GUIDE, JAC4_LABEL, LABELS, _pairs, load, tuning_in_force


class CZ:
    def __init__(self, prec: str = "f32", quiet: bool = True, device: int = -1):
        self.prec = prec
        self.real = np.float32 if prec == "f32" else np.float64
        self.lib = lib = load(prec)
        lib.cz_create.restype = C.c_void_p
        for name in ("cz_destroy", "cz_solve", "cz_result_iter"):
            getattr(lib, name).argtypes = [C.c_void_p]
        lib.cz_evaluate.argtypes = lib.cz_setup.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p)]
        lib.cz_sweeps.argtypes = [C.c_void_p, C.c_int]
        lib.cz_result_res.argtypes = [C.c_void_p]
        lib.cz_result_res.restype = C.c_double
        lib.cz_history.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int]
        lib.cz_field.argtypes = [C.c_void_p, C.c_void_p]
        lib.cz_local_size.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 4
        lib.cz_error_max.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        lib.cz_error_max.restype = C.c_double
        lib.cz_set_quiet.argtypes = lib.cz_set_debug.argtypes = [C.c_void_p, C.c_int]
        lib.cz_last_solve_seconds.argtypes = [C.c_void_p]
        lib.cz_last_solve_seconds.restype = C.c_double
        lib.cz_kernel_ms.argtypes = [C.c_void_p, C.c_char_p]
        lib.cz_kernel_ms.restype = C.c_double
        lib.czhip_timing_read.argtypes = [C.c_char_p, C.POINTER(C.c_double)]
        lib.cz_info.argtypes = [C.c_void_p, C.c_int]
        lib.cz_config_in_force.argtypes = [C.c_void_p]
        lib.cz_config_in_force.restype = C.c_char_p
        lib.cz_precondition.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        for name in ("cz_set_rhs", "cz_set_field", "cz_get_field"):
            getattr(lib, name).argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_longlong), C.c_int, C.c_void_p]
        lib.cz_get_residual.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_longlong), C.c_int, C.c_void_p, C.c_double, C.POINTER(C.c_double)]
        lib.cz_add_field.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_longlong), C.c_int, C.c_void_p, C.c_double]
        lib.cz_set_rhs_div.argtypes = [C.c_void_p] * 4 + [C.POINTER(C.c_longlong), C.c_int, C.c_void_p, C.c_double, C.POINTER(C.c_double)]
        lib.cz_sub_grad.argtypes = [C.c_void_p] * 4 + [C.POINTER(C.c_longlong), C.c_int, C.c_void_p, C.c_double]
        lib.cz_set_face_coef.argtypes = [C.c_void_p] * 4 + [C.POINTER(C.c_longlong), C.c_int, C.c_void_p]
        lib.cz_set_coef_mg.argtypes = [C.c_void_p, C.c_int]
        lib.cz_set_mg_lines.argtypes = [C.c_void_p, C.c_int]
        lib.cz_set_eps.argtypes = [C.c_void_p, C.c_double]
        lib.cz_set_neumann.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        lib.cz_set_closed_box.argtypes = [C.c_void_p, C.c_int]
        lib.cz_set_periodic.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        lib.cz_closed_mean.argtypes = [C.c_void_p, C.c_int]
        lib.cz_closed_mean.restype = C.c_double
        lib.cz_set_itr_max.argtypes = [C.c_void_p, C.c_int]
        self.device = int(device)
        if lib.czhip_init(int(device)) != 0:
            raise RuntimeError("czhip_init failed")
        self.h = lib.cz_create()
        lib.cz_set_quiet(self.h, 1 if quiet else 0)

    @staticmethod
    def _argv(args):
        argv = [b"cz"] + [str(a).encode() for a in args]
        arr = (C.c_char_p * len(argv))(*argv)
        return len(argv), arr

    def evaluate(self, args) -> int:
        n, arr = self._argv(args)
        return self.lib.cz_evaluate(self.h, n, arr)

    def setup(self, args) -> int:
        n, arr = self._argv(args)
        return self.lib.cz_setup(self.h, n, arr)

    def solve(self) -> int:
        return self.lib.cz_solve(self.h)

    def sweeps(self, n: int) -> int:
        return self.lib.cz_sweeps(self.h, int(n))

    @property
    def iter(self) -> int:
        return self.lib.cz_result_iter(self.h)

    @property
    def res(self) -> float:
        return self.lib.cz_result_res(self.h)

    @property
    def solve_seconds(self) -> float:
        return self.lib.cz_last_solve_seconds(self.h)

    def history(self):
        n = self.lib.cz_history(self.h, None, 0)
        out = (C.c_double * max(n, 1))()
        self.lib.cz_history(self.h, out, n)
        return [out[i] for i in range(n)]

    def history_text(self) -> str:
        return "Itration      Residual\n" + "".join("%6d, %13.6e\n" % (i + 1, r) for i, r in enumerate(self.history()))

    def local(self):
        a = [(C.c_int * 3)(), (C.c_int * 3)(), (C.c_int * 6)(), (C.c_int * 6)()]
        self.lib.cz_local_size(self.h, *a)
        return dict(size=list(a[0]), head=list(a[1]), nID=list(a[2]), inner=list(a[3]))

    def field(self) -> np.ndarray:
        sz = self.local()["size"]
        out = np.empty((sz[1] + 2 * GUIDE, sz[0] + 2 * GUIDE, sz[2] + 2 * GUIDE), dtype=self.real)
        self.lib.cz_field(self.h, out.ctypes.data_as(C.c_void_p))
        return out

    # -- the caller's own problem (cz_set_rhs / cz_set_field / cz_get_field of include/cz_hip.h): arrays of this rank's brick, shape
    # local()["size"] = (ni, nj, nk), indexed [i, j, k], any positive strides.  A numpy array goes the host path; anything with data_ptr(),
    # stride(), dtype, device and is_cuda (a torch tensor on the handle's GPU) is read / written in place on the device, handed over on
    # torch's current stream.
    # any_real (get_residual, add_field): the array may hold float32 or float64 whatever the handle's precision.
    def _brick(self, a, what, any_real=False):
        shape = tuple(self.local()["size"])
        names = ("float32", "float64") if any_real else (np.dtype(self.real).name,)
        if isinstance(a, np.ndarray):
            if a.dtype.name not in names:
                raise ValueError(f"{what}: dtype {a.dtype}, this handle is {np.dtype(self.real)}")
            if tuple(a.shape) != shape:
                raise ValueError(f"{what}: shape {tuple(a.shape)}, this rank's brick is {shape}")
            if any(st % a.itemsize or st < a.itemsize for st in a.strides):
                raise ValueError(f"{what}: strides {a.strides} are not positive multiples of the element size")
            return a.ctypes.data, [st // a.itemsize for st in a.strides], 0, None, None
        if not all(hasattr(a, n) for n in ("data_ptr", "stride", "dtype", "device", "is_cuda")):
            raise ValueError(f"{what}: a numpy array or a device tensor (data_ptr, stride, dtype, device, is_cuda) is needed")
        if str(a.dtype).split(".")[-1] not in names:
            raise ValueError(f"{what}: dtype {a.dtype}, this handle is {np.dtype(self.real)}")
        if tuple(a.shape) != shape:
            raise ValueError(f"{what}: shape {tuple(a.shape)}, this rank's brick is {shape}")
        import torch  # (only on this path: the package imports without it)
        mine = self.device if self.device >= 0 else torch.cuda.current_device()
        if not a.is_cuda or a.device.index != mine:
            raise ValueError(f"{what}: tensor on {a.device}, this handle runs on GPU {mine}")
        strides = [int(v) for v in a.stride()]
        if min(strides) < 1:
            raise ValueError(f"{what}: strides {strides} must be positive")
        ts = torch.cuda.current_stream(a.device)
        # torch's default stream is handle 0, which the C interface reads as "no stream to hand over on": wait for that stream (not the device)
        # before an import, and let the library wait for its kernel after an export
        return a.data_ptr(), strides, 1, ts.cuda_stream or None, ts

    def _io(self, fn, a, what):
        ptr, strides, on_dev, stream, ts = self._brick(a, what)
        if on_dev and stream is None:
            ts.synchronize()
        if fn(self.h, C.c_void_p(ptr), (C.c_longlong * 3)(*strides), on_dev, C.c_void_p(stream) if stream else None) != 1:
            raise RuntimeError(f"{what}: refused (see stderr)")

    def set_rhs(self, a):
        """the right-hand side b of  sum of the six neighbours - 6 p = b  on this rank's brick (collective in a decomposed run)"""
        self._io(self.lib.cz_set_rhs, a, "set_rhs")

    def set_field(self, a):
        """Dirichlet values (the layers on physical sides) and the initial guess (collective in a decomposed run)"""
        self._io(self.lib.cz_set_field, a, "set_field")

    def get_field(self, out=None):
        """the current iterate of this rank's brick into `out` (default: a new C-order numpy array [i, j, k]); returns it"""
        if out is None:
            out = np.empty(tuple(self.local()["size"]), dtype=self.real)
        self._io(self.lib.cz_get_field, out, "get_field")
        return out

    # -- mixed-precision refinement (cz_get_residual / cz_add_field of include/cz_hip.h)
    def get_residual(self, out=None, dtype=None, scale=1.0):
        """(out, sumsq): out = (r * scale) of the true residual r = b - A p of the iterate in the handle on this rank's brick (0 on Dirichlet
        faces), as float32 or float64 whatever the handle's precision; sumsq = the sum of r^2 (unscaled, in double) over the whole domain.
        out: a numpy array or a device tensor; None with a dtype: a new C-order numpy array; None without: the norm only, (None, sumsq).
        Collective in a decomposed run."""
        if out is None and dtype is not None:
            out = np.empty(tuple(self.local()["size"]), dtype=np.dtype(dtype))
        ss = C.c_double(0.0)
        if out is None:
            ok = self.lib.cz_get_residual(self.h, None, 0, None, 0, None, float(scale), C.byref(ss))
        else:
            ptr, strides, on_dev, stream, ts = self._brick(out, "get_residual", any_real=True)
            if on_dev and stream is None:
                ts.synchronize()
            ok = self.lib.cz_get_residual(self.h, C.c_void_p(ptr), self._itemsize(out), (C.c_longlong * 3)(*strides), on_dev,
                                          C.c_void_p(stream) if stream else None, float(scale), C.byref(ss))
        if ok != 1:
            raise RuntimeError("get_residual: refused (see stderr)")
        return out, ss.value

    def add_field(self, a, scale=1.0):
        """p = p + a * scale on the cells every sweep updates (a: float32 or float64, numpy array or device tensor); Dirichlet faces are not
        written (collective in a decomposed run)"""
        ptr, strides, on_dev, stream, ts = self._brick(a, "add_field", any_real=True)
        if on_dev and stream is None:
            ts.synchronize()
        if self.lib.cz_add_field(self.h, C.c_void_p(ptr), self._itemsize(a), (C.c_longlong * 3)(*strides), on_dev,
                                 C.c_void_p(stream) if stream else None, float(scale)) != 1:
            raise RuntimeError("add_field: refused (see stderr)")

    # -- the projection step on a staggered velocity (cz_set_rhs_div / cz_sub_grad of include/cz_hip.h): u, v, w of the brick's
    # shape, u[i, j, k] the normal velocity on the face between cells i and i + 1 (the last entry along its own direction is never touched),
    # v and w the same along j and k; three arrays of equal strides (three tensors of one layout, or vel[..., 0], vel[..., 1], vel[..., 2])
    def _velocity(self, u, v, w, what):
        parts = [self._brick(a, f"{what}: {n}") for a, n in zip((u, v, w), "uvw")]
        ptr0, strides, on_dev, stream, ts = parts[0]
        if any(q[1] != strides for q in parts[1:]):
            raise ValueError(f"{what}: the three components must have equal strides, not {[q[1] for q in parts]}")
        if any(q[2] != on_dev for q in parts[1:]):
            raise ValueError(f"{what}: the three components must be all numpy arrays or all device tensors")
        if on_dev and stream is None:
            ts.synchronize()
        return [C.c_void_p(q[0]) for q in parts], (C.c_longlong * 3)(*strides), on_dev, C.c_void_p(stream) if stream else None

    def set_rhs_div(self, u, v, w, scale=1.0, want_norm=True):
        """the right-hand side b = (discrete divergence of the staggered velocity) * scale at the inner cells, 0 elsewhere, and what set_rhs does
        after its import; returns the sum of div^2 (unscaled, in double) over the inner cells, or None with want_norm=False (then device
        tensors are handed over on torch's current stream without a host wait).  Single domain"""
        ptrs, strides, on_dev, stream = self._velocity(u, v, w, "set_rhs_div")
        ss = C.c_double(0.0)
        if self.lib.cz_set_rhs_div(self.h, *ptrs, strides, on_dev, stream, float(scale), C.byref(ss) if want_norm else None) != 1:
            raise RuntimeError("set_rhs_div: refused (see stderr)")
        return ss.value if want_norm else None

    def sub_grad(self, u, v, w, scale=1.0):
        """u[i, j, k] -= (p[i + 1, j, k] - p[i, j, k]) * scale on the faces at inner j, k, in place (p: the field in the handle, its face layers
        the mirror / the wrap / the Dirichlet values); v and w the same along j and k.  Single domain"""
        ptrs, strides, on_dev, stream = self._velocity(u, v, w, "sub_grad")
        if self.lib.cz_sub_grad(self.h, *ptrs, strides, on_dev, stream, float(scale)) != 1:
            raise RuntimeError("sub_grad: refused (see stderr)")

    def project(self, u, v, w):
        """the projection step: set_rhs_div, solve, sub_grad at scale 1 (a uniform scale cancels between the two: A p = s div u and
        u -= grad p / s); returns (iterations, sum of div^2 before).  Afterwards the divergence of (u, v, w) is the residual of the solve.
        (0, 0.0) means nothing was to be projected: the velocity was discretely divergence-free already (a fluid at rest) and the solve
        stopped before it touched the field (info()["void_start"] == 1).  sub_grad is called whatever the iteration count: it subtracts the
        gradient of whatever field the handle holds -- after a solve that stopped at a breakdown that is the field from before the
        breakdown (the caller's own at iteration 1), never a half-made iterate.  0 iterations with a non-zero sum: a divergence below the
        solver's absolute threshold (void_start 1), or an error"""
        ss = self.set_rhs_div(u, v, w)
        itr = self.solve()
        self.sub_grad(u, v, w)
        return itr, ss

    def set_face_coef(self, bx, by=None, bz=None):
        """face coefficients for pcg: div(beta grad p) = b with beta given on the faces -- bx, by, bz laid out as u, v, w of set_rhs_div
        (bx[i, j, k] on the face between cells i and i + 1; three numpy arrays or device tensors of equal strides), finite and positive on
        every face the operator reads.  The values are copied: the arrays are the caller's again on return.  From then on solve (pcg only),
        get_residual and sub_grad take the variable operator, the preconditioner is the constant one inside a diagonal scaling, and
        info()["face_coef"] is 1.  set_face_coef(None) goes back to the unit coefficients.  A value that is not finite and positive is
        refused and leaves the handle WITHOUT coefficients.  Single domain (cz_set_face_coef of include/cz_hip.h)"""
        if bx is None and by is None and bz is None:
            if self.lib.cz_set_face_coef(self.h, None, None, None, None, 0, None) != 1:
                raise RuntimeError("set_face_coef(None): refused (see stderr)")
            return
        if bx is None or by is None or bz is None:
            raise ValueError("set_face_coef: bx, by and bz, or None alone")
        ptrs, strides, on_dev, stream = self._velocity(bx, by, bz, "set_face_coef")
        if self.lib.cz_set_face_coef(self.h, *ptrs, strides, on_dev, stream) != 1:
            raise RuntimeError("set_face_coef: refused (see stderr)")

    def set_coef_mg(self, on=True):
        """the face coefficients inside the multigrid hierarchy: pcg ... mg | mgrb then preconditions with the V-cycle of the variable operator
        itself, whose coarse levels carry the summed face coefficients, in place of the constant cycle inside the diagonal scaling -- the
        preconditioner for large jumps (a density ratio of 1000).  The flag is remembered across set_face_coef and the boundary setters,
        which rebuild the hierarchy; info()["coef_mg"] is 1 while it is in force (flag on, coefficients set, mg or mgrb); setup clears it.
        Raises where the library refuses; a coarse weight that overflows is such a refusal, and it turns the flag off while the
        coefficients stay (cz_set_coef_mg of include/cz_hip.h)"""
        if self.lib.cz_set_coef_mg(self.h, 1 if on else 0) != 1:
            raise RuntimeError(f"set_coef_mg({bool(on)}): refused (see stderr)")

    def set_mg_lines(self, on=True):
        """zebra line iterations along Z in the V-cycle of pcg ... mgrb, for a grid refined towards a wall (cell aspect ratios of 30 and
        more, where point smoothers stall): lay the refined direction on Z.  The flag is remembered; info()["mg_lines"] is 1 while it is
        in force (flag on, info()["coef_mg"] 1, mgrb); with mg, jacobi or none it is accepted and idle; setup clears it.  Raises where the
        library refuses: before setup, a decomposed run, a coefficient above 1 (cz_set_mg_lines of include/cz_hip.h)"""
        if self.lib.cz_set_mg_lines(self.h, 1 if on else 0) != 1:
            raise RuntimeError(f"set_mg_lines({bool(on)}): refused (see stderr)")

    @staticmethod
    def _itemsize(a):
        return a.itemsize if isinstance(a, np.ndarray) else a.element_size()

    def set_eps(self, eps: float):
        if self.lib.cz_set_eps(self.h, float(eps)) != 1:
            raise ValueError(f"set_eps({eps}): refused")

    def set_neumann(self, faces):
        """zero-flux (Neumann) faces for pcg: six flags in the order X-, X+, Y-, Y+, Z-, Z+ of the global box, at least one of them zero (a
        Dirichlet face); after setup, collective with the same mask on every rank.  The face layers of the field there hold the mirror of the
        first inner layer from now on (cz_set_neumann of include/cz_hip.h)"""
        f = [1 if v else 0 for v in faces]
        if len(f) != 6:
            raise ValueError(f"set_neumann: six flags (X-, X+, Y-, Y+, Z-, Z+), not {len(f)}")
        if self.lib.cz_set_neumann(self.h, (C.c_int * 6)(*f)) != 1:
            raise ValueError(f"set_neumann({f}): refused (see stderr)")

    def set_closed_box(self, on=True):
        """the closed box for pcg: all six faces zero-flux; the right-hand side in the handle (and every later set_rhs) loses its mean, the
        solve keeps its residual in the range of the operator and returns a field of zero mean; after setup, collective with the same value
        on every rank.  on=False: Dirichlet faces again, the right-hand side stays projected (cz_set_closed_box of include/cz_hip.h,
        DESIGN.md §5.14)"""
        if self.lib.cz_set_closed_box(self.h, 1 if on else 0) != 1:
            raise ValueError(f"set_closed_box({bool(on)}): refused (see stderr)")

    def set_periodic(self, dirs):
        """periodic directions for pcg: three flags in the order X, Y, Z of the global box; after setup, collective with the same flags on every
        rank.  The two face layers of the field in such a direction hold the wrap from now on, and its Neumann flags are ignored.  With the
        closed box off, some face of a direction that is not periodic must stay a Dirichlet face: set_closed_box() first for the channel
        (1, 0, 1) and the triply periodic box (1, 1, 1) (cz_set_periodic of include/cz_hip.h)"""
        d = [1 if v else 0 for v in dirs]
        if len(d) != 3:
            raise ValueError(f"set_periodic: three flags (X, Y, Z), not {len(d)}")
        if self.lib.cz_set_periodic(self.h, (C.c_int * 3)(*d)) != 1:
            raise ValueError(f"set_periodic({d}): refused (see stderr)")

    def closed_mean(self, which: int) -> float:
        """the mean last removed in closed-box mode: 0 from the right-hand side, 1 from the initial residual of the last solve, 2 from its
        answer (NaN for another `which`)"""
        return float(self.lib.cz_closed_mean(self.h, int(which)))

    def set_itr_max(self, n: int):
        if self.lib.cz_set_itr_max(self.h, int(n)) != 1:
            raise ValueError(f"set_itr_max({n}): refused")

    def global_slice(self):
        """this rank's brick within an array of the whole domain indexed [i, j, k]"""
        from .decomp import brick_slice
        loc = self.local()
        return brick_slice(loc["size"], loc["head"])

    def error_max(self):
        loc = (C.c_int * 3)()
        d = self.lib.cz_error_max(self.h, loc)
        return d, tuple(loc)

    def info(self) -> dict:
        """what a (multi-GPU) run decided (cz_info of include/cz_hip.h)"""
        keys = ("ranks", "fused_pass", "shell_slabs", "overlap", "lagged_reduce", "rccl_ranks", "comm_cus", "pass_kind", "exchange_depth", "buffers", "bicg_fused", "rb4_passes",
                "exact_reruns", "cg_fused", "jac3_passes", "mg_levels", "mg_cycles", "mg_gather_level", "mg_exchanges", "mg_smoother", "field_form", "neumann", "closed", "periodic", "void_start",
                "face_coef", "jac4_passes", "coef_mg", "mg_lines")
        return {k: self.lib.cz_info(self.h, i) for i, k in enumerate(keys)}

    def config_in_force(self) -> dict:
        """the driver's and its communicator's copies of their own switches (cz_config_in_force of include/cz_hip.h)"""
        return _pairs(self.lib.cz_config_in_force(self.h))

    def tuning(self) -> dict:
        """the calling thread's kernel switches as parsed (czhip_tuning_describe)"""
        return tuning_in_force(self.lib)

    def precondition(self, r: np.ndarray) -> np.ndarray:
        """z = M^-1 r of the set-up pcg ... mg on this rank's brick (dense padded fields as field()); collective in a decomposed run"""
        r = np.ascontiguousarray(r, dtype=self.real)
        z = np.zeros_like(r)
        if self.lib.cz_precondition(self.h, r.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p)) != 1:
            raise RuntimeError("cz_precondition: no preconditioner set up")
        return z

    def timing(self, enable: bool):
        self.lib.czhip_timing(1 if enable else 0)

    def timing_read(self, label: str):
        tot = C.c_double(0.0)
        n = self.lib.czhip_timing_read(label.encode(), C.byref(tot))
        return n, tot.value

    def launches(self) -> dict:
        """launches recorded under every label since timing was enabled on the calling thread"""
        return {k: self.timing_read(k)[0] for k in LABELS + (JAC4_LABEL,)}

    def close(self):
        if self.h:
            self.lib.cz_destroy(self.h)
            self.h = None
