"""Mixed-precision iterative refinement: an FP64 answer for FP32 bytes.

The FP64 library holds the iterate, the right-hand side and the Dirichlet faces and is never asked to solve; every step it gives the true residual
r = b - A p (cz_get_residual) as a scaled float32 brick, the FP32 library solves the correction equation A e = r with `inner` (default
pcg 1000 1.2 mgrb), and the correction goes back into the FP64 iterate (cz_add_field).  The two libraries meet in one float32 device tensor;
torch is the plumbing, and their streams are ordered by the hand-over arguments of the field interface on a stream of this object's own.
"""
from __future__ import annotations

import math

from .driver import CZ

INNER_EPS = 1.0e-3  # 14 inner iterations in all to 1e-10 at 64^3, as 1e-2 (1e-4: 17), in 5 outer steps against 7 (tests/test_refine_oracle.py)


def scale_of(sumsq: float, npts: int) -> float:
    """2^-floor(log2 rms(r)), an exact power of two: the scaled residual has an rms in [1, 2), far from FP32's subnormals"""
    m, e = math.frexp(math.sqrt(sumsq / npts))  # rms = m 2^e, 0.5 <= m < 1
    return math.ldexp(1.0, min(max(1 - e, -100), 100))


class Refined:
    def __init__(self, gsz, inner=("pcg", 1000, 1.2, "mgrb"), division=None, device=-1, neumann=None, closed=False, periodic=None):
        """gsz: the global box; inner: the FP32 solver as on the command line (solver, ItrMax, coefficient[, preconditioner]); division: as on the
        command line (every rank of a decomposed run makes its own Refined after joining both libraries' communicators); neumann: the six
        flags of CZ.set_neumann, set on both libraries (the inner solver must then be pcg); closed: CZ.set_closed_box on both (all six faces
        zero-flux, right-hand sides projected, answers of zero mean; not together with neumann); periodic: the three flags of CZ.set_periodic (X, Y, Z), set on both after neumann= or
        closed=, with either of which it combines (closed=True with (1, 0, 1) is the channel, with (1, 1, 1) the triply periodic box)"""
        if closed and neumann is not None:
            raise ValueError("Refined: closed=True and neumann= exclude each other (the closed box is all six faces)")
        import torch  # (only here: the package imports without it)
        self.torch = torch
        div = list(division) if division else []
        self.hi = CZ("f64", quiet=True, device=device)
        self.lo = CZ("f32", quiet=True, device=device)
        if self.hi.setup(list(gsz) + ["jacobi", 1, 0.8] + div) != 1:
            raise RuntimeError("Refined: the FP64 set-up failed")
        if self.lo.setup(list(gsz) + list(inner) + div) != 1:
            raise RuntimeError(f"Refined: the FP32 set-up of {inner} failed")
        if neumann is not None:
            self.hi.set_neumann(neumann)
            self.lo.set_neumann(neumann)
        if closed:
            self.hi.set_closed_box(True)
            self.lo.set_closed_box(True)
        if periodic is not None:
            self.hi.set_periodic(periodic)
            self.lo.set_periodic(periodic)
        self.shape = tuple(self.hi.local()["size"])
        if tuple(self.lo.local()["size"]) != self.shape:
            raise RuntimeError("Refined: the two libraries cut the domain differently")
        self.npts = int((gsz[0] - 2) * (gsz[1] - 2) * (gsz[2] - 2))  # the cells every sweep updates, whole domain
        dev = torch.device("cuda", device if device >= 0 else torch.cuda.current_device())
        self.r32 = torch.zeros(self.shape, dtype=torch.float32, device=dev)  # the interchange: residual out, correction back
        self.stream = torch.cuda.Stream(dev)
        self.history = []

    def set_rhs(self, b64):
        self.hi.set_rhs(b64)

    def set_field(self, p64):
        self.hi.set_field(p64)

    def get_field(self, out=None):
        return self.hi.get_field(out)

    def set_face_coef(self, bx, by=None, bz=None):
        """CZ.set_face_coef on both libraries: the FP64 values as given, their FP32 roundings (made by torch) for the inner solver, which then
        corrects with the operator of the rounded coefficients -- a perturbation of relative size 6e-8 that the outer steps absorb.
        set_face_coef(None) clears both.  Raises where either library refuses (a refusal of a bad value leaves that library without
        coefficients: the other one is then cleared too)"""
        if bx is None and by is None and bz is None:
            self.hi.set_face_coef(None)
            self.lo.set_face_coef(None)
            return
        torch = self.torch
        self.hi.set_face_coef(bx, by, bz)
        try:
            lo3 = [torch.as_tensor(a).to(device=self.r32.device, dtype=torch.float32).contiguous() for a in (bx, by, bz)]
            self.lo.set_face_coef(*lo3)
        except Exception:
            self.hi.set_face_coef(None)
            self.lo.set_face_coef(None)
            raise

    def set_coef_mg(self, on=True):
        """CZ.set_coef_mg on both libraries.  The FP32 inner solver is the one that preconditions: with pcg mg | mgrb the flag is in force
        there (lo.info()["coef_mg"]); the FP64 handle only forms residuals, so the flag is accepted and idle on it.  Raises where either
        library refuses: both flags are then off"""
        try:
            self.hi.set_coef_mg(on)
            self.lo.set_coef_mg(on)
        except Exception:
            for cz in (self.hi, self.lo):
                cz.lib.cz_set_coef_mg(cz.h, 0)
            raise

    def set_mg_lines(self, on=True):
        """CZ.set_mg_lines on both libraries: in force on the FP32 inner solver with pcg mgrb under set_coef_mg (lo.info()["mg_lines"]),
        accepted and idle on the FP64 handle.  Raises where either library refuses: both flags are then off"""
        try:
            self.hi.set_mg_lines(on)
            self.lo.set_mg_lines(on)
        except Exception:
            for cz in (self.hi, self.lo):
                cz.lib.cz_set_mg_lines(cz.h, 0)
            raise

    def solve(self, tol=1e-10, max_outer=20, inner_eps=INNER_EPS) -> int:
        """refine until |b - A p| <= tol |b - A p0|; returns the outer steps taken, 0 where max_outer steps did not reach it.
        history: [(outer step, |r| / |r0| after it, inner iterations of it)].  Collective in a decomposed run.
        A start whose residual is exactly zero returns 0 too, with an empty history and the field untouched: there was nothing to refine."""
        torch, hi, lo, r32 = self.torch, self.hi, self.lo, self.r32
        self.history = []
        _, ss0 = hi.get_residual()
        ss, inner, k = ss0, 0, 0
        self.stream.wait_stream(torch.cuda.current_stream(r32.device))
        with torch.cuda.stream(self.stream):
            while True:
                scale = scale_of(ss, self.npts)
                _, ss = hi.get_residual(out=r32, scale=scale)  # (the one wait of the step: the sum comes to the host)
                if k > 0:
                    self.history.append((k, math.sqrt(ss) / math.sqrt(ss0), inner))
                if math.sqrt(ss) <= tol * math.sqrt(ss0):
                    break
                if k == max_outer:
                    k = 0
                    break
                lo.set_rhs(r32)
                r32.zero_()
                lo.set_field(r32)
                lo.set_eps(inner_eps)
                inner = lo.solve()
                if inner == 0:
                    raise RuntimeError(f"Refined: the inner solve failed at outer step {k + 1}")
                lo.get_field(r32)
                hi.add_field(r32, 1.0 / scale)
                k += 1
        torch.cuda.current_stream(r32.device).wait_stream(self.stream)
        return k

    def close(self):
        for h in (self.hi, self.lo):
            if h is not None:
                h.close()
        self.hi = self.lo = None
