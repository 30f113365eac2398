"""Matrix exponential -- host-side mirror of src/Expm/ExpmLib.fypp (LightKrylov_ExpmLib).

`kexpm(c, A, b, tau, tol)` approximates c = exp(tau A) b in the Krylov subspace of (A, b) (ExpmLib.fypp:128-232) and returns the
reference's `info`: kp > 0 = converged with kp Krylov vectors (an Arnoldi breakdown included), -1 = `kdim` steps did not reach
`tol` (c is then the kdim-step approximation).  `krylov_exptA` is the same with the reference's fixed settings (:365-392), the
procedure behind the `abstract_exptA` interface; `linops.exptA_linop` wraps it as an operator.

For an engine operator on `dense_vector_gpu` vectors the whole evaluation is ONE engine call (lk_kexpm: the Arnoldi steps are
enqueued back to back, the small exponential and the error estimate are evaluated on the host while the device runs ahead, the
projection runs once).  For any other operator or vector type the reference's loop runs on the package's primitives -- `arnoldi`
one step at a time, `expm`, `linear_combination` -- which is the extension API for user-defined operators, not a fallback.
The block variant kexpm_mat (:234-363) is not provided.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from .constants import atol_dp
from .krylov import arnoldi
from .linops import _engine_linop, abstract_linop
from .vectors import _DT, abstract_vector, copy, dense_vector_gpu, krylov_basis_gpu, linear_combination

_DP = C.POINTER(C.c_double)


def expm(A: np.ndarray) -> np.ndarray:
    """exp(A) of a small dense matrix on the host (stdlib_linalg's `expm`, ExpmLib.fypp:12, 207): scaling and squaring with the
    [13/13] Pade approximant (lk_expm_dense).  Needs no GPU."""
    A = np.asarray(A)
    if A.ndim != 2 or A.shape[0] != A.shape[1]:
        raise ValueError(f"expm needs a square matrix, got shape {A.shape}")
    dt = np.dtype(np.complex128 if A.dtype.kind == "c" else np.float64)
    A = np.asfortranarray(A, dtype=dt)
    n = A.shape[0]
    E = np.zeros((n, n), dtype=dt, order="F")
    _capi.check(_capi.load().lk_expm_dense(_DT[dt], n, A.ctypes.data_as(_DP), max(n, 1), E.ctypes.data_as(_DP), max(n, 1)))
    return E


def _workspace(b: abstract_vector, ncols: int):
    """`allocate(X(nk+1), source=b)` (ExpmLib.fypp:171): one device panel for GPU vectors, else vectors of b's type"""
    if isinstance(b, dense_vector_gpu):
        return krylov_basis_gpu(b.basis.n_local, ncols, b.dtype, b.basis.ctx)
    return [b.zeros_like() for _ in range(ncols)]


def _kexpm_host(c, A, b, tau, tol, trans, kdim, X) -> int:
    """ExpmLib.fypp:178-231 on the package's primitives.  The projection (:210-211) runs once, behind the loop: the reference forms it
    after every step and keeps the last."""
    X = X[:kdim + 1]
    dtype = np.dtype(getattr(b, "dtype", np.float64))
    H = np.zeros((kdim + 1, kdim + 1), dtype=dtype, order="F")
    beta = b.norm()                                                                 # :179
    if beta == 0.0:                                                                 # :180-184
        c.zero()
        return 1 if 0.0 <= tol else -1
    copy(X[0], b)                                                                   # :186-187
    X[0].scal(1.0 / beta)
    kp, err_est, E = 1, np.inf, None
    for k in range(1, kdim + 1):                                                    # :189
        info = arnoldi(A, X, H, kstart=k, kend=k, transpose=trans)                  # :196
        breakdown = info == k                                                       # :200-204
        kp = k if breakdown else k + 1
        E = expm(tau * H[:kp, :kp])                                                 # :207
        err_est = 0.0 if breakdown else abs(E[kp - 1, 0] * beta)                    # :215
        if err_est <= tol:                                                          # :218
            break
    y = linear_combination(X[:kp], beta * E[:kp, 0])                                # :210-211
    copy(c, y)
    return kp if err_est <= tol else -1                                             # :223-231


def kexpm(c: abstract_vector, A: abstract_linop, b: abstract_vector, tau: float, tol: float, trans: bool = False, kdim: int = 100,
          _basis=None) -> int:
    """kexpm(c, A, b, tau, tol, info, trans, kdim), vector form: c = exp(tau A) b (A^H with `trans`).  ExpmLib.fypp:128-232.
    Returns info.  `_basis`: workspace of at least kdim + 1 vectors to use instead of allocating one (a time stepper passes the
    same one to every call); on return it holds the Krylov basis."""
    kdim = int(kdim)
    if kdim < 1:
        raise ValueError("kexpm: kdim must be at least 1")
    X = _basis if _basis is not None else _workspace(b, kdim + 1)
    if len(X) < kdim + 1:
        raise ValueError(f"kexpm: the workspace has {len(X)} vectors, kdim = {kdim} needs {kdim + 1}")
    if (isinstance(A, _engine_linop) and isinstance(b, dense_vector_gpu) and isinstance(c, dense_vector_gpu)
            and isinstance(X, krylov_basis_gpu)):
        info, err = C.c_int(), C.c_double()
        _capi.check(X._lib.lk_kexpm(A._h, 1 if trans else 0, b.basis._h, b.col, c.basis._h, c.col, X._h, float(tau), float(tol), kdim,
                                    C.byref(info), C.byref(err)))
        # operator applications the result used: kp - 1 steps, kp after a breakdown (whose estimate is exactly zero)
        steps = kdim if info.value < 0 else (info.value if err.value == 0.0 else info.value - 1)
        if trans:
            A.rmatvec_counter += steps
        else:
            A.matvec_counter += steps
        return info.value
    return _kexpm_host(c, A, b, tau, tol, trans, kdim, X)


def krylov_exptA(vec_out: abstract_vector, A: abstract_linop, vec_in: abstract_vector, tau: float, trans: bool = False,
                 _basis=None) -> int:
    """The `abstract_exptA` procedure of the reference: kexpm with tol = atol_dp and kdim = 30.  ExpmLib.fypp:365-392.
    Returns kexpm's info (-1: thirty Krylov vectors did not reach atol_dp; the reference logs that as an error)."""
    return kexpm(vec_out, A, vec_in, tau, atol_dp, trans=trans, kdim=30, _basis=_basis)
