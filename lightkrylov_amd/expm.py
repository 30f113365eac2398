"""Matrix exponential -- host-side mirror of src/Expm/ExpmLib.fypp (LightKrylov_ExpmLib).

`kexpm(c, A, b, tau, tol)` approximates c = exp(tau A) b in the Krylov subspace of (A, b) (ExpmLib.fypp:128-232) and returns the
reference's `info`: kp > 0 = converged with kp Krylov vectors (an Arnoldi breakdown included), -1 = `kdim` steps did not reach
`tol` (c is then the kdim-step approximation).  `krylov_exptA` is the same with the reference's fixed settings (:365-392), the
procedure behind the `abstract_exptA` interface; `linops.exptA_linop` wraps it as an operator.

For an engine operator on `dense_vector_gpu` vectors the whole evaluation is ONE engine call (lk_kexpm: the Arnoldi steps are
enqueued back to back, the small exponential and the error estimate are evaluated on the host while the device runs ahead, the
projection runs once).  For any other operator or vector type the reference's loop runs on the package's primitives -- `arnoldi`
one step at a time, `expm`, `linear_combination` -- which is the extension API for user-defined operators, not a fallback.

`kexpm` is generic over the block form too, as in the reference: with bases (or sequences of p vectors) for `c` and `b` it is
kexpm_mat (:234-363) -- the column-pivoting qr of B, block Arnoldi steps, `expm` of the block Hessenberg matrix and the error
estimate `norm2(E(kp+1:kpp, :p) R)`.  One engine call (lk_kexpm_block) for an engine operator on device panels, the same loop on
the primitives otherwise.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from .constants import atol_dp
from .krylov import arnoldi, invperm, permcols, qr
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


def norm2(A: np.ndarray) -> float:
    """||A||_2, the largest singular value of a small dense matrix, on the host (`norm(., 2)` of ExpmLib.fypp:346): one-sided Jacobi
    rotations (lk_norm2_dense).  Needs no GPU."""
    A = np.asarray(A)
    if A.ndim != 2:
        raise ValueError(f"norm2 needs a matrix, got shape {A.shape}")
    dt = np.dtype(np.complex128 if A.dtype.kind == "c" else np.float64)
    A = np.asfortranarray(A, dtype=dt)
    m, n = A.shape
    out = C.c_double()
    _capi.check(_capi.load().lk_norm2_dense(_DT[dt], m, n, A.ctypes.data_as(_DP), max(m, 1), C.byref(out)))
    return out.value


MAX_BLOCK_COLUMNS = 512      # columns of workspace one block evaluation may use (lk_kexpm_block)


def _kexpm_mat_host(Cb, A, B, tau, tol, trans, nk, X) -> int:
    """ExpmLib.fypp:293-362 on the package's primitives.  The projection (:327-339) runs once, behind the loop: the reference forms
    it after every step and keeps the last."""
    p = len(B)
    X = X[:p * (nk + 1)]
    dtype = np.dtype(getattr(B[0], "dtype", np.float64))
    R = np.zeros((p, p), dtype=dtype, order="F")
    perm = np.zeros(p, dtype=np.intc)
    for i in range(p):                                                              # :293
        copy(X[i], B[i])
    qr(X[:p], R, perm=perm)                                                         # :297 (info discarded there as well)
    permcols(R, invperm(perm))
    if np.linalg.norm(R, "fro") == 0.0:                                             # :299-302
        for ci in Cb:
            ci.zero()
        return p if 0.0 <= tol else -1
    for x in X[p:]:                                                                 # initialize_krylov_subspace   :304
        x.zero()
    R0 = np.zeros((p, p), dtype=dtype, order="F")
    qr(X[:p], R0)
    H = np.zeros((p * (nk + 1), p * (nk + 1)), dtype=dtype, order="F")
    kpp, err_est, E = p, np.inf, None
    for k in range(1, nk + 1):                                                      # :306
        kp = k * p
        info = arnoldi(A, X, H, kstart=k, kend=k, transpose=trans, blksize=p)       # :314
        breakdown = info == kp                                                      # :317-321
        kpp = kp if breakdown else kp + p
        E = expm(tau * H[:kpp, :kpp])                                               # :324
        err_est = 0.0 if breakdown else norm2(E[kp:kpp, :p] @ R)                    # :342-347
        if err_est <= tol:                                                          # :349
            break
    Y = linear_combination(X[:kpp], np.asfortranarray(E[:kpp, :p] @ R))             # :327-339
    for i in range(p):
        copy(Cb[i], Y[i])
    return kpp if err_est <= tol else -1                                            # :354-362


def _kexpm_mat(Cb, A, B, tau, tol, trans, kdim, X) -> int:
    p = len(B)
    if p < 1 or len(Cb) != p:
        raise ValueError(f"kexpm: C has {len(Cb)} vectors, B has {p}")
    nk = kdim * p                                                                   # :276
    if X is None:
        # the reference allocates p (nk + 1) vectors (:289), thousands with its default kdim = 100: a workspace made here stops at
        # MAX_BLOCK_COLUMNS columns, i.e. at 512 // p - 1 block steps
        nk = max(min(nk, MAX_BLOCK_COLUMNS // p - 1), 1)
        X = _workspace(B[0], p * (nk + 1))
    if len(X) < p * (nk + 1):
        raise ValueError(f"kexpm: the workspace has {len(X)} vectors, kdim = {kdim} with {p} columns needs {p * (nk + 1)}")
    if (isinstance(A, _engine_linop) and isinstance(B, krylov_basis_gpu) and isinstance(Cb, krylov_basis_gpu)
            and isinstance(X, krylov_basis_gpu)):
        info, err = C.c_int(), C.c_double()
        _capi.check(X._lib.lk_kexpm_block(A._h, 1 if trans else 0, B._h, 0, Cb._h, 0, p, X._h, float(tau), float(tol), nk,
                                          C.byref(info), C.byref(err)))
        if info.value == p and err.value == 0.0 and all(B[i].norm() == 0.0 for i in range(p)):
            return info.value                                                      # B = 0: no operator application (:299-302)
        # block steps taken: kpp / p - 1, kpp / p after a breakdown (whose estimate is exactly zero)
        steps = nk if info.value < 0 else (info.value // p if err.value == 0.0 else info.value // p - 1)
        if trans:
            A.rmatvec_counter += steps * p
        else:
            A.matvec_counter += steps * p
        return info.value
    return _kexpm_mat_host(Cb, A, B, tau, tol, trans, nk, X)


def kexpm(c, A: abstract_linop, b, tau: float, tol: float, trans: bool = False, kdim: int = 100,
          _basis=None) -> int:
    """kexpm(c, A, b, tau, tol, info, trans, kdim): c = exp(tau A) b (A^H with `trans`).  Returns info.
    Vector form (c, b vectors; ExpmLib.fypp:128-232).  `_basis`: workspace of at least kdim + 1 vectors to use instead of allocating
    one (a time stepper passes the same one to every call); on return it holds the Krylov basis.
    Block form (c, b bases or sequences of p vectors; kexpm_mat, :234-363): at most nk = kdim * p block Arnoldi steps (:276), on a
    workspace of p (nk + 1) vectors.  Departure from the reference: a workspace allocated HERE holds at most 512 columns, so nk is
    capped at 512 // p - 1 (the reference's default kdim = 100 would allocate p (100 p + 1) vectors); a `_basis` passed in must hold
    p (nk + 1) vectors or the call raises."""
    kdim = int(kdim)
    if kdim < 1:
        raise ValueError("kexpm: kdim must be at least 1")
    if not isinstance(b, abstract_vector):
        return _kexpm_mat(c, A, b, tau, tol, trans, kdim, _basis)
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
