"""Nothing of an asynchronous batch outlives the call that ran it.

lk_arnoldi, lk_lanczos, lk_bidiag and lk_arnoldi_block enqueue their steps back to back.  While they do, every launch on the context
carries the guard (the device stop flag and a step number: once the flag is raised, the kernels of every later step do nothing) and, in
three of the four, only the sweeps carry profiling events.  Both are switches on the CONTEXT.  Left on after the call they are silent:
a later plain kernel would carry a stop flag that may still be raised and do nothing, and a later profiled kernel would not be counted.

Each case leaves one batch behind on a context -- (a) one that ran to the end, (b) one that the device stopped at its first or second
step (the start vectors are eigenvectors of the diagonal operator, so the first new direction is exactly zero), (c) one whose first
operator application failed inside the enqueue loop (an operator of n + 2 rows; no entry looks at the operator's size before its
batch starts, so all four reach the loop, and each must hand back the code lk_linop_apply returns for that pair on its own) -- and then,
on the same context:
  1. a profiled lk_vec_scal is counted under its tag "blas1";
  2. lk_vec_axpby and lk_dgs on fresh columns give what numpy gives: axpby per component within gamma(2) (real) / gamma(3) (complex) of
     its own products (tests/_blas1_cases.py), the Gram-Schmidt step against two passes in longdouble (tests/_gpu_helpers.py) at 1e-12 |y|;
  3. the factorisation run again equals, byte for byte, one run on a context created for it.  (After (c): the factorisation of (a).)
     Once with the single-launch step and once on the three sweeps.  Neither context may count a single launch that gave up meanwhile:
     something left on the used context that makes the next launch give up (a raised abort word) fails with a message of its own.

n = 4096, at most 12 steps (block: 4 steps of 2 columns)."""
import ctypes as C
import functools

import numpy as np
import pytest

import lightkrylov_amd as lk
from lightkrylov_amd import _capi
from tests._blas1_cases import check_axpby
from tests._gpu_helpers import KINDS, dgs_longdouble, is_cplx, orthonormal_basis, seeded
from tests._tol import assert_close

pytestmark = pytest.mark.gpu

_DP = C.POINTER(C.c_double)
N = 4096
ENTRIES = ("arnoldi", "lanczos", "bidiag", "arnoldi_block")
KDIM = {"arnoldi": 12, "lanczos": 12, "bidiag": 8, "arnoldi_block": 4}
P = 2                                                               # block size of arnoldi_block


def _diag(entry, dtype, n=N):
    g = np.arange(n) / n
    turn = np.exp(0.4j * g) if is_cplx(dtype) and entry != "lanczos" else 1.0          # (lanczos: Hermitian)
    return ((1.0 + g) * turn).astype(dtype)


@functools.lru_cache(maxsize=None)
def _start(entry, dtype, breakdown):
    """the start columns (n x 1, n x P for the block entry): unit random columns, or unit vectors e_1 (, e_2): eigenvectors of a diagonal"""
    p = P if entry == "arnoldi_block" else 1
    X0 = np.zeros((N, p), dtype=dtype, order="F")
    for j in range(p):
        if breakdown:
            X0[j, j] = 1.0
        else:
            X0[:, j] = seeded(N, dtype, 7 + j)
    if not breakdown:
        X0, _ = np.linalg.qr(X0)
    X0 = np.asfortranarray(X0)
    X0.setflags(write=False)
    return X0


def _bases(entry, dtype, c, X0):
    kdim = KDIM[entry]
    p = X0.shape[1]
    X = lk.krylov_basis_gpu(N, (kdim + 1) * p, dtype, c)
    X.upload(X0, 0)
    V = lk.krylov_basis_gpu(N, kdim, dtype, c) if entry == "bidiag" else None
    return X, V, np.zeros(((kdim + 1) * p, kdim * p), dtype=dtype, order="F")


def factorise(entry, dtype, c, breakdown=False):
    """(projected matrix, info, every basis column) of the entry on context c"""
    A = lk.diag_linop_gpu(_diag(entry, dtype), c)
    X, V, M = _bases(entry, dtype, c, _start(entry, np.dtype(dtype), breakdown))
    if entry == "arnoldi":
        info = lk.arnoldi(A, X, M)
    elif entry == "arnoldi_block":
        info = lk.arnoldi(A, X, M, blksize=P)
    elif entry == "lanczos":
        info = lk.lanczos(A, X, M)
    else:
        info = lk.bidiagonalization(A, X, V, M)
    out = (M, info, X.download()) + ((V.download(),) if V is not None else ())
    for o in (X, V, A):
        if o is not None:
            o.close()
    return out


def fail_in_the_loop(entry, dtype, c):
    """the entry with an operator of n + 2 rows: its first lk_linop_apply fails inside the enqueue loop"""
    lib = _capi.load()
    A = lk.diag_linop_gpu(_diag(entry, dtype, N + 2), c)
    X, V, M = _bases(entry, dtype, c, _start(entry, np.dtype(dtype), False))
    kdim, info, tol = KDIM[entry], C.c_int(), 1e-15
    if entry == "bidiag":
        alone = lib.lk_linop_apply(A._h, _capi.LK_OP_H, X._h, 0, V._h, 0)
        rc = lib.lk_bidiag(A._h, X._h, V._h, M.ctypes.data_as(_DP), M.shape[0], 1, kdim, tol, C.byref(info))
    else:
        alone = lib.lk_linop_apply(A._h, _capi.LK_OP_N, X._h, 0, X._h, X0_cols(entry))
        if entry == "arnoldi":
            rc = lib.lk_arnoldi(A._h, X._h, M.ctypes.data_as(_DP), M.shape[0], 1, kdim, tol, 0, C.byref(info))
        elif entry == "arnoldi_block":
            rc = lib.lk_arnoldi_block(A._h, X._h, M.ctypes.data_as(_DP), M.shape[0], P, 1, kdim, tol, 0, C.byref(info))
        else:
            rc = lib.lk_lanczos(A._h, X._h, M.ctypes.data_as(_DP), M.shape[0], 1, kdim, tol, C.byref(info))
    for o in (X, V, A):
        if o is not None:
            o.close()
    assert alone != 0, "lk_linop_apply accepted an operator of another size"
    assert rc == alone, f"lk_{entry} returned {rc}, lk_linop_apply alone returns {alone}"


def X0_cols(entry):
    return P if entry == "arnoldi_block" else 1


@functools.lru_cache(maxsize=None)
def _plain_inputs(dtype):
    """Q (n x 8, orthonormal), y, x and the longdouble Gram-Schmidt step of y against Q: computed once, never written"""
    Q = orthonormal_basis(N, 8, dtype, 300)
    y, x = seeded(N, dtype, 400), seeded(N, dtype, 401)
    h1, h2, _y1, y2 = dgs_longdouble(y, Q)
    for a in (Q, y, x):
        a.setflags(write=False)
    return Q, y, x, h1 + h2, y2


def plain_kernels_run(c, dtype, what):
    Q, y, x, beta, y2 = _plain_inputs(np.dtype(dtype))
    k = Q.shape[1]
    B = lk.krylov_basis_gpu(N, k + 3, dtype, c)
    B.upload(Q, 0)
    B.upload(np.stack([y, x, x], axis=1), k)
    # 1. the profiling switch
    c.profile_reset()
    B[k + 2].scal(2.0)
    count = c.profile_get("blas1")[0]
    assert count == 1, f"{what}: a profiled lk_vec_scal was counted {count} times under 'blas1'"
    # 2. the guard: a kernel that carried a raised stop flag would leave its output as it was
    a, b = (dtype(0.75 - 0.5j), dtype(-1.25 + 0.25j)) if is_cplx(dtype) else (dtype(0.75), dtype(-1.25))
    B[k + 1].axpby(a, B[k], b)
    check_axpby(B.download(k + 1, 1)[:, 0], a, y, b, x, f"{what}: lk_vec_axpby")
    h = np.zeros(k, dtype=dtype)
    assert lk.double_gram_schmidt_step(B[k], B[:k], False, beta=h) == 0
    scale = float(np.linalg.norm(y))
    assert_close(h, beta, f"{what}: lk_dgs beta", scale=scale)
    assert_close(B.download(k, 1)[:, 0], y2, f"{what}: lk_dgs y''", scale=scale)
    B.close()


def same_as_fresh(c, entry, dtype, breakdown, what):
    for resident in (1, 0):
        c.set_tuning("resident", resident)
        before = c.resident_stats()[1]
        got = factorise(entry, dtype, c, breakdown)
        gave_up = c.resident_stats()[1] - before
        fresh = lk.Context(device=0)
        try:
            fresh.set_tuning("resident", resident)
            ref = factorise(entry, dtype, fresh, breakdown)
            gave_up_fresh = fresh.resident_stats()[1]
        finally:
            fresh.close()
        assert gave_up == 0, f"{what} resident={resident}: {gave_up} single launches gave up on the used context"
        assert gave_up_fresh == 0, f"{what} resident={resident}: {gave_up_fresh} single launches gave up on the fresh context"
        assert len(got) == len(ref) and got[1] == ref[1], f"{what}: info {got[1]} against {ref[1]} on a fresh context"
        for i, (g, r) in enumerate(zip(got, ref)):
            g, r = np.asarray(g), np.asarray(r)
            assert g.shape == r.shape and g.tobytes() == r.tobytes(), f"{what} resident={resident}: result {i} differs from a fresh context's"
    c.set_tuning("resident", 1)
    return got


@pytest.mark.parametrize("left_behind", ["complete", "breakdown", "error"])
@pytest.mark.parametrize("dtype", KINDS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_nothing_of_a_batch_outlives_the_call(entry, dtype, left_behind):
    what = f"after a {left_behind} lk_{entry} batch, {np.dtype(dtype).name}"
    c = lk.Context(device=0)
    try:
        c.profile_enable(True)
        if left_behind == "error":
            fail_in_the_loop(entry, dtype, c)
        else:
            M, info, *_ = factorise(entry, dtype, c, left_behind == "breakdown")
            if left_behind == "breakdown":
                assert info in (1, 2, P), f"{what}: info = {info}, the start vectors should have broken the factorisation down at once"
            else:
                assert info == 0 and np.isfinite(M).all()
        plain_kernels_run(c, dtype, what)
        c.profile_enable(False)
        M, info, *_ = same_as_fresh(c, entry, dtype, left_behind == "breakdown", what)
        assert np.isfinite(M).all() and (info == 0) == (left_behind != "breakdown")
    finally:
        c.close()
