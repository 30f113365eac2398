"""Shared helpers of the GPU test files (test infrastructure: inputs come from the oracle's counter RNG, so CPU and GPU see identical data)."""
import ctypes as C
import functools

import numpy as np

import lightkrylov_amd as lk
from lightkrylov_amd import _capi
from oracle import oracle as ora

KINDS = [np.float64, np.complex128]


def seeded(n, dtype, seed):
    x = np.empty(n, dtype=dtype)
    ora.fill_counter(x, seed)
    return x


def basis(n, k, dtype, seed):
    X = np.empty((n, k), dtype=dtype, order="F")
    for j in range(k):
        ora.fill_counter(X[:, j], seed + j)
    return X


def orthonormal_basis(n, k, dtype, seed):
    Q, _ = np.linalg.qr(basis(n, k, dtype, seed))
    return np.asfortranarray(Q)


def skewed_basis(n, k, dtype, seed, delta=1e-3):
    """Q (I + delta S): Q from orthonormal_basis, S a k x k matrix from the counter generator (complex for the complex kind).  Off
    orthonormal by about delta * sqrt(k), cond about 1 + 2 delta ||S||: the second Gram-Schmidt pass has a correction of about delta |y|
    to make, and nothing amplifies rounding.  k > n: unit random columns (no orthonormal Q exists)."""
    if k > n:
        X = basis(n, k, dtype, seed)
        return np.asfortranarray(X / np.linalg.norm(X, axis=0))
    Q = orthonormal_basis(n, k, dtype, seed)
    S = basis(k, k, dtype, seed + 100_003)
    return np.asfortranarray(Q @ (np.eye(k, dtype=dtype) + delta * S))


def near_span(X, seed, eps=1e-6):
    """X c + eps r, c and r from the counter generator (`seed` and `seed + 1`: the caller picks them outside the seeds of X's columns):
    beta_{k+1} is about eps / |c|, and the second pass removes what the cancellation of the first left behind."""
    c = seeded(X.shape[1], X.dtype, seed)
    return X @ c + eps * seeded(X.shape[0], X.dtype, seed + 1)


@functools.lru_cache(maxsize=4)
def _second_pass_panel(n, k, dtype, skewed):
    X = (skewed_basis if skewed else orthonormal_basis)(n, k, dtype, 40 + k)
    X.setflags(write=False)                                        # (shared between the inputs of one shape)
    return X


def second_pass_input(n, k, dtype, which, p=1):
    """(X, Y) of the second-pass tests, Y of p columns: "skew_rand" = skewed X, random columns; "skew_span" = skewed X, columns near span(X);
    "orth_span" = orthonormal Q, columns near span(Q) (k > n: the unit random columns of skewed_basis in every case).  X has the column
    seeds 40 + k ..; column j of Y uses 5000 + k + 2 j (and + 1), which no column of X has.  X is read-only."""
    X = _second_pass_panel(n, k, dtype, which != "orth_span" or k > n)
    cols = [seeded(n, dtype, 5000 + k + 2 * j) if which == "skew_rand" else near_span(X, 5000 + k + 2 * j) for j in range(p)]
    return X, np.asfortranarray(np.stack(cols, axis=1))


def arnoldi_operator(n, dtype):
    """diagonal of the operator the continued factorisations run on: 1 + i / n, turned in the complex plane for the complex kind"""
    g = np.arange(n) / n
    return ((1.0 + g) * (np.exp(0.4j * g) if np.dtype(dtype).kind == "c" else 1.0)).astype(dtype)


def _long(a):
    a = np.asarray(a)
    return a.astype(np.clongdouble if a.dtype.kind == "c" else np.longdouble)


def dgs_longdouble(y, X):
    """two classical Gram-Schmidt passes in longdouble / clongdouble: h1 = X^H y, y' = y - X h1, h2 = X^H y', y'' = y' - X h2.  Returns
    h1, h2, y', y'' (beta of the step is h1 + h2).  The plain high-precision statement of gram_schmidt.fypp:12-57."""
    Xl, yl = _long(X), _long(y)
    Xh = Xl.conj().T
    h1 = Xh @ yl
    y1 = yl - Xl @ h1
    h2 = Xh @ y1
    y2 = y1 - Xl @ h2
    return h1, h2, y1, y2


def assert_second_pass_matters(h1, h2, y):
    """A condition on the INPUT of a test, not a measurement of the code under test: the reference's own second-pass coefficients reach
    1e-6 |y|, a million times the 1e-12 the results are compared at, so a wrong second pass cannot hide below the bound."""
    ynorm = float(np.linalg.norm(_long(y)))
    big = float(np.abs(h2).max()) if np.size(h2) else 0.0
    assert big >= 1e-6 * ynorm, f"second pass has nothing to do: max|h2| = {big:.2e} < 1e-6 |y| = {1e-6 * ynorm:.2e}"
    return big / ynorm


def _spd(n, seed, lead=(8.0, 6.0, 4.0)):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((n, n)) / np.sqrt(n)
    A = M.T @ M + np.eye(n)
    A[:len(lead), :len(lead)] += np.diag(lead)
    return np.asfortranarray(A)


def _lap5_csr(N):
    import scipy.sparse as sp
    T = sp.diags([-np.ones(N - 1), 4.0 * np.ones(N), -np.ones(N - 1)], [-1, 0, 1])
    S = sp.diags([-np.ones(N - 1), -np.ones(N - 1)], [-1, 1])
    return ((sp.kron(sp.identity(N), T) + sp.kron(S, sp.identity(N))) * float((N + 1) ** 2)).tocsr()


def _pool_fns(ctx):
    lib = _capi.load()

    def acquire(dtype, n, tag):
        slab, col = C.c_void_p(), C.c_int()
        _capi.check(lib.lk_pool_acquire(ctx._h, dtype, n, C.c_uint64(tag), C.byref(slab), C.byref(col)))
        return slab.value, col.value

    def info(slab, col):
        t, g = C.c_uint64(), C.c_uint64()
        _capi.check(lib.lk_pool_column_info(ctx._h, C.c_void_p(slab), col, C.byref(t), C.byref(g)))
        return t.value, g.value

    return lib, acquire, info


def _arnoldi_h(ctx, n=400_003, m=12):
    X = lk.krylov_basis_gpu(n, m + 1, np.float64, ctx)
    A = lk.diag_linop_gpu(n_local=n, row0=0, d0=1.0, dstep=1.0 / n, ctx=ctx)
    H = np.zeros((m + 1, m), order="F")
    X[0].rand(True, seed=7)
    assert lk.arnoldi(A, X, H) == 0
    return H, X.download()
