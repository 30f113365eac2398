"""Inputs of the lk_gmres tests, stated once: tests/test_gmres_host_logic.py pins them against the oracle without a GPU,
tests/test_gpu_gmres_engine.py runs them on the device."""
import numpy as np

from tests._gpu_helpers import seeded


def is_cplx(dtype):
    return np.dtype(dtype).kind == "c"


def pipelines_diag(dtype, n=30_011):
    """the diagonal operator and right-hand side of tests/test_gpu_pipelines.py::test_gmres_inner_cycle_..., restated"""
    rng = np.random.default_rng(4)
    d = (2.0 + np.arange(n) % 23 + rng.random(n)).astype(dtype)
    if is_cplx(dtype):
        d = d * np.exp(0.3j * rng.random(n))
    return d, seeded(n, dtype, 17)


def dense_nonsymmetric(dtype, n=300):
    """I * 4 + a full non-symmetric perturbation of norm about 1: GMRES(40) converges in one cycle, GMRES(5) needs restarts"""
    A = np.empty((n, n), dtype=dtype, order="F")
    for j in range(n):
        A[:, j] = seeded(n, dtype, 700 + j)
    A *= 1.0 / np.sqrt(n)
    A[np.diag_indices(n)] += 4.0
    return A, seeded(n, dtype, 18)


# (kdim, maxiter, rtol, what it covers)
UNPRECONDITIONED = ((40, 5, 1e-10, "converges inside the first cycle"), (5, 30, 1e-10, "converges after restarts"),
                    (5, 2, 1e-14, "does not converge"))


def tiny_diag(dtype, n=64):
    """gmres.fypp:171-172: A = 1e-12 * diag, ||b|| = 1, rtol = 1e-8, kdim = 3, maxiter = 1 -- every H(k+1, k) is about 1e-12 <= tol = 1e-8
    while the residual stays near 0.3: no Krylov vector behind the first is scaled"""
    d = (1e-12 * (1.0 + np.arange(n) % 7 + 0.25 * seeded(n, np.float64, 5))).astype(dtype)
    if is_cplx(dtype):
        d = d * np.exp(0.3j * seeded(n, np.float64, 6))
    b = seeded(n, dtype, 17)
    return d, b / np.linalg.norm(b)


TINY = dict(rtol=1e-8, atol=0.0, kdim=3, maxiter=1)


def variable_coefficient(dtype, n=400):
    """A sparse non-symmetric matrix whose diagonal runs from 1 to 1e4 (condition number 2.4e4; 3.2 after Jacobi scaling of the columns):
    sub- and super-diagonal of relative size 0.3 and 0.2 with 20 % of jitter and a seventh diagonal of 0.05.  Returns (csr, dense, 1 / diag, b)."""
    import scipy.sparse as sp
    dg = 10.0 ** (4.0 * np.arange(n) / (n - 1))
    lo = -0.30 * np.sqrt(dg[1:] * dg[:-1]) * (1.0 + 0.2 * seeded(n - 1, np.float64, 41))
    up = -0.20 * np.sqrt(dg[1:] * dg[:-1]) * (1.0 + 0.2 * seeded(n - 1, np.float64, 42))
    far = 0.05 * np.sqrt(dg[7:] * dg[:-7])
    A = sp.diags([lo, dg, up, far], (-1, 0, 1, 7), format="csr").astype(dtype)
    if is_cplx(dtype):
        A.data = A.data * np.exp(0.2j * seeded(A.data.size, np.float64, 43) * (A.data.real < 0))
    A.sort_indices()
    Ad = np.asfortranarray(A.toarray())
    return A, Ad, (1.0 / Ad.diagonal()).astype(dtype), seeded(n, dtype, 17)


PRECONDITIONED = dict(rtol=1e-10, atol=0.0, kdim=20, maxiter=10)
PRECONDITIONED_ITERATIONS = (24, -231)      # ora.gmres with and without the Jacobi preconditioner, both kinds (pinned on the CPU)
