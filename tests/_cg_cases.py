"""Inputs, the longdouble restatement and the sizes of the lk_cg tests: tests/test_cg_host_logic.py pins them without a GPU,
tests/test_gpu_cg_engine.py runs them on the device.

The restatement is CG.fypp:105-170 line by line in longdouble / clongdouble, with and without a preconditioner, for both kinds.  The new
passes (cg_update, cg_scalars, cg_direction, run inside k_axpby's symbol) are launched through the BLAS-1 grid rule, so the edge sizes are those of
tests/_blas1_cases.py (edge_sizes, POLICY_N)."""
import functools

import numpy as np

from tests._blas1_cases import DEFAULT_MULT, POLICY_N, edge_sizes, stride
from tests._gpu_helpers import _spd, ext, is_cplx, seeded

LOOKAHEAD = 24                                     # SEG_LOOKAHEAD of csrc/lk_engine.hip: iterations enqueued ahead of the host
DELIVERY_MAXITER = (1, 23, 24, 25, 49)             # one short of, at and beyond the look-ahead; two look-aheads and one


def cg_long(A, b, x0, rtol, atol, maxiter, M=None):
    """CG.fypp:105-170 in extended precision.  A, M: functions v -> A v, v -> M v on extended vectors.  Returns (info, res, x, r, p) as
    the reference holds them when it leaves the loop; dot(x, y) = conj(x) . y."""
    b, x = ext(b), ext(x0).copy()
    dot = lambda u, v: (u.conj() * v).sum()
    tol = atol + rtol * np.sqrt(dot(b, b).real)                                    # :87
    r = A(x) if np.sqrt(dot(x, x).real) > 0 else np.zeros_like(b)                  # :108
    r = -(r - b)                                                                   # :109
    if M is not None:
        z = M(r); p = z.copy(); rho = dot(r, z)                                    # :113-114
    else:
        z = r; p = r.copy(); rho = dot(r, r)                                       # :116
    res = [np.sqrt(np.abs(rho))]                                                   # :119
    n_iter, converged = 0, False
    for _ in range(maxiter):                                                       # :123
        Ap = A(p)                                                                  # :125
        alpha = rho / dot(p, Ap)                                                   # :127
        x = x + alpha * p                                                          # :129
        r = r - alpha * Ap                                                         # :131
        z = M(r) if M is not None else r                                           # :134
        rho_new = dot(r, z)                                                        # :134-137
        residual = np.sqrt(np.abs(rho_new))                                        # :141-145 (|.| of a real rho > 0 changes nothing)
        n_iter += 1
        res.append(residual)                                                       # :148-149
        if residual < tol:                                                         # :151-154
            converged = True
            break
        beta = rho_new / rho                                                       # :157
        p = z + beta * p                                                           # :160-164
        rho = rho_new                                                              # :167
    return (n_iter if converged else -n_iter), np.array(res, dtype=np.longdouble), x, r, p


def matop(A):
    Al = ext(A)
    return lambda v: Al @ v


def diagop(d):
    dl = ext(d)
    return lambda v: dl * v


# ---- parity cases at solver level -----------------------------------------------------------------------------------------------------------
N_PARITY = 600
MAXITER = 200
ATOL = 1e-14


@functools.lru_cache(maxsize=None)
def dense_spd():
    """I + G^T G with G = (counter stream) / sqrt(n): SPD, condition number about 2.3, so the residual falls by a factor of about 5 per
    iteration and a tolerance fits between two history entries with a factor 2 to spare on either side"""
    n = N_PARITY
    G = seeded(n * n, np.float64, 621).reshape(n, n) / np.sqrt(n)
    A = np.eye(n) + G.T @ G
    A = np.asfortranarray((A + A.T) / 2)
    b = seeded(n, np.float64, 3)
    A.setflags(write=False); b.setflags(write=False)
    return A, b


@functools.lru_cache(maxsize=None)
def hermitian_pd():
    """I + B^H B with B = (G + i H) / sqrt(2 n), G and H from the counter streams: Hermitian positive definite, condition number about 2.3"""
    n = N_PARITY
    B = (seeded(n * n, np.float64, 601) + 1j * seeded(n * n, np.float64, 602)).reshape(n, n) / np.sqrt(2.0 * n)
    A = np.asfortranarray(B.conj().T @ B + np.eye(n))
    A = np.asfortranarray((A + A.conj().T) / 2)
    b = seeded(n, np.complex128, 603)
    A.setflags(write=False); b.setflags(write=False)
    return A, b


@functools.lru_cache(maxsize=None)
def three_decades():
    """S (I + E) S with S^2 = a diagonal from 1 to 1000 and E a small symmetric perturbation: SPD, its diagonal spans three decades, and
    Jacobi (M = 1 / diag) brings the condition number from about 1e3 to about that of I + E.  Returns (A, m = 1 / diag(A), b)."""
    n = N_PARITY
    s = np.sqrt(np.logspace(0.0, 3.0, n))
    G = seeded(n * n, np.float64, 611).reshape(n, n) / np.sqrt(n)
    E = 0.3 * (G + G.T) / 2
    A = np.asfortranarray(s[:, None] * (np.eye(n) + E) * s[None, :])
    A = np.asfortranarray((A + A.T) / 2)
    b = seeded(n, np.float64, 613)
    m = 1.0 / np.diag(A).copy()
    for a in (A, m, b):
        a.setflags(write=False)
    return A, m, b


# name -> (builder, rtol, with M).  rtol per case such that no history entry lies within a factor 2 of tol at or before the stopping
# iteration (tests/test_cg_host_logic.py asserts it): the iteration count cannot flip on rounding.  The histories relative to ||b||:
#   dense_spd  iteration 13: 1.41e-09, 14: 2.72e-10;  hermitian_pd  13: 1.65e-09, 14: 3.40e-10;  three_decades_jacobi  10: 3.05e-10, 11: 3.76e-11
# (deep enough that the solution meets ||A x - b||_inf <= 1e-8 ||b||_inf)
PARITY = {
    "dense_spd": (lambda: dense_spd() + (None,), 6.2e-10, False),
    "hermitian_pd": (lambda: hermitian_pd() + (None,), 7.5e-10, False),
    "three_decades_jacobi": (lambda: (three_decades()[0], three_decades()[2], three_decades()[1]), 1.07e-10, True),
}
UNPRECONDITIONED_MAXITER = 110     # the three-decades system without M: nowhere near the tolerance after ten times the Jacobi solve's count


@functools.lru_cache(maxsize=None)
def parity_reference(name):
    """(A, b, m or None, rtol, info, res, x, r, p) of the restatement from x0 = 0"""
    build, rtol, _ = PARITY[name]
    A, b, m = build()
    info, res, x, r, p = cg_long(matop(A), b, np.zeros_like(b), rtol, ATOL, MAXITER, diagop(m) if m is not None else None)
    return A, b, m, rtol, info, res, x, r, p


def tol_of(b, rtol, atol=ATOL):
    return atol + rtol * float(np.linalg.norm(b))


# ---- kernel edges ------------------------------------------------------------------------------------------------------------------------------
EDGE_MAXITER = 3
SMALL_N = (1, 2, 3)


def edge_problem(n, dtype):
    """(d, b): a diagonal in [1, 2] (real for both kinds: Hermitian) and a right-hand side from the counter stream; kappa <= 2"""
    d = (1.0 + (np.arange(n) % 1021) / 1021.0).astype(dtype)
    return d, seeded(n, dtype, 8201)


def edge_reference(n, dtype):
    """(res, x, r, p) after EDGE_MAXITER iterations from x0 = 0 with a tolerance nothing reaches"""
    d, b = edge_problem(n, dtype)
    info, res, x, r, p = cg_long(diagop(d), b, np.zeros(n, dtype=dtype), 0.0, 0.0, EDGE_MAXITER)
    assert info == -EDGE_MAXITER
    return res, x, r, p


def loop_edge_sizes(num_cu, dtype):
    """n at the loop edges of the BLAS-1 grid at "blas1_grid_mult" = 1, plus the smallest vectors"""
    S = stride(10 ** 9, dtype, num_cu, 1)
    return SMALL_N + edge_sizes(S, dtype)


def policy_sizes(dtype):
    """last plain | first non-temporal | non-temporal with an odd last element, at the default multiplier"""
    return POLICY_N[dtype], DEFAULT_MULT


# ---- a solve that converges with look-ahead launches in flight -------------------------------------------------------------------------------
def stop_problem(dtype, n=4099):
    """(d, b, rtol): diagonal with 12 distinct values, so CG converges in at most 12 iterations whatever the tolerance"""
    vals = 1.0 + np.arange(12) / 4.0
    d = vals[np.arange(n) % 12].astype(dtype)
    return d, seeded(n, dtype, 8301), 1e-8


def stop_precond(dtype, n=4099):
    """a diagonal preconditioner that is constant where stop_problem's diagonal is: M A keeps at most 12 distinct values"""
    return (1.0 / (1.0 + 0.5 * ((np.arange(n) % 12) % 3))).astype(dtype)
