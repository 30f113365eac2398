"""Inputs of the lk_gmres tests, stated once: tests/test_gmres_host_logic.py pins them against the oracle without a GPU,
tests/test_gpu_gmres_engine.py and tests/test_gpu_gmres_edges.py run them on the device."""
import functools

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


# ---- the edges of lk_gmres' contract (tests/test_gpu_gmres_edges.py; pinned on the CPU in tests/test_gmres_host_logic.py) ----------------
EPS = float(np.finfo(np.float64).eps)


def powers_of_two_diag(dtype, n):
    """d_i = 2^(i mod 5), times 1 / i / -1 / -i in turn for the complex kind: b / d and d * (b / d) are exact in binary floating point"""
    i = np.arange(n)
    d = (2.0 ** (i % 5)).astype(dtype)
    if is_cplx(dtype):
        d = d * np.array([1.0, 1.0j, -1.0, -1.0j])[i % 4]
    return d


def exact_guess(dtype, n):
    """(d, b, x0) with b - d * x0 exactly zero: x0 = b / d on powers_of_two_diag"""
    d = powers_of_two_diag(dtype, n)
    b = seeded(n, dtype, 17)
    return d, b, b / d


EXACT_GUESS_N = (1, 257)
ZERO_B = dict(n=257, atols=(0.0, 1e-12))    # b = 0, x0 = 0 on powers_of_two_diag: a zero start residual whatever atol is


def few_eigenvalues_diag(dtype, n=257):
    """m = 3 distinct, well separated eigenvalues repeated over the diagonal: the Krylov space of any b has dimension 3"""
    vals = np.array([1.0, 2.0j, -4.0] if is_cplx(dtype) else [1.0, 2.0, 4.0], dtype=dtype)
    return vals[np.arange(n) % 3]


class EdgeCase:
    """One solve of op(A) x = b from x0.  `form`: "diag" (A is the diagonal, a vector) or "dense"; `atol` is RELATIVE to ||b||.
    `pin(dtype)`: what ora.gmres gives on the CPU, (info, n_inner, n_outer, len(history)), asserted there and on the GPU (EDGE_PINS)."""

    def __init__(self, name, form, make, kdim, maxiter, rtol, atol=0.0, trans=False, converges=True):
        self.name, self.form, self.make, self.kdim, self.maxiter, self.rtol, self.atol_rel = name, form, make, kdim, maxiter, rtol, atol
        self.trans, self.converges = trans, converges

    def pin(self, dtype):
        return EDGE_PINS[self.name][1 if is_cplx(dtype) else 0]

    def inputs(self, dtype):
        """(A, b, x0); A as stored (the product is op(A) = A^H with `trans`)"""
        return self.make(dtype)

    def op_matrix(self, A):
        return A.conj().T if self.form == "dense" and self.trans else (A.conj() if self.trans else A)

    def tolerances(self, b):
        return self.rtol, self.atol_rel * float(np.linalg.norm(b))


def _warm(base):
    def make(dtype):
        A, b = base(dtype)
        return A, b, seeded(b.size, dtype, 19)
    return make


def _cold(base, **kw):
    def make(dtype):
        A, b = base(dtype, **kw)
        return A, b, np.zeros(b.size, dtype=dtype)
    return make


def _atol_only(dtype):
    """pipelines_diag; for the complex kind its MODULUS, as a complex diagonal.  givens_rotation (submodule_utility_functions.fypp:173-204)
    builds c = h(k) / nrm without a conjugate, which is a rotation only where H's diagonal is real: on the complex diagonal itself the
    oracle's estimate |e(k+1)| ends 10 times below the residual it stands for (1.26e-4 against 1.45e-3 at tol = 1.41e-4) and the solve
    counts as converged outside the longdouble bound.  A Hermitian operator keeps H's diagonal real, estimate and residual agree."""
    d, b = pipelines_diag(dtype)
    return (np.abs(d).astype(dtype) if is_cplx(dtype) else d), b, np.zeros(b.size, dtype=dtype)


def _few(dtype):
    d = few_eigenvalues_diag(dtype)
    return d, seeded(d.size, dtype, 17), np.zeros(d.size, dtype=dtype)


def _edge_cases():
    out = []
    for form, base in (("dense", dense_nonsymmetric), ("diag", pipelines_diag)):
        for kdim, maxiter in ((40, 5), (5, 30)):
            for trans in (False, True):
                out.append(EdgeCase(f"warm_start-{form}-k{kdim}-{'H' if trans else 'N'}", form, _warm(base), kdim, maxiter, 1e-10, trans=trans))
    # the Krylov space of b has dimension 3: step 3 converges with H(4, 3) at rounding level -- history r0 | 3 steps | the cycle's residual
    out.append(EdgeCase("few_eigenvalues", "diag", _few, 10, 2, 1e-10))
    # the space is exhausted at step n: that step converges (its estimate is rounding noise), whatever kdim is; n > kdim restarts instead
    for n in (1, 2, 5):
        for kdim in (2, 8):
            # (n = 5, kdim = 2 is not exhausted: GMRES(2) restarts, and needs more than the 4 cycles of maxiter = 3 to reach 1e-10)
            out.append(EdgeCase(f"exhausted-n{n}-k{kdim}", "dense", _cold(dense_nonsymmetric, n=n), kdim, 3 if n <= kdim else 12, 1e-10))
    out.append(EdgeCase("min_kdim", "dense", _cold(dense_nonsymmetric), 2, 200, 1e-8))
    out.append(EdgeCase("atol_only", "diag", _atol_only, 30, 10, 0.0, atol=1e-6))
    out.append(EdgeCase("one_cycle", "dense", _cold(dense_nonsymmetric), 5, 0, 1e-14, converges=False))
    # tiny_diag from x0 != 0: every H(k+1, k) <= tol with the residual far above it, so each cycle's batch ends at its first step with the solve
    # going on -- the vector is scaled back and the remaining steps run one by one (gmres.fypp:171-172), behind a start residual with a product
    out.append(EdgeCase("unscaled_warm", "diag", _warm(tiny_diag), TINY["kdim"], TINY["maxiter"], TINY["rtol"], converges=False))
    return tuple(out)


EDGE_CASES = _edge_cases()

# (info, n_inner, n_outer, len(history)) of ora.gmres, real kind | complex kind.  The oracle returns info and the history; the history has
# 1 + n_inner + n_outer entries, |info| = n_inner + n_outer, and every cycle but the last runs all kdim steps, so n_outer =
# ceil(|info| / (kdim + 1)): tests/test_gmres_host_logic.py asserts all of that.  Nothing here rests on rounding noise: where a Krylov
# space is exhausted (few_eigenvalues at step 3, exhausted-n* at step n <= kdim) that step's estimate is 1e-16 |r0| against tol = 1e-10 |r0|
# and ends the cycle, so the oracle never takes the step behind it.
EDGE_PINS = {
    "warm_start-dense-k40-N": ((14, 13, 1, 15), (17, 16, 1, 18)),
    "warm_start-dense-k40-H": ((14, 13, 1, 15), (17, 16, 1, 18)),
    "warm_start-dense-k5-N": ((16, 13, 3, 17), (20, 16, 4, 21)),
    "warm_start-dense-k5-H": ((16, 13, 3, 17), (20, 16, 4, 21)),
    "warm_start-diag-k40-N": ((45, 43, 2, 46), (65, 63, 2, 66)),
    "warm_start-diag-k40-H": ((45, 43, 2, 46), (65, 63, 2, 66)),
    "warm_start-diag-k5-N": ((62, 51, 11, 63), (77, 64, 13, 78)),
    "warm_start-diag-k5-H": ((62, 51, 11, 63), (77, 64, 13, 78)),
    "few_eigenvalues": ((4, 3, 1, 5), (4, 3, 1, 5)),
    "exhausted-n1-k2": ((2, 1, 1, 3), (2, 1, 1, 3)),
    "exhausted-n1-k8": ((2, 1, 1, 3), (2, 1, 1, 3)),
    "exhausted-n2-k2": ((3, 2, 1, 4), (3, 2, 1, 4)),
    "exhausted-n2-k8": ((3, 2, 1, 4), (3, 2, 1, 4)),
    "exhausted-n5-k2": ((17, 11, 6, 18), (18, 12, 6, 19)),
    "exhausted-n5-k8": ((6, 5, 1, 7), (6, 5, 1, 7)),
    "min_kdim": ((15, 10, 5, 16), (18, 12, 6, 19)),
    "atol_only": ((25, 24, 1, 26), (25, 24, 1, 26)),
    "one_cycle": ((-6, 5, 1, 7), (-6, 5, 1, 7)),
    "unscaled_warm": ((-8, 6, 2, 9), (-8, 6, 2, 9)),
}


def oracle_operator(case, A):
    """the oracle's operator for op(A)"""
    from oracle import oracle as ora
    Ao = case.op_matrix(A)
    return ora.DiagOp(np.ascontiguousarray(Ao)) if case.form == "diag" else ora.DenseOp(np.asfortranarray(Ao))


def _ext(a):
    a = np.asarray(a)
    return a.astype(np.clongdouble if a.dtype.kind == "c" else np.longdouble)


def longdouble_solve(A, b):
    """A x = b by Gaussian elimination with partial pivoting in longdouble / clongdouble, written out (numpy's solvers stop at double)"""
    A, b = _ext(A).copy(), _ext(b).copy()
    n = b.size
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]
            b[[k, p]] = b[[p, k]]
        f = A[k + 1:, k] / A[k, k]
        A[k + 1:, k + 1:] -= np.outer(f, A[k, k + 1:])
        b[k + 1:] -= f * b[k]
    x = np.zeros(n, dtype=A.dtype)
    for k in range(n - 1, -1, -1):
        x[k] = (b[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


def long_product(case, A, v):
    """op(A) v in longdouble"""
    Ao, vl = _ext(case.op_matrix(A)), _ext(v)
    return Ao * vl if case.form == "diag" else Ao @ vl


def long_norm(v):
    return float(np.sqrt(np.sum(np.abs(_ext(v)) ** 2)))


def frobenius(A):
    return long_norm(np.asarray(A).ravel())


def reference_solution(case, A, b):
    """the longdouble solution of op(A) x = b: b / d for the diagonal cases, the written-out elimination for the dense ones"""
    Ao = case.op_matrix(A)
    return _ext(b) / _ext(Ao) if case.form == "diag" else longdouble_solve(Ao, b)


def residual_bound(case, A, b, x):
    """tol + 8 n eps ||A||_F ||x||: the stopping test plus the rounding of one double-precision residual"""
    rtol, atol = case.tolerances(b)
    return atol + rtol * float(np.linalg.norm(b)) + 8.0 * b.size * EPS * frobenius(A) * long_norm(x)


def start_residual_bound(A, x0):
    """8 n eps ||A||_F ||x0||: the rounding of the one double-precision residual b - op(A) x0"""
    return 8.0 * x0.size * EPS * frobenius(A) * long_norm(x0)


def assert_solves(case, A, b, x, xref, label):
    """||op(A) (x* - x)|| in longdouble -- the residual of x, through the longdouble solution x* -- within residual_bound; x*'s own
    residual is checked against the longdouble rounding of one product first, so that the reference is one"""
    own = long_norm(_ext(b) - long_product(case, A, xref))
    assert own <= 8.0 * b.size * 2.0 ** -63 * frobenius(A) * long_norm(xref), f"{label}: the longdouble reference leaves {own:.2e}"
    r, bound = long_norm(long_product(case, A, xref - _ext(x))), residual_bound(case, A, b, x)
    print(f"{label}: residual {r:.3e}, bound {bound:.3e}")
    assert r <= bound, f"{label}: ||b - op(A) x|| = {r:.3e} > {bound:.3e}"
    return r


@functools.lru_cache(maxsize=None)
def oracle_run(name, kind):
    """ora.gmres on the edge case `name` for the kind "float64" / "complex128", computed once per process and shared, read-only:
    (A, b, x0, info, history, x, the longdouble solution or None where the case does not converge)"""
    case = next(c for c in EDGE_CASES if c.name == name)
    from oracle import oracle as ora
    dtype = np.dtype(kind).type
    A, b, x0 = case.inputs(dtype)
    x = x0.copy()
    rtol, atol = case.tolerances(b)
    info, res = ora.gmres(oracle_operator(case, A), b, x, rtol=rtol, atol=atol, kdim=case.kdim, maxiter=case.maxiter)
    xref = reference_solution(case, A, b) if case.converges else None
    for a in (A, b, x0, res, x) + (() if xref is None else (xref,)):
        a.setflags(write=False)
    return A, b, x0, info, res, x, xref
