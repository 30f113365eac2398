"""Shapes, inputs, longdouble references and breakdown cases of the operator-kernel tests: tests/test_gpu_operator_kernels.py runs them on the
engine, tests/test_oracle_operators.py pins them without a GPU.  Inputs come from the oracle's counter generator."""
import functools

import numpy as np

from oracle import oracle as ora
from tests._gpu_helpers import arnoldi_operator, basis, ext, gamma, is_cplx, orthonormal_basis, seeded

DENSE_N = (1, 2, 3, 7, 8, 9, 255, 256, 257, 511, 512, 513, 769, 1025)          # 8-column unroll, 1 / 2 / 3 / 5 chunks, 512 / 256-row blocks
LAP5_N = (1, 2, 3, 4, 126, 127, 128, 129, 510, 511, 512, 513, 514, 1026)        # wave edge (128 points), 512-point segments 1 -> 2 -> 3
GL_CASES = [(n, nsub) for n in (3, 255, 256, 257, 513) for nsub in (1, 2)]     # the 256-thread block edge
GL_RTOL = 1e-13                   # tests/test_gpu_parity.py::test_ginzburg_landau_stepper_against_oracle: max |y - ref| <= 1e-13 max |ref|
DIAG_N = (1, 2, 3, 255, 257)
LINSPACE_ROW0 = (0, 1, 10 ** 9 + 1)
CSR_STREAM_N = (1, 257, 4099)
BREAKDOWN_TOL = 1e-10             # the tolerance the breakdown tests of tests/test_gpu_pipelines.py pass
BREAKDOWN_M = 12                  # columns of the factorisations with a breakdown: steps beyond it hold markers
LAP5_BREAKDOWN_TOL = 1e-6         # ||A|| = 8 (N+1)**2 = 8192 and the sines of x0 are rounded: the oracle leaves 8e-10 at the breakdown


@functools.lru_cache(maxsize=4)
def dense_case(n, dtype):
    """(A, x): an n x n matrix (column j from the counter stream 7000 + j) and a vector (stream 6999); read-only, shared"""
    A, x = basis(n, n, dtype, 7000), seeded(n, dtype, 6999)
    A.setflags(write=False)
    x.setflags(write=False)
    return A, x


def lap5_longdouble(N, u):
    """v = (N+1)**2 (4 u_c - left - right - lower - upper) on the N x N grid (point (i, j) at i + j N, Dirichlet) in longdouble, and
    the scale (N+1)**2 (4 |u_c| + sum |neighbours|) of its entrywise bound: each entry is at most 5 terms, a multiplication by 4
    (exact) and one by the scale -- gamma(7) covers any order"""
    s = np.longdouble((N + 1) ** 2)
    g = ext(u).reshape(N, N)                                       # g[j, i]
    nb, na = np.zeros_like(g), np.zeros_like(g)
    for sl_to, sl_from in (((slice(None), slice(1, None)), (slice(None), slice(None, -1))),
                           ((slice(None), slice(None, -1)), (slice(None), slice(1, None))),
                           ((slice(1, None), slice(None)), (slice(None, -1), slice(None))),
                           ((slice(None, -1), slice(None)), (slice(1, None), slice(None)))):
        nb[sl_to] += g[sl_from]
        na[sl_to] += np.abs(g[sl_from])
    return (s * (4 * g - nb)).ravel(), (s * (4 * np.abs(g) + na)).astype(np.float64).ravel()


def lap5_input(N, which="random"):
    """a counter-stream grid function, or a single 1.0 at point i of grid line 1 ("unit511" / "unit512": either side of a 512-point
    segment edge of N = 1026, where the product is the stencil column itself)"""
    if which == "random":
        return seeded(N * N, np.float64, 6000 + N)
    u = np.zeros(N * N)
    u[int(which[4:]) + N] = 1.0
    return u


def linspace_diag_exact(d0, dstep, row0, n):
    """d_i = d0 + dstep (row0 + i) evaluated EXACTLY (integers over a common power-of-two denominator) and rounded once to double --
    "ONE rounding per d_i" (k_diag_linspace).  A longdouble product of a 53-bit step and a 31-bit row index is not exact, and rounding
    its sum to 64 and then to 53 bits is not one rounding."""
    (an, ad), (sn, sd) = float(d0).as_integer_ratio(), float(dstep).as_integer_ratio()
    D = max(ad, sd)
    A, S = an * (D // ad), sn * (D // sd)
    return np.array([(A + S * g) / D for g in range(row0, row0 + n)], dtype=np.float64)      # int / int: correctly rounded


def diag_case(n, dtype):
    """(d, x): d = (1 + i / n) turned in the complex plane for the complex kind, times a counter stream; x another stream"""
    return (arnoldi_operator(n, dtype) * seeded(n, dtype, 6200)).astype(dtype), seeded(n, dtype, 6201)


def csr_stream_case(n, dtype):
    """(rowptr, colind, vals) of an n x n matrix of SHORT rows (mean length about 2: the CSR-stream route): rows of 0 .. 4 entries,
    an empty first and last row, a run of min(300, n // 2) empty rows from row n // 3, row 1 of exactly 32 entries (n >= 257);
    column indices ascending within a row, values from the counter stream 6300.  No scipy."""
    L = np.array([(7 * i) % 5 for i in range(n)], dtype=np.int64)
    L[n // 3:n // 3 + min(300, n // 2)] = 0
    L[0] = L[n - 1] = 0
    if n >= 257:
        L[1] = 32
    rowptr = np.concatenate([[0], np.cumsum(L)]).astype(np.int64)
    q = max(n // 4, 1)
    cols = [np.sort((5 + 8 * np.arange(32)) % n) if l == 32 else np.sort((i + q * np.arange(l)) % n) for i, l in enumerate(L)]
    colind = (np.concatenate(cols) if rowptr[-1] else np.zeros(0)).astype(np.int32)
    for i in range(n):
        c = colind[rowptr[i]:rowptr[i + 1]]
        assert len(np.unique(c)) == L[i] and (c >= 0).all() and (c < n).all()
    vals = seeded(int(rowptr[-1]), dtype, 6300)
    return rowptr, colind, vals


def csr_conj_transpose(rowptr, colind, vals):
    """A^H in CSR by a stable counting sort (column indices of a row of A^H ascending)"""
    n = len(rowptr) - 1
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    order = np.argsort(colind, kind="stable")
    tp = np.concatenate([[0], np.cumsum(np.bincount(colind, minlength=n))]).astype(np.int64)
    return tp, rows[order].astype(np.int32), np.conj(vals[order])


def csr_longdouble(rowptr, colind, vals, x):
    """the row loop y_i = sum_p a_p x_(col p) in longdouble, the scale sum |a_p| |x_(col p)| of its bound, and the row lengths"""
    xe, ve = ext(x), ext(vals)
    n = len(rowptr) - 1
    cp = np.iscomplexobj(vals)
    ref = np.zeros(n, dtype=ve.dtype)
    scale = np.zeros(n)
    ax = np.abs(x.real) + np.abs(x.imag) if cp else np.abs(x)
    av = np.abs(vals.real) + np.abs(vals.imag) if cp else np.abs(vals)
    for i in range(n):
        p = slice(rowptr[i], rowptr[i + 1])
        ref[i] = (ve[p] * xe[colind[p]]).sum()
        scale[i] = (av[p] * ax[colind[p]]).sum()
    return ref, scale, np.diff(rowptr)


def csr_dense(rowptr, colind, vals):
    n = len(rowptr) - 1
    A = np.zeros((n, n), dtype=vals.dtype, order="F")
    A[np.repeat(np.arange(n), np.diff(rowptr)), colind] = vals
    return A


# ---- breakdown inputs: operators whose Krylov space from x0 has a known small dimension ----------------------------------------------------
SIX = np.array([1.0, 1.5, 2.25, 3.0, 4.0, 5.5])


@functools.lru_cache(maxsize=8)
def six_eigenvalue_matrix(n, dtype, seed=6400):
    """A = Q diag(lambda) Q^H, Q from orthonormal_basis, the six values of SIX each repeated n / 6 times: symmetric / Hermitian, and
    the Krylov space of any start vector has dimension 6"""
    Q = orthonormal_basis(n, n, dtype, seed)
    A = np.asfortranarray((Q * SIX[np.arange(n) % 6]) @ Q.conj().T)
    A = np.asfortranarray((A + A.conj().T) / 2)
    A.setflags(write=False)
    return A


def start_vector(n, dtype, seed):
    """unit vector from a counter stream (a seed outside 6400 .. 7000, the streams of the columns that Q is made of)"""
    x = seeded(n, dtype, seed)
    return x / np.linalg.norm(x)


def six_diagonal_csr(n, dtype):
    """diag(SIX[i mod 6]) in CSR, one entry per row: the CSR-stream route"""
    return np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32), SIX[np.arange(n) % 6].astype(dtype)


def six_block_csr(nblocks, dtype):
    """nblocks copies of the dense 40 x 40 six-eigenvalue matrix on the diagonal, in CSR: rows of exactly 40 entries (mean row length
    above 32: the lanes-per-row route), six distinct eigenvalues"""
    B = six_eigenvalue_matrix(40, dtype, 6500)
    n = 40 * nblocks
    rowptr = 40 * np.arange(n + 1, dtype=np.int64)
    colind = (40 * (np.arange(n) // 40)[:, None] + np.arange(40)[None, :]).astype(np.int32).ravel()
    vals = np.ascontiguousarray(np.tile(np.ascontiguousarray(B), (nblocks, 1))).ravel()      # row i of the matrix = row i mod 40 of B
    return rowptr, colind, vals


LAP5_BREAKDOWN_N = 31
LAP5_MODES = ((1, 1), (2, 3), (5, 7))


def lap5_three_modes(N=LAP5_BREAKDOWN_N, modes=LAP5_MODES):
    """x0 = a normalised sum of three discrete sine modes sin(p pi i / (N+1)) sin(q pi j / (N+1)) with distinct eigenvalues
    (N+1)**2 (4 - 2 cos(p pi / (N+1)) - 2 cos(q pi / (N+1))): a 3-dimensional invariant subspace of the 5-point Laplacian"""
    i = np.arange(1, N + 1)
    lam = [(N + 1) ** 2 * (4 - 2 * np.cos(p * np.pi / (N + 1)) - 2 * np.cos(q * np.pi / (N + 1))) for p, q in modes]
    assert len(set(np.round(lam, 6))) == len(modes)
    x = sum(np.outer(np.sin(q * np.pi * i / (N + 1)), np.sin(p * np.pi * i / (N + 1))).ravel() * np.sqrt(2.0 / (N + 1)) ** 2 for p, q in modes)
    return x / np.linalg.norm(x)


def rank_two_operator(n, dtype):
    """(a b^H + c e^H) / n from the counter streams 31 .. 34, as tests/test_gpu_pipelines.py builds it: Golub-Kahan breaks down in the
    right half of step 3"""
    a, b, c_, e = (seeded(n, dtype, s_) for s_ in (31, 32, 33, 34))
    return np.asfortranarray((np.outer(a, b.conj()) + np.outer(c_, e.conj())).astype(dtype) / n)


def assert_guard_condition(sub, k, tol, what):
    """A condition on the INPUT of a breakdown test, from the oracle's factorisation alone: the entry that stops the factorisation at
    step k (`sub[k - 1]`) is at least 100 x below `tol`, every earlier one at least 1e3 x above it -- the guard of the asynchronous batch
    cannot trip a step early or late because of rounding that differs between the oracle and the engine"""
    sub = np.abs(np.asarray(sub))
    assert sub[k - 1] <= tol / 100, f"{what}: the stopping entry {sub[k - 1]:.2e} is not 100 x below tol = {tol:.0e}"
    assert (sub[:k - 1] >= 1e3 * tol).all(), f"{what}: an entry before the breakdown, {sub[:k - 1].min():.2e}, is within 1e3 x of tol = {tol:.0e}"


def breakdown_cases(dtype):
    """name -> (oracle operator, engine-operator recipe, n, x0, expected breakdown step, tol); the recipes: ("dense", A),
    ("csr", (rowptr, colind, vals)), ("lap5", N).  Dense and CSR for both kinds, the stencil for the real kind."""
    n = 600
    A = six_eigenvalue_matrix(n, dtype)
    out = {"dense": (ora.DenseOp(A), ("dense", A), n, start_vector(n, dtype, 5901), 6, BREAKDOWN_TOL)}
    d6 = six_diagonal_csr(n, dtype)
    out["csr_stream"] = (ora.DiagOp(d6[2]), ("csr", d6), n, start_vector(n, dtype, 5902), 6, BREAKDOWN_TOL)
    blk = six_block_csr(15, dtype)
    out["csr_lanes"] = (ora.DenseOp(csr_dense(*blk)), ("csr", blk), n, start_vector(n, dtype, 5903), 6, BREAKDOWN_TOL)
    if not is_cplx(dtype):
        N = LAP5_BREAKDOWN_N
        out["lap5"] = (ora.Lap5Op(N), ("lap5", N), N * N, lap5_three_modes(), 3, LAP5_BREAKDOWN_TOL)
    return out




@functools.lru_cache(maxsize=32)
def oracle_breakdown(name, dtype, which="arnoldi"):
    """(info, projected matrix, tol) of the oracle's Arnoldi / Lanczos factorisation of breakdown case `name`; computed once, read-only"""
    Ao, _rec, n, x0, _k, tol = breakdown_cases(dtype)[name]
    m = BREAKDOWN_M
    X = np.zeros((n, m + 1), dtype=dtype, order="F")
    X[:, 0] = x0
    H = np.zeros((m + 1, m), dtype=dtype, order="F")
    info = (ora.arnoldi if which == "arnoldi" else ora.lanczos)(Ao, X, H, tol=tol)
    H.setflags(write=False)
    return info, H, tol


BIDIAG_N = 601


@functools.lru_cache(maxsize=4)
def oracle_bidiag_breakdown(dtype):
    """(info, B, R, u0, tol): Golub-Kahan on the rank-two operator, oracle side"""
    n, m = BIDIAG_N, BREAKDOWN_M
    R = rank_two_operator(n, dtype)
    u0 = start_vector(n, dtype, 4)
    Uo = np.zeros((n, m + 1), dtype=dtype, order="F")
    Uo[:, 0] = u0
    Vo = np.zeros((n, m + 1), dtype=dtype, order="F")
    Bo = np.zeros((m + 1, m), dtype=dtype, order="F")
    info = ora.bidiagonalization(ora.DenseOp(R), ora.DenseOp(np.asfortranarray(R.conj().T)), Uo, Vo, Bo, tol=BREAKDOWN_TOL)
    return info, Bo, R, u0, BREAKDOWN_TOL


def dense_with_lda(A, lda):
    """the host image of A with leading dimension lda > n: an (lda, n) column-major buffer whose rows [n, lda) are NaN, and the
    n x n view of it that lk_linop_dense_create reads (the last element read is (n - 1) lda + n - 1 < lda n)"""
    n = A.shape[0]
    buf = np.full((lda, n), np.nan, dtype=A.dtype, order="F")
    buf[:n, :] = A
    assert lda >= n and (n - 1) * lda + n <= buf.size and buf.flags.f_contiguous
    return buf


def check_complex_diag(got, d, x, conj, label):
    """y = d x or conj(d) x, complex, per component within gamma(2) of that component's own two products:
        Re: fl(ar br -+ fl(ai bi)), Im: fl(ar bi +- fl(ai br))      (diag_cmul / diag_cmulconj: one rounded product, one fused multiply-add)
    err = -+ ai bi d1 + (ar br -+ ai bi (1 + d1)) d2, |d1|, |d2| <= u, so |err| <= u |ai bi| + u (|ar br| + |ai bi|) (1 + u)
    <= gamma(2) (|ar br| + |ai bi|); two rounded products and a rounded sum (no fused multiply-add) stay within (1 + u)^2 - 1 <= gamma(2) of the
    same scale.  Either scale is at most |d| |x|.  gamma() adds the longdouble reference's own rounding.  Returns the worst ratio."""
    from tests._tol import _report
    ref = (ext(d).conj() if conj else ext(d)) * ext(x)
    e = np.asarray(got).astype(ref.dtype) - ref
    ar, ai, br, bi = np.abs(d.real), np.abs(d.imag), np.abs(x.real), np.abs(x.imag)
    g2 = float(gamma(2))
    ratio = 0.0
    for err, scale in ((np.abs(e.real).astype(np.float64), ar * br + ai * bi), (np.abs(e.imag).astype(np.float64), ar * bi + ai * br)):
        bound = g2 * scale
        bad = ~(err <= bound)
        assert not bad.any(), f"{label}: entry {int(np.flatnonzero(bad)[0])} off by {err[bad][0]:.3e} > gamma(2) bound {bound[bad][0]:.3e}"
        ratio = max(ratio, float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0)
    _report(label, ratio, 1.0, "gamma(2) per component")
    return ratio
