"""What tests/test_gpu_operator_kernels.py compares the operator kernels with, checked without a GPU.

The oracle's operators (oracle/oracle.py: DenseOp, Lap5Op, GLOp, DiagOp, DiagLinOp; 'H' as the operator of the conjugate transpose) against
plain longdouble / clongdouble statements of the same operator at the shapes of the GPU tests -- A @ x and A.conj().T @ x, the 5-point
stencil written out with (N+1)**2, the Ginzburg-Landau step as the RK4 polynomial of the stencil's matrix, a scipy-free CSR row loop --, the
adjoint identity <A x, y> = <x, A^H y> in longdouble, the host layouts the GPU tests upload (a leading dimension above n, CSR matrices with
empty rows), and the guard condition of every breakdown input: the oracle stops at the expected step, the entry that stops it lies at least
100 x below the tolerance passed and every earlier one at least 1e3 x above it."""
import numpy as np
import pytest

from oracle import oracle as ora
from tests._gpu_helpers import KINDS, check_entrywise, ext, gamma, is_cplx, product_scale, seeded
from tests._operator_cases import (BIDIAG_N, BREAKDOWN_M, CSR_STREAM_N, DENSE_N, DIAG_N, GL_CASES, GL_RTOL, LAP5_N, LINSPACE_ROW0,
                                   assert_guard_condition, breakdown_cases, check_complex_diag, csr_conj_transpose, csr_dense, csr_longdouble,
                                   csr_stream_case, dense_case, dense_with_lda, diag_case, lap5_input, lap5_longdouble, lap5_three_modes,
                                   linspace_diag_exact, oracle_bidiag_breakdown, oracle_breakdown)

REF_AGREE = GL_RTOL / 10          # oracle against longdouble for the Ginzburg-Landau step: a tenth of the bar of the GPU comparison


def _apply(op, x):
    y = np.empty_like(x)
    op.matvec(np.ascontiguousarray(x), y)
    return y


def _dotl(a, b):
    return complex((ext(a).conj() * ext(b)).sum()) if np.iscomplexobj(a) or np.iscomplexobj(b) else float((ext(a) * ext(b)).sum())


def _assert_adjoint(Ax, y, x, Ahy, absAx_scale, m, what):
    """|<A x, y> - <x, A^H y>| in longdouble within the bound of the two products and the two dots: sums of m + 1 terms against
    |y|^T |A| |x|, taken four times over (two sides, real and imaginary parts)"""
    cp = np.iscomplexobj(x)
    lhs, rhs = (ext(Ax).conj() * ext(y)).sum(), (ext(x).conj() * ext(Ahy)).sum()
    ay = np.abs(y.real) + np.abs(y.imag) if cp else np.abs(y)
    bound = 4.0 * float(gamma(2 * (m + 2) + 5)) * float(ay @ absAx_scale)
    assert abs(lhs - rhs) <= bound, f"{what}: <A x, y> - <x, A^H y> = {abs(lhs - rhs):.2e} > {bound:.2e}"


@pytest.mark.parametrize("dtype", KINDS)
def test_dense_oracle_against_the_longdouble_product(dtype):
    cp = is_cplx(dtype)
    for n in DENSE_N:
        A, x = dense_case(n, dtype)
        Ah = np.asfortranarray(A.conj().T)
        y, yh = _apply(ora.DenseOp(A), x), _apply(ora.DenseOp(Ah), x)
        m = n + (2 if cp else 0)
        check_entrywise(y, ext(A) @ ext(x), product_scale(A, x), m, cp, f"oracle dense n={n} A x")
        check_entrywise(yh, ext(A).conj().T @ ext(x), product_scale(Ah, x), m, cp, f"oracle dense n={n} A^H x")
        w = seeded(n, dtype, 6998)
        _assert_adjoint(y, w, x, _apply(ora.DenseOp(Ah), w), product_scale(A, x), n, f"dense n={n}")
    A, _ = dense_case(257, dtype)
    buf = dense_with_lda(A, 300)                                   # what the GPU test uploads with lda = 300
    assert buf.shape == (300, 257) and np.array_equal(buf[:257], A) and np.isnan(buf[257:]).all()
    assert buf[:257].ctypes.data == buf.ctypes.data and buf.strides[1] == 300 * buf.itemsize


def test_lap5_oracle_against_the_stencil_written_out():
    for N in LAP5_N:
        u = lap5_input(N)
        v = _apply(ora.Lap5Op(N), u)
        ref, scale = lap5_longdouble(N, u)
        check_entrywise(v, ref, scale, 7, False, f"oracle lap5 N={N}")
        w = seeded(N * N, np.float64, 5990)
        _assert_adjoint(v, w, u, _apply(ora.Lap5Op(N), w), scale, 7, f"lap5 N={N}")
    # the stencil in words at a few points of a small grid, independent of the slicing in lap5_longdouble
    N = 4
    u = lap5_input(N)
    ref, _ = lap5_longdouble(N, u)
    g = lambda i, j: np.longdouble(u[i + j * N]) if 0 <= i < N and 0 <= j < N else np.longdouble(0)
    for i in range(N):
        for j in range(N):
            assert ref[i + j * N] == (N + 1) ** 2 * (4 * g(i, j) - g(i - 1, j) - g(i + 1, j) - g(i, j - 1) - g(i, j + 1))
    # a single 1.0 on either side of the segment edge: the product is the stencil column itself
    N = 1026
    for which, i in (("unit511", 511), ("unit512", 512)):
        v = _apply(ora.Lap5Op(N), lap5_input(N, which))
        want = np.zeros(N * N)
        c, s = i + N, float((N + 1) ** 2)
        want[c], want[c - 1], want[c + 1], want[c - N], want[c + N] = 4 * s, -s, -s, -s, -s
        assert np.array_equal(v, want) and np.array_equal(lap5_longdouble(N, lap5_input(N, which))[0].astype(np.float64), want)


def _gl_matrix(A):
    """the matrix of GLOp's right-hand side in clongdouble, written out entry by entry (Ginzburg_Landau.f90:126-136, adjoint :170-179,
    the last row of the second difference divided by 2 dx as there)"""
    n, dx = A.n, np.longdouble(A.dx)
    C, D = np.zeros((n, n), dtype=np.longdouble), np.zeros((n, n), dtype=np.longdouble)
    for i in range(n):
        if i + 1 < n:
            C[i, i + 1] = 1 / (2 * dx)
            D[i, i + 1] = 1 / dx ** 2
        if i > 0:
            C[i, i - 1] = -1 / (2 * dx)
            D[i, i - 1] = 1 / dx ** 2
        D[i, i] = -2 / dx ** 2
    D[n - 1, n - 1], D[n - 1, n - 2] = -2 / (2 * dx), 1 / (2 * dx)
    nu, ga = np.clongdouble(A.nu), np.clongdouble(A.gamma)
    L = (np.conj(nu) * C + np.conj(ga) * D) if A.adjoint else (-nu * C + ga * D)
    return L + np.diag(ext(A.mu))


def _gl_step_longdouble(A, u):
    """nsub steps of the RK4 polynomial u + dt L u + (dt L)^2 u / 2 + (dt L)^3 u / 6 + (dt L)^4 u / 24"""
    L, dt = _gl_matrix(A), np.longdouble(A.tau) / A.nsub
    u = ext(u)
    for _ in range(A.nsub):
        p, acc = u, u
        for k in (1, 2, 3, 4):
            p = dt * (L @ p) / k
            acc = acc + p
        u = acc
    return u


def _gl(n, nsub, adjoint):
    # the defaults of lightkrylov_amd.ginzburg_landau_linop_gpu
    dx, tau = 200.0 / 513.0, 0.01 * nsub
    mu2 = -0.01 * (200.0 / (dx * (n + 1))) ** 2
    return ora.GLOp(n, dx, tau, nsub, 2.0 + 0.2j, 1.0 - 1.0j, 0.38 - 0.2 ** 2, mu2, adjoint=adjoint)


@pytest.mark.parametrize("n,nsub", GL_CASES)
def test_ginzburg_landau_oracle_against_the_rk4_polynomial(n, nsub):
    x, y = seeded(n, np.complex128, 13), seeded(n, np.complex128, 14)
    for adjoint in (False, True):
        A = _gl(n, nsub, adjoint)
        ref = _gl_step_longdouble(A, x)
        err = float(np.abs(A.apply(x) - ref).max() / np.abs(ref).max())
        print(f"GL n={n} nsub={nsub} adjoint={adjoint}: oracle - longdouble = {err:.1e}")
        assert err <= REF_AGREE
    # the adjoint right-hand side is the conjugate transpose of the direct one EXCEPT in the last row / column pair, where the reference
    # divides the second difference by 2 dx: L_adj - L^H has the two entries (n-1, n-2) and (n-2, n-1) and no other
    L, La = _gl_matrix(_gl(n, nsub, False)), _gl_matrix(_gl(n, nsub, True))
    E = La - L.conj().T
    mask = np.zeros((n, n), dtype=bool)
    mask[n - 1, n - 2] = mask[n - 2, n - 1] = True
    assert not E[~mask].any() and E[mask].all()
    # so the adjoint RK4 step is the adjoint of the RK4 polynomial on everything that polynomial (bandwidth 4 nsub) keeps away from that
    # pair: <P x, y> = <x, P_adj y> to rounding for x, y that vanish on the last 4 nsub + 2 points
    keep = n - (4 * nsub + 2)
    if keep > 0:
        x0, y0 = x.copy(), y.copy()
        x0[keep:] = 0
        y0[keep:] = 0
        Px, Pay = _gl_step_longdouble(_gl(n, nsub, False), x0), _gl_step_longdouble(_gl(n, nsub, True), y0)
        lhs, rhs = (Px.conj() * ext(y0)).sum(), (ext(x0).conj() * Pay).sum()
        # the bound, from the longdouble arithmetic alone (u = 2^-64): every intermediate of P x is entrywise at most S |x|, S the same
        # polynomial of |L| (computed below), and an entry of the result has gone through at most 8 roundings per product with L (three
        # complex products of two, two sums, the factor dt, the division by k, the sum into the polynomial) on top of the 6 of an entry of L:
        # 4 nsub products, then a dot of n terms of a complex product each -- m = 14 * 4 nsub + n + 4 roundings on |y|^T S |x|; the same for
        # the adjoint side on |x|^T S_adj |y|; doubled for the real and imaginary parts of each
        m = 14 * 4 * nsub + n + 4
        scale = float(np.abs(y0) @ _gl_abs_polynomial(_gl(n, nsub, False), x0) + np.abs(x0) @ _gl_abs_polynomial(_gl(n, nsub, True), y0))
        bound = 2.0 * m * 2.0 ** -64 / (1.0 - m * 2.0 ** -64) * scale
        print(f"GL n={n} nsub={nsub}: <P x, y> - <x, P_adj y> = {float(abs(lhs - rhs)):.2e}, bound {bound:.2e}")
        assert abs(lhs - rhs) <= bound, (abs(lhs - rhs), bound)


def _gl_abs_polynomial(A, u):
    """S |u|: the RK4 polynomial with |L| (entrywise) in place of L, an entrywise bound of every intermediate of _gl_step_longdouble"""
    L, dt = np.abs(_gl_matrix(A)), np.longdouble(A.tau) / A.nsub
    u = np.abs(ext(u))
    for _ in range(A.nsub):
        p, acc = u, u
        for k in (1, 2, 3, 4):
            p = dt * (L @ p) / k
            acc = acc + p
        u = acc
    return u.astype(np.float64)


@pytest.mark.parametrize("dtype", KINDS)
def test_diagonal_oracles_round_once(dtype):
    cp = is_cplx(dtype)
    for n in DIAG_N:
        d, x = diag_case(n, dtype)
        y, yh = _apply(ora.DiagOp(d), x), _apply(ora.DiagOp(d.conj()), x)
        if cp:
            check_complex_diag(y, d, x, False, f"oracle diag n={n} d x")
            check_complex_diag(yh, d, x, True, f"oracle diag n={n} conj(d) x")
            sc = (np.abs(d.real) + np.abs(d.imag)) * (np.abs(x.real) + np.abs(x.imag))
            w = seeded(n, dtype, 6202)
            _assert_adjoint(y, w, x, _apply(ora.DiagOp(d.conj()), w), sc, 1, f"diag n={n}")
        else:
            assert np.array_equal(y, d * x) and np.array_equal(yh, y)               # one multiplication: one rounding
        if not cp:
            for row0 in LINSPACE_ROW0:
                d0, dstep = 1.0, 1.0 / 3.0e9
                dd = linspace_diag_exact(d0, dstep, row0, n)
                assert np.array_equal(_apply(ora.DiagLinOp(d0, dstep, row0), x), dd * x), (n, row0)
    if not cp:
        # the exact evaluation differs from the twice-rounded d0 + dstep * g somewhere: the inputs can tell one rounding from two
        g = np.arange(10 ** 9 + 1, 10 ** 9 + 1 + 257, dtype=np.float64)
        assert (linspace_diag_exact(1.0, 1.0 / 3.0e9, 10 ** 9 + 1, 257) != 1.0 + (1.0 / 3.0e9) * g).any()


@pytest.mark.parametrize("dtype", KINDS)
def test_csr_stream_inputs_and_the_row_loop(dtype):
    cp = is_cplx(dtype)
    for n in CSR_STREAM_N:
        rowptr, colind, vals = csr_stream_case(n, dtype)
        L = np.diff(rowptr)
        assert rowptr[0] == 0 and rowptr[-1] == len(colind) == len(vals) and (L >= 0).all()
        assert L[0] == 0 and L[-1] == 0 and (n < 257 or (L[1] == 32 and (L[n // 3:n // 3 + min(300, n // 2)] == 0).all()))
        assert n < 4099 or min(300, n // 2) == 300
        assert rowptr[-1] <= 32 * n                                  # mean row length at most 32: the CSR-stream route
        x = seeded(n, dtype, 6301)
        ref, scale, rl = csr_longdouble(rowptr, colind, vals, x)
        tp, tc, tv = csr_conj_transpose(rowptr, colind, vals)
        assert tp[-1] == rowptr[-1] and all((np.diff(tc[tp[i]:tp[i + 1]]) > 0).all() for i in range(n))
        refh, scaleh, rlh = csr_longdouble(tp, tc, tv, x)
        if n <= 257:
            A = csr_dense(rowptr, colind, vals)
            assert np.array_equal(csr_dense(tp, tc, tv), A.conj().T)
            check_entrywise((ext(A) @ ext(x)).astype(dtype), ref, scale, rl + (2 if cp else 0), cp, f"csr row loop n={n}")
            check_entrywise((ext(A).conj().T @ ext(x)).astype(dtype), refh, scaleh, rlh + (2 if cp else 0), cp, f"csr^H row loop n={n}")
        back = csr_conj_transpose(tp, tc, tv)
        assert all(np.array_equal(a, b) for a, b in zip(back, (rowptr, colind, vals)))
        w = seeded(n, dtype, 6302)
        _assert_adjoint(ref, w, x, csr_longdouble(tp, tc, tv, w)[0], scale, int(max(rl.max(), rlh.max(), 1)), f"csr n={n}")


@pytest.mark.parametrize("dtype", KINDS)
def test_breakdown_inputs_meet_the_guard_condition(dtype):
    for name, (_Ao, _rec, _n, _x0, k, _tol) in breakdown_cases(dtype).items():
        for which in ("arnoldi", "lanczos") if name in ("dense", "lap5") else ("arnoldi",):
            info, H, tol = oracle_breakdown(name, dtype, which)
            sub = np.abs(np.diag(H, -1))
            print(f"{np.dtype(dtype).name} {name} {which}: info = {info}, subdiagonal {sub[:k]}")
            assert info == k, (name, which, info)
            assert_guard_condition(sub, k, tol, f"{name} {which}")
            assert not H[:, k:].any()
    info, B, R, _u0, tol = oracle_bidiag_breakdown(dtype)
    assert info == 3 and R.shape == (BIDIAG_N, BIDIAG_N)
    # Golub-Kahan visits alpha_1, beta_1, alpha_2, beta_2, alpha_3: the fifth stops it
    order = np.abs([B[0, 0], B[1, 0], B[1, 1], B[2, 1], B[2, 2]])
    print(f"{np.dtype(dtype).name} bidiag: {order}")
    assert_guard_condition(order, 5, tol, "bidiag")
    assert BREAKDOWN_M > 7


def test_lap5_breakdown_start_vector_lies_in_three_modes():
    x0 = lap5_three_modes()
    N = 31
    i = np.arange(1, N + 1)
    S = np.sin(np.outer(i, i) * np.pi / (N + 1)) * np.sqrt(2.0 / (N + 1))           # orthonormal sine matrix
    coef = S @ x0.reshape(N, N) @ S
    big = np.abs(coef) > 1e-12
    assert big.sum() == 3 and np.allclose(np.abs(coef[big]), 1 / np.sqrt(3), rtol=1e-12)


@pytest.mark.parametrize("dtype", KINDS)
def test_entrywise_check_refuses_an_entry_nobody_wrote(dtype):
    """the GPU tests start y as NaN: check_entrywise must fail on a NaN left in the result, also where the bound is 0 (an empty CSR row),
    and so must the complex diagonal check"""
    cp = is_cplx(dtype)
    A, x = dense_case(9, dtype)
    ref, scale = ext(A) @ ext(x), product_scale(A, x)
    good = (ext(A) @ ext(x)).astype(dtype)
    assert check_entrywise(good, ref, scale, 9, cp, "finite") <= 1.0
    for i in (0, 8):
        bad = good.copy()
        bad[i] = np.nan
        with pytest.raises(AssertionError):
            check_entrywise(bad, ref, scale, 9, cp, "a NaN entry")
    with pytest.raises(AssertionError):
        check_entrywise(np.full(3, np.nan, dtype=dtype), ext(np.zeros(3, dtype=dtype)), np.zeros(3), np.zeros(3), cp, "NaN where the bound is 0")
    if cp:
        d, x = diag_case(3, dtype)
        y = d * x
        y[1] = np.nan
        with pytest.raises(AssertionError):
            check_complex_diag(y, d, x, False, "a NaN entry")
