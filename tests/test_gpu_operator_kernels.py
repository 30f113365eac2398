"""The operator kernels behind lk_linop_apply (k_gemv_n / k_gemv_n_finish, k_gemv_h, k_lap5, k_gl_stage, k_diag, k_diag_linspace, k_csr_stream),
each on its own, at the smallest sizes on either side of every tiling edge.

(a) Every entry of y = op(A) x against a longdouble statement of the same operator within the a-priori bound of its sum,
        |got - ref|_i <= gamma_m (|A| |x|)_i       (tests/_gpu_helpers.py: gamma, check_entrywise; m = the terms of the entry, + 2 complex),
    bit for bit where one rounding per entry is promised (the real diagonal operators, the symmetric stencil's rmatvec), the Ginzburg-Landau
    step against the oracle at the tolerance of tests/test_gpu_parity.py.  tests/test_oracle_operators.py pins every reference without a GPU.
(b) x and y as columns of two caller-owned panels (lk_basis_wrap) in two buffers with different ld: no word outside rows [0, n) of y's column
    changes, x's buffer does not change at all, and the result still meets (a).
(c) The guard every operator kernel opens with: a breakdown of the asynchronous Arnoldi / Lanczos / Golub-Kahan batch on a dense, a CSR
    (both routes) and the stencil operator leaves the marker columns beyond it bit-identical, on the three sweeps and on the single launch,
    with the oracle's info and projected matrix.

The measured worst ratio of every case goes to $LK_TOL_REPORT."""
import ctypes as C

import numpy as np
import pytest

import lightkrylov_amd as lk
from lightkrylov_amd import _capi
from lightkrylov_amd.linops import _engine_linop
from oracle import oracle as ora
from tests._gpu_helpers import KINDS, CallerPanel, check_entrywise, device_num_cu, ext, is_cplx, product_scale, seeded
from tests._operator_cases import (BIDIAG_N, BREAKDOWN_M, CSR_STREAM_N, DENSE_N, DIAG_N, GL_CASES, GL_RTOL, LAP5_N, LINSPACE_ROW0, breakdown_cases,
                                   check_complex_diag, csr_conj_transpose, csr_longdouble, csr_stream_case, dense_case, dense_with_lda,
                                   diag_case, lap5_input, lap5_longdouble, linspace_diag_exact, oracle_bidiag_breakdown, oracle_breakdown)
from tests._tol import _report, assert_columns_close

pytestmark = pytest.mark.gpu

BLAS1_GRID_MULT = 2
D0, DSTEP = 1.0, 1.0 / 3.0e9                      # the generated diagonal of these tests: d_i = D0 + DSTEP (row0 + i)


@pytest.fixture(scope="module")
def kctx():
    c = lk.Context(device=0)
    c.set_tuning("blas1_grid_mult", BLAS1_GRID_MULT)              # the defaults, stated once: _diag_big_n and the CSR route depend on them
    c.set_tuning("csr_stream", 1)
    yield c
    c.close()


def _name(dtype):
    return np.dtype(dtype).name


def _apply(op, trans, xh, c):
    """y = op(A) x on pool vectors; y starts as NaN, so an entry the kernel leaves out shows"""
    x = lk.dense_vector_gpu.from_array(np.ascontiguousarray(xh), c)
    y = lk.dense_vector_gpu.from_array(np.full(len(xh), np.nan, dtype=xh.dtype), c)
    (op.apply_rmatvec if trans else op.apply_matvec)(x, y)
    assert np.array_equal(x.to_array(), xh)
    return y.to_array()


def _dense_op(c, A, lda=None):
    """lk_linop_dense_create, with a host leading dimension above n through the C interface (rows [n, lda) of the host image are NaN)"""
    if lda is None:
        return lk.dense_linop_gpu(A, c)
    buf = dense_with_lda(A, lda)
    op = lk.dense_linop_gpu.__new__(lk.dense_linop_gpu)
    _engine_linop.__init__(op, c)
    op.dtype, op.n = A.dtype, A.shape[0]
    _capi.check(op._lib.lk_linop_dense_create(c._h, _capi.LK_C128 if is_cplx(A.dtype) else _capi.LK_F64, op.n, buf.ctypes.data_as(C.c_void_p),
                                              lda, C.byref(op._h)))
    return op


def _check_dense(got, A, x, trans, label):
    cp = is_cplx(A.dtype)
    Ao = A.conj().T if trans else A
    return check_entrywise(got, ext(Ao) @ ext(x), product_scale(Ao, x), A.shape[0] + (2 if cp else 0), cp, label)


def _check_lap5(got, N, u, label):
    ref, scale = lap5_longdouble(N, u)
    return check_entrywise(got, ref, scale, 7, False, label)


def _check_diag(got, d, x, trans, label):
    if not is_cplx(d.dtype):
        assert got.tobytes() == (d * x).tobytes(), label               # one multiplication per entry: one rounding
        return 0.0
    return check_complex_diag(got, d, x, trans, label)


def _gl_ops(c, n, nsub):
    A = lk.ginzburg_landau_linop_gpu(n, c, tau=0.01 * nsub, nsub=nsub)
    p = A.params
    return A, [ora.GLOp(n, p["dx"], p["tau"], nsub, p["nu"], p["gamma"], p["mu_c"], p["mu2"], adjoint=adj) for adj in (False, True)]


def _check_gl(got, oracle_op, x, label):
    ref = oracle_op.apply(x)
    err = float(np.abs(got - ref).max() / np.abs(ref).max())
    _report(label, err, GL_RTOL, "normwise vs oracle")
    assert err <= GL_RTOL, f"{label}: {err:.2e} > {GL_RTOL:.0e}"
    return err / GL_RTOL


# ---- (a) entry by entry ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", KINDS)
def test_dense_products_at_every_tiling_edge(kctx, dtype):
    """k_gemv_n + k_gemv_n_finish ('N') and k_gemv_h ('H') at n around the 8-column unroll (7, 8, 9), the 256-column chunks (1, 2, 3 and 5 of
    them), the 512-row (real) / 256-row (complex) block and an odd n; the host matrix with lda = 300 > n once; 'H' on A against 'N' on an
    operator made from A^H (other summation orders: the same bound, not the same bits)."""
    worst = 0.0
    for n in DENSE_N:
        A, x = dense_case(n, dtype)
        op, opH = _dense_op(kctx, A), _dense_op(kctx, np.asfortranarray(A.conj().T))
        yn, yh = _apply(op, False, x, kctx), _apply(op, True, x, kctx)
        worst = max(worst, _check_dense(yn, A, x, False, f"k_gemv_n n={n} {_name(dtype)}"),
                    _check_dense(yh, A, x, True, f"k_gemv_h n={n} {_name(dtype)}"),
                    _check_dense(_apply(opH, False, x, kctx), A, x, True, f"k_gemv_n on A^H n={n} {_name(dtype)}"),
                    _check_dense(_apply(opH, True, x, kctx), A, x, False, f"k_gemv_h on A^H n={n} {_name(dtype)}"))
        if n == 257:
            opl = _dense_op(kctx, A, lda=300)
            assert _apply(opl, False, x, kctx).tobytes() == yn.tobytes() and _apply(opl, True, x, kctx).tobytes() == yh.tobytes()
            del opl
        del op, opH
    print(f"dense {_name(dtype)}: worst ratio to the gamma bound {worst:.3f}")


def test_lap5_products_at_every_wave_and_segment_edge(kctx):
    """k_lap5: N = 1 .. 4 (no neighbour at all at 1 and 2), around the wave edge of the even path (128 points), around the 512-point segment
    (510 .. 514, 1026: two and three segments, lane 0 of a new segment loads u[c - 1] itself), odd N on the generic path; rmatvec = matvec bit
    for bit; a single 1.0 at i = 511 and i = 512 of line 1 of N = 1026 gives the stencil column itself."""
    worst = 0.0
    for N in LAP5_N:
        op = lk.laplacian2d_linop_gpu(N, kctx)
        u = lap5_input(N)
        v = _apply(op, False, u, kctx)
        worst = max(worst, _check_lap5(v, N, u, f"k_lap5 N={N}"))
        assert _apply(op, True, u, kctx).tobytes() == v.tobytes(), N
        if N == 1026:
            s = float((N + 1) ** 2)
            for i in (511, 512):
                got = _apply(op, False, lap5_input(N, f"unit{i}"), kctx)
                want = np.zeros(N * N)
                c = i + N
                want[c], want[c - 1], want[c + 1], want[c - N], want[c + N] = 4 * s, -s, -s, -s, -s
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, f"k_lap5 N={N}, 1.0 at point {i} of line 1: entries {bad[:8].tolist()} are not the stencil column's"
        del op
    print(f"lap5: worst ratio to the gamma bound {worst:.3f}")


@pytest.mark.parametrize("n,nsub", GL_CASES)
def test_ginzburg_landau_step_around_the_block_edge(kctx, n, nsub):
    """k_gl_stage at n = 3 and around the 256-thread block (255, 256, 257, 513), one and two RK4 steps, direct and adjoint, against the oracle
    at the tolerance of tests/test_gpu_parity.py::test_ginzburg_landau_stepper_against_oracle (whose sizes are not repeated here)."""
    A, oracles = _gl_ops(kctx, n, nsub)
    x = seeded(n, np.complex128, 13)
    for trans in (False, True):
        _check_gl(_apply(A, trans, x, kctx), oracles[trans], x, f"k_gl_stage n={n} nsub={nsub} {'H' if trans else 'N'}")


def _diag_big_n(c):
    """an odd size above 2 * num_cu * blas1_grid_mult * 256 16-byte lanes: every thread of the capped grid runs the two-element loop of
    k_diag_linspace, some its tail loop too, and the odd last element is on its own.  The compute-unit count is that of the context's
    device (tests/_gpu_helpers.py: device_num_cu)."""
    return 2 * (2 * device_num_cu(c) * BLAS1_GRID_MULT * 256 + 77) + 1


@pytest.mark.parametrize("dtype", KINDS)
def test_diagonal_operator_entry_by_entry(kctx, dtype):
    """k_diag: n = 1, 2, 3, 255, 257 and one size beyond the capped grid; the real kind bit for bit (one multiplication), the complex kind
    d x and conj(d) x per component within gamma(2) of the component's two products (check_complex_diag)."""
    worst = 0.0
    for n in DIAG_N + (_diag_big_n(kctx),):
        d, x = diag_case(n, dtype)
        op = lk.diag_linop_gpu(d, kctx)
        for trans in (False, True):
            worst = max(worst, _check_diag(_apply(op, trans, x, kctx), d, x, trans, f"k_diag n={n} {_name(dtype)} {'H' if trans else 'N'}"))
        del op
    print(f"diag {_name(dtype)}: worst ratio to the gamma bound {worst:.3f}")


def test_generated_diagonal_rounds_once_per_entry(kctx):
    """k_diag_linspace: d_i = fma(dstep, row0 + i, d0) is ONE rounding of the exact d0 + dstep (row0 + i), then one multiplication: bit for bit
    against the exact evaluation, row0 = 0, 1 and 10^9 + 1 (odd, with odd n), and beyond the capped grid where the two-element loop runs."""
    for n, row0s in [(m, LINSPACE_ROW0) for m in DIAG_N] + [(_diag_big_n(kctx), (1,))]:
        x = seeded(n, np.float64, 6201)
        for row0 in row0s:
            want = linspace_diag_exact(D0, DSTEP, row0, n) * x
            op = lk.diag_linop_gpu(n_local=n, row0=row0, d0=D0, dstep=DSTEP, ctx=kctx)
            for trans in (False, True):
                got = _apply(op, trans, x, kctx)
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, f"k_diag_linspace n={n} row0={row0}: {bad.size} entries differ, first {int(bad[0])}: {got[bad[0]]!r} != {want[bad[0]]!r}"
            del op


@pytest.mark.parametrize("dtype", KINDS)
def test_csr_stream_kernel_with_empty_rows(kctx, dtype):
    """k_csr_stream ("csr_stream" = 1, mean row length about 2): an empty first and last row, a run of 300 empty rows, a row of exactly 32
    entries, n = 1 (no entry at all), 257, 4099; A x and A^H x row by row against the longdouble row loop."""
    cp = is_cplx(dtype)
    worst = 0.0
    for n in CSR_STREAM_N:
        rowptr, colind, vals = csr_stream_case(n, dtype)
        assert rowptr[-1] == len(colind) == len(vals) and (n == 1 or colind.max() < n) and rowptr[-1] <= 32 * n
        op = lk.csr_linop_gpu((rowptr, colind, vals), kctx)
        x = seeded(n, dtype, 6301)
        for trans, mat in ((False, (rowptr, colind, vals)), (True, csr_conj_transpose(rowptr, colind, vals))):
            ref, scale, rl = csr_longdouble(*mat, x)
            worst = max(worst, check_entrywise(_apply(op, trans, x, kctx), ref, scale, rl + (2 if cp else 0), cp,
                                               f"k_csr_stream n={n} {_name(dtype)} {'H' if trans else 'N'}"))
        del op
    print(f"csr stream {_name(dtype)}: worst ratio to the gamma bound {worst:.3f}")


# ---- (b) nothing outside the n rows of y is written ----------------------------------------------------------------------------------------

def _operator_case(kind, size, dtype, c):
    """(operator, n, x, check(trans, got)) of one operator of (a)"""
    if kind == "dense":
        A, x = dense_case(size, dtype)
        return _dense_op(c, A), size, x, lambda t, got: _check_dense(got, A, x, t, f"caller panels: dense n={size} {_name(dtype)}")
    if kind == "lap5":
        u = lap5_input(size)
        return lk.laplacian2d_linop_gpu(size, c), size * size, u, lambda t, got: _check_lap5(got, size, u, f"caller panels: lap5 N={size}")
    if kind == "gl":
        A, oracles = _gl_ops(c, size, 2)
        x = seeded(size, np.complex128, 13)
        return A, size, x, lambda t, got: _check_gl(got, oracles[t], x, f"caller panels: gl n={size}")
    if kind == "diag":
        d, x = diag_case(size, dtype)
        return lk.diag_linop_gpu(d, c), size, x, lambda t, got: _check_diag(got, d, x, t, f"caller panels: diag n={size} {_name(dtype)}")
    if kind == "csr_stream":
        mat = csr_stream_case(size, dtype)
        mats = (mat, csr_conj_transpose(*mat))
        x = seeded(size, dtype, 6301)

        def check_csr(t, got):
            ref, scale, rl = csr_longdouble(*mats[t], x)
            return check_entrywise(got, ref, scale, rl + (2 if is_cplx(dtype) else 0), is_cplx(dtype), f"caller panels: csr stream n={size} {_name(dtype)}")
        return lk.csr_linop_gpu(mat, c), size, x, check_csr
    x = seeded(size, np.float64, 6201)
    want = linspace_diag_exact(D0, DSTEP, 10 ** 9 + 1, size) * x

    def check(t, got):
        assert got.tobytes() == want.tobytes(), f"caller panels: diag_linspace n={size}"
    return lk.diag_linop_gpu(n_local=size, row0=10 ** 9 + 1, d0=D0, dstep=DSTEP, ctx=c), size, x, check


PANEL_CASES = [("dense", 513, np.float64), ("dense", 512, np.float64), ("dense", 513, np.complex128), ("dense", 512, np.complex128),
               ("lap5", 127, np.float64), ("lap5", 128, np.float64), ("gl", 257, np.complex128), ("gl", 256, np.complex128),
               ("diag", 257, np.float64), ("diag", 257, np.complex128), ("diag_linspace", 257, np.float64),
               ("csr_stream", 257, np.float64), ("csr_stream", 257, np.complex128)]


@pytest.mark.parametrize("kind,size,dtype", PANEL_CASES, ids=[f"{k}-{s}-{np.dtype(d).name}" for k, s, d in PANEL_CASES])
def test_operators_write_only_their_rows_of_a_caller_panel(kctx, kind, size, dtype):
    """x = column 1 of a two-column panel, y = column 1 of a three-column panel, each wrapped in a buffer of its own with its own ld: NaN
    padding against live rows 48 bytes into the buffer, both ways round, and ld = n where the kind allows it (real: n even, complex: n odd).
    After y = op(A) x, 'N' and 'H': every word of y's buffer outside rows [0, n) of column 1 and every word of x's buffer is bit-identical,
    and y meets the bound of (a)."""
    op, n, x, check = _operator_case(kind, size, dtype, kctx)
    dt = np.dtype(x.dtype)
    pairs = [("nan_pad", 0, "off48", 2), ("off48", 2, "nan_pad", 0)]
    if (n % 2 == 1) == is_cplx(dt):
        pairs += [("unpadded", 0, "nan_pad", 0), ("nan_pad", 0, "unpadded", 0)]
    for lx, ex, ly, ey in pairs:
        Px = CallerPanel(kctx, dt, n, 2, lx, seed=1, extra_ld=ex)
        Py = CallerPanel(kctx, dt, n, 3, ly, seed=2, extra_ld=ey)
        assert Px.ld != Py.ld and Px.head + 2 * Px.ld <= Px.img.size and Py.head + 3 * Py.ld <= Py.img.size
        X0 = np.asfortranarray(np.stack([seeded(n, dt, 6600), x], axis=1))
        Y0 = np.asfortranarray(np.stack([seeded(n, dt, 6601 + j) for j in range(3)], axis=1))
        for trans in (False, True):
            Px.set(X0)
            Py.set(Y0)
            (op.apply_rmatvec if trans else op.apply_matvec)(Px.B[1], Py.B[1])
            what = f"{kind} {size} {'H' if trans else 'N'} x in {lx}, y in {ly}"
            got = Py.get(what)
            assert got[:, 0].tobytes() == Y0[:, 0].tobytes() and got[:, 2].tobytes() == Y0[:, 2].tobytes(), f"{what}: a neighbouring column of y changed"
            assert Px.get(what + " (x)").tobytes() == X0.tobytes(), f"{what}: x changed"
            check(trans, got[:, 1])


# ---- (c) the guard: a breakdown leaves the columns beyond it alone ---------------------------------------------------------------------------

@pytest.fixture(scope="module", params=[0, 1], ids=["three_sweeps", "single_launch"])
def gctx(request):
    c = lk.Context(device=0)
    c.set_tuning("resident", request.param)
    c.set_tuning("async_arnoldi", 1)
    yield c
    c.close()


def _engine_op(recipe, c):
    kind, arg = recipe
    if kind == "dense":
        return _dense_op(c, np.asfortranarray(arg))
    if kind == "csr":
        return lk.csr_linop_gpu(arg, c)
    return lk.laplacian2d_linop_gpu(arg, c)


def _marked_basis(c, n, dtype, x0, first_marker):
    """x0 in column 0, zeros up to the breakdown, a payload pattern (a counter stream, another per column) in every column from
    `first_marker` on"""
    m = BREAKDOWN_M
    X = lk.krylov_basis_gpu(n, m + 1, dtype, c)
    img = np.zeros((n, m + 1), dtype=dtype, order="F")
    if x0 is not None:
        img[:, 0] = x0
    for j in range(first_marker, m + 1):
        img[:, j] = seeded(n, dtype, 123 + j)
    X.upload(img)
    return X, img


def _markers_intact(X, img, first_marker, what):
    got = X.download(first_marker, X.ncols - first_marker)
    assert got.tobytes() == np.asfortranarray(img[:, first_marker:]).tobytes(), f"{what}: a column beyond the breakdown was written"


@pytest.mark.parametrize("dtype", KINDS)
def test_breakdown_on_each_operator_leaves_later_columns_alone(gctx, dtype):
    """lk_arnoldi (asynchronous batch) on the dense six-eigenvalue matrix, the same spectrum as a CSR diagonal (stream route) and as a CSR
    matrix of dense 40-entry rows (lanes route), and the stencil on three sine modes; lk_lanczos on the dense and the stencil case.  The
    operator launches enqueued beyond the breakdown would each write the next column: info and the projected matrix are the oracle's, and
    every marker column is bit-identical."""
    m = BREAKDOWN_M
    for name, (_Ao, recipe, n, x0, k, tol) in breakdown_cases(dtype).items():
        op = _engine_op(recipe, gctx)
        for which in ("arnoldi", "lanczos") if name in ("dense", "lap5") else ("arnoldi",):
            info_o, Ho, tol_o = oracle_breakdown(name, dtype, which)
            assert info_o == k and tol_o == tol
            X, img = _marked_basis(gctx, n, dtype, x0, k + 1)
            H = np.zeros((m + 1, m), dtype=dtype, order="F")
            info = (lk.arnoldi if which == "arnoldi" else lk.lanczos)(op, X, H, tol=tol)
            what = f"{which} breakdown {name} {_name(dtype)}"
            assert info == info_o, f"{what}: info = {info}, the oracle's {info_o}"
            assert_columns_close(H[:, :k], Ho[:, :k], what)
            assert not H[:, k:].any(), what
            _markers_intact(X, img, k + 1, what)
            del X
        del op


@pytest.mark.parametrize("dtype", KINDS)
def test_bidiagonalisation_breakdown_on_a_dense_operator_leaves_later_columns_alone(gctx, dtype):
    """lk_bidiag on the rank-two dense operator of tests/test_gpu_pipelines.py (n = 601): alpha_3 below tol stops it in the right half of
    step 3; k_gemv_h (V) and k_gemv_n (U) launches beyond it must not write: markers from column 3 of both bases."""
    info_o, Bo, R, u0, tol = oracle_bidiag_breakdown(dtype)
    m, n = BREAKDOWN_M, BIDIAG_N
    op = _dense_op(gctx, R)
    Ub, uimg = _marked_basis(gctx, n, dtype, u0, 3)
    Vb, vimg = _marked_basis(gctx, n, dtype, None, 3)
    B = np.zeros((m + 1, m), dtype=dtype, order="F")
    info = lk.bidiagonalization(op, Ub, Vb, B, tol=tol)
    what = f"bidiag breakdown {_name(dtype)}"
    assert info == info_o == 3, (info, info_o)
    assert_columns_close(B[:, :2], Bo[:, :2], what)
    assert abs(B[2, 2]) < tol and not B[3:, :].any() and not B[:, 3:].any()
    _markers_intact(Ub, uimg, 3, what + " U")
    _markers_intact(Vb, vimg, 3, what + " V")
