"""Two handles onto the same memory.  `krylov_basis_gpu.view(col0, ncols)` wraps columns of a panel in a handle of their own (lk_basis_wrap
at col(col0)), and the header tells C and Fortran callers to do the same; the engine must judge "is this the same memory?" by device
address, never by handle (include/lightkrylov_hip.h, "Model"; cols_overlap in lightkrylov_amd/csrc/lk_engine.hip).

1. Every entry twice (tests/_gpu_helpers.py: TwoRoutes): through ONE engine-owned panel with column indices, and through offset views of a
   wider parent, one handle per operand.  Same contents, same ld, same alignment, eager mode: the results must agree BIT FOR BIT -- host
   scalars, the projected matrices, and the whole downloaded parent, including the columns no call may write.  The parent route is checked
   against the oracle at the tolerance the entry's own test file uses, so the comparison does not rest on the engine alone.  (Most entries
   take X from column 0 of its handle and some take kdim from its column count, so the parent route's panel is one of exactly that
   width; TwoRoutes' docstring names every line of the engine that reads a handle's ncols or hwm: none chooses a kernel in eager mode.)
2. The lazy per-object path with every panel column reached through the parent or through one of three views, drawn at random.
3. Every refusal of the overlap rule provoked through views, and the legal neighbour: two panels living in each other's padding rows."""
import ctypes as C
import functools

import numpy as np
import pytest

import lightkrylov_amd as lk
from lightkrylov_amd import _capi
from lightkrylov_amd.constants import atol_dp
from oracle import oracle as ora
from tests import _pivot_ref as pref
from tests import test_gpu_kexpm as kx
from tests import test_gpu_kexpm_block as kb
from tests import test_gpu_lazy_fuzz as fuzz
from tests._gpu_helpers import KINDS, InterleavedPair, TwoRoutes, basis, bits, dptr, last_error, orthonormal_basis, seeded
from tests._tol import assert_close, assert_columns_close

pytestmark = pytest.mark.gpu

N = 4099                                            # odd, several blocks
INVALID = -1                                        # LK_ERR_INVALID
NORMALIZE = 1                                       # LK_DGS_NORMALIZE
_CTXS = {}


def tuned(**kw):
    key = tuple(sorted(kw.items()))
    if key not in _CTXS:
        c = lk.Context(device=0)
        for k, v in key:
            c.set_tuning(k, v)
        _CTXS[key] = c
    return _CTXS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in _CTXS.values():
        c.close()
    _CTXS.clear()


def _lib():
    return _capi.load()


def _sc(dtype, seed):
    r = np.random.default_rng(seed)
    return np.array([r.uniform(-2, 2), r.uniform(-2, 2) if np.dtype(dtype).kind == "c" else 0.0])


def _z(dtype, s):
    return complex(s[0], s[1]) if np.dtype(dtype).kind == "c" else float(s[0])


def _same(outs, what):
    """the host outputs of the two routes, bit for bit"""
    p, v = outs
    assert len(p) == len(v)
    for i, (a, b) in enumerate(zip(p, v)):
        assert np.array_equal(bits(np.atleast_1d(a)), bits(np.atleast_1d(b))), f"{what}: host output #{i} differs between the routes:\n{a}\n{b}"


def _scale_ok(got, ref, rtol, what):
    err = np.abs(np.asarray(got) - np.asarray(ref)).max()
    sc = max(float(np.abs(ref).max()), 1e-300)
    assert err <= rtol * sc, f"{what}: differs by {err / sc:.2e} (relative) > {rtol:.0e}"


# ---- 1. the two routes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", KINDS)
def test_blas1_through_views(ctx, dtype):
    """lk_vec_dot, norm, scal, axpby, copy with the operands in different views; oracle tolerances of test_blas1_on_caller_panels
    (tests/test_gpu_caller_memory.py): 1e-12 |x| |y| for the sums, 4e-15 for the elementwise results."""
    lib = _lib()
    X = basis(N, 6, dtype, 11)
    T = TwoRoutes(ctx, X)
    sa, sb = _sc(dtype, 1), _sc(dtype, 2)
    outs = []
    for h in T.routes():
        (hx, jx), (hy, jy), (hz, jz), (hw, jw) = h(0, 1), h(1, 1), h(2, 2), h(4, 2)
        d, d2, nr = np.zeros(2), np.zeros(2), np.zeros(1)
        _capi.check(lib.lk_vec_dot(hx, jx, hy, jy, dptr(d)))
        _capi.check(lib.lk_vec_norm(hy, jy, dptr(nr)))
        _capi.check(lib.lk_vec_scal(hx, jx, dptr(sa)))
        _capi.check(lib.lk_vec_axpby(dptr(sa), hz, jz + 1, dptr(sb), hy, jy))
        _capi.check(lib.lk_vec_copy(hw, jw + 1, hx, jx))
        _capi.check(lib.lk_vec_dot(hw, jw + 1, hz, jz, dptr(d2)))
        outs.append([d, nr, d2])
    got = T.check("blas1")
    _same(outs, "blas1")
    a, b = _z(dtype, sa), _z(dtype, sb)
    nx, ny = np.linalg.norm(X[:, 0]), np.linalg.norm(X[:, 1])
    assert abs(_z(dtype, outs[0][0]) - ora.dot(X[:, 0], X[:, 1])) <= 1e-12 * nx * ny
    assert abs(outs[0][1][0] - ora.norm(X[:, 1])) <= 1e-12 * ny
    ref = X.copy(order="F")
    ora.scal(ref[:, 0], a)
    ora.axpby(a, ref[:, 3], b, ref[:, 1])
    ref[:, 5] = ref[:, 0]
    for j in range(6):
        _scale_ok(got[:, j], ref[:, j], 4e-15, f"column {j}")
    assert abs(_z(dtype, outs[0][2]) - ora.dot(ref[:, 5], ref[:, 2])) <= 1e-12 * np.linalg.norm(ref[:, 5]) * np.linalg.norm(ref[:, 2])


@pytest.mark.parametrize("where", ["behind", "inside"])
@pytest.mark.parametrize("p", [2, 5])
@pytest.mark.parametrize("dtype", KINDS)
def test_innerprod_through_views(ctx, dtype, p, where):
    """lk_innerprod(X(:8), Y), Y behind X or INSIDE it (columns [2, 2 + p)): p = 2 on the vector units, p = 5 on the matrix cores.  Inside,
    entry (2 + q, q) is x^H x of one column: its imaginary part is exactly 0.0 on both routes (innerprod_impl's real_diagonal and the
    diagonal-block flags of dots_mfma, both decided by address).  Oracle: 1e-13 of the column norms, as test_innerprod_and_lincomb_on_caller_panels."""
    lib = _lib()
    k, j0 = 8, (8 if where == "behind" else 2)
    A = basis(N, k + 5, dtype, 31)
    T = TwoRoutes(ctx, A)
    outs = []
    for h in T.routes():
        (hx, _), (hy, jy) = h(0, k), h(j0, p)
        M = np.zeros((k, p), dtype=dtype, order="F")
        _capi.check(lib.lk_innerprod(hx, k, hy, jy, p, dptr(M)))
        outs.append([M])
    T.check("innerprod")
    for M, in outs:
        if where == "inside" and np.dtype(dtype).kind == "c":
            for q in range(p):
                assert M[j0 + q, q].imag == 0.0, f"x^H x of column {j0 + q} has imaginary part {M[j0 + q, q].imag!r}"
    _same(outs, f"innerprod p = {p} {where}")
    X, Y = A[:, :k], A[:, j0:j0 + p]
    scale = np.linalg.norm(X, axis=0).max() * np.linalg.norm(Y, axis=0).max()
    assert np.abs(outs[0][0] - ora.innerprod(X, Y).reshape(k, p, order="F")).max() <= 1e-13 * scale


@pytest.mark.parametrize("k", [5, 17])
@pytest.mark.parametrize("dtype", KINDS)
def test_gram_through_a_view(ctx, dtype, k):
    """lk_gram on the view [3, 3 + k); oracle: 1e-13 of the largest squared column norm (test_gram_on_caller_panels)"""
    lib = _lib()
    A = basis(N, k + 1, dtype, 51)
    T = TwoRoutes(ctx, A)
    outs = []
    for h in T.routes():
        hx, _ = h(0, k)
        G = np.zeros((k, k), dtype=dtype, order="F")
        _capi.check(lib.lk_gram(hx, k, dptr(G)))
        outs.append([G])
    T.check("gram")
    _same(outs, f"gram k = {k}")
    assert np.abs(outs[0][0] - ora.gram(A[:, :k])).max() <= 1e-13 * np.linalg.norm(A[:, :k], axis=0).max() ** 2


@pytest.mark.parametrize("q", [1, 2, 9])
@pytest.mark.parametrize("dtype", KINDS)
def test_lincomb_through_views(ctx, dtype, q):
    """lk_lincomb with X = view [1, 18) and Y the view behind it; oracle: 1e-14 |X| |c| (test_innerprod_and_lincomb_on_caller_panels)"""
    lib = _lib()
    k = 17
    A = basis(N, k + 9, dtype, 71)
    Cm = basis(k, q, dtype, 900 + q)
    T = TwoRoutes(ctx, A, a=1)
    for h in T.routes():
        (hx, _), (hy, jy) = h(0, k), h(k, q)
        _capi.check(lib.lk_lincomb(hx, k, dptr(Cm), q, hy, jy))
    got = T.check(f"lincomb q = {q}")
    assert np.array_equal(bits(got[:, :k]), bits(A[:, :k])) and np.array_equal(bits(got[:, k + q:]), bits(A[:, k + q:]))
    X = A[:, :k]
    for j in range(q):
        ref = ora.linear_combination(X, np.ascontiguousarray(Cm[:, j]))
        sc = (np.abs(X.real) + np.abs(X.imag)).max(axis=0) @ (np.abs(Cm[:, j].real) + np.abs(Cm[:, j].imag))
        assert np.abs(got[:, k + j] - ref).max() <= 1e-14 * sc, (q, j)


@pytest.mark.parametrize("resident", [1, 0])
@pytest.mark.parametrize("k", [3, 17])
@pytest.mark.parametrize("dtype", KINDS)
def test_dgs_through_views(dtype, k, resident):
    """lk_dgs with LK_DGS_NORMALIZE, y behind X in the same parent, as one launch and as three sweeps; oracle: 1e-12 (test_dgs_on_caller_panels)"""
    lib = _lib()
    c = tuned(resident=resident)
    Q, y = orthonormal_basis(N, k, dtype, 40 + k), seeded(N, dtype, 5000 + k)
    T = TwoRoutes(c, np.column_stack([Q, y, seeded(N, dtype, 6000 + k)]))
    before = c.resident_stats()
    outs = []
    for h in T.routes():
        (hx, _), (hy, jy) = h(0, k), h(k, 1)
        hh, norms, info = np.zeros(k, dtype=dtype), np.zeros(3), C.c_int(-7)
        _capi.check(lib.lk_dgs(hx, k, hy, jy, dptr(hh), dptr(norms), NORMALIZE, C.byref(info)))
        outs.append([hh, norms, np.array([info.value])])
    after = c.resident_stats()
    assert after[0] - before[0] == (2 if resident else 0), "the schedule under test did not run"
    got = T.check(f"dgs k = {k}")
    _same(outs, f"dgs k = {k} resident = {resident}")
    yo = y.copy()
    ho, _ = ora.double_gram_schmidt_step(yo, Q.copy(order="F"))
    _scale_ok(outs[0][0], ho, 1e-12, "beta")
    _scale_ok(got[:, k], yo / np.linalg.norm(yo), 1e-12, "y'' / |y''|")
    assert abs(outs[0][1][2] - np.linalg.norm(yo)) <= 1e-12 * np.linalg.norm(y)
    assert np.array_equal(bits(got[:, :k]), bits(Q))


@pytest.mark.parametrize("p", [2, 5])
@pytest.mark.parametrize("dtype", KINDS)
def test_dgs_block_through_views(ctx, dtype, p):
    """lk_dgs_block on the vector units (p = 2) and the matrix cores (p = 5); oracle: 1e-12 per column (test_dgs_block_on_caller_panels)"""
    lib = _lib()
    k = 17
    Q, Y = orthonormal_basis(N, k, dtype, 60 + k), basis(N, p, dtype, 700 + p)
    T = TwoRoutes(ctx, np.column_stack([Q, Y]))
    outs = []
    for h in T.routes():
        (hx, _), (hy, jy) = h(0, k), h(k, p)
        hh, info = np.zeros((k, p), dtype=dtype, order="F"), C.c_int(-7)
        _capi.check(lib.lk_dgs_block(hx, k, hy, jy, p, dptr(hh), C.byref(info)))
        outs.append([hh, np.array([info.value])])
    got = T.check(f"dgs_block p = {p}")
    _same(outs, f"dgs_block p = {p}")
    Yo = Y.copy(order="F")
    ho, _ = ora.double_gram_schmidt_step_block(Yo, Q.copy(order="F"))
    assert_columns_close(outs[0][0], ho, f"dgs_block through views p = {p}: beta")
    for j in range(p):
        _scale_ok(got[:, k + j], Yo[:, j], 1e-12, f"column {j}")


@pytest.mark.parametrize("dtype", KINDS)
def test_qr_through_a_view(ctx, dtype):
    """lk_qr of columns [2, 7): j0 = 2 on the parent against a view of exactly those columns; oracle: 1e-12 (test_factorisations_on_a_caller_basis)"""
    lib = _lib()
    p = 5
    A = basis(N, p + 3, dtype, 300)
    T = TwoRoutes(ctx, A)
    outs = []
    for h in T.routes():
        hq, j0 = h(2, p)
        R, info = np.zeros((p, p), dtype=dtype, order="F"), C.c_int(-7)
        _capi.check(lib.lk_qr(hq, j0, p, dptr(R), p, atol_dp, C.byref(info)))
        outs.append([R, np.array([info.value])])
    got = T.check("qr")
    _same(outs, "qr")
    Mo, Ro = A[:, 2:2 + p].copy(order="F"), np.zeros((p, p), dtype=dtype, order="F")
    assert ora.qr_no_pivoting(Mo, Ro) == 0 and outs[0][1][0] == 0
    assert_columns_close(outs[0][0], Ro, "qr through a view")
    _scale_ok(got[:, 2:2 + p], Mo, 1e-12, "Q")


@functools.lru_cache(maxsize=2)
def _dense(dtype):
    """a dense N x N operator, 2 I + a random matrix of norm about 2 (made once per kind)"""
    r = np.random.default_rng(5)
    A = r.standard_normal((N, N)) / np.sqrt(N)
    if np.dtype(dtype).kind == "c":
        A = A + 1j * r.standard_normal((N, N)) / np.sqrt(N)
    A[np.diag_indices(N)] += 2.0
    return np.asfortranarray(A.astype(dtype))


def _diag(dtype, hermitian=False):
    g = np.arange(N) / N
    return ((1.0 + g) * (np.exp(0.4j * g) if np.dtype(dtype).kind == "c" and not hermitian else 1.0)).astype(dtype)


def _start(n, dtype, seed):
    x = seeded(n, dtype, seed)
    return x / np.linalg.norm(x)


def _first(n, w, dtype, seed):
    X = np.zeros((n, w), dtype=dtype, order="F")
    X[:, 0] = _start(n, dtype, seed)
    return X


M_STEPS = 6


@pytest.mark.parametrize("dtype", KINDS)
def test_arnoldi_through_a_view(ctx, dtype):
    """lk_arnoldi on a dense operator, X = view [3, 3 + m + 1) of a wider parent, m = 6; oracle: 1e-12 per column of H
    (test_factorisations_on_a_caller_basis)"""
    lib, m = _lib(), M_STEPS
    Am = _dense(dtype)
    A, Ao = lk.dense_linop_gpu(Am, ctx), ora.DenseOp(Am)
    X0 = _first(N, m + 1, dtype, 7)
    T = TwoRoutes(ctx, X0)
    outs = []
    for h in T.routes():
        hx, _ = h(0, m + 1)
        H, info = np.zeros((m + 1, m), dtype=dtype, order="F"), C.c_int(-7)
        _capi.check(lib.lk_arnoldi(A._h, hx, dptr(H), m + 1, 1, m, atol_dp, 0, C.byref(info)))
        outs.append([H, np.array([info.value])])
    T.check("arnoldi")
    _same(outs, "arnoldi")
    Xo, Ho = X0.copy(order="F"), np.zeros((m + 1, m), dtype=dtype, order="F")
    assert ora.arnoldi(Ao, Xo, Ho) == 0 and outs[0][1][0] == 0
    assert_columns_close(outs[0][0], Ho, "arnoldi through a view")
    A.close()


@pytest.mark.parametrize("dtype", KINDS)
def test_lanczos_through_a_view(ctx, dtype):
    """lk_lanczos on a Hermitian (real diagonal) operator, X = view [3, 3 + m + 1); oracle: 1e-12 per column of T"""
    lib, m = _lib(), M_STEPS
    d = _diag(dtype, hermitian=True)
    A, Ao = lk.diag_linop_gpu(d, ctx), ora.DiagOp(d)
    X0 = _first(N, m + 1, dtype, 8)
    T = TwoRoutes(ctx, X0)
    outs = []
    for h in T.routes():
        hx, _ = h(0, m + 1)
        Tm, info = np.zeros((m + 1, m), dtype=dtype, order="F"), C.c_int(-7)
        _capi.check(lib.lk_lanczos(A._h, hx, dptr(Tm), m + 1, 1, m, atol_dp, C.byref(info)))
        outs.append([Tm, np.array([info.value])])
    T.check("lanczos")
    _same(outs, "lanczos")
    Xo, To = X0.copy(order="F"), np.zeros((m + 1, m), dtype=dtype, order="F")
    assert ora.lanczos(Ao, Xo, To) == 0 and outs[0][1][0] == 0
    assert_columns_close(outs[0][0], To, "lanczos through a view")


@pytest.mark.parametrize("dtype", KINDS)
def test_bidiag_on_two_views_of_one_parent(ctx, dtype):
    """lk_bidiag with U = view [3, 3 + m + 1) and V = view [3 + m + 1, 3 + 2 m + 1) of ONE parent (route P: two panels, kdim comes from
    U's column count); oracle: 1e-12 per column of B"""
    lib, m = _lib(), M_STEPS
    d = _diag(dtype)
    A, Ao, Aho = lk.diag_linop_gpu(d, ctx), ora.DiagOp(d), ora.DiagOp(d.conj())
    UV = _first(N, 2 * m + 1, dtype, 9)
    T = TwoRoutes(ctx, UV, split=m + 1)
    outs = []
    for h in T.routes():
        (hu, _), (hv, _) = h(0, m + 1), h(m + 1, m)
        Bm, info = np.zeros((m + 1, m), dtype=dtype, order="F"), C.c_int(-7)
        _capi.check(lib.lk_bidiag(A._h, hu, hv, dptr(Bm), m + 1, 1, m, atol_dp, C.byref(info)))
        outs.append([Bm, np.array([info.value])])
    T.check("bidiag")
    _same(outs, "bidiag")
    Uo, Vo, Bo = UV[:, :m + 1].copy(order="F"), np.zeros((N, m), dtype=dtype, order="F"), np.zeros((m + 1, m), dtype=dtype, order="F")
    assert ora.bidiagonalization(Ao, Aho, Uo, Vo, Bo) == 0
    assert_columns_close(outs[0][0], Bo, "bidiag through views")


@pytest.mark.parametrize("dtype", KINDS)
def test_arnoldi_block_through_a_view(ctx, dtype):
    """lk_arnoldi_block, p = 2, kdim = 3, X = view [3, 3 + 8); oracle: 1e-12 per column of H (test_factorisations_on_a_caller_basis)"""
    lib, p, kdim = _lib(), 2, 3
    ncol = (kdim + 1) * p
    d = _diag(dtype)
    A, Ao = lk.diag_linop_gpu(d, ctx), ora.DiagOp(d)
    X0 = np.zeros((N, ncol), dtype=dtype, order="F")
    X0[:, :p] = orthonormal_basis(N, p, dtype, 70 + p)
    T = TwoRoutes(ctx, X0)
    outs = []
    for h in T.routes():
        hx, _ = h(0, ncol)
        H, info = np.zeros((ncol, kdim * p), dtype=dtype, order="F"), C.c_int(-7)
        _capi.check(lib.lk_arnoldi_block(A._h, hx, dptr(H), ncol, p, 1, kdim, atol_dp, 0, C.byref(info)))
        outs.append([H, np.array([info.value])])
    T.check("arnoldi_block")
    _same(outs, "arnoldi_block")
    Xo, Ho = X0.copy(order="F"), np.zeros((ncol, kdim * p), dtype=dtype, order="F")
    assert ora.arnoldi_block(Ao, Xo, Ho, p) == 0 and outs[0][1][0] == 0
    assert_columns_close(outs[0][0], Ho, "arnoldi_block through a view")


@pytest.mark.parametrize("dtype", KINDS)
def test_qr_pivot_through_a_view(ctx, dtype):
    """lk_qr_pivot of columns [2, 7): j0 = 2 on the parent against a view of those columns, graded columns so that the pivots move;
    yardstick: tests/_pivot_ref.py, same perm and info, 1e-12 per column of R (tests/test_gpu_pivot_qr.py)"""
    lib, p = _lib(), 5
    A = basis(N, p + 3, dtype, 300)
    A[:, 2:2 + p] *= 2.0 ** (-np.random.default_rng(3).permutation(p).astype(float))
    T = TwoRoutes(ctx, A)
    outs = []
    for h in T.routes():
        hq, j0 = h(2, p)
        R, perm, info = np.zeros((p, p), dtype=dtype, order="F"), np.zeros(p, dtype=np.intc), C.c_int(-7)
        _capi.check(lib.lk_qr_pivot(hq, j0, p, dptr(R), p, perm.ctypes.data_as(C.POINTER(C.c_int)), atol_dp, C.byref(info)))
        outs.append([R, perm.astype(np.float64), np.array([info.value])])
    got = T.check("qr_pivot")
    _same(outs, "qr_pivot")
    Qr, Rr, permr = A[:, 2:2 + p].copy(order="F"), np.zeros((p, p), dtype=dtype, order="F"), np.zeros(p, dtype=int)
    gaps = []
    infor = pref.qr_with_pivoting(Qr, Rr, permr, pref.ATOL_DP, pref.engine_stream(2), gaps)
    assert min(gaps) > 1e-6 and not np.array_equal(permr, np.arange(1, p + 1)), (gaps, permr)
    assert outs[0][2][0] == infor and np.array_equal(outs[0][1], permr)
    assert_columns_close(outs[0][0], Rr, "qr_pivot through a view")
    assert np.abs(got[:, 2:2 + p] - Qr).max() <= 1e-12


KDIM = 6


@pytest.mark.parametrize("dtype", KINDS)
def test_kexpm_through_views(ctx, dtype):
    """lk_kexpm with the workspace the view [3, 3 + kdim + 1) and b, c the two columns behind it in the same parent (route P: the
    workspace is a panel of its own, c may not be a column of the workspace's handle); kdim = 6.  Yardstick as in tests/test_gpu_kexpm.py:
    the host loop on a user operator, same info, 1e-12 |b|."""
    lib = _lib()
    g = np.arange(N) / N
    d = ((-0.05 - 2.0 * g) * (np.exp(0.4j * g) if np.dtype(dtype).kind == "c" else 1.0)).astype(dtype)
    A, tau, w = lk.diag_linop_gpu(d, ctx), 0.02, KDIM + 1
    Z = np.zeros((N, w + 2), dtype=dtype, order="F")
    Z[:, w] = seeded(N, dtype, 11)
    T = TwoRoutes(ctx, Z, split=w)
    outs = []
    for h in T.routes():
        (hx, _), (hb, jb), (hc, jc) = h(0, w), h(w, 1), h(w + 1, 1)
        info, err = C.c_int(-7), C.c_double()
        _capi.check(lib.lk_kexpm(A._h, 0, hb, jb, hc, jc, hx, tau, kx.TOL, KDIM, C.byref(info), C.byref(err)))
        outs.append([np.array([info.value, err.value])])
    got = T.check("kexpm")
    _same(outs, "kexpm")
    b = lk.dense_vector_gpu.from_array(Z[:, w], ctx)
    chost = lk.dense_vector_gpu(N, dtype, ctx)
    info_h = lk.kexpm(chost, kx._user_op(A), b, tau, kx.TOL, kdim=KDIM)
    assert outs[0][0][0] == info_h and 0 < info_h <= KDIM + 1, (outs[0][0], info_h)
    assert np.linalg.norm(got[:, w + 1] - chost.to_array()) <= 1e-12 * np.linalg.norm(Z[:, w])
    assert np.array_equal(bits(got[:, w]), bits(Z[:, w]))


@pytest.mark.parametrize("dtype", KINDS)
def test_kexpm_block_through_views(ctx, dtype):
    """lk_kexpm_block, p = 2, nk = 6: workspace the view [3, 3 + 14), B and C the views behind it.  Yardstick: tests/_pivot_ref.kexpm_mat,
    same info, err_est within 1e-10 relative, 1e-12 per column of C, tol placed in a gap of the estimates (tests/test_gpu_kexpm_block.py)."""
    lib, p, nk = _lib(), 2, KDIM
    d = _diag(dtype)
    A, Ao, tau, w = lk.diag_linop_gpu(d, ctx), ora.DiagOp(d), 0.05, p * (nk + 1)
    Bh = basis(N, p, dtype, 21)
    Z = np.zeros((N, w + 2 * p), dtype=dtype, order="F")
    Z[:, w:w + p] = Bh
    hist = []
    pref.kexpm_mat(Ao, Bh, tau, 0.0, nk, history=hist)
    tol = kb._tol_between(hist)
    Cr, info_r, err_r, _ = pref.kexpm_mat(Ao, Bh, tau, tol, nk)
    T = TwoRoutes(ctx, Z, split=w)
    outs = []
    for h in T.routes():
        (hx, _), (hb, jb), (hc, jc) = h(0, w), h(w, p), h(w + p, p)
        info, err = C.c_int(-7), C.c_double()
        _capi.check(lib.lk_kexpm_block(A._h, 0, hb, jb, hc, jc, p, hx, tau, tol, nk, C.byref(info), C.byref(err)))
        outs.append([np.array([info.value, err.value])])
    got = T.check("kexpm_block")
    _same(outs, "kexpm_block")
    assert outs[0][0][0] == info_r and abs(outs[0][0][1] - err_r) <= max(1e-10 * err_r, 1e-14), (outs[0][0], info_r, err_r)
    assert_columns_close(got[:, w + p:], Cr, "kexpm_block through views")
    assert np.array_equal(bits(got[:, w:w + p]), bits(Bh))


@pytest.mark.parametrize("precond", [False, True])
@pytest.mark.parametrize("dtype", KINDS)
def test_gmres_through_views(ctx, dtype, precond):
    """lk_gmres, kdim = 6, workspace the view [3, 3 + ncw), b and x the columns behind it in the same parent; with and without a diagonal
    right preconditioner M.  Oracle: ora.gmres (on x -> A (M x) with M, the solution is M u), history and x at 1e-12
    (tests/test_gpu_gmres_engine.py)."""
    lib = _lib()
    d = _diag(dtype, hermitian=not precond) * (1.0 + 3.0 * (np.arange(N) % 7))      # (without M: a real spectrum, the complex kind's history stays bounded)
    mdiag = (1.0 / (1.0 + 3.0 * (np.arange(N) % 7) + 0.3 * np.cos(np.arange(N)))).astype(dtype)
    A = lk.diag_linop_gpu(d, ctx)
    M = lk.diag_linop_gpu(mdiag, ctx) if precond else None
    w, cap = KDIM + 1 + (1 if precond else 0), 64
    Z = np.zeros((N, w + 2), dtype=dtype, order="F")
    Z[:, w] = seeded(N, dtype, 31)
    T = TwoRoutes(ctx, Z)
    outs = []
    for h in T.routes():
        (hv, _), (hb, jb), (hx, jx) = h(0, w), h(w, 1), h(w + 1, 1)
        res, nres, ni, no, info = np.zeros(cap), C.c_int64(), C.c_int(), C.c_int(), C.c_int(-7)
        _capi.check(lib.lk_gmres(A._h, 0, M._h if M else None, hb, jb, hx, jx, hv, 1e-10, 0.0, KDIM, 4, dptr(res), cap, C.byref(nres),
                                 C.byref(ni), C.byref(no), C.byref(info)))
        outs.append([res, np.array([nres.value, ni.value, no.value, info.value])])
    got = T.check("gmres")
    _same(outs, f"gmres precond = {precond}")
    u = np.zeros(N, dtype=dtype)
    Ao = ora.PyOp(lambda v: d * (mdiag * v), dtype) if precond else ora.DiagOp(d)
    info_o, res_o = ora.gmres(Ao, Z[:, w].copy(), u, rtol=1e-10, atol=0.0, kdim=KDIM, maxiter=4)
    nres = int(outs[0][1][0])
    assert outs[0][1][3] == info_o and nres == len(res_o), (outs[0][1], info_o, len(res_o))
    assert_close(outs[0][0][:nres], res_o, "gmres through views [history]", scale=res_o[0])
    assert_close(got[:, w + 1], mdiag * u if precond else u, "gmres through views [x]")
    assert np.array_equal(bits(got[:, w]), bits(Z[:, w]))


# ---- 2. the lazy path through mixed handles -----------------------------------------------------------------------------------------------
VIEWS = ((1, fuzz.NV - 1), (3, 6), (5, 7))            # three fixed offset views of the fuzz panel: every column but the first is in one


@pytest.mark.parametrize("dtype", KINDS)
def test_lazy_context_equals_an_eager_one_through_mixed_handles(dtype):
    """tests/test_gpu_lazy_fuzz.py's sequences, each panel column named through the parent or through one of three offset views (drawn from
    a generator of its own: the calls are the same as without views).  Eager and lazy must agree as there, 1e-12 of the scale, over the
    same 24 seeds; at least a third of the vector operands of every seed go through a view, and the fused sweeps and virtual temporaries
    stay above that test's floors (fused > 50, virtual > 20): the views have not switched the path under test off."""
    fused = virtual = 0
    for seed in range(24):
        oe, fe, se = fuzz._run(seed, dtype, lazy=False, views=VIEWS)
        ol, fl, st = fuzz._run(seed, dtype, lazy=True, views=VIEWS)
        assert se[-2:] == st[-2:] and 3 * st[-1] >= st[-2], f"seed {seed}: {st[-1]} of {st[-2]} vector operands went through a view"
        assert len(oe) == len(ol)
        scale = max(1.0, max((abs(v) for v in oe), default=1.0))
        for i, (a, b) in enumerate(zip(oe, ol)):
            assert abs(a - b) <= 1e-12 * scale, f"seed {seed}: scalar #{i}: eager {a}, lazy {b}"
        for a, b in zip(fe, fl):
            assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(a).max()), f"seed {seed}: final vectors differ"
        fused += st[0]
        virtual += st[2]
    print(f"mixed handles, {np.dtype(dtype).name}: fused = {fused}, virtual = {virtual}")
    assert fused > 50 and virtual > 20


# ---- 3. refusals, and the legal neighbour -------------------------------------------------------------------------------------------------
def _shifted(ctx, P, col, ncols=1, rows=2):
    """`ncols` columns wrapped `rows` rows into column `col` of P: 16-byte aligned for either kind, each overlaps a column of P partially"""
    dt, n, _nc, ld, ptr = P.info()
    h = C.c_void_p()
    _capi.check(_lib().lk_basis_wrap(ctx._h, dt, n, ncols, ld, C.c_void_p(ptr + (col * ld + rows) * P.dtype.itemsize), C.byref(h)))
    return lk.krylov_basis_gpu(n, ncols, P.dtype, ctx, _handle=h, _owner=P)


def _refusals(ctx, P, A, dtype, k, m):
    """(entry name in lk_last_error, call) for every refusal of the rule; P holds k + 12 columns"""
    lib = _lib()
    one, h, M = np.array([1.0, 0.0]), np.zeros(64, dtype=dtype), np.zeros((m + 1, m), dtype=dtype, order="F")
    info, n64, ni = C.c_int(), C.c_int64(), C.c_int()
    X, Yin, Yedge = P.view(1, k), P.view(3, 2), P.view(k, 3)          # Yin inside X, Yedge: its first column is X's last
    s3, sk = _shifted(ctx, P, 3), _shifted(ctx, P, m + 1, ncols=m)     # sk: m columns, the first two rows into U's last
    U, V = P.view(1, m + 1), P.view(m + 1, m)                           # V's first column is U's last
    W = P.view(2, m + 2)                                                # a workspace: kdim = m writes [2, 2 + m + 1)
    Wb = P.view(2, 6)                                                   # block workspace: p = 2, nk = 2 writes all of [2, 8)
    Cfar, s6, sfar = P.view(12, 2), _shifted(ctx, P, 6, ncols=2), _shifted(ctx, P, 13, ncols=2)   # s6: two rows into the workspace; sfar: into Cfar
    Cm = np.zeros((k, 3), dtype=dtype, order="F")
    return [
        ("lk_lincomb", lambda: lib.lk_lincomb(X._h, k, dptr(Cm), 2, Yin._h, 0)),
        ("lk_lincomb", lambda: lib.lk_lincomb(X._h, k, dptr(Cm), 3, Yedge._h, 0)),
        ("lk_lincomb", lambda: lib.lk_lincomb(X._h, k, dptr(Cm), 1, s3._h, 0)),
        ("lk_dgs_block", lambda: lib.lk_dgs_block(X._h, k, Yin._h, 0, 2, dptr(h), C.byref(info))),
        ("lk_dgs_block", lambda: lib.lk_dgs_block(X._h, k, Yedge._h, 0, 3, dptr(h), C.byref(info))),
        ("lk_dgs_block", lambda: lib.lk_dgs_block(X._h, k, s3._h, 0, 1, dptr(h), C.byref(info))),
        ("double_gram_schmidt_step", lambda: lib.lk_dgs(X._h, k, Yin._h, 1, dptr(h), None, 0, C.byref(info))),
        ("double_gram_schmidt_step", lambda: lib.lk_dgs(X._h, k, s3._h, 0, dptr(h), None, 0, C.byref(info))),
        ("double_gram_schmidt_step", lambda: lib.lk_orthogonalize(X._h, k, Yedge._h, 0, dptr(h), C.byref(info))),
        ("double_gram_schmidt_step", lambda: lib.lk_orthogonalize(X._h, k, s3._h, 0, dptr(h), C.byref(info))),
        ("lk_kexpm_block", lambda: lib.lk_kexpm_block(A._h, 0, Yin._h, 0, Cfar._h, 0, 2, Wb._h, 0.1, 1e-10, 2, C.byref(info), None)),
        ("lk_kexpm_block", lambda: lib.lk_kexpm_block(A._h, 0, Cfar._h, 0, s6._h, 0, 2, Wb._h, 0.1, 1e-10, 2, C.byref(info), None)),
        ("lk_kexpm_block", lambda: lib.lk_kexpm_block(A._h, 0, Cfar._h, 0, sfar._h, 0, 2, Wb._h, 0.1, 1e-10, 2, C.byref(info), None)),
        ("lk_bidiag", lambda: lib.lk_bidiag(A._h, U._h, V._h, dptr(M), m + 1, 1, m, atol_dp, C.byref(info))),
        ("lk_bidiag", lambda: lib.lk_bidiag(A._h, U._h, sk._h, dptr(M), m + 1, 1, m, atol_dp, C.byref(info))),
        ("lk_linop_apply", lambda: lib.lk_linop_apply(A._h, 0, P._h, 3, s3._h, 0)),
        ("lk_linop_apply", lambda: lib.lk_linop_apply(A._h, 0, Yin._h, 0, P._h, 3)),
        ("lk_linop_residual", lambda: lib.lk_linop_residual(A._h, 0, P._h, 0, P._h, 3, s3._h, 0, None)),
        ("lk_linop_residual", lambda: lib.lk_linop_residual(A._h, 0, P._h, 3, P._h, 0, s3._h, 0, None)),
        ("lk_vec_copy", lambda: lib.lk_vec_copy(s3._h, 0, P._h, 3)),
        ("lk_vec_axpby", lambda: lib.lk_vec_axpby(dptr(one), P._h, 3, dptr(one), s3._h, 0)),
        ("lk_kexpm", lambda: lib.lk_kexpm(A._h, 0, Yin._h, 0, P._h, 0, W._h, 0.1, 1e-10, m, C.byref(info), None)),
        ("lk_kexpm", lambda: lib.lk_kexpm(A._h, 0, P._h, 0, s3._h, 0, W._h, 0.1, 1e-10, m, C.byref(info), None)),
        ("lk_gmres", lambda: lib.lk_gmres(A._h, 0, None, Yin._h, 0, P._h, 0, W._h, 1e-10, 1e-12, m, 1, None, 0, C.byref(n64), C.byref(ni),
                                          C.byref(ni), C.byref(info))),
        ("lk_gmres", lambda: lib.lk_gmres(A._h, 0, None, P._h, 0, s3._h, 0, W._h, 1e-10, 1e-12, m, 1, None, 0, C.byref(n64), C.byref(ni),
                                          C.byref(ni), C.byref(info))),
    ], (X, Yin, Yedge, s3, sk, U, V, W, Wb, Cfar, s6, sfar)


def _legal_call(ctx, A, dtype, n, k):
    """one legal call on `ctx`: a Gram-Schmidt step; returns (h, y'')"""
    Q, y = orthonormal_basis(n, k, dtype, 40 + k), seeded(n, dtype, 5000 + k)
    B = lk.krylov_basis_gpu(n, k + 1, dtype, ctx)
    B.upload(np.column_stack([Q, y]))
    h, info = np.zeros(k, dtype=dtype), C.c_int()
    _capi.check(_lib().lk_dgs(B._h, k, B._h, k, dptr(h), None, 0, C.byref(info)))
    return h, B.download()


@pytest.mark.parametrize("dtype", KINDS)
def test_overlap_through_views_is_refused(dtype):
    """Every refusal of the rule, provoked through views: the handles differ, the memory overlaps -- a whole column, the edge column of a
    range, or a column wrapped two rows into another (partial overlap).  LK_ERR_INVALID, lk_last_error names the entry, the parent is
    bit-identical afterwards, and the next legal call on the context gives what it gives on a fresh context."""
    n, k, m = 37, 6, 4
    c, fresh = lk.Context(device=0), lk.Context(device=0)
    try:
        d = (1.0 + np.arange(n) / n).astype(dtype)
        A = lk.diag_linop_gpu(d, c)
        img = basis(n, k + 12, dtype, 17)
        P = lk.krylov_basis_gpu(n, k + 12, dtype, c)
        P.upload(img)
        calls, keep = _refusals(c, P, A, dtype, k, m)
        want = _legal_call(fresh, None, dtype, n, k)
        for i, (name, call) in enumerate(calls):
            rc = call()
            assert rc == INVALID, f"refusal #{i} ({name}): returned {rc}"
            assert name in last_error(), f"refusal #{i}: lk_last_error() = {last_error()!r} does not name {name}"
            assert np.array_equal(bits(P.download()), bits(img)), f"refusal #{i} ({name}): the panel changed"
            got = _legal_call(c, None, dtype, n, k)
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, want)), f"after refusal #{i} ({name}): the next legal call differs"
        # the exact same column through two handles stays legal: a no-op copy, the in-place update
        one, two = np.array([1.0, 0.0]), np.array([2.0, 0.0])
        V3 = P.view(3, 1)
        assert _lib().lk_vec_copy(V3._h, 0, P._h, 3) == 0
        assert np.array_equal(bits(P.download()), bits(img))
        assert _lib().lk_vec_axpby(dptr(one), P._h, 3, dptr(two), V3._h, 0) == 0
        ref = img.copy(order="F")
        ref[:, 3] = 3.0 * ref[:, 3]
        assert np.abs(P.download() - ref).max() <= 4e-15 * np.abs(ref).max()
        del keep, calls, V3
    finally:
        c.close()
        fresh.close()


@pytest.mark.parametrize("dtype", KINDS)
def test_panels_in_each_others_padding_are_accepted(ctx, dtype):
    """One flat buffer, ld = 2 n_pad: panel A in rows [0, n) of every column, panel B n_pad rows further on -- each lives in the other's
    padding rows, which "are never read or written" and belong to nobody.  lk_dgs, lk_lincomb, lk_dgs_block, lk_bidiag, lk_kexpm and
    lk_gmres take the pair, with the bits the same calls give on two separate buffers of the same ld and alignment, and every word outside
    the two panels unchanged."""
    lib = _lib()
    n, k, m = 4099, 9, 6
    d = (1.0 + np.arange(n) / n).astype(dtype)
    A = lk.diag_linop_gpu(d, ctx)
    res = []
    for together in (True, False):
        out = []
        # Gram-Schmidt: X = A(:k), y = a column of B; then A -> B by lk_lincomb, then the block step
        Pr = InterleavedPair(ctx, dtype, n, k, together)
        Pr.set(0, orthonormal_basis(n, k, dtype, 40 + k))
        Pr.set(1, basis(n, k, dtype, 700))
        h, info = np.zeros(k, dtype=dtype), C.c_int()
        _capi.check(lib.lk_dgs(Pr.A._h, k, Pr.B._h, 1, dptr(h), None, 0, C.byref(info)))
        out += [h] + Pr.get("dgs")
        Cm = basis(k, 3, dtype, 900)
        _capi.check(lib.lk_lincomb(Pr.A._h, k, dptr(Cm), 3, Pr.B._h, 2))
        out += Pr.get("lincomb")
        hb = np.zeros((k, 5), dtype=dtype, order="F")
        _capi.check(lib.lk_dgs_block(Pr.A._h, k, Pr.B._h, 4, 5, dptr(hb), C.byref(info)))
        out += [hb] + Pr.get("dgs_block")
        # Golub-Kahan with U = A (m + 1 columns), V = B; kexpm and gmres with the workspace in A and the vectors in B
        Pr = InterleavedPair(ctx, dtype, n, m + 1, together)
        Z = np.zeros((n, m + 1), dtype=dtype, order="F")
        Z[:, 0] = _start(n, dtype, 9)
        Pr.set(0, Z)
        Pr.set(1, np.zeros((n, m + 1), dtype=dtype))
        Bm = np.zeros((m + 1, m), dtype=dtype, order="F")
        _capi.check(lib.lk_bidiag(A._h, Pr.A._h, Pr.B._h, dptr(Bm), m + 1, 1, m, atol_dp, C.byref(info)))
        out += [Bm] + Pr.get("bidiag")
        Pr.set(1, basis(n, m + 1, dtype, 800))
        err = C.c_double()
        _capi.check(lib.lk_kexpm(A._h, 0, Pr.B._h, 0, Pr.B._h, 1, Pr.A._h, 0.1, 1e-10, m, C.byref(info), C.byref(err)))
        out += [np.array([info.value, err.value])] + Pr.get("kexpm")
        n64, ni, no = C.c_int64(), C.c_int(), C.c_int()
        _capi.check(lib.lk_gmres(A._h, 0, None, Pr.B._h, 2, Pr.B._h, 3, Pr.A._h, 1e-10, 1e-12, m, 3, None, 0, C.byref(n64), C.byref(ni),
                                 C.byref(no), C.byref(info)))
        out += [np.array([info.value, ni.value, no.value])] + Pr.get("gmres")
        res.append(out)
    _same(res, "interleaved panels against two buffers")
