"""Kernels on caller-owned panels (lk_basis_wrap, include/lightkrylov_hip.h: a 16-byte aligned pointer, any ld >= n_local -- even for the real
kind --, "rows [n_local, ld) are never read or written").  Panels made by lk_basis_create start every column on a 256-byte boundary, round ld up
to 32 / 16 elements and zero the padding rows, so a kernel that reads padding adds zeros and one that writes padding writes zeros over zeros.
Here the panel lies inside a larger buffer whose rows outside [0, n) of every column hold something else:

  nan_pad   ld = n + 3 or n + 4, padding = a NaN with a distinctive payload (a read of it poisons the result);
  big_pad   the same with +-1e300 (a read of it swamps the result, a square of it overflows);
  offNNN    the panel starts NNN bytes (16, 48, 240: 16-byte but not 256-byte aligned) into the buffer, with live non-zero rows above it,
            between its columns and below it -- a sharded caller's layout;
  unpadded  ld = n (real kind: n even, complex kind: n odd), 16 bytes of NaN above and NaN below: no column starts on a 256-byte grid;
  far columns  ld = 2^26 or 2^28 bytes' worth of elements, columns beyond 2^32 bytes, 2^31 and 2^32 doubles from the base: tests/test_gpu_far_columns.py.

Every result is compared with the oracle, and every row of the buffer outside [0, n) of the panel must be BIT-identical after the call."""
import ctypes as C

import numpy as np
import pytest

import lightkrylov_amd as lk
from lightkrylov_amd import _capi
from oracle import oracle as ora
from tests._gpu_helpers import KINDS, POISON, CallerPanel, basis, fit, orthonormal_basis, seeded
from tests._tol import assert_columns_close

pytestmark = pytest.mark.gpu

LAYOUTS = ["nan_pad", "big_pad", "off16", "off48", "off240", "unpadded"]


_CTXS = {}


def tuned(**kw):
    """one context per tuning set for the whole module (closed at its end)"""
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


def _scale_ok(got, ref, rtol, what):
    got, ref = np.asarray(got), np.asarray(ref)
    err = np.abs(got - ref).max() if got.size else 0.0
    sc = max(float(np.abs(ref).max()) if ref.size else 0.0, 1e-300)
    assert err <= rtol * sc, f"{what}: differs by {err / sc:.2e} (relative) > {rtol:.0e}"


def _rand_scalar(dtype, seed):
    r = np.random.default_rng(seed)
    return complex(r.uniform(-2, 2), r.uniform(-2, 2)) if np.dtype(dtype).kind == "c" else float(r.uniform(-2, 2))


# ---- BLAS-1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", KINDS)
def test_blas1_on_caller_panels(ctx, dtype, layout):
    """scal, axpby, dot, norm, copy (AbstractVectors.fypp:505-555, 717-723) with n = 1, an odd n below a wave's share and one larger than a
    block's share, against the oracle's BLAS-1; the odd last element and the row pairs of the vector kernels meet the padding here."""
    for n0 in (1, 33, 100_003):
        n = fit(n0, dtype, layout)
        P = CallerPanel(ctx, dtype, n, 4, layout, seed=n0)
        X = basis(n, 4, dtype, 100 + n0)
        P.set(X)
        x, y, z, w = P.B[0], P.B[1], P.B[2], P.B[3]
        a, b = _rand_scalar(dtype, 1), _rand_scalar(dtype, 2)
        nx, ny = np.linalg.norm(X[:, 0]), np.linalg.norm(X[:, 1])
        assert abs(x.dot(y) - ora.dot(X[:, 0], X[:, 1])) <= 1e-12 * nx * ny
        assert abs(x.norm() - ora.norm(X[:, 0])) <= 1e-12 * nx
        ref = X.copy(order="F")
        x.scal(a)
        ora.scal(ref[:, 0], a)
        y.axpby(a, z, b)
        ora.axpby(a, ref[:, 2], b, ref[:, 1])
        lk.copy(w, x)
        ref[:, 3] = ref[:, 0]
        got = P.get("scal / axpby / copy")
        for j in range(4):
            _scale_ok(got[:, j], ref[:, j], 1e-15 * 4, f"column {j}, n = {n}")
        assert np.array_equal(got[:, 3], got[:, 0])


# ---- the Gram-Schmidt step on both schedules -----------------------------------------------------------------------------------------
SCHEDULES = {"three_sweeps": dict(resident=0), "single_onchip": dict(resident=1, resident_onchip=1),
             "single_cache": dict(resident=1, resident_onchip=0)}


def _dgs_basis(n, k, dtype, seed):
    """orthonormal when it can be; n < k: unit columns (the step's arithmetic is the same, the bound below is looser)"""
    if k <= n:
        return orthonormal_basis(n, k, dtype, seed)
    X = basis(n, k, dtype, seed)
    return np.asfortranarray(X / np.linalg.norm(X, axis=0))


@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", KINDS)
def test_dgs_on_caller_panels(dtype, layout, schedule):
    """lk_dgs (gram_schmidt.fypp:12-57) with k = 1, 8, 16, 32, 33, 128 at n < 32 and at a ragged n: the three sweeps, the single launch
    with the panel in registers and the single launch from the cache -- the resident counters show that the single launch ran."""
    c = tuned(**SCHEDULES[schedule])
    before = c.resident_stats()
    calls = 0
    for n0 in (29, 1037):
        n = fit(n0, dtype, layout)
        for k in (1, 8, 16, 32, 33, 128):
            Q = _dgs_basis(n, k, dtype, 40 + k)
            y = seeded(n, dtype, 5000 + k)             # (a seed of no column of Q)
            P = CallerPanel(c, dtype, n, k + 1, layout, seed=k)
            P.set(Q)
            P.set(y, k)
            yo = y.copy()
            ho, _ = ora.double_gram_schmidt_step(yo, Q.copy(order="F"))
            h = np.zeros(k, dtype=dtype)
            lk.double_gram_schmidt_step(P.B[k], P.B[:k], False, beta=h)
            calls += 1
            got = P.get(f"dgs k = {k}")
            rtol = 1e-12 if k <= n else 1e-11              # (n < k: a rank-deficient X amplifies both passes by ||X||_2^2 ~ 10)
            _scale_ok(h, ho, rtol, f"dgs k = {k}, n = {n}: beta")
            _scale_ok(got[:, k], yo, rtol, f"dgs k = {k}, n = {n}: y''")
            assert np.array_equal(got[:, :k], Q)           # X is read only
    after = c.resident_stats()
    if schedule == "three_sweeps":
        assert after[0] == before[0], (before, after)
    else:
        assert after[0] - before[0] == calls and after[1] == before[1], (before, after)
        assert (after[2] - before[2] > 0) == (schedule == "single_onchip"), (before, after)


# ---- Gram, innerprod, linear_combination ---------------------------------------------------------------------------------------------
GRAM_K = {np.float64: (4, 5, 32, 33, 128, 129), np.complex128: (32, 33, 80, 81, 112, 113)}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", KINDS)
def test_gram_on_caller_panels(ctx, dtype, layout):
    """lk_gram (AbstractVectors.fypp:645-657) on each side of every kernel change -- real: the VALU dots | panel_gram_rs | the wide
    matrix-core tiles; complex: panel_gram_rs3m | rs3m4 | mfma3m -- at n < 32 and at a ragged n (the LDS-DMA kernels stage ragged tiles)."""
    for n0 in (29, 1037):
        n = fit(n0, dtype, layout)
        for k in GRAM_K[dtype]:
            X = basis(n, k, dtype, 7 + k)
            P = CallerPanel(ctx, dtype, n, k, layout, seed=k)
            P.set(X)
            G = lk.Gram(P.B)
            P.get(f"Gram k = {k}")
            err = np.abs(G - ora.gram(X)).max()
            assert err <= 1e-13 * np.linalg.norm(X, axis=0).max() ** 2, f"Gram k = {k}, n = {n}: {err:.2e}"


PRODUCT_CFGS = {"valu": dict(xhy_mfma=0, gemm_mfma_min=100), "mfma": dict(gemm_mfma_min=0, gemm_3m=0), "mfma3m": dict(gemm_mfma_min=0, gemm_3m=1)}


@pytest.mark.parametrize("cfg", list(PRODUCT_CFGS))
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", KINDS)
def test_innerprod_and_lincomb_on_caller_panels(dtype, layout, cfg):
    """lk_innerprod (AbstractVectors.fypp:659-695) and lk_lincomb (:571-643) between two caller panels on the vector kernels, the matrix
    cores and the three-product complex kernels (`gemm_mfma_min` as in test_gpu_lincomb); the output panel's padding is live too."""
    c = tuned(**PRODUCT_CFGS[cfg])
    lib = _capi.load()
    for n0 in (29, 1037):
        n = fit(n0, dtype, layout)
        for k, p in ((33, 1), (40, 3), (64, 9), (129, 33)):
            X, Y = basis(n, k, dtype, 3 + k), basis(n, p, dtype, 500 + p)
            Px = CallerPanel(c, dtype, n, k, layout, seed=k)
            Py = CallerPanel(c, dtype, n, p + 1, layout, seed=p + 1000)
            Px.set(X)
            Py.set(Y)
            M = lk.innerprod(Px.B, Py.B[:p])
            scale = np.linalg.norm(X, axis=0).max() * np.linalg.norm(Y, axis=0).max()
            assert np.abs(np.asarray(M).reshape(k, p) - ora.innerprod(X, Y).reshape(k, p, order="F")).max() <= 1e-13 * scale, (n, k, p)
            Cm = basis(k, p, dtype, 900 + k)
            j0 = 1                                                  # (an output that does not start at column 0)
            _capi.check(lib.lk_lincomb(Px.B._h, k, Cm.ctypes.data_as(C.POINTER(C.c_double)), p, Py.B._h, j0))
            got = Py.get(f"lincomb k = {k}, q = {p}")
            Px.get(f"lincomb input k = {k}")
            for j in range(p):
                ref = ora.linear_combination(X, np.ascontiguousarray(Cm[:, j]))
                sc = (np.abs(X.real) + np.abs(X.imag)).max(axis=0) @ (np.abs(Cm[:, j].real) + np.abs(Cm[:, j].imag))
                assert np.abs(got[:, j0 + j] - ref).max() <= 1e-14 * sc, (n, k, p, j)


# ---- block Gram-Schmidt --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", KINDS)
def test_dgs_block_on_caller_panels(ctx, dtype, layout):
    """lk_dgs_block (gram_schmidt.fypp:59-105): p <= 4 on the fused sweeps, p = 9 on the matrix cores (complex: the four-pass schedule),
    real p = 20 and 32 on the fused pass by row-owner waves (panel_xhy_upd_rs, whose last 32-row tile is ragged at these n)."""
    for n0 in (301, 1037):
        n = fit(n0, dtype, layout)
        for k, p in ((40, 2), (64, 4), (100, 9), (128, 20), (96, 32)):
            Q = orthonormal_basis(n, k, dtype, 60 + k)
            Y = basis(n, p, dtype, 700 + p)
            Px = CallerPanel(ctx, dtype, n, k, layout, seed=k)
            Py = CallerPanel(ctx, dtype, n, p, layout, seed=p + 2000)
            Px.set(Q)
            Py.set(Y)
            Yo = Y.copy(order="F")
            ho, _ = ora.double_gram_schmidt_step_block(Yo, Q.copy(order="F"))
            h = np.zeros((k, p), dtype=dtype, order="F")
            lk.double_gram_schmidt_step(Py.B, Px.B, False, beta=h)
            got = Py.get(f"dgs_block k = {k}, p = {p}")
            assert np.array_equal(Px.get("dgs_block X"), Q)
            assert_columns_close(h, ho, f"dgs_block {layout} n = {n} k = {k} p = {p}: beta")
            for j in range(p):
                _scale_ok(got[:, j], Yo[:, j], 1e-12, f"dgs_block k = {k}, p = {p}, n = {n}: column {j}")


# ---- factorisations with the basis wrapped -------------------------------------------------------------------------------------------
def _tridiag_csr(n, dtype):
    import scipy.sparse as sp
    g = np.arange(n) / n
    A = sp.diags([-0.5 * np.ones(n - 1), 2.0 + g, -0.5 * np.ones(n - 1)], [-1, 0, 1]).tocsr()
    return A.astype(dtype)


def _ops(kind, n, dtype, ctx, hermitian=False):
    """(engine operator, oracle operator, oracle adjoint): a diagonal, or a CSR matrix (x and y are wrapped columns in its SpMV)"""
    if kind == "diag":
        g = np.arange(n) / n
        d = (1.0 + g) * (np.exp(0.4j * g) if np.dtype(dtype).kind == "c" and not hermitian else 1.0)
        d = d.astype(dtype)
        return lk.diag_linop_gpu(d, ctx), ora.DiagOp(d), ora.DiagOp(d.conj())
    A = _tridiag_csr(n, dtype)
    if np.dtype(dtype).kind == "c" and not hermitian:
        A = (A * (1.0 + 0.3j)).tocsr()
    Ah = A.conj().T.tocsr()
    return lk.csr_linop_gpu(A, ctx), ora.PyOp(lambda x: A @ x, dtype), ora.PyOp(lambda x: Ah @ x, dtype)


def _start(n, dtype, seed):
    x = seeded(n, dtype, seed)
    return x / np.linalg.norm(x)


@pytest.mark.parametrize("op", ["diag", "csr"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", KINDS)
def test_factorisations_on_a_caller_basis(dtype, layout, op):
    """lk_arnoldi (both schedules of the step), lk_lanczos, lk_bidiag, lk_qr and lk_arnoldi_block (p = 2, 4) with the basis wrapped, against
    ora.arnoldi / lanczos / bidiagonalization / qr_no_pivoting / arnoldi_block, 1e-12 per column of the projected matrix."""
    n = fit(1037, dtype, layout)
    m = 12
    for sched in ("three_sweeps", "single_onchip"):
        c = tuned(**SCHEDULES[sched])
        A, Ao, _ = _ops(op, n, dtype, c)
        x0 = _start(n, dtype, 7)
        P = CallerPanel(c, dtype, n, m + 1, layout, seed=1)
        P.set(np.zeros((n, m + 1), dtype=dtype))
        P.set(x0, 0)
        H = np.zeros((m + 1, m), dtype=dtype, order="F")
        assert lk.arnoldi(A, P.B, H) == 0
        Xo = np.zeros((n, m + 1), dtype=dtype, order="F")
        Xo[:, 0] = x0
        Ho = np.zeros((m + 1, m), dtype=dtype, order="F")
        assert ora.arnoldi(Ao, Xo, Ho) == 0
        assert_columns_close(H, Ho, f"arnoldi {op} {layout} {sched}")
        _scale_ok(P.get("arnoldi"), Xo, 1e-11, f"arnoldi {op} {sched}: basis")
    c = tuned()
    # Lanczos on the Hermitian variant of the operator
    A, Ao, _ = _ops(op, n, dtype, c, hermitian=True)
    P = CallerPanel(c, dtype, n, m + 1, layout, seed=2)
    P.set(np.zeros((n, m + 1), dtype=dtype))
    P.set(_start(n, dtype, 8), 0)
    T = np.zeros((m + 1, m), dtype=dtype, order="F")
    assert lk.lanczos(A, P.B, T) == 0
    Xo = np.zeros((n, m + 1), dtype=dtype, order="F")
    Xo[:, 0] = _start(n, dtype, 8)
    To = np.zeros((m + 1, m), dtype=dtype, order="F")
    assert ora.lanczos(Ao, Xo, To) == 0
    assert_columns_close(T, To, f"lanczos {op} {layout}")
    P.get("lanczos")
    # Golub-Kahan: both bases wrapped
    A, Ao, Aho = _ops(op, n, dtype, c)
    U = CallerPanel(c, dtype, n, m + 1, layout, seed=3)
    V = CallerPanel(c, dtype, n, m, layout, seed=4)
    U.set(np.zeros((n, m + 1), dtype=dtype))
    U.set(_start(n, dtype, 9), 0)
    V.set(np.zeros((n, m), dtype=dtype))
    Bm = np.zeros((m + 1, m), dtype=dtype, order="F")
    assert lk.bidiagonalization(A, U.B, V.B, Bm) == 0
    Uo = np.zeros((n, m + 1), dtype=dtype, order="F")
    Uo[:, 0] = _start(n, dtype, 9)
    Vo = np.zeros((n, m), dtype=dtype, order="F")
    Bo = np.zeros((m + 1, m), dtype=dtype, order="F")
    assert ora.bidiagonalization(Ao, Aho, Uo, Vo, Bo) == 0
    assert_columns_close(Bm, Bo, f"bidiag {op} {layout}")
    U.get("bidiag U")
    V.get("bidiag V")
    # qr_no_pivoting of a wrapped panel
    for p in (4, 6):
        M = basis(n, p, dtype, 300 + p)
        P = CallerPanel(c, dtype, n, p, layout, seed=5)
        P.set(M)
        R = np.zeros((p, p), dtype=dtype, order="F")
        assert lk.qr(P.B, R) == 0
        Mo, Ro = M.copy(order="F"), np.zeros((p, p), dtype=dtype, order="F")
        assert ora.qr_no_pivoting(Mo, Ro) == 0
        assert_columns_close(R, Ro, f"qr p = {p} {layout}")
        _scale_ok(P.get("qr"), Mo, 1e-12, f"qr p = {p}: Q")
    # block Arnoldi
    kdim = 5
    for p in (2, 4):
        Q0 = orthonormal_basis(n, p, dtype, 70 + p)
        ncol = (kdim + 1) * p
        P = CallerPanel(c, dtype, n, ncol, layout, seed=6)
        P.set(np.zeros((n, ncol), dtype=dtype))
        P.set(Q0, 0)
        H = np.zeros((ncol, kdim * p), dtype=dtype, order="F")
        assert lk.arnoldi(A, P.B, H, blksize=p) == 0
        Xo = np.zeros((n, ncol), dtype=dtype, order="F")
        Xo[:, :p] = Q0
        Ho = np.zeros((ncol, kdim * p), dtype=dtype, order="F")
        assert ora.arnoldi_block(Ao, Xo, Ho, p) == 0
        assert_columns_close(H, Ho, f"arnoldi_block p = {p} {op} {layout}")
        P.get("arnoldi_block")
