"""NaN and Inf in, "|beta| = NaN detected! Abort" (LK_ERR_NAN, [-5]) out -- and the context computes correctly afterwards.

The reference stops where qr_no_pivoting meets a NaN norm (qr.fypp:137-143; test_oracle_nonfinite.py pins where the oracle does).  The engine
returns LK_ERR_NAN from lk_dgs, lk_dgs_block, lk_qr, lk_arnoldi(_segments), lk_arnoldi_block, lk_lanczos and lk_bidiag; inside an asynchronous
batch the NaN step raises the device stop flag so that the steps queued behind it do nothing.  Every case checks that the columns before the
failing step are the oracle's, that the failing step is the oracle's (the first column holding a NaN), and then runs a clean factorisation on
the SAME context (the same basis object where there is one) against the oracle: a stop flag, a step slot or a lazy memo the NaN left behind
would show there.  A 1e300 entry (||y||^2 = +Inf, no NaN) must be classified as the oracle classifies it and must not raise."""
import numpy as np
import pytest

import lightkrylov_amd as lk
from lightkrylov_amd import _capi
from oracle import oracle as ora
from tests._gpu_helpers import KINDS, basis, orthonormal_basis, seeded
from tests._tol import assert_columns_close
from tests.test_oracle_nonfinite import first_nan_column, nan_on_call

pytestmark = pytest.mark.gpu
NAN_ERR = r"\[-5\] \|beta\| = NaN detected"
SCHEDULES = {"three_sweeps": dict(resident=0), "single_onchip": dict(resident=1, resident_onchip=1),
             "single_cache": dict(resident=1, resident_onchip=0)}


@pytest.fixture()
def fresh():
    ctxs = []

    def make(**kw):
        c = lk.Context(device=0)
        for key, val in kw.items():
            c.set_tuning(key, val)
        ctxs.append(c)
        return c
    yield make
    for c in ctxs:
        c.close()


def _diag(n, dtype, hermitian=False):
    g = np.arange(n) / n
    d = (1.0 + g) * (np.exp(0.4j * g) if np.dtype(dtype).kind == "c" and not hermitian else 1.0)
    return d.astype(dtype)


def _start(n, dtype, seed):
    x = seeded(n, dtype, seed)
    return x / np.linalg.norm(x)


def _clean_dgs(c, B, k, dtype, seed):
    """a clean Gram-Schmidt step on the columns of B against the oracle"""
    n = B.n_local
    Q, y = orthonormal_basis(n, k, dtype, seed), seeded(n, dtype, seed + 10_000)
    B.upload(Q, 0)
    B.upload(y.reshape(-1, 1), k)
    yo = y.copy()
    ho, _ = ora.double_gram_schmidt_step(yo, Q.copy(order="F"))
    h = np.zeros(k, dtype=dtype)
    lk.double_gram_schmidt_step(B[k], B[:k], False, beta=h)
    assert np.abs(h - ho).max() <= 1e-12 * np.abs(ho).max()
    assert np.abs(B.download(k, 1)[:, 0] - yo).max() <= 1e-12 * np.abs(yo).max()


def _arnoldi_oracle(d, x0, m, dtype, kend=None, Xo=None, Ho=None, kstart=1, op=None):
    n = len(x0)
    if Xo is None:
        Xo = np.zeros((n, m + 1), dtype=dtype, order="F")
        Xo[:, 0] = x0
        Ho = np.zeros((m + 1, m), dtype=dtype, order="F")
    info = ora.arnoldi(op or ora.DiagOp(d), Xo, Ho, kstart=kstart, kend=kend)
    return info, Xo, Ho


def _clean_arnoldi(c, X, dtype, seed, what):
    n, m = X.n_local, len(X) - 1
    d = _diag(n, dtype)
    x0 = _start(n, dtype, seed)
    X.upload(np.zeros((n, m + 1), dtype=dtype))
    X.upload(x0.reshape(-1, 1), 0)
    H = np.zeros((m + 1, m), dtype=dtype, order="F")
    assert lk.arnoldi(lk.diag_linop_gpu(d, c), X, H) == 0
    _, _, Ho = _arnoldi_oracle(d, x0, m, dtype)
    assert_columns_close(H, Ho, f"clean Arnoldi after {what}")


# ---- a NaN in the vector being orthogonalised, and in a basis column ----------------------------------------------------------------
@pytest.mark.parametrize("k", [128, 129], ids=["k128_single_launch", "k129_sweeps"])
@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("dtype", KINDS)
def test_dgs_with_nan_in_y_or_in_a_basis_column(fresh, dtype, schedule, k):
    """lk_dgs on both sides of the single launch's 128 columns: a NaN in y, then one in column 5 of X -- LK_ERR_NAN both times, then a clean
    step and a clean Arnoldi factorisation on the same context and panel."""
    c = fresh(**SCHEDULES[schedule])
    n = 20_011
    B = lk.krylov_basis_gpu(n, k + 1, dtype, c)
    st0 = c.resident_stats()
    for where in ("y", "basis"):
        Q, y = orthonormal_basis(n, k, dtype, 80), seeded(n, dtype, 5000)
        if where == "y":
            y[n // 2] = np.nan
        else:
            Q[n // 3, 5] = np.nan
        B.upload(Q, 0)
        B.upload(y.reshape(-1, 1), k)
        h = np.zeros(k, dtype=dtype)
        with pytest.raises(_capi.LightKrylovHipError, match=NAN_ERR):
            lk.double_gram_schmidt_step(B[k], B[:k], False, beta=h)
        _clean_dgs(c, B, k, dtype, 90)
    st1 = c.resident_stats()
    assert (st1[0] - st0[0] == 4) == (schedule != "three_sweeps" and k <= 128), (st0, st1)
    assert st1[1] == st0[1]
    X = lk.krylov_basis_gpu(n, 21, dtype, c)
    _clean_arnoldi(c, X, dtype, 7, f"lk_dgs NaN ({schedule})")


@pytest.mark.parametrize("k,p", [(40, 2), (64, 4), (100, 20), (96, 32)])
@pytest.mark.parametrize("dtype", KINDS)
def test_dgs_block_with_nan_in_a_basis_column(fresh, dtype, k, p):
    """lk_dgs_block with 1..4 columns per pass (fused sweeps) and 17..32 (matrix cores; real: the fused pass by row-owner waves)"""
    c = fresh()
    n = 10_037
    Q, Y = orthonormal_basis(n, k, dtype, 60), basis(n, p, dtype, 5000)
    Q[n // 2, k // 2] = np.nan
    Bx = lk.krylov_basis_gpu(n, k, dtype, c)
    By = lk.krylov_basis_gpu(n, p, dtype, c)
    Bx.upload(Q)
    By.upload(Y)
    h = np.zeros((k, p), dtype=dtype, order="F")
    with pytest.raises(_capi.LightKrylovHipError, match=NAN_ERR):
        lk.double_gram_schmidt_step(By, Bx, False, beta=h)
    # the same panels, clean
    Q = orthonormal_basis(n, k, dtype, 62)
    Bx.upload(Q)
    By.upload(Y)
    Yo = Y.copy(order="F")
    ho, _ = ora.double_gram_schmidt_step_block(Yo, Q.copy(order="F"))
    assert lk.double_gram_schmidt_step(By, Bx, False, beta=h) == 0
    assert_columns_close(h, ho, f"dgs_block k = {k}, p = {p} after a NaN")
    assert np.abs(By.download() - Yo).max() <= 1e-12 * np.abs(Yo).max()


@pytest.mark.parametrize("j", [0, 3])
@pytest.mark.parametrize("dtype", KINDS)
def test_qr_stops_at_the_nan_column(fresh, dtype, j):
    """lk_qr (qr.fypp:116-167) with a NaN in column j: R(:, :j) is the oracle's, the error comes at column j as the oracle's does"""
    c = fresh()
    n, p = 20_011, 5
    M = basis(n, p, dtype, 300)
    M[n // 4, j] = np.nan
    Mo, Ro = M.copy(order="F"), np.zeros((p, p), dtype=dtype, order="F")
    with pytest.raises(FloatingPointError):
        ora.qr_no_pivoting(Mo, Ro)
    B = lk.krylov_basis_gpu(n, p, dtype, c)
    B.upload(M)
    R = np.zeros((p, p), dtype=dtype, order="F")
    with pytest.raises(_capi.LightKrylovHipError, match=NAN_ERR):
        lk.qr(B, R)
    if j:
        assert_columns_close(R[:, :j], Ro[:, :j], "qr before the NaN column")
    # the same panel, clean
    M = basis(n, p, dtype, 301)
    B.upload(M)
    Mo, Ro = M.copy(order="F"), np.zeros((p, p), dtype=dtype, order="F")
    assert ora.qr_no_pivoting(Mo, Ro) == 0
    assert lk.qr(B, R) == 0
    assert_columns_close(R, Ro, "qr after a NaN")
    assert np.abs(B.download() - Mo).max() <= 1e-12


# ---- an operator that returns NaN inside an asynchronous batch ----------------------------------------------------------------------
@pytest.mark.parametrize("segments", [False, True], ids=["arnoldi", "arnoldi_segments"])
@pytest.mark.parametrize("schedule", ["three_sweeps", "single_onchip"])
@pytest.mark.parametrize("dtype", KINDS)
def test_arnoldi_batch_with_a_nan_operator(fresh, dtype, schedule, segments):
    """Steps 1..s-1 with a clean diagonal, then kstart = s with a diagonal that holds one NaN: steps s+1..m are queued behind step s in the
    same batch.  LK_ERR_NAN at step s, as the oracle's -1; H(:, :s-1) the oracle's; nothing reported beyond; then a clean factorisation
    on the same basis object."""
    c = fresh(**SCHEDULES[schedule])
    n, m, s = 20_011, 30, 5
    d = _diag(n, dtype)
    dn = d.copy()
    dn[n // 3] = np.nan
    x0 = _start(n, dtype, 11)
    X = lk.krylov_basis_gpu(n, m + 1, dtype, c)
    X.upload(x0.reshape(-1, 1), 0)
    H = np.zeros((m + 1, m), dtype=dtype, order="F")
    assert lk.arnoldi(lk.diag_linop_gpu(d, c), X, H, kend=s - 1) == 0
    seen = []
    kw = dict(_segments=list(range(s, m + 1)), _progress=lambda a, b: seen.append((a, b)) and False) if segments else {}
    with pytest.raises(_capi.LightKrylovHipError, match=NAN_ERR):
        lk.arnoldi(lk.diag_linop_gpu(dn, c), X, H, kstart=s, **kw)
    assert seen == []
    _, Xo, Ho = _arnoldi_oracle(d, x0, m, dtype, kend=s - 1)
    assert _arnoldi_oracle(dn, x0, m, dtype, Xo=Xo, Ho=Ho, kstart=s)[0] == -1
    assert first_nan_column(Ho) == s == first_nan_column(H)
    assert_columns_close(H[:, :s - 1], Ho[:, :s - 1], "Arnoldi before the NaN step")
    assert not H[:, s:].any()
    _clean_arnoldi(c, X, dtype, 12, f"a NaN batch ({schedule})")


@pytest.mark.parametrize("p", [2, 4])
@pytest.mark.parametrize("dtype", KINDS)
def test_block_arnoldi_with_a_nan_operator(fresh, dtype, p):
    c = fresh()
    n, kdim, s = 10_037, 6, 3
    d = _diag(n, dtype)
    dn = d.copy()
    dn[n // 3] = np.nan
    Q0 = orthonormal_basis(n, p, dtype, 70)
    ncol = (kdim + 1) * p
    X = lk.krylov_basis_gpu(n, ncol, dtype, c)
    X.upload(Q0, 0)
    H = np.zeros((ncol, kdim * p), dtype=dtype, order="F")
    assert lk.arnoldi(lk.diag_linop_gpu(d, c), X, H, blksize=p, kend=s - 1) == 0
    with pytest.raises(_capi.LightKrylovHipError, match=NAN_ERR):
        lk.arnoldi(lk.diag_linop_gpu(dn, c), X, H, blksize=p, kstart=s)
    Xo = np.zeros((n, ncol), dtype=dtype, order="F")
    Xo[:, :p] = Q0
    Ho = np.zeros((ncol, kdim * p), dtype=dtype, order="F")
    assert ora.arnoldi_block(ora.DiagOp(d), Xo, Ho, p, kend=s - 1) == 0
    with pytest.raises(FloatingPointError):
        ora.arnoldi_block(ora.DiagOp(dn), Xo, Ho, p, kstart=s)
    assert first_nan_column(Ho) == (s - 1) * p + 1
    assert first_nan_column(H) in (0, (s - 1) * p + 1) and not H[:, s * p:].any()       # (the engine stops before it writes step s's block)
    assert_columns_close(H[:, :(s - 1) * p], Ho[:, :(s - 1) * p], f"block Arnoldi p = {p} before the NaN step")
    # clean, same basis object
    X.upload(np.zeros((n, ncol), dtype=dtype))
    X.upload(Q0, 0)
    H[...] = 0
    assert lk.arnoldi(lk.diag_linop_gpu(d, c), X, H, blksize=p) == 0
    Xo[...] = 0
    Xo[:, :p] = Q0
    Ho[...] = 0
    assert ora.arnoldi_block(ora.DiagOp(d), Xo, Ho, p) == 0
    assert_columns_close(H, Ho, f"block Arnoldi p = {p} after a NaN")


@pytest.mark.parametrize("schedule", ["three_sweeps", "single_onchip"])
@pytest.mark.parametrize("dtype", KINDS)
def test_lanczos_and_bidiag_with_a_nan_operator(fresh, dtype, schedule):
    """The reference's Lanczos and Golub-Kahan loops have no NaN test and run on (test_oracle_nonfinite); the engine stops at the step whose
    column first holds a NaN in the oracle, with the columns before it the oracle's, and the context is sound afterwards."""
    c = fresh(**SCHEDULES[schedule])
    n, m, s = 20_011, 16, 4
    d = _diag(n, dtype, hermitian=True)
    dn = d.copy()
    dn[n // 3] = np.nan
    x0 = _start(n, dtype, 13)
    # Lanczos
    X = lk.krylov_basis_gpu(n, m + 1, dtype, c)
    X.upload(x0.reshape(-1, 1), 0)
    T = np.zeros((m + 1, m), dtype=dtype, order="F")
    assert lk.lanczos(lk.diag_linop_gpu(d, c), X, T, kend=s - 1) == 0
    with pytest.raises(_capi.LightKrylovHipError, match=NAN_ERR):
        lk.lanczos(lk.diag_linop_gpu(dn, c), X, T, kstart=s)
    Xo = np.zeros((n, m + 1), dtype=dtype, order="F")
    Xo[:, 0] = x0
    To = np.zeros((m + 1, m), dtype=dtype, order="F")
    assert ora.lanczos(ora.DiagOp(d), Xo, To, kend=s - 1) == 0
    ora.lanczos(ora.DiagOp(dn), Xo, To, kstart=s)
    assert first_nan_column(To) == s == first_nan_column(T)
    assert_columns_close(T[:, :s - 1], To[:, :s - 1], "Lanczos before the NaN step")
    assert not T[:, s:].any()
    # Golub-Kahan
    U = lk.krylov_basis_gpu(n, m + 1, dtype, c)
    V = lk.krylov_basis_gpu(n, m, dtype, c)
    U.upload(x0.reshape(-1, 1), 0)
    Bm = np.zeros((m + 1, m), dtype=dtype, order="F")
    assert lk.bidiagonalization(lk.diag_linop_gpu(d, c), U, V, Bm, kend=s - 1) == 0
    with pytest.raises(_capi.LightKrylovHipError, match=NAN_ERR):
        lk.bidiagonalization(lk.diag_linop_gpu(dn, c), U, V, Bm, kstart=s)
    Uo = np.zeros((n, m + 1), dtype=dtype, order="F")
    Uo[:, 0] = x0
    Vo = np.zeros((n, m), dtype=dtype, order="F")
    Bo = np.zeros((m + 1, m), dtype=dtype, order="F")
    assert ora.bidiagonalization(ora.DiagOp(d), ora.DiagOp(d.conj()), Uo, Vo, Bo, kend=s - 1) == 0
    ora.bidiagonalization(ora.DiagOp(dn), ora.DiagOp(dn.conj()), Uo, Vo, Bo, kstart=s)
    assert first_nan_column(Bo) == s
    assert first_nan_column(Bm) in (0, s) and not Bm[:, s:].any()                       # (the engine stops before it writes alpha(s))
    assert_columns_close(Bm[:, :s - 1], Bo[:, :s - 1], "Golub-Kahan before the NaN step")
    # clean Lanczos on the same basis object, then Arnoldi
    X.upload(np.zeros((n, m + 1), dtype=dtype))
    X.upload(x0.reshape(-1, 1), 0)
    T[...] = 0
    assert lk.lanczos(lk.diag_linop_gpu(d, c), X, T) == 0
    Xo[...] = 0
    Xo[:, 0] = x0
    To[...] = 0
    assert ora.lanczos(ora.DiagOp(d), Xo, To) == 0
    assert_columns_close(T, To, f"Lanczos after a NaN ({schedule})")
    _clean_arnoldi(c, lk.krylov_basis_gpu(n, m + 1, dtype, c), dtype, 14, f"a NaN Lanczos ({schedule})")


@pytest.mark.parametrize("dtype", KINDS)
def test_lazy_per_object_arnoldi_with_a_torch_operator_that_returns_nan(fresh, dtype):
    """Per-object Arnoldi in lazy mode (batched dots, the speculative sweep of the next norm) with a user operator written in torch that
    writes a NaN on its s-th call: the host-side qr raises FloatingPointError at step s, as the oracle's -1; then the same context and
    basis, a clean operator: H equals the oracle's and the speculation is used again (no memo of the NaN step survives)."""
    import torch
    c = fresh(lazy=1, lazy_speculate=1)
    n, m, s = 20_011, 12, 5
    d = _diag(n, dtype)
    dt = torch.as_tensor(d, device="cuda:0")
    calls = [0]

    class torch_diag(lk.abstract_linop):
        def __init__(self, poison_at):
            super().__init__()
            self.poison_at = poison_at

        def matvec(self, vi, vo):
            calls[0] += 1
            out = vo.as_torch("w")
            torch.mul(dt, vi.as_torch("r"), out=out)
            if calls[0] == self.poison_at:
                out[n // 3] = float("nan")

    x0 = _start(n, dtype, 15)
    B = lk.krylov_basis_gpu(n, m + 1, dtype, c)
    B.upload(x0.reshape(-1, 1), 0)
    X = [B[j] for j in range(m + 1)]
    H = np.zeros((m + 1, m), dtype=dtype, order="F")
    with pytest.raises(FloatingPointError):
        lk.arnoldi(torch_diag(s), X, H)
    _, _, Ho = _arnoldi_oracle(d, x0, m, dtype, op=ora.PyOp(nan_on_call(d, s), dtype))
    assert first_nan_column(Ho) == s == first_nan_column(H)
    assert_columns_close(H[:, :s - 1], Ho[:, :s - 1], "lazy Arnoldi before the NaN step")
    spec0 = c.lazy_speculation_stats()
    assert spec0[0] > 0
    # clean, same context and basis
    B.upload(np.zeros((n, m + 1), dtype=dtype))
    B.upload(x0.reshape(-1, 1), 0)
    H[...] = 0
    calls[0] = 0
    assert lk.arnoldi(torch_diag(0), X, H) == 0
    _, _, Ho = _arnoldi_oracle(d, x0, m, dtype)
    assert_columns_close(H, Ho, "lazy Arnoldi after a NaN")
    assert c.lazy_speculation_stats()[0] > spec0[0]


# ---- Inf without NaN ----------------------------------------------------------------------------------------------------------------
def _classify(v):
    v = np.atleast_1d(np.asarray(v))
    parts = [v.real, v.imag] if np.iscomplexobj(v) else [v]
    return np.stack([np.where(np.isnan(p), 2, np.where(np.isinf(p), np.sign(p) * 3, 0)) for p in parts])


@pytest.mark.parametrize("schedule", ["three_sweeps", "single_onchip"])
@pytest.mark.parametrize("dtype", KINDS)
def test_an_entry_of_1e300_overflows_like_the_oracle(fresh, dtype, schedule):
    """||y||^2 overflows to +Inf in the oracle and the engine alike: norm, dot and lk_dgs give the oracle's classification (finite, +-Inf,
    NaN) entry by entry, finite values within 1e-12, and no LK_ERR_NAN where the oracle does not stop."""
    c = fresh(**SCHEDULES[schedule])
    n, k = 20_011, 8
    y = seeded(n, dtype, 16)
    y[n // 2] = 1e300
    z = seeded(n, dtype, 17)
    B = lk.krylov_basis_gpu(n, k + 2, dtype, c)
    Q = orthonormal_basis(n, k, dtype, 18)
    B.upload(Q, 0)
    B.upload(y.reshape(-1, 1), k)
    B.upload(z.reshape(-1, 1), k + 1)
    for got, want in ((B[k].norm(), ora.norm(y)), (B[k].dot(B[k]), ora.dot(y, y)), (B[k].dot(B[k + 1]), ora.dot(y, z)),
                      (B[k + 1].dot(B[k]), ora.dot(z, y))):
        assert np.array_equal(_classify(got), _classify(want)), (got, want)
        if np.isfinite(want):
            assert abs(got - want) <= 1e-12 * abs(want)
    assert np.isposinf(ora.norm(y))
    yo = y.copy()
    ho, info_o = ora.double_gram_schmidt_step(yo, Q.copy(order="F"))
    h = np.zeros(k, dtype=dtype)
    info = lk.double_gram_schmidt_step(B[k], B[:k], False, beta=h)
    got = B.download(k, 1)[:, 0]
    assert info == info_o
    assert np.array_equal(_classify(h), _classify(ho))
    assert np.array_equal(_classify(got), _classify(yo))
    fin = np.isfinite(ho)
    assert np.abs(h[fin] - ho[fin]).max() <= 1e-12 * np.abs(ho[fin]).max()
    fin = np.isfinite(yo)
    assert np.abs(got[fin] - yo[fin]).max() <= 1e-12 * np.abs(yo[fin]).max()
    _clean_dgs(c, B, k, dtype, 19)
