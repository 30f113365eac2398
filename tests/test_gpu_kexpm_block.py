"""lk_kexpm_block / kexpm on bases: kexpm_mat (src/Expm/ExpmLib.fypp:234-363) as one engine call.

The yardstick is the NumPy restatement in tests/_pivot_ref.py: same info; err_est within 1e-10 relative or 1e-14 absolute; C within
1e-12 normwise per column.  tol is placed BETWEEN two consecutive estimates of the restatement that lie at least a factor of 100
apart, a factor of 10 from each (`_tol_between`, computed from the restatement alone), so that rounding cannot move the stopping
step.  The 5-point Laplacian needs a square number of unknowns: its cases (and the CSR copy of it) run n = 64 and 1024."""
import ctypes as C

import numpy as np
import pytest

import lightkrylov_amd as lk
from lightkrylov_amd import _capi
from lightkrylov_amd.expm import expm
from oracle import oracle as ora
from tests import _pivot_ref as ref
from tests._gpu_helpers import CallerPanel, _lap5_csr, basis
from tests._tol import assert_columns_close

pytestmark = pytest.mark.gpu
KINDS = [np.float64, np.complex128]


def _raw(A, B, Cb, p, X, tau, tol, nk, trans=False, jb0=0, jc0=0):
    info, err = C.c_int(-99), C.c_double(-99.0)
    rc = X._lib.lk_kexpm_block(A._h, 1 if trans else 0, B._h, jb0, Cb._h, jc0, p, X._h, float(tau), float(tol), int(nk),
                               C.byref(info), C.byref(err))
    return rc, info.value, err.value


def _operators(kind, n, dtype, ctx, trans=False):
    """(engine operator, restatement operator -- the adjoint one for trans --, tau) with tau * spectrum in about [-0.4, 0]: the estimates of
    consecutive steps then lie more than a factor of 100 apart"""
    cplx = np.dtype(dtype).kind == "c"
    if kind == "diag":
        g = np.arange(n) / n
        d = ((-0.05 - 2.0 * g) * (np.exp(0.4j * g) if cplx else 1.0)).astype(dtype)
        return lk.diag_linop_gpu(d, ctx), ora.DiagOp(d), 0.2
    if kind == "dense":
        rng = np.random.default_rng(n)
        M = rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if cplx else 0.0)
        M = np.asfortranarray((M / np.sqrt(n) - 1.5 * np.eye(n)).astype(dtype))
        return lk.dense_linop_gpu(M, ctx), ora.DenseOp(np.asfortranarray(M.conj().T) if trans else M), (0.03 if cplx else 0.1)
    N = int(round(np.sqrt(n)))
    assert N * N == n and not cplx
    tau = -0.4 / (8.0 * (N + 1) ** 2)
    if kind == "lap5":
        return lk.laplacian2d_linop_gpu(N, ctx), ora.Lap5Op(N), tau
    S = _lap5_csr(N)
    return lk.csr_linop_gpu(S, ctx), ora.PyOp(lambda x: S @ x, np.float64), tau


def _tol_between(hist):
    """sqrt(h[s-1] h[s]) for the first step s whose estimate is a factor >= 100 below the one before and below 1e-6"""
    for s in range(1, len(hist)):
        if hist[s] > 0 and hist[s] < 1e-6 and hist[s - 1] / hist[s] >= 100.0:
            return float(np.sqrt(hist[s - 1] * hist[s]))
    raise AssertionError(f"no gap of a factor 100 in the restatement's estimates: {hist}")


def _compare(ctx, Aeng, Aref, Bh, tau, nk, trans=False, tol=None, label=""):
    n, p = Bh.shape
    dtype = Bh.dtype
    if tol is None:
        hist = []
        ref.kexpm_mat(Aref, Bh, tau, 0.0, nk, history=hist)
        tol = _tol_between(hist)
    hist = []
    Cr, info_r, err_r, _ = ref.kexpm_mat(Aref, Bh, tau, tol, nk, history=hist)
    if info_r > 0 and len(hist) > 1:
        assert hist[-1] * 10 <= tol <= hist[-2] / 10, (hist, tol)
    B = lk.krylov_basis_gpu(n, p, dtype, ctx)
    B.upload(Bh)
    Cb = lk.krylov_basis_gpu(n, p, dtype, ctx)
    X = lk.krylov_basis_gpu(n, p * (nk + 1), dtype, ctx)
    rc, info, err = _raw(Aeng, B, Cb, p, X, tau, tol, nk, trans)
    print(f"{label}: info {info} (restatement {info_r}), err_est {err:.3e} ({err_r:.3e}), tol {tol:.2e}")
    assert rc == 0 and info == info_r, (rc, info, info_r)
    assert abs(err - err_r) <= max(1e-10 * err_r, 1e-14), (err, err_r)
    assert_columns_close(Cb.download(), Cr, f"kexpm_block {label}")
    assert np.array_equal(B.download(), Bh)                                   # B is read only
    for o in (B, Cb, X):
        o.close()
    return info


CASES = ([("diag", dt, False) for dt in KINDS] + [("dense", dt, tr) for dt in KINDS for tr in (False, True)]
         + [("lap5", np.float64, False), ("csr", np.float64, False)])


@pytest.mark.parametrize("p", [1, 2, 3, 5])
@pytest.mark.parametrize("n", [64, 1000])
@pytest.mark.parametrize("kind,dtype,trans", CASES, ids=[f"{k}-{np.dtype(d).name}-{'H' if t else 'N'}" for k, d, t in CASES])
def test_against_the_restatement(ctx, kind, dtype, trans, n, p):
    if kind in ("lap5", "csr") and n == 1000:
        n = 1024
    Aeng, Aref, tau = _operators(kind, n, dtype, ctx, trans)
    Bh = np.asfortranarray(basis(n, p, dtype, 31 + p) * 2.0 ** (-np.arange(p, dtype=float)))
    nk = min(12, 64 // p - 1, n // p - 1)
    _compare(ctx, Aeng, Aref, Bh, tau, nk, trans, label=f"{kind} n={n} p={p} {np.dtype(dtype).name} trans={trans}")
    Aeng.close()


@pytest.mark.parametrize("dtype", KINDS, ids=["rdp", "cdp"])
def test_one_column_agrees_with_the_vector_form(ctx, dtype):
    n, tol = 1000, 1e-9
    Aeng, _, tau = _operators("diag", n, dtype, ctx)
    bh = basis(n, 1, dtype, 5)
    B = lk.krylov_basis_gpu(n, 1, dtype, ctx)
    B.upload(bh)
    c1, c2 = lk.krylov_basis_gpu(n, 1, dtype, ctx), lk.krylov_basis_gpu(n, 1, dtype, ctx)
    X = lk.krylov_basis_gpu(n, 41, dtype, ctx)
    i1 = lk.kexpm(c1[0], Aeng, B[0], tau, tol, kdim=40, _basis=X)
    rc, i2, _ = _raw(Aeng, B, c2, 1, X, tau, tol, 40)
    assert rc == 0 and i1 == i2 > 0
    assert_columns_close(c2.download(), c1.download(), "kexpm_block p=1 vs lk_kexpm")


@pytest.mark.parametrize("trans", [False, True], ids=["N", "H"])
@pytest.mark.parametrize("dtype", KINDS, ids=["rdp", "cdp"])
def test_reference_block_kexptA(ctx, dtype, trans):
    """test/TestExpmlib.fypp:148-230: random dense operator, p = 3, tau = 0.1, kdim = 15, tol = rtol_dp, against the dense exponential"""
    n, p, tau, kdim = 100, 3, 0.1, 15
    rng = np.random.default_rng(11)
    cplx = np.dtype(dtype).kind == "c"
    Ah = np.asfortranarray((rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if cplx else 0)).astype(dtype))
    Bh = np.asfortranarray((rng.standard_normal((n, p)) + (1j * rng.standard_normal((n, p)) if cplx else 0)).astype(dtype))
    Cref = expm(tau * (Ah.conj().T if trans else Ah)) @ Bh
    A = lk.dense_linop_gpu(Ah, ctx)
    B, Cb = lk.krylov_basis_gpu(n, p, dtype, ctx), lk.krylov_basis_gpu(n, p, dtype, ctx)
    B.upload(Bh)
    X = lk.krylov_basis_gpu(n, p * (kdim * p + 1), dtype, ctx)
    info = lk.kexpm(Cb, A, B, tau, lk.rtol_dp, trans=trans, kdim=kdim, _basis=X)
    D = Cb.download() - Cref
    err = np.linalg.norm(np.abs(D.conj().T @ D), 2)
    assert info > 0 and info % p == 0 and err < lk.rtol_dp, (info, err)
    assert A.get_counter(trans) == (info // p - 1) * p and A.get_counter(not trans) == 0
    # the workspace the mirror allocates itself: nk capped at 512 // p - 1
    A2 = lk.dense_linop_gpu(Ah, ctx)
    info2 = lk.kexpm(Cb, A2, B, tau, lk.rtol_dp, trans=trans)
    assert info2 == info
    with pytest.raises(ValueError):
        lk.kexpm(Cb, A, B, tau, lk.rtol_dp, kdim=kdim, _basis=lk.krylov_basis_gpu(n, p * (kdim * p + 1) - 1, dtype, ctx))


@pytest.mark.parametrize("dtype", KINDS, ids=["rdp", "cdp"])
def test_degenerate_blocks(ctx, dtype):
    """B = 0; B with a zero column; B with two equal columns (the pivoted start, R with a zero row): still exp(tau A) B at rtol_dp"""
    n, p, nk = 200, 3, 12
    Aeng, Aref, tau = _operators("dense", n, dtype, ctx)
    M, tau = Aref.A, 0.3
    B, Cb = lk.krylov_basis_gpu(n, p, dtype, ctx), lk.krylov_basis_gpu(n, p, dtype, ctx)
    X = lk.krylov_basis_gpu(n, p * (nk + 1), dtype, ctx)
    Cb.upload(basis(n, p, dtype, 2))
    rc, info, err = _raw(Aeng, B, Cb, p, X, tau, 1e-10, nk)
    assert (rc, info, err) == (0, p, 0.0) and not np.any(Cb.download())
    assert lk.kexpm(Cb, Aeng, B, tau, 1e-10, kdim=4, _basis=X) == p and Aeng.get_counter(False) == 0
    for which in ("zero column", "equal columns"):
        Bh = basis(n, p, dtype, 8)
        if which == "zero column":
            Bh[:, 1] = 0
        else:
            Bh[:, 2] = Bh[:, 0]
        B.upload(Bh)
        rc, info, err = _raw(Aeng, B, Cb, p, X, tau, 1e-10, nk)
        assert rc == 0 and info > 0, (which, rc, info)
        want = expm(tau * np.asarray(M)) @ Bh
        assert np.abs(Cb.download() - want).max() < lk.rtol_dp, which


def test_breakdown_on_an_invariant_subspace(ctx):
    """a diagonal operator with two distinct values per column's support: the block of p = 2 columns spans an invariant subspace of
    dimension 4 after one step -- the second step breaks down: err_est = 0, info = kp"""
    n, p = 64, 2
    d = np.where(np.arange(n) % 2 == 0, -1.0, -2.0)
    Bh = np.zeros((n, p), order="F")
    Bh[:4, 0] = 1.0                                    # four ones: norm 2, every operation of the factorisation is exact
    Bh[4:8, 1] = 1.0
    A = lk.diag_linop_gpu(d, ctx)
    hist = []
    Cr, info_r, err_r, _ = ref.kexpm_mat(ora.DiagOp(d), Bh, 1.0, 1e-12, 6, history=hist)
    B, Cb = lk.krylov_basis_gpu(n, p, np.float64, ctx), lk.krylov_basis_gpu(n, p, np.float64, ctx)
    B.upload(Bh)
    X = lk.krylov_basis_gpu(n, p * 7, np.float64, ctx)
    rc, info, err = _raw(A, B, Cb, p, X, 1.0, 1e-12, 6)
    assert rc == 0 and info == info_r == 4 and err == err_r == 0.0, (info, info_r, err, err_r, hist)
    assert np.abs(Cb.download() - np.exp(d)[:, None] * Bh).max() <= 1e-12


@pytest.mark.parametrize("dtype", KINDS, ids=["rdp", "cdp"])
def test_not_converged_repeated_calls_and_caller_memory(ctx, dtype):
    """two block steps are not enough: info = -1 and C is the restatement's two-step approximation; the same call twice on one
    workspace, wrapped with C inside larger live buffers, gives the same bits and touches nothing outside the panels"""
    n, p, nk = 301, 2, 2
    Aeng, Aref, tau = _operators("diag", n, dtype, ctx)
    Bh = basis(n, p, dtype, 4)
    Cr, info_r, err_r, _ = ref.kexpm_mat(Aref, Bh, tau, 1e-300, nk)
    assert info_r == -1
    B = lk.krylov_basis_gpu(n, p, dtype, ctx)
    B.upload(Bh)
    XP = CallerPanel(ctx, dtype, n, p * (nk + 1) + 1, "off48", seed=1)
    CP = CallerPanel(ctx, dtype, n, p, "nan_pad")
    outs = []
    for _ in range(2):
        rc, info, err = _raw(Aeng, B, CP.B, p, XP.B, tau, 1e-300, nk)
        assert rc == 0 and info == -1 and abs(err - err_r) <= max(1e-10 * err_r, 1e-14)
        outs.append(CP.get("kexpm_block C"))
        XP.get("kexpm_block X")
    assert np.array_equal(outs[0], outs[1])
    assert_columns_close(outs[0], Cr, "kexpm_block not converged")


def test_argument_errors_write_nothing(ctx):
    n, p, nk = 64, 2, 3
    A, _, tau = _operators("diag", n, np.float64, ctx)
    W = basis(n, 12, np.float64, 6)
    X = lk.krylov_basis_gpu(n, 12, np.float64, ctx)
    X.upload(W)
    B, Cb = lk.krylov_basis_gpu(n, p, np.float64, ctx), lk.krylov_basis_gpu(n, p, np.float64, ctx)
    Bh, Ch = basis(n, p, np.float64, 1), basis(n, p, np.float64, 2)
    B.upload(Bh)
    Cb.upload(Ch)
    other = lk.krylov_basis_gpu(n + 1, p, np.float64, ctx)
    cplx = lk.krylov_basis_gpu(n, p, np.complex128, ctx)
    bad = [dict(p=0), dict(nk=0), dict(nk=6), dict(jb0=1), dict(jc0=-1), dict(Cb=X), dict(B=X), dict(Cb=B), dict(B=other), dict(Cb=cplx)]
    for kw in bad:
        args = dict(A=A, B=B, Cb=Cb, p=p, X=X, tau=tau, tol=1e-9, nk=nk)
        args.update(kw)
        rc, info, err = _raw(**args)
        assert rc == -1 and info == -99 and err == -99.0, kw
    assert np.array_equal(X.download(), W) and np.array_equal(B.download(), Bh) and np.array_equal(Cb.download(), Ch)
    assert _raw(A, B.view(0, p), Cb, p, X, tau, 1e-9, nk)[0] == 0       # B in a workspace column the call does NOT write is fine
    Xb = X.view(8, p)                                                    # columns 8, 9 of X: behind the p (nk + 1) = 8 written ones
    X.upload(W)
    assert _raw(A, Xb, Cb, p, X, tau, 1e-9, nk)[0] == 0
    assert _raw(A, X.view(7, p), Cb, p, X, tau, 1e-9, nk)[0] == -1      # ... column 7 is written


def test_row_sharded_context_is_refused():
    lib = _capi.load()
    c2 = lk.Context(device=0)
    cb = _capi.ALLREDUCE_FN(lambda _u, _p, _n, _s: 0)
    n, p = 64, 2
    A = lk.diag_linop_gpu(n_local=n, row0=0, d0=-1.0, dstep=-0.01, ctx=c2)
    B, Cb = lk.krylov_basis_gpu(n, p, np.float64, c2), lk.krylov_basis_gpu(n, p, np.float64, c2)
    B.upload(basis(n, p, np.float64, 1))
    X = lk.krylov_basis_gpu(n, 8, np.float64, c2)
    _capi.check(lib.lk_set_allreduce(c2._h, cb, None, 2, 0))
    try:
        rc, _info, _err = _raw(A, B, Cb, p, X, 1.0, 1e-9, 3)
        assert rc == -1 and b"row-sharded" in lib.lk_last_error()
        assert not np.any(X.download())
    finally:
        _capi.check(lib.lk_set_allreduce(c2._h, _capi.ALLREDUCE_FN(), None, 1, 0))
    assert _raw(A, B, Cb, p, X, 1.0, 1e-9, 3)[0] == 0
    for o in (A, B, Cb, X):
        o.close()
    c2.close()
