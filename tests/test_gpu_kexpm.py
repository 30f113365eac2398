"""lk_kexpm / kexpm / krylov_exptA / exptA_linop: c = exp(tau A) b by Krylov projection as one engine call (ExpmLib.fypp:128-232, 365-392).

The comparison route is the package's own host loop (lightkrylov_amd/expm.py: `arnoldi` one step at a time, `expm`, one
`linear_combination`), which an operator that is not an engine operator takes: `_user_op` forwards to the engine operator and is
nothing else.  Both routes run the same Arnoldi kernels on the same data, so they may differ by the rounding of another summation
order only; the operators compared have ||exp(tau A)|| <= 1 (negative spectra), so no condition number enters:
||c_engine - c_host|| <= 1e-12 ||b||.  The tolerance of those runs is 1e-10: err_est falls by a factor of three or more per step there,
and the two routes' estimates agree to many digits, so both stop at the same step."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sla

import lightkrylov_amd as lk
from lightkrylov_amd import _capi
from tests._gpu_helpers import CallerPanel, seeded
from tests._tol import _report, assert_ritz_close

pytestmark = pytest.mark.gpu
KINDS = [np.float64, np.complex128]
TOL = 1e-10


class _user_op(lk.abstract_linop):
    """a user's operator around an engine operator: kexpm runs its host loop for it"""

    def __init__(self, A):
        super().__init__()
        self.A = A

    def matvec(self, vec_in, vec_out):
        self.A.matvec(vec_in, vec_out)

    def rmatvec(self, vec_in, vec_out):
        self.A.rmatvec(vec_in, vec_out)


def _raw(A, b, c, X, tau, tol, kdim, trans=False):
    """lk_kexpm itself: (return code, info, err_est)"""
    info, err = C.c_int(-99), C.c_double(-99.0)
    rc = X._lib.lk_kexpm(A._h, 1 if trans else 0, b.basis._h, b.col, c.basis._h, c.col, X._h, float(tau), float(tol), int(kdim),
                         C.byref(info), C.byref(err))
    return rc, info.value, err.value


def _operator(kind, n, ctx):
    """(engine operator with a spectrum on one side of zero, tau with tau * spectrum in about [-4, 0], dtype)"""
    if kind == "diag":                                  # generated diagonal: -0.05 - 2 i / n
        return lk.diag_linop_gpu(n_local=n, row0=0, d0=-0.05, dstep=-2.0 / n, ctx=ctx), 2.0, np.float64
    if kind == "cdiag":                                 # complex diagonal in the left half plane
        g = np.arange(n) / n
        return lk.diag_linop_gpu(((-0.05 - 2.0 * g) * np.exp(0.4j * g)).astype(np.complex128), ctx), 2.0, np.complex128
    N = int(round(np.sqrt(n)))                          # 5-point Laplacian (positive definite, norm < 8 (N+1)^2), negated through tau
    assert N * N == n
    return lk.laplacian2d_linop_gpu(N, ctx), -4.0 / (8.0 * (N + 1) ** 2), np.float64


# the vector-loop tails of the start kernel (k_axpby with the scale read on the device; n = 1, 2; 255, 257 either side of one block of 16-byte lanes; 1001 odd), 175 000 and 419^2 on the
# single-launch Gram-Schmidt route; the Laplacian needs squares
CASES = [("diag", n) for n in (1, 2, 255, 257, 1001, 175_000)] + [("lap5", n) for n in (1, 256, 419 * 419)] + [("cdiag", 1), ("cdiag", 129)]


def _ulps(got, ref):
    """entrywise distance in units of the last place of ref (per component for the complex kind)"""
    g, r = (np.ascontiguousarray(a).view(np.float64) for a in (got, ref))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(g == r, 0.0, np.abs(g - r) / np.spacing(np.abs(r)))


@pytest.mark.parametrize("kind,n", CASES, ids=[f"{k}-{n}" for k, n in CASES])
def test_engine_call_matches_host_loop(ctx, kind, n):
    A, tau, dtype = _operator(kind, n, ctx)
    kdim = 40
    bh = seeded(n, dtype, 11 + n % 97)
    b = lk.dense_vector_gpu.from_array(bh, ctx)
    ce, chost = lk.dense_vector_gpu(n, dtype, ctx), lk.dense_vector_gpu(n, dtype, ctx)
    X = lk.krylov_basis_gpu(n, kdim + 1, dtype, ctx)
    info_e = lk.kexpm(ce, A, b, tau, TOL, kdim=kdim, _basis=X)
    info_h = lk.kexpm(chost, _user_op(A), b, tau, TOL, kdim=kdim)
    assert info_e == info_h and 0 < info_e <= min(n, kdim) + 1, (info_e, info_h)
    bn = np.linalg.norm(bh)
    err = float(np.linalg.norm(ce.to_array() - chost.to_array()) / bn)
    _report(f"kexpm engine vs host loop {kind} n={n} (info {info_e})", err, 1e-12)
    print(f"{kind} n={n}: info {info_e}, |c_engine - c_host| / |b| = {err:.3e}")
    assert err <= 1e-12, err
    assert np.array_equal(b.to_array(), bh)                                   # b is read only
    # the start kernel entry by entry: X(:, 0) = b * (1 / |b|) with the norm the device computes (lk_vec_norm: the same kernels)
    x0 = X.download(0, 1)[:, 0]
    beta = b.norm()
    worst = float(_ulps(x0, bh / beta).max())
    _report(f"kexpm first Krylov vector {kind} n={n} [ulp]", worst, 2.0)
    assert worst <= 2.0, worst
    # ... and the panel is the Krylov basis of the steps the result used
    k = info_e
    Q = X.download(0, k)
    assert np.abs(Q.conj().T @ Q - np.eye(k)).max() <= 1e-12


@pytest.mark.parametrize("trans", [False, True], ids=["N", "H"])
@pytest.mark.parametrize("dtype", KINDS, ids=["rdp", "cdp"])
def test_reference_kexptA(ctx, dtype, trans):
    """test_kexptA of the reference (test/TestExpmlib.fypp:91-143): random dense operator, n = 128, tau = 0.1, kdim = 64, tol = rtol_dp,
    then krylov_exptA, each against the dense exponential at rtol_dp"""
    n, tau, nkmax = 128, 0.1, 64
    rng = np.random.default_rng(5)
    Ah = rng.standard_normal((n, n))
    qh = rng.standard_normal(n)
    if np.dtype(dtype).kind == "c":
        Ah = Ah + 1j * rng.standard_normal((n, n))
        qh = qh + 1j * rng.standard_normal(n)
    Ah = np.asfortranarray(Ah.astype(dtype))
    ref = sla.expm(tau * (Ah.conj().T if trans else Ah)) @ qh
    A = lk.dense_linop_gpu(Ah, ctx)
    q = lk.dense_vector_gpu.from_array(qh.astype(dtype), ctx)
    x = lk.dense_vector_gpu(n, dtype, ctx)
    info = lk.kexpm(x, A, q, tau, lk.rtol_dp, trans=trans, kdim=nkmax)
    err = float(np.linalg.norm(x.to_array() - ref) / np.linalg.norm(ref))
    _report(f"kexpm reference test {np.dtype(dtype).name} trans={trans} (info {info})", err, lk.rtol_dp)
    assert info > 0 and err < lk.rtol_dp, (info, err)
    assert A.get_counter(trans) == info - 1 and A.get_counter(not trans) == 0
    x.zero()
    info = lk.krylov_exptA(x, A, q, tau, trans=trans)
    err = float(np.linalg.norm(x.to_array() - ref) / np.linalg.norm(ref))
    _report(f"krylov_exptA reference test {np.dtype(dtype).name} trans={trans} (info {info})", err, lk.rtol_dp)
    assert info > 0 and err < lk.rtol_dp, (info, err)


@pytest.mark.parametrize("dtype", KINDS, ids=["rdp", "cdp"])
def test_zero_input(ctx, dtype):
    n = 1001
    A, tau, _ = _operator("cdiag" if np.dtype(dtype).kind == "c" else "diag", n, ctx)
    b = lk.dense_vector_gpu(n, dtype, ctx)
    b.zero()
    c = lk.dense_vector_gpu.from_array(seeded(n, dtype, 3), ctx)
    X = lk.krylov_basis_gpu(n, 11, dtype, ctx)
    rc, info, err = _raw(A, b, c, X, tau, TOL, 10)
    assert (rc, info, err) == (0, 1, 0.0)
    assert np.array_equal(c.to_array(), np.zeros(n, dtype=dtype))
    assert lk.kexpm(c, _user_op(A), b, tau, TOL, kdim=10) == 1


def test_breakdown_is_exact(ctx):
    """b in an invariant subspace of dimension 3: Arnoldi breaks down at step 3, kp = 3, err_est = 0, c = exp(tau d_i) b_i"""
    n, tau = 1001, 1.5
    d = np.linspace(-2.0, -0.05, n)
    A = lk.diag_linop_gpu(d, ctx)
    bh = np.zeros(n)
    bh[[3, 500, 998]] = [0.7, -1.1, 0.4]
    b = lk.dense_vector_gpu.from_array(bh, ctx)
    c = lk.dense_vector_gpu(n, np.float64, ctx)
    X = lk.krylov_basis_gpu(n, 21, np.float64, ctx)
    rc, info, err = _raw(A, b, c, X, tau, TOL, 20)
    assert (rc, info, err) == (0, 3, 0.0)
    dev = float(np.abs(c.to_array() - np.exp(tau * d) * bh).max() / np.linalg.norm(bh))
    _report("kexpm breakdown at step 3: closed form", dev, 1e-13)
    assert dev <= 1e-13, dev
    ch = lk.dense_vector_gpu(n, np.float64, ctx)
    assert lk.kexpm(ch, _user_op(A), b, tau, TOL, kdim=20) == 3


def test_not_converged_returns_the_kdim_step_approximation(ctx):
    """tau ||A|| = 50 and four steps: info = -1, c = the host loop's four-step approximation"""
    n, tau, kdim = 1001, 1.0, 4
    A = lk.diag_linop_gpu(n_local=n, row0=0, d0=-0.05, dstep=-50.0 / n, ctx=ctx)
    bh = seeded(n, np.float64, 21)
    b = lk.dense_vector_gpu.from_array(bh, ctx)
    ce, chost = lk.dense_vector_gpu(n, np.float64, ctx), lk.dense_vector_gpu(n, np.float64, ctx)
    X = lk.krylov_basis_gpu(n, kdim + 1, np.float64, ctx)
    rc, info, err = _raw(A, b, ce, X, tau, TOL, kdim)
    assert rc == 0 and info == -1 and err > TOL, (rc, info, err)
    assert lk.kexpm(chost, _user_op(A), b, tau, TOL, kdim=kdim) == -1
    dev = float(np.linalg.norm(ce.to_array() - chost.to_array()) / np.linalg.norm(bh))
    _report("kexpm not converged: four-step approximation vs host loop", dev, 1e-12)
    assert dev <= 1e-12 and np.linalg.norm(ce.to_array()) > 0.0, dev


def test_repeated_calls_on_one_workspace(ctx):
    """a time stepper's use: 50 calls on one workspace, bit-identical to calls on fresh workspaces; no device memory is allocated and the
    column pool is not touched"""
    import torch
    n, kdim, ncalls = 1001, 30, 50
    A, tau, _ = _operator("diag", n, ctx)
    lib = _capi.load()
    X = lk.krylov_basis_gpu(n, kdim + 1, np.float64, ctx)
    b = lk.dense_vector_gpu(n, np.float64, ctx)
    c = lk.dense_vector_gpu(n, np.float64, ctx)
    bs = [seeded(n, np.float64, 300 + i) * (1.0 + i) for i in range(ncalls)]

    def pool():
        st = (C.c_int64 * 4)()
        _capi.check(lib.lk_pool_stats(ctx._h, st))
        return list(st)

    b.basis.upload(bs[0].reshape(-1, 1))
    assert _raw(A, b, c, X, tau, TOL, kdim)[0] == 0                            # (first use sizes the engine's own step buffers)
    ctx.sync()
    pool0, free0 = pool(), torch.cuda.mem_get_info(ctx.device)[0]
    reused = []
    for i in range(ncalls):
        b.basis.upload(bs[i].reshape(-1, 1))
        reused.append(_raw(A, b, c, X, tau, TOL, kdim) + (c.to_array(),))
    ctx.sync()
    assert pool() == pool0
    assert torch.cuda.mem_get_info(ctx.device)[0] == free0
    for i in range(ncalls):
        b.basis.upload(bs[i].reshape(-1, 1))
        Xf = lk.krylov_basis_gpu(n, kdim + 1, np.float64, ctx)
        rc, info, err = _raw(A, b, c, Xf, tau, TOL, kdim)
        assert (rc, info, err) == reused[i][:3] and rc == 0 and info > 0, (i, rc, info, err, reused[i][:3])
        assert np.array_equal(c.to_array(), reused[i][3]), i


def test_argument_errors_write_nothing(ctx):
    n, kdim = 257, 8
    A, tau, _ = _operator("diag", n, ctx)
    Xh = np.asfortranarray(np.stack([seeded(n, np.float64, 40 + j) for j in range(kdim + 2)], axis=1))
    X = lk.krylov_basis_gpu(n, kdim + 2, np.float64, ctx)
    X.upload(Xh)
    bh, ch = seeded(n, np.float64, 60), seeded(n, np.float64, 61)
    b, c = lk.dense_vector_gpu.from_array(bh, ctx), lk.dense_vector_gpu.from_array(ch, ctx)
    lib = _capi.load()
    cases = [("c is a column of the workspace", (A, b, X[kdim + 1], X, tau, TOL, kdim)),
             ("c and b are the same column", (A, b, b, X, tau, TOL, kdim)),
             ("kdim", (A, b, c, X, tau, TOL, kdim + 2)),
             ("kdim", (A, b, c, X, tau, TOL, 0)),
             ("b is one of the workspace columns", (A, X[2], c, X, tau, TOL, kdim))]
    for what, args in cases:
        rc, info, err = _raw(*args)
        assert rc == -1 and what.encode() in lib.lk_last_error(), (what, rc, lib.lk_last_error())
        assert np.array_equal(X.download(), Xh) and np.array_equal(c.to_array(), ch) and np.array_equal(b.to_array(), bh), what
    with pytest.raises(_capi.LightKrylovHipError):
        lk.kexpm(X[kdim + 1], A, b, tau, TOL, kdim=kdim, _basis=X)
    # 513 steps: beyond what one asynchronous batch holds
    assert _raw(A, b, c, lk.krylov_basis_gpu(n, 515, np.float64, ctx), tau, TOL, 513)[0] == -1
    # b in a column of X the call does not write is fine
    assert _raw(A, X[kdim + 1], c, X, tau, TOL, kdim)[0] == 0


def test_row_sharded_context_is_refused():
    lib = _capi.load()
    c2 = lk.Context(device=0)
    cb = _capi.ALLREDUCE_FN(lambda _u, _p, _n, _s: 0)
    n = 64
    A = lk.diag_linop_gpu(n_local=n, row0=0, d0=-1.0, dstep=-0.01, ctx=c2)
    b = lk.dense_vector_gpu.from_array(seeded(n, np.float64, 1), c2)
    c = lk.dense_vector_gpu(n, np.float64, c2)
    X = lk.krylov_basis_gpu(n, 9, np.float64, c2)
    _capi.check(lib.lk_set_allreduce(c2._h, cb, None, 2, 0))
    try:
        rc, _info, _err = _raw(A, b, c, X, 1.0, TOL, 8)
        assert rc == -1 and b"row-sharded" in lib.lk_last_error()
        assert np.array_equal(X.download(), np.zeros((n, 9)))
    finally:
        _capi.check(lib.lk_set_allreduce(c2._h, _capi.ALLREDUCE_FN(), None, 1, 0))
    assert _raw(A, b, c, X, 1.0, TOL, 8)[0] == 0
    for o in (A, b.basis, c.basis, X):
        o.close()
    c2.close()


@pytest.mark.parametrize("dtype", KINDS, ids=["rdp", "cdp"])
def test_caller_owned_workspace_with_live_padding(ctx, dtype):
    """X and c wrapped inside larger buffers whose other rows are live: rows [n_local, ld) and everything around the panels keep
    their bits (CallerPanel.get asserts it), and the result is the one of engine-owned panels (to rounding: the sweeps may split their
    rows differently on a panel with another alignment)"""
    n, kdim = 257, 24
    A, tau, _ = _operator("cdiag" if np.dtype(dtype).kind == "c" else "diag", n, ctx)
    bh = seeded(n, dtype, 77)
    b = lk.dense_vector_gpu.from_array(bh, ctx)
    PX = CallerPanel(ctx, dtype, n, kdim + 1, "off48", seed=1)
    PC = CallerPanel(ctx, dtype, n, 2, "off240", seed=2)
    rc, info, err = _raw(A, b, PC.B[1], PX.B, tau, TOL, kdim)
    assert rc == 0 and info > 0
    got_c = PC.get("lk_kexpm(c)")[:, 1]
    x0 = PX.get("lk_kexpm(X)")[:, 0]
    c = lk.dense_vector_gpu(n, dtype, ctx)
    X = lk.krylov_basis_gpu(n, kdim + 1, dtype, ctx)
    assert _raw(A, b, c, X, tau, TOL, kdim)[:2] == (rc, info)
    assert np.linalg.norm(got_c - c.to_array()) <= 1e-12 * np.linalg.norm(bh)
    assert float(_ulps(x0, bh / b.norm()).max()) <= 2.0


def test_exptA_linop_in_eigs(ctx):
    """eigs on the propagator exp(tau D): the leading Ritz values are exp(tau d_i).  The propagator is normal (diagonal), so the
    suite's Ritz bound is the bare 1e-12 ||exp(tau D)||_2"""
    n, nev, tau = 1000, 4, 1.0
    d = -2.5 - 1.5 * np.arange(n) / n
    d[:nev] = [0.0, -0.4, -0.8, -1.2]
    P = lk.exptA_linop(lk.diag_linop_gpu(d, ctx), tau)
    X = lk.krylov_basis_gpu(n, nev, np.float64, ctx)
    x0 = lk.dense_vector_gpu.from_array(seeded(n, np.float64, 9), ctx)
    vals, res, info = lk.eigs(P, X, x0=x0, kdim=30, tolerance=1e-10)
    assert P.matvec_counter > 0 and P.info != 0
    # (the bound's matrix: the leading 4 x 4 block of the propagator -- same norm, 1, and the same unit condition numbers as the whole)
    assert_ritz_close(vals, np.exp(tau * d[:nev]), np.diag(np.exp(tau * d[:nev])), "eigs on exptA_linop(diag, tau = 1), nev = 4")
