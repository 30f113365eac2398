"""lk_cg, conjugate gradient as one asynchronous engine call (CG.fypp:60-196), on the device.

Parity at solver level against the oracle's cg, the longdouble restatement of tests/_cg_cases.py and the package's host loop; the three new
passes (cg_update, cg_scalars, cg_direction, run inside k_axpby's symbol) at the loop edges and cache-policy sizes of the BLAS-1 grid, both kinds; exactness of
the stop (nothing of iteration i + 1 runs after a stop in iteration i); the deliveries around the look-ahead depth; the start residual
(no product for x = 0, the zero residual); non-finite input; every refusal of the contract; views of caller-owned panels; the Python
keyword.  The inputs are pinned without a GPU in tests/test_cg_host_logic.py."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import lightkrylov_amd as lk
from lightkrylov_amd import _capi
from oracle import oracle as ora
from tests import _cg_cases as cases
from tests._blas1_cases import DEFAULT_MULT
from tests._gpu_helpers import KINDS, CallerPanel, _sharded, basis, device_num_cu, is_cplx, seeded
from tests._tol import assert_close

pytestmark = pytest.mark.gpu

SENTINEL = -7.0


def _name(dtype):
    return np.dtype(dtype).name


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class _Out:
    def __init__(self, rc, info, nres, res, raw):
        self.rc, self.info, self.nres, self.res, self.raw = rc, info, nres, res, raw


def _cg(A, M, b, x, W, rtol, atol, maxiter, res=True, cap=None, counts=True):
    """lk_cg itself; b and x are vectors (basis, column), W a basis.  The history buffer has 4 sentinel entries behind its capacity."""
    cap = maxiter + 1 if cap is None else cap
    raw = np.full(cap + 4, SENTINEL)
    nres, info = C.c_int64(-99), C.c_int(-99)
    rc = _capi.load().lk_cg(A._h if A is not None else None, M._h if M is not None else None, b.basis._h, b.col, x.basis._h, x.col,
                            W._h if W is not None else None, float(rtol), float(atol), maxiter,
                            raw.ctypes.data_as(C.POINTER(C.c_double)) if res else None, cap if res else 0,
                            C.byref(nres) if counts else None, C.byref(info))
    hist = None
    if res and rc == 0 and counts:
        k = min(nres.value, cap)
        assert np.all(raw[k:] == SENTINEL), "lk_cg wrote behind the entries it reported"
        hist = raw[:k].copy()
    return _Out(rc, info.value, nres.value, hist, raw)


def _solve(ctx, A, M, bh, x0h, rtol, atol, maxiter, ncols=None, **kw):
    """b, x and W each in a basis of its own; returns (out, x, W contents)"""
    b, x = lk.dense_vector_gpu.from_array(bh, ctx), lk.dense_vector_gpu.from_array(x0h, ctx)
    W = lk.krylov_basis_gpu(bh.size, ncols or (4 if M is not None else 3), bh.dtype, ctx)
    W.upload(np.zeros((bh.size, W.ncols), dtype=bh.dtype))
    out = _cg(A, M, b, x, W, rtol, atol, maxiter, **kw)
    return out, x.to_array(), W.download()


@contextlib.contextmanager
def _tuned(c, **keys):
    try:
        for k, v in keys.items():
            c.set_tuning(k, v)
        yield c
    finally:
        c.set_tuning("blas1_grid_mult", DEFAULT_MULT)


# ---- parity at solver level -------------------------------------------------------------------------------------------------------------------

def _check_parity(label, out, x, A, bh, info_ref, res_ref, x_ref):
    res_ref, x_ref = np.asarray(res_ref, dtype=np.float64), np.asarray(x_ref).astype(bh.dtype)
    assert out.rc == 0 and out.info == info_ref > 0 and out.nres == len(res_ref) == len(out.res), f"{label}: {out.rc}, {out.info}, {out.nres}"
    eh, ex = np.abs(out.res - res_ref).max() / res_ref[0], np.abs(x - x_ref).max() / res_ref[0]
    er = np.abs(A @ x - bh).max() / np.abs(bh).max()
    print(f"{label}: info {out.info}, |d history| / res[0] = {eh:.2e}, |dx| / res[0] = {ex:.2e}, |Ax - b| / |b| = {er:.2e}")
    assert eh <= 1e-9 and ex <= 1e-9, label        # the project's cg bound (tests/test_gpu_solvers.py::test_cg_against_oracle)
    assert er <= 1e-8, label


def test_dense_spd_against_the_oracle(ctx):
    A, bh, _m, rtol, info_l, res_l, x_l, _r, _p = cases.parity_reference("dense_spd")
    A, bh = np.array(A), np.array(bh)
    xo = np.zeros(bh.size)
    info_o, res_o = ora.cg(ora.DenseOp(A), bh, xo, rtol=rtol, atol=cases.ATOL, maxiter=cases.MAXITER)
    Aop = lk.dense_linop_gpu(A, ctx)
    out, x, _W = _solve(ctx, Aop, None, bh, np.zeros_like(bh), rtol, cases.ATOL, cases.MAXITER)
    _check_parity("lk_cg dense SPD against the oracle", out, x, A, bh, info_o, res_o, xo)
    _check_parity("lk_cg dense SPD against the restatement", out, x, A, bh, info_l, res_l, x_l)
    # a warm start from a perturbed solution: the product for the start residual runs, and res[0] is ||b - A x0||
    x0 = x + 1e-3 * seeded(bh.size, np.float64, 77)
    out2, x2, _W = _solve(ctx, Aop, None, bh, x0, rtol, cases.ATOL, cases.MAXITER)
    assert out2.rc == 0 and out2.info > 0 and np.abs(A @ x2 - bh).max() <= 1e-8 * np.abs(bh).max()
    assert abs(out2.res[0] - np.linalg.norm(bh - A @ x0)) <= 1e-12 * out.res[0]


def test_hermitian_pd_against_the_restatement(ctx):
    A, bh, _m, rtol, info_l, res_l, x_l, _r, _p = cases.parity_reference("hermitian_pd")
    A, bh = np.array(A), np.array(bh)
    Aop = lk.dense_linop_gpu(A, ctx)
    out, x, _W = _solve(ctx, Aop, None, bh, np.zeros_like(bh), rtol, cases.ATOL, cases.MAXITER)
    _check_parity("lk_cg Hermitian PD against the restatement", out, x, A, bh, info_l, res_l, x_l)


def test_jacobi_on_a_diagonal_of_three_decades(ctx):
    A, bh, m, rtol, info_l, res_l, x_l, _r, _p = cases.parity_reference("three_decades_jacobi")
    A, bh, m = np.array(A), np.array(bh), np.array(m)
    Aop, Mop = lk.dense_linop_gpu(A, ctx), lk.diag_linop_gpu(m, ctx)
    out, x, _W = _solve(ctx, Aop, Mop, bh, np.zeros_like(bh), rtol, cases.ATOL, cases.MAXITER)
    _check_parity("lk_cg Jacobi against the restatement", out, x, A, bh, info_l, res_l, x_l)
    # the package's host loop with the same linop_precond_gpu
    b, xh, meta = lk.dense_vector_gpu.from_array(bh, ctx), lk.dense_vector_gpu.from_array(np.zeros_like(bh), ctx), lk.cg_dp_metadata()
    info_h = lk.cg(Aop, b, xh, rtol=rtol, atol=cases.ATOL, preconditioner=lk.linop_precond_gpu(Mop), options=lk.cg_dp_opts(maxiter=cases.MAXITER),
                   meta=meta, engine=False)
    _check_parity("lk_cg Jacobi against the host loop", out, x, A, bh, info_h, meta.res, xh.to_array())
    # fewer iterations than without M
    plain, _x, _W = _solve(ctx, Aop, None, bh, np.zeros_like(bh), rtol, cases.ATOL, cases.UNPRECONDITIONED_MAXITER)
    assert plain.rc == 0 and abs(plain.info) > out.info, (plain.info, out.info)


# ---- kernel edges -----------------------------------------------------------------------------------------------------------------------------

def _run_edge(c, n, dtype, precond):
    d, bh = cases.edge_problem(n, dtype)
    maxiter = cases.EDGE_MAXITER if n > max(cases.SMALL_N) else 1     # CG on n unknowns ends in n iterations: beyond them it divides rounding noise
    one = np.ones(n, dtype=dtype)
    info, res, xl, rl, pl = cases.cg_long(cases.diagop(d), bh, np.zeros(n, dtype=dtype), 0.0, 0.0, maxiter, cases.diagop(one) if precond else None)
    out, x, W = _solve(c, lk.diag_linop_gpu(d, c), lk.diag_linop_gpu(one, c) if precond else None, bh, np.zeros(n, dtype=dtype), 0.0, 0.0, maxiter)
    label = f"lk_cg edges n={n} {_name(dtype)}{' with M' if precond else ''}"
    assert out.rc == 0 and out.info == info == -maxiter and out.nres == maxiter + 1, f"{label}: rc {out.rc}, info {out.info}, nres {out.nres}"
    worst = assert_close(out.res, res.astype(np.float64), label + " [history]")
    for got, ref, what in ((x, xl, "x"), (W[:, 0], rl, "r"), (W[:, 1], pl, "p")):
        worst = max(worst, assert_close(got, ref.astype(dtype), f"{label} [{what}]"))
    return worst


@pytest.mark.parametrize("precond", [False, True], ids=["noM", "M"])
@pytest.mark.parametrize("dtype", KINDS)
def test_kernels_at_the_loop_edges(dtype, precond):
    """cg_update (with and without the r.r sums), cg_scalars and cg_direction at "blas1_grid_mult" = 1 over the loop edges of the
    BLAS-1 grid and n = 1, 2, 3; with M = I (an operator kernel and k_dot between update and scalars) at the deepest size and the small ones"""
    c = lk.Context(device=0)
    try:
        with _tuned(c, blas1_grid_mult=1):
            sizes = cases.loop_edge_sizes(device_num_cu(c), dtype)
            if precond:
                sizes = cases.SMALL_N + sizes[-2:]
            worst = max(_run_edge(c, n, dtype, precond) for n in sizes)
        print(f"lk_cg loop edges {_name(dtype)}: worst normwise difference {worst:.2e}")
    finally:
        c.close()


@pytest.mark.parametrize("which", [0, 1, 2], ids=["last_plain", "first_non_temporal", "non_temporal_odd"])
@pytest.mark.parametrize("dtype", KINDS)
def test_kernels_at_the_cache_policy_sizes(ctx, dtype, which):
    sizes, mult = cases.policy_sizes(dtype)
    with _tuned(ctx, blas1_grid_mult=mult):
        _run_edge(ctx, sizes[which], dtype, False)


# ---- stop exactness ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precond", [False, True], ids=["noM", "M"])
@pytest.mark.parametrize("dtype", KINDS)
def test_nothing_runs_behind_the_iteration_that_stops(ctx, dtype, precond):
    """a solve that converges at iteration k (look-ahead launches of up to 24 iterations in flight behind it) leaves x, r and p bit for
    bit as a solve with maxiter = k does, which enqueues nothing behind iteration k but its direction update"""
    d, bh, rtol = cases.stop_problem(dtype)
    A = lk.diag_linop_gpu(d, ctx)
    M = lk.diag_linop_gpu(cases.stop_precond(dtype), ctx) if precond else None
    free, xf, Wf = _solve(ctx, A, M, bh, np.zeros_like(bh), rtol, 0.0, 100)
    k = free.info
    assert free.rc == 0 and 5 <= k <= 15 and free.nres == k + 1, (free.rc, k)
    cut, xc, Wc = _solve(ctx, A, M, bh, np.zeros_like(bh), rtol, 0.0, k)
    assert cut.rc == 0 and cut.info == k and _same_bits(cut.res, free.res)
    assert _same_bits(xf, xc), f"x differs by {np.abs(xf - xc).max():.2e}"
    assert _same_bits(Wf[:, 0], Wc[:, 0]) and _same_bits(Wf[:, 1], Wc[:, 1]), "r or p changed behind the stop"
    # and one iteration fewer does NOT stop there: its direction update has run
    short, _xs, Ws = _solve(ctx, A, M, bh, np.zeros_like(bh), rtol, 0.0, k - 1)
    assert short.info == -(k - 1) and _same_bits(short.res, free.res[:k])


# ---- deliveries -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", KINDS)
def test_deliveries_around_the_look_ahead_depth(ctx, dtype):
    n = 1031
    d = (1.0 + 3.0 * seeded(n, np.float64, 41) ** 2).astype(dtype)
    bh = seeded(n, dtype, 42)
    A = lk.diag_linop_gpu(d, ctx)
    runs = {m: _solve(ctx, A, None, bh, np.zeros_like(bh), 0.0, 0.0, m)[0] for m in cases.DELIVERY_MAXITER}
    longest = runs[max(runs)]
    for m, out in runs.items():
        assert out.rc == 0 and out.nres == m + 1 and out.info == -m, (m, out.rc, out.nres, out.info)
        assert _same_bits(out.res, longest.res[:m + 1]), f"maxiter = {m}: the history is no prefix of the longest"
    m = 25
    for cap in (0, 1, 7, 25):
        out = _solve(ctx, A, None, bh, np.zeros_like(bh), 0.0, 0.0, m, cap=cap)[0]     # (_cg asserts the sentinels behind `cap`)
        assert out.rc == 0 and out.nres == m + 1 and out.info == -m and _same_bits(out.res, longest.res[:cap])
    out = _solve(ctx, A, None, bh, np.zeros_like(bh), 0.0, 0.0, m, res=False)[0]
    assert out.rc == 0 and out.nres == m + 1 and out.info == -m and np.all(out.raw == SENTINEL)
    out = _solve(ctx, A, None, bh, np.zeros_like(bh), 0.0, 0.0, m, res=False, counts=False)[0]
    assert out.rc == 0 and out.info == -m and out.nres == -99


# ---- start ------------------------------------------------------------------------------------------------------------------------------------

def _matvecs(c, A, bh, x0h, maxiter):
    c.profile_enable(True)
    c.profile_reset()
    try:
        out = _solve(c, A, None, bh, x0h, 0.0, 0.0, maxiter)[0]
        c.sync()
        return out, c.profile_get("matvec")[0], c.profile_get("blas1")[0]
    finally:
        c.profile_enable(False)


@pytest.mark.parametrize("dtype", KINDS)
def test_a_zero_guess_costs_no_product(dtype):
    n, maxiter = 777, 5
    d, bh = cases.edge_problem(n, dtype)
    c = lk.Context(device=0)
    try:
        A = lk.diag_linop_gpu(d, c)
        out, mv, _b1 = _matvecs(c, A, bh, np.zeros(n, dtype=dtype), maxiter)
        assert out.rc == 0 and out.info == -maxiter and mv == maxiter, (out.info, mv)
        out, mv, _b1 = _matvecs(c, A, bh, 0.5 * seeded(n, dtype, 9), maxiter)
        assert out.rc == 0 and out.info == -maxiter and mv == maxiter + 1, (out.info, mv)
    finally:
        c.close()


@pytest.mark.parametrize("precond", [False, True], ids=["noM", "M"])
@pytest.mark.parametrize("dtype", KINDS)
def test_a_zero_start_residual_and_maxiter_zero(ctx, dtype, precond):
    n = 257
    d = (2.0 ** (np.arange(n) % 4)).astype(dtype)                       # powers of two: d * x is exact
    x0h = (seeded(n, dtype, 5) * 1024).round() / 1024
    bh = d * x0h
    A = lk.diag_linop_gpu(d, ctx)
    M = lk.diag_linop_gpu(1.0 / d, ctx) if precond else None
    for what, b_, x_ in (("the exact solution as x", bh, x0h), ("b = 0, x = 0", np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype))):
        out, x, _W = _solve(ctx, A, M, b_, x_, 1e-10, 0.0, 30)
        assert out.rc == 0 and (out.info, out.nres) == (0, 1) and list(out.res) == [0.0], f"{what}: {out.rc}, {out.info}, {out.nres}, {out.res}"
        assert _same_bits(x, x_), what
    out, x, _W = _solve(ctx, A, M, bh, np.zeros(n, dtype=dtype), 1e-10, 0.0, 0)
    assert out.rc == 0 and (out.info, out.nres) == (0, 1) and not np.any(x)
    assert_close(out.res, [np.sqrt(abs(np.vdot(bh, bh / d if precond else bh)))], "maxiter = 0 [res[0]]")
    # a start residual below tol that is not zero still takes one iteration
    out, x, _W = _solve(ctx, A, M, bh, np.zeros(n, dtype=dtype), 10.0, 0.0, 30)
    assert out.rc == 0 and (out.info, out.nres) == (1, 2)


# ---- non-finite input -------------------------------------------------------------------------------------------------------------------------

def _context_still_works(c, dtype, label):
    """lk_vec_axpby and an lk_arnoldi of 4 steps against the oracle on the same context: the stop flag and the guard are down"""
    n, m = 513, 4
    xh, yh = seeded(n, dtype, 61), seeded(n, dtype, 62)
    x, y = lk.dense_vector_gpu.from_array(xh, c), lk.dense_vector_gpu.from_array(yh, c)
    y.axpby(0.5, x, 2.0)
    assert_close(y.to_array(), 0.5 * xh + 2.0 * yh, label + " [axpby afterwards]")
    d = (1.0 + np.arange(n) / n).astype(dtype)
    x0 = seeded(n, dtype, 63)
    x0 /= np.linalg.norm(x0)
    X = lk.krylov_basis_gpu(n, m + 1, dtype, c)
    X.upload(x0.reshape(-1, 1), 0)
    H = np.zeros((m + 1, m), dtype=dtype, order="F")
    info = lk.arnoldi(lk.diag_linop_gpu(d, c), X, H)
    Xo = np.zeros((n, m + 1), dtype=dtype, order="F")
    Xo[:, 0] = x0
    Ho = np.zeros((m + 1, m), dtype=dtype, order="F")
    info_o = ora.arnoldi(ora.DiagOp(d), Xo, Ho)
    assert info == info_o == 0, label
    assert_close(H, Ho, label + " [arnoldi afterwards]")
    assert_close(X.download(), Xo, label + " [basis afterwards]")


@pytest.mark.parametrize("dtype", KINDS)
def test_non_finite_input_ends_in_lk_err_nan_and_the_context_works_on(dtype):
    n = 600
    c = lk.Context(device=0)
    try:
        d, bh = cases.edge_problem(n, dtype)
        bad = bh.copy()
        bad[n // 2] = np.nan
        out, _x, _W = _solve(c, lk.diag_linop_gpu(d, c), None, bad, np.zeros(n, dtype=dtype), 1e-10, 0.0, 30)
        assert out.rc == -5, out.rc                                     # LK_ERR_NAN
        _context_still_works(c, dtype, f"after a NaN in b {_name(dtype)}")
        # p . Ap = 0 in the first iteration: d = (1, -1, 1, -1, ...), b = 1
        alt = np.where(np.arange(n) % 2 == 0, 1.0, -1.0).astype(dtype)
        out, x, _W = _solve(c, lk.diag_linop_gpu(alt, c), None, np.ones(n, dtype=dtype), np.zeros(n, dtype=dtype), 1e-10, 0.0, 30)
        assert out.rc == -5, out.rc
        assert not np.any(x), "the iteration that met p.Ap = 0 wrote x"
        _context_still_works(c, dtype, f"after p.Ap = 0 {_name(dtype)}")
        # and after a solve that converged early, its look-ahead launches drained
        ds, bs, rtol = cases.stop_problem(dtype)
        out, _x, _W = _solve(c, lk.diag_linop_gpu(ds, c), None, bs, np.zeros_like(bs), rtol, 0.0, 100)
        assert out.rc == 0 and 5 <= out.info <= 15
        _context_still_works(c, dtype, f"after an early stop {_name(dtype)}")
    finally:
        c.close()


@pytest.mark.parametrize("dtype", KINDS)
def test_a_residual_that_overflows_on_the_device_is_lk_err_nan(dtype):
    """finite b and x, a finite p.Ap, and a rho' that is not: A = I with A[0, 1] = 1e200 (not symmetric: the call does not check) and
    b = (0, 1, ..., 1) give p.Ap = rho, alpha = 1 and r[0] = -1e200 in the first iteration, so rho' overflows and the scalars pass raises the
    flag on it.  And a start residual that is not finite with ||b|| and ||x|| finite: d = 1e300, x = 1e10, so A x overflows."""
    from tests._gpu_helpers import last_error
    n = 8
    c = lk.Context(device=0)
    try:
        A = np.eye(n, dtype=dtype, order="F")
        A[0, 1] = 1e200
        bh = np.ones(n, dtype=dtype)
        bh[0] = 0.0
        out, _x, _W = _solve(c, lk.dense_linop_gpu(A, c), None, bh, np.zeros(n, dtype=dtype), 1e-10, 0.0, 30)
        assert out.rc == -5 and "residual of iteration 1 is not finite" in last_error(), (out.rc, last_error())
        _context_still_works(c, dtype, f"after an overflowing residual {_name(dtype)}")
        d = np.full(n, 1e300, dtype=dtype)
        out, _x, _W = _solve(c, lk.diag_linop_gpu(d, c), None, np.ones(n, dtype=dtype), np.full(n, 1e10, dtype=dtype), 1e-10, 0.0, 30)
        assert out.rc == -5 and "start residual is not finite" in last_error(), (out.rc, last_error())
        _context_still_works(c, dtype, f"after an overflowing start residual {_name(dtype)}")
    finally:
        c.close()


# ---- contract ---------------------------------------------------------------------------------------------------------------------------------

def _refused(label, P, img, call):
    out = call()
    assert out.rc == -1 and out.info == -99 and out.nres == -99 and np.all(out.raw == SENTINEL), f"{label}: rc {out.rc}, info {out.info}"
    assert _same_bits(P.download(), np.asfortranarray(img)), f"{label}: something was written"


@pytest.mark.parametrize("dtype", KINDS)
def test_every_refusal_writes_nothing(ctx, dtype):
    """x = column 6, b = column 7, W = a view of columns [1, 1 + w) of one panel P of 8 columns; each refusal of the header, one case each"""
    n = 300
    other = np.complex128 if dtype is np.float64 else np.float64
    d, _b = cases.edge_problem(n, dtype)
    A, M = lk.diag_linop_gpu(d, ctx), lk.diag_linop_gpu(1.0 / d, ctx)
    img = basis(n, 8, dtype, 700)
    P = lk.krylov_basis_gpu(n, 8, dtype, ctx)
    P.upload(img)
    W3, W4, W2 = P.view(1, 3), P.view(1, 4), P.view(1, 2)
    x, b = P[6], P[7]
    ok = dict(rtol=1e-10, atol=0.0, maxiter=10)
    A_short = lk.diag_linop_gpu(d[:n - 1], ctx)
    A_kind = lk.diag_linop_gpu(d.real.astype(other), ctx)
    Pk = lk.krylov_basis_gpu(n, 4, other, ctx)
    Ps = lk.krylov_basis_gpu(n - 1, 4, dtype, ctx)
    c2 = lk.Context(device=0)
    try:
        A_ctx, P_ctx = lk.diag_linop_gpu(d, c2), lk.krylov_basis_gpu(n, 4, dtype, c2)
        lib = _capi.load()
        null_info = lambda: _Out(lib.lk_cg(A._h, None, b.basis._h, b.col, x.basis._h, x.col, W3._h, 1e-10, 0.0, 10, None, 0, None, None),
                                 -99, -99, None, np.full(1, SENTINEL))
        refusals = {
            "null A": lambda: _cg(None, None, b, x, W3, **ok),
            "null W": lambda: _cg(A, None, b, x, None, **ok),
            "null info": null_info,
            "maxiter < 0": lambda: _cg(A, None, b, x, W3, 1e-10, 0.0, -1, cap=4),
            "W too narrow": lambda: _cg(A, None, b, x, W2, **ok),
            "W too narrow with M": lambda: _cg(A, M, b, x, W3, **ok),
            "x a written column of W": lambda: _cg(A, None, b, P[3], W3, **ok),
            "x the z column with M": lambda: _cg(A, M, b, P[4], W4, **ok),
            "b a written column of W": lambda: _cg(A, None, P[1], x, W3, **ok),
            "x and b the same column": lambda: _cg(A, None, x, x, W3, **ok),
            "operator of another size": lambda: _cg(A_short, None, b, x, W3, **ok),
            "operator of another kind": lambda: _cg(A_kind, None, b, x, W3, **ok),
            "operator of another context": lambda: _cg(A_ctx, None, b, x, W3, **ok),
            "preconditioner of another size": lambda: _cg(A, A_short, b, x, W4, **ok),
            "workspace of another kind": lambda: _cg(A, None, b, x, Pk, **ok),
            "workspace of another size": lambda: _cg(A, None, b, x, Ps, **ok),
            "workspace of another context": lambda: _cg(A, None, b, x, P_ctx, **ok),
        }
        for what, call in refusals.items():
            _refused(f"lk_cg {what} {_name(dtype)}", P, img, call)
        # x in the column behind the written ones is legal without M
        out = _cg(A, None, b, P[4], W3, **ok)
        assert out.rc == 0
    finally:
        c2.close()


def test_row_sharded_context_is_refused():
    n = 4099
    d = 2.0 + np.arange(n) % 5
    bh = seeded(n, np.float64, 17)

    def body(rank, c, row0, nl):
        A = lk.diag_linop_gpu(d[row0:row0 + nl], c)
        b = lk.dense_vector_gpu.from_array(bh[row0:row0 + nl], c)
        x = lk.dense_vector_gpu.from_array(np.zeros(nl), c)
        W = lk.krylov_basis_gpu(nl, 3, np.float64, c)
        img = basis(nl, 3, np.float64, 800 + rank)
        W.upload(img)
        out = _cg(A, None, b, x, W, 1e-10, 0.0, 10)
        refused = out.rc == -1 and out.info == -99 and not np.any(x.to_array()) and _same_bits(W.download(), img)
        try:
            lk.cg(A, b, x, engine=True)
            raised = False
        except TypeError:
            raised = True
        return refused, raised

    out, _grp = _sharded(n, 2, body)
    assert all(o[0] and o[1] for o in out), out


# ---- views ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precond", [False, True], ids=["noM", "M"])
@pytest.mark.parametrize("dtype", KINDS)
def test_views_of_caller_owned_panels(ctx, dtype, precond):
    """x and b views (lk_basis_wrap at a column address) of two caller-owned panels with live padding rows, W a view of a third: padding
    and neighbouring columns bit-unchanged, results bit for bit those on owned bases"""
    d, bh, rtol = cases.stop_problem(dtype, n=1023 if is_cplx(dtype) else 1022)
    n, ncw = bh.size, 4 if precond else 3
    A = lk.diag_linop_gpu(d, ctx)
    M = lk.diag_linop_gpu(cases.stop_precond(dtype, n), ctx) if precond else None
    plain, x_plain, W_plain = _solve(ctx, A, M, bh, np.zeros_like(bh), rtol, 0.0, 100)
    assert plain.rc == 0 and plain.info > 0
    px, pb, pw = (CallerPanel(ctx, dtype, n, k, layout, seed=s) for k, layout, s in ((3, "off48", 1), (3, "nan_pad", 2), (ncw + 2, "off16", 3)))
    ix, ib, iw = basis(n, 3, dtype, 910), basis(n, 3, dtype, 920), basis(n, ncw + 2, dtype, 930)
    ix[:, 1], ib[:, 1] = 0.0, bh
    px.set(ix); pb.set(ib); pw.set(iw)
    xv, bv, Wv = px.B.view(1, 1), pb.B.view(1, 1), pw.B.view(1, ncw)
    out = _cg(A, M, bv[0], xv[0], Wv, rtol, 0.0, 100)
    label = f"lk_cg on views {_name(dtype)}"
    assert out.rc == 0 and out.info == plain.info and _same_bits(out.res, plain.res), label
    gx, gb, gw = px.get(label + " x"), pb.get(label + " b"), pw.get(label + " W")          # (asserts the padding)
    assert _same_bits(gx[:, 1], x_plain) and _same_bits(gx[:, [0, 2]], np.asfortranarray(ix[:, [0, 2]])), label
    assert _same_bits(gb, np.asfortranarray(ib)), label
    assert _same_bits(gw[:, 1:1 + ncw], W_plain) and _same_bits(gw[:, [0, ncw + 1]], np.asfortranarray(iw[:, [0, ncw + 1]])), label


# ---- Python -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", KINDS)
def test_the_engine_keyword(dtype):
    d, bh, rtol = cases.stop_problem(dtype)
    n = bh.size
    c = lk.Context(device=0)
    try:
        A = lk.diag_linop_gpu(d, c)
        b = lk.dense_vector_gpu.from_array(bh, c)

        def run(rtol=rtol, maxiter=100, **kw):
            x, meta = lk.dense_vector_gpu.from_array(np.zeros(n, dtype=dtype), c), lk.cg_dp_metadata()
            c.profile_enable(True)
            c.profile_reset()
            info = lk.cg(A, b, x, rtol=rtol, atol=0.0, options=lk.cg_dp_opts(maxiter=maxiter), meta=meta, **kw)
            c.sync()
            blas1 = c.profile_get("blas1")[0]
            c.profile_enable(False)
            return info, meta, x.to_array(), blas1

        info_e, meta_e, x_e, n_e = run(engine=True)
        info_a, meta_a, x_a, n_a = run()
        info_n, meta_n, x_n, n_n = run(engine=None)
        info_f, meta_f, x_f, n_f = run(engine=False)
        assert info_e == meta_e.info == meta_e.n_iter > 0 and meta_e.converged and len(meta_e.res) == info_e + 1
        # None and False run the host loop: the same launches and the same bits as a call without the keyword
        assert info_a == info_n == info_f == info_e and n_a == n_n == n_f
        assert _same_bits(x_a, x_n) and _same_bits(x_a, x_f) and meta_a.res == meta_n.res == meta_f.res
        # the host loop launches 2 dots + 3 axpbys = 5 "blas1" kernels per iteration and nothing else under that tag: one iteration more
        # (tolerance out of reach) costs exactly 5, with the keyword absent, None and False.  lk_cg's iteration is dot, update, scalars,
        # direction = 4, so a call routed through it would show
        for kw in ({}, {"engine": None}, {"engine": False}):
            per_iteration = run(rtol=0.0, maxiter=4, **kw)[3] - run(rtol=0.0, maxiter=3, **kw)[3]
            assert per_iteration == 5, (kw, per_iteration)
        assert run(rtol=0.0, maxiter=4, engine=True)[3] - run(rtol=0.0, maxiter=3, engine=True)[3] == 4
        assert_close(x_e, x_a, f"cg(engine=True) against the host loop {_name(dtype)}", rtol=1e-9)
        # the zero start residual through the wrapper
        x, meta = lk.dense_vector_gpu.from_array(np.zeros(n, dtype=dtype), c), lk.cg_dp_metadata()
        info = lk.cg(A, lk.dense_vector_gpu.from_array(np.zeros(n, dtype=dtype), c), x, meta=meta, engine=True)
        assert info == meta.info == 0 and meta.converged and meta.n_iter == 0 and meta.res == [0.0] and not np.any(x.to_array())
        with pytest.raises(TypeError):
            lk.cg(A, b, lk.dense_vector_gpu.from_array(np.zeros(n, dtype=dtype), c), preconditioner=object(), engine=True)
    finally:
        c.close()
