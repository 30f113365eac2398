"""lk_gmres at the edges of its contract: a start from x0 != 0, a start residual of exactly zero, kdim at its minimum and beyond n, a
Krylov space exhausted inside the Arnoldi batch, x and b inside V's own panel or in one shared basis, a caller-owned workspace, the
stopping rule with rtol = 0 and with maxiter = 0, the optional outputs NULL, and a context reused across calls of different kdim.

The inputs are stated in tests/_gmres_cases.py (EDGE_CASES, exact_guess) and pinned against the oracle without a GPU in
tests/test_gmres_host_logic.py.  Two references: ora.gmres, at the bare 1e-12 of tests/test_gpu_gmres_engine.py (history relative to
the first residual, solution relative to its largest entry), and the longdouble solution, through the residual bound
tol + 8 n eps ||A||_F ||x|| (the stopping test plus the rounding of one double-precision residual)."""
import ctypes as C

import numpy as np
import pytest

import lightkrylov_amd as lk
from lightkrylov_amd import _capi
from oracle import oracle as ora
from tests import _gmres_cases as cases
from tests._gpu_helpers import KINDS, CallerPanel, basis, seeded
from tests._tol import assert_close

pytestmark = pytest.mark.gpu


def _name(dtype):
    return np.dtype(dtype).name


class _Out:
    def __init__(self, rc, info, nres, n_inner, n_outer, res):
        self.rc, self.info, self.nres, self.n_inner, self.n_outer, self.res = rc, info, nres, n_inner, n_outer, res

    def counts(self):
        return self.info, self.n_inner, self.n_outer, self.nres


def _gmres(A, trans, M, b, x, V, rtol, atol, kdim, maxiter, res=True, counts=True):
    """lk_gmres itself; b and x are vectors (basis, column), V a basis.  The outputs not asked for are passed as NULL."""
    cap = 1 + (maxiter + 1) * (kdim + 1)
    hist = np.full(cap, -7.0)
    nres, ni, no, info = C.c_int64(-99), C.c_int(-99), C.c_int(-99), C.c_int(-99)
    rc = _capi.load().lk_gmres(A._h, 1 if trans else 0, M._h if M is not None else None, b.basis._h, b.col, x.basis._h, x.col, V._h,
                               float(rtol), float(atol), kdim, maxiter, hist.ctypes.data_as(C.POINTER(C.c_double)) if res else None,
                               cap if res else 0, C.byref(nres) if counts else None, C.byref(ni) if counts else None,
                               C.byref(no) if counts else None, C.byref(info))
    if res and counts and rc == 0:
        assert np.all(hist[nres.value:] == -7.0)
        hist = hist[:nres.value]
    return _Out(rc, info.value, nres.value, ni.value, no.value, hist if res else None)


def _operator(ctx, case, A):
    return lk.diag_linop_gpu(A, ctx) if case.form == "diag" else lk.dense_linop_gpu(A, ctx)


def _plain(ctx, case, A, M, bh, x0h, **kw):
    """b, x and V each in a basis of its own, V of exactly the columns the call needs"""
    rtol, atol = case.tolerances(bh)
    b, x = lk.dense_vector_gpu.from_array(bh, ctx), lk.dense_vector_gpu.from_array(x0h, ctx)
    V = lk.krylov_basis_gpu(bh.size, case.kdim + (2 if M is not None else 1), bh.dtype, ctx)
    out = _gmres(A, case.trans, M, b, x, V, rtol, atol, case.kdim, case.maxiter, **kw)
    return out, x.to_array()


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _check_against_both_references(case, dtype, counts, res, x, label):
    A, bh, x0h, info_o, res_o, xo, xref = cases.oracle_run(case.name, _name(dtype))
    assert counts == case.pin(dtype), f"{label}: (info, n_inner, n_outer, nres) = {counts}, pinned {case.pin(dtype)}"
    assert counts[0] == info_o and len(res) == len(res_o) == counts[3], label
    assert_close(res, res_o, label + " [history]", scale=res_o[0])
    assert_close(x, xo, label + " [x]")
    if case.converges:
        cases.assert_solves(case, A, bh, x, xref, label)
    if case.name.startswith("warm_start"):
        # the first entry of the history is ||b - op(A) x0||: a product that is skipped leaves ||b|| there
        r0 = cases.long_norm(cases._ext(bh) - cases.long_product(case, A, x0h))
        bound = cases.start_residual_bound(A, x0h)
        print(f"{label}: |res[0] - ||r0||| = {abs(res[0] - r0):.3e}, bound {bound:.3e}, | ||b|| - ||r0|| | = {abs(np.linalg.norm(bh) - r0):.3e}")
        assert abs(res[0] - r0) <= bound < abs(res[0] - float(np.linalg.norm(bh))), label


@pytest.mark.parametrize("case", cases.EDGE_CASES, ids=lambda c: c.name)
@pytest.mark.parametrize("dtype", KINDS)
def test_edge_cases_through_the_c_call_and_the_wrapper(ctx, dtype, case):
    A, bh, x0h = cases.oracle_run(case.name, _name(dtype))[:3]
    Aop = _operator(ctx, case, A)
    label = f"lk_gmres {case.name} {_name(dtype)}"
    out, x = _plain(ctx, case, Aop, None, bh, x0h)
    assert out.rc == 0, label
    _check_against_both_references(case, dtype, out.counts(), out.res, x, label)
    # the Python wrapper: lk.gmres(engine=True)
    rtol, atol = case.tolerances(bh)
    b, xv, meta = lk.dense_vector_gpu.from_array(bh, ctx), lk.dense_vector_gpu.from_array(x0h, ctx), lk.gmres_dp_metadata()
    info = lk.gmres(Aop, b, xv, rtol=rtol, atol=atol, options=lk.gmres_dp_opts(kdim=case.kdim, maxiter=case.maxiter), transpose=case.trans,
                    meta=meta, engine=True)
    assert info == meta.info and meta.converged == case.converges and meta.n_iter == abs(info), label
    _check_against_both_references(case, dtype, (info, meta.n_inner, meta.n_outer, len(meta.res)), np.array(meta.res), xv.to_array(),
                                   label + " [wrapper]")


@pytest.mark.parametrize("dtype", KINDS)
def test_warm_start_with_a_jacobi_preconditioner(ctx, dtype):
    """tests/_gmres_cases.variable_coefficient with M = 1 / diag from x0 != 0, against ora.gmres with the same preconditioner: the oracle
    solves (A M) u = b from u0 = x0 / m, its residuals are those of x = M u"""
    _Acsr, Ad, m, bh = cases.variable_coefficient(dtype)
    n, p = bh.size, cases.PRECONDITIONED
    x0h = 0.01 * seeded(n, dtype, 77)
    u = x0h / m
    info_o, res_o = ora.gmres(ora.PyOp(lambda v: Ad @ (m * v), dtype), bh, u, rtol=p["rtol"], atol=p["atol"], kdim=p["kdim"], maxiter=p["maxiter"])
    case = cases.EdgeCase("jacobi", "dense", None, p["kdim"], p["maxiter"], p["rtol"])
    out, x = _plain(ctx, case, lk.dense_linop_gpu(Ad, ctx), lk.diag_linop_gpu(m, ctx), bh, x0h)
    label = f"lk_gmres Jacobi from x0 != 0 {_name(dtype)}"
    assert out.rc == 0 and out.info == info_o > 0 and out.nres == len(res_o) and out.n_inner + out.n_outer == out.info, label
    assert_close(out.res, res_o, label + " [history]", scale=res_o[0])
    assert_close(x, m * u, label + " [x]")
    r0 = cases.long_norm(cases._ext(bh) - cases._ext(Ad) @ cases._ext(x0h))
    bound = cases.start_residual_bound(Ad, x0h)
    assert abs(out.res[0] - r0) <= bound < abs(out.res[0] - float(np.linalg.norm(bh))), label
    cases.assert_solves(case, Ad, bh, x, cases.longdouble_solve(Ad, bh), label)


@pytest.mark.parametrize("dtype", KINDS)
def test_unscaled_steps_behind_a_small_subdiagonal_with_a_preconditioner(ctx, dtype):
    """tests/_gmres_cases.tiny_diag with a right preconditioner of size one, M = diag(1 + u / 2): every H(k+1, k) <= tol with the residual
    far above it, so each batch on the product operator ends at its first step, the vector is scaled back and the remaining steps run one
    by one through M's scratch column (gmres.fypp:171-172).  Against ora.gmres on x -> A (M x); the solution is M u."""
    d, bh = cases.tiny_diag(dtype)
    p = cases.TINY
    m = (1.0 + 0.5 * seeded(bh.size, np.float64, 8)).astype(dtype)
    u = np.zeros(bh.size, dtype=dtype)
    info_o, res_o = ora.gmres(ora.PyOp(lambda v: d * (m * v), dtype), bh, u, rtol=p["rtol"], atol=p["atol"], kdim=p["kdim"], maxiter=p["maxiter"])
    assert info_o == -8 and len(res_o) == 9 and np.abs(d * m).max() * 2 < p["rtol"] < res_o.min()
    case = cases.EdgeCase("tiny with M", "diag", None, p["kdim"], p["maxiter"], p["rtol"])
    out, x = _plain(ctx, case, lk.diag_linop_gpu(d, ctx), lk.diag_linop_gpu(m, ctx), bh, np.zeros(bh.size, dtype=dtype))
    label = f"lk_gmres tiny diag with M {_name(dtype)}"
    assert out.rc == 0 and out.counts() == (-8, 6, 2, 9), f"{label}: {out.counts()}"
    assert_close(out.res, res_o, label + " [history]", scale=res_o[0])
    assert_close(x, m * u, label + " [x]")


def _zero_residual_inputs(dtype):
    """(what, d, b, x0, atol): x0 the exact solution for n = 1 and 257; b = 0, x0 = 0 with atol = 0 and 1e-12"""
    for n in cases.EXACT_GUESS_N:
        d, b, x0 = cases.exact_guess(dtype, n)
        yield f"exact guess n = {n}", d, b, x0, 0.0
    n = cases.ZERO_B["n"]
    for atol in cases.ZERO_B["atols"]:
        yield f"b = 0, x0 = 0, atol = {atol:g}", cases.powers_of_two_diag(dtype, n), np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype), atol


@pytest.mark.parametrize("precond", [False, True], ids=["noM", "M"])
@pytest.mark.parametrize("dtype", KINDS)
def test_a_zero_start_residual_is_not_an_error(ctx, dtype, precond):
    """||r0|| = 0 exactly (the reference divides by it, gmres.fypp:142-143, and returns NaN): LK_OK, info = 0, no iteration, nres = 1,
    res[0] = 0, x bit-identical to x0, the columns of V behind those the call may write untouched -- both kinds, with and without M"""
    kdim, maxiter = 4, 3
    ncw = kdim + 1 + (1 if precond else 0)
    for what, d, bh, x0h, atol in _zero_residual_inputs(dtype):
        label = f"lk_gmres zero start residual, {what}, {_name(dtype)}, {'with' if precond else 'without'} M"
        n = bh.size
        A = lk.diag_linop_gpu(d, ctx)
        M = lk.diag_linop_gpu(1.0 / d, ctx) if precond else None
        W = lk.krylov_basis_gpu(n, ncw + 2, dtype, ctx)
        img = basis(n, ncw + 2, dtype, 300)
        W.upload(img)
        b, x = lk.dense_vector_gpu.from_array(bh, ctx), lk.dense_vector_gpu.from_array(x0h, ctx)
        out = _gmres(A, False, M, b, x, W, 1e-10, atol, kdim, maxiter)
        assert out.rc == 0, f"{label}: rc = {out.rc}"
        assert out.counts() == (0, 0, 0, 1) and list(out.res) == [0.0], f"{label}: {out.counts()}, {out.res}"
        assert _same_bits(x.to_array(), x0h), label
        assert _same_bits(W.download(ncw, 2), np.asfortranarray(img[:, ncw:])), label
        # the optional outputs NULL
        out = _gmres(A, False, M, b, x, W, 1e-10, atol, kdim, maxiter, res=False, counts=False)
        assert (out.rc, out.info) == (0, 0) and _same_bits(x.to_array(), x0h), label
        # the Python wrapper
        meta = lk.gmres_dp_metadata()
        info = lk.gmres(A, b, x, rtol=1e-10, atol=atol, preconditioner=lk.linop_precond_gpu(M) if precond else None,
                        options=lk.gmres_dp_opts(kdim=kdim, maxiter=maxiter), meta=meta, engine=True)
        assert info == meta.info == 0 and meta.converged and (meta.n_iter, meta.n_inner, meta.n_outer) == (0, 0, 0), label
        assert list(meta.res) == [0.0] and _same_bits(x.to_array(), x0h), label


def _placement_problem(ctx, dtype, precond):
    """(case, A, M, b, x0): without M the dense warm start with restarts; with M the Jacobi problem from x0 != 0"""
    if not precond:
        case = next(c for c in cases.EDGE_CASES if c.name == "warm_start-dense-k5-N")
        A, bh, x0h = cases.oracle_run(case.name, _name(dtype))[:3]
        return case, lk.dense_linop_gpu(A, ctx), None, bh, x0h
    _Acsr, Ad, m, bh = cases.variable_coefficient(dtype)
    p = cases.PRECONDITIONED
    case = cases.EdgeCase("jacobi", "dense", None, p["kdim"], p["maxiter"], p["rtol"])
    return case, lk.dense_linop_gpu(Ad, ctx), lk.diag_linop_gpu(m, ctx), bh, 0.01 * seeded(bh.size, dtype, 77)


@pytest.mark.parametrize("precond", [False, True], ids=["noM", "M"])
@pytest.mark.parametrize("dtype", KINDS)
def test_where_x_b_and_the_workspace_live_changes_no_bit(ctx, dtype, precond):
    """x and b behind the written columns of V's own panel; x and b in one shared basis at jb = 3, jx = 1; V a caller-owned panel with
    ld = n + 6 and NaN padding: history, counts and solution bit for bit those of the plain placement, every foreign column and the
    padding bit-unchanged.  With M the first legal column moves by one: jx = kdim + 1 is refused with nothing written."""
    case, A, M, bh, x0h = _placement_problem(ctx, dtype, precond)
    n, kdim = bh.size, case.kdim
    rtol, atol = case.tolerances(bh)
    ncw = kdim + 1 + (1 if precond else 0)
    label = f"lk_gmres placement {_name(dtype)} {'with' if precond else 'without'} M"
    plain, x_plain = _plain(ctx, case, A, M, bh, x0h)
    assert plain.rc == 0 and plain.info > 0 and plain.n_outer > 1, label          # restarts: the update and the residual run more than once

    def same(out, x, what):
        assert out.rc == 0 and out.counts() == plain.counts(), f"{label}, {what}: {out.counts()} against {plain.counts()}"
        assert _same_bits(out.res, plain.res), f"{label}, {what}: history differs by {np.abs(out.res - plain.res).max():.2e}"
        assert _same_bits(x, x_plain), f"{label}, {what}: x differs by {np.abs(x - x_plain).max():.2e}"

    # x and b in V's own panel, behind the columns the call writes; the columns in front hold finite garbage
    img = basis(n, ncw + 3, dtype, 500)
    img[:, ncw], img[:, ncw + 1] = x0h, bh
    W = lk.krylov_basis_gpu(n, ncw + 3, dtype, ctx)
    W.upload(img)
    if precond:
        out = _gmres(A, case.trans, M, W[ncw + 1], W[kdim + 1], W, rtol, atol, kdim, case.maxiter)
        assert out.rc == -1 and out.counts() == (-99, -99, -99, -99), f"{label}: x in the scratch column of the product operator"
        assert _same_bits(W.download(), np.asfortranarray(img)), label
    out = _gmres(A, case.trans, M, W[ncw + 1], W[ncw], W, rtol, atol, kdim, case.maxiter)
    got = W.download()
    same(out, got[:, ncw], "x and b in V's panel")
    assert _same_bits(got[:, ncw + 1:], np.asfortranarray(img[:, ncw + 1:])), f"{label}: b or the column behind it changed"

    # x and b in one basis of their own
    simg = basis(n, 5, dtype, 520)
    simg[:, 1], simg[:, 3] = x0h, bh
    S = lk.krylov_basis_gpu(n, 5, dtype, ctx)
    S.upload(simg)
    V = lk.krylov_basis_gpu(n, ncw, dtype, ctx)
    out = _gmres(A, case.trans, M, S[3], S[1], V, rtol, atol, kdim, case.maxiter)
    got = S.download()
    same(out, got[:, 1], "x and b in one basis, jb = 3, jx = 1")
    assert _same_bits(got[:, [0, 2, 3, 4]], np.asfortranarray(simg[:, [0, 2, 3, 4]])), f"{label}: a column beside x changed"

    # V in the caller's memory (tests/_gpu_helpers.CallerPanel: `get` asserts that no word outside the panel's rows changed)
    wimg = basis(n, ncw + 1, dtype, 540)
    panel = CallerPanel(ctx, dtype, n, ncw + 1, "nan_pad", pad=6)
    assert panel.ld == n + 6
    panel.set(wimg)
    b, x = lk.dense_vector_gpu.from_array(bh, ctx), lk.dense_vector_gpu.from_array(x0h, ctx)
    out = _gmres(A, case.trans, M, b, x, panel.B, rtol, atol, kdim, case.maxiter)
    same(out, x.to_array(), "V a caller-owned panel, ld = n + 6")
    assert _same_bits(panel.get(label)[:, ncw:], np.asfortranarray(wimg[:, ncw:])), f"{label}: the column behind V's changed"


@pytest.mark.parametrize("dtype", KINDS)
def test_optional_outputs_may_be_null(ctx, dtype):
    """res = NULL with nres, n_inner, n_outer wanted, and all of them NULL: everything else as in the plain call"""
    case, A, M, bh, x0h = _placement_problem(ctx, dtype, False)
    plain, x_plain = _plain(ctx, case, A, M, bh, x0h)
    out, x = _plain(ctx, case, A, M, bh, x0h, res=False)
    assert out.rc == 0 and out.counts() == plain.counts() and plain.nres > 1 and _same_bits(x, x_plain)
    out, x = _plain(ctx, case, A, M, bh, x0h, res=False, counts=False)
    assert out.rc == 0 and out.info == plain.info and _same_bits(x, x_plain)
    assert (out.nres, out.n_inner, out.n_outer) == (-99, -99, -99)


@pytest.mark.parametrize("dtype", KINDS)
def test_a_context_carries_nothing_from_one_call_to_the_next(dtype):
    """kdim = 40, then 5, then 40 on ONE context give the bits a fresh context gives each: the pinned slot that brings beta to the host
    and the reduction buffers are reused, nothing in them is"""
    by_kdim = {c.kdim: c for c in cases.EDGE_CASES if c.name in ("warm_start-dense-k40-N", "warm_start-dense-k5-N")}

    def run(c, kdim):
        case = by_kdim[kdim]
        A, bh, x0h = cases.oracle_run(case.name, _name(dtype))[:3]
        out, x = _plain(c, case, lk.dense_linop_gpu(A, c), None, bh, x0h)
        assert out.rc == 0 and out.counts() == case.pin(dtype)
        return out, x

    order = (40, 5, 40)
    one = lk.Context(device=0)
    try:
        reused = [run(one, k) for k in order]
    finally:
        one.close()
    for i, k in enumerate(order):
        fresh = lk.Context(device=0)
        try:
            out, x = run(fresh, k)
        finally:
            fresh.close()
        assert out.counts() == reused[i][0].counts() and _same_bits(out.res, reused[i][0].res) and _same_bits(x, reused[i][1]), (i, k)
