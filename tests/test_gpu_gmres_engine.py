"""lk_gmres: restarted GMRES with an optional right preconditioner as one engine call (gmres.fypp:65-255), against the oracle's gmres
and against the package's gmres on the paths that existed before it.  The cases are stated in tests/_gmres_cases.py and pinned against
the oracle without a GPU in tests/test_gmres_host_logic.py.  Histories are compared relative to the first residual and solutions
relative to their largest entry, both at the bare 1e-12 of tests/_tol.py."""
import ctypes as C

import numpy as np
import pytest

import lightkrylov_amd as lk
from lightkrylov_amd import _capi
from oracle import oracle as ora
from tests import _gmres_cases as cases
from tests._gpu_helpers import KINDS, _sharded, seeded
from tests._tol import assert_close

pytestmark = pytest.mark.gpu


def _name(dtype):
    return np.dtype(dtype).name


def _gpu_solve(ctx, A, bh, x0h, dtype, rtol, atol, kdim, maxiter, transpose=False, preconditioner=None, engine=None):
    b = lk.dense_vector_gpu.from_array(bh, ctx)
    x = lk.dense_vector_gpu.from_array(x0h, ctx)
    meta = lk.gmres_dp_metadata()
    info = lk.gmres(A, b, x, rtol=rtol, atol=atol, preconditioner=preconditioner, options=lk.gmres_dp_opts(kdim=kdim, maxiter=maxiter),
                    transpose=transpose, meta=meta, engine=engine)
    assert info == meta.info
    return info, np.array(meta.res), x.to_array(), meta


def _operators(ctx, which, dtype, transpose):
    """(engine operator, the oracle's operator for op(A), b)"""
    if which == "diag":
        d, b = cases.pipelines_diag(dtype)
        return lk.diag_linop_gpu(d, ctx), ora.DiagOp(np.conj(d) if transpose else d), b
    A, b = cases.dense_nonsymmetric(dtype)
    return lk.dense_linop_gpu(A, ctx), ora.DenseOp(np.asfortranarray(A.conj().T) if transpose else A), b


@pytest.mark.parametrize("transpose", [False, True], ids=["N", "H"])
@pytest.mark.parametrize("which", ["diag", "dense"])
@pytest.mark.parametrize("dtype", KINDS)
def test_unpreconditioned_solves_against_the_oracle_and_the_existing_path(ctx, dtype, which, transpose):
    A, Ao, bh = _operators(ctx, which, dtype, transpose)
    n = bh.size
    endings = []
    for kdim, maxiter, rtol, tag in cases.UNPRECONDITIONED:
        label = f"lk_gmres {which} {_name(dtype)} {'H' if transpose else 'N'}: {tag}"
        xo = np.zeros(n, dtype=dtype)
        info_o, res_o = ora.gmres(Ao, bh, xo, rtol=rtol, atol=0.0, kdim=kdim, maxiter=maxiter)
        info, res, x, meta = _gpu_solve(ctx, A, bh, np.zeros(n, dtype=dtype), dtype, rtol, 0.0, kdim, maxiter, transpose, engine=True)
        assert info == info_o and len(res) == len(res_o), label
        assert_close(res, res_o, label + " [history]", scale=res_o[0])
        assert_close(x, xo, label + " [x]")
        info_t, res_t, x_t, meta_t = _gpu_solve(ctx, A, bh, np.zeros(n, dtype=dtype), dtype, rtol, 0.0, kdim, maxiter, transpose)
        assert info == info_t and len(res) == len(res_t) and (meta.n_inner, meta.n_outer) == (meta_t.n_inner, meta_t.n_outer), label
        assert meta.n_iter == meta_t.n_iter and meta.converged == meta_t.converged, label
        assert_close(res, res_t, label + " [history, existing path]", scale=res_t[0])
        assert_close(x, x_t, label + " [x, existing path]")
        endings.append((info > 0, meta.n_outer > 1))
    # converged | converged after restarts | maxiter exhausted; on the dense operator the first is inside the first cycle (pinned on the
    # CPU in tests/test_gmres_host_logic.py; the complex diagonal operator needs a restart at kdim = 40 as well)
    assert [e[0] for e in endings] == [True, True, False] and endings[1][1] and endings[2][1], endings
    assert which != "dense" or not endings[0][1], endings


@pytest.mark.parametrize("dtype", KINDS)
def test_history_is_cut_at_res_cap(ctx, dtype):
    d, bh = cases.pipelines_diag(dtype, n=4099)
    A = lk.diag_linop_gpu(d, ctx)
    kdim, maxiter = 5, 30
    full = _gpu_solve(ctx, A, bh, np.zeros(bh.size, dtype=dtype), dtype, 1e-10, 0.0, kdim, maxiter, engine=True)[1]
    b, x = lk.dense_vector_gpu.from_array(bh, ctx), lk.dense_vector_gpu(bh.size, dtype, ctx)
    V = lk.krylov_basis_gpu(bh.size, kdim + 1, dtype, ctx)
    cap = 4
    res = np.full(cap + 3, -7.0)
    nres, ni, no, info = C.c_int64(), C.c_int(), C.c_int(), C.c_int()
    _capi.check(V._lib.lk_gmres(A._h, 0, None, b.basis._h, b.col, x.basis._h, x.col, V._h, 1e-10, 0.0, kdim, maxiter,
                                res.ctypes.data_as(C.POINTER(C.c_double)), cap, C.byref(nres), C.byref(ni), C.byref(no), C.byref(info)))
    assert nres.value == len(full) > cap and info.value > 0
    assert np.array_equal(res[:cap], full[:cap]) and np.all(res[cap:] == -7.0)
    assert ni.value + no.value == info.value
    # res = NULL and the optional outputs NULL
    x.zero()
    _capi.check(V._lib.lk_gmres(A._h, 0, None, b.basis._h, b.col, x.basis._h, x.col, V._h, 1e-10, 0.0, kdim, maxiter,
                                None, 0, None, None, None, C.byref(info)))
    assert info.value == ni.value + no.value


@pytest.mark.parametrize("dtype", KINDS)
def test_steps_behind_a_small_subdiagonal_go_on_unscaled(ctx, dtype):
    """gmres.fypp:171-172 on tests/_gmres_cases.tiny_diag (A = 1e-12 * diag, ||b|| = 1, rtol = 1e-8, kdim = 3, maxiter = 1): the Arnoldi batch
    stops at its first step on H(2, 1) <= tol with the residual at 0.4, the remaining steps of each cycle run one by one without scaling.
    On the CPU the oracle and the host mirror on oracle_vector agree on this case at 1e-12 (measured: history 1.2e-16, solution 3.5e-16;
    tests/test_gmres_host_logic.py asserts it), so the oracle is the reference here as everywhere else.  (The package's own gmres on GPU
    vectors is NOT compared here: its inner cycle takes the vector as lk_arnoldi leaves it at the stop, normalised, and its history departs
    from the oracle's at the second step -- 0.21 against 0.40 on this case.  lk_gmres undoes that scaling.)"""
    d, bh = cases.tiny_diag(dtype)
    p = cases.TINY
    xo = np.zeros(bh.size, dtype=dtype)
    info_o, res_o = ora.gmres(ora.DiagOp(d), bh, xo, rtol=p["rtol"], atol=p["atol"], kdim=p["kdim"], maxiter=p["maxiter"])
    A = lk.diag_linop_gpu(d, ctx)
    info, res, x, meta = _gpu_solve(ctx, A, bh, np.zeros(bh.size, dtype=dtype), dtype, p["rtol"], p["atol"], p["kdim"], p["maxiter"], engine=True)
    assert info == info_o == -8 and len(res) == len(res_o) == 9 and (meta.n_inner, meta.n_outer) == (6, 2)
    assert_close(res, res_o, f"lk_gmres tiny diag {_name(dtype)} [history]", scale=res_o[0])
    assert_close(x, xo, f"lk_gmres tiny diag {_name(dtype)} [x]")


@pytest.mark.parametrize("form", ["csr", "dense"])
@pytest.mark.parametrize("dtype", KINDS)
def test_jacobi_preconditioned_solves(ctx, dtype, form):
    """A: tests/_gmres_cases.variable_coefficient (n = 400, diagonal 1 .. 1e4), M = diag_linop_gpu(1 / diag).  On the CPU the oracle takes
    24 iterations with the preconditioner (converged) and 231 without (GMRES(20), maxiter 10: not converged), both kinds."""
    Acsr, Ad, m, bh = cases.variable_coefficient(dtype)
    n = bh.size
    p = cases.PRECONDITIONED
    A = lk.csr_linop_gpu(Acsr, ctx) if form == "csr" else lk.dense_linop_gpu(Ad, ctx)
    M = lk.diag_linop_gpu(m, ctx)
    pre = lk.linop_precond_gpu(M)
    label = f"lk_gmres Jacobi {form} {_name(dtype)}"
    # (a) x0 = 0 against the oracle on x -> A (M x): the solution is M u
    u = np.zeros(n, dtype=dtype)
    info_o, res_o = ora.gmres(ora.PyOp(lambda v: Ad @ (m * v), dtype), bh, u, rtol=p["rtol"], atol=p["atol"], kdim=p["kdim"], maxiter=p["maxiter"])
    info, res, x, meta = _gpu_solve(ctx, A, bh, np.zeros(n, dtype=dtype), dtype, p["rtol"], p["atol"], p["kdim"], p["maxiter"], preconditioner=pre)
    assert info == info_o == cases.PRECONDITIONED_ITERATIONS[0] and len(res) == len(res_o), label
    assert_close(res, res_o, label + " [history]", scale=res_o[0])
    assert_close(x, m * u, label + " [x]")
    # (b) x0 != 0 and transpose, against the step-by-step preconditioned path
    x0 = 0.01 * seeded(n, dtype, 77)
    got = _gpu_solve(ctx, A, bh, x0, dtype, p["rtol"], p["atol"], p["kdim"], p["maxiter"], transpose=True, preconditioner=pre)
    ref = _gpu_solve(ctx, A, bh, x0, dtype, p["rtol"], p["atol"], p["kdim"], p["maxiter"], transpose=True, preconditioner=pre, engine=False)
    assert got[0] == ref[0] and len(got[1]) == len(ref[1]) and (got[3].n_inner, got[3].n_outer) == (ref[3].n_inner, ref[3].n_outer), label
    assert_close(got[1], ref[1], label + " [history, x0 != 0, H, step by step]", scale=ref[1][0])
    assert_close(got[2], ref[2], label + " [x, x0 != 0, H, step by step]")
    # (c) strictly fewer iterations than without the preconditioner
    info_u = _gpu_solve(ctx, A, bh, np.zeros(n, dtype=dtype), dtype, p["rtol"], p["atol"], p["kdim"], p["maxiter"], engine=True)[0]
    assert info_u == cases.PRECONDITIONED_ITERATIONS[1] and 0 < info < abs(info_u), label


def _columns(W, col0, ncols):
    """columns [col0, col0 + ncols) of W as a basis with a handle of its own (W[:k] shares W's handle and its column count)"""
    _dt, n, _nc, ld, ptr = W.info()
    h = C.c_void_p()
    _capi.check(W._lib.lk_basis_wrap(W.ctx._h, _dt, n, ncols, ld, C.c_void_p(ptr + col0 * ld * W.dtype.itemsize), C.byref(h)))
    return lk.krylov_basis_gpu(n, ncols, W.dtype, W.ctx, _handle=h, _owner=W)


def _call(A, M, b, x, V, kdim, info=True, trans=0):
    out = C.c_int(-99)
    rc = _capi.load().lk_gmres(A._h if A is not None else None, trans, M._h if M is not None else None, b.basis._h, b.col, x.basis._h, x.col,
                               V._h if V is not None else None, 1e-10, 0.0, kdim, 3, None, 0, None, None, None, C.byref(out) if info else None)
    return rc, out.value


@pytest.mark.parametrize("dtype", KINDS)
def test_invalid_arguments_leave_everything_unchanged(ctx, dtype):
    n, kdim = 257, 4
    other_dtype = np.complex128 if dtype == np.float64 else np.float64
    d = 1.0 + 0.5 * seeded(n, dtype, 7)
    A, M = lk.diag_linop_gpu(d, ctx), lk.diag_linop_gpu(1.0 / d, ctx)
    W = lk.krylov_basis_gpu(n, kdim + 2 + 2, dtype, ctx)             # the workspace's parent: columns [0, kdim + 2) | x | b
    img = np.stack([seeded(n, dtype, 200 + j) for j in range(kdim + 4)], axis=1)
    W.upload(img)
    V1, V2 = _columns(W, 0, kdim + 1), _columns(W, 0, kdim + 2)
    x, b = W[kdim + 2], W[kdim + 3]
    short = lk.krylov_basis_gpu(n - 1, kdim + 2, dtype, ctx)
    other_kind = lk.krylov_basis_gpu(n, kdim + 2, other_dtype, ctx)
    ctx2 = lk.Context(device=0)
    try:
        foreign = lk.krylov_basis_gpu(n, kdim + 2, dtype, ctx2)
        bad = {
            "null A": lambda: _call(None, None, b, x, V1, kdim),
            "null V": lambda: _call(A, None, b, x, None, kdim),
            "null info": lambda: _call(A, None, b, x, V1, kdim, info=False),
            "kdim 1": lambda: _call(A, None, b, x, V1, 1),
            "kdim 513": lambda: _call(A, None, b, x, V1, 513),
            "workspace of kdim columns": lambda: _call(A, None, b, x, _columns(W, 0, kdim), kdim),
            "workspace of kdim + 1 columns with M": lambda: _call(A, M, b, x, V1, kdim),
            "x in V": lambda: _call(A, None, b, W[1], V1, kdim),
            "b in V": lambda: _call(A, None, W[kdim], x, V1, kdim),
            "x in the scratch column of V": lambda: _call(A, M, b, W[kdim + 1], V2, kdim),
            "x is b": lambda: _call(A, None, b, b, V1, kdim),
            "operator of another size": lambda: _call(lk.diag_linop_gpu(d[:-1], ctx), None, b, x, V1, kdim),
            "operator of another kind": lambda: _call(lk.diag_linop_gpu(np.ones(n, dtype=other_dtype), ctx), None, b, x, V1, kdim),
            "preconditioner of another size": lambda: _call(A, lk.diag_linop_gpu(d[:-1], ctx), b, x, V2, kdim),
            "workspace of another size": lambda: _call(A, None, b, x, short, kdim),
            "workspace of another kind": lambda: _call(A, None, b, x, other_kind, kdim),
            "workspace of another context": lambda: _call(A, None, b, x, foreign, kdim),
        }
        for what, call in bad.items():
            rc, info = call()
            assert rc == -1 and info == -99, what
            assert W.download().tobytes(order="F") == np.asfortranarray(img).tobytes(order="F"), what
        # the same workspace is wide enough without M, and x may be a column of V the call does not write
        rc, info = _call(A, None, b, W[kdim + 1], V1, kdim)
        assert rc == 0 and abs(info) == 4 * 5                          # it ran: GMRES(4), maxiter 3 on a random start is not converged
    finally:
        ctx2.close()


def test_nan_in_b_is_reported(ctx):
    n = 257
    A = lk.diag_linop_gpu(1.0 + 0.5 * seeded(n, np.float64, 7), ctx)
    bh = seeded(n, np.float64, 1)
    bh[5] = np.nan
    b, x = lk.dense_vector_gpu.from_array(bh, ctx), lk.dense_vector_gpu(n, np.float64, ctx)
    V = lk.krylov_basis_gpu(n, 5, np.float64, ctx)
    rc, _ = _call(A, None, b, x, V, 4)
    assert rc == -5
    with pytest.raises(_capi.LightKrylovHipError, match=r"\[-5\]"):
        lk.gmres(A, b, x, options=lk.gmres_dp_opts(kdim=4, maxiter=1), engine=True)


def test_row_sharded_context_is_refused_and_the_mirror_keeps_its_path():
    n, kdim = 4099, 6
    d = 2.0 + np.arange(n) % 5 + 0.5 * seeded(n, np.float64, 7)
    bh = seeded(n, np.float64, 17)
    xo = np.zeros(n)
    info_o, res_o = ora.gmres(ora.DiagOp(d), bh, xo, rtol=1e-10, atol=0.0, kdim=kdim, maxiter=30)

    def body(rank, c, row0, nl):
        A = lk.diag_linop_gpu(d[row0:row0 + nl], c)
        b = lk.dense_vector_gpu.from_array(bh[row0:row0 + nl], c)
        x = lk.dense_vector_gpu(nl, np.float64, c)
        x.zero()
        V = lk.krylov_basis_gpu(nl, kdim + 1, np.float64, c)
        rc, info = _call(A, None, b, x, V, kdim)
        refused = rc == -1 and info == -99 and not np.any(x.to_array())
        try:
            lk.gmres(A, b, x, options=lk.gmres_dp_opts(kdim=kdim, maxiter=30), engine=True)
            raised = False
        except TypeError:
            raised = True
        meta = lk.gmres_dp_metadata()
        info = lk.gmres(A, b, x, rtol=1e-10, atol=0.0, options=lk.gmres_dp_opts(kdim=kdim, maxiter=30), meta=meta)
        return refused, raised, info, np.array(meta.res), x.to_array()

    out, _grp = _sharded(n, 2, body)
    assert all(o[0] and o[1] for o in out)
    assert all(o[2] == info_o for o in out)
    assert_close(out[0][3], res_o, "sharded gmres on the existing path [history]", scale=res_o[0])
    assert_close(np.concatenate([o[4] for o in out]), xo, "sharded gmres on the existing path [x]")
