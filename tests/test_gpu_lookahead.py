"""Look-ahead of the asynchronous Arnoldi batch on a diagonal operator (tuning key "fuse_rowop" >= 2): sweep 3 of step k also forms the sums
sweep 1 of step k + 1 would form (h1 and ||y||^2 of y = D x_(k+1), from y'' still in registers), so step k + 1 starts at sweep 2 and a step
makes two passes over the basis instead of three.  Every test runs "fuse_rowop" = 3 (look-ahead at every size) on a context of its own, real
kind, with both diagonal operators (generated linspace and explicit array) and the adjoint of the explicit one, the single launch switched
off (a cache-resident step takes no look-ahead).

Bars: H against the oracle normwise per column at 1e-12 (tests/_tol.py), ||X^H X - I||max <= 1e-12, the Arnoldi relation on a sample of rows
at 1e-12.  Step 2 of the two routes (test 3): h1 of step 2 is (sum x (d y'')) / beta here and sum x (d (y'' / beta)) on the three-sweep route,
the same number rounded differently, so the column may differ by a few units in the last place of its norm: bar 4 * 2^-52 * ||H(:, 2)||_2."""
import numpy as np
import pytest

import lightkrylov_amd as lk
from lightkrylov_amd import _capi
from oracle import oracle as ora
from tests._gpu_helpers import seeded
from tests._tol import assert_columns_close

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
# odd n and a ragged last tile; k crossing 16 -> 17 and 32 -> 33 (a wave-column more); k = 128 (every register slot, all k + 3 partial slots);
# 8 waves x 64 lanes x 2 rows x 3 tiles + 1 row
EDGES = [(1, 1), (2, 2), (999, 3), (2001, 40), (4099, 128), (8 * 64 * 2 * 3 + 1, 33)]
OPERATORS = [("lin", False), ("d", False), ("d", True)]
OP_IDS = ["linspace", "d", "d_adjoint"]


@pytest.fixture()
def fresh():
    ctxs = []

    def make(**kw):
        c = lk.Context(device=0)
        for key, val in dict(dict(resident=0, fuse_rowop=3), **kw).items():
            c.set_tuning(key, val)
        ctxs.append(c)
        return c
    yield make
    for c in ctxs:
        c.close()


def _diag(which, n, dtype=np.float64):
    g = np.arange(n) / n
    return ((1.0 + g) * (np.exp(1j * g) if np.dtype(dtype).kind == "c" else 1.0)).astype(dtype)


def _operator(c, which, n, dtype=np.float64):
    if which == "lin":
        return lk.diag_linop_gpu(n_local=n, row0=0, d0=1.0, dstep=1.0 / n, ctx=c)
    return lk.diag_linop_gpu(_diag(which, n, dtype), c)


def _x0(n, dtype=np.float64, seed=7):
    x0 = seeded(n, dtype, seed)
    return x0 / np.linalg.norm(x0)


def _run(c, A, n, m, x0, transpose=False, dtype=np.float64, **kw):
    """one factorisation with the engine's profile on: info, H, the basis, launches of (sweep 1, sweep 2, sweep 3, operator)"""
    X = lk.krylov_basis_gpu(n, m + 1, dtype, c)
    X.upload(x0.reshape(-1, 1), 0)
    H = np.zeros((m + 1, m), dtype=dtype, order="F")
    c.profile_reset()
    c.profile_enable(True)
    info = lk.arnoldi(A, X, H, transpose=transpose, **kw)
    c.sync()
    c.profile_enable(False)
    counts = tuple(c.profile_get(t)[0] for t in ("dgs_sweep1", "dgs_sweep2", "dgs_sweep3", "matvec"))
    return info, H, X.download(), counts


_ORACLE = {}


def _oracle(n, m):
    """(H, info) of the reference's Arnoldi on diag(1 + i / n) from the seeded start vector: computed once per shape, never modified.
    (n = 1, m = 1 and n = 2, m = 2 exhaust the space at their last step: info = m there.)"""
    if (n, m) not in _ORACLE:
        Xo = np.zeros((n, m + 1), order="F")
        Xo[:, 0] = _x0(n)
        Ho = np.zeros((m + 1, m), order="F")
        info = ora.arnoldi(ora.DiagOp(_diag("d", n)), Xo, Ho)
        assert info == (m if n <= m else 0)
        Ho.setflags(write=False)
        _ORACLE[(n, m)] = (Ho, info)
    return _ORACLE[(n, m)]


def _check_against_oracle(c, which, transpose, n, m, label):
    info, H, X, counts = _run(c, _operator(c, which, n), n, m, _x0(n), transpose)
    Ho, info_o = _oracle(n, m)
    assert info == info_o
    assert_columns_close(H, Ho, label)
    # an exhausted space (info = the step that found it): columns 0 .. info - 1 are Krylov vectors, the one behind them is a random draw,
    # and the relation holds for the info - 1 steps before it
    kv, ks = (info, info - 1) if info else (m + 1, m)
    G = X[:, :kv].T @ X[:, :kv]
    orth = np.abs(G - np.eye(kv)).max()
    rows = np.unique(np.linspace(0, n - 1, 50).astype(np.int64))
    AX = _diag("d", n)[rows, None] * X[rows, :ks]
    R = AX - X[rows, :ks + 1] @ H[:ks + 1, :ks]
    rel = np.abs(R).max(axis=0) / np.maximum(np.abs(AX).max(axis=0), 1e-300) if ks else np.zeros(1)
    print(f"{label}: ||X^H X - I||max = {orth:.2e}, Arnoldi relation on {len(rows)} rows: {rel.max():.2e}, launches {counts}")
    assert orth <= 1e-12, f"{label}: ||X^H X - I||max = {orth:.2e}"
    assert rel.max() <= 1e-12, f"{label}: A X_m - X_(m+1) H on the sampled rows: {rel.max():.2e} of the column's largest entry"
    return counts


@pytest.mark.parametrize("which,transpose", OPERATORS, ids=OP_IDS)
@pytest.mark.parametrize("n,m", EDGES, ids=[f"n{n}_m{m}" for n, m in EDGES])
def test_lookahead_against_the_oracle_at_the_edges(fresh, n, m, which, transpose):
    c = fresh()
    counts = _check_against_oracle(c, which, transpose, n, m, f"look-ahead Arnoldi vs oracle ({which}, adjoint={transpose}, n={n}, m={m})")
    if m >= 2:     # (a call of one step is no batch: operator kernel and three sweeps on the host-synchronous schedule)
        assert counts == (1, m, m, 0), f"(sweep 1, sweep 2, sweep 3, operator) launches {counts}: the batch did not look ahead"


@pytest.mark.parametrize("which,transpose", OPERATORS, ids=OP_IDS)
def test_the_pass_is_really_gone(fresh, which, transpose):
    """one m-step call is one batch: sweep 1 runs for its first step only"""
    c = fresh()
    n, m = 6001, 20
    A = _operator(c, which, n)
    _, _, _, counts = _run(c, A, n, m, _x0(n), transpose)
    assert counts == (1, m, m, 0), f"look-ahead: (sweep 1, sweep 2, sweep 3, operator) launches = {counts}"
    c.set_tuning("fuse_rowop", 1)
    _, _, _, three = _run(c, A, n, m, _x0(n), transpose)
    assert three == (m, m, m, 0), f"three sweeps: launches = {three}"


@pytest.mark.parametrize("which,transpose", OPERATORS, ids=OP_IDS)
@pytest.mark.parametrize("n", [n for n, m in EDGES if n >= 3], ids=lambda n: f"n{n}")
def test_y2_and_beta_are_the_tile_sweeps_and_step_2_agrees(fresh, n, which, transpose):
    """two steps in one call, against the same two steps on three sweeps with the tile sweep 3 ("stream_two" = 0).  Step 1 has the same
    inputs on both routes, so x_2 and H(:, 1) -- y'' and beta of the look-ahead sweep -- are byte-equal; for the explicit diagonal they
    are also what lk_dgs leaves for that step on y = D x_1 written out.  Step 2 differs only through its h1 (bar: module docstring)."""
    c = fresh(stream_two=0)
    A = _operator(c, which, n)
    x0 = _x0(n)
    _, Hl, Xl, counts = _run(c, A, n, 2, x0, transpose)
    c.set_tuning("fuse_rowop", 1)
    _, H3, X3, _ = _run(c, A, n, 2, x0, transpose)
    assert counts == (1, 2, 2, 0), f"sweep launches {counts}: no look-ahead"
    assert Xl[:, 1].tobytes() == X3[:, 1].tobytes(), "x_2 (y'' of step 1, normalised) differs from the tile sweep 3's"
    assert Hl[:, 0].tobytes() == H3[:, 0].tobytes(), "H(:, 1) (h and beta of step 1) differs from the tile sweep 3's"
    if which == "d":
        X1, Y = lk.krylov_basis_gpu(n, 1, np.float64, c), lk.krylov_basis_gpu(n, 1, np.float64, c)
        X1.upload(x0.reshape(-1, 1), 0)
        Y.upload((_diag("d", n) * x0).reshape(-1, 1), 0)
        h, norms = np.zeros(1), []
        assert lk.double_gram_schmidt_step(Y[0], X1, if_chk_orthonormal=False, beta=h, _normalize=True, _norms=norms) == 0
        assert h.tobytes() == Hl[:1, 0].tobytes() and np.float64(norms[2]).tobytes() == Hl[1, 0].tobytes(), "lk_dgs gives another h, beta"
        assert Y.download()[:, 0].tobytes() == Xl[:, 1].tobytes(), "lk_dgs gives another x_2"
    nrm = np.linalg.norm(H3[:, 1])
    diff = np.abs(Hl[:, 1] - H3[:, 1]).max()
    print(f"step 2, n={n} {which} adjoint={transpose}: max |dH(:, 2)| = {diff:.3e} = {diff / (EPS * nrm):.2f} ulp of ||H(:, 2)||")
    assert diff <= 4.0 * EPS * nrm, f"H(:, 2) differs from the three-sweep route by {diff / (EPS * nrm):.2f} ulp of its norm (bar 4)"


@pytest.mark.parametrize("which,transpose", OPERATORS, ids=OP_IDS)
@pytest.mark.parametrize("k", [17, 40, 100], ids=lambda k: f"k{k}")
def test_y2_and_beta_are_the_tile_sweeps_with_an_lds_exchange(fresh, k, which, transpose):
    """the same byte comparison where the waves split over the columns (k = 17, 40, 100: 2, 4, 8 wave-columns, shares through the LDS exchange,
    coefficients read from LDS): steps 1 .. k - 1 on three sweeps give one basis; from it, steps k and k + 1 in one call on either route.
    Step k opens the call, so it runs a sweep 1 of its own and has the same inputs on both routes: x_(k+1) and H(:, k) are byte-equal."""
    c = fresh(stream_two=0, fuse_rowop=1)
    n = 4099
    A = _operator(c, which, n)
    X = lk.krylov_basis_gpu(n, k + 2, np.float64, c)
    X.upload(_x0(n).reshape(-1, 1), 0)
    H0 = np.zeros((k + 2, k + 1), order="F")
    assert lk.arnoldi(A, X, H0, transpose=transpose, kend=k - 1) == 0
    start = X.download()
    out = {}
    for fuse in (3, 1):
        c.set_tuning("fuse_rowop", fuse)
        X.upload(np.asfortranarray(start[:, :k]), 0)
        H = H0.copy(order="F")
        c.profile_reset()
        c.profile_enable(True)
        assert lk.arnoldi(A, X, H, transpose=transpose, kstart=k, kend=k + 1) == 0
        c.sync()
        c.profile_enable(False)
        out[fuse] = (H, X.download(), c.profile_get("dgs_sweep1")[0])
    assert (out[3][2], out[1][2]) == (1, 2), f"sweep 1 launches {out[3][2]} with look-ahead, {out[1][2]} on three sweeps"
    assert out[3][1][:, k].tobytes() == out[1][1][:, k].tobytes(), f"x_{k + 1} (y'' of step {k}, normalised) differs from the tile sweep 3's"
    assert out[3][0][:, k - 1].tobytes() == out[1][0][:, k - 1].tobytes(), f"H(:, {k}) differs from the tile sweep 3's"
    nrm = np.linalg.norm(out[1][0][:, k])
    diff = np.abs(out[3][0][:, k] - out[1][0][:, k]).max()
    print(f"step {k + 1}, {which} adjoint={transpose}: max |dH(:, {k + 1})| = {diff / (EPS * nrm):.2f} ulp of its norm")
    assert diff <= 4.0 * EPS * nrm, f"H(:, {k + 1}) differs from the three-sweep route by {diff / (EPS * nrm):.2f} ulp of its norm (bar 4)"


@pytest.mark.parametrize("which,transpose", OPERATORS, ids=OP_IDS)
def test_segments_and_resumption(fresh, which, transpose):
    c = fresh()
    n, m = 5003, 25
    A = _operator(c, which, n)
    x0 = _x0(n)
    _, H1, X1, _ = _run(c, A, n, m, x0, transpose)
    calls = []
    _, Hs, Xs, counts = _run(c, A, n, m, x0, transpose, _segments=(8, 16, 24), _progress=lambda a, b: calls.append((a, b)))
    assert calls and calls[0] == (1, 8)
    assert counts == (1, m, m, 0), f"segmented batch: sweep launches {counts}"
    assert Hs.tobytes() == H1.tobytes() and Xs.tobytes() == X1.tobytes(), "lk_arnoldi_segments differs from lk_arnoldi"
    # two calls: each runs a real sweep 1 at its first step
    X = lk.krylov_basis_gpu(n, m + 1, np.float64, c)
    X.upload(x0.reshape(-1, 1), 0)
    H = np.zeros((m + 1, m), order="F")
    assert lk.arnoldi(A, X, H, transpose=transpose, kend=12) == 0
    assert lk.arnoldi(A, X, H, transpose=transpose, kstart=13, kend=24) == 0
    assert_columns_close(H[:25, :24], _oracle(n, m)[0][:25, :24], f"look-ahead Arnoldi in two calls vs oracle ({which}, adjoint={transpose})")


@pytest.mark.parametrize("which,transpose", OPERATORS, ids=OP_IDS)
def test_breakdown_and_nan_stop_as_on_three_sweeps_and_leave_no_stale_section(fresh, which, transpose):
    c = fresh()
    n, m = 20_011, 12
    marker = seeded(n, np.float64, 123)
    # (a) an operator with 6 distinct eigenvalues: invariant subspace after 6 steps   (b) a NaN in d: step 1 reports it
    d6 = 1.0 + (np.arange(n) % 6).astype(np.float64)
    dnan = _diag("d", n)
    dnan[n // 3] = np.nan
    for name, d, first_marker in (("breakdown", d6, 7), ("nan", dnan, 2)):
        res = {}
        for fuse in (3, 1):
            c.set_tuning("fuse_rowop", fuse)
            X = lk.krylov_basis_gpu(n, m + 1, np.float64, c)
            X.upload(_x0(n, seed=9).reshape(-1, 1), 0)
            for j in range(1, m + 1):
                X.upload(marker.reshape(-1, 1), j)
            H = np.zeros((m + 1, m), order="F")
            if name == "nan":
                with pytest.raises(_capi.LightKrylovHipError, match=r"\[-5\] \|beta\| = NaN detected") as ei:
                    lk.arnoldi(lk.diag_linop_gpu(d, c), X, H, transpose=transpose)
                status = str(ei.value)
            else:
                status = lk.arnoldi(lk.diag_linop_gpu(d, c), X, H, tol=1e-10, transpose=transpose)
                assert status == 6
            Xh = X.download()
            for j in range(first_marker, m + 1):
                assert np.array_equal(Xh[:, j], marker), f"{name}: column {j} behind the stop was touched (fuse_rowop = {fuse})"
            res[fuse] = status
        assert res[3] == res[1], f"{name}: {res[3]!r} with look-ahead, {res[1]!r} on three sweeps"
        # the context goes on: nothing of the stopped batch is consumed by the next one
        c.set_tuning("fuse_rowop", 3)
        _check_against_oracle(c, which, transpose, 2001, 40, f"look-ahead Arnoldi after a {name} on the same context ({which}, adjoint={transpose})")


def test_routing_default_below_the_size_rule_is_the_three_sweep_route(fresh):
    n, m = 4096, 12
    out = {}
    for fuse in (2, 1):
        c = fresh(fuse_rowop=fuse)
        _, H, X, counts = _run(c, _operator(c, "lin", n), n, m, _x0(n))
        out[fuse] = (H.tobytes(), X.tobytes(), counts)
    assert out[2] == out[1] and out[2][2] == (m, m, m, 0)


def test_routing_complex_kind_keeps_three_sweeps(fresh):
    n, m, dtype = 4099, 12, np.complex128
    out = {}
    for fuse in (3, 1):
        c = fresh(fuse_rowop=fuse)
        _, H, X, counts = _run(c, _operator(c, "d", n, dtype), n, m, _x0(n, dtype), dtype=dtype)
        out[fuse] = (H.tobytes(), X.tobytes(), counts)
    assert out[3] == out[1] and out[3][2] == (m, m, m, 0)


def test_routing_one_rank_communicator_keeps_three_sweeps(fresh):
    """with a communicator every sweep's scalars pass through the all-reduce before its finish is read: no look-ahead"""
    n, m = 4099, 12
    c = fresh()
    c.init_native_comm(1, 0, lk.Context.comm_unique_id())
    try:
        _, H, X, counts = _run(c, _operator(c, "lin", n), n, m, _x0(n))
    finally:
        c.destroy_native_comm()
    assert counts == (m, m, m, 0), f"launches {counts}"
    c1 = fresh(fuse_rowop=1)
    _, H1, X1, _ = _run(c1, _operator(c1, "lin", n), n, m, _x0(n))
    assert H.tobytes() == H1.tobytes() and X.tobytes() == X1.tobytes()


def test_default_takes_the_lookahead_at_size():
    """n = 2^25 rows (above the size rule of 8 runs per CU), m = 6, a context nobody tuned"""
    n, m = 1 << 25, 6
    out = {}
    for fuse in (None, 1):
        c = lk.Context(device=0)
        try:
            if fuse is not None:
                c.set_tuning("fuse_rowop", fuse)
            X = lk.krylov_basis_gpu(n, m + 1, np.float64, c)
            X[0].rand(True, seed=7)
            H = np.zeros((m + 1, m), order="F")
            c.profile_reset()
            c.profile_enable(True)
            assert lk.arnoldi(_operator(c, "lin", n), X, H) == 0
            c.sync()
            c.profile_enable(False)
            out[fuse] = (H, tuple(c.profile_get(t)[0] for t in ("dgs_sweep1", "dgs_sweep2", "dgs_sweep3", "matvec")))
            del X
        finally:
            c.close()
    assert out[None][1] == (1, m, m, 0), f"default at n = 2^25: launches {out[None][1]}"
    assert out[1][1] == (m, m, m, 0)
    H, H3 = out[None][0], out[1][0]
    # every column at the bar of the step-2 test (column 1 too: at this size the three-sweep route's sweep 3 is the column walk, whose beta
    # is summed in another order than the tile's)
    for j in range(m):
        diff, nrm = np.abs(H[:, j] - H3[:, j]).max(), np.linalg.norm(H3[:, j])
        print(f"n = 2^25, column {j + 1}: max |dH| = {diff / (EPS * nrm):.2f} ulp of its norm")
        assert diff <= 4.0 * EPS * nrm, f"H(:, {j + 1}) differs from the three-sweep route by {diff / (EPS * nrm):.2f} ulp of its norm (bar 4)"
