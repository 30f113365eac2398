"""The real kind's long-panel sweep shape, on panels of a few thousand rows.

sweepm (lk_engine.hip) moves sweeps 2 and 3 of a real step with 33 <= k <= 128 from 16-column to 32-column register tiles when the GLOBAL
row count is at least 2^25: panel_sweep<false, 32, 8, true, true, false, 1, 1>, <false, 32, 8, true, false, true, 1, 1> and the column walk
panel_update<false, 32, 8, true>, with WC = 2 wave-columns and four row groups per block for k <= 64 (tiles of 512 rows), WC = 4 and two row
groups beyond (tiles of 256 rows).  The wide-basis tests run the same instances with WC = 8 and ONE row group, so the wide tile's own code
(scalar-base addressing, one accumulator per column) together with a second row group exists on this shape only -- the shape of every
step at the headline size.  The size that decides is the one the host announced with lk_set_partition where it announced one, so a
one-rank context with set_partition(0, 2^25) runs the long shape on any panel: every test here has such a context and a second one with the
same tuning that announced nothing (the control, on 16-column tiles).  "resident" = 0 everywhere: the three sweeps.

Inputs are the skewed panels of tests/test_gpu_second_pass.py (h2 is about 1e-3 |y|, not noise).  Shapes: k on both sides of every change
of (WC, kcw) -- 33 (groups of 17 and 16), 48, 64 (both groups full), 65 (17, 17, 17, 14), 96, 97 (last group 22), 127, 128 (every slot) and
the control k = 32; n = 1 and 127 (one row group), the tile edges 255 / 256 / 257 (k >= 65) and 511 / 512 / 513 (k <= 64), the column walk's
run of 8192 rows (8191, 8193), and 2 G T + 77 rows at "grid_mult" = 1 (G the CU count, T the tile height: blocks walk two tiles or three and
the last tile is ragged).

Bounds, none of them new:
  h = h1 + h2   entrywise against dgs_longdouble under the a-priori bound tests/test_gpu_tile_prefetch.py derives (step_bound_from,
                check_entrywise, m = n + k + 16)
  y''           max |got - ref| <= RTOL |y| (tests/_tol.py, 1e-12) against the longdouble y'' and against the oracle's, as
                tests/test_gpu_second_pass.py::check holds it
  ||y''||       1e-12 relative to the longdouble norm of the y'' the call returned
  bytes         y'' and h of "stream_two" = 0 and 1 are equal (the contract of tests/test_gpu_stream_two.py, here on the 32-column tile);
                X is bit-identical after every call
Route witness: at k = 32 the two contexts return the same bytes; for k > 32 and n >= 4097 at least one double of (h, y'') differs between
them -- the shapes add the columns' shares in different orders, so equality of every entry would mean the long shape did not run.  (lk_dgs
returns h1 + h2 only, and h1 comes from sweep 1, which is not routed by size: it is y'' that tells.)

Beside lk_dgs (a, b): sweep 2 with its store on ("recompute_update" = 0) and as the lazy path's fused update + dots (c); lk_arnoldi on a
diagonal operator formed inside the sweeps ("fuse_rowop" = 1) against the operator kernel's route, byte for byte, each new column of H
and y'' = beta x_(k+1) against the longdouble step on the basis as the device holds it (d); a look-ahead batch whose last step runs on the
long shape (e); a caller-owned panel with NaN padding and a NaN in the second row group (f); two emulated ranks (g).

The one-row panels.  At n = 1 no near-orthonormal panel of k > 1 columns exists: skewed_basis returns unit columns, every entry +-1, and
the two passes return y'' = (k - 1)^2 y exactly -- 1024 |y| at k = 33, 4096 |y| at k = 65.  The oracle's own y'' is 6.5e-13 |y| (k = 33) and
2.1e-12 |y| (k = 65) from the longdouble one there (measured on the host, no GPU involved), so no result can be within 1e-12 |y| of both
references at k = 65.  The scale of the y'' comparison is therefore max(|y|, max |y''| of the longdouble reference): |y| on every panel
with n >= k (there max |y''| < |y|), the size of the result on the two one-row panels.  Every other assertion is the same at n = 1."""
import functools

import numpy as np
import pytest

import lightkrylov_amd as lk
from lightkrylov_amd import _capi
from oracle import oracle as ora
from tests._gpu_helpers import (CallerPanel, _sharded, assert_second_pass_matters, check_entrywise, device_num_cu, dgs_longdouble,
                                second_pass_input, seeded, step_bound_from)
from tests._tol import assert_close

pytestmark = pytest.mark.gpu

ANNOUNCED = 1 << 25              # the global row count from which sweepm takes the 32-column tiles
RTOL_NORM = 1e-12                # tests/test_gpu_parity.py: |norm - reference| <= 1e-12 * reference
WITNESS_ROWS = 4097              # from this many rows on, two summation orders cannot agree in every bit of y''
MULTI = "multi"                  # 2 G T + 77 rows

# (k, n): every k meets a tile edge of its WC and the multi-tile panel, every n both values of WC
A_CASES = [(32, 513), (32, 8193),
           (33, 1), (33, 511), (33, 8191), (33, MULTI),
           (48, 127), (48, 512), (48, 8193), (48, MULTI),
           (64, 513), (64, 8191), (64, MULTI),
           (65, 1), (65, 255), (65, 8193), (65, MULTI),
           (96, 127), (96, 256), (96, MULTI),
           (97, 257), (97, 8191), (97, MULTI),
           (127, 255), (127, 8193), (127, MULTI),
           (128, 256), (128, 257), (128, 8191), (128, MULTI)]


def tile_rows(k):
    """rows of a block's tile on the long shape: 8 / WC row groups of 128 rows"""
    return 512 if k <= 64 else 256


def rows(k, n, c):
    return 2 * device_num_cu(c) * tile_rows(k) + 77 if n == MULTI else n


_CTXS = {}


def pair(**kw):
    """(announced, control) contexts with one tuning set, once per module"""
    key = tuple(sorted(dict(dict(resident=0), **kw).items()))
    if key not in _CTXS:
        made = []
        for announce in (True, False):
            c = lk.Context(device=0)
            for name, val in key:
                c.set_tuning(name, val)
            if announce:
                c.set_partition(0, ANNOUNCED)
            made.append(c)
        _CTXS[key] = tuple(made)
    return _CTXS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for cs in _CTXS.values():
        for c in cs:
            c.close()
    _CTXS.clear()
    case.cache_clear()
    _START.clear()


@functools.lru_cache(maxsize=3)
def case(n, k):
    """X, y and the references of one step, read-only: h* and the scale of its entrywise bound, y'' in longdouble, h and y'' of the oracle"""
    X, Y = second_pass_input(n, k, np.float64, "skew_rand")
    y = Y[:, 0].copy()
    h1, h2, y1, y2 = dgs_longdouble(y, X)
    if 4 * k <= n <= 10_000:
        assert_second_pass_matters(h1, h2, y)
    href, scale = step_bound_from(X, y, h1, h2, y1)
    yo = y.copy()
    ho, _ = ora.double_gram_schmidt_step(yo, X.copy(order="F"))
    ynorm = float(np.linalg.norm(y))
    ref = dict(X=X, y=y, href=href, scale=scale, y2=y2, ho=np.asarray(ho).reshape(k), yo=yo, ynorm=ynorm,
               yscale=max(ynorm, float(np.abs(y2).max())))         # (the module docstring: |y| wherever n >= k)
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref


def step(c, B, k, y, two=0):
    """lk_dgs of y (uploaded into column k) against columns 0 .. k - 1 of B with "stream_two" = two: h, y'', ||y''||"""
    c.set_tuning("stream_two", two)
    B.upload(y.reshape(-1, 1), k)
    h = np.zeros(k)
    norms = []
    assert lk.double_gram_schmidt_step(B[k], B[:k], False, beta=h, _norms=norms) == 0
    return h, B.download(k, 1)[:, 0], norms[2]


def check_refs(label, got, ref):
    h, y2, nrm = got
    n, k = ref["X"].shape
    check_entrywise(h, ref["href"], ref["scale"], n + k + 16, False, f"{label}: h = h1 + h2")
    assert_close(y2, ref["y2"], f"{label}: y'' / longdouble", scale=ref["yscale"])
    assert_close(y2, ref["yo"], f"{label}: y'' / oracle", scale=ref["yscale"])
    yl = y2.astype(np.longdouble)
    want = float(np.sqrt(np.sum(yl * yl)))
    print(f"{label}: ||y''|| {nrm!r} longdouble {want!r}")
    assert abs(nrm - want) <= RTOL_NORM * want, f"{label}: ||y''|| off by {abs(nrm - want) / max(want, 1e-300):.2e}"


def same_bytes(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def witness(label, k, n, long_out, ctl_out):
    """the module docstring's route witness"""
    if k <= 32:
        assert same_bytes(long_out, ctl_out), f"{label}: k = {k} must not be routed by size"
    elif n >= WITNESS_ROWS:
        differ = int(np.count_nonzero(long_out[1] != ctl_out[1])) + int(np.count_nonzero(long_out[0] != ctl_out[0]))
        print(f"{label}: {differ} doubles of (h, y'') differ between the announced and the control context")
        assert differ > 0, f"{label}: every bit agrees with the 16-column route -- the long shape did not run"


# ---- a, b. lk_dgs on both sweep-3 routes, and the route witness -------------------------------------------------------------------------
@pytest.mark.parametrize("k,n", A_CASES, ids=[f"k{k}-n{n}" for k, n in A_CASES])
def test_dgs_on_the_long_shape_against_references(k, n):
    long, ctl = pair(grid_mult=1) if n == MULTI else pair()
    n = rows(k, n, long)
    ref = case(n, k)
    label = f"long shape n = {n} k = {k}"
    B = lk.krylov_basis_gpu(n, k + 1, np.float64, long)
    B.upload(ref["X"], 0)
    tile = step(long, B, k, ref["y"], 0)
    walk = step(long, B, k, ref["y"], 1)
    assert B.download(0, k).tobytes() == np.asfortranarray(ref["X"]).tobytes(), f"{label}: X is read only"
    del B
    assert tile[0].tobytes() == walk[0].tobytes(), f"{label}: h differs between the tile kernel and the column walk"
    assert tile[1].tobytes() == walk[1].tobytes(), (f"{label}: y'' differs between the tile kernel and the column walk "
                                                    f"({np.count_nonzero(tile[1] != walk[1])} of {n} entries)")
    check_refs(label + " tile", tile, ref)
    check_refs(label + " column walk", walk, ref)
    Bc = lk.krylov_basis_gpu(n, k + 1, np.float64, ctl)
    Bc.upload(ref["X"], 0)
    control = step(ctl, Bc, k, ref["y"], 0)
    del Bc
    check_refs(label + " control", control, ref)
    witness(label, k, n, tile, control)


# ---- c. the first-pass store and the single-coefficient partner ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [33, 65, 128], ids=lambda k: f"k{k}")
def test_sweep_2_stores_y1_on_the_long_shape(k):
    """"recompute_update" = 0: sweep 2 writes y' from the 32-column tile (store = 1), sweep 3 is the 16-column panel_update<.., false>"""
    long, ctl = pair(recompute_update=0)
    n = 4099
    ref = case(n, k)
    label = f"long shape, y' stored, n = {n} k = {k}"
    out = []
    for c in (long, ctl):
        B = lk.krylov_basis_gpu(n, k + 1, np.float64, c)
        B.upload(ref["X"], 0)
        out.append(step(c, B, k, ref["y"], 0))
        assert B.download(0, k).tobytes() == np.asfortranarray(ref["X"]).tobytes(), f"{label}: X is read only"
        del B
    check_refs(label, out[0], ref)
    check_refs(label + " control", out[1], ref)
    witness(label, k, n, out[0], out[1])


def test_lazy_fused_update_and_dots_on_the_long_shape():
    """"lazy" = 1: y.sub(X a) followed by the norm and the dots against X is ONE sweep 2 with store = 1 (fused_sub_with_dots), driven as
    tests/test_gpu_lazy_fuzz.py drives it.  a = h1 rounded to double, so that the dots are a real second pass."""
    long, ctl = pair(lazy=1)
    n, k = 4099, 65
    ref = case(n, k)
    X, y = ref["X"], ref["y"]
    Xl, yl = X.astype(np.longdouble), y.astype(np.longdouble)
    a = np.asarray(Xl.T @ yl).astype(np.float64)
    y1 = yl - Xl @ a.astype(np.longdouble)
    d = Xl.T @ y1
    Xa = np.abs(X)
    # y1' = y1 + eu, |eu| <= gamma_(k+2) (|y| + |X| |a|); dots' = X^T y1' + e2, |e2| <= gamma_n |X|^T |y1'|
    scale = Xa.T @ (np.abs(y) + Xa @ np.abs(a)) + Xa.T @ np.abs(y1).astype(np.float64)
    out = []
    for c in (long, ctl):
        label = f"lazy fused sweep on the {'long shape' if c is long else 'control'} n = {n} k = {k}"
        B = lk.krylov_basis_gpu(n, k + 1, np.float64, c)
        B.upload(X, 0)
        B.upload(y.reshape(-1, 1), k)
        T = lk.dense_vector_gpu(n, np.float64, c)
        before = c.lazy_fusion_stats()
        T.zero()
        for j in range(k):
            T.axpby(float(a[j]), B[j], 1.0)
        B[k].axpby(-1.0, T, 1.0)
        nrm = B[k].norm()
        dots = np.array([B[j].dot(B[k]) for j in range(k)])
        after = c.lazy_fusion_stats()
        assert after[0] - before[0] == 1, f"{label}: no fused update + dot sweep ran {before} -> {after}"
        got = B.download()
        assert got[:, :k].tobytes() == np.asfortranarray(X).tobytes(), f"{label}: X is read only"
        assert_close(got[:, k], y1, f"{label}: y - X a / longdouble", scale=ref["ynorm"])
        check_entrywise(dots, d, scale, n + k + 16, False, f"{label}: X^T (y - X a)")
        g = got[:, k].astype(np.longdouble)
        want = float(np.sqrt(np.sum(g * g)))
        assert abs(nrm - want) <= RTOL_NORM * want, f"{label}: norm off by {abs(nrm - want) / want:.2e}"
        out.append((dots, got[:, k]))
        del T, B
    witness(f"lazy fused sweep n = {n} k = {k}", k, n, out[0], out[1])


# ---- d. the fused row operator on the 32-column tile --------------------------------------------------------------------------------------
OPERATORS = [("lin", False), ("d", False), ("d", True)]
OP_IDS = ["linspace", "d", "d_adjoint"]


def _diag(n):
    return 1.0 + np.arange(n) / n


def _operator(c, which, n):
    if which == "lin":
        return lk.diag_linop_gpu(n_local=n, row0=0, d0=1.0, dstep=1.0 / n, ctx=c)
    return lk.diag_linop_gpu(_diag(n), c)


_START = {}


def _start(c, n, k):
    """an orthonormal basis of k columns (Arnoldi steps 1 .. k - 1 on the control context) and H so far: once per shape, read-only"""
    if (n, k) not in _START:
        X = lk.krylov_basis_gpu(n, k + 4, np.float64, c)
        x0 = seeded(n, np.float64, 7)
        X.upload((x0 / np.linalg.norm(x0)).reshape(-1, 1), 0)
        H0 = np.zeros((k + 4, k + 3), order="F")
        assert lk.arnoldi(_operator(c, "lin", n), X, H0, kend=k - 1) == 0
        S = np.asfortranarray(X.download()[:, :k])
        S.setflags(write=False)
        H0.setflags(write=False)
        if len(_START) >= 2:
            _START.clear()
        _START[(n, k)] = (S, H0)
    return _START[(n, k)]


def _steps(c, A, S, H0, k, kend, transpose, marker):
    """lk_arnoldi from step k to kend on a basis that starts as S, a marker column behind the last step; H, the basis, sweep 1 launches"""
    n = S.shape[0]
    X = lk.krylov_basis_gpu(n, H0.shape[0], np.float64, c)
    X.upload(np.asfortranarray(S), 0)
    X.upload(marker.reshape(-1, 1), kend + 1)
    H = H0.copy(order="F")
    c.profile_reset()
    c.profile_enable(True)
    assert lk.arnoldi(A, X, H, kstart=k, kend=kend, transpose=transpose) == 0
    c.sync()
    c.profile_enable(False)
    got = X.download()
    assert got[:, :k].tobytes() == S.tobytes(), "a column of the basis the call started from changed"
    assert got[:, kend + 1].tobytes() == marker.tobytes(), "the column behind the last step was touched"
    return H, got, c.profile_get("dgs_sweep1")[0]


def _check_columns(label, H, X, k, kend):
    """column j of H, j = k .. kend, against the longdouble step on the basis as the device holds it"""
    n = X.shape[0]
    for j in range(k, kend + 1):
        Xd = X[:, :j]
        y = _diag(n) * Xd[:, j - 1]
        h1, h2, y1, y2 = dgs_longdouble(y, Xd)
        href, scale = step_bound_from(Xd, y, h1, h2, y1)
        check_entrywise(H[:j, j - 1], href, scale, n + j + 16, False, f"{label}: H(:{j}, {j})")
        # y'' = beta x_(j+1) as the step left it (two more roundings of 2^-53 |y''| each), held as lk_dgs's y'' is held above
        assert_close(H[j, j - 1] * X[:, j], y2, f"{label}: H({j + 1}, {j}) x_{j + 1} / longdouble y''", scale=float(np.linalg.norm(y)))


@pytest.mark.parametrize("which,transpose", OPERATORS, ids=OP_IDS)
@pytest.mark.parametrize("k", [33, 64, 65, 127], ids=lambda k: f"k{k}")
def test_fused_row_operator_on_the_long_shape(k, which, transpose):
    """"fuse_rowop" = 1: sweeps 2 and 3 form y = D x_k themselves on the 32-column tile; 0: the operator kernel writes y.  Same bytes."""
    n = 4099
    kend = k if k == 127 else k + 1
    marker = seeded(n, np.float64, 123)
    out = {}
    for fuse in (1, 0):
        long, ctl = pair(fuse_rowop=fuse)
        S, H0 = _start(ctl, n, k)
        out[fuse] = _steps(long, _operator(long, which, n), S, H0, k, kend, transpose, marker)
    control = _steps(ctl, _operator(ctl, which, n), S, H0, k, kend, transpose, marker)          # ("fuse_rowop" = 0, 16-column tiles)
    (Hf, Xf, _), (H0_, X0_, _) = out[1], out[0]
    label = f"long shape, fused {which} (adjoint = {transpose}) n = {n} k = {k}"
    for j in range(k, kend + 1):
        assert Hf[:, j - 1].tobytes() == H0_[:, j - 1].tobytes(), f"{label}: H(:, {j}) differs from the operator kernel's route"
        assert Xf[:, j].tobytes() == X0_[:, j].tobytes(), f"{label}: x_{j + 1} differs from the operator kernel's route"
    _check_columns(label, Hf, Xf, k, kend)
    _check_columns(label + " control", control[0], control[1], k, kend)
    witness(label, k, n, (Hf[:, k - 1], Xf[:, k]), (control[0][:, k - 1], control[1][:, k]))


# ---- e. a look-ahead batch that ends on the long shape ------------------------------------------------------------------------------------
def test_lookahead_batch_ends_on_the_long_shape():
    """"fuse_rowop" = 3, steps 40 .. 42: steps 40 and 41 look ahead on 16-column tiles, step 42 takes its h1 from the look-ahead sums, skips
    sweep 1 and runs sweeps 2 and 3 on 32-column tiles."""
    long, ctl = pair(fuse_rowop=3, grid_mult=1)
    k, kend = 40, 42
    n = 2 * device_num_cu(long) * 256 + 77
    S, H0 = _start(ctl, n, k)
    marker = seeded(n, np.float64, 123)
    H, X, s1 = _steps(long, _operator(long, "d", n), S, H0, k, kend, False, marker)
    Hc, Xc, s1c = _steps(ctl, _operator(ctl, "d", n), S, H0, k, kend, False, marker)
    assert (s1, s1c) == (1, 1), f"sweep 1 launches {s1} (announced), {s1c} (control): steps 41 and 42 must skip it"
    label = f"look-ahead batch ending on the long shape n = {n}"
    _check_columns(label, H, X, k, kend)
    _check_columns(label + " control", Hc, Xc, k, kend)
    for j in (k, k + 1):                                  # the steps that look ahead keep the 16-column tiles: the control's bytes
        assert X[:, j].tobytes() == Xc[:, j].tobytes() and H[:, j - 1].tobytes() == Hc[:, j - 1].tobytes(), \
            f"{label}: step {j} looks ahead and must not be routed by size"
    witness(label, kend, n, (H[:, kend - 1], X[:, kend]), (Hc[:, kend - 1], Xc[:, kend]))


# ---- f. caller-owned memory and non-finite input ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [65, 128], ids=lambda k: f"k{k}")
def test_long_shape_on_a_caller_owned_panel(k):
    """a panel with NaN padding behind every column, last tile ragged: CallerPanel.get asserts that no word outside the rows changed"""
    long, ctl = pair()
    n = 4100
    ref = case(n, k)
    out = {}
    for two in (0, 1):
        P = CallerPanel(long, np.float64, n, k + 1, "nan_pad")
        P.set(np.concatenate([ref["X"], ref["y"].reshape(-1, 1)], axis=1))
        long.set_tuning("stream_two", two)
        h = np.zeros(k)
        norms = []
        assert lk.double_gram_schmidt_step(P.B[k], P.B[:k], False, beta=h, _norms=norms) == 0
        got = P.get(f"long shape on a caller panel, stream_two = {two}")
        assert got[:, :k].tobytes() == np.asfortranarray(ref["X"]).tobytes(), "X is read only"
        out[two] = (h, got[:, k].copy(), norms[2])
        check_refs(f"long shape on a caller panel n = {n} k = {k} stream_two = {two}", out[two], ref)
        del P
    assert same_bytes(out[0], out[1]), "the tile kernel and the column walk differ on a caller panel"
    Bc = lk.krylov_basis_gpu(n, k + 1, np.float64, ctl)
    Bc.upload(ref["X"], 0)
    witness(f"caller panel n = {n} k = {k}", k, n, out[0], step(ctl, Bc, k, ref["y"], 0))


def _outcome(c, X, y, k, two):
    """what lk_dgs makes of the input: the error's text, or (h, y'') where it returns"""
    B = lk.krylov_basis_gpu(X.shape[0], k + 1, np.float64, c)
    B.upload(X, 0)
    try:
        h, y2, _nrm = step(c, B, k, y, two)
        return None, np.isnan(h), np.isnan(y2)
    except _capi.LightKrylovHipError as exc:
        return str(exc), None, np.isnan(B.download(k, 1)[:, 0])


@pytest.mark.parametrize("k", [65, 128], ids=lambda k: f"k{k}")
def test_nan_in_the_second_row_group_surfaces_as_on_the_control(k):
    """one NaN in y at row 200 of the fourth tile (the second row group of a block holds rows 128 .. 255 of a tile)"""
    long, ctl = pair()
    n = 4100
    ref = case(n, k)
    y = ref["y"].copy()
    y[3 * 256 + 200] = np.nan
    want = _outcome(ctl, ref["X"], y, k, 0)
    assert want[0] is not None or (want[1].all() and want[2].all()), "the control neither raised nor returned NaN"
    for two in (0, 1):
        got = _outcome(long, ref["X"], y, k, two)
        assert got[0] == want[0], f"stream_two = {two}: the long shape reports {got[0]!r}, the control {want[0]!r}"
        assert (got[1] is None) == (want[1] is None) and (got[1] is None or np.array_equal(got[1], want[1]))
        assert np.array_equal(got[2], want[2]), f"stream_two = {two}: NaN in other rows of y than on the control"
    # and a clean step on the same contexts afterwards
    B = lk.krylov_basis_gpu(n, k + 1, np.float64, long)
    B.upload(ref["X"], 0)
    check_refs(f"clean step after the NaN n = {n} k = {k}", step(long, B, k, ref["y"], 0), ref)


# ---- g. two emulated ranks ----------------------------------------------------------------------------------------------------------------
def test_two_emulated_ranks_take_the_long_shape_together():
    n, k = 5003, 65
    ref = case(n, k)
    X, y = ref["X"], ref["y"]

    def body(rank, c, row0, nl):
        c.set_tuning("resident", 0)
        out = []
        for announce in (False, True):                     # (_sharded announced the panel's own 5003 rows)
            if announce:
                c.set_partition(row0, ANNOUNCED)
            B = lk.krylov_basis_gpu(nl, k + 1, np.float64, c)
            B.upload(np.asfortranarray(X[row0:row0 + nl]), 0)
            out.append(step(c, B, k, y[row0:row0 + nl], 0))
            assert B.download(0, k).tobytes() == np.asfortranarray(X[row0:row0 + nl]).tobytes(), "X is read only"
            del B
        return out

    res, grp = _sharded(n, 2, body)
    assert grp.rank_calls[0] == grp.rank_calls[1] and grp.calls >= 6, (grp.rank_calls, grp.calls)
    for i, name in enumerate(("control", "announced")):
        h = res[0][i][0]
        assert res[1][i][0].tobytes() == h.tobytes(), f"{name}: the ranks hold different h"
        label = f"two ranks, {name}, n = {n} k = {k}"
        check_entrywise(h, ref["href"], ref["scale"], n + k + 16, False, f"{label}: h = h1 + h2")
        ys = np.concatenate([res[r][i][1] for r in range(2)])
        assert_close(ys, ref["y2"], f"{label}: y'' / longdouble", scale=ref["ynorm"])
        assert_close(ys, ref["yo"], f"{label}: y'' / oracle", scale=ref["ynorm"])
        assert res[0][i][2] == res[1][i][2], f"{name}: the ranks hold different norms"
        yl = ys.astype(np.longdouble)
        want = float(np.sqrt(np.sum(yl * yl)))
        assert abs(res[0][i][2] - want) <= RTOL_NORM * want, f"{label}: ||y''|| off by {abs(res[0][i][2] - want) / want:.2e}"
    for r in range(2):
        differ = int(np.count_nonzero(res[r][0][1] != res[r][1][1]))
        print(f"rank {r}: {differ} of {res[r][0][1].size} entries of y'' differ between the announced and the un-announced run")
        assert differ > 0, f"rank {r} did not take the long shape"
