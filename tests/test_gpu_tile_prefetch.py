"""Sweep 2 and the look-ahead sweep of the real kind fetch a block's NEXT tile through LDS while they work on the current one
(lk_kernels.hip.h, panel_sweep, PF).  The loop is entered only by a block that walks at least two tiles, which no small-n test gives:
here the grids are pinned to one block per CU ("grid_mult" = 1; sweep 2 has that by default) and n = 3 G T + 1 or 2 G T + 77 rows, G the
CU count and T the tile height of the k at hand (128 rows for k > 64, 256 / 512 / 1024 for k > 32 / > 16 / <= 16), so that some blocks
walk three tiles and some two, or two and one, and the panel ends in a ragged tile that takes the plain loads.  k: a wave with no
columns, with fewer than the look-ahead sweep stages through LDS (15), exactly 15, and all 16 (k = 127: kcw = 16 -- the 16th column
waits in registers); k = 128 for sweep 2 alone (the look-ahead sweep takes k + 1 <= 128).  "resident" = 0 everywhere.

1. y'' and beta of the look-ahead sweep are byte-equal to the three-sweep route's tile sweep 3 (panel_sweep<.., TWO>, "stream_two" = 0),
   which has no prefetch -- after the first step (k = 1) and after late steps.
2. The sums.  (a) Column k + 1 of H from the SECOND step of a look-ahead call (h1 from the look-ahead sums, h2 from sweep 2) against the
   longdouble step on the downloaded basis.  (b) Sweep 2's h2 where it is not rounding noise: lk_dgs on a skewed basis (y loaded: the
   prefetch's path without a row operator), h = h1 + h2 against dgs_longdouble.  Bound, entrywise and a priori: with e1, e2 the
   rounding of the two dot sweeps and eu that of the update, h - h* = (I - X^T X) e1 + X^T eu + e2, so
       |h - h*| <= gamma_m (|X^T X - I| |X|^T |y| + |X|^T (|y| + |X| |h1*|) + |X|^T |y'*| + |h*|),   m = n + k + 16
   (n terms per dot, k + 2 per update row, the look-ahead's three extra roundings per term -- d y'' formed before the division by beta --,
   two for d_i of the generated operator, the final addition; first order, the slack of 16 covers the second) -- check_entrywise.
3. Columns behind the last step keep their marker bytes, and on a caller-owned panel with NaN padding no word outside the panel's rows
   changes (CallerPanel.get asserts it)."""
import numpy as np
import pytest

import lightkrylov_amd as lk
from tests._gpu_helpers import (CallerPanel, _step_bound, check_entrywise, device_num_cu, dgs_longdouble, seeded, skewed_basis)

pytestmark = pytest.mark.gpu

OPERATORS = [("lin", False), ("d", False), ("d", True)]
OP_IDS = ["linspace", "d", "d_adjoint"]
KS = [1, 16, 17, 33, 65, 100, 113, 120, 127]        # kcw = 13 (k = 100), 15 (k = 113, 120: the staged count exactly), 16 (k = 127)


def tile_rows(k):
    return 128 if k > 64 else 256 if k > 32 else 512 if k > 16 else 1024


def rows(k, which, G):
    """three tiles for some blocks and two for the others, or two and one; a ragged last tile either way"""
    return 3 * G * tile_rows(k) + 1 if which % 2 == 0 else 2 * G * tile_rows(k) + 77


@pytest.fixture()
def fresh():
    ctxs = []

    def make(**kw):
        c = lk.Context(device=0)
        for key, val in dict(dict(resident=0, stream_two=0, fuse_rowop=1, grid_mult=1), **kw).items():
            c.set_tuning(key, val)
        ctxs.append(c)
        return c
    yield make
    for c in ctxs:
        c.close()


def _diag(n):
    return 1.0 + np.arange(n) / n


def _operator(c, which, n):
    if which == "lin":
        return lk.diag_linop_gpu(n_local=n, row0=0, d0=1.0, dstep=1.0 / n, ctx=c)
    return lk.diag_linop_gpu(_diag(n), c)


_START = {}


def _start(c, n, k):
    """an orthonormal basis of k columns (Arnoldi steps 1 .. k - 1 on three sweeps) and H so far: once per shape, read-only"""
    if (n, k) not in _START:
        X = lk.krylov_basis_gpu(n, k + 3, np.float64, c)
        x0 = seeded(n, np.float64, 7)
        X.upload((x0 / np.linalg.norm(x0)).reshape(-1, 1), 0)
        H0 = np.zeros((k + 3, k + 2), order="F")            # (the engine call takes H of the basis's k + 3 columns)
        if k > 1:
            assert lk.arnoldi(_operator(c, "lin", n), X, H0, kend=k - 1) == 0
        S = np.asfortranarray(X.download()[:, :k])
        S.setflags(write=False)
        H0.setflags(write=False)
        if len(_START) >= 2:                            # (the two row counts of one k at a time: the largest start is 100 MB)
            _START.clear()
        _START[(n, k)] = (S, H0)
    return _START[(n, k)]


def _two_steps(c, A, B, H0, k, transpose, fuse):
    c.set_tuning("fuse_rowop", fuse)
    H = H0.copy(order="F")
    c.profile_reset()
    c.profile_enable(True)
    span = dict(kstart=k, kend=k + 1) if k > 1 else dict(kend=2)        # (the first two steps: a call from the start vector)
    assert lk.arnoldi(A, B, H, transpose=transpose, **span) == 0
    c.sync()
    c.profile_enable(False)
    return H, c.profile_get("dgs_sweep1")[0]


@pytest.mark.parametrize("idx,op", list(enumerate(OPERATORS)), ids=OP_IDS)
@pytest.mark.parametrize("k", KS, ids=lambda k: f"k{k}")
def test_lookahead_sweep_on_blocks_of_several_tiles(fresh, k, idx, op):
    which, transpose = op
    c = fresh()
    n = rows(k, idx + KS.index(k), device_num_cu(c))    # (every operator meets both row counts, on neighbouring k)
    S, H0 = _start(c, n, k)
    A = _operator(c, which, n)
    marker = seeded(n, np.float64, 123)
    out = {}
    for fuse in (3, 1):
        X = lk.krylov_basis_gpu(n, k + 3, np.float64, c)
        X.upload(np.asfortranarray(S), 0)
        X.upload(marker.reshape(-1, 1), k + 2)
        H, s1 = _two_steps(c, A, X, H0, k, transpose, fuse)
        out[fuse] = (H, X.download(), s1)
        del X
    assert (out[3][2], out[1][2]) == (1, 2), f"sweep 1 launches {out[3][2]} with look-ahead, {out[1][2]} on three sweeps"
    (Hl, Xl, _), (H3, X3, _) = out[3], out[1]
    assert Xl[:, k].tobytes() == X3[:, k].tobytes(), f"x_{k + 1} (y'' of step {k}, normalised) differs from the tile sweep 3's"
    assert Hl[:, k - 1].tobytes() == H3[:, k - 1].tobytes(), f"H(:, {k}) (h and beta of step {k}) differs from the tile sweep 3's"
    for name, Xg in (("look-ahead", Xl), ("three sweeps", X3)):
        assert Xg[:, k + 2].tobytes() == marker.tobytes(), f"{name}: the column behind the last step was touched"
        assert Xg[:, :k].tobytes() == S.tobytes(), f"{name}: a column of the basis the call started from changed"
    # 2 (a): step k + 1 of the look-ahead call from the basis as the device holds it
    Xd = Xl[:, :k + 1]
    href, scale = _step_bound(Xd, _diag(n) * Xd[:, k])
    check_entrywise(Hl[:k + 1, k], href, scale, n + k + 16, False, f"H(:{k + 1}, {k + 1}) of the look-ahead's second step, n = {n}")


@pytest.mark.parametrize("k", [17, 100], ids=lambda k: f"k{k}")
def test_lookahead_sweep_on_the_default_grid_and_a_caller_owned_panel(fresh, k):
    """two blocks per CU for the look-ahead sweep (one resident: the second half of the grid starts as the first ends), on a panel with
    NaN padding behind every column"""
    c = fresh(grid_mult=2)
    n = rows(k, 0, device_num_cu(c))
    n += n % 2                                          # (a real panel's ld is even; n even keeps the padding at three or four rows)
    S, H0 = _start(c, n, k)
    A = _operator(c, "d", n)
    marker = seeded(n, np.float64, 123)
    out = {}
    for fuse in (3, 1):
        P = CallerPanel(c, np.float64, n, k + 3, "nan_pad")
        P.set(np.concatenate([S, np.zeros((n, 2)), marker.reshape(-1, 1)], axis=1))
        H, s1 = _two_steps(c, A, P.B, H0, k, False, fuse)
        out[fuse] = (H, P.get(f"look-ahead call, fuse_rowop = {fuse}"), s1)
        del P
    assert out[3][1][:, k].tobytes() == out[1][1][:, k].tobytes() and out[3][0][:, k - 1].tobytes() == out[1][0][:, k - 1].tobytes()
    assert out[3][1][:, k + 2].tobytes() == marker.tobytes(), "the column behind the last step was touched"
    assert out[3][2] == 1, f"sweep 1 launches {out[3][2]} with look-ahead"


@pytest.mark.parametrize("k,which", [(17, 1), (100, 1), (128, 0)], ids=["k17", "k100", "k128"])
def test_sweep_2_sums_a_real_second_pass_on_blocks_of_several_tiles(fresh, k, which):
    c = fresh()
    n = rows(k, which, device_num_cu(c))
    X = skewed_basis(n, k, np.float64, 40 + k)
    y = seeded(n, np.float64, 5000 + k)
    href, scale = _step_bound(X, y)
    h2 = dgs_longdouble(y, X)[1]
    assert np.abs(h2).max() >= 1e-6 * np.linalg.norm(y), "the second pass has nothing to do on this input"
    Xg, Yg = lk.krylov_basis_gpu(n, k, np.float64, c), lk.krylov_basis_gpu(n, 1, np.float64, c)
    Xg.upload(X, 0)
    Yg.upload(y.reshape(-1, 1), 0)
    h = np.zeros(k)
    c.profile_reset()
    c.profile_enable(True)
    assert lk.double_gram_schmidt_step(Yg[0], Xg, if_chk_orthonormal=False, beta=h) == 0
    c.sync()
    c.profile_enable(False)
    assert c.profile_get("dgs_sweep2")[0] == 1, "lk_dgs did not run its three sweeps"
    check_entrywise(h, href, scale, n + k + 16, False, f"h = h1 + h2 of lk_dgs on a skewed basis, n = {n}, k = {k}")
    assert np.array_equal(Xg.download(), X), "lk_dgs changed the basis"
