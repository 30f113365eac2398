"""Recovery from a single-launch Gram-Schmidt step that gives up (csrc/lk_resident.hip.h) on every entry that enqueues one.

A launch whose first grid-wide wait times out writes status 1 into its result slot, raises the device stop flag and raises the context's
abort word; the host redoes the step on the three-sweep schedule and clears the word (resident_recover).  These cases reach that path
somewhere else than the first step of a batch -- on a look-ahead step of a cancelled segmented batch (whose slot nobody reads), in the
middle of a batch whose segments were already delivered, inside block Arnoldi / qr_no_pivoting -- and then use the same context again.
`resident_spin_ms` = 0 is the designed way in: the launch gives up at its first wait without waiting.  Every result is compared with the
oracle (1e-12, normwise per column), and the context's counters show that single launches ran and that the give-up was seen."""
import functools

import numpy as np
import pytest

import lightkrylov_amd as lk
from oracle import oracle as ora
from tests._gpu_helpers import KINDS, basis, orthonormal_basis, seeded

pytestmark = pytest.mark.gpu
RTOL = 1e-12
LOOKAHEAD = 24          # steps the engine keeps enqueued beyond the segment it waits for (SEG_LOOKAHEAD in lk_engine.hip)


def _diag(n, dtype, phase):
    d = 1.0 + np.arange(n) / n
    if dtype is np.complex128:
        return d * np.exp(phase * 1j * np.arange(n) / n)
    return d.astype(dtype)


def _start(n, dtype, seed):
    x0 = seeded(n, dtype, seed)
    return x0 / np.linalg.norm(x0)


@functools.lru_cache(maxsize=None)
def _oracle_arnoldi(n, m, dtype, phase, seed):
    Xo = np.zeros((n, m + 1), dtype=dtype, order="F")
    Xo[:, 0] = _start(n, dtype, seed)
    Ho = np.zeros((m + 1, m), dtype=dtype, order="F")
    assert ora.arnoldi(ora.DiagOp(_diag(n, dtype, phase)), Xo, Ho) == 0
    return Ho


@functools.lru_cache(maxsize=None)
def _oracle_lanczos(n, m, dtype, seed):
    Xo = np.zeros((n, m + 1), dtype=dtype, order="F")
    Xo[:, 0] = _start(n, dtype, seed)
    To = np.zeros((m + 1, m), dtype=dtype, order="F")
    assert ora.lanczos(ora.DiagOp(_diag(n, dtype, 0.0)), Xo, To) == 0
    return To


def _assert_columns(H, Ho, cols, what):
    for j in cols:
        err = np.abs(H[:, j] - Ho[:, j]).max()
        assert err <= RTOL * np.abs(Ho[:, j]).max(), f"{what}: column {j + 1} differs by {err:.3e}"


def _assert_orthonormal(Xg, what):
    err = np.abs(Xg.conj().T @ Xg - np.eye(Xg.shape[1])).max()
    assert err <= 1e-12, f"{what}: |X^H X - I| = {err:.3e}"


@pytest.fixture()
def fresh():
    """a context of its own per test: a give-up changes a context's state (the single launch pauses), the shared one must not see it"""
    ctxs = []

    def make(onchip=1):
        c = lk.Context(device=0)
        c.set_tuning("resident_onchip", onchip)
        ctxs.append(c)
        return c
    yield make
    for c in ctxs:
        c.close()


@pytest.mark.parametrize("onchip", [1, 0], ids=["dgs_onchip", "dgs_resident"])
@pytest.mark.parametrize("dtype", KINDS)
def test_give_up_on_a_look_ahead_step_of_a_cancelled_batch_leaves_the_context_usable(fresh, dtype, onchip):
    """One-step segments: spin 0 is set when step 1 is delivered, while steps 1..25 are already enqueued, so step 26 gives up; the progress
    function stops the factorisation when step 2 is delivered.  Nobody reads step 26's slot -- the abort word it raised must still be
    cleared, and every later single launch on the context (asynchronous Arnoldi, the host-synchronous step, Lanczos) must be correct.  The
    follow-up calls use other operators and start vectors: a launch that did nothing would leave the previous call's numbers in the slots."""
    ctx = fresh(onchip)
    n, m = 100_003, 32
    Ho = _oracle_arnoldi(n, m, dtype, 0.3, 7)
    X = lk.krylov_basis_gpu(n, m + 1, dtype, ctx)
    X.upload(_start(n, dtype, 7).reshape(-1, 1), 0)
    H = np.zeros((m + 1, m), dtype=dtype, order="F")
    seen = []

    def progress(kfirst, klast):
        seen.append((kfirst, klast))
        if klast == 1:
            ctx.set_tuning("resident_spin_ms", 0)
        return klast == 2
    lk.arnoldi(lk.diag_linop_gpu(_diag(n, dtype, 0.3), ctx), X, H, _segments=list(range(1, m)), _progress=progress)
    assert seen == [(1, 1), (2, 2)]
    _assert_columns(H, Ho, range(2), "cancelled batch, delivered columns")
    st0 = ctx.resident_stats()
    assert st0[0] == 2 + LOOKAHEAD, st0                   # steps 1..26 were enqueued as single launches, nothing after the request to stop

    ctx.set_tuning("resident_spin_ms", 2000)
    ctx.set_tuning("resident", 1)
    st1 = ctx.resident_stats()
    # asynchronous Arnoldi: another operator, another start vector, the same batch shape
    Ho2 = _oracle_arnoldi(n, m, dtype, -0.7, 11)
    d2 = _diag(n, dtype, -0.7)
    X2 = lk.krylov_basis_gpu(n, m + 1, dtype, ctx)
    X2.upload(_start(n, dtype, 11).reshape(-1, 1), 0)
    H2 = np.zeros((m + 1, m), dtype=dtype, order="F")
    assert lk.arnoldi(lk.diag_linop_gpu(d2, ctx), X2, H2) == 0
    _assert_columns(H2, Ho2, range(m), "Arnoldi after the cancelled batch")
    Xg = X2.download()
    _assert_orthonormal(Xg, "Arnoldi after the cancelled batch")
    assert np.abs(d2[:, None] * Xg[:, :m] - Xg @ H2).max() <= 1e-12
    # the host-synchronous entry
    k = 9
    Q = orthonormal_basis(n, k, dtype, 40)
    y = seeded(n, dtype, 41)
    yo = y.copy()
    ho, _ = ora.double_gram_schmidt_step(yo, Q.copy(order="F"))
    B = lk.krylov_basis_gpu(n, k + 1, dtype, ctx)
    B.upload(Q, 0)
    B.upload(y.reshape(-1, 1), k)
    beta = np.zeros(k, dtype=dtype)
    lk.double_gram_schmidt_step(B[k], B[:k], False, beta=beta)
    ynorm = np.linalg.norm(y)
    assert np.abs(beta - ho).max() <= RTOL * ynorm
    assert np.abs(B.download(k, 1)[:, 0] - yo).max() <= RTOL * ynorm
    # Lanczos
    ml = 20
    To = _oracle_lanczos(n, ml, dtype, 13)
    X3 = lk.krylov_basis_gpu(n, ml + 1, dtype, ctx)
    X3.upload(_start(n, dtype, 13).reshape(-1, 1), 0)
    T = np.zeros((ml + 1, ml), dtype=dtype, order="F")
    assert lk.lanczos(lk.diag_linop_gpu(_diag(n, dtype, 0.0), ctx), X3, T) == 0
    _assert_columns(T, To, range(ml), "Lanczos after the cancelled batch")
    _assert_orthonormal(X3.download(), "Lanczos after the cancelled batch")

    st2 = ctx.resident_stats()
    assert st1[1] == 1, st1                               # the give-up of step 26 was seen when the cancelled batch ended
    assert st2[1] == 1, st2                               # ... and no launch after it found the abort word still raised
    assert st2[0] - st1[0] == m + 1 + ml, (st1, st2)      # every follow-up step ran as a single launch
    assert (st2[2] - st1[2] > 0) == bool(onchip), (st1, st2)


@pytest.mark.parametrize("dtype", KINDS)
def test_give_up_in_the_middle_of_a_segmented_batch(fresh, dtype):
    """Step 26 of an uncancelled batch of one-step segments gives up after steps 1..25 were delivered: the batch stops there, the step runs
    again on the three sweeps and the rest of the factorisation follows.  H and the basis are the oracle's; every step is reported once,
    in order, and a reported column is final (test_gpu_pipelines' delivery contract)."""
    ctx = fresh()
    n, m = 80_021, 40
    Ho = _oracle_arnoldi(n, m, dtype, 0.5, 17)
    d = _diag(n, dtype, 0.5)
    X = lk.krylov_basis_gpu(n, m + 1, dtype, ctx)
    X.upload(_start(n, dtype, 17).reshape(-1, 1), 0)
    H = np.zeros((m + 1, m), dtype=dtype, order="F")
    seen, snapshots = [], []

    def progress(kfirst, klast):
        seen.append((kfirst, klast))
        snapshots.append(H[:klast + 1, kfirst - 1:klast].copy())
        if klast == 1:
            ctx.set_tuning("resident_spin_ms", 0)
        return False
    assert lk.arnoldi(lk.diag_linop_gpu(d, ctx), X, H, _segments=list(range(1, m)), _progress=progress) == 0
    assert seen == [(j, j) for j in range(1, m + 1)], seen
    _assert_columns(H, Ho, range(m), "segmented batch with a give-up at step 26")
    for (a, b), snap in zip(seen, snapshots):
        assert np.array_equal(snap, H[:b + 1, a - 1:b]), (a, b)
    Xg = X.download()
    _assert_orthonormal(Xg, "segmented batch with a give-up at step 26")
    assert np.abs(d[:, None] * Xg[:, :m] - Xg @ H).max() <= 1e-12
    st = ctx.resident_stats()
    assert st[:2] == (m, 1), st                           # all m steps were enqueued as single launches in the first batch; one gave up


@pytest.mark.parametrize("p", [2, 4])
@pytest.mark.parametrize("dtype", KINDS)
def test_block_arnoldi_and_qr_finish_a_column_whose_single_launch_gave_up(fresh, dtype, p):
    """Block Arnoldi (arnoldi.fypp:20-73) and qr_no_pivoting (qr.fypp:116-167) on a device panel with spin 0: the single launch of column 1
    of a block gives up, the batch stops there and the host finishes the block from that column on the three sweeps."""
    ctx = fresh()
    ctx.set_tuning("resident_spin_ms", 0)
    n, kdim = 60_013, 6
    d = _diag(n, dtype, 0.2)
    Q0 = orthonormal_basis(n, p, dtype, 70)
    ncol = (kdim + 1) * p
    Xo = np.zeros((n, ncol), dtype=dtype, order="F")
    Xo[:, :p] = Q0
    Ho = np.zeros((ncol, kdim * p), dtype=dtype, order="F")
    assert ora.arnoldi_block(ora.DiagOp(d), Xo, Ho, p) == 0
    X = lk.krylov_basis_gpu(n, ncol, dtype, ctx)
    X.upload(Q0, 0)
    H = np.zeros((ncol, kdim * p), dtype=dtype, order="F")
    assert lk.arnoldi(lk.diag_linop_gpu(d, ctx), X, H, blksize=p) == 0
    st = ctx.resident_stats()
    assert st[0] >= 1 and st[1] >= 1, st
    _assert_columns(H, Ho, range(kdim * p), f"block Arnoldi p = {p}")
    Xg = X.download()
    _assert_orthonormal(Xg, f"block Arnoldi p = {p}")
    assert np.abs(d[:, None] * Xg[:, :kdim * p] - Xg @ H).max() <= 1e-12

    ctx.set_tuning("resident", 1)                         # (re-arm: the next single launch gives up again)
    M = basis(n, p, dtype, 300)
    Mo = M.copy(order="F")
    Ro = np.zeros((p, p), dtype=dtype, order="F")
    assert ora.qr_no_pivoting(Mo, Ro) == 0
    B = lk.krylov_basis_gpu(n, p, dtype, ctx)
    B.upload(M, 0)
    R = np.zeros((p, p), dtype=dtype, order="F")
    before = ctx.resident_stats()
    assert lk.qr(B, R) == 0
    after = ctx.resident_stats()
    assert after[0] > before[0] and after[1] - before[1] == 1, (before, after)
    _assert_columns(R, Ro, range(p), f"qr p = {p}")
    Qg = B.download()
    _assert_orthonormal(Qg, f"qr p = {p}")
    assert np.abs(Qg - Mo).max() <= 1e-12


@pytest.mark.parametrize("dtype", KINDS)
def test_qr_of_a_device_panel_sets_the_whole_of_R(ctx, dtype):
    """qr.fypp:125 sets ALL of R to zero before the loop: an R larger than p x p comes back with zeros outside the factor, whatever it held"""
    n, p = 60_013, 4
    M = basis(n, p, dtype, 500)
    Mo = M.copy(order="F")
    Ro = np.full((p + 2, p + 2), 7.0, dtype=dtype, order="F")
    assert ora.qr_no_pivoting(Mo, Ro) == 0
    B = lk.krylov_basis_gpu(n, p, dtype, ctx)
    B.upload(M, 0)
    R = np.full((p + 2, p + 2), 7.0, dtype=dtype, order="F")
    assert lk.qr(B, R) == 0
    assert not R[p:, :].any() and not R[:, p:].any(), R
    _assert_columns(R, Ro, range(p + 2), "qr into a larger R")
    assert np.abs(B.download() - Mo).max() <= 1e-12


def test_qr_refuses_an_R_with_fewer_columns_than_the_panel(ctx):
    """an R that cannot hold p columns is an error, raised before anything is computed (the engine would write p columns into it)"""
    n, p = 60_013, 4
    M = basis(n, p, np.float64, 600)
    B = lk.krylov_basis_gpu(n, p, np.float64, ctx)
    B.upload(M, 0)
    for shape in ((p + 2, p - 1), (p - 1, p), (p,)):
        R = np.zeros(shape, order="F")
        with pytest.raises(ValueError, match="R has shape"):
            lk.qr(B, R)
        assert not R.any()
    assert np.array_equal(B.download(), M)
