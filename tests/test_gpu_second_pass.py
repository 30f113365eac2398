"""The second Gram-Schmidt pass with corrections that are not zero.

double_gram_schmidt_step (gram_schmidt.fypp:12-105) is two classical passes, beta = h1 + h2, y'' = y - X h1 - X h2.  On an orthonormal
basis h2 = X^H y' is rounding noise, 1e-16 |y|, and everything the second pass contributes lies four orders below the 1e-12 the suite
compares at.  Here the basis is `skewed_basis` (off orthonormal by 1e-3, cond about 1.03: nothing is amplified), so h2 is about 1e-3 |y|
and a kernel that drops the pass, adds h2 with the wrong sign or mis-indexes it at a ragged column tail is 10^7 or more above the bound
(tests/test_oracle_second_pass.py shows that without a GPU).  Three inputs per shape:

  skew_rand   skewed X, random y
  skew_span   skewed X, y = X c + 1e-6 r: a small beta_{k+1}, h2 from the basis and from the cancellation
  orth_span   orthonormal Q, y = Q c + 1e-6 r: h2 from the cancellation of the first pass only, about 1e-16 |y| -- the guard
              `assert_second_pass_matters` does NOT apply to this one; it is here for the small |y''| (compared normwise, scale |y|)

Bound: max |got - ref| <= RTOL |y| (tests/_tol.py, 1e-12) for beta and for y'', against the longdouble evaluation AND against the oracle;
X bit-identical after the call.  The bound is the same where a panel has more columns than rows (n = 29 below): no orthonormal or
near-orthonormal X exists there, the columns are unit random vectors, ||X||_2^2 is about k / n and y'' grows to as much as 400 |y| at
k = 600 -- the scale stays |y|."""
import functools

import numpy as np
import pytest

import lightkrylov_amd as lk
from oracle import oracle as ora
from tests._gpu_helpers import (KINDS, arnoldi_operator, assert_second_pass_matters, dgs_longdouble, second_pass_input, skewed_basis)
from tests._tol import RTOL, assert_close, assert_columns_close
from tests.test_gpu_caller_memory import SCHEDULES
from tests.test_gpu_sharded_emulation import _sharded

pytestmark = pytest.mark.gpu

INPUTS = ("skew_rand", "skew_span", "orth_span")
# every key this module sets, with the engine's default (restored after each use)
DEFAULTS = dict(resident=1, resident_onchip=1, resident_rev=1, recompute_update=1, wide_regs=2, wide_s3=1, dot_colwise=1, store_split=0,
                store_policy=2, grid_mult=2, xhy_mfma=1, block_fused=1, upd_rs=1, gemm_3m=1, async_arnoldi=1, lazy=0, lazy_speculate=1)

_CTXS = {}


def tuned(**kw):
    """one context per tuning set for the whole module (closed at its end)"""
    key = tuple(sorted(kw.items()))
    if key not in _CTXS:
        c = lk.Context(device=0)
        for k, v in key:
            c.set_tuning(k, v)
        _CTXS[key] = c
    return _CTXS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in _CTXS.values():
        c.close()
    _CTXS.clear()
    case.cache_clear()


def name(dtype):
    return np.dtype(dtype).name


@functools.lru_cache(maxsize=None)
def case(n, k, dtype, which, p=0):
    """(X, Y, beta and y'' in longdouble, beta and y'' of the oracle, |y| per column); Y is one vector (p = 0) or a block of p columns.
    The guard runs here, on the reference values, for the two inputs it applies to."""
    X, Y = second_pass_input(n, k, dtype, which, max(p, 1))
    h1, h2, _y1, y2 = dgs_longdouble(Y, X)
    if which != "orth_span":
        for j in range(Y.shape[1]):
            assert_second_pass_matters(h1[:, j], h2[:, j], Y[:, j])
    Yo = Y.copy(order="F")
    if p:
        ho, _ = ora.double_gram_schmidt_step_block(Yo, X.copy(order="F"))
        ho = ho.reshape(k, p, order="F")
    else:
        ho, _ = ora.double_gram_schmidt_step(Yo[:, 0], X.copy(order="F"))
        ho = ho.reshape(k, 1)
    scale = np.linalg.norm(Y, axis=0)
    for a in (Y, Yo, ho):
        a.setflags(write=False)
    return X, Y, h1 + h2, y2, ho, Yo, scale


def check(group, label, got_h, got_y, ref):
    """beta and y'' of every column against both references, normwise with the scale |y|"""
    _X, _Y, hl, yl, ho, yo, scale = ref
    got_h, got_y = np.asarray(got_h).reshape(hl.shape), np.asarray(got_y).reshape(yl.shape)
    for j in range(hl.shape[1]):
        tag = f"second pass {group}: {label}" + (f" column {j}" if hl.shape[1] > 1 else "")
        assert_close(got_h[:, j], hl[:, j], tag + " beta / longdouble", scale=scale[j])
        assert_close(got_y[:, j], yl[:, j], tag + " y'' / longdouble", scale=scale[j])
        assert_close(got_h[:, j], ho[:, j], tag + " beta / oracle", scale=scale[j])
        assert_close(got_y[:, j], yo[:, j], tag + " y'' / oracle", scale=scale[j])


def step(c, ref, panel=None, again=False):
    """lk_dgs of the case's y against its X on context c; returns beta, y'' and asserts that X is bit-identical afterwards (`again`: X is
    in the panel already and the caller looks at it after its last step)"""
    X, Y = ref[0], ref[1]
    n, k = X.shape
    B = panel if panel is not None else lk.krylov_basis_gpu(n, k + 1, X.dtype, c)
    if not again:
        B.upload(X, 0)
    B.upload(Y[:, :1], k)
    h = np.zeros(k, dtype=X.dtype)
    assert lk.double_gram_schmidt_step(B[k], B[:k], False, beta=h) == 0
    if again:
        return h, B.download(k, 1)[:, 0]
    got = B.download()
    assert np.array_equal(got[:, :k], X), "X is read only"
    return h, got[:, k]


# ---- a. lk_dgs on every schedule --------------------------------------------------------------------------------------------------
# k on each side of every change the engine makes in k (lk_dgs, sweepm, sweep_cfg in lk_engine.hip): wave-columns of 16 / 8 register
# columns (16 | 17, 32 | 33, 64 | 65), the complex kind's block shape (32 | 33; the dot-only sweep 56 | 57), the single launch and the
# plain sweeps up to 128 | 129 the wide shapes (complex register tiles to 192 | 193, real to 256 | 257, "wide_regs" 2 to 384 | 385, the
# four-way lane split to 512 | 513 the column panels of 512)
K_ALL = (1, 2, 15, 16, 17, 31, 32, 33, 56, 57, 64, 65, 100, 127, 128, 129, 192, 193, 200, 256, 257, 300, 384, 385, 512, 513, 600)
K_SINGLE = tuple(k for k in K_ALL if k <= 129)                     # the single launch takes k <= 128; 129 must go to the three sweeps


@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("dtype", KINDS)
def test_dgs_second_pass_on_every_schedule(dtype, schedule):
    """lk_dgs on the three sweeps, the single launch with the panel in registers and the single launch from the cache, at n = 29 (< 32, and
    below k for most k), at a ragged odd n and once at n = 300 007; the resident counters show which route ran."""
    c = tuned(**SCHEDULES[schedule])
    single = schedule != "three_sweeps"
    before = c.resident_stats()
    launched = 0
    shapes = [(n, k) for n in (29, 701) for k in (K_SINGLE if single else K_ALL)] + [(300_007, 16)]
    for n, k in shapes:
        for which in INPUTS:
            if which == "orth_span" and k > n:
                continue                                             # (no orthonormal panel of more columns than rows)
            ref = case(n, k, dtype, which)
            h, y = step(c, ref)
            launched += 1 if single and k <= 128 else 0
            check("a " + schedule, f"{name(dtype)} n = {n} k = {k} {which}", h, y, ref)
        if n == 701 and k == K_SINGLE[-1]:
            small = c.resident_stats()
    after = c.resident_stats()
    assert after[1] == before[1], (before, after)                    # no launch gave up
    assert after[0] - before[0] == launched, (before, after, launched)
    if single:
        assert (small[2] - before[2] > 0) == (schedule == "single_onchip"), (before, small)   # panels in registers at the small sizes


# ---- b. every key that changes how sweeps 2 and 3 run -------------------------------------------------------------------------------
def _with(c, keys, fn):
    try:
        for k, v in keys.items():
            c.set_tuning(k, v)
        return fn()
    finally:
        for k in keys:
            c.set_tuning(k, DEFAULTS[k])


# "grid_mult" (domain 1 .. 16, default 2): both ends, the default's neighbours and two values between -- the key only sets how many per-block
# partial sums a dot is assembled from
BITS_KEYS = [dict(store_policy=0), dict(store_policy=1), dict(store_policy=3), dict(store_split=1), dict(store_policy=1, store_split=1)]
BOUND_KEYS = ([dict(recompute_update=0), dict(wide_regs=0), dict(wide_regs=1), dict(wide_regs=0, wide_s3=0), dict(wide_regs=2, wide_s3=0),
               dict(dot_colwise=0), dict(recompute_update=0, dot_colwise=0), dict(recompute_update=0, wide_regs=0)]
              + [dict(grid_mult=g) for g in (1, 3, 4, 8, 16)])


@pytest.mark.parametrize("dtype", KINDS)
def test_sweep_keys_with_a_real_second_pass(dtype):
    """The three sweeps ("resident" 0) under every key that changes sweeps 2 and 3, at k = 33, 150, 200, 300 and 400 (the plain shape, the
    register tiles, the two- and four-way lane split).  "store_policy", "store_split" and "wide_s3" -- the keys of this group that
    include/lightkrylov_hip.h marks [bits] -- against the default bit for bit on the skewed input; every setting within the bound."""
    c = tuned(resident=0)
    n = 2053
    for k in (33, 150, 200, 300, 400):
        B = lk.krylov_basis_gpu(n, k + 1, dtype, c)
        for which in INPUTS:
            ref = case(n, k, dtype, which)
            h0, y0 = step(c, ref, B)
            check("b default", f"{name(dtype)} k = {k} {which}", h0, y0, ref)
            for keys in BITS_KEYS:
                h, y = _with(c, keys, lambda: step(c, ref, B, again=True))
                assert h.tobytes() == h0.tobytes() and y.tobytes() == y0.tobytes(), (keys, k, which)
            for keys in BOUND_KEYS:
                h, y = _with(c, keys, lambda: step(c, ref, B, again=True))
                check(f"b {keys}", f"{name(dtype)} k = {k} {which}", h, y, ref)
            for regs in (0, 2):                                      # "wide_s3" [bits]: the same y' re-formed in the same order
                a = _with(c, dict(wide_regs=regs, wide_s3=0), lambda: step(c, ref, B, again=True))
                b = _with(c, dict(wide_regs=regs, wide_s3=1), lambda: step(c, ref, B, again=True))
                assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), (regs, k, which)
            assert np.array_equal(B.download(0, k), ref[0]), "X is read only"
        del B


@pytest.mark.parametrize("schedule", ["single_onchip", "single_cache"])
@pytest.mark.parametrize("dtype", KINDS)
def test_single_launch_keys_with_a_real_second_pass(dtype, schedule):
    """"resident_rev" 0 / 1 (phase 2 walks the tiles backwards or forwards) and "grid_mult" on the single launch, n large enough for
    several tiles per block"""
    c = tuned(**SCHEDULES[schedule])
    n = 8009
    for k in (17, 100):
        for which in INPUTS:
            ref = case(n, k, dtype, which)
            for keys in (dict(resident_rev=0), dict(resident_rev=1), dict(grid_mult=1), dict(grid_mult=16)):
                before = c.resident_stats()
                h, y = _with(c, keys, lambda: step(c, ref))
                after = c.resident_stats()
                assert after[0] == before[0] + 1 and after[1] == before[1], (before, after)
                check(f"b {schedule} {keys}", f"{name(dtype)} k = {k} {which}", h, y, ref)


# ---- c. lk_dgs_block ---------------------------------------------------------------------------------------------------------------
BLOCK_CFGS = [dict(xhy_mfma=0), dict(block_fused=0), dict(block_fused=1), dict(block_fused=2), dict(upd_rs=0), dict(upd_rs=1),
              dict(gemm_3m=0), dict(gemm_3m=1)]


@pytest.mark.parametrize("cfg", BLOCK_CFGS, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
@pytest.mark.parametrize("dtype", KINDS)
def test_block_step_with_a_real_second_pass(ctx, dtype, cfg):
    """lk_dgs_block, four columns per pass on the vector units and on the matrix cores under each of their keys, per column against
    dgs_longdouble and ora.double_gram_schmidt_step_block.  The engine's own launch counts (lk_profile_get) say which route ran
    (dgs_block_fused_ok / dgs_block_on_mfma in lk_engine.hip): one vector (p = 1), and k > 128 with "xhy_mfma" 0, go column by column
    through lk_dgs; "xhy_mfma" 1 with p >= 5 or k > 128 runs on the matrix cores (panel_xhy_mfma and the fused update kernels; "upd_rs"
    acts for the real kind at p = 17 and 32, "gemm_3m" for the complex kind); the rest -- p = 4, or "xhy_mfma" 0 up to 128 columns --
    takes four columns per pass on the vector units (panel_dot_p and the block sweeps)."""
    n = 301
    mfma_on = cfg.get("xhy_mfma", 1) == 1

    def route(k, p):
        if p == 1 or (k > 128 and not mfma_on):
            return "columns"
        return "mfma" if mfma_on and (p >= 5 or k > 128) else "valu"

    def launches():
        return {t: ctx.profile_get(t)[0] for t in ("dgs", "dots_p", "dgs_block_sweep2", "xhy_mfma", "xhy_upd_mfma")}

    def run():
        for k in (8, 33, 128, 200):
            Bx = lk.krylov_basis_gpu(n, k, dtype, ctx)
            for p in (1, 4, 5, 16, 17, 32):
                By = lk.krylov_basis_gpu(n, p, dtype, ctx)
                for which in INPUTS:
                    ref = case(n, k, dtype, which, p)
                    Bx.upload(ref[0])
                    By.upload(ref[1])
                    h = np.zeros((k, p), dtype=dtype, order="F")
                    ctx.profile_reset()
                    ctx.profile_enable(True)
                    try:
                        assert lk.double_gram_schmidt_step(By, Bx, False, beta=h) == 0
                        ctx.sync()
                        ran = launches()
                    finally:
                        ctx.profile_enable(False)
                    on_cols, on_valu, on_mfma = ran["dgs"], ran["dots_p"] + ran["dgs_block_sweep2"], ran["xhy_mfma"] + ran["xhy_upd_mfma"]
                    want = route(k, p)
                    assert (on_cols == p if want == "columns" else on_cols == 0) and (on_valu > 0) == (want == "valu") \
                        and (on_mfma > 0) == (want == "mfma"), (cfg, k, p, want, ran)
                    assert np.array_equal(Bx.download(), ref[0]), "X is read only"
                    check(f"c {cfg}", f"{name(dtype)} k = {k} p = {p} {which}", h, By.download(), ref)
                del By
            del Bx
    _with(ctx, cfg, run)


# ---- d. factorisations that continue from a skewed leading block ----------------------------------------------------------------------
def _start_block(n, ncols, k0, dtype):
    X0 = np.zeros((n, ncols), dtype=dtype, order="F")
    X0[:, :k0] = skewed_basis(n, k0, dtype, 40 + k0)
    return X0


@pytest.mark.parametrize("schedule", ["three_sweeps", "single_onchip"])
@pytest.mark.parametrize("dtype", KINDS)
def test_arnoldi_continued_from_a_skewed_block(dtype, schedule):
    """lk_arnoldi(kstart = k0) on k0 uploaded skewed columns (the convention of ora.arnoldi and of arnoldi.fypp:36: step k applies A to
    column k and orthogonalises against columns 1 .. k), one round trip per step, all steps enqueued, and delivered in segments: columns
    k0 .. m of H against the oracle run from the same start, which tests/test_oracle_second_pass.py ties to the longdouble restatement."""
    c = tuned(**SCHEDULES[schedule])
    n, k0, m = 5003, 12, 24
    d = arnoldi_operator(n, dtype)
    X0 = _start_block(n, m + 1, k0, dtype)
    Xo, Ho = X0.copy(order="F"), np.zeros((m + 1, m), dtype=dtype, order="F")
    assert ora.arnoldi(ora.DiagOp(d), Xo, Ho, kstart=k0) == 0
    A = lk.diag_linop_gpu(d, c)
    for mode in ("sync", "async", "segments"):
        before = c.resident_stats()
        X = lk.krylov_basis_gpu(n, m + 1, dtype, c)
        X.upload(X0)
        H = np.zeros((m + 1, m), dtype=dtype, order="F")
        seen = []
        kw = dict(_segments=[15, 16, 21], _progress=lambda a, b: seen.append((a, b)) or False) if mode == "segments" else {}
        info = _with(c, dict(async_arnoldi=0 if mode == "sync" else 1), lambda: lk.arnoldi(A, X, H, kstart=k0, **kw))
        assert info == 0
        after = c.resident_stats()
        assert (after[0] - before[0] > 0) == (schedule != "three_sweeps") and after[1] == before[1], (before, after)
        if mode == "segments":
            assert seen and seen[0][0] == k0 and seen[-1][1] == m, seen
        label = f"second pass d arnoldi kstart = {k0} {schedule} {mode} {name(dtype)}"
        assert_columns_close(H[:, k0 - 1:], Ho[:, k0 - 1:], label)
        got = X.download()
        assert np.array_equal(got[:, :k0], X0[:, :k0])                # the leading block is the caller's
        assert_close(got[:, k0:], Xo[:, k0:], label + " basis")    # (unit columns, entrywise against max |x|: the same bare 1e-12)
        del X


@pytest.mark.parametrize("schedule", ["three_sweeps", "single_onchip"])
@pytest.mark.parametrize("dtype", KINDS)
def test_lanczos_bidiagonalization_and_block_arnoldi_continued_from_skewed_blocks(dtype, schedule):
    """lk_lanczos, lk_bidiag and lk_arnoldi_block (p = 2) with kstart = k0 on uploaded skewed leading blocks against ora.lanczos /
    bidiagonalization / arnoldi_block from the same start, each with "async_arnoldi" 1 and 0.  (Only lk_arnoldi and lk_arnoldi_block read
    that key; lk_lanczos and lk_bidiag always enqueue their steps, so for them the two runs must agree bit for bit.)"""
    c = tuned(**SCHEDULES[schedule])
    n, k0, m = 5003, 12, 24
    g = np.arange(n) / n
    dh = (1.0 + g).astype(dtype)                                      # Hermitian
    X0 = _start_block(n, m + 1, k0, dtype)
    Xo, To = X0.copy(order="F"), np.zeros((m + 1, m), dtype=dtype, order="F")
    assert ora.lanczos(ora.DiagOp(dh), Xo, To, kstart=k0) == 0
    Ts = []
    for a in (1, 0):
        X = lk.krylov_basis_gpu(n, m + 1, dtype, c)
        X.upload(X0)
        T = np.zeros((m + 1, m), dtype=dtype, order="F")
        assert _with(c, dict(async_arnoldi=a), lambda: lk.lanczos(lk.diag_linop_gpu(dh, c), X, T, kstart=k0)) == 0
        assert_columns_close(T[:, k0 - 1:], To[:, k0 - 1:], f"second pass d lanczos kstart = {k0} {schedule} async {a} {name(dtype)}")
        Ts.append(T)
        del X
    assert np.array_equal(Ts[0], Ts[1])

    d = arnoldi_operator(n, dtype)
    U0 = _start_block(n, m + 1, k0, dtype)
    V0 = np.zeros((n, m), dtype=dtype, order="F")
    V0[:, :k0 - 1] = skewed_basis(n, k0 - 1, dtype, 900)              # step k0 orthogonalises A^H u_k0 against v_1 .. v_(k0 - 1)
    Uo, Vo, Bo = U0.copy(order="F"), V0.copy(order="F"), np.zeros((m + 1, m), dtype=dtype, order="F")
    assert ora.bidiagonalization(ora.DiagOp(d), ora.DiagOp(d.conj()), Uo, Vo, Bo, kstart=k0) == 0
    Bs = []
    for a in (1, 0):
        U, V = lk.krylov_basis_gpu(n, m + 1, dtype, c), lk.krylov_basis_gpu(n, m, dtype, c)
        U.upload(U0)
        V.upload(V0)
        Bm = np.zeros((m + 1, m), dtype=dtype, order="F")
        assert _with(c, dict(async_arnoldi=a), lambda: lk.bidiagonalization(lk.diag_linop_gpu(d, c), U, V, Bm, kstart=k0)) == 0
        assert_columns_close(Bm[:, k0 - 1:], Bo[:, k0 - 1:], f"second pass d bidiag kstart = {k0} {schedule} async {a} {name(dtype)}")
        Bs.append(Bm)
        del U, V
    assert np.array_equal(Bs[0], Bs[1])

    p, kb0, kdim = 2, 4, 9
    ncol = (kdim + 1) * p
    X0 = _start_block(n, ncol, kb0 * p, dtype)
    Xo, Ho = X0.copy(order="F"), np.zeros((ncol, kdim * p), dtype=dtype, order="F")
    assert ora.arnoldi_block(ora.DiagOp(d), Xo, Ho, p, kstart=kb0) == 0
    c0 = (kb0 - 1) * p
    for a in (1, 0):
        X = lk.krylov_basis_gpu(n, ncol, dtype, c)
        X.upload(X0)
        H = np.zeros((ncol, kdim * p), dtype=dtype, order="F")
        assert _with(c, dict(async_arnoldi=a), lambda: lk.arnoldi(lk.diag_linop_gpu(d, c), X, H, kstart=kb0, blksize=p)) == 0
        assert_columns_close(H[:, c0:], Ho[:, c0:], f"second pass d arnoldi_block p = {p} kstart = {kb0} {schedule} async {a} {name(dtype)}")
        del X


# ---- e. lazy per-object path --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("speculate", [0, 1])
@pytest.mark.parametrize("dtype", KINDS)
def test_lazy_per_object_step_with_a_real_second_pass(dtype, speculate):
    """The reference's per-object loop (a dot per column, an axpby per column, sub, norm: gram_schmidt.fypp:113-150 twice) on a skewed panel
    with "lazy" 1: the second pass's k dots come out of the fused update + dot sweep (lk_lazy_fusion_stats), whose h2 is not noise here.
    Two vectors one after the other in neighbouring columns, so that the anticipated sweep of "lazy_speculate" has its chance."""
    c = tuned(lazy=1, lazy_speculate=speculate)
    for n, k in ((1037, 33), (5003, 128), (2053, 200)):
        for which in INPUTS:
            ref = case(n, k, dtype, which, 2)
            X, Y = ref[0], ref[1]
            B = lk.krylov_basis_gpu(n, k + 2, dtype, c)
            B.upload(X, 0)
            B.upload(Y, k)
            cols = [B[j] for j in range(k)]                            # a python list of vectors: the per-object path
            h = np.zeros((k, 2), dtype=dtype, order="F")
            before = c.lazy_fusion_stats()
            for j in range(2):
                hj = np.zeros(k, dtype=dtype)
                assert B[k + j].norm() > 0                              # (arnoldi's / qr's norm before the step: what arms the speculation)
                assert lk.double_gram_schmidt_step(B[k + j], cols, False, beta=hj) == 0
                h[:, j] = hj
            got = B.download()
            after = c.lazy_fusion_stats()
            assert after[0] - before[0] == 2 and after[3] == before[3], (before, after)   # one fused sweep per step, no temporary written
            assert np.array_equal(got[:, :k], X)
            check(f"e lazy_speculate = {speculate}", f"{name(dtype)} n = {n} k = {k} {which}", h, got[:, k:], ref)
            del cols, B


# ---- f. row-sharded emulation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks", [2, 3])
@pytest.mark.parametrize("dtype", KINDS)
def test_sharded_step_with_a_real_second_pass(ctx, dtype, nranks):
    """lk_dgs on row blocks of a skewed panel, two and three emulated ranks: the second all-reduce carries a real h2.  Every rank holds the
    same beta, and beta and the stitched y'' agree with the references and with the single-context step within the bound."""
    n = 4001
    cases = [(k, which, case(n, k, dtype, which)) for k in (33, 150) for which in INPUTS]

    def body(rank, c, row0, nl):
        out = []
        for k, _which, ref in cases:
            X, Y = ref[0], ref[1]
            B = lk.krylov_basis_gpu(nl, k + 1, dtype, c)
            B.upload(np.asfortranarray(X[row0:row0 + nl]), 0)
            B.upload(np.asfortranarray(Y[row0:row0 + nl]), k)
            h = np.zeros(k, dtype=dtype)
            info = lk.double_gram_schmidt_step(B[k], B[:k], False, beta=h)
            got = B.download()
            assert np.array_equal(got[:, :k], X[row0:row0 + nl])
            out.append((info, h, got[:, k]))
            del B
        return out

    res, grp = _sharded(n, nranks, body)
    assert grp.calls >= 3 * len(cases)                              # h1, h2 and the last norm of every step
    for i, (k, which, ref) in enumerate(cases):
        mine = [r[i] for r in res]
        assert all(r[0] == 0 for r in mine)
        assert all(np.array_equal(r[1], mine[0][1]) for r in mine)
        ys = np.concatenate([r[2] for r in mine])
        label = f"{name(dtype)} {nranks} ranks k = {k} {which}"
        check("f sharded", label, mine[0][1], ys, ref)
        h1, y1 = step(ctx, ref)
        assert_close(mine[0][1], h1, f"second pass f sharded: {label} beta / single context", scale=ref[6][0])
        assert_close(ys, y1, f"second pass f sharded: {label} y'' / single context", scale=ref[6][0])
