"""Every entry point on bases wider than 512 columns.

One sweep holds at most 512 basis columns (KMAX_WIDE in lk_engine.hip); the reference has no cap on the Krylov dimension (lanczos.fypp:20,
golub_kahan.fypp:18), so beyond it the engine changes schedule, and each of these schedules is the only route for its width:

  lk_dgs / lk_orthogonalize   513 .. 2048 columns: 2 to 4 column panels of 512 on the device, the coefficient sections of every panel side
                              by side, one copy to the host; wider: panels of 128, a host round trip each, h accumulated on the host
  lk_innerprod / lk_gram      512-column chunks for one vector, 128-column chunks for 2 .. 4, 128 x 128 matrix-core blocks from 5 on
  lk_lincomb                  128-column chunks that accumulate into the output after the first
  lk_dgs_block                column by column through lk_dgs
  lk_qr and the factorisations  lk_dgs on a view of the leading columns

The Gram-Schmidt inputs are skewed panels (tests/_gpu_helpers.py: off orthonormal by 1e-3, so the second pass has corrections of 1e-3 |y|
to make; tests/test_oracle_very_wide.py pins that on the reference alone), the bound is the bare 1e-12 |y| against the longdouble evaluation,
entry by entry; the products are compared entrywise with their a-priori bound (check_entrywise).  The worst ratio of every part goes to the
tolerance report."""
import ctypes as C
import functools

import numpy as np
import pytest

import lightkrylov_amd as lk
from lightkrylov_amd import _capi
from oracle import oracle as ora
from tests._gpu_helpers import (KINDS, VERY_WIDE_BLOCK_K, VERY_WIDE_FLAG_K, VERY_WIDE_K, VERY_WIDE_PANEL_K, CallerPanel, _long, _sharded,
                                arnoldi_block_step_longdouble, arnoldi_operator, arnoldi_step_longdouble, assert_second_pass_matters, basis,
                                bidiag_step_longdouble, check_entrywise, dgs_longdouble, ext, is_cplx, lanczos_step_longdouble, product_scale,
                                second_pass_input, skewed_basis, very_wide_n)
from tests._tol import RTOL, _report, assert_close, assert_columns_close

pytestmark = pytest.mark.gpu

_DP = C.POINTER(C.c_double)
LK_OK, LK_ERR_INVALID, LK_ERR_NAN = 0, -1, -5
INPUTS = ("skew_rand", "skew_span")
DEFAULTS = dict(resident=1, gemm_3m=1, xhy_mfma=1)                # every key this module sets, with the engine's default
KWIDE, KFUSED = 512, 128                                           # KMAX_WIDE, KMAX_FUSED of lk_engine.hip

_CTXS = {}
WORST = {}                                                         # part -> worst measured / bound


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
def _close_contexts_and_report():
    yield
    for c in _CTXS.values():
        c.close()
    _CTXS.clear()
    case.cache_clear()
    for part in sorted(WORST):
        print(f"very wide bases, part {part}: worst measured / bound = {WORST[part]:.3e}")
        _report(f"very wide bases, part {part}: worst of the part", WORST[part], 1.0, "measured / bound")


def _with(c, keys, fn):
    try:
        for k, v in keys.items():
            c.set_tuning(k, v)
        return fn()
    finally:
        for k in keys:
            c.set_tuning(k, DEFAULTS[k])


def name(dtype):
    return np.dtype(dtype).name


def panels(k):
    """(width, count) of the column panels lk_dgs walks at k columns"""
    w = KWIDE if k <= 4 * KWIDE else KFUSED
    return w, (k + w - 1) // w


def close(part, got, ref, label, scale=None):
    """max |got - ref| <= 1e-12 * scale, entry by entry (scale: |y|; max |ref| unless given); keeps the part's worst ratio to the bound"""
    err = assert_close(np.asarray(got), ref, f"very wide {part}: {label}", scale=scale)
    WORST[part] = max(WORST.get(part, 0.0), float(err) / RTOL)
    return err


def columns_close(part, got, ref, label):
    err = assert_columns_close(np.asarray(got), np.asarray(ref), f"very wide {part}: {label}")
    WORST[part] = max(WORST.get(part, 0.0), float(err) / RTOL)


def entrywise(part, got, ref, scale, m, cplx, label):
    WORST[part] = max(WORST.get(part, 0.0), check_entrywise(got, ref, scale, m, cplx, f"very wide {part}: {label}"))


@functools.lru_cache(maxsize=2)
def case(n, k, dtype, which, p=1):
    """X, Y (p columns) and the longdouble h1, h2, y', y'' of every column, the norms ||y||, ||y'||, ||y''|| and the scale |y|"""
    X, Y = second_pass_input(n, k, dtype, which, p)
    h1, h2, y1, y2 = dgs_longdouble(Y, X)
    for j in range(p):
        assert_second_pass_matters(h1[:, j], h2[:, j], Y[:, j])
    nrm = np.array([[np.sqrt((v[:, j].conj() @ v[:, j]).real) for v in (_long(Y), y1, y2)] for j in range(p)])
    Y.setflags(write=False)
    return X, Y, h1, h2, y1, y2, nrm, np.linalg.norm(Y, axis=0)


def dgs_raw(Bx, k, By, jy, h=True, norms=True, info=True, flags=0, two_pass=True):
    """lk_dgs / lk_orthogonalize through the ABI with any of the outputs NULL; returns (status, h, norms, info).  The outputs start as NaN /
    -7, so an entry the call does not write shows."""
    lib = _capi.load()
    hbuf = np.full(k, np.nan, dtype=Bx.dtype) if h else None
    nbuf = (C.c_double * 3)(np.nan, np.nan, np.nan)
    ibuf = C.c_int(-7)
    hp = hbuf.ctypes.data_as(_DP) if h else None
    ip = C.byref(ibuf) if info else None
    if two_pass:
        rc = lib.lk_dgs(Bx._h, k, By._h, jy, hp, nbuf if norms else None, flags, ip)
    else:
        rc = lib.lk_orthogonalize(Bx._h, k, By._h, jy, hp, ip)
    return rc, hbuf, np.array(list(nbuf)), ibuf.value


def check_step(part, label, ref, h, norms, y, j=0):
    _X, _Y, h1, h2, _y1, y2, nrm, scale = ref
    close(part, h, h1[:, j] + h2[:, j], label + " beta", scale[j])
    if norms is not None:
        close(part, norms, nrm[j], label + " norms", scale[j])
    close(part, y, y2[:, j], label + " y''", scale[j])


# ---- a. lk_dgs and lk_orthogonalize over the three schedules ------------------------------------------------------------------------
@pytest.mark.parametrize("k", VERY_WIDE_K)
@pytest.mark.parametrize("dtype", KINDS)
def test_dgs_and_orthogonalize_over_the_three_schedules(dtype, k):
    """512 (the last single sweep), both sides of 2 | 3 | 4 device panels and of the host-driven panels of 128, a full last panel (2176) and
    one of a single column (2177); "resident" 1 and 0 -- the key must not matter here, and no single launch may be enqueued: h, the three
    norms and y'' of the two-pass entry, h1 and y' of the one-pass entry, X bit-identical afterwards."""
    n = very_wide_n(k)
    for resident in (1, 0):
        c = tuned(resident=resident)
        before = c.resident_stats()
        B = lk.krylov_basis_gpu(n, k + 1, dtype, c)
        for which in INPUTS:
            ref = case(n, k, dtype, which)
            X, Y, h1, _h2, y1 = ref[0], ref[1], ref[2], ref[3], ref[4]
            if which == INPUTS[0]:
                B.upload(X, 0)
            label = f"{name(dtype)} n = {n} k = {k} {which} resident = {resident}"
            B.upload(Y, k)
            rc, h, norms, info = dgs_raw(B, k, B, k)
            assert (rc, info) == (LK_OK, 0), (label, rc, info, _capi.load().lk_last_error())
            check_step("a", label, ref, h, norms, B.download(k, 1)[:, 0])
            B.upload(Y, k)
            rc, h, _norms, info = dgs_raw(B, k, B, k, two_pass=False)
            assert (rc, info) == (LK_OK, 0), (label, rc, info)
            close("a", h, h1[:, 0], label + " one pass h1", ref[7][0])
            close("a", B.download(k, 1)[:, 0], y1[:, 0], label + " one pass y'", ref[7][0])
        assert np.array_equal(B.download(0, k), X), "X is read only"
        after = c.resident_stats()
        assert after[:2] == before[:2], (before, after)              # nothing enqueued as a single launch, nothing gave up
        del B


# ---- b. flags and outputs, once per schedule ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", VERY_WIDE_FLAG_K)
@pytest.mark.parametrize("dtype", KINDS)
def test_flags_outputs_and_refusals(dtype, k):
    c = tuned()
    n = very_wide_n(k)
    ref = case(n, k, dtype, "skew_rand")
    X, Y, y2, nrm, scale = ref[0], ref[1], ref[5], ref[6], ref[7][0]
    label = f"{name(dtype)} k = {k}"
    B = lk.krylov_basis_gpu(n, k + 1, dtype, c)
    B.upload(X, 0)

    def run(**kw):
        B.upload(Y, k)
        return dgs_raw(B, k, B, k, **kw) + (B.download(k, 1)[:, 0],)

    rc, h0, norms0, info, y0 = run()
    assert (rc, info) == (LK_OK, 0)
    check_step("b", label, ref, h0, norms0, y0)
    # LK_DGS_NORMALIZE: the same coefficients and norms, y'' / ||y''||
    rc, h, norms, info, y = run(flags=_capi.LK_DGS_NORMALIZE)
    assert (rc, info) == (LK_OK, 0)
    assert np.array_equal(h, h0) and np.array_equal(norms, norms0)
    close("b", y, y2[:, 0] / nrm[0, 2], label + " normalised y''")
    # NULL h, NULL norms, NULL info, each alone: the same y'' bit for bit, and the other outputs as before
    for null in ("h", "norms", "info"):
        rc, h, norms, info, y = run(**{null: False})
        assert rc == LK_OK and np.array_equal(y, y0), (label, null)
        assert null == "h" or np.array_equal(h, h0)
        assert null == "norms" or np.array_equal(norms, norms0)
        assert null == "info" or info == 0
    # y = 0: flagged, left alone, no NaN from the normalisation either
    for flags in (0, _capi.LK_DGS_NORMALIZE):
        B.upload(np.zeros((n, 1), dtype=dtype), k)
        rc, h, norms, info = dgs_raw(B, k, B, k, flags=flags)
        assert (rc, info) == (LK_OK, 1), (label, flags, rc, info)
        assert not norms.any() and not h.any() and not B.download(k, 1).any(), (label, flags, norms)
    # a NaN in y, in a column of the first, of a middle and of the last panel: LK_ERR_NAN; the context serves a clean call afterwards
    w, npan = panels(k)
    bad = Y.copy()
    bad[n // 2, 0] = np.nan
    B.upload(bad, k)
    assert dgs_raw(B, k, B, k)[0] == LK_ERR_NAN, label
    for col in (1, min((npan // 2) * w + 1, k - 1), k - 1):
        xc = X[:, col:col + 1].copy()
        xc[n // 3, 0] = np.nan
        B.upload(xc, col)
        B.upload(Y, k)
        assert dgs_raw(B, k, B, k)[0] == LK_ERR_NAN, (label, col)
        B.upload(X[:, col:col + 1], col)
    rc, h, norms, info, y = run()
    assert (rc, info) == (LK_OK, 0)
    assert np.array_equal(h, h0) and np.array_equal(norms, norms0) and np.array_equal(y, y0), label
    # y among the basis columns, by index and as a view of the same memory: refused, the panel untouched
    B.upload(Y, k)
    whole = B.download()
    assert dgs_raw(B, k, B, k - 1)[0] == LK_ERR_INVALID
    assert dgs_raw(B, k, B.view(k - 1, 1), 0)[0] == LK_ERR_INVALID
    assert dgs_raw(B, k, B.view(k - 1, 1), 0, two_pass=False)[0] == LK_ERR_INVALID
    assert np.array_equal(B.download(), whole)
    del B


# ---- c. launch accounting of the device panels ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [600, 1100, 1600])
@pytest.mark.parametrize("dtype", KINDS)
def test_launches_and_bytes_of_the_device_panels(dtype, k):
    """2, 3 and 4 panels of 512: the engine's own counters (lk_profile_get) show 2 npan - 1 dot sweeps (h1 of every panel, h2 of all but the
    last), ONE fused update + dot sweep (the last panel) and 2 npan - 1 update sweeps, priced at the header's 4k - |last panel| columns of X
    plus the columns of y each sweep reads or writes (1 per dot sweep, 2 per update); the one-pass entry npan + npan."""
    c = tuned()
    n = very_wide_n(k)
    X, Y = second_pass_input(n, k, dtype, "skew_rand")
    npan = (k + KWIDE - 1) // KWIDE
    klast = k - (npan - 1) * KWIDE
    B = lk.krylov_basis_gpu(n, k + 1, dtype, c)
    B.upload(X, 0)
    s = np.dtype(dtype).itemsize
    for two_pass in (True, False):
        B.upload(Y, k)
        c.profile_reset()
        c.profile_enable(True)
        try:
            assert dgs_raw(B, k, B, k, two_pass=two_pass)[0] == LK_OK
            c.sync()
            got = [c.profile_get(f"dgs_sweep{i}") for i in (1, 2, 3)]
            steps = c.profile_get("dgs")[0]
        finally:
            c.profile_enable(False)
        launches, by = [g[0] for g in got], sum(g[2] for g in got)
        if two_pass:
            assert launches == [2 * npan - 1, 1, 2 * npan - 1], (k, launches)
            assert by == pytest.approx(s * n * ((4 * k - klast) + (2 * npan - 1) + 2 + 2 * (2 * npan - 1)))
        else:
            assert launches == [npan, 0, npan], (k, launches)
            assert by == pytest.approx(s * n * (2 * k + npan + 2 * npan))
        assert steps == 1
    del B


# ---- d. caller-owned panels -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["nan_pad", "off48"])
@pytest.mark.parametrize("k", VERY_WIDE_PANEL_K)
@pytest.mark.parametrize("dtype", KINDS)
def test_dgs_on_caller_panels_beyond_512_columns(dtype, k, layout):
    """the device panels (1030) and the host-driven ones (2060) on a wrapped panel whose padding rows are NaN, and on one that starts 48
    bytes into a buffer of live rows: the result of (a), and every word outside the panel's rows unchanged"""
    c = tuned()
    n = very_wide_n(k)
    P = CallerPanel(c, dtype, n, k + 1, layout, seed=k)
    for which in INPUTS:
        ref = case(n, k, dtype, which)
        if which == INPUTS[0]:
            P.set(ref[0])
        P.set(ref[1], k)
        rc, h, norms, info = dgs_raw(P.B, k, P.B, k)
        assert (rc, info) == (LK_OK, 0)
        got = P.get(f"dgs k = {k}")
        check_step("d", f"{name(dtype)} k = {k} {layout} {which}", ref, h, norms, got[:, k])
        assert np.array_equal(got[:, :k], ref[0]), "X is read only"


# ---- e. row-sharded emulation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks", [2, 3])
@pytest.mark.parametrize("k", VERY_WIDE_PANEL_K)
@pytest.mark.parametrize("dtype", KINDS)
def test_sharded_step_beyond_512_columns(dtype, k, nranks):
    """lk_dgs on row blocks of a skewed panel, two and three emulated ranks: every coefficient section and every norm is all-reduced (one
    call per sweep that delivers one: 2 npan + 1 on the device panels, two per panel and pass on the host-driven ones), every rank makes the
    same number of calls and holds the same beta; beta and the gathered y'' against the reference."""
    n = very_wide_n(k)
    refs = [case(n, k, dtype, which) for which in INPUTS]
    refs = [(r[0], r[1]) + r[2:] for r in refs]

    def body(rank, c, row0, nl):
        out = []
        B = lk.krylov_basis_gpu(nl, k + 1, dtype, c)
        B.upload(np.asfortranarray(refs[0][0][row0:row0 + nl]), 0)
        for ref in refs:
            B.upload(np.asfortranarray(ref[1][row0:row0 + nl]), k)
            rc, h, norms, info = dgs_raw(B, k, B, k)
            out.append((rc, info, h, norms, B.download(k, 1)[:, 0]))
        assert np.array_equal(B.download(0, k), refs[0][0][row0:row0 + nl])
        del B
        return out

    res, grp = _sharded(n, nranks, body)
    w, npan = panels(k)
    per_step = 2 * npan + 1 if w == KWIDE else 4 * npan
    assert grp.rank_calls == [len(refs) * per_step] * nranks, (grp.rank_calls, per_step)
    for i, (which, ref) in enumerate(zip(INPUTS, refs)):
        mine = [r[i] for r in res]
        assert all((r[0], r[1]) == (LK_OK, 0) for r in mine)
        assert all(np.array_equal(r[2], mine[0][2]) and np.array_equal(r[3], mine[0][3]) for r in mine)
        check_step("e", f"{name(dtype)} {nranks} ranks k = {k} {which}", ref, mine[0][2], mine[0][3], np.concatenate([r[4] for r in mine]))


# ---- f. lk_innerprod, lk_gram and lk_lincomb ------------------------------------------------------------------------------------------
def _gpu_basis(c, A):
    B = lk.krylov_basis_gpu(A.shape[0], A.shape[1], A.dtype, c)
    B.upload(np.asfortranarray(A))
    return B


@pytest.mark.parametrize("n", [701, 1037])
@pytest.mark.parametrize("dtype", KINDS)
def test_innerprod_beyond_512_columns(dtype, n):
    """X^H Y with 513, 640 and 1025 columns of X: one vector (chunks of 512), three (chunks of 128 on the vector units), seven (128 x 128
    blocks on the matrix cores; with "xhy_mfma" 0 the vector units again, and for the complex kind with four real products per complex
    one too); every entry against the longdouble product, inner length n"""
    c = tuned()
    cp = is_cplx(dtype)
    Y = basis(n, 7, dtype, 8100)
    By = _gpu_basis(c, Y)
    cfgs = [(1, {}), (3, {}), (7, {}), (7, dict(xhy_mfma=0))] + ([(7, dict(gemm_3m=0))] if cp else [])
    for k in (513, 640, 1025):
        X = basis(n, k, dtype, 8200 + k)
        Bx = _gpu_basis(c, X)
        ref = ext(X).conj().T @ ext(Y)
        scale = product_scale(X.conj().T, Y)
        for p, keys in cfgs:
            M = _with(c, keys, lambda: lk.innerprod(Bx, By[:p]))
            entrywise("f", np.asarray(M).reshape(k, p), ref[:, :p], scale[:, :p], n, cp, f"innerprod {name(dtype)} n = {n} k = {k} p = {p} {keys}")
        M1 = lk.innerprod(Bx, By[2])                                # one vector that is not column 0
        entrywise("f", M1, ref[:, 2], scale[:, 2], n, cp, f"innerprod {name(dtype)} n = {n} k = {k} vector")
        del Bx
    del By


@pytest.mark.parametrize("k", [513, 641])
@pytest.mark.parametrize("dtype", KINDS)
def test_gram_beyond_512_columns(dtype, k):
    """Gram(X) on 5 x 5 and 6 x 6 blocks of 128 (the last one a single column): the upper triangle entrywise, the mirror without
    conjugation (AbstractVectors.fypp:650-655), and a complex diagonal whose imaginary part is exactly zero"""
    c = tuned()
    cp = is_cplx(dtype)
    n = 701
    X = basis(n, k, dtype, 8300 + k)
    B = _gpu_basis(c, X)
    ref = ext(X).conj().T @ ext(X)
    scale = product_scale(X.conj().T, X)
    iu = np.triu_indices(k)
    for keys in [{}] + ([dict(gemm_3m=0)] if cp else []):
        G = _with(c, keys, lambda: lk.Gram(B))
        entrywise("f", G[iu], ref[iu], scale[iu], n, cp, f"gram {name(dtype)} k = {k} {keys}")
        assert np.array_equal(G, np.triu(G) + np.triu(G, 1).T)
        if cp:
            assert not np.diag(G).imag.any()
    del B


@pytest.mark.parametrize("k", [513, 1100])
@pytest.mark.parametrize("dtype", KINDS)
def test_lincomb_beyond_512_columns(dtype, k):
    """Y = X C over 5 and 9 chunks of 128 columns (the last of one column / of 76): one and three outputs on the vector units, seventeen
    on the matrix cores (the complex kind with three and with four real products); every entry against the longdouble product, inner
    length k.  The reference shows that a product which loses a chunk -- the first 128 columns alone, or the last chunk alone -- is off by
    far more than the bound in nearly every entry."""
    c = tuned()
    cp = is_cplx(dtype)
    n = 701
    lib = _capi.load()
    X = basis(n, k, dtype, 8400 + k)
    Bx = _gpu_basis(c, X)
    for q in (1, 3, 17):
        Cm = basis(k, q, dtype, 8500 + k + q)
        ref = ext(X) @ ext(Cm)
        scale = product_scale(X, Cm)
        tail = (k - 1) // KFUSED * KFUSED
        for part in (ext(X[:, :KFUSED]) @ ext(Cm[:KFUSED]), ext(X[:, tail:]) @ ext(Cm[tail:])):
            assert (np.abs(part - ref) > 1e6 * 4 * k * 2.0 ** -53 * scale).mean() > 0.99
        By = lk.krylov_basis_gpu(n, q + 1, dtype, c)
        for keys in [{}] + ([dict(gemm_3m=0)] if cp and q == 17 else []):
            By.upload(np.full((n, q + 1), np.nan, dtype=dtype))     # (an output the kernel must overwrite, not add to)
            _with(c, keys, lambda: _capi.check(lib.lk_lincomb(Bx._h, k, Cm.ctypes.data_as(_DP), q, By._h, 1)))
            got = By.download()
            entrywise("f", got[:, 1:], ref, scale, k, cp, f"lincomb {name(dtype)} k = {k} q = {q} {keys}")
            assert np.isnan(got[:, 0]).all()                         # the column before the output range is not touched
        del By
    assert np.array_equal(Bx.download(), X)
    del Bx


# ---- g. lk_dgs_block, column by column beyond 512 columns ----------------------------------------------------------------------------
@pytest.mark.parametrize("p", [3, 6])
@pytest.mark.parametrize("k", VERY_WIDE_BLOCK_K)
@pytest.mark.parametrize("dtype", KINDS)
def test_block_step_beyond_512_columns(dtype, k, p):
    """p = 3 and 6 columns against 600 and 1100: each column through lk_dgs (the engine's counters show p steps), against dgs_longdouble;
    info = the LAST zero column (gram_schmidt.fypp:171-173), 1-based"""
    c = tuned()
    n = very_wide_n(k)
    Bx = lk.krylov_basis_gpu(n, k, dtype, c)
    By = lk.krylov_basis_gpu(n, p, dtype, c)
    for which in INPUTS:
        ref = case(n, k, dtype, which, 6)
        X, Y = ref[0], ref[1][:, :p]
        if which == INPUTS[0]:
            Bx.upload(X)
        By.upload(Y)
        h = np.full((k, p), np.nan, dtype=dtype, order="F")
        c.profile_reset()
        c.profile_enable(True)
        try:
            assert lk.double_gram_schmidt_step(By, Bx, False, beta=h) == 0
            c.sync()
            steps = c.profile_get("dgs")[0]
        finally:
            c.profile_enable(False)
        assert steps == p
        got = By.download()
        for j in range(p):
            check_step("g", f"{name(dtype)} k = {k} p = {p} {which} column {j}", ref, h[:, j], None, got[:, j], j)
    assert np.array_equal(Bx.download(), X), "X is read only"
    Z = np.array(Y)
    Z[:, 1] = 0
    By.upload(Z)
    assert lk.double_gram_schmidt_step(By, Bx, False) == 2
    assert not By.download(1, 1).any()
    Z[:, 0] = 0
    Z[:, 1] = Y[:, 1]
    By.upload(Z)
    assert lk.double_gram_schmidt_step(By, Bx, False) == 1
    del Bx, By


# ---- h. lk_qr on 530 columns ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", KINDS)
def test_qr_of_530_columns(dtype):
    """qr_no_pivoting (qr.fypp:116-167) of a skewed 541 x 530 panel: from column 513 on the step runs on a view of the leading columns
    in two device panels.  R, Q, Q R = A and Q^H Q = I with the tolerances of tests/test_gpu_block_arnoldi.py, against ora.qr_no_pivoting;
    then column 520 an exact copy of column 3: info = 521, R(520, 520) = 0, and the re-drawn column -- orthogonalised by the same step
    with NULL outputs -- has unit norm and is orthogonal to the 520 before it."""
    c = tuned()
    n, p = 541, 530
    A = skewed_basis(n, p, dtype, 40 + p)
    B = lk.krylov_basis_gpu(n, p, dtype, c)
    B.upload(A)
    R = np.zeros((p, p), dtype=dtype, order="F")
    Ao, Ro = A.copy(order="F"), np.zeros((p, p), dtype=dtype, order="F")
    assert lk.qr(B, R) == ora.qr_no_pivoting(Ao, Ro) == 0
    Q = B.download()
    columns_close("h", R, Ro, f"qr {name(dtype)} R")
    assert np.abs(Q - Ao).max() <= 1e-12
    assert np.abs(A - Q @ R).max() <= 1e-12 * np.abs(A).max() * p
    assert np.abs(Q.conj().T @ Q - np.eye(p)).max() <= 1e-12
    WORST["h"] = max(WORST["h"], float(np.abs(Q - Ao).max()) / 1e-12, float(np.abs(Q.conj().T @ Q - np.eye(p)).max()) / 1e-12)
    A2 = A.copy(order="F")
    A2[:, 520] = A2[:, 3]
    B.upload(A2)
    assert lk.qr(B, R, tol=1e-10) == 521
    assert R[520, 520] == 0
    Q = B.download()
    orth, unit = float(np.abs(Q[:, :520].conj().T @ Q[:, 520]).max()), abs(float(np.linalg.norm(Q[:, 520])) - 1.0)
    assert orth <= 1e-12 and unit <= 1e-12, (orth, unit)
    assert np.abs(Q.conj().T @ Q - np.eye(p)).max() <= 1e-12
    keep = [j for j in range(p) if j != 520]
    assert np.abs(A2[:, keep] - Q @ R[:, keep]).max() <= 1e-12 * np.abs(A2).max() * p
    WORST["h"] = max(WORST["h"], orth / 1e-12, unit / 1e-12)
    del B


# ---- i. one step of each factorisation from a prepared basis --------------------------------------------------------------------------
@pytest.mark.parametrize("k0", VERY_WIDE_PANEL_K)
@pytest.mark.parametrize("dtype", KINDS)
def test_one_step_of_each_factorisation_from_a_very_wide_block(dtype, k0):
    """lk_arnoldi, lk_lanczos, lk_bidiag and lk_arnoldi_block (p = 2) with kstart = kend on k0 = 1030 and 2060 uploaded skewed columns
    (as part d of tests/test_gpu_second_pass.py): the new column of H / T / B normwise per column and the new basis vectors against the
    longdouble step, which tests/test_oracle_very_wide.py ties to the oracle.  (A whole factorisation of a thousand steps is not compared:
    rounding differences grow along it.)"""
    c = tuned()
    n = very_wide_n(k0)
    label = f"{name(dtype)} k0 = {k0}"
    d = arnoldi_operator(n, dtype)
    X0 = second_pass_input(n, k0, dtype, "skew_rand")[0]              # = skewed_basis(n, k0, dtype, 40 + k0)

    def start(ncols, lead=X0):
        S = np.zeros((n, ncols), dtype=dtype, order="F")
        S[:, :lead.shape[1]] = lead
        B = lk.krylov_basis_gpu(n, ncols, dtype, c)
        B.upload(S)
        return B

    X = start(k0 + 1)
    H = np.zeros((k0 + 1, k0), dtype=dtype, order="F")
    assert lk.arnoldi(lk.diag_linop_gpu(d, c), X, H, kstart=k0, kend=k0) == 0
    hcol, x = arnoldi_step_longdouble(d, X0)
    columns_close("i", H[:, k0 - 1:], hcol.reshape(-1, 1), label + " arnoldi")
    assert not H[:, :k0 - 1].any()
    got = X.download()
    assert np.array_equal(got[:, :k0], X0)                            # the leading block is the caller's
    close("i", got[:, k0], x, label + " arnoldi vector")
    del X

    dh = (1.0 + np.arange(n) / n).astype(dtype)                      # Hermitian
    X = start(k0 + 1)
    T = np.zeros((k0 + 1, k0), dtype=dtype, order="F")
    assert lk.lanczos(lk.diag_linop_gpu(dh, c), X, T, kstart=k0, kend=k0) == 0
    tcol, x = lanczos_step_longdouble(dh, X0)
    columns_close("i", T[:, k0 - 1:], tcol.reshape(-1, 1), label + " lanczos")
    close("i", X.download(k0, 1)[:, 0], x, label + " lanczos vector")
    del X

    V0 = skewed_basis(n, k0 - 1, dtype, 900)                          # step k0 orthogonalises A^H u_k0 against v_1 .. v_(k0 - 1)
    U, V = start(k0 + 1), start(k0, V0)
    Bm = np.zeros((k0 + 1, k0), dtype=dtype, order="F")
    assert lk.bidiagonalization(lk.diag_linop_gpu(d, c), U, V, Bm, kstart=k0, kend=k0) == 0
    alpha, vk, beta, u = bidiag_step_longdouble(d, X0, V0)
    bcol = np.zeros(k0 + 1, dtype=hcol.dtype)
    bcol[k0 - 1], bcol[k0] = alpha, beta
    columns_close("i", Bm[:, k0 - 1:], bcol.reshape(-1, 1), label + " bidiag")
    close("i", V.download(k0 - 1, 1)[:, 0], vk, label + " bidiag v")
    close("i", U.download(k0, 1)[:, 0], u, label + " bidiag u")
    del U, V

    p = 2
    X = start(k0 + p)
    H = np.zeros((k0 + p, k0), dtype=dtype, order="F")
    assert lk.arnoldi(lk.diag_linop_gpu(d, c), X, H, kstart=k0 // p, kend=k0 // p, blksize=p) == 0
    Hb, R, W = arnoldi_block_step_longdouble(d, X0, p)
    columns_close("i", H[:, k0 - p:], np.concatenate([Hb, R]), label + " arnoldi_block p = 2")
    close("i", X.download(k0, p), W, label + " arnoldi_block vectors")
    del X
