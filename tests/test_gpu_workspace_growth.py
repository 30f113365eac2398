"""A context whose workspaces other shapes have grown gives the same bits as a fresh one.

The engine's workspaces (the product workspace `xhy`, the block coefficient sections `blk_red`, the per-step slots `step_red`, the
Lanczos sections `lz_red`, the segment stop flags, the scratch vector) grow on demand and are never shrunk; which kernel runs, on what
grid and in what order of summation, must depend on the call's shape and the tuning keys alone, never on what an earlier call left
allocated.  One context (`grown`) serves every test of this module in file order; each entry runs at a small shape, a larger one and
the small one again, and every call is repeated in a context created for that call alone.  The two must agree byte for byte in every
host result (H / T / B / R / h / G), in `info` and in every basis column the call wrote.  No tolerance: the same kernels on the same
data.  "resident" = 0 in both contexts: a single launch that gives up on a shared chip would change the schedule of one side only.

n = 4099 (real) / 2053 (complex): a few row tiles, fewer than the CU count -- where a pass of the block Gram-Schmidt needs less of
`xhy` than the fused pass behind it, the regime of the sizing bug that tests/test_gpu_far_columns.py guards by its k = 64-then-128 order.

The last test creates and destroys twenty operators of every kind and two contexts, and destroys an operator AFTER its context was
finalised (the order the header allows)."""
import ctypes as C

import numpy as np
import pytest

import lightkrylov_amd as lk
from lightkrylov_amd import _capi
from tests._gpu_helpers import KINDS, basis, is_cplx, orthonormal_basis, seeded

pytestmark = pytest.mark.gpu

_DP = C.POINTER(C.c_double)
N = {np.dtype(np.float64): 4099, np.dtype(np.complex128): 2053}


def _ctx(**keys):
    c = lk.Context(device=0)
    c.set_tuning("resident", 0)
    for k, v in keys.items():
        c.set_tuning(k, v)
    return c


@pytest.fixture(scope="module")
def grown():
    c = _ctx()
    yield c
    c.close()


def same_as_fresh(grown, call, what, **keys):
    """call(ctx) -> tuple of host arrays / ints, run in the grown context and in a fresh one (both with the tuning `keys`)"""
    for k, v in keys.items():
        grown.set_tuning(k, v)
    got = call(grown)
    fresh = _ctx(**keys)
    try:
        ref = call(fresh)
    finally:
        fresh.close()
    assert len(got) == len(ref)
    for i, (a, b) in enumerate(zip(got, ref)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what}: result {i} differs from a fresh context's"
    return got


def _n(dtype):
    return N[np.dtype(dtype)]


def _start(dtype, seed=7):
    x = seeded(_n(dtype), dtype, seed)
    return x / np.linalg.norm(x)


def _diag(dtype, hermitian=False):
    g = np.arange(_n(dtype)) / _n(dtype)
    return ((1.0 + g) * (np.exp(0.4j * g) if is_cplx(dtype) and not hermitian else 1.0)).astype(dtype)


_CACHE = {}


def _cached(key, make):
    """host inputs computed once per module and never written"""
    if key not in _CACHE:
        _CACHE[key] = make()
        _CACHE[key].setflags(write=False)
    return _CACHE[key]


# ---- lk_dgs_block: xhy, blk_red and the may_grow rule -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", KINDS)
def test_block_gram_schmidt(grown, dtype):
    n, lib = _n(dtype), _capi.load()
    for k, p in ((64, 17), (128, 17), (200, 40), (64, 17)):
        Q = _cached(("Q", np.dtype(dtype), k), lambda: orthonormal_basis(n, k, dtype, 60 + k))
        Y = _cached(("Y", np.dtype(dtype), p), lambda: basis(n, p, dtype, 700 + p))

        def call(c):
            B = lk.krylov_basis_gpu(n, k + p, dtype, c)
            B.upload(Q, 0)
            B.upload(Y, k)
            h, info = np.zeros((k, p), dtype=dtype, order="F"), C.c_int()
            _capi.check(lib.lk_dgs_block(B._h, k, B._h, k, p, h.ctypes.data_as(_DP), C.byref(info)))
            out = B.download(k, p)
            B.close()
            return h, info.value, out

        h, info, out = same_as_fresh(grown, call, f"lk_dgs_block k={k} p={p} {np.dtype(dtype).name}")
        assert info == 0 and np.isfinite(h).all() and np.isfinite(out).all()


# ---- the factorisations: step_red (across the change of section stride at 128 columns), seg_stop_host, lz_red ---------------------------
def _factorise(dtype, kdim, what, d, run, two_bases=False):
    """call(ctx) for a factorisation of `kdim` steps on the diagonal operator d: returns (projected matrix, info, basis[, second basis])"""
    n, x0 = _n(dtype), _start(dtype)

    def call(c):
        A = lk.diag_linop_gpu(d, c)
        X = lk.krylov_basis_gpu(n, kdim + 1, dtype, c)
        X.upload(x0.reshape(-1, 1), 0)
        M = np.zeros((kdim + 1, kdim), dtype=dtype, order="F")
        if two_bases:
            V = lk.krylov_basis_gpu(n, kdim, dtype, c)
            info = run(A, X, V, M)
            out = (M, info, X.download(), V.download())
            V.close()
        else:
            info = run(A, X, M)
            out = (M, info, X.download())
        X.close()
        A.close()
        return out
    return call


@pytest.mark.parametrize("dtype", KINDS)
def test_arnoldi(grown, dtype):
    for kdim in (8, 200, 8):
        call = _factorise(dtype, kdim, "arnoldi", _diag(dtype), lambda A, X, H: lk.arnoldi(A, X, H))
        H, info, X = same_as_fresh(grown, call, f"lk_arnoldi kdim={kdim} {np.dtype(dtype).name}")
        assert info == 0 and np.isfinite(H).all() and np.isfinite(X).all()


@pytest.mark.parametrize("dtype", KINDS)
def test_arnoldi_segments(grown, dtype):
    kdim = 12
    for nseg in (1, 6, 1):
        segs = tuple(range(kdim // nseg, kdim + 1, kdim // nseg))
        seen = []

        def run(A, X, H):
            del seen[:]
            return lk.arnoldi(A, X, H, _segments=segs, _progress=lambda a, b: seen.append((a, b)) and 0)

        call = _factorise(dtype, kdim, "segments", _diag(dtype), run)
        H, info, _X = same_as_fresh(grown, call, f"lk_arnoldi_segments {nseg} segments {np.dtype(dtype).name}")
        assert info == 0 and np.isfinite(H).all()
        assert [b for _a, b in seen] == list(segs), (seen, segs)


@pytest.mark.parametrize("dtype", KINDS)
def test_lanczos(grown, dtype):
    for kdim in (4, 40, 4):
        call = _factorise(dtype, kdim, "lanczos", _diag(dtype, hermitian=True), lambda A, X, T: lk.lanczos(A, X, T))
        T, info, _X = same_as_fresh(grown, call, f"lk_lanczos kdim={kdim} {np.dtype(dtype).name}")
        assert info == 0 and np.isfinite(T).all()


@pytest.mark.parametrize("dtype", KINDS)
def test_bidiag(grown, dtype):
    for kdim in (3, 30):
        call = _factorise(dtype, kdim, "bidiag", _diag(dtype), lambda A, U, V, B: lk.bidiagonalization(A, U, V, B), two_bases=True)
        B, info, _U, _V = same_as_fresh(grown, call, f"lk_bidiag kdim={kdim} {np.dtype(dtype).name}")
        assert info == 0 and np.isfinite(B).all()


@pytest.mark.parametrize("dtype", KINDS)
def test_qr(grown, dtype):
    n = _n(dtype)
    for p in (2, 8):
        M0 = _cached(("M0", np.dtype(dtype), p), lambda: basis(n, p, dtype, 300))

        def call(c):
            B = lk.krylov_basis_gpu(n, p, dtype, c)
            B.upload(M0)
            R, info = np.zeros((p, p), dtype=dtype, order="F"), C.c_int()
            _capi.check(_capi.load().lk_qr(B._h, 0, p, R.ctypes.data_as(_DP), p, 1e-12, C.byref(info)))
            out = B.download()
            B.close()
            return R, info.value, out

        R, info, _Q = same_as_fresh(grown, call, f"lk_qr p={p} {np.dtype(dtype).name}")
        assert info == 0 and np.isfinite(R).all()


# ---- lk_gram and lk_lincomb: xhy and the scratch vector ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", KINDS)
def test_gram_and_lincomb(grown, dtype):
    n, q, lib = _n(dtype), 4, _capi.load()
    for k in (8, 128):
        X = _cached(("X", np.dtype(dtype), k), lambda: basis(n, k, dtype, 500 + k))
        Cm = _cached(("C", np.dtype(dtype), k), lambda: basis(k, q, dtype, 900 + k))

        def call(c):
            B = lk.krylov_basis_gpu(n, k + q, dtype, c)
            B.upload(X, 0)
            G = np.zeros((k, k), dtype=dtype, order="F")
            _capi.check(lib.lk_gram(B._h, k, G.ctypes.data_as(_DP)))
            _capi.check(lib.lk_lincomb(B._h, k, Cm.ctypes.data_as(_DP), q, B._h, k))
            out = B.download(k, q)
            B.close()
            return G, out

        G, out = same_as_fresh(grown, call, f"lk_gram / lk_lincomb k={k} {np.dtype(dtype).name}")
        assert np.isfinite(G).all() and np.isfinite(out).all()


# ---- lk_linop_apply of a CSR operator through both kernels ------------------------------------------------------------------------------
def _csr(dtype):
    """five entries per row (the diagonal and four pseudo-random columns), 0-based CSR"""
    n = _n(dtype)
    rng = np.random.default_rng(11)
    cols = np.sort(np.concatenate([np.arange(n).reshape(-1, 1), rng.integers(0, n, (n, 4))], axis=1), axis=1)
    vals = rng.standard_normal(5 * n) + (1j * rng.standard_normal(5 * n) if is_cplx(dtype) else 0.0)
    return np.arange(0, 5 * n + 1, 5, dtype=np.int64), cols.reshape(-1).astype(np.int32), vals.astype(dtype)


@pytest.mark.parametrize("dtype", KINDS)
def test_csr_apply_on_one_operator(grown, dtype):
    """ONE operator of the grown context through "csr_stream" = 0 (the lanes-per-row kernel), then 1 (the LDS stream), then 0 again: each
    against a fresh context and a fresh operator with the same key.  What a call chooses for itself never stays in the operator."""
    n, x = _n(dtype), seeded(_n(dtype), dtype, 99)
    A_host = _csr(dtype)
    A_grown = lk.csr_linop_gpu(A_host, grown)

    def call(c):
        A = A_grown if c is grown else lk.csr_linop_gpu(A_host, c)
        xv, yv, zv = lk.dense_vector_gpu.from_array(x, c), lk.dense_vector_gpu(n, dtype, c), lk.dense_vector_gpu(n, dtype, c)
        A.apply_matvec(xv, yv)
        A.apply_rmatvec(xv, zv)
        out = yv.to_array(), zv.to_array()
        if c is not grown:
            A.close()
        return out

    try:
        first = None
        for stream in (0, 1, 0):
            y, z = same_as_fresh(grown, call, f"csr apply csr_stream={stream} {np.dtype(dtype).name}", csr_stream=stream)
            assert np.isfinite(y).all() and np.isfinite(z).all()
            if stream == 0:
                first = first or (y.tobytes(), z.tobytes())
                assert first == (y.tobytes(), z.tobytes())
    finally:
        A_grown.close()
        grown.set_tuning("csr_stream", 1)


# ---- lifetimes --------------------------------------------------------------------------------------------------------------------------
def test_operator_and_context_lifetimes(grown):
    """Twenty operators of every kind created and destroyed in two contexts; a wrapped dense matrix is still the caller's afterwards;
    an operator destroyed after its context's lk_finalize; the grown context still computes afterwards."""
    n = 257
    d = {dt: (1.0 + np.arange(n) / n).astype(dt) for dt in KINDS}
    Ad = {dt: basis(n, n, dt, 40) for dt in KINDS}
    rowptr = np.arange(0, 2 * n + 1, 2, dtype=np.int64)
    colind = np.stack([np.arange(n), (np.arange(n) + 1) % n], axis=1).reshape(-1).astype(np.int32)
    for _round in range(2):
        c = _ctx()
        panel = lk.krylov_basis_gpu(n, n, np.float64, c)
        panel.upload(Ad[np.float64])
        for _i in range(20):
            made = [lk.diag_linop_gpu(n_local=n, row0=0, d0=1.0, dstep=1.0 / n, ctx=c), lk.laplacian2d_linop_gpu(16, c),
                    lk.ginzburg_landau_linop_gpu(n, c), lk.dense_linop_gpu.from_device_panel(panel, row_starts=[0, n])]
            for dt in KINDS:
                made += [lk.diag_linop_gpu(d[dt], c), lk.dense_linop_gpu(Ad[dt], c), lk.csr_linop_gpu((rowptr, colind, np.ones(2 * n, dtype=dt)), c)]
            for op in made:
                op.close()
        assert panel.download().tobytes() == Ad[np.float64].tobytes()              # wrapped memory: never freed, never written
        panel.close()
        c.close()
    c = _ctx()
    late = [lk.diag_linop_gpu(d[np.float64], c), lk.dense_linop_gpu(Ad[np.complex128], c), lk.laplacian2d_linop_gpu(16, c),
            lk.ginzburg_landau_linop_gpu(n, c), lk.csr_linop_gpu((rowptr, colind, np.ones(2 * n)), c)]
    c.close()
    for op in late:
        op.close()
    call = _factorise(np.float64, 8, "arnoldi", _diag(np.float64), lambda A, X, H: lk.arnoldi(A, X, H))
    same_as_fresh(grown, call, "lk_arnoldi after the lifetime cycles")
