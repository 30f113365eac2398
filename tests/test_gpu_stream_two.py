"""Sweep 3 of the recomputing Gram-Schmidt step one column at a time (tuning key "stream_two", panel_update<.., true>) against the tile
kernel (panel_sweep<.., TWO>) on the three sweeps ("resident" 0).

The column walk adds, per row, what the tile kernel adds with sweep 2's wave split (WC, kcw): a column group's share in slot order
from zero, the groups' shares from zero in the order of the LDS exchange, both coefficient sets, then y - s - s2.  So for the same X,
y, h1 and h2 -- sweeps 1 and 2 do not read the key -- y'' and h must come out BYTE FOR BYTE.  Only ||y''|| is summed over another
row-to-lane mapping: it is held to the bound tests/test_gpu_parity.py uses for a norm (1e-12, relative) against the longdouble norm of
the y'' the call returned, on both routes.

Shapes: the smallest at which the order or the tiling can go wrong -- one group, two and three groups with a short last one, every group
full (k = 128), ragged runs, an n one below and one above a whole run (8192 real rows; 2048 / 4096 complex rows for the 1024- / 512-thread
block), an n at which blocks take more than one run, and one panel of 2^25 real rows, the size at which the real kind moves to 32-column
register tiles (WC = 2, kcw = 17 at k = 33).  The inputs are the skewed panels of tests/test_gpu_second_pass.py, so h2 is not noise."""
import functools

import numpy as np
import pytest

import lightkrylov_amd as lk
from oracle import oracle as ora
from tests._gpu_helpers import KINDS, assert_second_pass_matters, dgs_longdouble, second_pass_input, seeded
from tests._tol import assert_close, assert_columns_close

pytestmark = pytest.mark.gpu

DEFAULT_TWO = 2              # the engine's default of the key (by size), put back after every use
RTOL_NORM = 1e-12            # tests/test_gpu_parity.py: |norm - reference| <= 1e-12 * reference

# (n, k): see the module docstring.  2 100 001 real rows = 257 runs of 8192 rows on at most 256 blocks; 1 100 001 complex rows at k = 33
# (512-thread blocks, runs of 4096 rows) and 600 001 at k = 2 (1024-thread blocks, runs of 2048 rows) likewise
SHAPES = [(1, 1), (65, 8), (999, 3), (4097, 17), (4097, 33), (5003, 128), (8191, 5), (8193, 5), (2047, 5), (2049, 5), (4095, 33)]
LONG = {np.float64: [(2_100_001, 2)], np.complex128: [(600_001, 2), (1_100_001, 33)]}


@pytest.fixture(scope="module")
def c():
    ctx = lk.Context(device=0)
    ctx.set_tuning("resident", 0)
    yield ctx
    ctx.close()
    case.cache_clear()


@functools.lru_cache(maxsize=None)
def case(n, k, dtype):
    X, Y = second_pass_input(n, k, dtype, "skew_rand")
    # the guard of tests/test_gpu_second_pass.py on the input, where it applies: a panel with room to be nearly orthonormal, and short
    # enough that max |h2| (about 1e-3 |h1|, |h1| about 1) is measured against a |y| = sqrt(n / 3) of the same order.  On the long
    # panels h2 X still changes every entry of y'' by 10^9 ulps, which is what a byte comparison needs
    if 4 * k <= n <= 10_000:
        h1, h2, _y1, _y2 = dgs_longdouble(Y[:, 0], X)
        assert_second_pass_matters(h1, h2, Y[:, 0])
    return X, Y


def step(ctx, B, k, y, two):
    """lk_dgs of y (uploaded into column k) against columns 0 .. k-1 of B with "stream_two" = two: h, y'', ||y''||"""
    ctx.set_tuning("stream_two", two)
    try:
        B.upload(y.reshape(-1, 1), k)
        h = np.zeros(k, dtype=y.dtype)
        norms = []
        assert lk.double_gram_schmidt_step(B[k], B[:k], False, beta=h, _norms=norms) == 0
        return h, B.download(k, 1)[:, 0], norms[2]
    finally:
        ctx.set_tuning("stream_two", DEFAULT_TWO)


def compare(tile, cw, label):
    (h0, y0, b0), (h1, y1, b1) = tile, cw
    assert h0.tobytes() == h1.tobytes(), f"{label}: h differs between the routes"
    assert y0.tobytes() == y1.tobytes(), f"{label}: y'' differs between the routes ({np.count_nonzero(y0 != y1)} of {y0.size} entries)"
    yl = y1.astype(np.clongdouble if y1.dtype.kind == "c" else np.longdouble)
    ref = float(np.sqrt(np.sum(yl.real * yl.real + yl.imag * yl.imag)))
    for name, b in (("tile", b0), ("column walk", b1)):
        print(f"{label}: ||y''|| {name} {b!r} longdouble {ref!r} rel {abs(b - ref) / max(ref, 1e-300):.2e}")
        assert abs(b - ref) <= RTOL_NORM * ref, f"{label}: ||y''|| of the {name} route off by {abs(b - ref) / ref:.2e}"


@pytest.mark.parametrize("dtype", KINDS, ids=["f64", "c128"])
def test_column_walk_writes_the_tile_kernels_bytes(c, dtype):
    for n, k in SHAPES + LONG[dtype]:
        X, Y = case(n, k, dtype)
        B = lk.krylov_basis_gpu(n, k + 1, dtype, c)
        B.upload(X, 0)
        tile = step(c, B, k, Y[:, 0], 0)
        cw = step(c, B, k, Y[:, 0], 1)
        compare(tile, cw, f"stream_two {np.dtype(dtype).name} n = {n} k = {k}")
        assert np.array_equal(B.download(0, k), X), "X is read only"
        del B


def test_column_walk_on_the_long_panel_shape():
    """2^25 real rows, k = 33: the 32-column register tiles of long panels (two groups of 17 and 16 columns), filled on the device.  The
    columns are unit random vectors, not orthonormal: h1 and h2 are both far from zero."""
    n, k = 1 << 25, 33
    ctx = lk.Context(device=0)
    try:
        ctx.set_tuning("resident", 0)
        B = lk.krylov_basis_gpu(n, k + 1, np.float64, ctx)
        for j in range(k):
            B[j].rand(True, seed=300 + j)
        out = []
        for two in (None, 0, 1):                     # None: the context as lk_init leaves it -- the size rule that ships (2)
            if two is not None:
                ctx.set_tuning("stream_two", two)
            B[k].rand(True, seed=299)
            h = np.zeros(k)
            norms = []
            assert lk.double_gram_schmidt_step(B[k], B[:k], False, beta=h, _norms=norms) == 0
            out.append((h, B.download(k, 1)[:, 0], norms[2]))
        compare(out[1], out[2], f"stream_two float64 n = 2^25 k = {k}")
        compare(out[1], out[0], f"stream_two float64 n = 2^25 k = {k}, the default against 0")
        # this panel is above the size rule, so the default took the column walk: its norm is the forced route's, bit for bit
        assert out[0][2] == out[2][2], "the default did not take the route of stream_two = 1 on a panel above the size rule"
    finally:
        ctx.close()


def _operator(ctx, which, n, dtype):
    if which == "lin":
        return lk.diag_linop_gpu(n_local=n, row0=0, d0=1.0, dstep=1.0 / n, ctx=ctx)
    g = np.arange(n) / n
    d = (1.0 + g) * (np.exp(1j * g) if np.dtype(dtype).kind == "c" else 1.0)
    return lk.diag_linop_gpu(d.astype(dtype), ctx)


ARNOLDI = [("lin", np.float64, False), ("d", np.float64, False), ("d", np.complex128, False), ("d", np.complex128, True)]


@pytest.mark.parametrize("which,dtype,transpose", ARNOLDI, ids=["linspace_f64", "d_f64", "d_c128", "d_c128_adjoint"])
def test_arnoldi_on_the_column_walk_with_and_without_the_fused_operator(c, which, dtype, transpose):
    """lk_arnoldi, 12 steps at n = 4096 with "stream_two" 1: forming y = D x_k inside the sweeps ("fuse_rowop" 1) gives the bytes the
    operator kernel's y gives (0), and H and the basis agree with the oracle."""
    n, m = 4096, 12
    x0 = seeded(n, dtype, 7)
    x0 /= np.linalg.norm(x0)
    out = {}
    c.set_tuning("stream_two", 1)
    try:
        for fuse in (0, 1):
            c.set_tuning("fuse_rowop", fuse)
            X = lk.krylov_basis_gpu(n, m + 1, dtype, c)
            X.upload(x0.reshape(-1, 1), 0)
            H = np.zeros((m + 1, m), dtype=dtype, order="F")
            assert lk.arnoldi(_operator(c, which, n, dtype), X, H, transpose=transpose) == 0
            out[fuse] = (H, X.download())
            del X
    finally:
        c.set_tuning("fuse_rowop", 1)
        c.set_tuning("stream_two", DEFAULT_TWO)
    assert out[0][0].tobytes() == out[1][0].tobytes(), "H differs between fuse_rowop = 0 and 1"
    assert out[0][1].tobytes() == out[1][1].tobytes(), "the basis differs between fuse_rowop = 0 and 1"
    g = np.arange(n) / n
    d = ((1.0 + g) * (np.exp(1j * g) if np.dtype(dtype).kind == "c" else 1.0)).astype(dtype)
    Xo = np.zeros((n, m + 1), dtype=dtype, order="F")
    Xo[:, 0] = x0
    Ho = np.zeros((m + 1, m), dtype=dtype, order="F")
    assert ora.arnoldi(ora.DiagOp(d.conj() if transpose else d), Xo, Ho) == 0
    label = f"stream_two Arnoldi vs oracle ({which}, {np.dtype(dtype).name}, adjoint = {transpose})"
    assert_columns_close(out[1][0], Ho, label)
    assert_close(out[1][1], Xo, label + " basis")      # (unit columns, entrywise against max |x|: tests/test_gpu_second_pass.py's bare 1e-12)


@pytest.mark.parametrize("dtype", KINDS, ids=["f64", "c128"])
def test_breakdown_on_the_column_walk_leaves_the_columns_behind_it(c, dtype):
    """six distinct eigenvalues: invariant subspace after 6 steps; the marker columns behind the stopped step survive"""
    n, m = 4096, 12
    d6 = (1.0 + (np.arange(n) % 6)).astype(dtype)
    marker = seeded(n, dtype, 123)
    c.set_tuning("stream_two", 1)
    try:
        X = lk.krylov_basis_gpu(n, m + 1, dtype, c)
        X[0].rand(True, seed=9)
        for j in range(7, m + 1):
            X.upload(marker.reshape(-1, 1), j)
        H = np.zeros((m + 1, m), dtype=dtype, order="F")
        assert lk.arnoldi(lk.diag_linop_gpu(d6, c), X, H, tol=1e-10) == 6
        Xh = X.download()
    finally:
        c.set_tuning("stream_two", DEFAULT_TWO)
    for j in range(7, m + 1):
        assert np.array_equal(Xh[:, j], marker), f"column {j} behind the breakdown was touched"
