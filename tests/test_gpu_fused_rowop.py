"""The asynchronous Arnoldi batch on a diagonal operator forms y = D x_k inside the three Gram-Schmidt sweeps (tuning key "fuse_rowop",
default 1: no operator kernel, y never in memory) -- and must return BIT FOR BIT what it returns when the operator kernel writes y
first ("fuse_rowop" = 0): the same single multiplication per row produces y and the sweeps keep their summation order.  Compared here
as bytes of H and of the whole basis for the generated (linspace) and the explicit diagonal, both kinds, the adjoint of the complex
kind, and the sweep shapes a step can take; with a breakdown (marker columns beyond it survive), with a NaN in x0, against the oracle,
and by counting the operator launches the engine's profile records.

lk_lanczos keeps the operator kernel (its two one-column passes update y in place before the re-orthogonalisation), and so does the
single launch of a cache-resident step and a complex basis of more than 128 columns: those cases pass here because nothing changed,
and they are in the list so that they keep passing when that changes."""
import numpy as np
import pytest

import lightkrylov_amd as lk
from lightkrylov_amd import _capi
from oracle import oracle as ora
from tests._gpu_helpers import seeded
from tests._tol import assert_columns_close

pytestmark = pytest.mark.gpu


@pytest.fixture()
def fresh():
    ctxs = []

    def make(**kw):
        c = lk.Context(device=0)
        for key, val in kw.items():
            c.set_tuning(key, val)
        ctxs.append(c)
        return c
    yield make
    for c in ctxs:
        c.close()


def _operator(c, which, n, dtype):
    """"lin": the generated diagonal d_i = 1 + i / n (real kind only); "d": the same numbers (turned in the complex plane for the complex
    kind) as an explicit array"""
    if which == "lin":
        return lk.diag_linop_gpu(n_local=n, row0=0, d0=1.0, dstep=1.0 / n, ctx=c)
    g = np.arange(n) / n
    d = (1.0 + g) * (np.exp(1j * g) if np.dtype(dtype).kind == "c" else 1.0)
    return lk.diag_linop_gpu(d.astype(dtype), c)


def _factorise(c, which, n, m, dtype, transpose, fuse, seed=7):
    c.set_tuning("fuse_rowop", fuse)
    X = lk.krylov_basis_gpu(n, m + 1, dtype, c)
    X[0].rand(True, seed=seed)
    H = np.zeros((m + 1, m), dtype=dtype, order="F")
    c.profile_reset()
    c.profile_enable(True)
    info = lk.arnoldi(_operator(c, which, n, dtype), X, H, transpose=transpose)
    c.sync()
    c.profile_enable(False)
    launches = c.profile_get("matvec")[0]
    return info, H, X.download(), launches


# (id, n, m, tuning, steps that still launch the operator kernel with fuse_rowop = 1: f(m, complex kind))
SHAPES = [
    # 16 (real) / 8 and 16 (complex) columns per wave; n odd, last tile ragged
    ("narrow", 250_003, 40, dict(resident=0), lambda m, cplx: 0),
    # sweep 1 as an all-columns-per-tile sweep instead of one column at a time
    ("narrow_dot_tile", 100_001, 20, dict(resident=0, dot_colwise=0), lambda m, cplx: 0),
    # beyond 128 columns: 32-column register tiles (real); the complex kind keeps the operator kernel there
    ("tiles32", 60_001, 140, dict(resident=0), lambda m, cplx: m - 128 if cplx else 0),
    # beyond 256 columns: the 64 lanes split over two column groups, sweep 3 with both groups per wave
    ("lane_split", 20_001, 262, dict(resident=0), lambda m, cplx: m - 128 if cplx else 0),
    # the 16-column lane split (two and four groups) for 129..512 columns
    ("lane_split16", 12_001, 300, dict(resident=0, wide_regs=0), lambda m, cplx: m - 128 if cplx else 0),
    # a panel that crosses the single-launch limit half way: cache-resident steps first (operator kernel), three sweeps after
    ("crossover", 2_000_001, 24, dict(resident=1), None),
    # single launch throughout: every step launches the operator
    ("resident", 30_001, 12, dict(resident=1), lambda m, cplx: m),
]
CASES = [("lin", np.float64, False), ("d", np.float64, False), ("d", np.complex128, False), ("d", np.complex128, True)]


@pytest.mark.parametrize("which,dtype,transpose", CASES, ids=["linspace_f64", "d_f64", "d_c128", "d_c128_adjoint"])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_fused_operator_is_bit_identical_and_launches_no_operator_kernel(fresh, shape, which, dtype, transpose):
    name, n, m, tuning, unfused_steps = shape
    cplx = np.dtype(dtype).kind == "c"
    if name in ("lane_split", "lane_split16") and (cplx or which == "d"):
        m = 140                  # (the wide shapes of the complex kind are not fused; the explicit real d: one wide shape is enough)
    c = fresh(**tuning)
    out = {}
    for fuse in (0, 1):
        info, H, X, launches = _factorise(c, which, n, m, dtype, transpose, fuse)
        assert info == 0
        print(f"{name} {which} {np.dtype(dtype)} adjoint={transpose} fuse_rowop={fuse}: {launches} operator launches in {m} steps")
        out[fuse] = (H.tobytes(), X.tobytes(), launches)
    assert out[0][0] == out[1][0], "H differs between fuse_rowop = 0 and 1"
    assert out[0][1] == out[1][1], "the basis differs between fuse_rowop = 0 and 1"
    assert out[0][2] == m, f"materialised schedule: {out[0][2]} operator launches for {m} steps"
    if unfused_steps is None:
        # the single launch takes the panel while (k + 1) columns fit resident_max_mb (320 MB): those steps launch the operator
        col_mb = n * (16 if cplx else 8) / (1024.0 * 1024.0)
        expect = sum(1 for k in range(1, m + 1) if col_mb * (k + 1) <= 320.0)
        assert 0 < expect < m, "the case must cross the single-launch limit"
    else:
        expect = unfused_steps(m, cplx)
    assert out[1][2] == expect, f"fused schedule: {out[1][2]} operator launches, expected {expect}"


@pytest.mark.parametrize("dtype", [np.float64, np.complex128], ids=["f64", "c128"])
def test_fused_operator_with_a_breakdown_leaves_the_columns_beyond_it(fresh, dtype):
    """the operator with 6 distinct eigenvalues (test_gpu_pipelines.py): invariant subspace after 6 steps.  Column 6 holds what the stopped step
    left there, the marker columns beyond it survive, and all of it equals the materialised schedule's bytes."""
    c = fresh(resident=0)
    n, m = 250_003, 40
    d6 = (1.0 + (np.arange(n) % 6)).astype(dtype)
    marker = seeded(n, dtype, 123)
    res = {}
    for fuse in (0, 1):
        c.set_tuning("fuse_rowop", fuse)
        X = lk.krylov_basis_gpu(n, m + 1, dtype, c)
        X[0].rand(True, seed=9)
        for j in range(7, m + 1):
            X.upload(marker.reshape(-1, 1), j)
        H = np.zeros((m + 1, m), dtype=dtype, order="F")
        info = lk.arnoldi(lk.diag_linop_gpu(d6, c), X, H, tol=1e-10)
        assert info == 6
        Xh = X.download()
        for j in range(7, m + 1):
            assert np.array_equal(Xh[:, j], marker), f"column {j} beyond the breakdown was touched (fuse_rowop = {fuse})"
        res[fuse] = (H.tobytes(), Xh.tobytes())
    assert res[0] == res[1]


@pytest.mark.parametrize("which,dtype", [("lin", np.float64), ("d", np.float64), ("d", np.complex128)], ids=["linspace_f64", "d_f64", "d_c128"])
def test_fused_operator_with_a_nan_in_x0(fresh, which, dtype):
    """a NaN in the starting vector: the first step reports it, column 1 holds the same bytes either way, the columns beyond stay untouched"""
    c = fresh(resident=0)
    n, m = 100_003, 10
    x0 = seeded(n, dtype, 31)
    x0 /= np.linalg.norm(x0)
    x0[n // 3] = np.nan
    marker = seeded(n, dtype, 124)
    res = {}
    for fuse in (0, 1):
        c.set_tuning("fuse_rowop", fuse)
        X = lk.krylov_basis_gpu(n, m + 1, dtype, c)
        X.upload(x0.reshape(-1, 1), 0)
        for j in range(1, m + 1):
            X.upload(marker.reshape(-1, 1), j)
        H = np.zeros((m + 1, m), dtype=dtype, order="F")
        with pytest.raises(_capi.LightKrylovHipError, match=r"\[-5\] \|beta\| = NaN detected"):
            lk.arnoldi(_operator(c, which, n, dtype), X, H)
        Xh = X.download()
        for j in range(2, m + 1):
            assert np.array_equal(Xh[:, j], marker), f"column {j} behind the NaN step was touched (fuse_rowop = {fuse})"
        res[fuse] = (H.tobytes(), Xh.tobytes())
    assert res[0] == res[1]


def test_fused_operator_restarted_range_is_bit_identical(fresh):
    """a factorisation continued from kstart > 1 runs the same fused steps: same bytes as one call, fused or not"""
    c = fresh(resident=0)
    n, m, dtype = 150_001, 24, np.float64
    _, H1, X1, _ = _factorise(c, "lin", n, m, dtype, False, 0)
    c.set_tuning("fuse_rowop", 1)
    X = lk.krylov_basis_gpu(n, m + 1, dtype, c)
    X[0].rand(True, seed=7)
    H = np.zeros((m + 1, m), dtype=dtype, order="F")
    A = _operator(c, "lin", n, dtype)
    assert lk.arnoldi(A, X, H, kend=9) == 0
    assert lk.arnoldi(A, X, H, kstart=10) == 0
    assert H.tobytes() == H1.tobytes() and X.download().tobytes() == X1.tobytes()


@pytest.mark.parametrize("which,dtype", [("lin", np.float64), ("d", np.complex128)], ids=["linspace_f64", "d_c128"])
def test_fused_operator_against_the_oracle(fresh, which, dtype):
    c = fresh(resident=0)
    n, m = 200_003, 16
    c.set_tuning("fuse_rowop", 1)
    x0 = seeded(n, dtype, 7)
    x0 /= np.linalg.norm(x0)
    X = lk.krylov_basis_gpu(n, m + 1, dtype, c)
    X.upload(x0.reshape(-1, 1), 0)
    H = np.zeros((m + 1, m), dtype=dtype, order="F")
    c.profile_reset()
    c.profile_enable(True)
    assert lk.arnoldi(_operator(c, which, n, dtype), X, H) == 0
    c.sync()
    c.profile_enable(False)
    assert c.profile_get("matvec")[0] == 0
    g = np.arange(n) / n
    d = ((1.0 + g) * (np.exp(1j * g) if np.dtype(dtype).kind == "c" else 1.0)).astype(dtype)
    Xo = np.zeros((n, m + 1), dtype=dtype, order="F")
    Xo[:, 0] = x0
    Ho = np.zeros((m + 1, m), dtype=dtype, order="F")
    assert ora.arnoldi(ora.DiagOp(d), Xo, Ho) == 0
    assert_columns_close(H, Ho, f"fused row operator Arnoldi vs oracle ({which}, {np.dtype(dtype)})")
