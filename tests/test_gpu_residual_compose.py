"""lk_linop_residual (the residual branch of k_axpby in csrc/lk_kernels.hip.h: r = b - op(A) x and ||r|| in one pass behind the product, gmres.fypp:134-142)
and lk_linop_compose_create (the product of two engine operators as one operator), each against the existing entries it replaces.

The residual vector must be what lk_linop_apply + sub + chsgn leave BIT FOR BIT -- on a caller-owned panel with NaN in the padding rows,
which must still be NaN afterwards --, its norm the correctly rounded sum of the downloaded squares (math.fsum) within 1e-12.  Sizes: the
16-byte lane edges (1, 2, 3), the block edges (255..257), several blocks (8191..8193) and one size just beyond a single pass of the grid at
"blas1_grid_mult" = 1, computed from the device's CU count.  The composed operator must equal the two applications through a temporary
bit for bit, for every transA / transB setting and both directions, and lk_arnoldi on it must match the oracle on the product."""
import ctypes as C
import math

import numpy as np
import pytest

import lightkrylov_amd as lk
from lightkrylov_amd import _capi
from oracle import oracle as ora
from tests._gpu_helpers import KINDS, CallerPanel, device_num_cu, is_cplx, seeded
from tests._tol import RTOL, _report, assert_columns_close

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 255, 256, 257, 8191, 8192, 8193)


@pytest.fixture(scope="module")
def kctx():
    c = lk.Context(device=0)
    yield c
    c.set_tuning("blas1_grid_mult", 2)
    c.close()


def _beyond_one_pass(c, dtype):
    """n whose 16-byte lanes are a few more than the num_cu * 256 threads of the grid at "blas1_grid_mult" = 1: the second trip of the loop"""
    S = device_num_cu(c) * 256
    return S + 5 if is_cplx(dtype) else 2 * (S + 5) + 1


def _diag(n, dtype, seed):
    d = 1.0 + 0.5 * seeded(n, dtype, seed)
    return d


def _dense(n, dtype, seed):
    A = np.empty((n, n), dtype=dtype, order="F")
    for j in range(n):
        ora.fill_counter(A[:, j], seed + j)
    return A


def _residual(op, trans, x, b, r, want_norm=True):
    out = C.c_double(-1.0)
    rc = op._lib.lk_linop_residual(op._h, trans, x.basis._h, x.col, b.basis._h, b.col, r.basis._h, r.col,
                                   C.byref(out) if want_norm else None)
    return rc, out.value


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _check_one(c, op, trans, n, dtype, label):
    xh, bh = seeded(n, dtype, 31), seeded(n, dtype, 32)
    P = CallerPanel(c, dtype, n, 3, "nan_pad")                       # columns: x | b | r, ld > n, NaN in the padding rows
    P.set(np.stack([xh, bh, np.full(n, np.nan, dtype=dtype)], axis=1))
    x, b, r = P.B[0], P.B[1], P.B[2]
    # the three-call sequence through the existing entries, on an engine-owned vector
    ref = lk.dense_vector_gpu(n, dtype, c)
    (op.rmatvec if trans else op.matvec)(x, ref)
    ref.sub(b)
    ref.chsgn()
    want = ref.to_array()
    rc, nrm = _residual(op, trans, x, b, r)
    assert rc == 0, label
    got = P.get(label)                                               # asserts that the padding is still the NaN it was
    assert np.array_equal(_bits(got[:, 2]), _bits(want)), f"{label}: r differs from apply + sub + chsgn"
    assert np.array_equal(_bits(got[:, 0]), _bits(xh)) and np.array_equal(_bits(got[:, 1]), _bits(bh)), f"{label}: x or b changed"
    exact = math.sqrt(math.fsum(float(v) ** 2 for v in np.ascontiguousarray(got[:, 2]).view(np.float64)))
    err = abs(nrm - exact) / exact
    _report(label + " [norm]", err, RTOL)
    assert err <= RTOL, f"{label}: norm off by {err:.2e}"
    # nrm = NULL: no synchronisation, the same vector after lk_sync
    r.zero()
    rc, _ = _residual(op, trans, x, b, r, want_norm=False)
    assert rc == 0, label
    c.sync()
    assert np.array_equal(_bits(P.get(label + " (no norm)")[:, 2]), _bits(want)), f"{label}: r differs when the norm is not asked for"


@pytest.mark.parametrize("trans", [0, 1], ids=["N", "H"])
@pytest.mark.parametrize("dtype", KINDS)
def test_residual_on_a_diagonal_operator_at_the_loop_edges(kctx, dtype, trans):
    kctx.set_tuning("blas1_grid_mult", 1)
    try:
        for n in SIZES + (_beyond_one_pass(kctx, dtype),):
            op = lk.diag_linop_gpu(_diag(n, dtype, 7), kctx)
            _check_one(kctx, op, trans, n, dtype, f"residual diag n={n} {np.dtype(dtype).name} trans={trans}")
    finally:
        kctx.set_tuning("blas1_grid_mult", 2)


@pytest.mark.parametrize("dtype", KINDS)
def test_residual_on_a_dense_operator(kctx, dtype):
    """The residual pass never sees the operator -- it starts from op(A) x as the product left it in r --, so its loop edges are the
    diagonal test's; here the product in front of it is the dense one, at the lane edges, either side of one block of 16-byte lanes and
    across the blocks of the dense product (512 real / 256 complex rows each)."""
    for n in (1, 3, 255, 256, 257, 600):
        op = lk.dense_linop_gpu(_dense(n, dtype, 50), kctx)
        for trans in (0, 1):
            _check_one(kctx, op, trans, n, dtype, f"residual dense n={n} {np.dtype(dtype).name} trans={trans}")


def test_residual_python_wrapper_and_default_grid(kctx):
    n = 8193
    op = lk.diag_linop_gpu(_diag(n, np.float64, 7), kctx)
    xh, bh = seeded(n, np.float64, 31), seeded(n, np.float64, 32)
    x, b = lk.dense_vector_gpu.from_array(xh, kctx), lk.dense_vector_gpu.from_array(bh, kctx)
    r = lk.dense_vector_gpu(n, np.float64, kctx)
    nrm = lk.residual(op, x, b, r)
    want = -(_diag(n, np.float64, 7) * xh - bh)
    assert np.array_equal(r.to_array(), want) and op.matvec_counter == 1
    assert abs(nrm - math.sqrt(math.fsum(v * v for v in want))) <= RTOL * nrm


@pytest.mark.parametrize("dtype", KINDS)
def test_residual_refuses_aliases_and_passes_nan_on(kctx, dtype):
    n = 257
    op = lk.diag_linop_gpu(_diag(n, dtype, 7), kctx)
    X = lk.krylov_basis_gpu(n, 3, dtype, kctx)
    X.upload(np.stack([seeded(n, dtype, 1), seeded(n, dtype, 2), seeded(n, dtype, 3)], axis=1))
    before = X.download()
    for r in (X[0], X[1]):                                           # r aliased with x, with b
        rc, _ = _residual(op, 0, X[0], X[1], r)
        assert rc == -1
    assert np.array_equal(_bits(X.download()), _bits(before))
    short = lk.krylov_basis_gpu(n - 1, 1, dtype, kctx)
    assert _residual(op, 0, X[0], X[1], short[0])[0] == -1           # shapes
    bh = seeded(n, dtype, 2)
    bh[n // 2] = np.nan
    X.upload(bh.reshape(-1, 1), 1)
    rc, nrm = _residual(op, 0, X[0], X[1], X[2])
    assert rc == 0 and math.isnan(nrm)


# ---- the composed operator ---------------------------------------------------------------------------------------------------------------

def _csr(n, dtype, seed):
    """a banded matrix in CSR: three diagonals, bandwidth 5"""
    import scipy.sparse as sp
    diags = [seeded(n, dtype, seed + k)[:n - abs(o)] for k, o in enumerate((-5, 0, 2))]
    return sp.diags(diags, (-5, 0, 2), format="csr", dtype=dtype)


def _factor(kind, n, dtype, seed, c):
    if kind == "dense":
        return lk.dense_linop_gpu(_dense(n, dtype, seed), c)
    if kind == "csr":
        return lk.csr_linop_gpu(_csr(n, dtype, seed), c)
    return lk.diag_linop_gpu(_diag(n, dtype, seed), c)


@pytest.mark.parametrize("pair", [("dense", "diag"), ("csr", "diag"), ("diag", "dense")], ids=lambda p: "-".join(p))
@pytest.mark.parametrize("dtype", KINDS)
def test_composed_operator_equals_the_two_applications(kctx, dtype, pair):
    n = 257
    A, B = _factor(pair[0], n, dtype, 100, kctx), _factor(pair[1], n, dtype, 500, kctx)
    x = lk.dense_vector_gpu.from_array(seeded(n, dtype, 9), kctx)
    for ta in (False, True):
        for tb in (False, True):
            AB = lk.compose_linop_gpu(A, B, transA=ta, transB=tb)
            for adjoint in (False, True):
                y, t, want = (lk.dense_vector_gpu(n, dtype, kctx) for _ in range(3))
                (AB.apply_rmatvec if adjoint else AB.apply_matvec)(x, y)
                # op_a(A) op_b(B) x, or its adjoint op_b(B)^H op_a(A)^H x, through a temporary
                first, second = ((A, not ta), (B, not tb)) if adjoint else ((B, tb), (A, ta))
                (first[0].rmatvec if first[1] else first[0].matvec)(x, t)
                (second[0].rmatvec if second[1] else second[0].matvec)(t, want)
                assert np.array_equal(_bits(y.to_array()), _bits(want.to_array())), (pair, ta, tb, adjoint)
            AB.close()


def test_compose_refuses_mismatched_factors(kctx):
    lib = _capi.load()
    A = lk.diag_linop_gpu(_diag(16, np.float64, 1), kctx)
    other = lk.Context(device=0)
    try:
        for B in (lk.diag_linop_gpu(_diag(17, np.float64, 1), kctx), lk.diag_linop_gpu(_diag(16, np.complex128, 1), kctx),
                  lk.diag_linop_gpu(_diag(16, np.float64, 1), other)):
            h = C.c_void_p()
            assert lib.lk_linop_compose_create(A._h, 0, B._h, 0, C.byref(h)) == -1 and not h.value
            with pytest.raises(_capi.LightKrylovHipError, match=r"\[-1\]"):
                lk.compose_linop_gpu(A, B)
            B.close()
    finally:
        other.close()


@pytest.mark.parametrize("dtype", KINDS)
def test_arnoldi_on_a_composed_operator_matches_the_oracle(kctx, dtype):
    n, m = 257, 8
    Ah, d = _dense(n, dtype, 100), _diag(n, dtype, 500)
    AB = lk.compose_linop_gpu(lk.dense_linop_gpu(Ah, kctx), lk.diag_linop_gpu(d, kctx))
    x0 = seeded(n, dtype, 3)
    x0 /= np.linalg.norm(x0)
    X = lk.krylov_basis_gpu(n, m + 1, dtype, kctx)
    X.upload(x0.reshape(-1, 1), 0)
    H = np.zeros((m + 1, m), dtype=dtype, order="F")
    info = lk.arnoldi(AB, X, H)
    Xo = np.zeros((n, m + 1), dtype=dtype, order="F")
    Xo[:, 0] = x0
    Ho = np.zeros((m + 1, m), dtype=dtype, order="F")
    info_o = ora.arnoldi(ora.PyOp(lambda v: Ah @ (d * v), dtype), Xo, Ho)
    assert info == info_o == 0
    assert_columns_close(H, Ho, f"arnoldi on dense * diag {np.dtype(dtype).name}")
