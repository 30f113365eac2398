"""lk_qr_pivot / qr(..., perm=): qr_with_pivoting (src/Krylov/qr.fypp:32-107) on columns of a device panel, and the in-place column
swap inside k_copy that it runs on.

The yardstick is the NumPy restatement of the reference's control flow in tests/_pivot_ref.py (the CPU oracle has no pivoting qr).
Column i of every input is scaled by 2^-sigma(i) for a fixed shuffle sigma, so the pivot order is decided by factors of four in
|Rii| and rounding cannot change it: the restatement's pivot gaps are asserted to exceed 1e-6 in every case, none is skipped.
Bounds: perm and info equal; R normwise per column at 1e-12 (tests/_tol.py); A(:, perm) = Q R and Q^H Q = I at 1e-12, the
bounds of tests/test_gpu_block_arnoldi.py."""
import ctypes as C

import numpy as np
import pytest

import lightkrylov_amd as lk
from lightkrylov_amd import _capi
from tests import _pivot_ref as ref
from tests._gpu_helpers import CallerPanel, basis, device_num_cu, fit, seeded
from tests._tol import assert_columns_close

pytestmark = pytest.mark.gpu
KINDS = [np.float64, np.complex128]
_DP = C.POINTER(C.c_double)
_IP = C.POINTER(C.c_int)


def _raw(B, j0, p, R, perm, tol=ref.ATOL_DP):
    info = C.c_int(-99)
    rc = B._lib.lk_qr_pivot(B._h, j0, p, R.ctypes.data_as(_DP), R.shape[0], perm.ctypes.data_as(_IP), float(tol), C.byref(info))
    return rc, info.value


def _graded(n, p, dtype, seed):
    """p columns of counter numbers, column i scaled by 2^-sigma(i)"""
    sigma = np.random.default_rng(seed).permutation(p)
    return np.asfortranarray(basis(n, p, dtype, 100 + seed) * 2.0 ** (-sigma.astype(float)))


def _reference(A, j0=0, tol=ref.ATOL_DP):
    Q = A.copy(order="F")
    p = A.shape[1]
    R, perm, gaps = np.zeros((p, p), dtype=A.dtype, order="F"), np.zeros(p, dtype=int), []
    info = ref.qr_with_pivoting(Q, R, perm, tol, ref.engine_stream(j0), gaps)
    return Q, R, perm, info, gaps


def _engine_source():
    import os
    return open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lightkrylov_amd", "csrc", "lk_engine.hip")).read()


def _grid_stride(ctx):
    """16-byte lanes one grid of the BLAS-1 kernels covers: blas1_grid caps the grid at num_cu x "blas1_grid_mult" blocks of 256
    threads.  The engine has no accessor for either rule, so the default multiplier is READ from the engine's source: a change of it
    moves these sizes along instead of leaving them beside the boundary."""
    import re
    mult = int(re.search(r"int blas1_grid_mult = (\d+);", _engine_source()).group(1))
    return device_num_cu(ctx) * mult * 256


def _nt_bytes():
    """bytes of a column from which blas1_nt turns the non-temporal path on, read from the engine's source"""
    import re
    m = re.search(r"inline int blas1_nt\(lk_basis_t B\) \{ return \(int64_t\)B->n \* B->ed\(\) \* 8 >= \(int64_t\)(\d+) << (\d+); \}", _engine_source())
    return int(m.group(1)) << int(m.group(2))


# ---- the swap inside k_copy ------------------------------------------------------------------------------------------------
def _swap_sizes(ctx, dtype):
    S = _grid_stride(ctx)                              # lanes of 16 bytes: two reals or one complex
    per = 1 if np.dtype(dtype).kind == "c" else 2
    return [1, 2, 3, 255 * 2 + 1, S * per - 1, S * per + 1, 2 * S * per + 3]


@pytest.mark.parametrize("dtype", KINDS, ids=["rdp", "cdp"])
def test_swap_moves_every_element_and_nothing_else(ctx, dtype):
    """p = 2 with the larger column second: the factorisation opens with the swap.  The columns have disjoint supports (even / odd
    rows) and entries +-2^e with norms that are powers of two, so every later operation is exact -- h = 0, the scalings are by powers
    of two -- and BOTH columns can be compared bit for bit with the exchanged, scaled inputs.  A third column and the padding rows of
    the caller-owned panel (ld > n) keep their bits.  Sizes: the tails (1, 2, 3), one block + 1, one grid stride -1 / +1, two + 3."""
    for n in _swap_sizes(ctx, dtype):
        n = fit(n, dtype, "nan_pad")
        rng = np.random.default_rng(n)
        x = np.zeros((n, 3), dtype=dtype, order="F")
        ev, od = np.arange(0, n, 2), np.arange(1, n, 2)
        # 4^a entries of magnitude 2^e on the even rows (column 0), on the odd rows (column 1, larger): norms 2^(a + e)
        def dyadic(rows, e):
            cnt = 1 if len(rows) else 0
            while cnt and cnt * 4 <= len(rows):
                cnt *= 4
            v = np.zeros(n, dtype=dtype)
            v[rows[:cnt]] = rng.choice([-1.0, 1.0], cnt) * 2.0 ** e
            return v
        x[:, 0], x[:, 1] = dyadic(ev, -3), dyadic(od, 2)
        x[:, 2] = seeded(n, dtype, 5)
        if n == 1:                                     # no odd row: one entry each, the second one larger
            x[0, 0], x[0, 1] = 1.0, 2.0
        P = CallerPanel(ctx, dtype, n, 3, "nan_pad")
        P.set(x)
        R, perm = np.zeros((2, 2), dtype=dtype, order="F"), np.zeros(2, dtype=np.intc)
        rc, info = _raw(P.B, 0, 2, R, perm)
        got = P.get(f"swap n={n}")                     # asserts the padding rows and everything around the panel
        assert rc == 0 and list(perm) == [2, 1], (n, rc, list(perm))
        n1 = np.linalg.norm(x[:, 1])
        assert R[0, 0] == n1
        assert np.array_equal(got[:, 0].view(np.float64), (x[:, 1] / n1).view(np.float64)), n
        assert np.array_equal(got[:, 2].view(np.float64), x[:, 2].view(np.float64)), n
        if n > 1:
            n0 = np.linalg.norm(x[:, 0])
            assert info == 0 and R[0, 1] == 0 and R[1, 1] == n0, (n, info, R)
            assert np.array_equal(got[:, 1].view(np.float64), (x[:, 0] / n0).view(np.float64)), n
        else:
            assert info == 2 and R[0, 1] == 1.0       # the second column is (exactly) dependent: re-drawn


@pytest.mark.parametrize("dtype", KINDS, ids=["rdp", "cdp"])
def test_swap_on_random_columns_against_the_restatement(ctx, dtype):
    """the same sizes with full random columns (every lane carries data): Q and R as the restatement's"""
    for n in _swap_sizes(ctx, dtype)[2:]:
        A = basis(n, 2, dtype, 40 + n % 89)
        A[:, 0] *= 0.25
        Qr, Rr, permr, infor, gaps = _reference(A)
        assert list(permr) == [2, 1] and min(gaps) > 1e-6
        X = lk.krylov_basis_gpu(n, 2, dtype, ctx)
        X.upload(A)
        R, perm = np.zeros((2, 2), dtype=dtype, order="F"), np.zeros(2, dtype=np.intc)
        rc, info = _raw(X, 0, 2, R, perm)
        assert rc == 0 and info == infor and list(perm) == [2, 1]
        assert_columns_close(R, Rr, f"qr_pivot swap n={n}")
        Q = X.download()
        assert np.abs(Q - Qr).max() <= 1e-12 * np.abs(Qr).max()
        X.close()


def test_swap_on_the_non_temporal_path(ctx):
    """the smallest odd n whose column reaches blas1_nt's threshold (32 MB: 2^22 reals), odd for the tail; real kind"""
    n = _nt_bytes() // 8 + 1
    assert n % 2 == 1
    A = basis(n, 2, np.float64, 77)
    A[:, 0] *= 0.25
    X = lk.krylov_basis_gpu(n, 3, np.float64, ctx)
    X.upload(A)
    X[2].zero()
    lk.copy(X[2], X[1])                                 # the copy path at the same size
    assert np.array_equal(X.download(2, 1)[:, 0], A[:, 1])
    R, perm = np.zeros((2, 2), order="F"), np.zeros(2, dtype=np.intc)
    rc, info = _raw(X, 0, 2, R, perm)
    assert rc == 0 and info == 0 and list(perm) == [2, 1]
    Q = X.download(0, 2)
    n1 = np.linalg.norm(A[:, 1])
    assert abs(R[0, 0] - n1) <= 1e-12 * n1
    assert np.abs(Q[:, 0] - A[:, 1] / n1).max() <= 4 * 2.0 ** -53 * np.abs(A[:, 1] / n1).max()     # the swapped column, scaled once
    assert np.abs(A[:, [1, 0]] - Q @ R).max() <= 1e-12
    X.close()


@pytest.mark.parametrize("dtype", KINDS, ids=["rdp", "cdp"])
def test_plain_copy_is_unchanged(ctx, dtype):
    """lk_vec_copy (swap = 0) at the sizes of the swap test: a bit copy, the source and a bystander column untouched"""
    for n in _swap_sizes(ctx, dtype):
        A = basis(n, 3, dtype, 7)
        X = lk.krylov_basis_gpu(n, 3, dtype, ctx)
        X.upload(A)
        lk.copy(X[1], X[0])
        got = X.download()
        assert np.array_equal(got, A[:, [0, 0, 2]]), n
        X.close()


# ---- against the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", KINDS, ids=["rdp", "cdp"])
@pytest.mark.parametrize("n", [37, 4099])
@pytest.mark.parametrize("p", [1, 2, 4, 5, 8, 20])
def test_against_the_restatement(ctx, dtype, n, p):
    A = _graded(n, p, dtype, p + n % 13)
    Qr, Rr, permr, infor, gaps = _reference(A)
    assert infor == 0 and min(gaps) > 1e-6, (infor, min(gaps))
    X = lk.krylov_basis_gpu(n, p, dtype, ctx)
    X.upload(A)
    R, perm = np.full((p, p), 7.0, dtype=dtype, order="F"), np.zeros(p, dtype=np.intc)
    info = lk.qr(X, R, perm=perm)
    assert info == infor and np.array_equal(perm, permr), (info, list(perm), list(permr))
    assert_columns_close(R, Rr, f"qr_pivot p={p} n={n} {np.dtype(dtype).name}")
    Q = X.download()
    assert np.abs(A[:, perm - 1] - Q @ R).max() <= 1e-12 * np.abs(A).max()
    assert np.abs(Q.conj().T @ Q - np.eye(p)).max() <= 1e-12
    X.close()


@pytest.mark.parametrize("dtype", KINDS, ids=["rdp", "cdp"])
def test_inside_a_wider_panel(ctx, dtype):
    """j0 > 0, ldr > p: the columns either side and the rows of R below p keep their contents"""
    n, p, j0, ncols = 301, 5, 3, 10
    W = basis(n, ncols, dtype, 3)
    A = _graded(n, p, dtype, 9)
    W[:, j0:j0 + p] = A
    Qr, Rr, permr, infor, gaps = _reference(A, j0)
    assert min(gaps) > 1e-6
    X = lk.krylov_basis_gpu(n, ncols, dtype, ctx)
    X.upload(W)
    R, perm = np.full((p + 2, p), 7.0, dtype=dtype, order="F"), np.zeros(p, dtype=np.intc)
    rc, info = _raw(X, j0, p, R, perm)
    assert rc == 0 and info == infor and np.array_equal(perm, permr)
    assert np.all(R[p:, :] == 7.0)
    assert_columns_close(R[:p, :], Rr, "qr_pivot j0=3")
    got = X.download()
    assert np.array_equal(got[:, :j0], W[:, :j0]) and np.array_equal(got[:, j0 + p:], W[:, j0 + p:])
    assert np.abs(got[:, j0:j0 + p] - Qr).max() <= 1e-12
    X.close()


# ---- rank deficiency ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", KINDS, ids=["rdp", "cdp"])
def test_reference_rank_deficiency(ctx, dtype):
    """test/TestKrylov.fypp:101-174: 5 zero columns of 20, info = 16; the re-drawn columns entry by entry as the restatement's on the
    engine's streams"""
    n, p, nzero = 100, 20, 5
    A = _graded(n, p, dtype, 17)
    A[:, [2, 7, 11, 12, 19]] = 0
    Qr, Rr, permr, infor, gaps = _reference(A)
    assert infor == p - nzero + 1 and min(gaps) > 1e-6
    X = lk.krylov_basis_gpu(n, p, dtype, ctx)
    X.upload(A)
    R, perm = np.zeros((p, p), dtype=dtype, order="F"), np.zeros(p, dtype=np.intc)
    info = lk.qr(X, R, perm=perm, tol=lk.atol_dp)
    assert info == 16 and np.array_equal(perm, permr)
    assert_columns_close(R, Rr, "qr_pivot rank deficient")
    Q = X.download()
    assert np.abs(Q - Qr).max() <= 1e-12
    assert np.abs(A[:, perm - 1] - Q @ R).max() < lk.rtol_dp
    assert np.linalg.norm(np.abs(Q.conj().T @ Q - np.eye(p)), 2) < lk.rtol_dp
    X.close()


def _check_against(ctx, A, Qr, Rr, permr, infor, label, tol=ref.ATOL_DP):
    n, p = A.shape
    X = lk.krylov_basis_gpu(n, p, A.dtype, ctx)
    X.upload(A)
    R, perm = np.zeros((p, p), dtype=A.dtype, order="F"), np.zeros(p, dtype=np.intc)
    info = lk.qr(X, R, tol=tol, perm=perm)
    assert info == infor and np.array_equal(perm, permr), (info, infor, list(perm), list(permr))
    assert_columns_close(R, Rr, label)
    Q = X.download()
    assert np.abs(Q - Qr).max() <= 1e-12
    assert np.abs(Q.conj().T @ Q - np.eye(p)).max() <= 1e-12
    X.close()


def test_exactly_repeated_column(ctx):
    """real kind, two equal columns: once the first is factored the other is left at rounding level -- |Rii| about eps |a|^2 and the
    column about eps |a|, both far below atol_dp at this scaling (|a| about 2^-9) --, the pivot search takes it last and re-draws it:
    info = p, R(p, p) = 0, through the pivot test (:55).  (In the real kind the branch at :79-85 -- |Rii| above the tolerance, the norm
    below -- needs an |Rii| that is WRONG by more than the tolerance: for an exact duplicate the downdate cancels exactly, at any scaling
    and tolerance, and for a near duplicate the sign and size of what is left are rounding, different in every implementation.  The
    complex test below reaches that branch by construction; its host code does not depend on the kind.)"""
    n, p = 203, 4
    A = _graded(n, p, np.float64, 23) * 2.0 ** -12
    A[:, 3] = A[:, 0]
    Qr, Rr, permr, infor, _ = _reference(A)
    assert infor == p and Rr[p - 1, p - 1] == 0
    br = []
    ref.qr_with_pivoting(A.copy(order="F"), np.zeros((p, p), order="F"), np.zeros(p, dtype=int), branches=br)
    assert [b[:2] for b in br] == [(":55", p)], br
    _check_against(ctx, A, Qr, Rr, permr, infor, "qr_pivot repeated column")


def test_complex_downdate_is_the_square_not_the_modulus(ctx):
    """Rii(i) -= R(j, i)**2 (:102) is the complex SQUARE in the reference.  Column 2 = (i / 2) column 1: after the first step
    R(1, 2) = (i / 2) |a|, its square is -|a|^2 / 4, and Rii(2) GROWS to |a|^2 / 2 although the column is annihilated (with |R|^2 it
    would drop to zero and the pivot search would pass it by).  So step 2 takes that column, finds its norm below the tolerance (about
    eps |a| = 2e-17 here) and goes through :79-85: info = 2, R(2, 2) = 0, a re-draw, and the factorisation continues.  With the modulus
    the order of the pivots would be 1, 3, 4, 2 and info = 4."""
    n, p = 203, 4
    A = np.asfortranarray(basis(n, p, np.complex128, 61) * 2.0 ** -np.array([6.0, 0.0, 8.0, 9.0]))
    A[:, 1] = 0.5j * A[:, 0]
    Qr, Rr, permr, infor, _ = _reference(A)
    assert infor == 2 and list(permr) == [1, 2, 3, 4] and Rr[1, 1] == 0
    assert abs(Rr[0, 1] ** 2 + np.linalg.norm(A[:, 0]) ** 2 / 4) <= 1e-12 * np.linalg.norm(A[:, 0]) ** 2
    br = []
    ref.qr_with_pivoting(A.copy(order="F"), np.zeros((p, p), dtype=A.dtype, order="F"), np.zeros(p, dtype=int), branches=br)
    assert [b[:2] for b in br] == [(":79", 2)] and br[0][2] >= 100 * ref.ATOL_DP and br[0][3] <= ref.ATOL_DP / 10, br
    _check_against(ctx, A, Qr, Rr, permr, infor, "qr_pivot complex square")


# ---- failure handling --------------------------------------------------------------------------------------------------------
def test_nan_input_and_argument_errors(ctx):
    n, p = 65, 3
    A = _graded(n, p, np.float64, 1)
    X = lk.krylov_basis_gpu(n, p, np.float64, ctx)
    bad = A.copy(order="F")
    bad[5, 1] = np.nan
    X.upload(bad)
    R, perm = np.zeros((p, p), order="F"), np.zeros(p, dtype=np.intc)
    rc, _ = _raw(X, 0, p, R, perm)
    assert rc == -5 and b"NaN" in X._lib.lk_last_error()
    X.upload(A)                                        # the context stays usable
    rc, info = _raw(X, 0, p, R, perm)
    assert rc == 0 and info == 0
    X.upload(A)
    R[...] = 7.0
    perm[...] = -3
    for j0, pp, ldr in [(-1, p, p), (1, p, p), (0, 0, p), (0, p, p - 1), (0, 513, 513)]:
        info = C.c_int(-99)
        rc = X._lib.lk_qr_pivot(X._h, j0, pp, R.ctypes.data_as(_DP), ldr, perm.ctypes.data_as(_IP), 1e-15, C.byref(info))
        assert rc == -1, (j0, pp, ldr)
    info = C.c_int(-99)
    assert X._lib.lk_qr_pivot(X._h, 0, p, None, p, perm.ctypes.data_as(_IP), 1e-15, C.byref(info)) == -1
    assert X._lib.lk_qr_pivot(X._h, 0, p, R.ctypes.data_as(_DP), p, None, 1e-15, C.byref(info)) == -1
    assert X._lib.lk_qr_pivot(None, 0, p, R.ctypes.data_as(_DP), p, perm.ctypes.data_as(_IP), 1e-15, C.byref(info)) == -1
    assert np.all(R == 7.0) and np.all(perm == -3) and info.value == -99
    assert np.array_equal(X.download(), A)
    X.close()


def test_row_sharded_context_is_refused():
    lib = _capi.load()
    c2 = lk.Context(device=0)
    cb = _capi.ALLREDUCE_FN(lambda _u, _p, _n, _s: 0)
    n, p = 64, 3
    A = _graded(n, p, np.float64, 2)
    X = lk.krylov_basis_gpu(n, p, np.float64, c2)
    X.upload(A)
    R, perm = np.zeros((p, p), order="F"), np.zeros(p, dtype=np.intc)
    _capi.check(lib.lk_set_allreduce(c2._h, cb, None, 2, 0))
    try:
        rc, _ = _raw(X, 0, p, R, perm)
        assert rc == -1 and b"row-sharded" in lib.lk_last_error()
        assert np.array_equal(X.download(), A)
    finally:
        _capi.check(lib.lk_set_allreduce(c2._h, _capi.ALLREDUCE_FN(), None, 1, 0))
    assert _raw(X, 0, p, R, perm)[0] == 0
    X.close()
    c2.close()
