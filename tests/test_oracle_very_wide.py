"""The inputs of tests/test_gpu_very_wide_bases.py, checked without a GPU.

Beyond 512 basis columns lk_dgs runs column panels (2 to 4 of 512 on the device up to 2048 columns, panels of 128 with a host round trip
each beyond).  Its tests compare at the bare 1e-12 |y|, so the inputs must make every part of the schedule visible at that level: on an
orthonormal basis the whole second pass is 1e-16 |y|.  For every (n, k, kind, input) the GPU file uses, the reference alone shows here that

  * the second pass has corrections of at least 1e-6 |y| to make (`assert_second_pass_matters`; measured 2e-3 |y| and more), and
  * plain double-precision two-pass Gram-Schmidt lies within 1e-13 |y| of the longdouble evaluation the GPU results are compared with,
    for beta and for y'' -- nothing in these inputs amplifies rounding, so a GPU result outside 1e-12 |y| is wrong.

The same for the blocks of lk_dgs_block's column-by-column route and for the single factorisation steps from a prepared basis, whose
longdouble restatements (tests/_gpu_helpers.py) are tied to the oracle's Arnoldi, Lanczos, Golub-Kahan and block Arnoldi here."""
import numpy as np
import pytest

from oracle import oracle as ora
from tests._gpu_helpers import (KINDS, VERY_WIDE_BLOCK_K, VERY_WIDE_FLAG_K, VERY_WIDE_K, VERY_WIDE_PANEL_K, _long, arnoldi_block_step_longdouble,
                                arnoldi_operator, arnoldi_step_longdouble, assert_second_pass_matters, bidiag_step_longdouble,
                                dgs_longdouble, lanczos_step_longdouble, second_pass_input, skewed_basis, very_wide_n)

REF_AGREE = 1e-13                # double against longdouble: a tenth of the 1e-12 of the GPU tests
ALL_K = tuple(sorted(set(VERY_WIDE_K + VERY_WIDE_FLAG_K + VERY_WIDE_PANEL_K + VERY_WIDE_BLOCK_K)))


def _double_two_pass(y, X):
    Xh = X.conj().T
    h1 = Xh @ y
    y1 = y - X @ h1
    h2 = Xh @ y1
    return h1 + h2, y1 - X @ h2


def _pin(X, Y, labels):
    """the two conditions for every column of Y (one longdouble evaluation for all of them)"""
    h1, h2, _y1, y2 = dgs_longdouble(Y, X)
    beta, yy = _double_two_pass(Y, X)
    for j, label in enumerate(labels):
        ynorm = float(np.linalg.norm(Y[:, j]))
        share = assert_second_pass_matters(h1[:, j], h2[:, j], Y[:, j])
        db, dy = float(np.abs(beta[:, j] - (h1 + h2)[:, j]).max()) / ynorm, float(np.abs(yy[:, j] - y2[:, j]).max()) / ynorm
        print(f"{label}: max|h2| / |y| = {share:.1e}, double - longdouble: beta {db:.1e}, y'' {dy:.1e}")
        assert db <= REF_AGREE and dy <= REF_AGREE, (label, db, dy)


@pytest.mark.parametrize("k", ALL_K)
@pytest.mark.parametrize("dtype", KINDS)
def test_very_wide_inputs_have_a_real_second_pass_and_nothing_amplifies_rounding(dtype, k):
    n = very_wide_n(k)
    kinds = ("skew_rand", "skew_span")
    X = second_pass_input(n, k, dtype, kinds[0])[0]
    Y = np.concatenate([second_pass_input(n, k, dtype, which)[1] for which in kinds], axis=1)
    _pin(X, Y, [f"{np.dtype(dtype).name} n = {n} k = {k} {which}" for which in kinds])


@pytest.mark.parametrize("k", VERY_WIDE_BLOCK_K)
@pytest.mark.parametrize("dtype", KINDS)
def test_block_inputs_beyond_512_columns(dtype, k):
    n = very_wide_n(k)
    for which in ("skew_rand", "skew_span"):
        X, Y = second_pass_input(n, k, dtype, which, 6)              # (a block of 3 columns is the first 3 of these)
        _pin(X, Y, [f"{np.dtype(dtype).name} n = {n} k = {k} {which} column {j}" for j in range(6)])


def _cols_close(got, ref, label):
    ref = np.asarray(ref)
    err = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"{label}: {err:.1e}")
    assert err <= REF_AGREE, (label, err)


@pytest.mark.parametrize("k0", VERY_WIDE_PANEL_K)
@pytest.mark.parametrize("dtype", KINDS)
def test_one_step_of_each_factorisation_from_a_very_wide_skewed_block(dtype, k0):
    """step k0 of ora.arnoldi / lanczos / bidiagonalization / arnoldi_block (p = 2) from k0 skewed columns against the longdouble
    restatement of that step, normwise per column within 1e-13; and the step's vector leaves the second pass work to do"""
    n = very_wide_n(k0)
    name = f"{np.dtype(dtype).name} k0 = {k0}"
    d = arnoldi_operator(n, dtype)
    X0 = skewed_basis(n, k0, dtype, 40 + k0)
    v = d * X0[:, -1]
    h1, h2, _y1, _y2 = dgs_longdouble(v, X0)
    assert_second_pass_matters(h1, h2, v)

    def start(ncols, X0=X0):
        X = np.zeros((n, ncols), dtype=dtype, order="F")
        X[:, :X0.shape[1]] = X0
        return X

    Xo, Ho = start(k0 + 1), np.zeros((k0 + 1, k0), dtype=dtype, order="F")
    assert ora.arnoldi(ora.DiagOp(d), Xo, Ho, kstart=k0, kend=k0) == 0
    hcol, x = arnoldi_step_longdouble(d, X0)
    _cols_close(Ho[:, k0 - 1], hcol, name + " arnoldi H column")
    _cols_close(Xo[:, k0], x, name + " arnoldi vector")

    dh = (1.0 + np.arange(n) / n).astype(dtype)
    Xo, To = start(k0 + 1), np.zeros((k0 + 1, k0), dtype=dtype, order="F")
    assert ora.lanczos(ora.DiagOp(dh), Xo, To, kstart=k0, kend=k0) == 0
    tcol, x = lanczos_step_longdouble(dh, X0)
    _cols_close(To[:, k0 - 1], tcol, name + " lanczos T column")
    _cols_close(Xo[:, k0], x, name + " lanczos vector")

    V0 = skewed_basis(n, k0 - 1, dtype, 900)
    Uo, Vo, Bo = start(k0 + 1), start(k0, V0), np.zeros((k0 + 1, k0), dtype=dtype, order="F")
    assert ora.bidiagonalization(ora.DiagOp(d), ora.DiagOp(d.conj()), Uo, Vo, Bo, kstart=k0, kend=k0) == 0
    alpha, vk, beta, u = bidiag_step_longdouble(d, X0, V0)
    _cols_close(Bo[k0 - 1:, k0 - 1], np.array([alpha, beta]), name + " bidiag B column")
    assert not Bo[:k0 - 1, k0 - 1].any()
    _cols_close(Vo[:, k0 - 1], vk, name + " bidiag v")
    _cols_close(Uo[:, k0], u, name + " bidiag u")

    p = 2
    Xo, Ho = start(k0 + p), np.zeros((k0 + p, k0), dtype=dtype, order="F")
    assert ora.arnoldi_block(ora.DiagOp(d), Xo, Ho, p, kstart=k0 // p, kend=k0 // p) == 0
    Hb, R, W = arnoldi_block_step_longdouble(d, X0, p)
    for j in range(p):
        _cols_close(Ho[:, k0 - p + j], np.concatenate([Hb[:, j], R[:, j]]), name + f" arnoldi_block H column {j}")
    _cols_close(Xo[:, k0:], W, name + " arnoldi_block vectors")
