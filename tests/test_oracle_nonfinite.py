"""Where the reference stops on a NaN, pinned on the oracle before the engine is compared with it (test_gpu_nonfinite.py).

qr_no_pivoting stops with "|beta| = NaN detected! Abort" (qr.fypp:137-143) at the first column whose norm is NaN; Arnoldi reaches it through the
one-column qr of every step (arnoldi.fypp:53; the C oracle returns -1, lk_oracle_body.inc).  Lanczos (lanczos.fypp:24-40) and the Gram-Schmidt
step (gram_schmidt.fypp:12-57) have no such test: they run on and leave NaN behind.  The step that "fails" is, on every path, the first one
whose column of the projected matrix holds a NaN."""
import numpy as np
import pytest

from oracle import oracle as ora
from tests._gpu_helpers import KINDS, basis, orthonormal_basis, seeded


def first_nan_column(H):
    """1-based index of the first column of H holding a NaN (0: none)"""
    bad = np.flatnonzero(np.isnan(H).any(axis=0))
    return int(bad[0]) + 1 if bad.size else 0


def nan_on_call(d, s):
    """y = d .* x, except that the s-th application (1-based) puts a NaN into one entry of y (a time-stepper that diverged)"""
    calls = [0]

    def f(x):
        calls[0] += 1
        y = d * x
        if calls[0] == s:
            y[len(y) // 3] = np.nan
        return y
    return f


def _diag(n, dtype):
    g = np.arange(n) / n
    return ((1.0 + g) * (np.exp(0.4j * g) if np.dtype(dtype).kind == "c" else 1.0)).astype(dtype)


@pytest.mark.parametrize("dtype", KINDS)
def test_arnoldi_aborts_at_the_step_whose_operator_output_is_nan(dtype):
    n, m, s = 203, 10, 4
    d = _diag(n, dtype)
    x0 = seeded(n, dtype, 3)
    X = np.zeros((n, m + 1), dtype=dtype, order="F")
    X[:, 0] = x0 / np.linalg.norm(x0)
    H = np.zeros((m + 1, m), dtype=dtype, order="F")
    assert ora.arnoldi(ora.PyOp(nan_on_call(d, s), dtype), X, H) == -1
    assert first_nan_column(H) == s and np.isfinite(H[:, :s - 1]).all() and not H[:, s:].any()
    # a NaN in the start vector: step 1
    X[5, 0] = np.nan
    H[...] = 0
    assert ora.arnoldi(ora.DiagOp(d), X, H) == -1
    assert first_nan_column(H) == 1 and not H[:, 1:].any()


@pytest.mark.parametrize("dtype", KINDS)
def test_qr_aborts_at_the_first_nan_column(dtype):
    n, p, j = 203, 5, 3
    Q = basis(n, p, dtype, 30)
    Q[17, j] = np.nan
    R = np.zeros((p, p), dtype=dtype, order="F")
    with pytest.raises(FloatingPointError, match="NaN detected"):
        ora.qr_no_pivoting(Q, R)
    assert np.isfinite(R[:, :j]).all() and np.isnan(R[:j, j]).all() and not R[:, j + 1:].any()
    assert np.isfinite(Q[:, :j]).all()


@pytest.mark.parametrize("dtype", KINDS)
def test_lanczos_does_not_abort_on_nan(dtype):
    n, m, s = 203, 10, 4
    d = np.real(_diag(n, dtype)).astype(dtype)
    x0 = seeded(n, dtype, 5)
    X = np.zeros((n, m + 1), dtype=dtype, order="F")
    X[:, 0] = x0 / np.linalg.norm(x0)
    T = np.zeros((m + 1, m), dtype=dtype, order="F")
    assert ora.lanczos(ora.PyOp(nan_on_call(d, s), dtype), X, T) == 0           # `beta < tol` is false for a NaN: the loop runs on
    assert first_nan_column(T) == s and np.isfinite(T[:, :s - 1]).all() and np.isnan(T[:, s:]).any(axis=0).all()


@pytest.mark.parametrize("where", ["y", "basis"])
@pytest.mark.parametrize("dtype", KINDS)
def test_dgs_runs_on_through_nan(dtype, where):
    """no NaN test in double_gram_schmidt_step: every coefficient and every entry of y'' is NaN, info stays 0 (NaN < atol is false)"""
    n, k = 203, 8
    X = orthonormal_basis(n, k, dtype, 50)
    y = seeded(n, dtype, 51)
    if where == "y":
        y[11] = np.nan
    else:
        X[11, 3] = np.nan
    h, info = ora.double_gram_schmidt_step(y, X)
    assert info == 0 and np.isnan(h).all() and np.isnan(y).all()
