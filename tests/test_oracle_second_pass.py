"""The inputs and the two references of tests/test_gpu_second_pass.py, checked without a GPU.

On an orthonormal basis the second pass of double_gram_schmidt_step (gram_schmidt.fypp:12-57) corrects rounding noise: h2 = X^H y' is about
1e-16 |y|, four orders below the 1e-12 the results are compared at, and a step that skips the pass, adds h2 with the wrong sign or drops
one of its entries agrees with the reference.  On `skewed_basis` (off orthonormal by 1e-3) h2 is about 1e-3 |y|, and here every such mutant,
built in numpy from the longdouble pieces, is shown to lie at least 1e3 x the 1e-12 bar away from the oracle -- while the oracle (the
reference's own double arithmetic) and the longdouble evaluation agree within 1e-13 |y|, a tenth of the bar, so the two references of the GPU
tests cannot pull apart by more than a tenth of what those tests allow."""
import numpy as np
import pytest

from oracle import oracle as ora
from tests._gpu_helpers import (KINDS, arnoldi_operator, assert_second_pass_matters, dgs_longdouble, orthonormal_basis, second_pass_input,
                                seeded, skewed_basis, _long)
from tests._tol import RTOL

REF_AGREE = 1e-13                # oracle against longdouble: a tenth of RTOL (measured <= 2e-16 on these inputs)
MARGIN = 1e3 * RTOL              # what a mutant must differ by from the oracle, relative to |y|
SHAPES = [(29, 5), (1037, 1), (1037, 2), (1037, 33), (4099, 17), (5003, 129), (20011, 128)]


def _inputs(n, k, dtype):
    """the inputs of the GPU tests that the guard applies to, from the builder those tests use: (skewed X, random y) and
    (skewed X, y near span(X))"""
    out = []
    for which in ("skew_rand", "skew_span"):
        X, Y = second_pass_input(n, k, dtype, which)
        out.append((which, X, Y[:, 0].copy()))
    return out


def _mutants(X, y, h1, h2, y1, y2):
    """(name, beta, y'') of the five wrong second passes, in longdouble"""
    Xl = _long(X)
    drop = h2.copy()
    drop[-1] = 0
    out = [("pass 2 skipped", h1, y1),
           ("h = h1 - h2", h1 - h2, y2),
           ("y' + X h2", h1 + h2, y1 + Xl @ h2),
           ("last h2 entry dropped", h1 + drop, y1 - Xl @ drop)]
    if X.dtype.kind == "c":
        noconj = Xl.T @ y1
        out.append(("h2 without conj", h1 + noconj, y1 - Xl @ noconj))
    return out


def _dist(beta, yy, ho, yo, ynorm):
    return max(float(np.abs(beta - ho).max()), float(np.abs(yy - yo).max())) / ynorm


@pytest.mark.parametrize("dtype", KINDS)
@pytest.mark.parametrize("n,k", SHAPES)
def test_step_references_agree_and_every_mutant_is_far(dtype, n, k):
    for what, X, y in _inputs(n, k, dtype):
        ynorm = float(np.linalg.norm(y))
        h1, h2, y1, y2 = dgs_longdouble(y, X)
        share = assert_second_pass_matters(h1, h2, y)
        yo = y.copy()
        ho, info = ora.double_gram_schmidt_step(yo, X.copy(order="F"))
        assert info == 0
        agree = _dist(h1 + h2, y2, ho, yo, ynorm)
        print(f"{np.dtype(dtype).name} n = {n} k = {k} {what}: max|h2| / |y| = {share:.1e}, oracle - longdouble = {agree:.1e}")
        assert agree <= REF_AGREE, (what, agree)
        for name, beta, yy in _mutants(X, y, h1, h2, y1, y2):
            d = _dist(beta, yy, ho, yo, ynorm)
            print(f"    {name}: {d:.1e}")
            assert d >= MARGIN, f"{what}, {name}: only {d:.2e} from the oracle; a GPU test at {RTOL:.0e} could not see it"


@pytest.mark.parametrize("dtype", KINDS)
def test_orthonormal_inputs_hide_the_second_pass(dtype):
    """what the new inputs are for: on an orthonormal Q and a random y the guard refuses the input, and the mutants that leave the first pass
    alone pass the 1e-12 bar"""
    n, k = 1037, 33
    Q = orthonormal_basis(n, k, dtype, 40 + k)
    y = seeded(n, dtype, 5000 + k)
    ynorm = float(np.linalg.norm(y))
    h1, h2, y1, y2 = dgs_longdouble(y, Q)
    with pytest.raises(AssertionError):
        assert_second_pass_matters(h1, h2, y)
    yo = y.copy()
    ho, _ = ora.double_gram_schmidt_step(yo, Q.copy(order="F"))
    for name, beta, yy in _mutants(Q, y, h1, h2, y1, y2)[:4]:
        assert _dist(beta, yy, ho, yo, ynorm) <= RTOL, name


def arnoldi_longdouble(d, X0, m, passes=2):
    """Arnoldi steps k0 .. m on the diagonal operator d, continued from the k0 columns of X0, everything in longdouble: step k
    orthogonalises A x_k against columns 1 .. k with `passes` Gram-Schmidt passes, normalises, and fills column k of H (arnoldi.fypp:36-62)."""
    n, k0 = X0.shape
    dl = _long(d)
    X = np.zeros((n, m + 1), dtype=_long(X0).dtype)
    X[:, :k0] = _long(X0)
    H = np.zeros((m + 1, m), dtype=X.dtype)
    for k in range(k0, m + 1):
        v = dl * X[:, k - 1]
        Xk = X[:, :k]
        h = np.zeros(k, dtype=X.dtype)
        for _ in range(passes):
            c = Xk.conj().T @ v
            v = v - Xk @ c
            h += c
        beta = np.sqrt((v.conj() @ v).real)
        H[:k, k - 1], H[k, k - 1] = h, beta
        X[:, k] = v / beta
    return H


@pytest.mark.parametrize("dtype", KINDS)
def test_arnoldi_continued_from_a_skewed_block(dtype):
    """ora.arnoldi(kstart = k0) on a leading block of k0 skewed columns against the longdouble restatement, columns k0 .. m of H normwise
    per column within 1e-13; with one pass per step instead of two the columns differ by far more than 1e3 x the bar."""
    n, k0, m = 5003, 12, 24
    d = arnoldi_operator(n, dtype)
    X0 = skewed_basis(n, k0, dtype, 40 + k0)
    Xo = np.zeros((n, m + 1), dtype=dtype, order="F")
    Xo[:, :k0] = X0
    Ho = np.zeros((m + 1, m), dtype=dtype, order="F")
    assert ora.arnoldi(ora.DiagOp(d), Xo, Ho, kstart=k0) == 0
    assert not Ho[:, :k0 - 1].any()                                    # the columns before kstart are not touched

    def worst(H):
        return max(float(np.abs(H[:, j] - Ho[:, j]).max() / np.abs(Ho[:, j]).max()) for j in range(k0 - 1, m))

    two, one = worst(arnoldi_longdouble(d, X0, m)), worst(arnoldi_longdouble(d, X0, m, passes=1))
    print(f"{np.dtype(dtype).name}: oracle - longdouble per column {two:.1e}; one pass only {one:.1e}")
    assert two <= REF_AGREE
    assert one >= MARGIN
