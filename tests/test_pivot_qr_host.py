"""Column-pivoting qr and block kexpm, the parts that need no GPU.

  * the NumPy restatement the GPU tests compare against (tests/_pivot_ref.py) passes the reference's own known answers: the
    rank-deficiency test of the pivoting qr (test/TestKrylov.fypp:101-174) and the block kexpm test (test/TestExpmlib.fypp:148-230);
  * lk_norm2_dense (one-sided Jacobi, host only) against numpy.linalg.norm(., 2) at 1e-13 relative -- the bound the tests of
    lk_expm_dense use --, and its argument errors;
  * permcols / invperm, the C signatures, and the host route of `qr(..., perm=)` and block `kexpm` on a user vector type against
    the restatement (same arithmetic: the results agree to rounding)."""
import ctypes as C

import numpy as np
import pytest

import lightkrylov_amd as lk
from lightkrylov_amd import _capi
from lightkrylov_amd.expm import expm, norm2
from oracle import oracle as ora
from tests import _pivot_ref as ref
from tests._oracle_vector import oracle_dense_linop, oracle_vector

KINDS = [np.float64, np.complex128]
_DP = C.POINTER(C.c_double)


def _rand(rng, shape, dtype):
    a = rng.standard_normal(shape)
    if np.dtype(dtype).kind == "c":
        a = a + 1j * rng.standard_normal(shape)
    return np.asfortranarray(a, dtype=dtype)


# ---- the restatement against the reference's known answers -------------------------------------------------------------
@pytest.mark.parametrize("dtype", KINDS)
def test_restatement_rank_deficiency(dtype):
    """test/TestKrylov.fypp:101-174: 20 columns, 5 of them zero; A(:, perm) = Q R and Q^H Q = I below rtol_dp"""
    rng = np.random.default_rng(5)
    n, p, nzero = 100, 20, 5
    A = _rand(rng, (n, p), dtype)
    A[:, rng.choice(p, nzero, replace=False)] = 0
    Q = A.copy(order="F")
    R = np.zeros((p, p), dtype=dtype, order="F")
    perm = np.zeros(p, dtype=int)
    info = ref.qr_with_pivoting(Q, R, perm, tol=ref.ATOL_DP)
    assert info == p - nzero + 1
    assert sorted(perm) == list(range(1, p + 1))
    assert np.abs(A[:, perm - 1] - Q @ R).max() < ref.RTOL_DP
    assert np.linalg.norm(np.abs(Q.conj().T @ Q - np.eye(p)), 2) < ref.RTOL_DP


@pytest.mark.parametrize("dtype", KINDS)
def test_restatement_block_kexpm_against_dense(dtype):
    """test/TestExpmlib.fypp:148-230: p = 3, tau = 0.1, tol = rtol_dp, kdim = 15, against the dense exponential below rtol_dp"""
    rng = np.random.default_rng(11)
    n, p, tau, kdim = 100, 3, 0.1, 15
    A = _rand(rng, (n, n), dtype)
    B = _rand(rng, (n, p), dtype)
    Cref = expm(tau * A) @ B
    Cb, info, err, _ = ref.kexpm_mat(ora.DenseOp(A), B, tau, ref.RTOL_DP, kdim * p)
    assert info > 0 and err <= ref.RTOL_DP
    D = Cb - Cref
    assert np.linalg.norm(np.abs(D.conj().T @ D), 2) < ref.RTOL_DP


# ---- lk_norm2_dense ------------------------------------------------------------------------------------------------------
def _norm2_cases():
    rng = np.random.default_rng(3)
    for dtype in KINDS:
        for m in (0, 1, 2, 3, 8):
            for n in (0, 1, 2, 3, 8):
                yield f"rand-{np.dtype(dtype).name}-{m}x{n}", _rand(rng, (m, n), dtype)
        U, _ = np.linalg.qr(_rand(rng, (8, 8), dtype))
        V, _ = np.linalg.qr(_rand(rng, (8, 8), dtype))
        yield f"graded-{np.dtype(dtype).name}", np.asfortranarray((U * np.logspace(0, -12, 8)) @ V.conj().T)
        yield f"graded-small-first-{np.dtype(dtype).name}", np.asfortranarray((U * np.logspace(-12, 0, 8)) @ V.conj().T)
        d = np.array([3.0, 1.0, 0.5, 0, 0, 0, 0, 0])
        yield f"rank3-{np.dtype(dtype).name}", np.asfortranarray((U * d) @ V.conj().T)
        yield f"tall-{np.dtype(dtype).name}", _rand(rng, (8, 3), dtype)
        yield f"wide-{np.dtype(dtype).name}", _rand(rng, (3, 8), dtype)
        yield f"zero-{np.dtype(dtype).name}", np.zeros((4, 4), dtype=dtype, order="F")
        x = _rand(rng, (5, 1), dtype)
        yield f"equal-columns-{np.dtype(dtype).name}", np.asfortranarray(np.hstack([x, x, 2 * x]))


@pytest.mark.parametrize("name,A", list(_norm2_cases()), ids=[c[0] for c in _norm2_cases()])
def test_norm2_dense_against_numpy(name, A):
    want = float(np.linalg.norm(A, 2)) if A.size else 0.0
    got = norm2(A)
    print(f"{name}: got {got:.17g} want {want:.17g}")
    assert abs(got - want) <= 1e-13 * want


def test_norm2_dense_leading_dimension_and_errors():
    lib = _capi.load()
    rng = np.random.default_rng(4)
    big = np.asfortranarray(rng.standard_normal((7, 4)))
    out = C.c_double(-1.0)
    assert lib.lk_norm2_dense(_capi.LK_F64, 3, 4, big.ctypes.data_as(_DP), 7, C.byref(out)) == 0
    want = np.linalg.norm(big[:3, :], 2)
    assert abs(out.value - want) <= 1e-13 * want
    a = big.ctypes.data_as(_DP)
    out = C.c_double(-1.0)
    for args in [(7, 3, 4, a, 7), (_capi.LK_F64, -1, 4, a, 7), (_capi.LK_F64, 3, -4, a, 7), (_capi.LK_F64, 3, 4, None, 7),
                 (_capi.LK_F64, 3, 4, a, 2)]:
        assert lib.lk_norm2_dense(*args, C.byref(out)) == -1, args
        assert out.value == -1.0
    assert lib.lk_norm2_dense(_capi.LK_F64, 3, 4, a, 7, None) == -1
    assert lib.lk_norm2_dense(_capi.LK_F64, 0, 4, None, 0, C.byref(out)) == 0 and out.value == 0.0
    with pytest.raises(ValueError):
        norm2(np.zeros(3))
    assert np.isnan(norm2(np.array([[1.0, np.nan], [0.0, 1.0]])))


# ---- permutations, signatures --------------------------------------------------------------------------------------------
def test_permcols_invperm_invert_a_column_permutation():
    rng = np.random.default_rng(8)
    R = np.asfortranarray(rng.standard_normal((6, 6)))
    perm = (rng.permutation(6) + 1).astype(np.intc)
    P = np.asfortranarray(R[:, perm - 1])
    lk.permcols(P, lk.invperm(perm))
    assert np.array_equal(P, R)
    assert np.array_equal(lk.invperm(lk.invperm(perm)), perm)
    assert np.array_equal(lk.invperm(perm), ref.invperm(perm))
    vecs = [oracle_vector(np.full(3, float(i))) for i in range(6)]
    lk.permcols(vecs, perm)
    assert [v.data[0] for v in vecs] == [float(i - 1) for i in perm]


def test_new_entries_are_bound():
    for name, nargs in (("lk_norm2_dense", 6), ("lk_qr_pivot", 8), ("lk_kexpm_block", 13)):
        assert name in _capi.SIGNATURES
        assert len(_capi.SIGNATURES[name][1]) == nargs
        assert getattr(_capi.load(), name) is not None


# ---- the host route (user vector types) against the restatement ------------------------------------------------------------
def _vectors(M, seeds=None):
    return [oracle_vector(M[:, j].copy(), seed=(seeds(j) if seeds else 0)) for j in range(M.shape[1])]


@pytest.mark.parametrize("dtype", KINDS)
def test_qr_with_perm_on_a_user_vector_type(dtype):
    rng = np.random.default_rng(21)
    n, p = 37, 6
    A = _rand(rng, (n, p), dtype) * 2.0 ** (-rng.permutation(p))
    A[:, 4] = 0
    Q, R, perm = A.copy(order="F"), np.zeros((p, p), dtype=dtype, order="F"), np.zeros(p, dtype=int)
    info_r = ref.qr_with_pivoting(Q, R, perm)
    vecs = _vectors(A, seeds=ref.engine_stream())
    Rh, permh = np.zeros((p, p), dtype=dtype, order="F"), np.zeros(p, dtype=np.intc)
    info = lk.qr(vecs, Rh, perm=permh)
    assert info == info_r == p
    assert np.array_equal(permh, perm)
    assert np.abs(Rh - R).max() <= 1e-13 * np.abs(R).max()
    Qh = np.column_stack([v.data for v in vecs])
    assert np.abs(Qh - Q).max() <= 1e-12
    with pytest.raises(ValueError):
        lk.qr(vecs, Rh, perm=np.zeros(p - 1, dtype=np.intc))
    with pytest.raises(ValueError):
        lk.qr(vecs, Rh, perm=np.zeros(p))


@pytest.mark.parametrize("dtype", KINDS)
def test_block_kexpm_on_a_user_vector_type(dtype):
    """kexpm with sequences of vectors runs kexpm_mat on the primitives: same info and result as the restatement, operator counter
    advanced by p per block step, a workspace that is too small refused, nk capped at 512 // p - 1 for a workspace made inside"""
    rng = np.random.default_rng(12)
    n, p, tau, tol = 60, 3, 0.05, 1e-9
    A = _rand(rng, (n, n), dtype)
    B = _rand(rng, (n, p), dtype)
    hist = []
    Cr, info_r, err_r, _ = ref.kexpm_mat(ora.DenseOp(A), B, tau, tol, 4 * p, history=hist)
    assert info_r > 0
    op = oracle_dense_linop(A)
    Cv = _vectors(np.zeros_like(B))
    info = lk.kexpm(Cv, op, _vectors(B), tau, tol, kdim=4)
    assert info == info_r
    Ch = np.column_stack([v.data for v in Cv])
    assert np.abs(Ch - Cr).max() <= 1e-12 * np.abs(Cr).max()
    assert op.matvec_counter == len(hist) * p and op.rmatvec_counter == 0
    assert np.abs(Ch - expm(tau * A) @ B).max() < ref.RTOL_DP
    with pytest.raises(ValueError):
        lk.kexpm(Cv, op, _vectors(B), tau, tol, kdim=4, _basis=_vectors(np.zeros((n, p * (4 * p + 1) - 1), dtype=dtype)))
    # not converged: info = -1 and the nk-step approximation
    Cr1, info_r1, _, _ = ref.kexpm_mat(ora.DenseOp(A), B, tau, 1e-300, p)           # kdim = 1: nk = p block steps (:276)
    info1 = lk.kexpm(Cv, op, _vectors(B), tau, 1e-300, kdim=1, _basis=_vectors(np.zeros((n, p * (p + 1)), dtype=dtype)))
    assert info1 == info_r1 == -1
    Ch = np.column_stack([v.data for v in Cv])
    assert np.abs(Ch - Cr1).max() <= 1e-12 * np.abs(Cr1).max()


def test_block_kexpm_caps_the_workspace_it_allocates():
    import sys
    E = sys.modules["lightkrylov_amd.expm"]          # (the package attribute of that name is the function)
    seen = {}
    orig = E._workspace

    def spy(b, ncols):
        seen["ncols"] = ncols
        return orig(b, ncols)
    E._workspace = spy
    try:
        n, p = 30, 3
        rng = np.random.default_rng(2)
        A, B = _rand(rng, (n, n), np.float64), _rand(rng, (n, p), np.float64)
        Cv = _vectors(np.zeros_like(B))
        info = lk.kexpm(Cv, oracle_dense_linop(A), _vectors(B), 0.1, 1e-9)          # kdim = 100: nk = 300 -> capped
    finally:
        E._workspace = orig
    assert seen["ncols"] == p * (512 // p) <= 512
    assert info > 0
