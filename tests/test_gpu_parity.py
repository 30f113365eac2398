"""GPU parity tests: the HIP engine (through the C ABI / its host mirror) against the CPU oracle
on the same seeded inputs.  Floating-point path => tolerances, stated per test:

  * primitives that are one rounding per element (scal, axpby, copy, zero, rand, diag matvec):
    element-wise <= 4 ulp-ish (1e-15 relative) -- FMA contraction on the GPU is the only difference;
  * reductions (dot, norm, innerprod, DGS coefficients, H): NORMWISE 1e-12 -- the GPU sums in a
    tree, the reference sequentially; north_star's tolerance is 1e-12 rtol.
"""
import numpy as np
import pytest

import lightkrylov_amd as lk
from oracle import oracle as ora
from tests._tol import assert_close, assert_columns_close, assert_ritz_close

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[1, 0], ids=["single_launch", "three_sweeps"])
def ctx(request, ctx):
    """Every test of this file that takes the shared context runs on BOTH schedules of the Gram-Schmidt step: the single persistent
    launch for cache-resident panels (csrc/lk_resident.hip.h, the default) and the three sweeps -- at these sizes the single launch
    would otherwise take every panel and the sweeps would lose their small-size coverage.  (Full-size cases never fit the caches:
    once is enough.)"""
    if request.param == 0 and "full_size" in request.node.name:
        pytest.skip("the panel does not fit the caches: the three-sweep schedule ran in the other parametrisation")
    ctx.set_tuning("resident", request.param)
    yield ctx
    ctx.set_tuning("resident", 1)

KINDS = [np.float64, np.complex128]
SIZES = [1, 2, 3, 63, 64, 65, 127, 128, 129, 1000, 4099, 100_003]
RTOL_RED = 1e-12


def seeded(n, dtype, seed):
    x = np.empty(n, dtype=dtype)
    ora.fill_counter(x, seed)
    return x


def basis(n, k, dtype, seed):
    X = np.empty((n, k), dtype=dtype, order="F")
    for j in range(k):
        ora.fill_counter(X[:, j], seed + j)
    return X


def orthonormal_basis(n, k, dtype, seed):
    Q, _ = np.linalg.qr(basis(n, k, dtype, seed))
    return np.asfortranarray(Q)


def scalars(dtype):
    return (0.37 - 1.2j, -1.5 + 0.25j) if np.dtype(dtype).kind == "c" else (0.37, -1.5)


# ----------------------------------------------------------------------------- primitives
@pytest.mark.parametrize("dtype", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_blas1_against_oracle(ctx, dtype, n):
    a, b = scalars(dtype)
    x, y = seeded(n, dtype, 1), seeded(n, dtype, 2)
    vx, vy = lk.dense_vector_gpu.from_array(x, ctx), lk.dense_vector_gpu.from_array(y, ctx)
    assert vx.get_size() == n

    # dot / norm (conjugation on self)
    ref = ora.dot(x, y)
    got = vx.dot(vy)
    scale = np.linalg.norm(x) * np.linalg.norm(y)
    assert abs(got - ref) <= RTOL_RED * scale
    assert abs(vx.norm() - ora.norm(x)) <= RTOL_RED * ora.norm(x)

    # scal
    xs = x.copy()
    ora.scal(xs, a)
    vx.scal(a)
    np.testing.assert_allclose(vx.to_array(), xs, rtol=1e-15, atol=1e-15)

    # axpby (true y = a x + b y)
    ys = y.copy()
    ora.axpby(a, xs, b, ys)
    vy.axpby(a, vx, b)
    np.testing.assert_allclose(vy.to_array(), ys, rtol=4e-15, atol=4e-15)

    # add / sub / chsgn
    vy.add(vx); ora.axpby(1.0, xs, 1.0, ys)
    vy.sub(vx); vy.sub(vx); ora.axpby(-1.0, xs, 1.0, ys); ora.axpby(-1.0, xs, 1.0, ys)
    vy.chsgn(); ora.scal(ys, -1.0)
    np.testing.assert_allclose(vy.to_array(), ys, rtol=1e-14, atol=1e-14)

    # copy / zero
    vz = vx.zeros_like()
    lk.copy(vz, vx)
    assert np.array_equal(vz.to_array(), vx.to_array())
    vz.zero()
    assert not vz.to_array().any()
    # axpby with beta = 0 overwrites (true axpby)
    vz.axpby(a, vx, 0.0)
    np.testing.assert_allclose(vz.to_array(), a * vx.to_array(), rtol=4e-15, atol=1e-300)


@pytest.mark.parametrize("dtype", KINDS)
def test_rand_is_the_shared_counter_generator(ctx, dtype):
    n = 10_007
    v = lk.dense_vector_gpu(n, dtype, ctx)
    v.rand(False, seed=42)
    assert np.array_equal(v.to_array(), seeded(n, dtype, 42))      # bit-exact: integer hash + exact scaling
    v.rand(True, seed=43)
    assert abs(v.norm() - 1.0) < 1e-14


def test_empty_vector(ctx):
    v = lk.dense_vector_gpu(0, np.float64, ctx)
    w = lk.dense_vector_gpu(0, np.float64, ctx)
    v.zero(); v.scal(2.0); v.axpby(1.0, w, 1.0)
    assert v.dot(w) == 0.0 and v.norm() == 0.0 and v.get_size() == 0


def test_size_mismatch_is_an_error(ctx):
    v = lk.dense_vector_gpu(10, np.float64, ctx)
    w = lk.dense_vector_gpu(11, np.float64, ctx)
    with pytest.raises(lk._capi.LightKrylovHipError, match="Inconsistent size"):
        v.axpby(1.0, w, 1.0)                       # reference: stop_error("Inconsistent size between the two vectors.")
    c = lk.dense_vector_gpu(10, np.complex128, ctx)
    with pytest.raises(lk._capi.LightKrylovHipError):
        v.dot(c)


# ----------------------------------------------------------------------------- basis helpers
@pytest.mark.parametrize("dtype", KINDS)
@pytest.mark.parametrize("n,k,p", [(1000, 1, 1), (1003, 7, 1), (4099, 16, 2), (4099, 17, 1), (20_001, 64, 1),
                                   (20_001, 128, 1), (777, 130, 1), (5000, 200, 2), (3001, 100, 40), (2999, 128, 17)])
def test_innerprod_lincomb_gram(ctx, dtype, n, k, p):
    X, Y = basis(n, k, dtype, 10), basis(n, p, dtype, 500)
    Bx = lk.krylov_basis_gpu(n, k, dtype, ctx); Bx.upload(X)
    By = lk.krylov_basis_gpu(n, p, dtype, ctx); By.upload(Y)
    M = lk.innerprod(Bx, By)
    Mo = ora.innerprod(X, Y)
    scale = np.linalg.norm(X, axis=0).max() * np.linalg.norm(Y, axis=0).max()
    assert np.abs(M - Mo).max() <= RTOL_RED * scale
    m1 = lk.innerprod(Bx, By[0])
    assert np.abs(m1 - Mo[:, 0]).max() <= RTOL_RED * scale

    # linear_combination: Y = X C
    Cm = basis(k, p, dtype, 900)
    Yg = lk.linear_combination(Bx, Cm).download()
    for j in range(p):
        ref = ora.linear_combination(X, np.ascontiguousarray(Cm[:, j]))
        assert np.abs(Yg[:, j] - ref).max() <= 1e-13 * np.abs(ref).max() * max(1, k) ** 0.5

    if k <= 17:
        G = lk.Gram(Bx)
        Go = ora.gram(X)
        assert np.abs(G - Go).max() <= RTOL_RED * scale * (n / 1000)


# ----------------------------------------------------------------------------- the sweep
DGS_CASES = [(1000, 1), (1001, 2), (999, 3), (4096, 15), (4097, 16), (4099, 17), (10_000, 31), (10_001, 33),
             (30_000, 64), (30_011, 100), (30_011, 127), (30_011, 128), (5003, 129), (5003, 200), (4001, 256), (4001, 300),
             (3001, 512), (3001, 513), (129, 64), (65, 8),
             (1, 1), (300_007, 32)]


@pytest.mark.parametrize("dtype", KINDS)
@pytest.mark.parametrize("n,k", DGS_CASES)
def test_double_gram_schmidt_step_against_oracle(ctx, dtype, n, k):
    k = min(k, n)
    Q = orthonormal_basis(n, k, dtype, 3)
    y = seeded(n, dtype, 7700)                                            # (a seed of no column: the basis uses 3 .. 3 + k - 1)
    B = lk.krylov_basis_gpu(n, k + 1, dtype, ctx)
    B.upload(Q, 0)
    B.upload(y.reshape(-1, 1), k)
    beta = np.zeros(k, dtype=dtype)
    info = lk.double_gram_schmidt_step(B[k], B[:k], if_chk_orthonormal=False, beta=beta)

    yo = y.copy()
    ho, info_o = ora.double_gram_schmidt_step(yo, Q)
    assert info == info_o
    ynorm = np.linalg.norm(y)
    assert np.abs(beta - ho).max() <= RTOL_RED * ynorm                    # coefficients, normwise
    yg = B.download(k, 1)[:, 0]
    assert np.abs(yg - yo).max() <= RTOL_RED * ynorm                      # the orthogonalised vector
    if k < n:
        assert np.abs(Q.conj().T @ yg).max() <= 1e-13 * ynorm             # orthogonality after two passes

    # single pass + shape assertion on beta
    B.upload(y.reshape(-1, 1), k)
    b1 = np.zeros(k, dtype=dtype)
    lk.orthogonalize_against_basis(B[k], B[:k], if_chk_orthonormal=False, beta=b1)
    y1 = y.copy()
    h1, _ = ora.orthogonalize_against_basis(y1, Q)
    assert np.abs(b1 - h1).max() <= RTOL_RED * ynorm
    assert np.abs(B.download(k, 1)[:, 0] - y1).max() <= RTOL_RED * ynorm
    with pytest.raises(ValueError):
        lk.double_gram_schmidt_step(B[k], B[:k], False, beta=np.zeros(k + 1, dtype=dtype))


@pytest.mark.parametrize("dtype", KINDS)
def test_dgs_zero_vector_flag_and_orthonormality_check(ctx, dtype):
    n, k = 2000, 5
    Q = orthonormal_basis(n, k, dtype, 5)
    B = lk.krylov_basis_gpu(n, k + 1, dtype, ctx)
    B.upload(Q, 0)                                                      # y = 0
    assert lk.double_gram_schmidt_step(B[k], B[:k], if_chk_orthonormal=False) == 1   # gram_schmidt.fypp:126-127
    B.upload(seeded(n, dtype, 9).reshape(-1, 1), k)
    assert lk.double_gram_schmidt_step(B[k], B[:k]) == 0                # default if_chk_orthonormal=True passes
    B.upload((2.0 * Q[:, 0]).reshape(-1, 1), 0)
    with pytest.raises(RuntimeError, match="not orthonormal"):
        lk.double_gram_schmidt_step(B[k], B[:k])


@pytest.mark.parametrize("dtype", KINDS)
def test_block_dgs_and_qr(ctx, dtype):
    n, k, p = 6001, 12, 3
    Q = orthonormal_basis(n, k, dtype, 21)
    Y = basis(n, p, dtype, 99)
    B = lk.krylov_basis_gpu(n, k + p, dtype, ctx)
    B.upload(Q, 0); B.upload(Y, k)
    beta = np.zeros((k, p), dtype=dtype, order="F")
    info = lk.double_gram_schmidt_step(B[k:k + p], B[:k], False, beta)
    assert info == 0
    for j in range(p):
        yo = Y[:, j].copy()
        ho, _ = ora.double_gram_schmidt_step(yo, Q)
        assert np.abs(beta[:, j] - ho).max() <= RTOL_RED * np.linalg.norm(Y[:, j])
    # qr_no_pivoting on the block: A = Q R, Q^H Q = I   (test/TestKrylov.fypp:52-99)
    A = B.download(k, p)
    R = np.zeros((p, p), dtype=dtype, order="F")
    assert lk.qr(B[k:k + p], R) == 0
    Qg = B.download(k, p)
    assert np.abs(Qg @ R - A).max() <= 1e-13 * np.abs(A).max() * 10
    assert np.abs(Qg.conj().T @ Qg - np.eye(p)).max() <= 1e-13


# ----------------------------------------------------------------------------- Arnoldi
def _arnoldi_pair(ctx, dtype, n, m, d, x0, fused=True):
    X = lk.krylov_basis_gpu(n, m + 1, dtype, ctx)
    X.upload(x0.reshape(-1, 1), 0)
    H = np.zeros((m + 1, m), dtype=dtype, order="F")
    A = lk.diag_linop_gpu(d, ctx)
    if not fused:
        class wrapped(lk.abstract_linop):                      # python operator => python step loop
            def matvec(self, vi, vo): A.matvec(vi, vo)
        info = lk.arnoldi(wrapped(), X, H)
    else:
        info = lk.arnoldi(A, X, H)
    Xo = np.zeros((n, m + 1), dtype=dtype, order="F")
    Xo[:, 0] = x0
    Ho = np.zeros((m + 1, m), dtype=dtype, order="F")
    info_o = ora.arnoldi(ora.DiagOp(d), Xo, Ho)
    return X, H, info, Xo, Ho, info_o


@pytest.mark.parametrize("dtype", KINDS)
@pytest.mark.parametrize("n,m,fused", [(1000, 8, True), (1000, 8, False), (100_000, 64, True), (1_000_000, 32, True),
                                       (50_001, 128, True), (20_000, 140, False)])
def test_arnoldi_diag_against_oracle(ctx, dtype, n, m, fused):
    d = (1.0 + np.arange(n) / n).astype(dtype)
    if np.dtype(dtype).kind == "c":
        d = d * np.exp(1j * 0.3 * np.arange(n) / n)
    x0 = seeded(n, dtype, 7)
    x0 /= np.linalg.norm(x0)
    X, H, info, Xo, Ho, info_o = _arnoldi_pair(ctx, dtype, n, m, d, x0, fused)
    assert info == info_o == 0
    # Hessenberg entries: normwise per column, 1e-12 (north_star)
    for j in range(m):
        assert np.abs(H[:, j] - Ho[:, j]).max() <= RTOL_RED * np.abs(Ho[:, j]).max(), f"column {j}"
    # Ritz values: 1e-12 * kappa_i * ||H||, kappa_i the COMPUTED condition number of each eigenvalue of the projected matrix (1 for the
    # real kind, whose H is symmetric tridiagonal; the rotated spectrum of the complex kind gives a non-normal H): tests/_tol.py
    rg = np.linalg.eigvals(H[:m, :m])
    ro = np.linalg.eigvals(Ho[:m, :m])
    assert_ritz_close(rg, ro, Ho[:m, :m], f"arnoldi diag n={n} m={m} {np.dtype(dtype)}")
    # invariants of test/TestKrylov.fypp:194-242 at machine precision instead of rtol_dp
    Xg = X.download()
    assert np.abs(Xg.conj().T @ Xg - np.eye(m + 1)).max() <= 1e-12
    assert np.abs(d[:, None] * Xg[:, :m] - Xg @ H).max() <= 1e-12


def test_arnoldi_kstart_kend_and_breakdown(ctx):
    n, m = 5000, 12
    d = 1.0 + np.arange(n) / n
    x0 = seeded(n, np.float64, 7); x0 /= np.linalg.norm(x0)
    X, H, *_ = _arnoldi_pair(ctx, np.float64, n, m, d, x0)
    X2 = lk.krylov_basis_gpu(n, m + 1, np.float64, ctx); X2.upload(x0.reshape(-1, 1), 0)
    H2 = np.zeros((m + 1, m), order="F")
    A = lk.diag_linop_gpu(d, ctx)
    for k in range(1, m + 1):                                   # one step at a time, as eigs drives it
        assert lk.arnoldi(A, X2, H2, kstart=k, kend=k) == 0
    assert np.array_equal(H, H2)
    assert A.matvec_counter == m
    # invariant subspace: x0 supported on 3 distinct eigenvalues => breakdown at k = 3 (arnoldi.fypp:65-71)
    d3 = np.where(np.arange(n) % 3 == 0, 1.0, np.where(np.arange(n) % 3 == 1, 2.0, 3.0))
    Xb = lk.krylov_basis_gpu(n, m + 1, np.float64, ctx); Xb.upload(x0.reshape(-1, 1), 0)
    Hb = np.zeros((m + 1, m), order="F")
    info = lk.arnoldi(lk.diag_linop_gpu(d3, ctx), Xb, Hb, tol=1e-10)
    Xo = np.zeros((n, m + 1), order="F"); Xo[:, 0] = x0
    Ho = np.zeros((m + 1, m), order="F")
    assert info == ora.arnoldi(ora.DiagOp(d3), Xo, Ho, tol=1e-10) == 3
    assert np.allclose(np.sort(np.linalg.eigvals(Hb[:3, :3]).real), [1, 2, 3], rtol=1e-12)


@pytest.mark.parametrize("dtype", KINDS)
def test_arnoldi_dense_linop_cfg1_shape(ctx, dtype):
    """configs[0]: 1000 x 1000 random dense linop, m = 30 (the reference's CPU-runnable case)."""
    n, m = 1000, 30
    rng = np.random.default_rng(1)
    A = rng.standard_normal((n, n)) / np.sqrt(n)
    if np.dtype(dtype).kind == "c":
        A = A + 1j * rng.standard_normal((n, n)) / np.sqrt(n)
    A = np.asfortranarray(A.astype(dtype))
    x0 = seeded(n, dtype, 2); x0 /= np.linalg.norm(x0)
    X = lk.krylov_basis_gpu(n, m + 1, dtype, ctx); X.upload(x0.reshape(-1, 1), 0)
    H = np.zeros((m + 1, m), dtype=dtype, order="F")
    op = lk.dense_linop_gpu(A, ctx)
    assert lk.arnoldi(op, X, H) == 0
    Xo = np.zeros((n, m + 1), dtype=dtype, order="F"); Xo[:, 0] = x0
    Ho = np.zeros((m + 1, m), dtype=dtype, order="F")
    assert ora.arnoldi(ora.DenseOp(A), Xo, Ho) == 0
    assert_columns_close(H, Ho, f"arnoldi dense 1000 x 1000 {np.dtype(dtype)}")
    # rmatvec: A^H x   (test/TestLinops.fypp:48-184)
    v, w = lk.dense_vector_gpu.from_array(x0, ctx), lk.dense_vector_gpu(n, dtype, ctx)
    op.apply_rmatvec(v, w)
    assert np.abs(w.to_array() - A.conj().T @ x0).max() <= 1e-13
    op.apply_matvec(v, w)
    assert np.abs(w.to_array() - A @ x0).max() <= 1e-13


def test_lanczos_spd_toeplitz_known_answer(ctx):
    """SPD tridiagonal Toeplitz => eigenvalues a + 2|b| cos(i pi/(n+1))  (test/TestIterativeSolvers.fypp:254-280)."""
    n = 128
    a, b = 2.5, 0.8
    A = a * np.eye(n) + b * (np.eye(n, k=1) + np.eye(n, k=-1))
    X = lk.krylov_basis_gpu(n, n + 1, np.float64, ctx)
    x0 = seeded(n, np.float64, 5); X.upload((x0 / np.linalg.norm(x0)).reshape(-1, 1), 0)
    T = np.zeros((n + 1, n), order="F")
    info = lk.lanczos(lk.dense_linop_gpu(A, ctx), X, T)
    k = info if info > 0 else n
    lam = np.sort(np.linalg.eigvalsh((T[:k, :k] + T[:k, :k].T) / 2))[::-1]
    true = np.array([a + 2 * abs(b) * np.cos(i * np.pi / (n + 1)) for i in range(1, n + 1)])
    # the reference asserts rtol_dp; symmetric T: every eigenvalue has condition number 1 -> north_star's 1e-12, elementwise
    assert k == n
    assert_close(lam / true, np.ones(n), "HIP lanczos SPD Toeplitz KAT (elementwise relative)")


# ----------------------------------------------------------------------------- solvers on the path
def test_eigs_complex_known_answer(ctx):
    """The reference's deterministic complex KAT: eigenvalues 2(n-i+1)-1 (TestIterativeSolvers.fypp:176-203)."""
    n = 128
    A = np.zeros((n, n), dtype=np.complex128)
    for i in range(1, n + 1):
        A[i - 1, i - 1] = n
        if i < n:
            A[i - 1, i] = 1j * np.sqrt(1.0 * i * (n - i))
            A[i, i - 1] = -A[i - 1, i]
    X = lk.krylov_basis_gpu(n, n, np.complex128, ctx)
    x0 = lk.dense_vector_gpu.from_array(seeded(n, np.complex128, 3), ctx)
    vals, res, info = lk.eigs(lk.dense_linop_gpu(A, ctx), X, x0=x0, tolerance=lk.atol_dp)
    true = np.array([2 * (n - i + 1) - 1 for i in range(1, n + 1)], dtype=float)
    # the reference asserts rtol_dp; A is Hermitian (normal): 1e-12, elementwise relative as in tests/test_oracle_kat.py
    assert_close(vals / true, np.ones(n), "HIP eigs complex KAT 255, 253, ..., 1 (elementwise relative)")
    V = X.download()
    assert_close(A @ V, V * vals[None, :], "HIP eigs complex KAT: A V = V diag(w)", scale=np.abs(true).max())


def test_eigs_leading_pairs_against_oracle(ctx):
    """configs[0] as an eigenproblem: nev = 4 outliers planted on a 1000 x 1000 random matrix, kdim = 30."""
    n, nev, kdim = 1000, 4, 30
    rng = np.random.default_rng(1)
    A = rng.standard_normal((n, n)) / np.sqrt(n)
    A[np.arange(4), np.arange(4)] += np.array([2.0, 1.8, 1.6, 1.4])
    A = np.asfortranarray(A)
    x0 = rng.standard_normal(n)
    X = lk.krylov_basis_gpu(n, nev, np.float64, ctx)
    vals, res, info = lk.eigs(lk.dense_linop_gpu(A, ctx), X, x0=lk.dense_vector_gpu.from_array(x0, ctx), kdim=kdim,
                              tolerance=1e-10)
    vo, ro, Vo, info_o = ora.eigs(ora.DenseOp(A), x0, nev, kdim, 1e-10)
    assert info == info_o
    assert_ritz_close(vals, vo, A, "eigs dense 1000 x 1000, nev = 4 (kappa from A)")
    V = X.download()
    for i in range(nev):
        r = A @ V[:, i] - vals[i].real * V[:, i] if abs(vals[i].imag) < 1e-14 else None
        if r is not None:
            assert np.linalg.norm(r) <= 1e-8


def test_gmres_poisson_against_oracle(ctx):
    """configs[2] at a size the oracle finishes in seconds: 5-point Laplacian, N = 96, GMRES(30), 3 cycles."""
    N = 96
    n = N * N
    b = seeded(n, np.float64, 11)
    opts = lk.gmres_dp_opts(kdim=30, maxiter=2)
    x = lk.dense_vector_gpu(n, np.float64, ctx)
    meta = lk.gmres_dp_metadata()
    info = lk.gmres(lk.laplacian2d_linop_gpu(N, ctx), lk.dense_vector_gpu.from_array(b, ctx), x, rtol=1e-8,
                    options=opts, meta=meta)
    xo = np.zeros(n)
    info_o, res_o = ora.gmres(ora.Lap5Op(N), b, xo, rtol=1e-8, kdim=30, maxiter=2)
    assert info == info_o
    assert len(meta.res) == len(res_o)
    assert_close(np.array(meta.res), res_o, "gmres Poisson N=96: residual history vs oracle", scale=res_o[0])
    assert_close(x.to_array(), xo, "gmres Poisson N=96: solution vs oracle")


# ----------------------------------------------------------------------------- size-independent properties
@pytest.mark.parametrize("dtype,n,m", [(np.float64, 10_000_000, 64), (np.complex128, 1_000_000, 128)])
def test_arnoldi_full_size_properties(ctx, dtype, n, m):
    """BASELINE configs 2 and 4 sizes: no oracle run (too slow); factorisation + orthonormality invariants,
    and linearity of the sweep (DGS of a y + b z equals a DGS(y) + b DGS(z) up to rounding)."""
    if np.dtype(dtype).kind == "c":
        dvals = (1.0 + np.arange(n) / n) * np.exp(1j * np.arange(n) / n)
        op = lk.diag_linop_gpu(dvals.astype(dtype), ctx)
    else:
        dvals = 1.0 + np.arange(n) / n
        op = lk.diag_linop_gpu(n_local=n, d0=1.0, dstep=1.0 / n, ctx=ctx)
    X = lk.krylov_basis_gpu(n, m + 1, dtype, ctx)
    X[0].rand(True, seed=7)
    H = np.zeros((m + 1, m), dtype=dtype, order="F")
    assert lk.arnoldi(op, X, H) == 0
    G = lk.Gram(X[:m + 1]) if m <= 64 else None
    if G is not None:
        assert np.abs(G - np.eye(m + 1)).max() <= 1e-12
    # A X_m - X_{m+1} H = 0 checked through random probes:  w^H (A X - X H) for a few rows blocks
    Xh = X.download(0, m + 1)[:200_000]
    assert np.abs(dvals[:200_000, None] * Xh[:, :m] - Xh @ H).max() <= 1e-12
    # Ritz values are those of a normal operator with spectrum on a known curve
    ritz = np.linalg.eigvals(H[:m, :m])
    assert (np.abs(ritz) >= 1.0 - 1e-9).all() and (np.abs(ritz) <= 2.0 + 1e-9).all()


# ----------------------------------------------------------------------------- Ginzburg-Landau stepper (config 4)
def _gl_pair(ctx, n, tau, nsub):
    A = lk.ginzburg_landau_linop_gpu(n, ctx, tau=tau, nsub=nsub)
    p = A.params
    Ao = ora.GLOp(n, p["dx"], tau, nsub, p["nu"], p["gamma"], p["mu_c"], p["mu2"])
    Aadj = ora.GLOp(n, p["dx"], tau, nsub, p["nu"], p["gamma"], p["mu_c"], p["mu2"], adjoint=True)
    return A, Ao, Aadj


@pytest.mark.parametrize("n,nsub", [(1, 1), (2, 1), (512, 1), (512, 3), (100_001, 2)])
def test_ginzburg_landau_stepper_against_oracle(ctx, n, nsub):
    A, Ao, Aadj = _gl_pair(ctx, n, 0.01 * nsub, nsub)
    x = seeded(n, np.complex128, 13)
    vx, vy = lk.dense_vector_gpu.from_array(x, ctx), lk.dense_vector_gpu(n, np.complex128, ctx)
    A.apply_matvec(vx, vy)
    ref = Ao.apply(x) if n > 1 else None
    if n > 2:
        assert np.abs(vy.to_array() - ref).max() <= 1e-13 * np.abs(ref).max()
        A.apply_rmatvec(vx, vy)
        refa = Aadj.apply(x)
        assert np.abs(vy.to_array() - refa).max() <= 1e-13 * np.abs(refa).max()
    assert np.isfinite(vy.to_array()).all() and np.array_equal(vx.to_array(), x)      # input untouched


def test_eigs_ginzburg_landau_reference_size_against_oracle(ctx):
    """The example's own size (nx = 512, nev = 8): leading eigenvalues of the propagator, engine vs oracle."""
    n, nev, kdim = 512, 8, 64
    A, Ao, _ = _gl_pair(ctx, n, 1.0, 40)
    x0 = seeded(n, np.complex128, 13)
    X = lk.krylov_basis_gpu(n, nev, np.complex128, ctx)
    vals, res, info = lk.eigs(A, X, x0=lk.dense_vector_gpu.from_array(x0, ctx), kdim=kdim, tolerance=1e-10)
    vo, ro, Vo, info_o = ora.eigs(Ao, x0, nev, kdim, 1e-10)
    assert info == info_o
    # 1e-12 * kappa_i * ||P||: kappa_i from the propagator's own matrix (the operator is non-normal: kappa_i > 1, printed)
    P = np.stack([Ao.apply(e) for e in np.eye(n, dtype=np.complex128)], axis=1)
    assert_ritz_close(vals, vo, P, "eigs Ginzburg-Landau nx = 512, unit-time propagator (kappa from the propagator)")
    V = X.download()
    for i in range(nev):
        assert np.linalg.norm(Ao.apply(V[:, i]) - vals[i] * V[:, i]) <= 1e-7 * abs(vals[i])


@pytest.mark.parametrize("tau,nsub", [(0.01, 1), (1.0, 40)])
def test_eigs_ginzburg_landau_full_size_properties(ctx, tau, nsub):
    """BASELINE config 4: complex(dp) n = 10^6, kdim = 128, nev = 8, with SURVEY 8(d)'s operator (ONE classical RK4
    step of tau = 0.01, main.f90:20) and with a unit-time propagator (40 sub-steps).  No oracle run at this size, and on
    a domain this long the spectrum is too clustered for Krylov-Schur to converge in a test's time.  What is
    checked is every step eigs takes: the 128-step Arnoldi factorisation A X_m = X_{m+1} H and X^H X = I,
    the same relation after a krylov_schur restart, and that a bounded eigs run returns sorted Ritz values."""
    n, nev, kdim = 1_000_000, 8, 128
    A = lk.ginzburg_landau_linop_gpu(n, ctx, tau=tau, nsub=nsub)
    X = lk.krylov_basis_gpu(n, kdim + 1, np.complex128, ctx)
    X[0].rand(True, seed=13)
    H = np.zeros((kdim + 1, kdim), dtype=np.complex128, order="F")
    assert lk.arnoldi(A, X, H) == 0
    G = lk.Gram(X)
    assert np.abs(G - np.eye(kdim + 1)).max() <= 1e-12

    w = lk.dense_vector_gpu(n, np.complex128, ctx)

    def relation_residual(ncols, j):
        A.apply_matvec(X[j], w)
        y = lk.linear_combination(X[:ncols + 1], np.ascontiguousarray(H[:ncols + 1, j]))
        w.sub(y)
        return w.norm()

    for j in (0, 63, 127):
        assert relation_residual(kdim, j) <= 1e-12 * np.abs(H[:, j]).max()
    nsel = lk.krylov_schur(X, H, lambda lam: np.abs(lam) > np.median(np.abs(lam)))
    assert 0 < nsel < kdim
    Gs = lk.Gram(X[:nsel + 1])
    assert np.abs(Gs - np.eye(nsel + 1)).max() <= 1e-12
    for j in (0, nsel - 1):
        assert relation_residual(nsel, j) <= 1e-11 * np.abs(H[:nsel + 1, :nsel]).max()

    V = lk.krylov_basis_gpu(n, nev, np.complex128, ctx)
    x0 = lk.dense_vector_gpu(n, np.complex128, ctx)
    x0.rand(False, seed=13)
    vals, res, info = lk.eigs(A, V, x0=x0, kdim=kdim, tolerance=1e-10, max_restarts=1)
    assert info >= kdim and np.isfinite(vals).all() and np.isfinite(res).all()
    assert (np.abs(vals[:-1]) >= np.abs(vals[1:]) - 1e-12).all()                       # sorted by |lambda| descending
    assert np.abs(vals).max() <= 1.05 * np.exp(A.params["mu_c"] * A.params["tau"])   # Ritz values inside ~the numerical range


def test_gmres_poisson_full_size_properties(ctx):
    """BASELINE config 3 at full size: 5-point Laplacian, N = 4096 (n = 16.8 M), GMRES(30), maxiter = 2
    (3 cycles of fixed work).  Properties: the recorded residual history equals the true residual
    ||b - A x|| at every cycle end, and is non-increasing within a cycle."""
    N = 4096
    n = N * N
    A = lk.laplacian2d_linop_gpu(N, ctx)
    b = lk.dense_vector_gpu(n, np.float64, ctx); b.rand(False, seed=11)
    x = lk.dense_vector_gpu(n, np.float64, ctx)
    meta = lk.gmres_dp_metadata()
    info = lk.gmres(A, b, x, rtol=1e-8, options=lk.gmres_dp_opts(kdim=30, maxiter=2), meta=meta)
    assert info == -meta.n_iter and meta.n_outer == 3 and meta.n_inner == 90     # not converged: info = -n_iter
    r = lk.dense_vector_gpu(n, np.float64, ctx)
    A.apply_matvec(x, r); r.sub(b)
    assert abs(r.norm() - meta.res[-1]) <= 1e-10 * meta.res[0]
    res = np.array(meta.res)
    assert res[-1] < res[0]
    for c in range(3):                                                               # [init | 30 inner, outer] x 3
        seg = res[1 + 31 * c: 1 + 31 * c + 30]
        assert (np.diff(seg) <= 1e-12 * res[0]).all()
        assert abs(res[1 + 31 * c + 30] - seg[-1]) <= 1e-8 * res[0]                  # least-squares vs true residual


@pytest.mark.parametrize("dtype", KINDS)
def test_bidiagonalization_against_oracle(ctx, dtype):
    """lanczos_bidiagonalization (golub_kahan.fypp:7-64) on a dense operator: B vs oracle, A V = U B, bases orthonormal."""
    n, kdim = 300, 40
    rng = np.random.default_rng(5)
    A = rng.standard_normal((n, n))
    if np.dtype(dtype).kind == "c":
        A = A + 1j * rng.standard_normal((n, n))
    A = np.asfortranarray(A.astype(dtype))
    u0 = seeded(n, dtype, 21); u0 /= np.linalg.norm(u0)
    U = lk.krylov_basis_gpu(n, kdim + 1, dtype, ctx); U.upload(u0.reshape(-1, 1), 0)
    V = lk.krylov_basis_gpu(n, kdim + 1, dtype, ctx)
    B = np.zeros((kdim + 1, kdim), dtype=dtype, order="F")
    assert lk.bidiagonalization(lk.dense_linop_gpu(A, ctx), U, V, B) == 0
    Uo = np.zeros((n, kdim + 1), dtype=dtype, order="F"); Uo[:, 0] = u0
    Vo = np.zeros((n, kdim + 1), dtype=dtype, order="F")
    Bo = np.zeros((kdim + 1, kdim), dtype=dtype, order="F")
    assert ora.bidiagonalization(ora.DenseOp(A), ora.DenseOp(np.asfortranarray(A.conj().T)), Uo, Vo, Bo) == 0
    assert_columns_close(B, Bo, f"bidiagonalization dense 300 x 300 {np.dtype(dtype)}")
    Ug, Vg = U.download(), V.download(0, kdim)
    assert_close(A @ Vg, Ug @ B, f"bidiagonalization relation A V = U B {np.dtype(dtype)}", scale=np.abs(B).max())
    assert np.abs(Ug.conj().T @ Ug - np.eye(kdim + 1)).max() <= 1e-12
    assert np.abs(Vg.conj().T @ Vg - np.eye(kdim)).max() <= 1e-12


# ----------------------------------------------------------------------------- lazy per-object path
@pytest.mark.parametrize("dtype", KINDS)
def test_lazy_per_object_path_batches_the_reference_schedule(dtype):
    """What an unchanged LightKrylov drives through the type-bound procedures: innerprod = k dots, then
    linear_combination = k axpbys, twice per DGS.  With the engine's lazy mode the k dots cost ONE sweep and
    the k axpbys ONE panel update, and the results equal the eager per-object path and the oracle."""
    n, k = 50_001, 37
    Q = orthonormal_basis(n, k, dtype, 3)
    y0 = seeded(n, dtype, 77)
    results = {}
    for lazy in (0, 1):
        c = lk.Context(device=0)
        c.set_tuning("lazy", lazy)
        B = lk.krylov_basis_gpu(n, k + 1, dtype, c)
        B.upload(Q, 0); B.upload(y0.reshape(-1, 1), k)
        X = [B[j] for j in range(k)]                       # python LIST of vectors => generic per-object path
        beta = np.zeros(k, dtype=dtype)
        info = lk.double_gram_schmidt_step(B[k], X, if_chk_orthonormal=False, beta=beta)
        yk = B.download(k, 1)[:, 0]
        results[lazy] = (info, beta.copy(), yk, c.lazy_stats(), c.lazy_fusion_stats())
        del X, B
        c.close()
    (i0, b0, y_eager, s0, f0), (i1, b1, y_lazy, s1, f1) = results[0], results[1]
    assert s0 == (0, 0, 0, 0) and f0 == (0, 0, 0, 0)
    hits, sweeps, queued, flushes = s1
    fused, plain, dropped, written = f1
    # pass 1: one batched dot sweep (k-1 memo hits); its projection stays virtual and is applied by pass 2's y%norm()
    # in ONE sweep that also yields the norm (1 hit) and all k dots of pass 2 (k hits); pass 2's projection is applied
    # as a plain panel update when the result is downloaded.  Neither temporary is ever written.
    assert sweeps == 1 and hits == (k - 1) + 1 + k
    assert queued == 2 * k and flushes == 0
    assert (fused, plain, dropped, written) == (1, 1, 1, 0)         # (the second temporary is still virtual: nothing has asked for it)
    yo = y0.copy()
    ho, info_o = ora.double_gram_schmidt_step(yo, Q)
    ynorm = np.linalg.norm(y0)
    assert i0 == i1 == info_o
    for b, yy in ((b0, y_eager), (b1, y_lazy)):
        assert np.abs(b - ho).max() <= RTOL_RED * ynorm and np.abs(yy - yo).max() <= RTOL_RED * ynorm


def test_lazy_mode_arnoldi_gmres_and_interleaved_calls_stay_correct():
    """Lazy mode through whole solvers (generic per-object path) and with calls that must flush / invalidate:
    a queued axpby followed by a read of y, a memo followed by a write to y, a write to a memoised column."""
    n, m = 20_011, 24
    c = lk.Context(device=0)
    c.set_tuning("lazy", 1)
    d = 1.0 + np.arange(n) / n
    A = lk.diag_linop_gpu(d, c)

    class pyop(lk.abstract_linop):                        # python operator => python step loop
        def matvec(self, vi, vo): A.matvec(vi, vo)
    x0 = seeded(n, np.float64, 7); x0 /= np.linalg.norm(x0)
    B = lk.krylov_basis_gpu(n, m + 1, np.float64, c); B.upload(x0.reshape(-1, 1), 0)
    X = [B[j] for j in range(m + 1)]
    H = np.zeros((m + 1, m), order="F")
    assert lk.arnoldi(pyop(), X, H) == 0
    Xo = np.zeros((n, m + 1), order="F"); Xo[:, 0] = x0
    Ho = np.zeros((m + 1, m), order="F")
    assert ora.arnoldi(ora.DiagOp(d), Xo, Ho) == 0
    for j in range(m):
        assert np.abs(H[:, j] - Ho[:, j]).max() <= RTOL_RED * np.abs(Ho[:, j]).max()
    assert c.lazy_stats()[1] >= m - 1 and c.lazy_fusion_stats()[0] >= 2 * (m - 1)   # batched dots (pass 1) and fused sweeps (pass 2, qr) happened

    # interleavings
    P = lk.krylov_basis_gpu(n, 4, np.float64, c)
    for j in range(4):
        P[j].rand(False, seed=30 + j)
    Ph = P.download()
    y = lk.dense_vector_gpu.from_array(seeded(n, np.float64, 40), c)
    yh = y.to_array()
    y.axpby(2.0, P[0], 1.0); y.axpby(-3.0, P[1], 1.0)     # queued
    assert abs(y.norm() - np.linalg.norm(yh + 2 * Ph[:, 0] - 3 * Ph[:, 1])) <= 1e-12 * np.linalg.norm(yh)   # norm flushes
    d0 = P[0].dot(y); d1 = P[1].dot(y)                    # d1 is a memo hit
    y.scal(0.5)                                           # write to y invalidates the memo
    d0b = P[0].dot(y)
    assert abs(d0b - 0.5 * d0) <= 1e-12 * abs(d0) and abs(d1 - Ph[:, 1] @ (yh + 2 * Ph[:, 0] - 3 * Ph[:, 1])) <= 1e-9
    P[1].scal(2.0)                                        # write to a memoised column invalidates too
    assert abs(P[1].dot(y) - 2.0 * 0.5 * d1) <= 1e-12 * abs(d1)
    y.axpby(1.0, P[2], 1.0)                               # queued, then a non-unit beta forces eager order
    y.axpby(1.0, P[3], 0.25)
    ref = 0.25 * (0.5 * (yh + 2 * Ph[:, 0] - 3 * Ph[:, 1]) + Ph[:, 2]) + Ph[:, 3]
    assert np.abs(y.to_array() - ref).max() <= 1e-13 * np.abs(ref).max()
    c.close()


@pytest.mark.parametrize("dtype", KINDS)
def test_lazy_virtual_temporary_is_written_exactly_when_something_reads_it(dtype):
    """linear_combination's temporary stays virtual in lazy mode (lk_lazy_fusion_stats).  Every way of observing it
    must see X h: reading it after it was consumed, changing a column it is defined from and then reading it, scaling
    it in place; overwriting it (zero / copy) drops it unwritten."""
    n, k = 30_007, 9
    c = lk.Context(device=0)
    c.set_tuning("lazy", 1)
    B = lk.krylov_basis_gpu(n, k + 3, dtype, c)
    for j in range(k + 3):
        B[j].rand(False, seed=50 + j)
    Xh = B.download()
    X = [B[j] for j in range(k)]
    y, T = B[k], B[k + 1]
    h = seeded(k, dtype, 5)
    tol = 1e-13 * np.abs(Xh).max() * k

    def lincomb_into_T():
        T.zero()
        for i in range(k):
            T.axpby(h[i], X[i], 1.0)

    # 1. consumed by y%sub, then read: y is updated by the fused sweep (norm), T is written when it is read
    lincomb_into_T(); y.sub(T)
    yref = Xh[:, k] - Xh[:, :k] @ h
    assert abs(y.norm() - np.linalg.norm(yref)) <= 1e-12 * np.linalg.norm(yref)
    assert c.lazy_fusion_stats()[0] == 1 and c.lazy_fusion_stats()[3] == 0
    d = np.array([X[i].dot(y) for i in range(k)])                      # memo hits of that same sweep
    assert np.abs(d - Xh[:, :k].conj().T @ yref).max() <= 1e-12 * np.linalg.norm(yref) * np.sqrt(n)
    assert np.abs(T.to_array() - Xh[:, :k] @ h).max() <= tol           # now it had to be written
    assert c.lazy_fusion_stats()[3] == 1
    assert np.abs(y.to_array() - yref).max() <= tol
    # 2. a column T is defined from changes while T is virtual: T keeps the value it had
    lincomb_into_T()
    X[2].scal(3.0)
    assert np.abs(T.to_array() - Xh[:, :k] @ h).max() <= tol
    X[2].scal(1.0 / 3.0)
    Xh2 = B.download()
    # 3. partial update of the virtual vector itself
    lincomb_into_T(); T.scal(2.0)
    assert np.abs(T.to_array() - 2.0 * (Xh2[:, :k] @ h)).max() <= 4 * tol
    # 4. overwriting drops it: no write of X h, and the new contents win
    before = c.lazy_fusion_stats()
    lincomb_into_T(); lk.copy(T, B[k + 2])
    assert np.array_equal(T.to_array(), Xh2[:, k + 2])
    lincomb_into_T(); T.zero()
    assert np.all(T.to_array() == 0)
    after = c.lazy_fusion_stats()
    assert after[2] == before[2] + 2 and after[3] == before[3]
    # 5. x%add(dx) (gmres.fypp:202) with a non-unit scale, applied by an unrelated read of x
    lincomb_into_T(); ybefore = y.to_array()
    y.axpby(-0.5, T, 1.0)
    assert np.abs(y.to_array() - (ybefore - 0.5 * (Xh2[:, :k] @ h))).max() <= 4 * tol
    # 6. the consumer is one of the columns the temporary is defined from: eager order
    lincomb_into_T(); X[1].sub(T)
    assert np.abs(X[1].to_array() - (Xh2[:, 1] - Xh2[:, :k] @ h)).max() <= 4 * tol
    c.close()


def test_lazy_per_object_arnoldi_runs_one_sweep_per_gram_schmidt_pass():
    """The reference's arnoldi through per-object vectors (python LIST => the type-bound-procedure schedule): every
    Gram-Schmidt pass after the first costs ONE fused sweep (update + dots + norm); no temporary is ever written."""
    n, m = 40_009, 12
    c = lk.Context(device=0)
    c.set_tuning("lazy", 1)
    d = 1.0 + np.arange(n) / n
    A = lk.diag_linop_gpu(d, c)

    class pyop(lk.abstract_linop):
        def matvec(self, vi, vo): A.matvec(vi, vo)
    x0 = seeded(n, np.float64, 7); x0 /= np.linalg.norm(x0)
    B = lk.krylov_basis_gpu(n, m + 1, np.float64, c); B.upload(x0.reshape(-1, 1), 0)
    X = [B[j] for j in range(m + 1)]
    H = np.zeros((m + 1, m), order="F")
    assert lk.arnoldi(pyop(), X, H) == 0
    fused, plain, dropped, written = c.lazy_fusion_stats()
    assert fused == 2 * m and plain == 0 and written == 0 and dropped == 2 * m - 1   # the last temporary is still virtual
    assert c.lazy_stats()[3] == 0                                      # no panel update outside the fused sweeps
    Xo = np.zeros((n, m + 1), order="F"); Xo[:, 0] = x0
    Ho = np.zeros((m + 1, m), order="F")
    assert ora.arnoldi(ora.DiagOp(d), Xo, Ho) == 0
    for j in range(m):
        assert np.abs(H[:, j] - Ho[:, j]).max() <= RTOL_RED * np.abs(Ho[:, j]).max()
    G = B.download()
    assert np.abs(G.T @ G - np.eye(m + 1)).max() <= 1e-12
    c.close()


@pytest.mark.parametrize("dtype", KINDS)
@pytest.mark.parametrize("p", [2, 4, 5])
def test_block_arnoldi_on_gpu_panels(ctx, dtype, p):
    """Block Arnoldi (arnoldi.fypp:34-56 with blksize = p; test/TestKrylov.fypp:244-296): the block DGS runs as a
    panel x panel schedule (two Y columns per pass over X).  A X = X+ H+ and X^H X = I; H against the oracle's
    per-column DGS applied to the same block."""
    n, kdim = 3001, 6
    rng = np.random.default_rng(11)
    A = rng.standard_normal((n, n)) / np.sqrt(n)
    if np.dtype(dtype).kind == "c":
        A = A + 1j * rng.standard_normal((n, n)) / np.sqrt(n)
    A = np.asfortranarray(A.astype(dtype))
    Q0, _ = np.linalg.qr(basis(n, p, dtype, 70))
    X = lk.krylov_basis_gpu(n, (kdim + 1) * p, dtype, ctx)
    X.upload(np.asfortranarray(Q0), 0)
    H = np.zeros(((kdim + 1) * p, kdim * p), dtype=dtype, order="F")
    assert lk.arnoldi(lk.dense_linop_gpu(A, ctx), X, H, blksize=p) == 0
    Xg = X.download()
    assert np.abs(A @ Xg[:, :kdim * p] - Xg @ H).max() <= 1e-12
    assert np.abs(Xg.conj().T @ Xg - np.eye((kdim + 1) * p)).max() <= 1e-12
    # block DGS coefficients vs the oracle on one block
    Qb = np.asfortranarray(Xg[:, :2 * p])
    Y = basis(n, p, dtype, 300)
    B = lk.krylov_basis_gpu(n, 3 * p, dtype, ctx)
    B.upload(Qb, 0); B.upload(Y, 2 * p)
    beta = np.zeros((2 * p, p), dtype=dtype, order="F")
    assert lk.double_gram_schmidt_step(B[2 * p:3 * p], B[:2 * p], False, beta) == 0
    Yg = B.download(2 * p, p)
    for j in range(p):
        yo = Y[:, j].copy()
        ho, _ = ora.double_gram_schmidt_step(yo, Qb)
        assert np.abs(beta[:, j] - ho).max() <= RTOL_RED * np.linalg.norm(Y[:, j])
        assert np.abs(Yg[:, j] - yo).max() <= RTOL_RED * np.linalg.norm(Y[:, j])


@pytest.mark.parametrize("dtype", KINDS)
def test_dgs_randomised_shapes_against_oracle(ctx, dtype):
    """60 seeded random (n, k) pairs, ragged everywhere: tile tails, k around the wave-split boundaries
    (8/16/32/64/128), k > n impossible cases clipped, fused and wide (k > 128) paths, normalise flag."""
    rng = np.random.default_rng(2024)
    for case in range(60):
        n = int(rng.choice([rng.integers(1, 40), rng.integers(40, 700), rng.integers(700, 9000)]))
        k = int(min(n, rng.choice([rng.integers(1, 10), rng.integers(10, 70), rng.integers(70, 150)])))
        Q = orthonormal_basis(n, k, dtype, 1000 + case)
        y = seeded(n, dtype, 5000 + case)
        B = lk.krylov_basis_gpu(n, k + 1, dtype, ctx)
        B.upload(Q, 0); B.upload(y.reshape(-1, 1), k)
        beta = np.zeros(k, dtype=dtype)
        norms: list = []
        info = lk.double_gram_schmidt_step(B[k], B[:k], False, beta, _normalize=bool(case % 2), _norms=norms)
        yo = y.copy()
        ho, info_o = ora.double_gram_schmidt_step(yo, Q)
        ynorm = np.linalg.norm(y)
        assert info == info_o, (case, n, k)
        assert np.abs(beta - ho).max() <= RTOL_RED * ynorm, (case, n, k)
        yg = B.download(k, 1)[:, 0]
        nyo = np.linalg.norm(yo)
        assert abs(norms[2] - nyo) <= RTOL_RED * ynorm, (case, n, k)
        if case % 2 and nyo >= lk.atol_dp:
            if nyo > 1e-10 * ynorm:                       # direction is meaningful only when y is not (numerically) in span(Q)
                assert np.abs(yg - yo / nyo).max() <= 1e-9, (case, n, k)
        else:
            assert np.abs(yg - yo).max() <= RTOL_RED * ynorm, (case, n, k)


def test_unseeded_rand_draws_fresh_vectors_and_qr_survives_colinear_columns(ctx):
    """rand() without a seed must not repeat itself (the reference's random_number does not), otherwise
    qr_no_pivoting's replacement of two colinear columns (qr.fypp:146-162) would re-create a colinear pair."""
    n = 4001
    a = lk.dense_vector_gpu(n, np.float64, ctx); b = lk.dense_vector_gpu(n, np.float64, ctx)
    a.rand(); b.rand()
    assert abs(a.dot(b)) < 0.2 * a.norm() * b.norm()
    v = seeded(n, np.float64, 1)
    v /= 4 * np.linalg.norm(v)          # residual of a colinear column is ~eps*||column||: keep it below atol_dp = 1e-15
    Q = lk.krylov_basis_gpu(n, 4, np.float64, ctx)
    Q.upload(np.asfortranarray(np.stack([v, 2 * v, -v, seeded(n, np.float64, 2)], axis=1)))
    R = np.zeros((4, 4), order="F")
    assert lk.qr(Q, R) == 2 and R[1, 1] == 0.0 and R[2, 2] == 0.0
    Qg = Q.download()
    assert np.abs(Qg.T @ Qg - np.eye(4)).max() < 1e-12


@pytest.mark.parametrize("dtype", KINDS)
def test_dense_vector_gpu_passes_the_reference_axiom_harness(ctx, dtype):
    """verify_vector_axioms on the GPU type, the reference's own conformance check for user vector types
    (AbstractVectors.fypp:733-927; test/TestVectors.fypp:50-60): test_size = 128, 100 trials, tolerance 1e-14."""
    assert lk.verify_vector_axioms(lk.dense_vector_gpu(128, dtype, ctx), ntrials=100)


@pytest.mark.parametrize("dtype", KINDS)
def test_arnoldi_and_gmres_with_transpose(ctx, dtype):
    """`transpose=.true.` (arnoldi.fypp:39-43, gmres.fypp:134-165): the factorisation / solve of A^H, through the
    engine's fused loop (rmatvec kernel) and through the python loop, against the oracle run on A^H."""
    n, m = 400, 25
    rng = np.random.default_rng(8)
    A = rng.standard_normal((n, n)) / np.sqrt(n) + 2.0 * np.eye(n)
    if np.dtype(dtype).kind == "c":
        A = A + 1j * rng.standard_normal((n, n)) / np.sqrt(n)
    A = np.asfortranarray(A.astype(dtype))
    AH = np.asfortranarray(A.conj().T)
    x0 = seeded(n, dtype, 3); x0 /= np.linalg.norm(x0)
    Xo = np.zeros((n, m + 1), dtype=dtype, order="F"); Xo[:, 0] = x0
    Ho = np.zeros((m + 1, m), dtype=dtype, order="F")
    assert ora.arnoldi(ora.DenseOp(AH), Xo, Ho) == 0
    op = lk.dense_linop_gpu(A, ctx)

    class wrapped(lk.abstract_linop):
        def matvec(self, vi, vo): op.matvec(vi, vo)
        def rmatvec(self, vi, vo): op.rmatvec(vi, vo)
    for A_ in (op, wrapped()):
        X = lk.krylov_basis_gpu(n, m + 1, dtype, ctx); X.upload(x0.reshape(-1, 1), 0)
        H = np.zeros((m + 1, m), dtype=dtype, order="F")
        assert lk.arnoldi(A_, X, H, transpose=True) == 0
        assert A_.rmatvec_counter == m and A_.matvec_counter == 0
        assert_columns_close(H, Ho, f"arnoldi transpose dense 400 x 400 {np.dtype(dtype)}")
    b = seeded(n, dtype, 4)
    x = lk.dense_vector_gpu(n, dtype, ctx)
    info = lk.gmres(op, lk.dense_vector_gpu.from_array(b, ctx), x, rtol=1e-10, transpose=True,
                    options=lk.gmres_dp_opts(kdim=40, maxiter=5))
    assert info > 0
    assert np.linalg.norm(AH @ x.to_array() - b) <= 1e-9 * np.linalg.norm(b)


def test_lazy_pending_work_survives_the_destruction_of_a_view_handle():
    """A basis VIEW (lk_basis_wrap) is a handle on memory that lives on: destroying the handle while a virtual
    linear combination targets one of its columns must write it out, not drop it."""
    n, k = 20_011, 5
    c = lk.Context(device=0)
    c.set_tuning("lazy", 1)
    B = lk.krylov_basis_gpu(n, k + 3, np.float64, c)
    for j in range(k + 3):
        B[j].rand(False, seed=70 + j)
    Xh = B.download()
    V = B[k + 1:]                                  # columns k+1, k+2 through a wrapped handle
    T = V[0]
    T.zero()
    for i in range(k):
        T.axpby(0.5 + i, B[i], 1.0)
    del T, V                                       # the view handle goes away; column k+1 of B does not
    import gc; gc.collect()
    want = Xh[:, :k] @ (0.5 + np.arange(k))
    assert np.abs(B.download(k + 1, 1)[:, 0] - want).max() <= 1e-13 * np.abs(want).max()
    c.close()
