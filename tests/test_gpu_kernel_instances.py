"""Kernel instances and tuning-key settings the rest of the suite never dispatched (tests/kernel_instances.txt), each against a plain
extended-precision reference of the same operation (numpy longdouble / clongdouble products over the same host data).

Products and dots are checked ENTRY BY ENTRY against the deterministic a-priori bound of a length-m sum in any order:
    real:     |got - ref|_ij <= gamma_m (|X|^T |Y|)_ij,                         gamma_m = m u / (1 - m u), u = 2^-53
    complex:  |Re|, |Im| of (got - ref)_ij <= 2 gamma_(2m+5) ((|Xr|+|Xi|)^T (|Yr|+|Yi|))_ij
(gamma_m also carries the same term at u = 2^-64 for the rounding of the longdouble reference; the complex bound covers the
four-product form -- each part a real sum of 2m products -- and the three-product one, whose imaginary part P3 - P1 - P2 sums
three products of up to that scale).  A dropped or doubled row tile, a wrong column, a single-precision partial
or a stale LDS buffer is many orders of magnitude beyond it.  The measured worst ratio goes to $LK_TOL_REPORT.  Keys marked [bits] in
include/lightkrylov_hip.h are compared bit for bit with the default; the others against the reference over their whole domain."""
import contextlib

import numpy as np
import pytest

import lightkrylov_amd as lk
from tests._gpu_helpers import KINDS, basis, check_entrywise, ext, is_cplx, orthonormal_basis, product_scale, seeded
from tests._tol import _report

pytestmark = pytest.mark.gpu

DEFAULTS = dict(grid_mult=2, blas1_grid_mult=2, cw_u=0, cw_grid_mult=3, dot_colwise=1, xhy_db=1, gram_rs=1, gemm_3m=1, gemm_roll=1,
                gemm_mfma_min=0, store_policy=2, store_split=0, recompute_update=1, pool_slab_cols=160, csr_stream=1, wide_s3=1,
                wide_regs=2, async_arnoldi=1)


def check_xhy(got, X, Y, label):
    """got = X^H Y (k x p) against the longdouble product, inner length n = rows of X"""
    ref = ext(X).conj().T @ ext(Y)
    check_entrywise(got, ref, product_scale(X.conj().T, Y), X.shape[0], np.iscomplexobj(X), label)


@pytest.fixture(scope="module")
def kctx():
    c = lk.Context(device=0)
    yield c
    c.close()


@contextlib.contextmanager
def tuned(c, **keys):
    """set keys; restore the defaults of every key this module touches on the way out"""
    try:
        for k, v in keys.items():
            c.set_tuning(k, v)
        yield c
    finally:
        for k in keys:
            c.set_tuning(k, DEFAULTS[k])


def gpu_basis(c, A):
    B = lk.krylov_basis_gpu(A.shape[0], A.shape[1], A.dtype, c)
    B.upload(np.asfortranarray(A))
    return B


# ---- CSR: every lanes-per-row width -----------------------------------------------------------------------------------------------

def _csr_with_mean_row_length(n, m, dtype, rng):
    """n x n CSR whose rows have mean length exactly m (so the engine picks the lanes per row from m), ragged: row 0 empty, row 1 of
    length 2m, the rest in pairs m - d, m + d"""
    import scipy.sparse as sp
    L = np.full(n, m, dtype=np.int64)
    for i in range(2, n - 1, 2):
        d = int(rng.integers(0, m + 1))
        L[i] -= d
        L[i + 1] += d
    L[0], L[1] = 0, 2 * m
    indptr = np.concatenate([[0], np.cumsum(L)])
    indices = np.concatenate([np.sort(rng.choice(n, int(l), replace=False)) for l in L]).astype(np.int32)
    vals = rng.standard_normal(indptr[-1]) + (1j * rng.standard_normal(indptr[-1]) if is_cplx(dtype) else 0)
    return sp.csr_matrix((vals.astype(dtype), indices, indptr), shape=(n, n))


def _check_csr(y, A, x, label):
    """row i: a sum of nnz_i products"""
    A = A.tocsr()
    xe, ve = ext(x), ext(A.data)
    ref = np.array([(ve[A.indptr[i]:A.indptr[i + 1]] * xe[A.indices[A.indptr[i]:A.indptr[i + 1]]]).sum() for i in range(A.shape[0])],
                   dtype=xe.dtype if is_cplx(A.dtype) else ve.dtype)
    absA = A.copy()
    if is_cplx(A.dtype):
        absA.data = np.abs(A.data.real) + np.abs(A.data.imag)
        scale = absA @ (np.abs(x.real) + np.abs(x.imag))
    else:
        absA.data = np.abs(A.data)
        scale = absA @ np.abs(x)
    check_entrywise(y, ref, scale, np.diff(A.indptr), is_cplx(A.dtype), label)


@pytest.mark.parametrize("dtype", KINDS)
def test_csr_lanes_per_row_kernel_at_every_width(kctx, dtype):
    """k_csr<CPLX, W> for W = 1 .. 64 lanes per row: the engine doubles W from 1 while 2W <= mean / 2 (up to 64), so a mean row length
    of 3W (ragged, an empty row, a row twice the mean) selects each width in turn, with the LDS-streaming
    kernel switched off ("csr_stream" = 0); y = A x and y = A^H x row by row against the longdouble sums."""
    rng = np.random.default_rng(11)
    n = 1031
    with tuned(kctx, csr_stream=0):
        for W in (1, 2, 4, 8, 16, 32, 64):
            A = _csr_with_mean_row_length(n, 3 * W, dtype, rng)
            op = lk.csr_linop_gpu(A, kctx)
            xh = seeded(n, dtype, 40 + W)
            x = lk.dense_vector_gpu.from_array(xh, kctx)
            y = lk.dense_vector_gpu(n, dtype, kctx)
            op.apply_matvec(x, y)
            _check_csr(y.to_array(), A, xh, f"k_csr W={W} {np.dtype(dtype).name} A x")
            op.apply_rmatvec(x, y)
            _check_csr(y.to_array(), A.conj().T.tocsr(), xh, f"k_csr W={W} {np.dtype(dtype).name} A^H x")
            del op, x, y


# ---- tall-skinny product on the matrix cores: the rolling ring at every group count -----------------------------------------------

@pytest.mark.parametrize("dtype", KINDS)
def test_product_on_the_rolling_ring_at_every_group_count(kctx, dtype):
    """panel_gemm_mfma<CPLX, NG, false, true> for NG = 1, 2, 4 (both kinds, four real products per complex one: "gemm_3m" = 0) and the
    complex NG = 8 that has no ring: Y = X C with k = 64 and 128 (the widths the ring is unrolled for), "gemm_mfma_min" = 1 so that
    the narrowest group reaches the matrix cores, "gemm_roll" = 2; every entry against the longdouble product, and "gemm_roll"
    ([bits]) 0 / 1 / 2 bit-identical."""
    cp = is_cplx(dtype)
    n = 2051 if cp else 4099                                # ragged: 8 / 9 tiles of 256 / 512 rows
    qs = (5, 12, 30, 50) if cp else (3, 20, 40)             # 8 (complex) / 16 (real) outputs per group
    for k in (64, 128):
        Xh = basis(n, k, dtype, 300 + k)
        B = gpu_basis(kctx, Xh)
        for q in qs:
            Cm = basis(k, q, dtype, 900 + q)
            ref = ext(Xh) @ ext(Cm)
            scale = product_scale(Xh, Cm)
            outs = []
            for roll in (2, 1, 0):
                with tuned(kctx, gemm_3m=0, gemm_mfma_min=1, gemm_roll=roll):
                    Y = lk.linear_combination(B, Cm)
                    outs.append(Y.download())
                    del Y
            check_entrywise(outs[0], ref, scale, k, cp, f"panel_gemm_mfma ring k={k} q={q} {np.dtype(dtype).name}")
            assert all(o.tobytes() == outs[0].tobytes() for o in outs[1:]), (k, q)
        del B


# ---- X^H Y on the matrix cores: every double-buffer setting ----------------------------------------------------------------------

@pytest.mark.parametrize("dtype", KINDS)
def test_xhy_on_the_matrix_cores_at_every_double_buffer_setting(kctx, dtype):
    """innerprod(X, Y) with 5..32 (32-row tiles) and 33..64 right-hand sides for "xhy_db" = 0, 1, 2 (2: the 32-row variants
    double-buffered too, panel_xhy_mfma<CPLX, 2, 32, true>), the complex kind with four and with three real products per complex one;
    k = 40 columns (three 16-column blocks, the last ragged), n ragged around the 32-row tile."""
    cp = is_cplx(dtype)
    k = 40
    for n in (1, 31, 3001):
        Xh = basis(n, k, dtype, 500)
        Bx = gpu_basis(kctx, Xh)
        for p in (5, 32, 48):
            Yh = basis(n, p, dtype, 600 + p)
            By = gpu_basis(kctx, Yh)
            for three in ((0, 1) if cp else (1,)):
                for db in (0, 1, 2):
                    with tuned(kctx, xhy_db=db, gemm_3m=three):
                        M = lk.innerprod(Bx, By)
                    check_xhy(M, Xh, Yh, f"panel_xhy_mfma n={n} p={p} xhy_db={db} 3m={three} {np.dtype(dtype).name}")
            del By
        del Bx


# ---- Gram matrix: every row-split setting ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", KINDS)
def test_gram_at_every_row_split_setting(kctx, dtype):
    """Gram(X) for "gram_rs" = 0 (panel_xhy_mfma / panel_gram_mfma3m, the 32-row complex one double-buffered with "xhy_db" = 2 too),
    1 (the resident blocks per CU), 2 and 16 (more blocks than the 70001-row panel has 16- / 32-row tiles: the grid is capped at the
    tile count); upper triangle entrywise against the longdouble X^H X (the lower one is the mirror, AbstractVectors.fypp:645-657)."""
    cp = is_cplx(dtype)
    for n, k in ((70_001, 16), (1000, 40), (33, 100)):
        Xh = basis(n, k, dtype, 700 + k)
        B = gpu_basis(kctx, Xh)
        ref = ext(Xh).conj().T @ ext(Xh)
        scale = product_scale(Xh.conj().T, Xh)
        iu = np.triu_indices(k)
        for rs in (0, 1, 2, 16):
            for db in ((1, 2) if rs == 0 else (1,)):
                with tuned(kctx, gram_rs=rs, xhy_db=db):
                    G = lk.Gram(B)
                check_entrywise(G[iu], ref[iu], scale[iu], n, cp, f"gram n={n} k={k} gram_rs={rs} xhy_db={db} {np.dtype(dtype).name}")
                assert np.array_equal(G, np.triu(G) + np.triu(G, 1).T)
        del B


# ---- sweeps: grid multipliers and the column-at-a-time dot -----------------------------------------------------------------------

@pytest.mark.parametrize("dtype", KINDS)
def test_sweep_dots_over_the_whole_grid_and_load_domain(kctx, dtype):
    """h = X^H y by the all-columns sweep (panel_sweep<DOT>, "dot_colwise" = 0) for "grid_mult" = 1, 2, 16 -- k = 8 and k = 200 (the
    lane-split dot-only sweep, panel_sweep<CPLX, 16, 8, false, true, false, 2, 1>) -- and by the column-at-a-time kernel (panel_dot_cw)
    for "cw_u" = 0, 4, 8 x "cw_grid_mult" = 1, 3, 16; one row, tiles +- 1 row, and a panel of several tiles per block at
    "grid_mult" = 1; every coefficient against the longdouble sum over the n rows."""
    cp = is_cplx(dtype)
    for n in (1, 1023, 1025, 100_003):
        for k in (8, 200):
            A = basis(n, k + 1, dtype, 1000 + k)
            B = gpu_basis(kctx, A)
            ref = ext(A[:, :k]).conj().T @ ext(A[:, k])
            scale = product_scale(A[:, :k].conj().T, A[:, k])
            for gm in (1, 2, 16):
                with tuned(kctx, dot_colwise=0, grid_mult=gm):
                    h = np.asarray(lk.innerprod(B[:k], B[k]))
                check_entrywise(h, ref, scale, n, cp, f"panel_sweep dot n={n} k={k} grid_mult={gm} {np.dtype(dtype).name}")
            for u in (0, 4, 8):
                for cgm in (1, 3, 16):
                    with tuned(kctx, dot_colwise=1, cw_u=u, cw_grid_mult=cgm):
                        h = np.asarray(lk.innerprod(B[:k], B[k]))
                    check_entrywise(h, ref, scale, n, cp, f"panel_dot_cw n={n} k={k} cw_u={u} cw_grid_mult={cgm} {np.dtype(dtype).name}")
            del B


@pytest.mark.parametrize("dtype", KINDS)
def test_gram_schmidt_step_over_the_grid_multiplier_domain(kctx, dtype):
    """double_gram_schmidt_step for "grid_mult" = 1, 2, 5, 16 (sweep 3 takes it; 16 puts more blocks than tiles on the short panel):
    the algorithm whose schedule the oracle defines, so beta and y against the oracle's step as the rest of the suite does (normwise
    1e-12 of |y|), on a long panel (several tiles per block at "grid_mult" = 1) and a short one."""
    from oracle import oracle as ora
    for n, k in ((50_003, 24), (700, 24)):
        Q = orthonormal_basis(n, k, dtype, 70)
        y0 = seeded(n, dtype, 71)
        yo = y0.copy()
        ho, _ = ora.double_gram_schmidt_step(yo, Q)
        B = lk.krylov_basis_gpu(n, k + 1, dtype, kctx)
        for gm in (1, 2, 5, 16):
            B.upload(Q); B.upload(y0.reshape(-1, 1), k)
            h = np.zeros(k, dtype=dtype)
            with tuned(kctx, grid_mult=gm):
                assert lk.double_gram_schmidt_step(B[k], B[:k], False, h) == 0
            yg = B.download(k, 1)[:, 0]
            err = max(np.abs(h - ho).max(), np.abs(yg - yo).max()) / np.linalg.norm(y0)
            _report(f"dgs n={n} k={k} grid_mult={gm} {np.dtype(dtype).name}", err, 1e-12, "normwise vs oracle")
            assert err <= 1e-12, (n, gm, err)
        del B


# ---- BLAS-1 grid multiplier -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", KINDS)
def test_blas1_over_the_grid_multiplier_domain(kctx, dtype):
    """"blas1_grid_mult" = 1, 2, 13, 64 (64: more blocks than the partial buffer holds at 2.1e6 rows -- the dot caps its grid at it):
    the dot (k_dot) against the longdouble sum; axpby, scal and the counter-based rand are elementwise, so bit-identical across the
    domain."""
    cp = is_cplx(dtype)
    for n in (1, 257, 2_100_001):
        xh, yh = seeded(n, dtype, 81), seeded(n, dtype, 82)
        ref = np.array([(ext(xh).conj() * ext(yh)).sum()])
        scale = product_scale(xh.conj().reshape(1, -1), yh.reshape(-1, 1))[0]
        B = lk.krylov_basis_gpu(n, 4, dtype, kctx)
        outs = []
        for bm in (2, 1, 13, 64):
            B.upload(np.asfortranarray(np.stack([xh, yh], axis=1)))
            with tuned(kctx, blas1_grid_mult=bm):
                d = B[0].dot(B[1])
                B[1].axpby(0.75 - (0.5j if cp else 0), B[0], 1.25)
                B[0].scal(-3.0)
                B[2].rand(False, seed=5)
            check_entrywise(np.array([d]), ref, np.array([scale]), n, cp, f"k_dot n={n} blas1_grid_mult={bm} {np.dtype(dtype).name}")
            outs.append(B.download(0, 3))
        assert all(o.tobytes() == outs[0].tobytes() for o in outs[1:]), n
        del B


# ---- [bits] keys ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", KINDS)
def test_bits_keys_change_no_bit(kctx, dtype):
    """The keys include/lightkrylov_hip.h marks [bits], each over its domain against the default: "store_policy" 0..3, "store_split",
    "recompute_update" and "wide_s3" on a Gram-Schmidt step (k = 150, lane-split shape with "wide_regs" = 0 for "wide_s3"),
    "async_arnoldi" on an Arnoldi factorisation, "pool_slab_cols" 2 / 4096 on pool vectors."""
    n, k = 30_011, 150
    Q = orthonormal_basis(n, k, dtype, 90)
    y0 = seeded(n, dtype, 91)
    B = lk.krylov_basis_gpu(n, k + 1, dtype, kctx)

    def dgs(**keys):
        B.upload(Q); B.upload(y0.reshape(-1, 1), k)
        h = np.zeros(k, dtype=dtype)
        with tuned(kctx, **keys):
            lk.double_gram_schmidt_step(B[k], B[:k], False, h)
        return h.tobytes() + B.download(k, 1).tobytes()

    base = dgs()
    for keys in [dict(store_policy=v) for v in (0, 1, 3)] + [dict(store_split=1)]:
        assert dgs(**keys) == base, keys
    assert dgs(wide_regs=0, wide_s3=0) == dgs(wide_regs=0, wide_s3=1)
    # "recompute_update" = 0 stores y' and runs sweep 3 as y' - X h2 on the streaming update kernel, whose sum over the columns runs
    # in another order than the re-forming sweep's: beta is the same bits, y'' agrees within the bound of its 2k + 1 terms
    # (|y| + |X| (|h1| + |h2|), h2 = O(u |y|) on an orthonormal X) -- the key is not [bits]
    other = dgs(recompute_update=0)
    hb = k * np.dtype(dtype).itemsize
    assert other[:hb] == base[:hb]
    beta = np.frombuffer(base[:hb], dtype=dtype)
    y1, y0s = np.frombuffer(base[hb:], dtype=dtype), np.frombuffer(other[hb:], dtype=dtype)
    scale = np.abs(y0.real) + np.abs(y0.imag) + 2.0 * product_scale(Q, beta.reshape(-1, 1))[:, 0]
    check_entrywise(y0s, ext(y1), 2.0 * scale, 2 * k + 1, is_cplx(dtype), f"recompute_update 0 vs 1 k={k} {np.dtype(dtype).name}")
    del B

    m = 12
    d = 1.0 + np.arange(2001) / 2001.0
    x0 = seeded(2001, dtype, 92)
    x0 /= np.linalg.norm(x0)
    res = []
    for a in (1, 0):
        with tuned(kctx, async_arnoldi=a):
            X = lk.krylov_basis_gpu(2001, m + 1, dtype, kctx)
            X.upload(x0.reshape(-1, 1), 0)
            H = np.zeros((m + 1, m), dtype=dtype, order="F")
            assert lk.arnoldi(lk.diag_linop_gpu(d.astype(dtype), kctx), X, H) == 0
            res.append(H.tobytes() + X.download().tobytes())
            del X
    assert res[0] == res[1]

    res = []
    for cols in (160, 2, 4096):
        with tuned(kctx, pool_slab_cols=cols):
            v = [lk.dense_vector_gpu.from_array(seeded(10_007, dtype, 93 + i), kctx) for i in range(3)]
            v[0].axpby(0.5, v[1], 2.0)
            v[2].scal(1.5)
            r = [v[0].dot(v[1]), v[2].norm()]
            res.append(np.array(r).tobytes() + b"".join(w.to_array().tobytes() for w in v))
            del v
    assert res[1] == res[0] and res[2] == res[0]
