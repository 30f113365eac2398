"""Every panel kernel on columns more than 4 GB apart: address arithmetic that is only right while offsets fit in 32 bits.

lk_basis_wrap takes any ld >= n_local and promises that rows [n_local, ld) are never read or written, so a panel of a few thousand rows
whose columns lie 2^28 (geometry A) or 2^26 bytes (geometry B) apart moves megabytes while its columns reach beyond every limit of
narrowed address arithmetic (tests/_gpu_helpers.py, FarPanel, has the arithmetic):

                           > 2^32 bytes      > 2^31 doubles     > 2^32 doubles     from the panel base
  geometry A, from column      16                 64                 128            (176 columns, 44 GiB of address space)
  geometry B, from column      64                256                 512            (513 columns, 32.06 GiB)

Every case is checked three ways:
  1. against the independent reference the suite uses for that operation: products, dots and operators entry by entry against the
     longdouble result within the a-priori bound stated at the top of tests/test_gpu_kernel_instances.py (check_entrywise; the worst
     ratio goes to $LK_TOL_REPORT), Gram-Schmidt steps and factorisations against the oracle at the suite's normwise 1e-12 (1e-13
     for orthogonality);
  2. bit for bit against the same call, in the same context with the same tuning keys, on an engine-made panel (lk_basis_create) of the
     same n and data: the arithmetic of a kernel must not depend on ld (no dispatch decision of lk_engine.hip reads ld: it is only
     ever handed to the kernels; the base is 256-byte aligned and ld a multiple of 32 elements, as on an engine-made panel);
  3. every column the call must not write, and both 4 KB guard bands of every column, bit for bit with what was set: a store whose
     offset wrapped modulo 2^32 bytes or doubles lands on the same row of a lower column.

Kernel family -> the case that dispatches it, and the furthest limit its IN-KERNEL offsets cross (an operand that starts at column 128 or 175
reaches its kernel as a pointer the host formed, B->col(j) in 64 bits: that tests the host side beyond 2^31 and 2^32 doubles, the kernel's own
offsets from it stay small):
  hipMemcpy2DAsync of lk_basis_upload / _download     test_upload_download          host: columns 14.. | 62.. | 126.. straddle all three limits
  k_zero / k_rand / k_scal / k_copy / k_axpby / k_dot test_blas1                    host pointers only (columns 17 | 65 | 129, 175)
  panel_sweep, panel_dot_cw, panel_update             test_three_sweep_step         X columns 0..127 in kernel: 2^32 B and 2^31 doubles; y by host pointer
  the fused row operator inside the sweeps            test_factorisations           column k-1 of X, k up to 72: 2^32 B and 2^31 doubles
  dgs_onchip, dgs_resident                            test_single_launch_step       X columns 0..127: 2^32 B and 2^31 doubles
  panel_dot_p, panel_sweep_p                          test_multi_rhs_sweeps         X 0..127: 2^32 B, 2^31 doubles; Y: 4 columns from a host pointer
  panel_xhy_mfma, panel_xhy_mfma3m, finish_xhy        test_xhy_on_the_matrix_cores  X 0..127: 2^32 B, 2^31 doubles; Y: 48 columns from column 128, 2^32 B
  panel_gram_rs, _rs3m, _rs3m4, panel_gram_mfma3m     test_gram                     X 0..127 (LDS-DMA sources): 2^32 B and 2^31 doubles, never 2^32 doubles
  panel_gemm, panel_gemm_mfma (ring and batch),
    panel_gemm_mfma3m, pack_coef*                     test_tall_skinny_product      X 0..127: 2^32 B, 2^31 doubles; output: 40 columns from column 128, 2^32 B
  panel_xhy_upd_mfma, panel_xhy_upd_rs                test_fused_block_pass         X 0..127: 2^32 B, 2^31 doubles; Y: 32 columns from column 128, 2^32 B
  lane-split panel_sweep (SC = 2, 4; G = 2)           test_lane_split_sweeps        geometry B, X 0..511 in kernel: 2^32 B (k = 129) | 2^31 doubles (385) |
                                                                                    column 511 ends 2^26 B short of 2^32 doubles; y in column 512 by host pointer
  k_gemv_n, k_gemv_h                                  test_dense_operator_far_lda   columns 0..95 in kernel at lda = 2^28 B: 2^32 B and 2^31 doubles
So beyond 2^32 doubles only the host-side pointer arithmetic (B->col(j), hipMemcpy2DAsync) is exercised: no kernel takes more than 512 columns
from one base, and geometry A's 2^28-byte stride puts 2^32 doubles at column 128, where every kernel's k ends.

Tiles per block.  n = 4099 is one tile per block for every kernel whose grid is capped by the CU count.  The kernels that keep state across the
tiles of a block have a case of their own whose n exceeds tile rows x grid cap (the cap from the context's CU count): the rolling rings of
panel_gemm_mfma (real) and panel_gemm_mfma3m (complex) with their prefetch into the block's next tile
(test_ring_across_the_tiles_of_a_block, n = 2 x 512 | 256 x 4 CUs + 3), the double-buffered
panel_xhy_mfma (test_xhy_on_the_matrix_cores, n = 70 001 real / 20 001 complex), the row-split Gram kernels and panel_gram_mfma3m (test_gram),
panel_xhy_upd_mfma and panel_xhy_upd_rs (test_fused_block_pass, n = 70 001 real / 20 001 complex).  The sweeps form every address from
the tile index (no offset runs from tile to tile), and tests/test_gpu_fullsize.py runs them with many tiles per block."""
import ctypes as C

import numpy as np
import pytest

import lightkrylov_amd as lk
from lightkrylov_amd import _capi
from oracle import oracle as ora
from tests._blas1_cases import check_axpby, check_scal, rand_reference
from tests._gpu_helpers import (FAR_COLS_A, FAR_COLS_B, FAR_STRIDE_A, FAR_STRIDE_B, KINDS, FarPanel, basis, check_entrywise, ext, is_cplx,
                                orthonormal_basis, product_scale, seeded)
from tests._tol import _report, assert_columns_close

pytestmark = pytest.mark.gpu

_DP = C.POINTER(C.c_double)
NA = 4099                                         # eight full 512-row tiles (sixteen of 256 rows) and a ragged one: one tile per block


def _name(dtype):
    return np.dtype(dtype).name


def assert_several_tiles(n, tile_rows, blocks_per_cu, what):
    """a condition on the SHAPE of a case: on this device's CU count every block of a grid capped at blocks_per_cu x CUs takes two tiles of
    tile_rows rows or more"""
    import torch
    cus = torch.cuda.get_device_properties(tuned().device).multi_processor_count
    assert n // tile_rows >= 2 * blocks_per_cu * cus, f"{what}: {n // tile_rows} full tiles for {blocks_per_cu * cus} blocks: one tile per block"


class _Arena:
    """the one backing buffer alive at a time: asking for another size releases the previous one first"""

    def __init__(self, device):
        self.buf, self.device = None, device

    def get(self, nbytes):
        import torch
        if self.buf is not None and self.buf.numel() == nbytes:
            return self.buf
        self.buf = None
        torch.cuda.empty_cache()
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=f"cuda:{self.device}")
        return self.buf


_CTXS = {}


def tuned(**kw):
    """one context per tuning set for the whole module (closed at its end)"""
    key = tuple(sorted(kw.items()))
    if key not in _CTXS:
        c = lk.Context(device=0)
        for k, v in key:
            c.set_tuning(k, v)
        _CTXS[key] = c
    return _CTXS[key]


@pytest.fixture(scope="module")
def arena():
    """the module skips as a whole, before anything is allocated, when the largest backing buffer (geometry A) + 8 GiB is not free"""
    import torch
    dev = tuned().device
    free, _total = torch.cuda.mem_get_info(dev)
    print(f"far columns: {free / 2 ** 30:.1f} GiB of device memory free at the start")
    need = FAR_COLS_A * FAR_STRIDE_A + (8 << 30)
    if free < need:
        pytest.skip(f"{free / 2 ** 30:.1f} GiB of device memory free, the far-column panels need {need / 2 ** 30:.1f} GiB")
    a = _Arena(dev)
    yield a
    for c in _CTXS.values():
        c.close()
    _CTXS.clear()
    a.buf = None
    torch.cuda.empty_cache()


def far_a(arena, dtype, n=NA, ncols=FAR_COLS_A):
    return FarPanel(tuned(), dtype, n, ncols, FAR_STRIDE_A, backing=arena.get(FAR_COLS_A * FAR_STRIDE_A))


def wrap(P, c, ncols=None):
    """the far panel's memory (its first ncols columns) as a basis of context c"""
    h = C.c_void_p()
    _capi.check(_capi.load().lk_basis_wrap(c._h, _capi.LK_C128 if is_cplx(P.dtype) else _capi.LK_F64, P.n, ncols or P.ncols, P.ld,
                                           C.c_void_p(P.backing.data_ptr()), C.byref(h)))
    return lk.krylov_basis_gpu(P.n, ncols or P.ncols, P.dtype, c, _handle=h, _owner=P.backing)


def both(P, c, init, call, written, what, ncols=None):
    """set `init` ({first column: data}, or pairs in order), run call(B) -> tuple of host arrays on the far panel and on an engine-made panel with the same
    contents; checks 2 and 3 of the module docstring.  Returns (host results, all columns of the far panel)."""
    for col0, A in (init.items() if isinstance(init, dict) else init):
        P.set(A, col0)
    nc = ncols or P.ncols
    Bf = wrap(P, c, nc)
    rf = call(Bf)
    got = P.get(what)
    P.assert_untouched(got, written, what)
    Be = lk.krylov_basis_gpu(P.n, nc, P.dtype, c)
    Be.upload(P.shadow[:, :nc])
    re = call(Be)
    ge = Be.download()
    for i, (a, b) in enumerate(zip(rf, re)):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), f"{what}: host result {i} differs from the engine-made panel's"
    w = list(written)
    if w:
        assert got[:, w].tobytes() == ge[:, w].tobytes(), f"{what}: written columns differ from the engine-made panel's"
        P.shadow[:, w] = got[:, w]                                  # (what the panel holds from here on)
    del Bf, Be
    return rf, got


def check_xhy(got, X, Y, label):
    ref = ext(X).conj().T @ ext(Y)
    return check_entrywise(np.asarray(got).reshape(ref.shape, order="F"), ref, product_scale(X.conj().T, Y), X.shape[0], np.iscomplexobj(X), label)


def check_step(h, y, Q, y0, label, orth=True):
    """beta and y'' of a two-pass step against the oracle, normwise 1e-12 of |y|; Q^H y'' at 1e-13"""
    yo = y0.copy()
    ho, _ = ora.double_gram_schmidt_step(yo, np.asfortranarray(Q))
    ny = np.linalg.norm(y0)
    err = max(np.abs(h - ho).max(), np.abs(y - yo).max()) / ny
    _report(label, err, 1e-12, "normwise vs oracle")
    assert err <= 1e-12, (label, err)
    if orth:
        o = np.abs(Q.conj().T @ y).max() / ny
        assert o <= 1e-13, (label, o)


# ---- upload / download ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", KINDS)
def test_upload_download(arena, dtype):
    """lk_basis_upload / lk_basis_download (hipMemcpy2DAsync with the panel's 256 MB pitch) of 4 columns starting at columns 14, 62 and
    126: each range straddles a limit.  Against the torch strided copy, bit for bit."""
    P = far_a(arena, dtype)
    for col0 in (14, 62, 126):
        A = basis(NA, 4, dtype, 10 + col0)
        P.B.upload(A, col0)
        P.shadow[:, col0:col0 + 4] = A
        got = P.get(f"upload at {col0}")
        assert got[:, col0:col0 + 4].tobytes() == A.tobytes(), col0
        P.assert_untouched(got, range(col0, col0 + 4), f"upload at {col0}")
        D = basis(NA, 4, dtype, 20 + col0)
        P.set(D, col0)
        assert P.B.download(col0, 4).tobytes() == D.tobytes(), col0


# ---- BLAS-1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", KINDS)
def test_blas1(arena, dtype):
    """k_zero, k_rand, k_scal, k_copy, k_axpby, k_dot + finish_partials with operands in columns 3, 17, 65, 129 and 175 (n = 1031):
    across and within the limits.  scal / axpby with the checks of tests/_blas1_cases.py, rand against the header's formula, dot and
    norm against the longdouble sums."""
    n, cols = 1031, (3, 17, 65, 129, 175)
    cp = is_cplx(dtype)
    P = far_a(arena, dtype, n)
    X = basis(n, 5, dtype, 300)
    a, b = (0.75 - 0.5j, -1.25 + 0.3j) if cp else (0.75, -1.25)
    c = tuned()

    def call(B):
        v = [B[j] for j in cols]
        d = [v[0].dot(v[3]), v[2].dot(v[4]), v[4].norm(), v[1].norm()]
        v[4].axpby(a, v[0], b)                    # 175 <- a 3 + b 175
        v[1].scal(a)                              # 17
        lk.copy(v[2], v[3])                       # 65 <- 129
        v[3].rand(False, seed=77)                 # 129
        v[0].zero()                               # 3
        return (np.array(d),)

    (d,), got = both(P, c, {j: X[:, i] for i, j in enumerate(cols)}, call, cols, f"blas1 {_name(dtype)}")
    x3, x17, x65, x129, x175 = (X[:, i] for i in range(5))
    lab = f"far blas1 {_name(dtype)}"
    for val, (u, v) in zip(d[:2], ((x3, x129), (x65, x175))):
        check_entrywise(np.array([val]), np.array([(ext(u).conj() * ext(v)).sum()]), product_scale(u.conj().reshape(1, -1), v.reshape(-1, 1))[0],
                        n, cp, lab + " k_dot")
    for val, u in zip(d[2:], (x175, x17)):
        ref = np.sqrt((ext(u).conj() * ext(u)).sum().real)
        err, bound = abs(val.real - float(ref)), (n + 2) * 2.0 ** -53 * float(ref)          # gamma_n on the sum of squares, halved by the root, + its rounding
        _report(lab + " norm", err, bound, "gamma bound of the sum of squares")
        assert err <= bound, lab
    check_axpby(got[:, 175], a, x3, b, x175, lab + " k_axpby")
    check_scal(got[:, 17], x17, a, lab + " k_scal")
    assert got[:, 65].tobytes() == x129.tobytes()
    assert got[:, 129].tobytes() == rand_reference(n, dtype, 77, 0).astype(dtype).tobytes()
    assert not got[:, 3].view(np.uint64).any()


# ---- the three-sweep step ---------------------------------------------------------------------------------------------------------------
SWEEP_KEYS = [dict(dot_colwise=0), dict(dot_colwise=1), dict(dot_colwise=1, recompute_update=0), dict(dot_colwise=0, store_policy=0),
              dict(dot_colwise=1, recompute_update=0, store_policy=0)]


@pytest.mark.parametrize("dtype", KINDS)
def test_three_sweep_step(arena, dtype):
    """lk_dgs on the three-sweep schedule ("resident" = 0): panel_sweep<DOT> ("dot_colwise" = 0) or panel_dot_cw (1), panel_sweep<UPDATE + DOT>,
    the re-forming two-coefficient sweep ("recompute_update" = 1) or panel_update (0), stores with "store_policy" 2 and 0; k = 16, 17, 65, 128
    with y in column k, and k = 128 with y in column 175.  Also lk_orthogonalize (one pass) and lk_dgs with LK_DGS_NORMALIZE."""
    P = far_a(arena, dtype)
    lib = _capi.load()
    for k, jy in ((16, 16), (17, 17), (65, 65), (128, 128), (128, 175)):
        Q = orthonormal_basis(NA, k, dtype, 40 + k)
        y0 = seeded(NA, dtype, 5000 + k)
        for keys in SWEEP_KEYS if k in (17, 128) else SWEEP_KEYS[:2]:
            c = tuned(resident=0, **keys)

            def call(B):
                h = np.zeros(k, dtype=dtype)
                assert lk.double_gram_schmidt_step(B[jy], B[:k], False, h) == 0
                return (h,)

            what = f"dgs 3 sweeps k={k} y@{jy} {keys} {_name(dtype)}"
            (h,), got = both(P, c, {0: Q, jy: y0}, call, [jy], what)
            check_step(h, got[:, jy], Q, y0, what)
    k, jy = 128, 175
    Q, y0 = orthonormal_basis(NA, k, dtype, 40 + k), seeded(NA, dtype, 5000 + k)
    c = tuned(resident=0)

    def one_pass(B):
        h, info = np.zeros(k, dtype=dtype), C.c_int()
        _capi.check(lib.lk_orthogonalize(B._h, k, B._h, jy, h.ctypes.data_as(_DP), C.byref(info)))
        return (h,)

    (h,), got = both(P, c, {0: Q, jy: y0}, one_pass, [jy], f"orthogonalize {_name(dtype)}")
    check_xhy(h, Q, y0.reshape(-1, 1), f"far lk_orthogonalize h k={k} {_name(dtype)}")
    ref = ext(y0) - ext(Q) @ ext(h)
    scale = np.abs(y0.real) + np.abs(y0.imag) + product_scale(Q, h.reshape(-1, 1))[:, 0]
    check_entrywise(got[:, jy], ref, scale, k + 1, is_cplx(dtype), f"far lk_orthogonalize y k={k} {_name(dtype)}")

    def normalised(B):
        h, norms, info = np.zeros(k, dtype=dtype), (C.c_double * 3)(), C.c_int()
        _capi.check(lib.lk_dgs(B._h, k, B._h, jy, h.ctypes.data_as(_DP), norms, _capi.LK_DGS_NORMALIZE, C.byref(info)))
        return h, np.array(list(norms))

    (h, norms), got = both(P, c, {0: Q, jy: y0}, normalised, [jy], f"dgs normalize {_name(dtype)}")
    check_step(h, got[:, jy] * norms[2], Q, y0, f"far lk_dgs normalize k={k} {_name(dtype)}")
    assert abs(np.linalg.norm(got[:, jy]) - 1.0) <= 1e-12


# ---- the single launch ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("onchip", [1, 0])
@pytest.mark.parametrize("dtype", KINDS)
def test_single_launch_step(arena, dtype, onchip):
    """lk_dgs as ONE launch ("resident" = 1; resident_would_apply sizes the panel by n, not ld): dgs_onchip ("resident_onchip" = 1) and
    dgs_resident (0), k = 64 and 128 with y in column k; lk_resident_stats shows that the launch ran and did not give up."""
    P = far_a(arena, dtype)
    c = tuned(resident=1, resident_onchip=onchip)
    for k in (64, 128):
        Q, y0 = orthonormal_basis(NA, k, dtype, 40 + k), seeded(NA, dtype, 5000 + k)
        before = c.resident_stats()

        def call(B):
            h = np.zeros(k, dtype=dtype)
            assert lk.double_gram_schmidt_step(B[k], B[:k], False, h) == 0
            return (h,)

        what = f"dgs single launch onchip={onchip} k={k} {_name(dtype)}"
        (h,), got = both(P, c, {0: Q, k: y0}, call, [k], what)
        after = c.resident_stats()
        assert after[0] - before[0] == 2 and after[1] == before[1], (before, after)          # (the far and the engine-made panel)
        assert (after[2] - before[2] == 2) == bool(onchip), (before, after)
        check_step(h, got[:, k], Q, y0, what)


# ---- multi-right-hand-side sweeps ---------------------------------------------------------------------------------------------------------
def _block_call(lib, k, j0, p, dtype):
    def call(B):
        M = np.zeros((k, p), dtype=dtype, order="F")
        _capi.check(lib.lk_innerprod(B._h, k, B._h, j0, p, M.ctypes.data_as(_DP)))
        h, info = np.zeros((k, p), dtype=dtype, order="F"), C.c_int()
        _capi.check(lib.lk_dgs_block(B._h, k, B._h, j0, p, h.ctypes.data_as(_DP), C.byref(info)))
        assert info.value == 0
        return M, h
    return call


def _check_block(M, h, got, Q, Y, j0, what):
    p = Y.shape[1]
    check_xhy(M, Q, Y, "far " + what + " innerprod")
    for j in range(p):
        check_step(h[:, j], got[:, j0 + j], Q, Y[:, j], "far " + what + f" column {j}", orth=False)
    assert np.abs(Q.conj().T @ got[:, j0:j0 + p]).max() <= 1e-13 * np.linalg.norm(Y, axis=0).max(), what


@pytest.mark.parametrize("dtype", KINDS)
def test_multi_rhs_sweeps(arena, dtype):
    """lk_innerprod and lk_dgs_block with p = 4 right-hand sides: panel_dot_p and panel_sweep_p ("block_fused" = 0: dots / update / dots /
    update, 1: the fused three-pass schedule); X = columns 0..127 with Y = columns 128..131, and k = 64 with Y = columns 64..67."""
    P = far_a(arena, dtype)
    lib = _capi.load()
    for k in (128, 64):
        Q, Y = orthonormal_basis(NA, k, dtype, 60 + k), basis(NA, 4, dtype, 700 + k)
        for fused in (0, 1):
            what = f"p=4 k={k} block_fused={fused} {_name(dtype)}"
            (M, h), got = both(P, tuned(block_fused=fused), {0: Q, k: Y}, _block_call(lib, k, k, 4, dtype), range(k, k + 4), what)
            _check_block(M, h, got, Q, Y, k, what)


# ---- X^H Y and Gram on the matrix cores -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", KINDS)
def test_xhy_on_the_matrix_cores(arena, dtype):
    """lk_innerprod with 5, 32 and 48 right-hand sides in columns 128.. against X = columns 0..k-1, k = 40 and 128: panel_xhy_mfma at
    "xhy_db" = 0, 1, 2, panel_xhy_mfma3m for the complex kind at "gemm_3m" = 1, the VALU schedule ("xhy_mfma" = 0) once (n = 4099: one tile per block); then k = 72 with 32 and 48 right-hand sides at n = 70 001
    (real) / 20 001 (complex) and "xhy_db" = 1, 2: several tiles per block, so the staging of a block's next tile runs."""
    P = far_a(arena, dtype)
    lib = _capi.load()
    cp = is_cplx(dtype)
    Yall = basis(NA, 48, dtype, 600)
    for k in (40, 128):
        X = basis(NA, k, dtype, 500 + k)
        for p in (5, 32, 48):
            cfgs = [dict(xhy_db=db, gemm_3m=t) for db in (0, 1, 2) for t in ((0, 1) if cp else (1,))]
            if (k, p) == (128, 5):
                cfgs.append(dict(xhy_mfma=0))
            for cfg in cfgs:
                def call(B):
                    M = np.zeros((k, p), dtype=dtype, order="F")
                    _capi.check(lib.lk_innerprod(B._h, k, B._h, 128, p, M.ctypes.data_as(_DP)))
                    return (M,)
                what = f"xhy k={k} p={p} {cfg} {_name(dtype)}"
                (M,), _got = both(P, tuned(**cfg), {0: X, 128: Yall}, call, [], what)
                check_xhy(M, X, Yall[:, :p], "far " + what)
    # several tiles per block: the double-buffered kernels stage the block's NEXT tile (tile T + gridDim.x) while they multiply this one.  The
    # grids are 3 (real) / 2 (complex) blocks per CU on 32-row tiles up to 32 right-hand sides and one per CU beyond: n = 70 001 real
    # (2188 | 1094 tiles) and 20 001 complex (1251 tiles) give every block of a 256-CU chip two tiles or more; k = 72 crosses column 64
    n, k = (20_001 if cp else 70_001), 72
    assert_several_tiles(n, 16 if cp else 32, 2 if cp else 3, "panel_xhy_mfma, 32-row tiles")            # (a complex row is two doubles of a 32-row tile)
    assert_several_tiles(n, 16 if cp else 64, 1, "panel_xhy_mfma beyond 32 right-hand sides")
    P = far_a(arena, dtype, n, 176)
    X, Yall = basis(n, k, dtype, 520), basis(n, 48, dtype, 620)
    for p in (32, 48):
        for cfg in [dict(xhy_db=db, gemm_3m=t) for db in (1, 2) for t in ((0, 1) if cp else (1,))]:
            def call(B):
                M = np.zeros((k, p), dtype=dtype, order="F")
                _capi.check(lib.lk_innerprod(B._h, k, B._h, 128, p, M.ctypes.data_as(_DP)))
                return (M,)
            what = f"xhy n={n} k={k} p={p} {cfg} {_name(dtype)}"
            (M,), _got = both(P, tuned(**cfg), {0: X, 128: Yall}, call, [], what)
            check_xhy(M, X, Yall[:, :p], "far " + what)


def _upper_reference(X):
    """upper triangle of X^H X in longdouble, by column blocks (the lower one is never compared)"""
    Xe = ext(X)
    k = X.shape[1]
    ref = np.zeros((k, k), dtype=Xe.dtype)
    for j0 in range(0, k, 32):
        j1 = min(k, j0 + 32)
        ref[:j1, j0:j1] = Xe[:, :j1].conj().T @ Xe[:, j0:j1]
    return ref


@pytest.mark.parametrize("dtype", KINDS)
def test_gram(arena, dtype):
    """lk_gram with k = 16, 40, 100, 128 and "gram_rs" = 0 (panel_xhy_mfma / panel_gram_mfma3m), 1, 2 (the LDS-DMA kernels: real
    panel_gram_rs up to 128 columns; complex panel_gram_rs3m up to 80, panel_gram_rs3m4 up to 112, panel_gram_mfma3m beyond), n = 4099.
    Several tiles per block for the row-split kernels: the real kind at n = 70 001 with k = 128 (2188 tiles of 32 rows on one block per CU);
    the complex kind at n = 20 001 with k = 100 (1251 tiles of 16 rows for panel_gram_rs3m4 on one block per CU) and k = 128
    (panel_gram_mfma3m: 626 tiles of 32 rows on one block per CU; a longdouble reference of 70 001 complex rows takes tens of seconds)."""
    cp = is_cplx(dtype)
    big = (20_001, (100, 128)) if cp else (70_001, (128,))
    assert_several_tiles(big[0], 32, 1, "row-split Gram kernels and panel_gram_mfma3m at one block per CU")
    for n, ks in ((NA, (16, 40, 100, 128)), big):
        P = far_a(arena, dtype, n, 132)
        for k in ks:
            X = basis(n, k, dtype, 700 + k)
            ref, scale = _upper_reference(X), product_scale(X.conj().T, X)
            iu = np.triu_indices(k)
            for rs in (0, 1, 2):
                def call(B):
                    G = np.zeros((k, k), dtype=dtype, order="F")
                    _capi.check(_capi.load().lk_gram(B._h, k, G.ctypes.data_as(_DP)))
                    return (G,)
                what = f"gram n={n} k={k} gram_rs={rs} {_name(dtype)}"
                (G,), _got = both(P, tuned(gram_rs=rs), {0: X}, call, [], what)
                check_entrywise(G[iu], ref[iu], scale[iu], n, cp, "far " + what)
                assert np.array_equal(G, np.triu(G) + np.triu(G, 1).T)
        del P


# ---- the tall-skinny product ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", KINDS)
def test_tall_skinny_product(arena, dtype):
    """lk_lincomb with X = columns 0..k-1 (k = 64, 128) and the output in columns 128..: panel_gemm_mfma<ROLL> on the rolling ring
    ("gemm_mfma_min" = 1, "gemm_roll" = 2 / 1 -- n = 4099: eight full tiles through the straight-line ring, one per block, and a ragged one; the
    prefetch into a block's next tile is test_ring_across_the_tiles_of_a_block's) and on the batch schedule (0), four real products per complex one ("gemm_3m" = 0) and panel_gemm_mfma3m
    (1), the streaming panel_gemm ("gemm_mfma_min" = 100); pack_coef* with every call."""
    P = far_a(arena, dtype)
    lib = _capi.load()
    cp = is_cplx(dtype)
    cfgs = [dict(gemm_mfma_min=1, gemm_roll=r, gemm_3m=t) for r in (0, 1, 2) for t in ((0, 1) if cp else (1,))] + [dict(gemm_mfma_min=100)]
    for k in (64, 128):
        X = basis(NA, k, dtype, 300 + k)
        for q in ((1, 4, 12, 30) if cp else (1, 4, 20, 40)):
            Cm = basis(k, q, dtype, 900 + q)
            ref, scale = ext(X) @ ext(Cm), product_scale(X, Cm)
            for cfg in cfgs:
                def call(B):
                    _capi.check(lib.lk_lincomb(B._h, k, Cm.ctypes.data_as(_DP), q, B._h, 128))
                    return ()
                what = f"lincomb k={k} q={q} {cfg} {_name(dtype)}"
                _r, got = both(P, tuned(**cfg), {0: X}, call, range(128, 128 + q), what)
                check_entrywise(got[:, 128:128 + q], ref, scale, k, cp, "far " + what)


@pytest.mark.parametrize("dtype", KINDS)
def test_ring_across_the_tiles_of_a_block(arena, dtype):
    """The rolling ring of the tall-skinny product with TWO full tiles per block and a ragged last one: the refills of a tile's last four k-steps
    are then the first k-steps of the block's NEXT tile (`next_fast`, the running scalar offsets xo | xo2 = dnext, `primed`), so the cross-tile
    offset runs on columns 16..63, beyond 2^32 bytes.  k = 64, q = 3 (one output group), output in columns 64..66, "gemm_mfma_min" = 1.
      real     panel_gemm_mfma<false, 1, false, true>: 512-row tiles, grid capped at 4 blocks per CU (gemm_mfma_one), n = 2 x 512 x 4 x CUs + 3.
               One output group takes the ring at "gemm_roll" = 2 only; 1 and 0 are the batch schedule (the default key reaches the ring with
               49..64 outputs, which tests/test_gpu_kernel_instances.py runs).
      complex  panel_gemm_mfma3m<1, 2, true> ("gemm_3m" = 1, the default complex product): 256-row tiles, the same cap (gemm_mfma3m_one),
               n = 2 x 256 x 4 x CUs + 3; the ring at "gemm_roll" = 2 and 1, the batch schedule at 0.  (The four-product complex
               panel_gemm_mfma keeps nothing across tiles.)
    The CU count is the device's.  Every entry against the longdouble product, and "gemm_roll" ([bits]) changes no bit."""
    cp = is_cplx(dtype)
    import torch
    cap = 4 * torch.cuda.get_device_properties(tuned().device).multi_processor_count
    n, k, q = 2 * (256 if cp else 512) * cap + 3, 64, 3
    P = far_a(arena, dtype, n, k + q)
    X, Cm = basis(n, k, dtype, 1300), basis(k, q, dtype, 1390)
    ref, scale = ext(X) @ ext(Cm), product_scale(X, Cm)
    lib = _capi.load()
    outs = []
    for roll in (2, 1, 0):
        def call(B):
            _capi.check(lib.lk_lincomb(B._h, k, Cm.ctypes.data_as(_DP), q, B._h, k))
            return ()
        what = f"ring across tiles n={n} gemm_roll={roll} {_name(dtype)}"
        _r, got = both(P, tuned(gemm_mfma_min=1, gemm_roll=roll, gemm_3m=1), {0: X} if roll == 2 else {}, call, range(k, k + q), what)
        check_entrywise(got[:, k:], ref, scale, k, cp, "far " + what)
        outs.append(got[:, k:].tobytes())
    assert outs[1] == outs[0] and outs[2] == outs[0]


# ---- the fused block pass ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", KINDS)
def test_fused_block_pass(arena, dtype):
    """lk_dgs_block with 8, 17 and 32 right-hand sides in columns 128.. against X = columns 0..k-1 (k = 64, 128): the matrix-core passes
    ("block_fused" = 0), the fused update + product panel_xhy_upd_mfma (1, 2) and, for the real kind, panel_xhy_upd_rs by row-owner waves
    ("upd_rs" = 1; 0 = off).  k = 128, p = 32 also at n = 70 001 (real: 2188 row tiles on 2 blocks per CU for panel_xhy_upd_mfma, on one
    for panel_xhy_upd_rs, whose two teams and LDS-DMA stages then take several tiles) and n = 20 001 (complex: 1251 tiles on one block per CU).
    One context per tuning set serves every shape in the order k = 64 then 128: the regression guard of the product workspace's sizing (a workspace
    grown for k = 64, p = 17 held the coefficient pass at k = 128 on these few row tiles but not the fused pass, and lk_dgs_block failed)."""
    cp = is_cplx(dtype)
    lib = _capi.load()
    shapes = [(NA, k, p) for k in (64, 128) for p in (8, 17, 32)] + [(20_001 if cp else 70_001, 128, 32)]
    assert_several_tiles(shapes[-1][0], 16 if cp else 32, 1 if cp else 2, "panel_xhy_upd_mfma / panel_xhy_upd_rs")
    P = None
    for n, k, p in shapes:
        if P is None or P.n != n:
            P = far_a(arena, dtype, n, 160)
        Q, Y = orthonormal_basis(n, k, dtype, 60 + k), basis(n, p, dtype, 700 + p)
        cfgs = [dict(block_fused=f) for f in (0, 1, 2)] if cp else [dict(block_fused=f, upd_rs=u) for f in (0, 1, 2) for u in (0, 1)]
        for cfg in cfgs if n == NA else cfgs[-2:]:
            what = f"dgs_block n={n} k={k} p={p} {cfg} {_name(dtype)}"
            (M, h), got = both(P, tuned(**cfg), {0: Q, 128: Y}, _block_call(lib, k, 128, p, dtype), range(128, 128 + p), what)
            _check_block(M, h, got, Q, Y, 128, what)


# ---- factorisations ---------------------------------------------------------------------------------------------------------------------
def _diag(n, dtype, hermitian=False):
    g = np.arange(n) / n
    return ((1.0 + g) * (np.exp(0.4j * g) if is_cplx(dtype) and not hermitian else 1.0)).astype(dtype)


def _start(n, dtype, seed):
    x = seeded(n, dtype, seed)
    return x / np.linalg.norm(x)


@pytest.mark.parametrize("dtype", KINDS)
def test_factorisations(arena, dtype):
    """n = 2001, the basis in columns 0..72 (it crosses columns 16 and 64): lk_arnoldi on lk_linop_diag_create and, real kind, on
    lk_linop_diag_linspace_create with the row operator fused into the sweeps ("fuse_rowop" = 1) and as a kernel of its own (0), batched
    ("async_arnoldi" = 1) and step by step (0); lk_arnoldi_segments with three segments; lk_lanczos; lk_bidiag with U in the far panel
    and V in an engine-made one and the other way round; lk_arnoldi_block with p = 4 over 20 steps (columns 0..83); lk_qr on columns 120..131.
    Against ora.arnoldi / lanczos / bidiagonalization / arnoldi_block / qr_no_pivoting at 1e-12 per column of the projected matrix."""
    n, m = 2001, 72
    P = far_a(arena, dtype, n)
    x0 = _start(n, dtype, 7)
    Z = np.zeros((n, 132), dtype=dtype, order="F")
    d = _diag(n, dtype)

    def oracle_arnoldi(dd):
        Xo, Ho = np.zeros((n, m + 1), dtype=dtype, order="F"), np.zeros((m + 1, m), dtype=dtype, order="F")
        Xo[:, 0] = x0
        assert ora.arnoldi(ora.DiagOp(dd), Xo, Ho) == 0
        return Xo, Ho

    ops = {"diag": (lambda c: lk.diag_linop_gpu(d, c), oracle_arnoldi(d))}
    if not is_cplx(dtype):
        ops["linspace"] = (lambda c: lk.diag_linop_gpu(n_local=n, row0=0, d0=1.0, dstep=1.0 / n, ctx=c), oracle_arnoldi(1.0 + np.arange(n) * (1.0 / n)))
    for opname, (mk, (_Xo, Ho)) in ops.items():
        for keys in (dict(fuse_rowop=1, async_arnoldi=1), dict(fuse_rowop=0, async_arnoldi=1), dict(fuse_rowop=1, async_arnoldi=0)):
            for segs in ((None, (24, 48, 72)) if keys == dict(fuse_rowop=1, async_arnoldi=1) else (None,)):
                c = tuned(**keys)
                A = mk(c)

                def call(B):
                    H = np.zeros((m + 1, m), dtype=dtype, order="F")
                    if segs is None:
                        assert lk.arnoldi(A, B, H) == 0
                    else:
                        assert lk.arnoldi(A, B, H, _segments=segs, _progress=lambda a, b: 0) == 0
                    return (H,)

                what = f"arnoldi {opname} {keys} segments={segs} {_name(dtype)}"
                (H,), got = both(P, c, [(0, Z), (0, x0)], call, range(1, m + 1), what, ncols=m + 1)
                assert_columns_close(H, Ho, "far " + what)
                assert np.abs(got[:, :m + 1].conj().T @ got[:, :m + 1] - np.eye(m + 1)).max() <= 1e-12, what
                assert got[:, 0].tobytes() == x0.tobytes()
                del A
    c = tuned()
    # Lanczos on the Hermitian diagonal
    dh = _diag(n, dtype, hermitian=True)
    A = lk.diag_linop_gpu(dh, c)

    def lanczos(B):
        T = np.zeros((m + 1, m), dtype=dtype, order="F")
        assert lk.lanczos(A, B, T) == 0
        return (T,)

    (T,), got = both(P, c, [(0, Z), (0, x0)], lanczos, range(1, m + 1), f"lanczos {_name(dtype)}", ncols=m + 1)
    Xo, To = np.zeros((n, m + 1), dtype=dtype, order="F"), np.zeros((m + 1, m), dtype=dtype, order="F")
    Xo[:, 0] = x0
    assert ora.lanczos(ora.DiagOp(dh), Xo, To) == 0
    assert_columns_close(T, To, f"far lanczos {_name(dtype)}")
    del A
    # Golub-Kahan: one basis far, the other engine-made
    A = lk.diag_linop_gpu(d, c)
    Uo, Vo, Bo = np.zeros((n, m + 1), dtype=dtype, order="F"), np.zeros((n, m), dtype=dtype, order="F"), np.zeros((m + 1, m), dtype=dtype, order="F")
    Uo[:, 0] = x0
    assert ora.bidiagonalization(ora.DiagOp(d), ora.DiagOp(d.conj()), Uo, Vo, Bo) == 0
    for far_is_u in (True, False):
        def bidiag(B):
            other = lk.krylov_basis_gpu(n, m + (0 if far_is_u else 1), dtype, c)
            other.upload(np.zeros((n, other.ncols), dtype=dtype))
            U, V = (B, other) if far_is_u else (other, B)
            if not far_is_u:
                U.upload(x0.reshape(-1, 1), 0)
            Bm = np.zeros((m + 1, m), dtype=dtype, order="F")
            assert lk.bidiagonalization(A, U, V, Bm) == 0
            return Bm, other.download()
        nc = m + 1 if far_is_u else m
        what = f"bidiag far {'U' if far_is_u else 'V'} {_name(dtype)}"
        (Bm, _o), got = both(P, c, [(0, Z), (0, x0)] if far_is_u else {0: Z}, bidiag, range(1 if far_is_u else 0, nc), what, ncols=nc)
        assert_columns_close(Bm, Bo, "far " + what)
        assert np.abs(got[:, :nc].conj().T @ got[:, :nc] - np.eye(nc)).max() <= 1e-12, what
    # block Arnoldi, p = 4 over 20 steps
    p, kdim = 4, 20
    ncol = (kdim + 1) * p
    Q0 = orthonormal_basis(n, p, dtype, 74)

    def block(B):
        H = np.zeros((ncol, kdim * p), dtype=dtype, order="F")
        assert lk.arnoldi(A, B, H, blksize=p) == 0
        return (H,)

    (H,), got = both(P, c, [(0, Z), (0, Q0)], block, range(p, ncol), f"arnoldi_block {_name(dtype)}", ncols=ncol)
    Xo, Ho = np.zeros((n, ncol), dtype=dtype, order="F"), np.zeros((ncol, kdim * p), dtype=dtype, order="F")
    Xo[:, :p] = Q0
    assert ora.arnoldi_block(ora.DiagOp(d), Xo, Ho, p) == 0
    assert_columns_close(H, Ho, f"far arnoldi_block {_name(dtype)}")
    del A
    # qr_no_pivoting of columns 120..131
    M0 = basis(n, 12, dtype, 300)

    def qr(B):
        R, info = np.zeros((12, 12), dtype=dtype, order="F"), C.c_int()
        _capi.check(_capi.load().lk_qr(B._h, 120, 12, R.ctypes.data_as(_DP), 12, 1e-12, C.byref(info)))
        assert info.value == 0
        return (R,)

    (R,), got = both(P, c, {0: Z, 120: M0}, qr, range(120, 132), f"qr {_name(dtype)}", ncols=132)
    Mo, Ro = M0.copy(order="F"), np.zeros((12, 12), dtype=dtype, order="F")
    assert ora.qr_no_pivoting(Mo, Ro) == 0
    assert_columns_close(R, Ro, f"far qr {_name(dtype)}")
    assert np.abs(got[:, 120:132] - Mo).max() <= 1e-12 * np.abs(Mo).max()


# ---- geometry B: the lane-split sweeps --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", KINDS)
def test_lane_split_sweeps(arena, dtype):
    """Geometry B (columns 2^26 bytes apart, n = 2051): lk_dgs with k = 129, 256, 385, 512, X = columns 0..k-1 and y in column k -- column 512
    lies beyond 2^32 doubles --, on the lane-split sweeps with their wide register tiles and scalar-base loads ("wide_regs" = 2) and without
    (0; there "wide_s3" = 1 / 0: the column-group sweep 3 or the lane-split one); lk_innerprod of 200 columns against column 512 at
    "dot_colwise" = 0: the dot-only lane-split sweep."""
    n = 2051
    P = FarPanel(tuned(), dtype, n, FAR_COLS_B, FAR_STRIDE_B, backing=arena.get(FAR_COLS_B * FAR_STRIDE_B))
    for k in (129, 256, 385, 512):
        Q, y0 = orthonormal_basis(n, k, dtype, 40 + k), seeded(n, dtype, 5000 + k)
        for keys in (dict(wide_regs=2), dict(wide_regs=0, wide_s3=1), dict(wide_regs=0, wide_s3=0)):
            def call(B):
                h = np.zeros(k, dtype=dtype)
                assert lk.double_gram_schmidt_step(B[k], B[:k], False, h) == 0
                return (h,)
            what = f"dgs lane split k={k} {keys} {_name(dtype)}"
            (h,), got = both(P, tuned(resident=0, **keys), {0: Q, k: y0}, call, [k], what)
            check_step(h, got[:, k], Q, y0, what)
    X, y = basis(n, 200, dtype, 1200), seeded(n, dtype, 1199)

    def dots(B):
        M = np.zeros((200, 1), dtype=dtype, order="F")
        _capi.check(_capi.load().lk_innerprod(B._h, 200, B._h, 512, 1, M.ctypes.data_as(_DP)))
        return (M,)

    (M,), _got = both(P, tuned(dot_colwise=0), {0: X, 512: y}, dots, [], f"dot-only lane split {_name(dtype)}")
    check_xhy(M, X, y.reshape(-1, 1), f"far dot-only lane-split sweep k=200 {_name(dtype)}")


# ---- the dense operator with a far lda --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", KINDS)
def test_dense_operator_far_lda(arena, dtype):
    """lk_linop_dense_wrap_sharded on one rank (row_starts = [0, n]) with n = 96 and lda = 2^28 bytes' worth of elements (a 24 GiB buffer of
    which 96 x 96 entries are live, guard bands as on the panels): k_gemv_n + k_gemv_n_finish (LK_OP_N) and k_gemv_h (LK_OP_H), every
    entry of y against the longdouble product within gamma_(n (+ 2 complex)), as tests/test_gpu_operator_kernels.py checks the dense operator."""
    n = 96
    cp = is_cplx(dtype)
    c = tuned()
    P = FarPanel(c, dtype, n, n, FAR_STRIDE_A, backing=arena.get(n * FAR_STRIDE_A))
    A, xh = basis(n, n, dtype, 7000), seeded(n, dtype, 6999)
    P.set(A)
    op = lk.dense_linop_gpu.from_device_panel(P.B, row_starts=[0, n])
    E = lk.krylov_basis_gpu(n, n, dtype, c)
    E.upload(A)
    ref_op = lk.dense_linop_gpu.from_device_panel(E, row_starts=[0, n])                  # the same entry on an engine-made panel
    x, y = lk.dense_vector_gpu.from_array(xh, c), lk.dense_vector_gpu(n, dtype, c)
    for trans in (False, True):
        out = []
        for o in (op, ref_op):
            (o.apply_rmatvec if trans else o.apply_matvec)(x, y)
            out.append(y.to_array())
        Ao = A.conj().T if trans else A
        check_entrywise(out[0], ext(Ao) @ ext(xh), product_scale(Ao, xh), n + (2 if cp else 0), cp,
                        f"far lda k_gemv_{'h' if trans else 'n'} {_name(dtype)}")
        assert out[0].tobytes() == out[1].tobytes(), trans
    got = P.get("dense operator")
    assert got.tobytes() == A.tobytes()
    del op, ref_op
