"""Shared helpers of the GPU test files (test infrastructure: inputs come from the oracle's counter RNG, so CPU and GPU see identical data)."""
import ctypes as C
import functools
import threading

import numpy as np

import lightkrylov_amd as lk
from lightkrylov_amd import _capi
from lightkrylov_amd.context import _DevMem
from oracle import oracle as ora
from tests._tol import _report

KINDS = [np.float64, np.complex128]
U = 2.0 ** -53


# ---- entrywise a-priori bounds (tests/test_gpu_kernel_instances.py states them; tests/test_gpu_operator_kernels.py uses them too) --------
def gamma(m):
    """gamma_m of the double sum plus that of the longdouble reference (u = 2^-64), which is not exact either: a row of one product
    rounds by up to u of it, so the measured ratio can come within 2 % of 1"""
    m = np.asarray(m, dtype=np.float64)
    return m * U / (1.0 - m * U) + m * 2.0 ** -64 / (1.0 - m * 2.0 ** -64)


def is_cplx(dtype):
    return np.dtype(dtype).kind == "c"


def ext(A):
    A = np.asarray(A)
    return A.astype(np.clongdouble) if np.iscomplexobj(A) else A.astype(np.longdouble)


def product_scale(A, B):
    """|A| |B| (real) or (|Ar|+|Ai|)(|Br|+|Bi|) (complex): the scale of the bound; A, B already in the orientation of the product"""
    if np.iscomplexobj(A) or np.iscomplexobj(B):
        return (np.abs(A.real) + np.abs(A.imag)) @ (np.abs(B.real) + np.abs(B.imag))
    return np.abs(A) @ np.abs(B)


def check_entrywise(got, ref, scale, m, cplx, label):
    """entrywise |got - ref| against the bound for sums of m terms (m: scalar or array broadcast like got); returns the worst ratio"""
    got = np.asarray(got)
    bound = (2.0 * gamma(2 * np.asarray(m) + 5) if cplx else gamma(m)) * scale
    d = got.astype(ref.dtype) - ref
    errs = [np.abs(d.real), np.abs(d.imag)] if cplx else [np.abs(d)]
    ratio = 0.0
    for e in errs:
        e = e.astype(np.float64)
        over = ~(e <= bound)                                        # a NaN (an entry nobody wrote) is over any bound
        assert not over.any(), f"{label}: entry {np.argwhere(over)[0].tolist()} off by {e[over][0]:.3e} > bound {bound[over][0]:.3e}"
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(bound > 0, e / np.where(bound > 0, bound, 1.0), 0.0)
        ratio = max(ratio, float(r.max()) if r.size else 0.0)
    _report(label, ratio, 1.0, "entrywise gamma bound")
    return ratio


def device_num_cu(c):
    """the compute-unit count of the context's device, as lk_init reads it (the context has no accessor for it): blas1_grid caps the
    BLAS-1 grids at num_cu * "blas1_grid_mult" blocks"""
    import torch
    return torch.cuda.get_device_properties(c.device).multi_processor_count


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


def skewed_basis(n, k, dtype, seed, delta=1e-3):
    """Q (I + delta S): Q from orthonormal_basis, S a k x k matrix from the counter generator (complex for the complex kind).  Off
    orthonormal by about delta * sqrt(k), cond about 1 + 2 delta ||S||: the second Gram-Schmidt pass has a correction of about delta |y|
    to make, and nothing amplifies rounding.  k > n: unit random columns (no orthonormal Q exists)."""
    if k > n:
        X = basis(n, k, dtype, seed)
        return np.asfortranarray(X / np.linalg.norm(X, axis=0))
    Q = orthonormal_basis(n, k, dtype, seed)
    S = basis(k, k, dtype, seed + 100_003)
    return np.asfortranarray(Q @ (np.eye(k, dtype=dtype) + delta * S))


def near_span(X, seed, eps=1e-6):
    """X c + eps r, c and r from the counter generator (`seed` and `seed + 1`: the caller picks them outside the seeds of X's columns):
    beta_{k+1} is about eps / |c|, and the second pass removes what the cancellation of the first left behind."""
    c = seeded(X.shape[1], X.dtype, seed)
    return X @ c + eps * seeded(X.shape[0], X.dtype, seed + 1)


@functools.lru_cache(maxsize=4)
def _second_pass_panel(n, k, dtype, skewed):
    X = (skewed_basis if skewed else orthonormal_basis)(n, k, dtype, 40 + k)
    X.setflags(write=False)                                        # (shared between the inputs of one shape)
    return X


def second_pass_input(n, k, dtype, which, p=1):
    """(X, Y) of the second-pass tests, Y of p columns: "skew_rand" = skewed X, random columns; "skew_span" = skewed X, columns near span(X);
    "orth_span" = orthonormal Q, columns near span(Q) (k > n: the unit random columns of skewed_basis in every case).  X has the column
    seeds 40 + k ..; column j of Y uses 5000 + k + 2 j (and + 1), which no column of X has.  X is read-only."""
    X = _second_pass_panel(n, k, dtype, which != "orth_span" or k > n)
    cols = [seeded(n, dtype, 5000 + k + 2 * j) if which == "skew_rand" else near_span(X, 5000 + k + 2 * j) for j in range(p)]
    return X, np.asfortranarray(np.stack(cols, axis=1))


def arnoldi_operator(n, dtype):
    """diagonal of the operator the continued factorisations run on: 1 + i / n, turned in the complex plane for the complex kind"""
    g = np.arange(n) / n
    return ((1.0 + g) * (np.exp(0.4j * g) if np.dtype(dtype).kind == "c" else 1.0)).astype(dtype)


def _long(a):
    a = np.asarray(a)
    return a.astype(np.clongdouble if a.dtype.kind == "c" else np.longdouble)


def dgs_longdouble(y, X):
    """two classical Gram-Schmidt passes in longdouble / clongdouble: h1 = X^H y, y' = y - X h1, h2 = X^H y', y'' = y' - X h2.  Returns
    h1, h2, y', y'' (beta of the step is h1 + h2).  The plain high-precision statement of gram_schmidt.fypp:12-57."""
    Xl, yl = _long(X), _long(y)
    Xh = Xl.conj().T
    h1 = Xh @ yl
    y1 = yl - Xl @ h1
    h2 = Xh @ y1
    y2 = y1 - Xl @ h2
    return h1, h2, y1, y2


def step_bound_from(X, y, h1, h2, y1):
    """(h*, scale) of the a-priori entrywise bound on h = h1 + h2 of one two-pass step of y against X (tests/test_gpu_tile_prefetch.py
    derives it), from the longdouble h1, h2 and y' of dgs_longdouble(y, X)"""
    # the scale in double: it multiplies gamma_m, so its own rounding (n u of each entry, added back below) is all that matters.
    # |X^T X - I| <= |fl(X^T X) - I| + gamma_n |X|^T |X|
    Xa, ya = np.abs(X), np.abs(y)
    G = np.abs(X.T @ X - np.eye(X.shape[1])) + gamma(X.shape[0]) * (Xa.T @ Xa)
    scale = G @ (Xa.T @ ya) + Xa.T @ (ya + Xa @ np.abs(h1).astype(np.float64)) + Xa.T @ np.abs(y1).astype(np.float64) + np.abs(h1 + h2).astype(np.float64)
    return h1 + h2, scale * (1.0 + 4.0 * X.shape[0] * 2.0 ** -53)


def _step_bound(X, y):
    """(h*, scale) of that bound for one two-pass step of y against X, in longdouble"""
    h1, h2, y1, _y2 = dgs_longdouble(y, X)
    return step_bound_from(X, y, h1, h2, y1)


def assert_second_pass_matters(h1, h2, y):
    """A condition on the INPUT of a test, not a measurement of the code under test: the reference's own second-pass coefficients reach
    1e-6 |y|, a million times the 1e-12 the results are compared at, so a wrong second pass cannot hide below the bound."""
    ynorm = float(np.linalg.norm(_long(y)))
    big = float(np.abs(h2).max()) if np.size(h2) else 0.0
    assert big >= 1e-6 * ynorm, f"second pass has nothing to do: max|h2| = {big:.2e} < 1e-6 |y| = {1e-6 * ynorm:.2e}"
    return big / ynorm


def _spd(n, seed, lead=(8.0, 6.0, 4.0)):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((n, n)) / np.sqrt(n)
    A = M.T @ M + np.eye(n)
    A[:len(lead), :len(lead)] += np.diag(lead)
    return np.asfortranarray(A)


def _lap5_csr(N):
    import scipy.sparse as sp
    T = sp.diags([-np.ones(N - 1), 4.0 * np.ones(N), -np.ones(N - 1)], [-1, 0, 1])
    S = sp.diags([-np.ones(N - 1), -np.ones(N - 1)], [-1, 1])
    return ((sp.kron(sp.identity(N), T) + sp.kron(S, sp.identity(N))) * float((N + 1) ** 2)).tocsr()


def _pool_fns(ctx):
    lib = _capi.load()

    def acquire(dtype, n, tag):
        slab, col = C.c_void_p(), C.c_int()
        _capi.check(lib.lk_pool_acquire(ctx._h, dtype, n, C.c_uint64(tag), C.byref(slab), C.byref(col)))
        return slab.value, col.value

    def info(slab, col):
        t, g = C.c_uint64(), C.c_uint64()
        _capi.check(lib.lk_pool_column_info(ctx._h, C.c_void_p(slab), col, C.byref(t), C.byref(g)))
        return t.value, g.value

    return lib, acquire, info


def _arnoldi_h(ctx, n=400_003, m=12):
    X = lk.krylov_basis_gpu(n, m + 1, np.float64, ctx)
    A = lk.diag_linop_gpu(n_local=n, row0=0, d0=1.0, dstep=1.0 / n, ctx=ctx)
    H = np.zeros((m + 1, m), order="F")
    X[0].rand(True, seed=7)
    assert lk.arnoldi(A, X, H) == 0
    return H, X.download()


# ---- caller-owned panels (lk_basis_wrap) inside a larger buffer whose other rows are live -----------------------------------------
POISON = 0x7FF8DEADBEEF0001                       # a quiet NaN whose payload no arithmetic produces


def fit(n, dtype, layout):
    """n as the layout can take it: ld = n must be even for the real kind; the complex kind's unpadded case is the odd one"""
    if layout == "unpadded" and (n % 2 == 1) != (np.dtype(dtype).kind == "c"):
        return n + 1
    return n


class CallerPanel:
    """An n x ncols panel wrapped (lk_basis_wrap) inside one flat engine-owned buffer laid out as `layout` says.  `set` writes panel
    contents, `get` reads them back and asserts that nothing outside the panel's rows changed.  The layouts (tests/test_gpu_caller_memory.py):
    "nan_pad" / "big_pad" ld = n + 3 or n + 4 with NaN / +-1e300 padding, "offNNN" the same ld NNN bytes into a buffer of live non-zero
    rows, "unpadded" ld = n; `extra_ld` (even) more padding rows per column, for two panels of one shape with different ld; `pad`: ld = n + pad
    exactly, for either kind (the caller keeps ld even for the real kind)."""

    def __init__(self, ctx, dtype, n, ncols, layout, seed=0, extra_ld=0, pad=None):
        dt = np.dtype(dtype)
        cplx = dt.kind == "c"
        es = dt.itemsize
        if layout == "unpadded":
            assert (n % 2 == 1) == cplx, "fit() the size first"
            ld, head = n, 16 // es
        else:
            ld = n + (3 if cplx else 3 + (n + 3) % 2) + extra_ld if pad is None else n + pad
            assert cplx or ld % 2 == 0
            head = int(layout[3:]) // es if layout.startswith("off") else 0
        total = head + ld * ncols + 64
        img = np.empty(total, dtype=dt)
        if layout in ("nan_pad", "unpadded"):
            img.view(np.uint64)[:] = POISON
        elif layout == "big_pad":
            img.view(np.float64)[:] = 1e300
            img.view(np.float64)[1::2] = -1e300
        else:
            ora.fill_counter(img, 9000 + seed)
            img += np.where(img.real >= 0, 0.5, -0.5)              # |live entry| >= 0.5
        self.inside = np.zeros(total, dtype=bool)
        for j in range(ncols):
            self.inside[head + j * ld:head + j * ld + n] = True
        self.n, self.ncols, self.ld, self.head, self.dtype, self.layout = n, ncols, ld, head, dt, layout
        self.img = img
        self.backing = lk.krylov_basis_gpu(total, 1, dt, ctx)
        self.backing.upload(img.reshape(-1, 1))
        ptr = self.backing.info()[4] + head * es
        assert ptr % 16 == 0 and (layout == "nan_pad" or layout == "big_pad" or ptr % 256 != 0)
        h = C.c_void_p()
        _capi.check(self.backing._lib.lk_basis_wrap(ctx._h, _capi.LK_C128 if cplx else _capi.LK_F64, n, ncols, ld, C.c_void_p(ptr),
                                                    C.byref(h)))
        self.B = lk.krylov_basis_gpu(n, ncols, dt, ctx, _handle=h, _owner=self.backing)

    def _cols(self, buf):
        return np.stack([buf[self.head + j * self.ld:self.head + j * self.ld + self.n] for j in range(self.ncols)], axis=1)

    def set(self, A, col0=0):
        A = np.asarray(A, dtype=self.dtype).reshape(self.n, -1, order="F")
        buf = self.backing.download()[:, 0]
        for j in range(A.shape[1]):
            o = self.head + (col0 + j) * self.ld
            buf[o:o + self.n] = A[:, j]
        self.backing.upload(buf.reshape(-1, 1))

    def get(self, what=""):
        buf = self.backing.download()[:, 0]
        out = ~self.inside
        got, want = buf[out].view(np.uint64), self.img[out].view(np.uint64)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (f"{what} [{self.layout}, n = {self.n}, ld = {self.ld}]: {bad.size} words outside the panel changed, first at "
                               f"outside word {int(bad[0])}: {got[bad[0]]:#x} (was {want[bad[0]]:#x})")
        return np.asfortranarray(self._cols(buf))


# ---- panels whose columns lie further apart than 32-bit offsets reach (tests/test_gpu_far_columns.py) ---------------------------------
# Column j of a panel starts j * stride bytes from the base.  The three limits of narrowed address arithmetic and the first column
# that lies at or beyond each (8-byte doubles):
#   geometry A, stride 2^28 B: 2^32 B = 16 strides -> column 16;  2^31 doubles = 2^34 B -> column 64;   2^32 doubles = 2^35 B -> column 128
#                              176 columns = 176 * 2^28 B = 44 GiB of address space
#   geometry B, stride 2^26 B: 2^32 B -> column 64;               2^34 B -> column 256;                 2^35 B -> column 512
#                              513 columns = 513 * 2^26 B = 32.06 GiB
FAR_STRIDE_A, FAR_COLS_A = 1 << 28, 176
FAR_STRIDE_B, FAR_COLS_B = 1 << 26, 513
FAR_BAND = 4096                                   # bytes of each guard band


class FarPanel:
    """An n x ncols panel wrapped (lk_basis_wrap) at ld = stride_bytes / itemsize inside one torch byte buffer of ncols * stride_bytes:
    only rows [0, n) of a column are ever touched, so the panel moves megabytes while its columns lie up to 44 GiB from its base.
    `set` / `get` go through a torch strided view (64-bit strides), never through the engine.  Rows [0, n) of every column start as
    POISON, the 4 KB after row n of every column and the last 4 KB before the next column are POISON guard bands: `get` asserts
    that both bands of every column are bit-identical and returns ALL columns; `shadow` is what was set, for the columns a call must
    not write.  `backing`: a buffer to reuse (one allocation per geometry and module)."""

    def __init__(self, ctx, dtype, n, ncols, stride_bytes, backing=None):
        import torch
        dt = np.dtype(dtype)
        es = dt.itemsize
        assert stride_bytes % (32 * es) == 0 and n * es + 2 * FAR_BAND <= stride_bytes
        if backing is None:
            backing = torch.empty(ncols * stride_bytes, dtype=torch.uint8, device=f"cuda:{ctx.device}")
        assert backing.numel() >= ncols * stride_bytes and backing.data_ptr() % 256 == 0
        self.backing, self.torch = backing, torch
        self.n, self.ncols, self.stride, self.dtype, self.ld = n, ncols, stride_bytes, dt, stride_bytes // es
        self.words = backing[:ncols * stride_bytes].view(torch.int64).view(ncols, stride_bytes // 8)       # one row per column
        nw, bw = n * es // 8, FAR_BAND // 8
        self._rows = self.words[:, :nw]
        self._bands = (self.words[:, nw:nw + bw], self.words[:, -bw:])
        self._rows.fill_(POISON)                                        # (below 2^63: the pattern is a positive 64-bit word)
        for b in self._bands:
            b.fill_(POISON)
        torch.cuda.synchronize()
        img = np.empty((ncols, n), dtype=dt)
        img.view(np.uint64)[...] = POISON
        self.shadow = img.T                                             # (n x ncols, column-major)
        h = C.c_void_p()
        lib = _capi.load()
        _capi.check(lib.lk_basis_wrap(ctx._h, _capi.LK_C128 if dt.kind == "c" else _capi.LK_F64, n, ncols, self.ld,
                                      C.c_void_p(backing.data_ptr()), C.byref(h)))
        self.B = lk.krylov_basis_gpu(n, ncols, dt, ctx, _handle=h, _owner=backing)

    def set(self, A, col0=0):
        A = np.asarray(A, dtype=self.dtype).reshape(self.n, -1, order="F")
        m = A.shape[1]
        host = np.ascontiguousarray(A.T).view(np.int64).reshape(m, -1)                                 # one row per column
        self.B.ctx.sync()
        self._rows[col0:col0 + m].copy_(self.torch.from_numpy(host))
        self.torch.cuda.synchronize()
        self.shadow[:, col0:col0 + m] = A

    def get(self, what=""):
        self.B.ctx.sync()
        self.torch.cuda.synchronize()
        for name, b in zip(("after row n", "before the next column"), self._bands):
            w = b.contiguous().cpu().numpy().view(np.uint64)
            bad = np.argwhere(w != POISON)
            assert bad.size == 0, (f"{what}: guard band {name} of column {int(bad[0][0])} changed at word {int(bad[0][1])}: "
                                   f"{int(w[tuple(bad[0])]):#x}")
        rows = self._rows.contiguous().cpu().numpy()
        return np.asfortranarray(rows.view(self.dtype).T)

    def assert_untouched(self, got, written, what=""):
        """every column of `got` outside `written` is bit-identical with what was set (a store whose offset wrapped modulo 2^32 bytes
        or doubles lands on the same row of a lower column)"""
        keep = np.setdiff1d(np.arange(self.ncols), np.asarray(list(written), dtype=np.int64))
        a, b = (np.ascontiguousarray(M.T[keep]).view(np.uint64) for M in (got, self.shadow))           # one row per column
        bad = np.argwhere(a != b)
        assert bad.size == 0, (f"{what}: column {int(keep[bad[0][0]])} (not an output) changed at row "
                               f"{int(bad[0][1]) // (self.dtype.itemsize // 8)}")


# ---- row-sharded emulation on one GPU (tests/test_gpu_sharded_emulation.py describes it) --------------------------------------------
class _EmulatedGroup:
    """Sum all-reduce between `nranks` threads; buffers live on the same device."""

    def __init__(self, nranks):
        import torch
        self.torch = torch
        self.n = nranks
        self.barrier = threading.Barrier(nranks)
        self.slots = [None] * nranks
        self.calls = 0
        self.rank_calls = [0] * nranks                  # all-reduce calls each rank made (they must agree)

    def hook(self, rank, ctx):
        torch = self.torch

        def _cb(_user, dev_ptr, count, stream_ptr):
            try:
                self.rank_calls[rank] += 1
                ctx.sync_stream_only()
                self.slots[rank] = torch.as_tensor(_DevMem(int(dev_ptr), int(count)), device="cuda:0")
                self.barrier.wait(timeout=120)
                if rank == 0:
                    total = self.slots[0].clone()
                    for r in range(1, self.n):
                        total += self.slots[r]
                    for r in range(self.n):
                        self.slots[r].copy_(total)
                    torch.cuda.synchronize()
                    self.calls += 1
                self.barrier.wait(timeout=120)
                return 0
            except Exception as exc:  # noqa: BLE001
                print("emulated all-reduce failed:", repr(exc))
                self.barrier.abort()
                return 1
        return _capi.ALLREDUCE_FN(_cb)


def _sharded(n, nranks, body):
    """Run body(rank, ctx, row0, n_local) on `nranks` threads with an emulated all-reduce; returns results."""
    lib = _capi.load()
    grp = _EmulatedGroup(nranks)
    out, errs = [None] * nranks, []

    def worker(rank):
        try:
            ctx = lk.Context(device=0, use_torch_stream=False)           # own stream per rank
            ctx.sync_stream_only = lambda: _capi.check(lib.lk_sync(ctx._h))
            cb = grp.hook(rank, ctx)
            _capi.check(lib.lk_set_allreduce(ctx._h, cb, None, nranks, rank))
            ctx._cb, ctx.nranks, ctx.rank = cb, nranks, rank
            row0, nl = lk.row_partition(n, nranks, rank)
            ctx.set_partition(row0, n)
            out[rank] = body(rank, ctx, row0, nl)
        except Exception as exc:  # noqa: BLE001
            errs.append(exc)
            grp.barrier.abort()

    ts = [threading.Thread(target=worker, args=(r,)) for r in range(nranks)]
    [t.start() for t in ts]
    [t.join(600) for t in ts]
    assert not errs, errs
    return out, grp


# ---- bases wider than 512 columns (tests/test_oracle_very_wide.py pins these inputs, tests/test_gpu_very_wide_bases.py runs them) --------
# lk_dgs changes schedule at 512 | 513 (one sweep holds 512 columns), runs 2 / 3 / 4 device panels of 512 up to 2048 and panels of 128
# with a host round trip each beyond: both sides of every panel count, 2176 = 17 * 128 (a full last panel), 2177 (a last panel of one)
VERY_WIDE_K = (512, 513, 1023, 1024, 1025, 1536, 1537, 2047, 2048, 2049, 2100, 2176, 2177)
VERY_WIDE_FLAG_K = (600, 1600, 2100)              # one k per schedule for the flags and outputs
VERY_WIDE_PANEL_K = (1030, 2060)                  # caller-owned panels, sharded emulation, one step of each factorisation
VERY_WIDE_BLOCK_K = (600, 1100)                   # lk_dgs_block's column-by-column route


def very_wide_n(k):
    """the smallest odd n >= k + 11: a skewed (near orthonormal) panel needs n >= k, and an odd n leaves every row tile ragged"""
    n = k + 11
    return n if n % 2 == 1 else n + 1


def step_longdouble(v, X):
    """(beta = h1 + h2, ||y''||, y'' / ||y''||) of one two-pass step in longdouble"""
    h1, h2, _y1, y2 = dgs_longdouble(v, X)
    nrm = np.sqrt((y2.conj() @ y2).real)
    return h1 + h2, nrm, y2 / nrm


def arnoldi_step_longdouble(d, X):
    """column k of H (k + 1 entries) and x_(k+1) of the Arnoldi step on diag(d) from the k columns of X (arnoldi.fypp:36-62)"""
    h, beta, x = step_longdouble(_long(d) * _long(X[:, -1]), X)
    return np.concatenate([h, [beta]]), x


def lanczos_step_longdouble(d, X):
    """column k of T (k + 1 entries) and x_(k+1) of the Lanczos step on diag(d): the two local projections in sequence (lanczos.fypp:57-60),
    the full step whose coefficients are dropped (:62), the norm (:29)"""
    Xl = _long(X)
    k = X.shape[1]
    v = _long(d) * Xl[:, -1]
    t = np.zeros(k + 1, dtype=Xl.dtype)
    for i in range(max(1, k - 1), k + 1):
        t[i - 1] = Xl[:, i - 1].conj() @ v
        v = v - t[i - 1] * Xl[:, i - 1]
    _h, beta, x = step_longdouble(v, X)
    t[k] = beta
    return t, x


def bidiag_step_longdouble(d, U, V):
    """step k of golub_kahan.fypp:27-52 on diag(d) from the k columns of U and the k - 1 of V: (alpha, v_k, beta, u_(k+1)); A^H = conj(d)"""
    dl = _long(d)
    _h, alpha, v = step_longdouble(dl.conj() * _long(U[:, -1]), V)
    _h, beta, u = step_longdouble(dl * v, U)
    return alpha, v, beta, u


def arnoldi_block_step_longdouble(d, X, p):
    """the kp x p block of H, the p x p factor R and the p new columns of the block Arnoldi step on diag(d) from the kp columns of X
    (arnoldi.fypp:39-55): p products, the block step column by column, qr_no_pivoting of the new block (qr.fypp:129-165)"""
    Xl = _long(X)
    kp = X.shape[1]
    W = _long(d)[:, None] * Xl[:, kp - p:]
    Hb = np.zeros((kp, p), dtype=Xl.dtype)
    for j in range(p):
        h1, h2, _y1, W[:, j] = dgs_longdouble(W[:, j], X)
        Hb[:, j] = h1 + h2
    R = np.zeros((p, p), dtype=Xl.dtype)
    for j in range(p):
        if j > 0:
            h1, h2, _y1, W[:, j] = dgs_longdouble(W[:, j], W[:, :j])
            R[:j, j] = h1 + h2
        R[j, j] = np.sqrt((W[:, j].conj() @ W[:, j]).real)
        W[:, j] = W[:, j] / R[j, j]
    return Hb, R, W


# ---- two routes to the same columns (tests/test_gpu_views.py) ---------------------------------------------------------------------------
def dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def bits(a):
    """the 64-bit words of an array, column by column"""
    return np.ascontiguousarray(np.asarray(a).T).view(np.uint64)


def last_error():
    return _capi.load().lk_last_error().decode()


class TwoRoutes:
    """The same n x w contents A twice.  Route P: an engine-owned panel R of exactly w columns, every operand named as (R, column index).
    Route V: columns [a, a + w) of a wider engine-owned parent, every operand named through an offset view of its own (`P.view`, i.e.
    lk_basis_wrap at col(a + j0)): the handles differ, the memory is one panel.  Both parents come from lk_basis_create with the same n, so
    ld and the alignment of every column agree.  `check` asserts that the two panels hold the same bits afterwards and that the columns
    of the wide parent outside [a, a + w) are untouched; it returns the contents.  `split`: route P holds columns [0, split) and
    [split, w) in two panels (an entry that takes its column count from the handle -- a workspace, U against V -- cannot share one handle
    with its other operands); an operand then lies on one side of the split.

    Route P's panel has its own address and its own ncols, so the comparison holds only where no kernel is chosen from either.  In eager
    mode lk_engine.hip reads a handle's ncols for range checks, for kdim = ncols - 1 of lk_arnoldi / lk_lanczos / lk_bidiag / lk_kexpm
    (`const int kdim = X->ncols - 1`: the same on both routes, the view is made that wide), for lk_arnoldi_block's kdim = (ncols - p) / p and
    for the HOST leading dimension of lk_kexpm's projected matrix (`const int64_t ldh = X->ncols`); hwm is read by the lazy path only
    (lk_vec_dot's batched sweeps, speculative_first_pass).  No kernel or grid is chosen from them, and the columns of both parents start
    on the same 256-byte grid with the same ld."""

    def __init__(self, ctx, A, a=3, tail=2, split=None):
        A = np.asfortranarray(A)
        n, w = A.shape
        self.a, self.w = a, w
        self.split = w if split is None else split
        self.Rs = [lk.krylov_basis_gpu(n, c1 - c0, A.dtype, ctx) for c0, c1 in ((0, self.split), (self.split, w)) if c1 > c0]
        for R, c0 in zip(self.Rs, (0, self.split)):
            R.upload(A[:, c0:c0 + R.ncols])
        self.R = self.Rs[0]
        self.img = basis(n, a + w + tail, A.dtype, 7100)
        self.img[:, a:a + w] = A
        self.P = lk.krylov_basis_gpu(n, a + w + tail, A.dtype, ctx)
        self.P.upload(self.img)
        self._views = []

    def p(self, j0, w):
        assert j0 + w <= self.split or j0 >= self.split
        return (self.Rs[0]._h, j0) if j0 < self.split else (self.Rs[1]._h, j0 - self.split)

    def v(self, j0, w):
        V = self.P.view(self.a + j0, w)
        assert V._h.value != self.P._h.value
        self._views.append(V)
        return V._h, 0

    def routes(self):
        return (self.p, self.v)

    def check(self, what):
        r, g = np.asfortranarray(np.column_stack([R.download() for R in self.Rs])), self.P.download()
        a, w = self.a, self.w
        assert np.array_equal(bits(g[:, a:a + w]), bits(r)), f"{what}: the panel differs between the parent route and the view route"
        out = np.r_[0:a, a + w:g.shape[1]]
        assert np.array_equal(bits(g[:, out]), bits(self.img[:, out])), f"{what}: a column outside the views changed"
        return r


class InterleavedPair:
    """Two n x ncols panels A and B in ONE flat buffer with ld = 2 n_pad: A in rows [0, n) of every column, B wrapped n_pad rows further
    on, so each lives entirely in the other's padding rows (`together`), or the same two panels with the same ld and alignment in two
    buffers of their own (`together = False`).  Every other word is POISON; `get` asserts it still is and returns (A, B)."""

    def __init__(self, ctx, dtype, n, ncols, together):
        dt = np.dtype(dtype)
        es = dt.itemsize
        self.n, self.ncols, self.npad = n, ncols, (n + 31) // 32 * 32
        self.ld = 2 * self.npad
        total = self.ld * ncols
        self.bufs, self.h = [], []
        lib = _capi.load()
        for i in range(1 if together else 2):
            img = np.empty(total, dtype=dt)
            img.view(np.uint64)[:] = POISON
            b = lk.krylov_basis_gpu(total, 1, dt, ctx)
            b.upload(img.reshape(-1, 1))
            self.bufs.append(b)
        for i in range(2):
            b = self.bufs[0 if together else i]
            h = C.c_void_p()
            _capi.check(lib.lk_basis_wrap(ctx._h, _capi.LK_C128 if dt.kind == "c" else _capi.LK_F64, n, ncols, self.ld,
                                          C.c_void_p(b.info()[4] + i * self.npad * es), C.byref(h)))
            self.h.append(lk.krylov_basis_gpu(n, ncols, dt, ctx, _handle=h, _owner=b))
        self.A, self.B = self.h
        self.together, self.dtype = together, dt

    def _rows(self, i, j):
        o = j * self.ld + i * self.npad
        return slice(o, o + self.n)

    def set(self, i, M, col0=0):
        M = np.asarray(M, dtype=self.dtype).reshape(self.n, -1, order="F")
        b = self.bufs[0 if self.together else i]
        buf = b.download()[:, 0]
        for j in range(M.shape[1]):
            buf[self._rows(i, col0 + j)] = M[:, j]
        b.upload(buf.reshape(-1, 1))

    def get(self, what=""):
        out = []
        bufs = [b.download()[:, 0] for b in self.bufs]
        live = [np.zeros(bufs[0].size, dtype=bool) for _ in bufs]
        for i in range(2):
            k = 0 if self.together else i
            out.append(np.asfortranarray(np.stack([bufs[k][self._rows(i, j)] for j in range(self.ncols)], axis=1)))
            for j in range(self.ncols):
                live[k][self._rows(i, j)] = True
        for buf, lv in zip(bufs, live):
            bad = np.flatnonzero(buf[~lv].view(np.uint64) != POISON)
            assert bad.size == 0, f"{what}: {bad.size} words outside both panels changed"
        return out
