"""Shared helpers of the GPU test files (test infrastructure: inputs come from the oracle's counter RNG, so CPU and GPU see identical data)."""
import ctypes as C
import functools

import numpy as np

import lightkrylov_amd as lk
from lightkrylov_amd import _capi
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
    rows, "unpadded" ld = n; `extra_ld` (even) more padding rows per column, for two panels of one shape with different ld."""

    def __init__(self, ctx, dtype, n, ncols, layout, seed=0, extra_ld=0):
        dt = np.dtype(dtype)
        cplx = dt.kind == "c"
        es = dt.itemsize
        if layout == "unpadded":
            assert (n % 2 == 1) == cplx, "fit() the size first"
            ld, head = n, 16 // es
        else:
            ld = n + (3 if cplx else 3 + (n + 3) % 2) + extra_ld
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
