"""Sizes, inputs, longdouble references and bounds of the BLAS-1 kernel tests (k_scal, k_axpby, k_copy, k_dot + finish_partials, k_rand of
csrc/lk_kernels.hip.h): tests/test_gpu_blas1_kernels.py runs them on the engine, tests/test_oracle_blas1.py pins them without a GPU.

The launch geometry, restated from csrc/lk_engine.hip (blas1_grid, blas1_nt, dot_device): a vector of n elements is nv = n ed / 2 lanes of 16
bytes (ed = 1 real, 2 complex) plus, for an odd real n, one last element that thread 0 handles alone.  The grid is min(ceil((nv + 1) / 256),
num_cu * blas1_grid_mult) blocks of 256 threads (the dot: at most MAX_GRID = 4096 as well), so the grid stride is at most
S = num_cu * blas1_grid_mult * 256 lanes; thread t handles lanes t, t + S, t + 2 S, ...  The two-element loops (k_scal, k_axpby with beta = 0,
k_dot, k_copy's non-temporal loop) take lanes i and i + S while i + S < nv, the norm loop of k_dot (x == y) four lanes while i + 3 S < nv, and
a tail loop takes what is left.  Non-temporal accesses start at n ed 8 >= 32 MiB."""
import functools

import numpy as np

from tests._gpu_helpers import ext, gamma, is_cplx, seeded
from tests._operator_cases import check_complex_diag
from tests._tol import _report

NT_BYTES = 32 << 20
MAX_GRID = 4096
CPU_NUM_CU = 256                                   # tests/test_oracle_blas1.py: S = 65 536 lanes at blas1_grid_mult = 1
DEFAULT_MULT = 2
POLICY_N = {np.float64: (4_194_303, 4_194_304, 4_194_305),         # last plain | first non-temporal | non-temporal with an odd last element
            np.complex128: (2_097_151, 2_097_152, 2_097_153)}
ALPHA = {np.float64: 0.37, np.complex128: 0.37 - 1.2j}              # (the scalars of tests/test_gpu_parity.py: both parts non-zero)
BETA = {np.float64: -1.5, np.complex128: -1.5 + 0.25j}
RAND_ROW0 = (0, 1, 10 ** 9 + 1)


def ed(dtype):
    return 2 if is_cplx(dtype) else 1


def lanes(n, dtype):
    return n * ed(dtype) // 2


def is_nt(n, dtype):
    return n * ed(dtype) * 8 >= NT_BYTES


def edge_lanes(S):
    """for each loop the last size that does not enter it, the first that does, sizes where every thread runs the unrolled loop and the tail,
    and sizes where only some threads do"""
    return (S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 3 * S + 1, 4 * S - 1, 4 * S, 4 * S + 1, 5 * S + 3)


def edge_sizes(S, dtype):
    """n of the loop-edge cases: complex n = nv; real n = 2 nv and 2 nv + 1 (the odd last element on top of a deep loop)"""
    if is_cplx(dtype):
        return tuple(edge_lanes(S))
    return tuple(n for nv in edge_lanes(S) for n in (2 * nv, 2 * nv + 1))


def deep_size(S, dtype):
    """nv = 5 S + 3: three rounds of a two-element loop (the third for three threads only), one round of the four-element loop and a tail;
    odd for the real kind"""
    return 5 * S + 3 if is_cplx(dtype) else 2 * (5 * S + 3) + 1


def grid(nvec, num_cu, mult):
    return int(max(1, min(-(-nvec // 256), num_cu * mult)))


def stride(n, dtype, num_cu, mult, dot=False):
    """grid stride in lanes of the kernels launched on nv + 1 (scal, axpby, copy; `dot`: capped at MAX_GRID blocks)"""
    g = grid(lanes(n, dtype) + 1, num_cu, mult)
    return 256 * (min(g, MAX_GRID) if dot else g)


def rand_stride(n, num_cu, mult):
    """k_rand is launched on n ELEMENTS (one element per thread and round)"""
    return 256 * grid(n, num_cu, mult)


def dot_depth(n, dtype, num_cu, mult):
    """The number of roundings m on the longest path from a product to the result of k_dot + finish_partials, from the kernels' own tree:
      L = ceil(nv / stride) lanes per thread, accumulated one after the other into a two-component accumulator (norm loop: a0 .. a3 in
          order too): the first product starts from zero, so a real component's chain is its product's rounding and L - 1 additions = L
          (a fused multiply-add only removes roundings); a complex term is two products and their sum before it is added: L + 2;
      real kind: + 1 for acc.x + acc.y, + 1 for the odd last element added to thread 0's acc.x first (together the complex kind's + 2);
      wave_sum: four DPP additions and (r0 + r1) + (r2 + r3) = 6;  the four waves of a block: (w0 + w1) + (w2 + w3) = 2;
      finish_partials: P = ceil(g / 64) partials per lane, one after the other, = P;  its wave_sum = 6.
    m = L + P + 16 for both kinds.  At the defaults and n = 4 194 304: L = 16, P = 8, m = 40 against n = 4e6 products."""
    s = stride(n, dtype, num_cu, mult, dot=True)
    L = max(1, -(-lanes(n, dtype) // s))
    P = -(-(s // 256) // 64)
    return L + P + 16


# ---- inputs, shared and read-only ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=12)
def vectors(n, dtype):
    """(x, y) from the counter streams 8101 and 8102"""
    x, y = seeded(n, dtype, 8101), seeded(n, dtype, 8102)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=12)
def neighbours(n, dtype):
    """columns 0 and 2 of the three-column bases whose middle column the kernels work on (streams 8103 and 8104)"""
    a, b = seeded(n, dtype, 8103), seeded(n, dtype, 8104)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def three_columns(mid, dtype=None):
    """an n x 3 column-major image with `mid` between the two neighbour columns"""
    mid = np.asarray(mid)
    dtype = mid.dtype if dtype is None else np.dtype(dtype)
    a, b = neighbours(mid.shape[0], dtype.type)
    return np.asfortranarray(np.stack([a, mid.astype(dtype, copy=False), b], axis=1))


def nan_vector(n, dtype):
    """every component a NaN: an entry a kernel leaves out shows"""
    return np.full(n, np.nan + (1j * np.nan if is_cplx(dtype) else 0), dtype=dtype)


def special_source(n, dtype):
    """the x of vectors() with -0.0, a subnormal, +-inf and a NaN with a payload at the first and last rows, either side of the middle and at
    rows 7 .. 11 (n >= 32): a copy is a copy of BYTES"""
    x = vectors(n, dtype)[0].copy()
    w = x.view(np.uint64)
    specials = np.array([0x8000000000000000, 0x0000000000000123, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF80000DEADBEEF], dtype=np.uint64)
    for start in (0, 7, len(w) // 2 - 2, len(w) - 5):
        w[start:start + 5] = specials
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def dot_references(n, dtype):
    """(x . y, its scale sum |x| |y|, x . x, its scale, ||x||) in longdouble: conj(x) on the left; the complex scale is product_scale's
    sum (|xr| + |xi|)(|yr| + |yi|).  numpy sums longdoubles pairwise: about log2(n) + 8 roundings of 2^-64, 2^-11 of one double rounding."""
    x, y = vectors(n, dtype)
    xe, ye = ext(x), ext(y)
    if is_cplx(dtype):
        ax, ay = np.abs(x.real) + np.abs(x.imag), np.abs(y.real) + np.abs(y.imag)
    else:
        ax, ay = np.abs(x), np.abs(y)
    xx = (xe.conj() * xe).sum()
    return (xe.conj() * ye).sum(), float(ax @ ay), xx, float(ax @ ax), np.sqrt(xx.real)


# ---- the counter generator, from the formula of include/lightkrylov_hip.h alone ---------------------------------------------------------------

def splitmix_u01(seed, ctr):
    """u = (splitmix64(seed 2^32 + ctr) >> 11) 2^-53 for an array of uint64 counters (arithmetic modulo 2^64)"""
    ctr = np.asarray(ctr, dtype=np.uint64)
    z = ctr + np.uint64(((int(seed) << 32) + 0x9E3779B97F4A7C15) % 2 ** 64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def rand_reference(n, dtype, seed, row0):
    """entry i (global row row0 + i) = 2 u - 1; ctr = row for the real kind, 2 row (real part) and 2 row + 1 (imaginary part) for the complex"""
    rows = np.uint64(row0) + np.arange(n, dtype=np.uint64)
    if not is_cplx(dtype):
        return 2.0 * splitmix_u01(seed, rows) - 1.0
    out = np.empty(n, dtype=np.complex128)
    out.real = 2.0 * splitmix_u01(seed, np.uint64(2) * rows) - 1.0
    out.imag = 2.0 * splitmix_u01(seed, np.uint64(2) * rows + np.uint64(1)) - 1.0
    return out


# ---- checks: each returns the worst ratio to its bound (0.0 where the comparison is bit for bit) ---------------------------------------------

def first_difference(got, want):
    """index of the first element whose bytes differ, or None"""
    g, w = np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(want).view(np.uint64)
    assert g.shape == w.shape
    bad = np.flatnonzero(g != w)
    return int(bad[0]) if bad.size else None


def assert_same_bytes(got, want, label):
    i = first_difference(got, want)
    assert i is None, f"{label}: 8-byte word {i} is {np.ascontiguousarray(got).view(np.uint64)[i]:#x}, expected {np.ascontiguousarray(want).view(np.uint64)[i]:#x}"


def check_scal(got, x, a, label):
    """x <- a x.  Real kind: one multiplication per entry, bit for bit.  Complex kind: per component within gamma(2) of its two products
    (check_complex_diag with the constant diagonal a)."""
    if not is_cplx(x.dtype):
        assert_same_bytes(got, x * a, label)
        return 0.0
    return check_complex_diag(got, np.full(x.shape, a, dtype=x.dtype), x, False, label)


def check_axpby(got, a, x, b, y, label):
    """y <- a x + b y, per entry (per component for the complex kind) within gamma(d) of that component's own absolute products.  The kernel's
    expression is r = a x; r += b y (cmul for the complex kind: two products and their sum or difference per component), so the deepest path
    is: real d = 2 (a product's rounding, the addition), complex d = 3 (a product, the sum inside cmul, the addition); contraction to fused
    multiply-adds only removes roundings.  b = 0 (the kernel then never reads y): the real kind bit for bit against a x, the complex kind as
    check_scal (d = 2)."""
    if b == 0:
        return check_scal(got, x, a, label)
    cp = is_cplx(x.dtype)
    ref = ext(np.asarray(a)) * ext(x) + ext(np.asarray(b)) * ext(y)
    e = np.asarray(got).astype(ref.dtype) - ref
    if cp:
        ar, ai, br, bi = abs(a.real), abs(a.imag), abs(b.real), abs(b.imag)
        xr, xi, yr, yi = np.abs(x.real), np.abs(x.imag), np.abs(y.real), np.abs(y.imag)
        parts = ((e.real, ar * xr + ai * xi + br * yr + bi * yi), (e.imag, ar * xi + ai * xr + br * yi + bi * yr))
        g = float(gamma(3))
    else:
        parts = ((e, abs(a) * np.abs(x) + abs(b) * np.abs(y)),)
        g = float(gamma(2))
    ratio = 0.0
    for err, scale in parts:
        err, bound = np.abs(err).astype(np.float64), g * scale
        bad = ~(err <= bound)
        assert not bad.any(), f"{label}: entry {int(np.flatnonzero(bad)[0])} off by {err[bad][0]:.3e} > bound {bound[bad][0]:.3e}"
        ratio = max(ratio, float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0)
    _report(label, ratio, 1.0, f"gamma({3 if cp else 2}) per component")
    return ratio


def check_normalised(got, x, m, label):
    """x / ||x|| as k_scal's fused normalise forms it from a device-side ||x||^2 of summation depth m: s = ||x||^2 (1 + t), |t| <= gamma(m)
    (every term is positive, so the scale of the sum is the sum); nr = sqrt(s) (1 + d1) = ||x|| (1 + t)^(1/2) (1 + d1); ar = (1 / nr) (1 + d2);
    x_i ar (1 + d3) -- for the complex kind ar x_r - 0 x_i, one rounding as well.  |got_i - x_i / ||x||| <= gamma(m + 3) |x_i| / ||x||,
    per component, the reference norm and quotient in longdouble."""
    xf = np.ascontiguousarray(x).view(np.float64)
    xe = xf.astype(np.longdouble)
    ref = xe / np.sqrt((xe * xe).sum())
    err = np.abs(np.ascontiguousarray(got).view(np.float64).astype(np.longdouble) - ref).astype(np.float64)
    bound = float(gamma(m + 3)) * np.abs(ref).astype(np.float64)
    bad = ~(err <= bound)
    assert not bad.any(), f"{label}: component {int(np.flatnonzero(bad)[0])} off by {err[bad][0]:.3e} > bound {bound[bad][0]:.3e}"
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    _report(label, ratio, 1.0, f"gamma({m} + 3) per component")
    return ratio
