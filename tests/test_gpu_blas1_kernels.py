"""The BLAS-1 kernels behind lk_vec_scal / axpby / copy / dot / norm / rand (k_scal, k_axpby, k_copy, k_dot + finish_partials, k_rand of
csrc/lk_kernels.hip.h), each entry by entry against a plain high-precision statement of the same operation, at the sizes where their
grid-stride loops and their cache policy change (tests/_blas1_cases.py states the launch geometry; tests/test_oracle_blas1.py pins the
references and bounds without a GPU).

Loop edges: "blas1_grid_mult" = 1, so the stride is S = num_cu * 256 lanes of 16 bytes; nv = S - 1, S, S + 1, 2S - 1, 2S, 2S + 1, 3S + 1,
4S - 1, 4S, 4S + 1, 5S + 3 lanes -- complex n = nv, real n = 2 nv and 2 nv + 1.  Cache policy: the default multiplier, the last size with
plain accesses, the first with non-temporal ones and a non-temporal one with an odd last element.

  k_scal   real: bit for bit against x * a; complex: per component within gamma(2) of its two products.  The fused normalise (rand(True) and
           the three-sweep lk_dgs with LK_DGS_NORMALIZE) against x / ||x|| in longdouble (check_normalised).
  k_axpby  beta != 0, beta = 0 and beta = 0 onto a y of NaN; real beta = 0 bit for bit, otherwise per component within gamma(2) (real) /
           gamma(3) (complex) of the component's own absolute products (check_axpby); add, sub, chsgn; the lazy queue's single-term flush.
  k_copy   the bytes of a source holding -0.0, a subnormal, +-inf and a NaN with a payload, onto a destination of NaN.
  k_dot    x . y, x . x and ||x|| against the longdouble sums within gamma(m) of sum |x| |y|, m = dot_depth() from the kernels' own tree.
  k_rand   bit for bit against the counter generator, around the wrap of the grid-stride loop, row0 = 0, 1, 10^9 + 1.

Every elementwise operation works on the MIDDLE column of a three-column basis whose neighbours must come back byte-identical; the input of
every operation that is not in place is read back and compared byte by byte; one odd real and one complex non-temporal size run again on a
caller-owned panel whose padding rows [n, ld) hold a NaN payload no arithmetic produces.  The worst ratio of every case goes to
$LK_TOL_REPORT."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import lightkrylov_amd as lk
from oracle import oracle as ora
from tests._blas1_cases import (ALPHA, BETA, DEFAULT_MULT, MAX_GRID, POLICY_N, RAND_ROW0, assert_same_bytes, check_axpby, check_normalised,
                                check_scal, deep_size, dot_depth, dot_references, edge_sizes, is_nt, lanes, nan_vector, rand_reference,
                                rand_stride, special_source, stride, three_columns, vectors)
from tests._gpu_helpers import KINDS, CallerPanel, check_entrywise, device_num_cu, is_cplx

pytestmark = pytest.mark.gpu

RESTORE = dict(blas1_grid_mult=DEFAULT_MULT, lazy=0, resident=1)
CASES = [("loop_edges", None), ("cache_policy", 0), ("cache_policy", 1), ("cache_policy", 2)]
CASE_IDS = ["loop_edges", "last_plain", "first_non_temporal", "non_temporal_odd"]


@pytest.fixture(scope="module")
def kctx():
    c = lk.Context(device=0)
    c.set_tuning("blas1_grid_mult", DEFAULT_MULT)                  # the default, stated: the cache-policy sizes and dot_depth() depend on it
    yield c
    for k, v in RESTORE.items():
        c.set_tuning(k, v)
    c.close()


@contextlib.contextmanager
def tuned(c, **keys):
    try:
        for k, v in keys.items():
            c.set_tuning(k, v)
        yield c
    finally:
        for k in keys:
            c.set_tuning(k, RESTORE[k])


def _name(dtype):
    return np.dtype(dtype).name


def _sizes(c, case, dtype):
    """(the sizes of the case, its "blas1_grid_mult")"""
    group, i = case
    if group == "loop_edges":
        return edge_sizes(device_num_cu(c) * 256, dtype), 1
    return (POLICY_N[dtype][i],), DEFAULT_MULT


class Mid:
    """a vector as the middle column of a three-column basis between two live neighbours"""

    def __init__(self, c, mid, extra_ld=0):
        self.img = three_columns(mid)
        self.B = lk.krylov_basis_gpu(self.img.shape[0], 3, self.img.dtype, c)
        self.B.upload(self.img)
        self.v = self.B[1]

    def reset(self, mid):
        self.img[:, 1] = mid
        self.B.upload(np.ascontiguousarray(mid).reshape(-1, 1), 1)

    def mid(self):
        """the middle column alone (a one-column read: what a lazy context flushes for)"""
        return self.B.download(1, 1)[:, 0]

    def _all(self, what):
        return self.B.download()

    def read(self, what):
        got = self._all(what)
        for j in (0, 2):
            assert_same_bytes(got[:, j], self.img[:, j], f"{what}: neighbouring column {j}")
        return np.ascontiguousarray(got[:, 1])

    def unchanged(self, what):
        assert_same_bytes(self.read(what), self.img[:, 1], f"{what}: the input vector")


class PanelMid(Mid):
    """the same inside a caller-owned panel (lk_basis_wrap) with ld > n: reading it back asserts that no word of rows [n, ld) changed"""

    def __init__(self, c, mid, extra_ld=0):
        self.img = three_columns(mid)
        self.P = CallerPanel(c, self.img.dtype, self.img.shape[0], 3, "nan_pad", extra_ld=extra_ld)
        assert self.P.ld > self.P.n
        self.P.set(self.img)
        self.B = self.P.B
        self.v = self.B[1]

    def reset(self, mid):
        self.img[:, 1] = mid
        self.P.set(np.ascontiguousarray(mid).reshape(-1, 1), col0=1)

    def _all(self, what):
        return self.P.get(what)


# ---- one operation on vectors made by `make` (Mid or PanelMid): each returns the worst ratio to its bound ------------------------------------

def _run_scal(make, c, n, dtype, label):
    x, _ = vectors(n, dtype)
    m = make(c, x)
    m.v.scal(ALPHA[dtype])
    return check_scal(m.read(label), x, ALPHA[dtype], label)


def _run_axpby(make, c, n, dtype, label):
    x, y = vectors(n, dtype)
    a = ALPHA[dtype]
    mx, my = make(c, x), make(c, y, extra_ld=2)
    worst = 0.0
    for what, beta, y0 in (("beta != 0", BETA[dtype], y), ("beta = 0", 0.0, y), ("beta = 0 onto NaN", 0.0, nan_vector(n, dtype))):
        my.reset(y0)
        my.v.axpby(a, mx.v, beta)
        worst = max(worst, check_axpby(my.read(f"{label} {what}"), a, x, beta, y0, f"{label} {what}"))
        mx.unchanged(f"{label} {what}")
    return worst


def _run_copy(make, c, n, dtype, label):
    src = special_source(n, dtype)
    ms, md = make(c, src), make(c, nan_vector(n, dtype), extra_ld=2)
    assert md.B.info()[3] != ms.B.info()[3] or make is Mid         # caller panels: two different leading dimensions
    lk.copy(md.v, ms.v)
    assert_same_bytes(md.read(label), src, label)
    ms.unchanged(label)
    return 0.0


def _check_dot(got, ref, scale, m, cp, label):
    return check_entrywise(np.array([got]), np.array([ref]), np.array([scale]), m, cp, label)


def _run_dot(make, c, n, dtype, mult, label):
    """x . y and x . x within gamma(m) of sum |x| |y| (check_entrywise; complex: its 2 gamma(2 m + 5) of sum (|xr| + |xi|)(|yr| + |yi|)),
    m = dot_depth().  ||x|| = sqrt(hypot(re, im)) of x . x: the sum's relative error gamma(m) is halved by the root, the imaginary part is
    at most rounding noise whose square vanishes, hypot and the root round once or twice each: |got - ||x||| <= gamma(m + 3) ||x||."""
    cp = is_cplx(dtype)
    x, y = vectors(n, dtype)
    mx, my = make(c, x), make(c, y, extra_ld=2)
    m = dot_depth(n, dtype, device_num_cu(c), mult)
    xy, xy_scale, xx, xx_scale, nrm = dot_references(n, dtype)
    worst = max(_check_dot(mx.v.dot(my.v), xy, xy_scale, m, cp, f"{label} x.y"),
                _check_dot(mx.v.dot(mx.v), xx, xx_scale, m, cp, f"{label} x.x"),
                _check_dot(mx.v.norm(), nrm, float(nrm), m + 3, False, f"{label} norm"))
    mx.unchanged(label)
    my.unchanged(label)
    return worst


def _run_rand(make, c, n, dtype, row0, label, seed=77):
    """real kind: the oracle's generator from counter row0; complex kind: the numpy generator written from the header's formula"""
    m = make(c, nan_vector(n, dtype))
    lk._capi.check(m.v._lib.lk_vec_rand(m.v.basis._h, m.v.col, C.c_uint64(seed), C.c_int64(row0), 0))
    if is_cplx(dtype):
        want = rand_reference(n, dtype, seed, row0)
    else:
        want = np.empty(n)
        ora.fill_counter(want, seed, i0=row0)
    assert_same_bytes(m.read(label), want, label)
    return 0.0


def _run_normalise_rand(make, c, n, dtype, mult, label, seed=91):
    """rand(True): k_rand, k_dot + finish_partials, then k_scal reads ||x||^2 on the device.  x is the generator's stream (k_rand is compared
    bit for bit above); the bound is check_normalised's with the dot's depth."""
    m = make(c, nan_vector(n, dtype))
    m.v.rand(True, seed=seed)
    return check_normalised(m.read(label), rand_reference(n, dtype, seed, 0), dot_depth(n, dtype, device_num_cu(c), mult), label)


def _run_normalise_dgs(make, c, n, dtype, label):
    """lk_dgs(k = 1, LK_DGS_NORMALIZE) on the three sweeps against X = e_0: h = x_0 and y'' = x with entry 0 zeroed are EXACT (products with 1
    and 0), so k_scal normalises a known vector.  Its ||y''||^2 comes from the third sweep, not from k_dot; whatever that sweep's order, a
    sum of n positive terms is within gamma(n) of itself: check_normalised with m = n (5e-10 per entry at n = 4e6; a lane stored in the
    wrong place is off by the size of the entry)."""
    x, _ = vectors(n, dtype)
    e0 = np.zeros((n, 1), dtype=dtype)
    e0[0] = 1.0
    E = lk.krylov_basis_gpu(n, 1, dtype, c)
    E.upload(e0)
    m = make(c, x)
    h = np.zeros(1, dtype=dtype)
    with tuned(c, resident=0):
        info = lk.double_gram_schmidt_step(m.v, E, False, h, _normalize=True)
    assert info == 0 and h[0] == x[0], (info, h[0], x[0])
    x1 = x.copy()
    x1[0] = 0.0
    got = m.read(label)
    assert got[0] == 0.0, label
    return check_normalised(got, x1, n, label)


# ---- every kernel at every loop edge and either side of the cache-policy switch ----------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("dtype", KINDS)
def test_scal_entry_by_entry(kctx, dtype, case):
    sizes, mult = _sizes(kctx, case, dtype)
    with tuned(kctx, blas1_grid_mult=mult):
        worst = max(_run_scal(Mid, kctx, n, dtype, f"k_scal n={n} {_name(dtype)}") for n in sizes)
    print(f"k_scal {_name(dtype)} {case[0]}: worst ratio to the bound {worst:.3f}")


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("dtype", KINDS)
def test_axpby_entry_by_entry(kctx, dtype, case):
    sizes, mult = _sizes(kctx, case, dtype)
    with tuned(kctx, blas1_grid_mult=mult):
        worst = max(_run_axpby(Mid, kctx, n, dtype, f"k_axpby n={n} {_name(dtype)}") for n in sizes)
    print(f"k_axpby {_name(dtype)} {case[0]}: worst ratio to the bound {worst:.3f}")


@pytest.mark.parametrize("dtype", KINDS)
def test_add_sub_chsgn_at_a_deep_loop_size(kctx, dtype):
    """add = axpby(1, x, 1), sub = axpby(-1, x, 1), chsgn = scal(-1) (AbstractVectors.fypp:434-460) at nv = 5 S + 3: the products with +-1
    are exact, so the real kind is x + y, y - x and -y bit for bit; the complex kind within check_axpby's bound"""
    n = deep_size(device_num_cu(kctx) * 256, dtype)
    x, y = vectors(n, dtype)
    label = f"k_axpby add/sub/chsgn n={n} {_name(dtype)}"
    with tuned(kctx, blas1_grid_mult=1):
        mx, my = Mid(kctx, x), Mid(kctx, y)
        my.v.add(mx.v)
        y1 = my.read(label + " add")
        check_axpby(y1, 1.0, x, 1.0, y, label + " add")
        my.v.sub(mx.v)
        y2 = my.read(label + " sub")
        check_axpby(y2, -1.0, x, 1.0, y1, label + " sub")
        my.v.chsgn()
        y3 = my.read(label + " chsgn")
        mx.unchanged(label)
    if not is_cplx(dtype):
        assert_same_bytes(y1, x + y, label + " add")
        assert_same_bytes(y2, y1 - x, label + " sub")
    assert np.array_equal(y3, -y2), label + " chsgn"


@pytest.mark.parametrize("dtype", KINDS)
def test_single_term_flush_of_the_lazy_queue_takes_the_blas1_route(kctx, dtype):
    """materialise_queue with ONE queued term launches k_axpby itself (cg's update pattern): y.axpby(a, X[j], 1) then a read of y (b = 1), and
    y.zero(); y.axpby(a, X[j], 1) then a read (b = 0: y's memory, NaN here, is never read), X a three-column panel, at nv = 5 S + 3 and at
    a non-temporal size.  The counters show the route: lk_lazy_stats[3] (queue flushes) advances by one each time, lk_lazy_fusion_stats[3]
    (virtual temporaries written after all) for the zeroed one only."""
    a = ALPHA[dtype]
    for n, mult in ((deep_size(device_num_cu(kctx) * 256, dtype), 1), (POLICY_N[dtype][2], DEFAULT_MULT)):
        x, y = vectors(n, dtype)
        label = f"k_axpby lazy flush n={n} {_name(dtype)}"
        with tuned(kctx, blas1_grid_mult=mult, lazy=1):
            mx, my = Mid(kctx, x), Mid(kctx, y)
            lazy0, fus0 = kctx.lazy_stats(), kctx.lazy_fusion_stats()
            my.v.axpby(a, mx.v, 1.0)
            assert kctx.lazy_stats()[2] == lazy0[2] + 1 and kctx.lazy_stats()[3] == lazy0[3], label      # queued, nothing launched yet
            got = my.mid()
            assert kctx.lazy_stats()[3] == lazy0[3] + 1 and kctx.lazy_fusion_stats()[3] == fus0[3], label
            check_axpby(got, a, x, 1.0, y, label + " b=1")
            my.img[:, 1] = got
            my.unchanged(label + " b=1")
            mx.unchanged(label + " b=1")
            my.reset(nan_vector(n, dtype))
            lazy0, fus0 = kctx.lazy_stats(), kctx.lazy_fusion_stats()
            my.v.zero()
            my.v.axpby(a, mx.v, 1.0)
            got = my.mid()
            assert kctx.lazy_stats()[3] == lazy0[3] + 1 and kctx.lazy_fusion_stats()[3] == fus0[3] + 1, label
            check_axpby(got, a, x, 0.0, nan_vector(n, dtype), label + " b=0")
            my.img[:, 1] = got
            my.unchanged(label + " b=0")
            mx.unchanged(label + " b=0")


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("dtype", KINDS)
def test_copy_byte_for_byte(kctx, dtype, case):
    sizes, mult = _sizes(kctx, case, dtype)
    with tuned(kctx, blas1_grid_mult=mult):
        for n in sizes:
            _run_copy(Mid, kctx, n, dtype, f"k_copy n={n} {_name(dtype)}")


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("dtype", KINDS)
def test_dot_and_norm_against_the_longdouble_sum(kctx, dtype, case):
    sizes, mult = _sizes(kctx, case, dtype)
    with tuned(kctx, blas1_grid_mult=mult):
        worst = max(_run_dot(Mid, kctx, n, dtype, mult, f"k_dot n={n} {_name(dtype)}") for n in sizes)
    print(f"k_dot {_name(dtype)} {case[0]}: worst ratio to the bound {worst:.3f}")


@pytest.mark.parametrize("dtype", KINDS)
def test_dot_with_the_grid_capped_at_the_partial_buffer(kctx, dtype):
    """"blas1_grid_mult" = 64: num_cu * 64 blocks exceed MAX_GRID = 4096, the dot's grid is capped there and every lane of finish_partials
    adds 64 partials"""
    n = POLICY_N[dtype][2]
    assert stride(n, dtype, device_num_cu(kctx), 64, dot=True) == MAX_GRID * 256
    with tuned(kctx, blas1_grid_mult=64):
        worst = _run_dot(Mid, kctx, n, dtype, 64, f"k_dot n={n} blas1_grid_mult=64 {_name(dtype)}")
    print(f"k_dot {_name(dtype)} capped grid: worst ratio to the bound {worst:.3f}")


@pytest.mark.parametrize("dtype", KINDS)
def test_rand_around_the_wrap_of_the_grid_stride_loop(kctx, dtype):
    """k_rand takes one ELEMENT per thread and round: n = S - 1, S, S + 1 and 3 S + 5 elements at "blas1_grid_mult" = 1, row0 = 0, 1 and
    10^9 + 1 (the complex counters 2 g and 2 g + 1 beyond 2^31) through lk_vec_rand's own argument"""
    S = device_num_cu(kctx) * 256
    with tuned(kctx, blas1_grid_mult=1):
        for n in (S - 1, S, S + 1, 3 * S + 5):
            assert rand_stride(n, device_num_cu(kctx), 1) == S                       # the grid is at its cap from n = S - 1 on
            for row0 in RAND_ROW0:
                _run_rand(Mid, kctx, n, dtype, row0, f"k_rand n={n} row0={row0} {_name(dtype)}")


@pytest.mark.parametrize("dtype", KINDS)
def test_fused_normalise_entry_by_entry(kctx, dtype):
    """k_scal with inv_sqrt_of: rand(True) and the three-sweep lk_dgs with LK_DGS_NORMALIZE, at nv = 5 S + 3 and at a non-temporal size"""
    worst = 0.0
    for n, mult in ((deep_size(device_num_cu(kctx) * 256, dtype), 1), (POLICY_N[dtype][2], DEFAULT_MULT)):
        assert lanes(n, dtype) > stride(n, dtype, device_num_cu(kctx), mult) and (mult == 1) != is_nt(n, dtype)
        with tuned(kctx, blas1_grid_mult=mult):
            worst = max(worst, _run_normalise_rand(Mid, kctx, n, dtype, mult, f"k_scal normalise rand(True) n={n} {_name(dtype)}"),
                        _run_normalise_dgs(Mid, kctx, n, dtype, f"k_scal normalise lk_dgs n={n} {_name(dtype)}"))
    print(f"k_scal normalise {_name(dtype)}: worst ratio to the bound {worst:.3f}")


# ---- caller-owned panels with live padding ---------------------------------------------------------------------------------------------------

PANEL_KERNELS = ("scal", "axpby", "copy", "dot", "rand", "normalise")


@pytest.mark.parametrize("kernel", PANEL_KERNELS)
@pytest.mark.parametrize("dtype", KINDS)
def test_kernels_leave_the_padding_of_a_caller_panel_alone(kctx, dtype, kernel):
    """n = 4 194 305 (real, odd) / 2 097 153 (complex), non-temporal, on the middle column of a three-column panel wrapped inside a buffer
    whose rows [n, ld) hold a NaN payload (two panels with different ld where the operation has two operands): the checks above, the
    neighbours, and every word outside the panel's rows bit-identical (CallerPanel.get)."""
    n = POLICY_N[dtype][2]
    assert is_nt(n, dtype) and (is_cplx(dtype) or n & 1)
    label = f"caller panel: k_{kernel} n={n} {_name(dtype)}"
    if kernel == "scal":
        _run_scal(PanelMid, kctx, n, dtype, label)
    elif kernel == "axpby":
        _run_axpby(PanelMid, kctx, n, dtype, label)
    elif kernel == "copy":
        _run_copy(PanelMid, kctx, n, dtype, label)
    elif kernel == "dot":
        _run_dot(PanelMid, kctx, n, dtype, DEFAULT_MULT, label)
    elif kernel == "rand":
        _run_rand(PanelMid, kctx, n, dtype, 10 ** 9 + 1, label)
    else:
        _run_normalise_rand(PanelMid, kctx, n, dtype, DEFAULT_MULT, label)
        _run_normalise_dgs(PanelMid, kctx, n, dtype, label)
