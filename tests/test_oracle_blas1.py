"""What tests/test_gpu_blas1_kernels.py compares the BLAS-1 kernels with, checked without a GPU (tests/_blas1_cases.py holds the shared parts).

At the loop-edge sizes for S = 65 536 lanes (256 compute units, "blas1_grid_mult" = 1) and at the six cache-policy sizes:
  * plain double numpy evaluations of every operation -- for axpby both orders that contraction to fused multiply-adds allows, for the dot an
    emulation of the kernels' own summation tree -- stay within the stated bounds of the longdouble references: the bounds can be met;
  * numpy emulations of subtly wrong kernels (one wrong index in an unrolled loop, a forgotten term, a skipped last element, a wrong counter)
    exceed the bounds or break bit equality at every size at which the mutated loop runs: the bounds are not vacuous;
  * the dot's summation depth is a small fraction of the number of products;
  * the numpy counter generator written from the header's formula reproduces the oracle's real-kind stream."""
import numpy as np
import pytest

from oracle import oracle as ora
from tests._blas1_cases import (ALPHA, BETA, CPU_NUM_CU, DEFAULT_MULT, POLICY_N, RAND_ROW0, check_axpby, check_normalised, check_scal,
                                deep_size, dot_depth, dot_references, edge_lanes, edge_sizes, first_difference, is_nt, lanes, nan_vector,
                                rand_reference, rand_stride, special_source, stride, vectors)
from tests._gpu_helpers import KINDS, check_entrywise, ext, is_cplx, seeded

S1 = CPU_NUM_CU * 256                                # the stride of the loop-edge cases


def _cases(dtype):
    """(n, blas1_grid_mult) of every case of the GPU file"""
    return [(n, 1) for n in edge_sizes(S1, dtype)] + [(n, DEFAULT_MULT) for n in POLICY_N[dtype]]


def _name(dtype):
    return np.dtype(dtype).name


def _as_lanes(v):
    """(the nv x 2 doubles of the 16-byte lanes -- a view --, the odd last double or None)"""
    f = np.ascontiguousarray(v).view(np.float64)
    nv = f.size // 2
    return f[:2 * nv].reshape(nv, 2), (f[-1:] if f.size & 1 else None)


def _second_repeats_first(out, src, s, f):
    """the mutant of a two-element loop: lane i + s receives f(lane i) for every round i, i + s of the loop (every lane of an odd round)"""
    o, _ = _as_lanes(out)
    fs, _ = _as_lanes(f(src))
    for r in range(1, -(-o.shape[0] // s), 2):
        hi = min((r + 1) * s, o.shape[0])
        o[r * s:hi] = fs[(r - 1) * s:(r - 1) * s + hi - r * s]


def _detected(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


# ---- scal, axpby, copy ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", KINDS)
def test_scal_reference_and_its_mutants(dtype):
    a = ALPHA[dtype]
    for n, mult in _cases(dtype):
        x, _ = vectors(n, dtype)
        s = stride(n, dtype, CPU_NUM_CU, mult)
        good = x * a
        check_scal(good, x, a, f"numpy scal n={n}")
        twice = good.copy()
        _second_repeats_first(twice, x, s, lambda v: v * a)
        assert _detected(check_scal, twice, x, a, "f(v0) stored twice") == (lanes(n, dtype) > s), n
        if n & 1 and not is_cplx(dtype):
            skipped = good.copy()
            skipped[-1] = x[-1]
            assert _detected(check_scal, skipped, x, a, "odd last element skipped"), n


def _axpby_orders(a, x, b, y):
    """fl(fl(a x) + fl(b y)) (numpy's own), and the contracted form r = fl(a x); fma(b, y, r) with the 64-bit product of a longdouble standing
    in for the fused multiply-add's unrounded one (real kind; the complex kind contracts inside cmul in ways numpy cannot spell: its second
    form is the longdouble expression rounded once, the fewest roundings any contraction can reach)"""
    plain = a * x + b * y
    if is_cplx(x.dtype):
        return plain, (ext(np.asarray(a)) * ext(x) + ext(np.asarray(b)) * ext(y)).astype(x.dtype)
    return plain, (ext(np.asarray(b)) * ext(y) + ext(a * x)).astype(x.dtype)


@pytest.mark.parametrize("dtype", KINDS)
def test_axpby_reference_and_its_mutants(dtype):
    a, b = ALPHA[dtype], BETA[dtype]
    for n, mult in _cases(dtype):
        x, y = vectors(n, dtype)
        s = stride(n, dtype, CPU_NUM_CU, mult)
        for got in _axpby_orders(a, x, b, y):
            check_axpby(got, a, x, b, y, f"numpy axpby n={n}")
        good0 = a * x
        check_axpby(good0, a, x, 0.0, nan_vector(n, dtype), f"numpy axpby beta=0 n={n}")
        twice = good0.copy()
        _second_repeats_first(twice, x, s, lambda v: v * a)
        assert _detected(check_axpby, twice, a, x, 0.0, y, "ax(a0) stored twice") == (lanes(n, dtype) > s), n
        if is_nt(n, dtype):                                        # the non-temporal beta != 0 loop forgets r += by(b)
            assert _detected(check_axpby, a * x, a, x, b, y, "beta term dropped"), n
        if n & 1 and not is_cplx(dtype):
            for beta, good in ((b, a * x + b * y), (0.0, good0)):
                skipped = good.copy()
                skipped[-1] = y[-1]
                assert _detected(check_axpby, skipped, a, x, beta, y, "odd last element skipped"), n
        left_out = good0.copy()                                    # beta = 0 on a NaN y: an entry nobody wrote fails
        left_out[n // 2] = np.nan
        assert _detected(check_axpby, left_out, a, x, 0.0, y, "entry left as NaN"), n


@pytest.mark.parametrize("dtype", KINDS)
def test_copy_source_and_its_mutants(dtype):
    for n, mult in _cases(dtype):
        src = special_source(n, dtype)
        w = src.view(np.uint64)
        for special in (0x8000000000000000, 0x0000000000000123, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF80000DEADBEEF):
            assert (w == np.uint64(special)).sum() >= 4
        assert first_difference(src.copy(), src) is None
        s = stride(n, dtype, CPU_NUM_CU, mult)
        if is_nt(n, dtype):                                        # only the non-temporal loop of k_copy takes two lanes per round
            twice = src.copy()
            _second_repeats_first(twice, src, s, lambda v: v)
            assert (first_difference(twice, src) is not None) == (lanes(n, dtype) > s), n
        if n & 1 and not is_cplx(dtype):
            skipped = src.copy()
            skipped[-1] = np.nan                                   # the destination starts as NaN
            assert first_difference(skipped, src) == n - 1


# ---- dot and norm ---------------------------------------------------------------------------------------------------------------------------------

def _tree(v):
    """wave_sum / the four waves / finish_partials' wave: adjacent pairs, level by level (additions commute: the DPP tree's bits)"""
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def emulate_dot(x, y, s, drop_fourth=False, skip_odd=False):
    """k_dot + finish_partials in numpy doubles without fused multiply-adds, in the kernels' order: thread t accumulates lanes t, t + s, ...
    one after the other, acc.x + acc.y (real), the odd last element into thread 0's acc.x, the wave and block trees, then lane b of
    finish_partials adds the partials b, b + 64, ... and the wave tree.  `drop_fourth`: the fourth load of every round of the four-element
    norm loop is never added; `skip_odd`: the odd last element is never added."""
    cp = is_cplx(x.dtype)
    xl, xo = _as_lanes(x)
    yl, yo = _as_lanes(y)
    nv = xl.shape[0]
    acc = np.zeros((s, 2))
    for r in range(-(-nv // s)):
        if drop_fourth and r % 4 == 3:
            continue
        a, b = xl[r * s:(r + 1) * s], yl[r * s:(r + 1) * s]
        if cp:
            acc[:len(a), 0] += a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]
            acc[:len(a), 1] += a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        else:
            acc[:len(a)] += a * b
    if xo is not None and not skip_odd:
        acc[0, 0] += xo[0] * yo[0]
    per_thread = acc.T if cp else (acc[:, 0] + acc[:, 1])[None, :]
    partial = _tree(per_thread.reshape(per_thread.shape[0], s // 256, 256))
    g = s // 256
    padded = np.zeros((partial.shape[0], -(-g // 64) * 64))
    padded[:, :g] = partial
    lane = np.zeros((partial.shape[0], 64))
    for r in range(padded.shape[1] // 64):
        lane += padded[:, r * 64:(r + 1) * 64]
    out = _tree(lane)
    return complex(out[0], out[1]) if cp else float(out[0])


def _check_dot(got, ref, scale, m, cp, label):
    return check_entrywise(np.array([got]), np.array([ref]), np.array([scale]), m, cp, label)


@pytest.mark.parametrize("dtype", KINDS)
def test_dot_reference_depth_and_mutants(dtype):
    cp = is_cplx(dtype)
    for n, mult in _cases(dtype) + [(POLICY_N[dtype][2], 64)]:
        x, y = vectors(n, dtype)
        xy, xy_scale, xx, xx_scale, _nrm = dot_references(n, dtype)
        s = stride(n, dtype, CPU_NUM_CU, mult, dot=True)
        m = dot_depth(n, dtype, CPU_NUM_CU, mult)
        assert m <= n // 1000, (n, m)                              # one product dropped or doubled is far beyond gamma(m) of the scale
        what = f"emulated k_dot n={n} mult={mult} {_name(dtype)}"
        _check_dot(emulate_dot(x, y, s), xy, xy_scale, m, cp, what)
        _check_dot(emulate_dot(x, x, s), xx, xx_scale, m, cp, what + " (norm)")
        runs_four = lanes(n, dtype) > 3 * s
        assert _detected(_check_dot, emulate_dot(x, x, s, drop_fourth=True), xx, xx_scale, m, cp, "a3 never added") == runs_four, n
        if n & 1 and not cp:
            assert abs(x[-1] * y[-1]) >= 1e-6 and x[-1] ** 2 >= 1e-6, n         # (a condition on the input: the last product is not tiny)
            assert _detected(_check_dot, emulate_dot(x, y, s, skip_odd=True), xy, xy_scale, m, cp, "odd last element skipped"), n
            assert _detected(_check_dot, emulate_dot(x, x, s, skip_odd=True), xx, xx_scale, m, cp, "odd last element skipped (norm)"), n
    n, mult = POLICY_N[dtype][2], 64                               # the grid capped at the partial buffer: 64 partials per lane of the finish
    assert stride(n, dtype, CPU_NUM_CU, mult, dot=True) == 4096 * 256 and dot_depth(n, dtype, CPU_NUM_CU, mult) == (3 if cp else 2) + 64 + 16


def test_dot_depth_formula_at_the_documented_point():
    assert dot_depth(4_194_304, np.float64, 256, 2) == 40
    assert stride(4_194_304, np.float64, 256, 2) == 131_072 and stride(100_003, np.float64, 256, 2) < 131_072
    for dtype in KINDS:
        nvs = [lanes(n, dtype) for n in edge_sizes(S1, dtype)]
        assert sorted(set(nvs)) == sorted(edge_lanes(S1))
        assert all(stride(n, dtype, CPU_NUM_CU, 1) == S1 for n in edge_sizes(S1, dtype))      # the grid is at its cap from nv = S - 1 on
        assert [is_nt(n, dtype) for n in POLICY_N[dtype]] == [False, True, True]
        assert lanes(deep_size(S1, dtype), dtype) == 5 * S1 + 3 and (is_cplx(dtype) or deep_size(S1, dtype) & 1)


# ---- the fused normalise ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", KINDS)
def test_normalised_reference_and_its_mutants(dtype):
    for n, mult in ((deep_size(S1, dtype), 1), (POLICY_N[dtype][2], DEFAULT_MULT)):
        x, _ = vectors(n, dtype)
        m = dot_depth(n, dtype, CPU_NUM_CU, mult)
        s = stride(n, dtype, CPU_NUM_CU, mult)
        ar = 1.0 / np.sqrt(abs(emulate_dot(x, x, stride(n, dtype, CPU_NUM_CU, mult, dot=True))))
        good = x * ar
        check_normalised(good, x, m, f"numpy normalise n={n}")
        twice = good.copy()
        _second_repeats_first(twice, x, s, lambda v: v * ar)
        assert _detected(check_normalised, twice, x, m, "f(v0) stored twice")
        if n & 1 and not is_cplx(dtype):
            skipped = good.copy()
            skipped[-1] = x[-1]
            assert _detected(check_normalised, skipped, x, m, "odd last element skipped")


# ---- rand -------------------------------------------------------------------------------------------------------------------------------------------

def test_numpy_generator_is_the_oracle_generator_for_the_real_kind():
    """ora.fill_counter is what tests/test_gpu_parity.py::test_rand_is_the_shared_counter_generator compares the engine with (n = 10 007,
    seed 42, row0 = 0); the formula of include/lightkrylov_hip.h in numpy gives the same bits there, at every row0 of the GPU test and at the
    sizes around the wrap of k_rand's grid-stride loop"""
    assert first_difference(rand_reference(10_007, np.float64, 42, 0), seeded(10_007, np.float64, 42)) is None
    for n in (S1 - 1, S1, S1 + 1, 3 * S1 + 5):
        assert rand_stride(n, CPU_NUM_CU, 1) == min(S1, 256 * -(-n // 256))
        for row0 in RAND_ROW0:
            want = np.empty(n)
            ora.fill_counter(want, 77, i0=row0)
            assert first_difference(rand_reference(n, np.float64, 77, row0), want) is None, (n, row0)


def test_rand_mutants_break_bit_equality():
    n = S1 + 1
    for dtype in KINDS:
        for row0 in RAND_ROW0[1:]:                                 # the counter ignores row0
            assert first_difference(rand_reference(n, dtype, 77, 0), rand_reference(n, dtype, 77, row0)) is not None
        wrapped = rand_reference(n, dtype, 77, 5)                  # a grid-stride loop that does not advance the counter when it wraps
        wrapped[S1:] = wrapped[:n - S1]
        assert first_difference(wrapped, rand_reference(n, dtype, 77, 5)) == S1 * (2 if is_cplx(dtype) else 1)
    for row0 in RAND_ROW0:                                         # the imaginary part from ctr = row instead of 2 row + 1
        good = rand_reference(n, np.complex128, 77, row0)
        bad = good.copy()
        bad.imag = rand_reference(n, np.float64, 77, row0)
        assert first_difference(bad, good) is not None
        assert np.array_equal(good.real[1:3], rand_reference(5, np.float64, 77, 2 * row0)[[2, 4]])     # real part of row r: counter 2 r
        assert np.array_equal(good.imag[:2], rand_reference(4, np.float64, 77, 2 * row0)[[1, 3]])      # imaginary part: 2 r + 1
    u = rand_reference(1000, np.float64, 3, 10 ** 9 + 1)
    assert (np.abs(u) <= 1.0).all() and abs(u.mean()) < 0.1 and len(np.unique(u)) == 1000
