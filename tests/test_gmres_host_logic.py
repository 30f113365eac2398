"""What the lk_gmres tests rest on, checked without a GPU: the cases of tests/_gmres_cases.py do on the oracle what
tests/test_gpu_gmres_engine.py says they do, the new Python classes fail loudly without a device, and the header documents the three
new entries with their reference lines.

The tests that pin the cases against the oracle exercise no code of the engine call and pass with or without it: they are the support of
the GPU tests (which fail without lk_gmres), not tests of the feature.  The header, binding and no-device tests do fail without it."""
import os
import re

import numpy as np
import pytest

import lightkrylov_amd as lk
from oracle import oracle as ora
from tests import _gmres_cases as cases
from tests._oracle_vector import oracle_diag_linop, oracle_vector
from tests._tol import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = [np.float64, np.complex128]


@pytest.mark.parametrize("dtype", KINDS)
def test_unpreconditioned_cases_cover_the_three_endings(dtype):
    A, b = cases.dense_nonsymmetric(dtype)
    seen = []
    for kdim, maxiter, rtol, tag in cases.UNPRECONDITIONED:
        x = np.zeros(b.size, dtype=dtype)
        info, res = ora.gmres(ora.DenseOp(A), b, x, rtol=rtol, atol=0.0, kdim=kdim, maxiter=maxiter)
        seen.append((info > 0, len(res) > kdim + 2))
    assert seen == [(True, False), (True, True), (False, True)], seen     # one cycle | restarts | maxiter exhausted


@pytest.mark.parametrize("dtype", KINDS)
def test_unscaled_vector_case_agrees_between_oracle_and_host_mirror(dtype):
    """gmres.fypp:171-172 on tests/_gmres_cases.tiny_diag: every sub-diagonal entry of H is below tol, the residual is not, and the oracle
    and the package's host mirror on oracle_vector agree on history and solution at 1e-12"""
    d, b = cases.tiny_diag(dtype)
    xo = np.zeros(b.size, dtype=dtype)
    info_o, res_o = ora.gmres(ora.DiagOp(d), b, xo, rtol=cases.TINY["rtol"], atol=0.0, kdim=cases.TINY["kdim"], maxiter=cases.TINY["maxiter"])
    x, meta = oracle_vector(np.zeros(b.size, dtype=dtype)), lk.gmres_dp_metadata()
    info = lk.gmres(oracle_diag_linop(d), oracle_vector(b.copy()), x, rtol=cases.TINY["rtol"], atol=0.0,
                    options=lk.gmres_dp_opts(kdim=cases.TINY["kdim"], maxiter=cases.TINY["maxiter"]), meta=meta)
    assert info == info_o == -8 and len(res_o) == 9
    assert np.abs(d).max() * 2 < cases.TINY["rtol"] < res_o.min()       # H(k+1, k) <= ||A|| <= tol < every residual
    assert_close(meta.res, res_o, f"tiny diag history {np.dtype(dtype).name}", scale=res_o[0])
    assert_close(x.data, xo, f"tiny diag solution {np.dtype(dtype).name}")


@pytest.mark.parametrize("dtype", KINDS)
def test_jacobi_preconditioner_cuts_the_iterations_on_the_oracle(dtype):
    _A, Ad, m, b = cases.variable_coefficient(dtype)
    assert abs(Ad.diagonal()).min() == 1.0 and abs(abs(Ad.diagonal()).max() - 1e4) < 1e-8
    p = cases.PRECONDITIONED
    u = np.zeros(b.size, dtype=dtype)
    ip, _ = ora.gmres(ora.PyOp(lambda v: Ad @ (m * v), dtype), b, u, rtol=p["rtol"], atol=0.0, kdim=p["kdim"], maxiter=p["maxiter"])
    x = np.zeros(b.size, dtype=dtype)
    iu, _ = ora.gmres(ora.DenseOp(Ad), b, x, rtol=p["rtol"], atol=0.0, kdim=p["kdim"], maxiter=p["maxiter"])
    assert (ip, iu) == cases.PRECONDITIONED_ITERATIONS


def test_new_classes_fail_loudly_without_a_device():
    import torch
    if torch.cuda.device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(lk._capi.LightKrylovHipError, match="no HIP device"):
        lk.compose_linop_gpu(None, None)
    with pytest.raises(lk._capi.LightKrylovHipError, match="no HIP device"):
        lk.linop_precond_gpu(lk.diag_linop_gpu(np.ones(4)))
    with pytest.raises(TypeError):
        lk.linop_precond_gpu(np.ones(4))                               # not an engine operator: no quiet fall-back to anything
    with pytest.raises(TypeError):
        lk.gmres(oracle_diag_linop(np.ones(4)), oracle_vector(np.ones(4)), oracle_vector(np.zeros(4)), engine=True)


def test_header_documents_the_new_entries_with_reference_lines():
    text = open(os.path.join(ROOT, "include", "lightkrylov_hip.h")).read()
    for name in ("lk_gmres", "lk_linop_residual", "lk_linop_compose_create"):
        head = text[:text.index(f"int {name}(")]
        last_comment = head[head.rindex("/*"):]
        assert re.search(r"\.fypp:\d+", last_comment), f"{name} lacks a reference file:line citation"
    from lightkrylov_amd import _capi
    for name in ("lk_gmres", "lk_linop_residual", "lk_linop_compose_create"):
        assert name in _capi.SIGNATURES


def test_engine_keyword_leaves_the_host_path_alone():
    """engine=None / False on host vectors is today's path: same history as without the keyword"""
    d, b = cases.tiny_diag(np.float64)
    out = []
    for kw in ({}, {"engine": None}, {"engine": False}):
        x, meta = oracle_vector(np.zeros(b.size)), lk.gmres_dp_metadata()
        lk.gmres(oracle_diag_linop(d * 1e12), oracle_vector(b.copy()), x, rtol=1e-10, options=lk.gmres_dp_opts(kdim=10, maxiter=3), meta=meta, **kw)
        out.append((meta.info, tuple(meta.res)))
    assert out[0] == out[1] == out[2]


# ---- the edges of lk_gmres' contract: the inputs of tests/test_gpu_gmres_edges.py on the oracle ------------------------------------------
@pytest.mark.parametrize("case", cases.EDGE_CASES, ids=lambda c: c.name)
@pytest.mark.parametrize("dtype", KINDS)
def test_edge_cases_on_the_oracle(dtype, case):
    """ora.gmres on every edge case: info, n_inner, n_outer and the history length as tests/_gmres_cases.EDGE_PINS states them, and the
    solution inside tol + 8 n eps ||A||_F ||x|| of the longdouble one (one_cycle does not converge: counts only)"""
    A, b, x0, info, res, x, xref = cases.oracle_run(case.name, np.dtype(dtype).name)
    pin_info, n_inner, n_outer, nres = case.pin(dtype)
    assert (info, len(res)) == (pin_info, nres), (info, len(res))
    assert n_inner + n_outer == abs(info) and nres == 1 + abs(info) and n_outer == -(-abs(info) // (case.kdim + 1))
    assert (info > 0) == case.converges and n_outer <= case.maxiter + 1
    if case.converges:
        cases.assert_solves(case, A, b, x, xref, f"oracle {case.name} {np.dtype(dtype).name}")
    if case.name.startswith("warm_start"):
        # the first entry is ||b - op(A) x0||, not ||b||: a skipped product shows
        r0 = cases.long_norm(cases._ext(b) - cases.long_product(case, A, x0))
        bound = cases.start_residual_bound(A, x0)
        assert abs(res[0] - r0) <= bound < abs(res[0] - np.linalg.norm(b))


def test_edge_cases_are_the_ones_the_gpu_file_expects():
    names = [c.name for c in cases.EDGE_CASES]
    assert len(set(names)) == len(names) == 19 and set(names) == set(cases.EDGE_PINS)
    # exhausted: n <= kdim ends inside the first cycle at step n; few_eigenvalues at step m = 3 of kdim = 10
    for c in cases.EDGE_CASES:
        if c.name.startswith("exhausted"):
            n = c.inputs(np.float64)[1].size
            if n <= c.kdim:
                assert c.pin(np.float64) == c.pin(np.complex128) == (n + 1, n, 1, n + 2)
    assert cases.EDGE_PINS["few_eigenvalues"][0] == (4, 3, 1, 5) and cases.EDGE_PINS["one_cycle"][0][0] == -6


@pytest.mark.parametrize("dtype", KINDS)
def test_unscaled_warm_keeps_every_subdiagonal_below_tol_and_every_residual_above(dtype):
    """a condition on the input: H(k+1, k) <= ||A|| <= tol < every residual, from a start residual that needs the product (x0 != 0)"""
    A, b, x0, info, res, _x, _xref = cases.oracle_run("unscaled_warm", np.dtype(dtype).name)
    assert np.abs(A).max() * 2 < cases.TINY["rtol"] * np.linalg.norm(b) < res.min() and np.linalg.norm(x0) > 1 and info == -8


@pytest.mark.parametrize("dtype", KINDS)
def test_exact_guess_has_a_start_residual_of_exactly_zero(dtype):
    for n in cases.EXACT_GUESS_N:
        d, b, x0 = cases.exact_guess(dtype, n)
        assert np.all(b != 0) and np.all(b - d * x0 == 0) and np.all(d * x0 == b)
        m = 1.0 / d                                                    # the Jacobi preconditioner of the GPU test: exact as well
        assert np.all(m * d == 1)


@pytest.mark.parametrize("dtype", KINDS)
def test_zero_start_residual_on_the_host_path(dtype):
    """The contract of lk_gmres for ||r0|| = 0 exactly, mirrored by the package's step-by-step gmres (the reference divides by beta = 0
    at gmres.fypp:142-143 and returns NaN): info = 0, converged, no iteration, history [0], x untouched -- from an exact guess and from
    b = 0, x0 = 0 whatever atol is."""
    d, b, x0 = cases.exact_guess(dtype, 257)
    zero = np.zeros(257, dtype=dtype)
    for bh, xh, atol in ((b, x0, 0.0), (zero, zero, 0.0), (zero, zero, 1e-12)):
        x, meta = oracle_vector(xh.copy()), lk.gmres_dp_metadata()
        info = lk.gmres(oracle_diag_linop(d), oracle_vector(bh.copy()), x, rtol=1e-10, atol=atol, options=lk.gmres_dp_opts(kdim=4, maxiter=3), meta=meta)
        assert info == meta.info == 0 and meta.converged and (meta.n_iter, meta.n_inner, meta.n_outer) == (0, 0, 0)
        assert list(meta.res) == [0.0] and x.data.tobytes() == xh.tobytes()
