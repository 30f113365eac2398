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
