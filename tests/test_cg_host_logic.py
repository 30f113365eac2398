"""The inputs of tests/test_gpu_cg_engine.py pinned without a GPU: the longdouble restatement of CG.fypp:105-170 (tests/_cg_cases.py)
agrees with the oracle's cg, every parity case keeps its history a factor 2 away from the tolerance up to the stopping iteration (so the
iteration count cannot flip on rounding), cg(engine=True) fails loudly on host vectors, and the ABI table knows lk_cg."""
import numpy as np
import pytest

import lightkrylov_amd as lk
from lightkrylov_amd import _capi
from oracle import oracle as ora
from tests import _cg_cases as cases


def test_restatement_agrees_with_the_oracle_on_the_real_unpreconditioned_case():
    A, b, _m, rtol, info, res, x, _r, _p = cases.parity_reference("dense_spd")
    xo = np.zeros(b.size)
    info_o, res_o = ora.cg(ora.DenseOp(np.array(A)), np.array(b), xo, rtol=rtol, atol=cases.ATOL, maxiter=cases.MAXITER)
    assert info == info_o > 0 and len(res) == len(res_o)
    # the project's bound for cg (tests/test_gpu_solvers.py::test_cg_against_oracle)
    assert np.abs(res.astype(np.float64) - res_o).max() <= 1e-9 * res_o[0]
    assert np.abs(x.astype(np.float64) - xo).max() <= 1e-9 * res_o[0]


@pytest.mark.parametrize("name", sorted(cases.PARITY))
def test_no_history_entry_within_a_factor_two_of_the_tolerance(name):
    _A, b, _m, rtol, info, res, _x, _r, _p = cases.parity_reference(name)
    tol = cases.tol_of(b, rtol)
    assert 5 <= info <= 15, f"{name}: info = {info}"
    q = res.astype(np.float64) / tol
    near = [(i, float(v)) for i, v in enumerate(q[:info + 1]) if 0.5 <= v <= 2.0]
    print(f"{name}: info = {info}, res / tol at the last two iterations {q[info - 1]:.3f}, {q[info]:.3f}")
    assert not near, f"{name}: history entries within a factor 2 of tol: {near}"
    assert q[info] < 0.5 and np.all(q[:info] > 2.0)


def test_jacobi_case_has_a_diagonal_of_three_decades():
    A, m, _b = cases.three_decades()
    d = np.diag(A)
    assert d.max() / d.min() >= 1e3 * 0.5 and np.allclose(m * d, 1.0) and np.linalg.eigvalsh(A).min() > 0


@pytest.mark.parametrize("dtype", [np.float64, np.complex128])
def test_stop_problem_converges_with_look_ahead_in_flight(dtype):
    d, b, rtol = cases.stop_problem(dtype)
    info, res, *_ = cases.cg_long(cases.diagop(d), b, np.zeros_like(b), rtol, 0.0, 100)
    tol = rtol * float(np.linalg.norm(b))
    assert 5 <= info <= 15 and res[info - 1] > 2 * tol and res[info] < 0.5 * tol, (info, res[-2:] / tol)


def test_engine_keyword_needs_gpu_vectors():
    class HostOp:
        def reset_counter(self, *a):
            pass

    class HostVec:
        pass

    with pytest.raises(TypeError):
        lk.cg(HostOp(), HostVec(), HostVec(), engine=True)


def test_the_abi_table_knows_lk_cg():
    assert "lk_cg" in _capi.SIGNATURES
    restype, argtypes = _capi.SIGNATURES["lk_cg"]
    assert len(argtypes) == 14
