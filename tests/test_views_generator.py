"""The generator of tests/test_gpu_views.py's mixed-handle fuzz, replayed without a device: tests/test_gpu_lazy_fuzz.py's `_run` on a
stand-in for the package whose calls do nothing.  The sequence of calls depends on the two generators only, never on a result, so the
operands the GPU run names -- and the handle each is named through -- are the ones counted here."""
import contextlib

import numpy as np
import pytest

from tests import test_gpu_lazy_fuzz as fuzz
from tests.test_gpu_views import VIEWS


class _Tensor:
    def abs(self): return self
    def sum(self): return self
    def item(self): return 0.0
    def fill_(self, v): pass
    def mul_(self, v): pass


class _Vec:
    def __init__(self, basis, col): self.basis, self.col = basis, col
    def rand(self, *a, **k): pass
    def zero(self): pass
    def scal(self, a): pass
    def axpby(self, a, x, b): pass
    def norm(self): return 0.0
    def dot(self, y): return 0.0
    def to_array(self): return np.zeros(1)
    def as_torch(self, acc): return _Tensor()


class _Basis:
    def __init__(self, n, ncols, dtype=None, ctx=None): self.ncols = ncols
    def __getitem__(self, j): return self if isinstance(j, slice) else _Vec(self, j)
    def view(self, a, w): return _Basis(0, w)
    def upload(self, host, col0=0): pass
    def download(self): return np.zeros((1, 1))


class _Context:
    def __init__(self, device=0): pass
    def set_tuning(self, k, v): pass
    def torch_stream(self): return contextlib.nullcontext()
    def lazy_fusion_stats(self): return [0, 0, 0, 0]
    def lazy_stats(self): return [0, 0, 0, 0]
    def close(self): pass


class _Package:
    Context, krylov_basis_gpu = _Context, _Basis
    dense_vector_gpu = staticmethod(lambda n, dtype, c: _Vec(_Basis(n, 1), 0))
    copy = staticmethod(lambda out, frm: None)
    innerprod = staticmethod(lambda X, y: np.zeros(1))


@pytest.mark.parametrize("dtype", [np.float64, np.complex128])
def test_a_third_of_the_operands_of_every_seed_go_through_a_view(dtype):
    for seed in range(24):
        named, through = fuzz._run(seed, dtype, lazy=True, views=VIEWS, lk=_Package)[2][-2:]
        assert named > 100 and 3 * through >= named, f"seed {seed}: {through} of {named} vector operands went through a view"
        assert fuzz._run(seed, dtype, lazy=False, views=(), lk=_Package)[2][-2:] == [named, 0]      # the same calls without views
