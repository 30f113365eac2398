#!/usr/bin/env python3
"""The Poisson case of examples/poisson_gmres.py with conjugate gradient: the 5-point Laplacian of an N x N grid (symmetric positive
definite) with the matrix-free stencil operator, then the variable-coefficient matrix C^(1/2) A C^(1/2), c_i from 1 to 1e4, in CSR with
the Jacobi preconditioner `diag_linop_gpu(1 / diag)` -- each once through the package's host loop and once as ONE engine call (lk_cg,
`engine=True`), where alpha and beta never leave the device.

  python examples/poisson_cg.py [N=418]"""
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lightkrylov_amd as lk  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 418
n = N * N
ctx = lk.Context(device=0)
T = sp.diags([-np.ones(N - 1), 4.0 * np.ones(N), -np.ones(N - 1)], [-1, 0, 1])
S = sp.diags([-np.ones(N - 1), -np.ones(N - 1)], [-1, 1])
Acsr = ((sp.kron(sp.identity(N), T) + sp.kron(S, sp.identity(N))) * float((N + 1) ** 2)).tocsr()
c = 10.0 ** (4.0 * np.random.default_rng(3).random(n))
Cs = sp.diags(np.sqrt(c))
Avar = (Cs @ Acsr @ Cs).tocsr()
b = lk.dense_vector_gpu(n, np.float64, ctx)
b.rand(False, seed=11)
legs = (("stencil", lk.laplacian2d_linop_gpu(N, ctx), None),
        ("csr, variable coefficients + Jacobi", lk.csr_linop_gpu(Avar, ctx), lk.linop_precond_gpu(lk.diag_linop_gpu(1.0 / Avar.diagonal(), ctx))))
for name, A, pre in legs:
    for engine in (False, True):
        x = lk.dense_vector_gpu(n, np.float64, ctx)
        x.zero()
        meta = lk.cg_dp_metadata()
        ctx.sync(); t0 = time.perf_counter()
        info = lk.cg(A, b, x, rtol=1e-8, preconditioner=pre, options=lk.cg_dp_opts(maxiter=5000), meta=meta, engine=engine)
        ctx.sync(); dt = time.perf_counter() - t0
        r = lk.dense_vector_gpu(n, np.float64, ctx)
        print(f"{name:36s} {'lk_cg    ' if engine else 'host loop'} info = {info:5d}  {meta.n_iter} iterations in {dt:.3f} s   "
              f"|b - A x| / |b| = {lk.residual(A, x, b, r) / b.norm():.3e}")
ctx.close()
