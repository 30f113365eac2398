#!/usr/bin/env python3
"""Heat equation on the unit square, u_t = Laplace(u) with u = 0 on the boundary, advanced by the exponential propagator:
u(t + tau) = exp(tau Laplace_h) u(t), each step one `krylov_exptA` call (src/Expm/ExpmLib.fypp:365-392) on the engine's 5-point
Laplacian.  `laplacian2d_linop_gpu` is -Laplace_h (positive definite), so the propagator is exp(-tau A).

  python examples/expm_heat.py [N=256] [steps=20]

The initial state is the lowest Dirichlet mode sin(pi x) sin(pi y) plus a higher one; the discrete operator damps mode (p, q) by
exp(-tau lambda_pq), lambda_pq = 4 (N+1)^2 (sin^2(p pi / (2 (N+1))) + sin^2(q pi / (2 (N+1)))), which is what the run is checked against."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lightkrylov_amd as lk  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
h = 1.0 / (N + 1)
tau = 2.0 * h * h                                   # tau ||A|| < 16: about 25 Krylov vectors per step

x = np.arange(1, N + 1) * h
modes = [(1, 1, 1.0), (3, 2, 0.5)]
lam = lambda p, q: 4.0 * (N + 1) ** 2 * (np.sin(p * np.pi * h / 2) ** 2 + np.sin(q * np.pi * h / 2) ** 2)  # noqa: E731
u0 = sum(a * np.outer(np.sin(q * np.pi * x), np.sin(p * np.pi * x)) for p, q, a in modes).reshape(-1)

ctx = lk.Context(device=0)
A = lk.laplacian2d_linop_gpu(N, ctx)
u = lk.dense_vector_gpu.from_array(u0, ctx)
v = lk.dense_vector_gpu(N * N, np.float64, ctx)
X = lk.krylov_basis_gpu(N * N, 31, np.float64, ctx)     # the workspace every step reuses
for s in range(steps):
    info = lk.krylov_exptA(v, A, u, -tau, _basis=X)
    u, v = v, u
    print(f"step {s + 1:3d}: t = {(s + 1) * tau:.3e}, {info if info > 0 else 'not converged with 30'} Krylov vectors, |u| = {u.norm():.6e}")
t = steps * tau
exact = sum(a * np.exp(-t * lam(p, q)) * np.outer(np.sin(q * np.pi * x), np.sin(p * np.pi * x)) for p, q, a in modes).reshape(-1)
err = np.linalg.norm(u.to_array() - exact) / np.linalg.norm(exact)
print(f"after {steps} steps: relative deviation from the discrete solution {err:.2e}")
ctx.close()
