"""Iterations per second of cg as ONE engine call (lk_cg, `engine=True`) against the package's host loop (`engine=False`: a product, two
dots that each stop the host and three axpbys per iteration -- the path that existed before lk_cg and is untouched by it), interleaved in
one process (one warm-up round, then ROUNDS rounds A B A B ..., median and range).  The tolerance is out of reach (rtol = atol = 0), so
every solve runs exactly `maxiter` iterations.
  (i)   the 5-point Laplacian, N = 418 (n = 174 724: launch-bound), unpreconditioned
  (ii)  the 5-point Laplacian, N = 4096 (n = 16 777 216: bandwidth-bound), unpreconditioned
  (iii) the variable-coefficient CSR leg of examples/poisson_gmres.py at N = 418 (C^(1/2) A C^(1/2), c_i over four decades) with the
        Jacobi preconditioner `linop_precond_gpu(diag_linop_gpu(1 / diag))`
  python tools/bench_cg.py [out.jsonl]"""
import json, os, statistics, sys, time
import numpy as np
import scipy.sparse as sp
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lightkrylov_amd as lk
ROUNDS = 7
ctx = lk.Context(device=0)
out = open(sys.argv[1], "a") if len(sys.argv) > 1 else None


def solve(A, b, x, maxiter, pre, engine):
    x.zero()
    meta = lk.cg_dp_metadata()
    ctx.sync()
    t0 = time.perf_counter()
    lk.cg(A, b, x, rtol=0.0, atol=0.0, preconditioner=pre, options=lk.cg_dp_opts(maxiter=maxiter), meta=meta, engine=engine)
    ctx.sync()
    return meta.n_iter / (time.perf_counter() - t0), meta


def case(name, A, n, maxiter, pre=None):
    b, x = lk.dense_vector_gpu(n, np.float64, ctx), lk.dense_vector_gpu(n, np.float64, ctx)
    b.rand(False, seed=11)
    routes = (("lk_cg", True), ("host_loop", False))
    rates, metas = {r: [] for r, _ in routes}, {}
    for rnd in range(ROUNDS + 1):
        for r, engine in routes:
            rate, metas[r] = solve(A, b, x, maxiter, pre, engine)
            if rnd:
                rates[r].append(rate)
    med = {r: statistics.median(v) for r, v in rates.items()}
    rec = {"case": name, "n": n, "maxiter": maxiter, "rounds": ROUNDS, "compared_with": "lk.cg(engine=False): the host loop, three host round trips per iteration",
           "iterations_per_s": {r: {"median": round(med[r], 1), "min": round(min(v), 1), "max": round(max(v), 1)} for r, v in rates.items()},
           "ratio": round(med["lk_cg"] / med["host_loop"], 3),
           "n_iter": {r: m.n_iter for r, m in metas.items()}, "last_residual": {r: m.res[-1] for r, m in metas.items()}}
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def lap5_csr(N):
    T = sp.diags([-np.ones(N - 1), 4.0 * np.ones(N), -np.ones(N - 1)], [-1, 0, 1])
    S = sp.diags([-np.ones(N - 1), -np.ones(N - 1)], [-1, 1])
    return ((sp.kron(sp.identity(N), T) + sp.kron(S, sp.identity(N))) * float((N + 1) ** 2)).tocsr()


N = 418
case("(i) lap5 N=418", lk.laplacian2d_linop_gpu(N, ctx), N * N, 300)
case("(ii) lap5 N=4096", lk.laplacian2d_linop_gpu(4096, ctx), 4096 * 4096, 100)
c = 10.0 ** (4.0 * np.random.default_rng(3).random(N * N))
Cs = sp.diags(np.sqrt(c))
Avar = (Cs @ lap5_csr(N) @ Cs).tocsr()
pre = lk.linop_precond_gpu(lk.diag_linop_gpu(1.0 / Avar.diagonal(), ctx))
case("(iii) csr variable coefficients N=418 + Jacobi", lk.csr_linop_gpu(Avar, ctx), N * N, 300, pre)
ctx.close()
