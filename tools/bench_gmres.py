"""Solver steps per second of gmres as ONE engine call (lk_gmres) against the package's gmres on the paths that existed before it,
interleaved in one process (one warm-up round, then ROUNDS rounds A B A B ..., median and range).  The comparison routes are untouched
by lk_gmres: the unpreconditioned one is `lk.gmres` without the `engine` keyword (inner cycle as one lk_arnoldi_segments call, restart
logic in Python), the preconditioned one is `engine=False` (one host round trip per step).  A step = one count of n_iter.
  (i)   the 5-point Laplacian of BASELINE configs[2], N = 4096, GMRES(30), maxiter 3 (rtol out of reach: four full cycles)
  (ii)  n = 175 000, diagonal operator d_i = 1 + 99 i / n, GMRES(10) and GMRES(30), rtol 1e-10 (restarts counted in the record)
  (iii) the operator of (ii) with an INEXACT diagonal preconditioner M_i = 1 / (d_i (1 + 0.9 u_i)), u_i in (-1, 1): the exact Jacobi
        preconditioner of a diagonal operator is its inverse and would end every solve at the first step
  python tools/bench_gmres.py [out.jsonl]"""
import json, os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lightkrylov_amd as lk
ROUNDS = 7
ctx = lk.Context(device=0)
out = open(sys.argv[1], "a") if len(sys.argv) > 1 else None


def solve(A, b, x, kdim, maxiter, rtol, pre, engine):
    x.zero()
    meta = lk.gmres_dp_metadata()
    ctx.sync()
    t0 = time.perf_counter()
    lk.gmres(A, b, x, rtol=rtol, atol=0.0, preconditioner=pre, options=lk.gmres_dp_opts(kdim=kdim, maxiter=maxiter), meta=meta, engine=engine)
    ctx.sync()
    return meta.n_iter / (time.perf_counter() - t0), meta


def case(name, A, n, kdim, maxiter, rtol, pre=None):
    b, x = lk.dense_vector_gpu(n, np.float64, ctx), lk.dense_vector_gpu(n, np.float64, ctx)
    b.rand(False, seed=11)
    routes = (("lk_gmres", True if pre is None else None), ("before", None if pre is None else False))
    rates, metas = {r: [] for r, _ in routes}, {}
    for rnd in range(ROUNDS + 1):
        for r, engine in routes:
            rate, metas[r] = solve(A, b, x, kdim, maxiter, rtol, pre, engine)
            if rnd:
                rates[r].append(rate)
    med = {r: statistics.median(v) for r, v in rates.items()}
    rec = {"case": name, "n": n, "kdim": kdim, "maxiter": maxiter, "rtol": rtol, "rounds": ROUNDS,
           "compared_with": "lk.gmres without engine=" if pre is None else "lk.gmres(engine=False): one host round trip per step",
           "steps_per_s": {r: {"median": round(med[r], 1), "min": round(min(v), 1), "max": round(max(v), 1)} for r, v in rates.items()},
           "ratio": round(med["lk_gmres"] / med["before"], 3),
           "n_iter": {r: m.n_iter for r, m in metas.items()}, "n_outer": {r: m.n_outer for r, m in metas.items()},
           "converged": {r: m.converged for r, m in metas.items()}}
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


N = 4096
case("(i) lap5 N=4096 GMRES(30)", lk.laplacian2d_linop_gpu(N, ctx), N * N, 30, 3, 1e-300)
n = 175_000
d = 1.0 + 99.0 * np.arange(n) / n
A = lk.diag_linop_gpu(d, ctx)
case("(ii) diag n=175000 GMRES(10)", A, n, 10, 200, 1e-10)
case("(ii) diag n=175000 GMRES(30)", A, n, 30, 60, 1e-10)
u = 2.0 * np.random.default_rng(5).random(n) - 1.0
pre = lk.linop_precond_gpu(lk.diag_linop_gpu(1.0 / (d * (1.0 + 0.9 * u)), ctx))
case("(iii) diag n=175000 inexact diagonal M GMRES(10)", A, n, 10, 200, 1e-10, pre)
case("(iii) diag n=175000 inexact diagonal M GMRES(30)", A, n, 30, 60, 1e-10, pre)
ctx.close()
