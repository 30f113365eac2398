#!/usr/bin/env python3
"""Calls per second of krylov_exptA (c = exp(tau A) b, tol = atol_dp, kdim = 30) on the negated 5-point Laplacian, the engine call
(lk_kexpm) against the host-loop route of lightkrylov_amd/expm.py on the same build: both routes in ONE process, interleaved round by
round, every round timed by a host clock around work that ends in a device synchronisation.  Also the host time one call spends in
lk_expm_dense (the kp - 1 small exponentials of a call, timed inside the host-loop route, ctypes overhead included).

  python tools/bench_kexpm.py [--out profiles/kexpm.jsonl] [--rounds 7] [--calls 40]
  python tools/bench_kexpm.py --block 4 [--out profiles/kexpm_block.jsonl]

tau = -3 / (8 (N + 1)^2): tau ||A|| < 3, which converges in about 20 steps.  One JSON line per size.

--block p: the block form instead -- ONE lk_kexpm_block call on p columns (nk = 30 block steps at most, workspace of p * 31 columns)
against p lk_kexpm calls on the same columns (kdim = 30), same tau and tol = atol_dp, interleaved round by round in one process.  The
line carries evaluations of p columns per second for either side, their ratio, and how far the two results lie apart."""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lightkrylov_amd as lk  # noqa: E402
from lightkrylov_amd import _capi  # noqa: E402
lkexpm = importlib.import_module("lightkrylov_amd.expm")   # (the package attribute of that name is the function)


class _user_op(lk.abstract_linop):
    """not an engine operator: krylov_exptA runs the host loop for it"""

    def __init__(self, A):
        super().__init__()
        self.A = A

    def matvec(self, vec_in, vec_out):
        self.A.matvec(vec_in, vec_out)

    rmatvec = matvec


def block_leg(args, ctx):
    p, kdim = args.block, 30
    lines = []
    for N in args.grids:
        n = N * N
        A = lk.laplacian2d_linop_gpu(N, ctx)
        tau = -3.0 / (8.0 * (N + 1) ** 2)
        B = lk.krylov_basis_gpu(n, p, np.float64, ctx)
        for j in range(p):
            B[j].rand(True, seed=5 + j)
        Cb, Cv = lk.krylov_basis_gpu(n, p, np.float64, ctx), lk.krylov_basis_gpu(n, p, np.float64, ctx)
        Xb = lk.krylov_basis_gpu(n, p * (kdim + 1), np.float64, ctx)
        Xv = lk.krylov_basis_gpu(n, kdim + 1, np.float64, ctx)
        info = {}

        def block():
            # kexpm's nk = kdim * p (ExpmLib.fypp:276) would need p (30 p + 1) columns: the engine entry takes nk itself
            i, e = C.c_int(), C.c_double()
            _capi.check(Xb._lib.lk_kexpm_block(A._h, 0, B._h, 0, Cb._h, 0, p, Xb._h, tau, lk.atol_dp, kdim, C.byref(i), C.byref(e)))
            info["block"] = i.value

        def vectors():
            info["vectors"] = [lk.kexpm(Cv[j], A, B[j], tau, lk.atol_dp, kdim=kdim, _basis=Xv) for j in range(p)]

        routes = {"block": block, "vectors": vectors}
        for fn in routes.values():                                              # warm-up: code objects, step buffers, scratch
            for _ in range(3):
                fn()
        ctx.sync()
        cb, cv = Cb.download(), Cv.download()
        rates = {name: [] for name in routes}
        for _ in range(args.rounds):
            for name, fn in routes.items():
                ctx.sync()
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    fn()
                ctx.sync()
                rates[name].append(args.calls / (time.perf_counter() - t0))
        rec = {"bench": f"kexpm on {p} columns: one lk_kexpm_block call against {p} lk_kexpm calls", "operator": "-lap5", "N": N, "n": n,
               "tau": tau, "p": p, "nk": kdim, "kdim": kdim, "tol": lk.atol_dp, "info": info, "rounds": args.rounds,
               "calls_per_round": args.calls,
               "max_abs_difference_of_results": float(np.abs(cb - cv).max()), "max_abs_result": float(np.abs(cv).max())}
        for name in routes:
            rec[f"{name}_evaluations_per_s_median"] = statistics.median(rates[name])
            rec[f"{name}_evaluations_per_s_min"] = min(rates[name])
            rec[f"{name}_evaluations_per_s_max"] = max(rates[name])
        rec["block_over_vectors_median"] = rec["block_evaluations_per_s_median"] / rec["vectors_evaluations_per_s_median"]
        print(json.dumps(rec))
        lines.append(json.dumps(rec))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kexpm.jsonl"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--grids", type=int, nargs="*", default=[418, 1000])       # n = 174 724 and 10^6
    ap.add_argument("--block", type=int, default=0, metavar="P", help="time lk_kexpm_block on P columns against P lk_kexpm calls")
    args = ap.parse_args()
    ctx = lk.Context(device=0)
    if args.block:
        if "--out" not in " ".join(sys.argv):
            args.out = os.path.join(ROOT, "profiles", "kexpm_block.jsonl")
        return block_leg(args, ctx)
    expm_time = [0.0]
    plain_expm = lkexpm.expm

    def timed_expm(A):
        t0 = time.perf_counter()
        E = plain_expm(A)
        expm_time[0] += time.perf_counter() - t0
        return E

    lines = []
    for N in args.grids:
        n = N * N
        A = lk.laplacian2d_linop_gpu(N, ctx)
        U = _user_op(A)
        tau = -3.0 / (8.0 * (N + 1) ** 2)
        b = lk.dense_vector_gpu(n, np.float64, ctx)
        b.rand(True, seed=5)
        c = lk.dense_vector_gpu(n, np.float64, ctx)
        X = lk.krylov_basis_gpu(n, 31, np.float64, ctx)
        routes = {"engine": A, "host_loop": U}
        info = {}
        for name, op in routes.items():                                         # warm-up: code objects, step buffers, scratch
            for _ in range(3):
                info[name] = lk.krylov_exptA(c, op, b, tau, _basis=X)
        ctx.sync()
        rates = {name: [] for name in routes}
        lkexpm.expm = timed_expm
        expm_time[0] = 0.0
        try:
            for _ in range(args.rounds):
                for name, op in routes.items():
                    ctx.sync()
                    t0 = time.perf_counter()
                    for _ in range(args.calls):
                        lk.krylov_exptA(c, op, b, tau, _basis=X)
                    ctx.sync()
                    rates[name].append(args.calls / (time.perf_counter() - t0))
        finally:
            lkexpm.expm = plain_expm
        rec = {"bench": "krylov_exptA", "operator": "-lap5", "N": N, "n": n, "tau": tau, "kdim": 30, "tol": lk.atol_dp,
               "info": info, "rounds": args.rounds, "calls_per_round": args.calls,
               "expm_dense_host_ms_per_call": 1e3 * expm_time[0] / (args.rounds * args.calls)}
        for name in routes:
            rec[f"{name}_calls_per_s_median"] = statistics.median(rates[name])
            rec[f"{name}_calls_per_s_min"] = min(rates[name])
            rec[f"{name}_calls_per_s_max"] = max(rates[name])
        rec["speedup_median"] = rec["engine_calls_per_s_median"] / rec["host_loop_calls_per_s_median"]
        print(json.dumps(rec))
        lines.append(json.dumps(rec))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
