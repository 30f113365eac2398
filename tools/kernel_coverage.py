"""Which kernel instances does the GPU suite dispatch, and from which tests?  Produces profiles/kernel_coverage_gpu_suite.csv, the record
tests/test_kernel_coverage.py checks tests/kernel_instances.txt against.

1. Run (a slice of) the GPU suite under a kernel trace with this file as a pytest plugin; it appends each test's wall interval to
   $LK_COV_INTERVALS:
       PYTHONPATH=tools LK_COV_INTERVALS=/tmp/iv.tsv timeout -k 10 1500 rocprofv3 --kernel-trace --stats -d /tmp/tr -o %pid% -f csv -- \\
           python -m pytest -m gpu -q -p kernel_coverage
   (the suite's child processes inherit the trace; each process writes its own <pid>_kernel_trace.csv).
2. Attribute every dispatch of an lk:: kernel to the test whose interval holds its start timestamp:
       python tools/kernel_coverage.py merge /tmp/tr /tmp/iv.tsv slice.json
3. Write the record from one or more slices (instances of the code object that no slice dispatched get 0 calls):
       python tools/kernel_coverage.py csv --commit <sha> --out profiles/kernel_coverage_gpu_suite.csv slice*.json
"""
import bisect
import collections
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- pytest plugin ---------------------------------------------------------------------------------------------------------------

def _clocks():
    return time.clock_gettime_ns(time.CLOCK_MONOTONIC), time.clock_gettime_ns(time.CLOCK_BOOTTIME)


try:
    import pytest

    @pytest.hookimpl(hookwrapper=True)
    def pytest_runtest_protocol(item, nextitem):
        t0 = _clocks()
        yield
        t1 = _clocks()
        path = os.environ.get("LK_COV_INTERVALS")
        if path:
            with open(path, "a") as f:
                f.write(f"{item.nodeid}\t{t0[0]}\t{t1[0]}\t{t0[1]}\t{t1[1]}\n")
except ImportError:  # merge / csv need no pytest
    pass


# ---- merge -----------------------------------------------------------------------------------------------------------------------

def _normalise(demangled):
    name = demangled.split("(")[0].strip()
    return name[5:] if name.startswith("void ") else name


def merge(tracedir, intervals, out):
    rows = [l.rstrip("\n").split("\t") for l in open(intervals) if l.strip()]
    # rocprofv3's timestamps are one of the two clocks; take the one under which the dispatches fall inside the tests' intervals
    ivs = {clk: sorted((int(r[a]), int(r[b]), r[0]) for r in rows) for clk, (a, b) in (("monotonic", (1, 2)), ("boottime", (3, 4)))}
    starts = {clk: [iv[0] for iv in ivs[clk]] for clk in ivs}

    def owner(clk, t):
        i = bisect.bisect_right(starts[clk], t) - 1
        return ivs[clk][i][2] if i >= 0 and ivs[clk][i][0] <= t <= ivs[clk][i][1] else None

    dispatches = []
    for fn in glob.glob(os.path.join(tracedir, "**", "*kernel_trace.csv"), recursive=True):
        with open(fn, newline="") as f:
            for r in csv.DictReader(f):
                k = _normalise(r["Kernel_Name"])
                if k.startswith("lk::"):
                    dispatches.append((k, int(r["Start_Timestamp"])))
    fit = {clk: sum(owner(clk, t) is not None for _, t in dispatches[:20000]) for clk in ivs}
    clk = max(fit, key=fit.get)
    calls = collections.Counter(k for k, _ in dispatches)
    tests = collections.defaultdict(collections.Counter)
    unattributed = 0
    for k, t in dispatches:
        node = owner(clk, t)
        if node is None:
            unattributed += 1
        else:
            tests[k][node] += 1
    json.dump({"clock": clk, "dispatches": len(dispatches), "unattributed": unattributed, "tests_run": len(rows),
               "calls": dict(calls), "tests": {k: dict(v) for k, v in tests.items()}}, open(out, "w"), indent=0)
    print(f"{out}: {len(dispatches)} dispatches of {len(calls)} instances over {len(rows)} tests ({clk} clock, {unattributed} unattributed)")


def write_csv(slices, commit, out):
    sys.path.insert(0, ROOT)
    from tests.test_kernel_coverage import code_object_instances
    calls = collections.Counter()
    ntests = 0
    for s in slices:
        d = json.load(open(s))
        calls.update(d["calls"])
        ntests += d["tests_run"]
    inst = code_object_instances()
    unknown = sorted(set(calls) - set(inst))
    assert not unknown, f"traced instances the built code object does not hold (stale build?): {unknown}"
    with open(out, "w", newline="") as f:
        f.write(f"# lk:: kernel dispatches of the GPU suite (pytest -m gpu, {ntests} tests) under rocprofv3 --kernel-trace; taken at "
                f"commit {commit}\n# one row per instance of the gfx950 code object (tests/test_kernel_coverage.py); 0 = never dispatched\n")
        w = csv.writer(f, lineterminator="\n")
        w.writerow(["instance", "calls"])
        for i in inst:
            w.writerow([i, calls.get(i, 0)])
    print(f"{out}: {sum(1 for i in inst if calls.get(i))} of {len(inst)} instances dispatched")


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "merge":
        merge(*sys.argv[2:])
    elif len(sys.argv) >= 7 and sys.argv[1] == "csv" and sys.argv[2] == "--commit" and sys.argv[4] == "--out":
        write_csv(sys.argv[6:], sys.argv[3], sys.argv[5])
    else:
        sys.exit(__doc__)
