"""Every kernel instance in the shipped gfx950 code object is either dispatched by a named GPU test or declared unreachable
(tests/kernel_instances.txt), and the committed coverage record of the GPU suite (profiles/kernel_coverage_gpu_suite.csv, one
kernel-trace run of `pytest -m gpu`, tools/kernel_coverage.py) shows calls for every reachable one.  Adding a `template __global__`
instantiation without a test that reaches it, or deleting a manifest line, fails here.  The tuning keys lk_set_tuning accepts are
the ones include/lightkrylov_hip.h documents, and every one is named in a GPU test.  No GPU needed: the code object is read from
the built library with the ROCm LLVM tools."""
import ast
import csv
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lightkrylov_amd", "liblightkrylov_hip.so")
MANIFEST = os.path.join(ROOT, "tests", "kernel_instances.txt")
COVERAGE = os.path.join(ROOT, "profiles", "kernel_coverage_gpu_suite.csv")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def _llvm(tool):
    base = os.environ.get("ROCM_PATH", "/opt/rocm")
    path = os.path.join(base, "llvm", "bin", tool)
    assert os.path.exists(path), f"{path} missing: the ROCm LLVM tools read the code object"
    return path


def normalise(demangled):
    """'void lk::k_csr<false, 1>(double const*, ...)' -> 'lk::k_csr<false, 1>' (the name rocprofv3 reports, argument list dropped)"""
    name = demangled.split("(")[0].strip()
    return name[5:] if name.startswith("void ") else name


def code_object_instances(lib=LIB):
    """Unique kernel symbols (.kd) of the gfx950 code object in the library's .hip_fatbin, demangled and normalised."""
    assert os.path.exists(lib), "run __graft_entry__.build() first"
    with tempfile.TemporaryDirectory() as tmp:
        fatbin, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "gfx950.co")
        subprocess.check_call([_llvm("llvm-objcopy"), f"--dump-section=.hip_fatbin={fatbin}", lib, os.path.join(tmp, "stripped")])
        subprocess.check_call([_llvm("clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fatbin}", f"--targets={TARGET}",
                               f"--output={co}"])
        syms = subprocess.run([_llvm("llvm-readelf"), "-s", "-W", co], check=True, capture_output=True, text=True).stdout
    mangled = sorted({f[7][:-3] for f in (l.split() for l in syms.splitlines()) if len(f) >= 8 and f[7].endswith(".kd")})
    assert mangled, "no kernel descriptors in the gfx950 code object"
    out = subprocess.run(["c++filt"], input="\n".join(mangled) + "\n", check=True, capture_output=True, text=True).stdout
    return sorted({normalise(l) for l in out.splitlines() if l.strip()})


def read_manifest(path=MANIFEST):
    """{instance: [pytest node ids]} or {instance: 'unreachable: why'}; '#' lines are comments, fields are separated by ' | '."""
    entries = {}
    for ln, line in enumerate(open(path), 1):
        line = line.strip()
        if not line or line.startswith("#"):
            continue
        name, *rest = [f.strip() for f in line.split(" | ")]
        assert rest and all(rest), f"kernel_instances.txt:{ln}: '{name}' names no test and no 'unreachable: <reason>'"
        assert name not in entries, f"kernel_instances.txt:{ln}: '{name}' listed twice"
        if rest[0].startswith("unreachable:"):
            assert len(rest) == 1 and len(rest[0]) > len("unreachable:") + 10, f"kernel_instances.txt:{ln}: give the reason"
            entries[name] = rest[0]
        else:
            entries[name] = rest
    return entries


def read_coverage(path=COVERAGE):
    calls = {}
    with open(path, newline="") as f:
        rows = [r for r in csv.reader(l for l in f if not l.startswith("#"))]
    assert rows[0] == ["instance", "calls"], rows[0]
    for name, n in rows[1:]:
        calls[name] = int(n)
    return calls


def _test_functions(relpath, cache={}):
    """names of the test functions a test file defines (module level and inside classes), by parsing it"""
    if relpath not in cache:
        tree = ast.parse(open(os.path.join(ROOT, relpath)).read())
        names = set()
        for node in ast.walk(tree):
            if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)) and node.name.startswith("test"):
                names.add(node.name)
        cache[relpath] = names
    return cache[relpath]


@pytest.fixture(scope="module")
def instances():
    return code_object_instances()


def test_every_instance_is_in_the_manifest_and_nothing_else(instances):
    listed = read_manifest()
    missing = sorted(set(instances) - set(listed))
    stale = sorted(set(listed) - set(instances))
    assert not missing, "instances in the code object that tests/kernel_instances.txt does not list (name the GPU test that " \
                        "dispatches each, or 'unreachable: <reason>'):\n  " + "\n  ".join(missing)
    assert not stale, "tests/kernel_instances.txt lists instances the code object does not hold:\n  " + "\n  ".join(stale)


def test_every_named_test_exists():
    bad = []
    for name, tests in read_manifest().items():
        if isinstance(tests, str):
            continue
        for node in tests:
            path, _, func = node.partition("::")
            func = func.split("::")[-1].split("[")[0]
            if not (path.startswith("tests/test_") and path.endswith(".py") and os.path.exists(os.path.join(ROOT, path))):
                bad.append(f"{name}: {node} (not a test file of this suite)")
            elif func not in _test_functions(path):
                bad.append(f"{name}: {node} (no test function '{func}' in {path})")
    assert not bad, "\n".join(bad)


def test_every_reachable_instance_was_dispatched_by_the_gpu_suite(instances):
    calls = read_coverage()
    listed = read_manifest()
    unreached = sorted(i for i in instances if not isinstance(listed.get(i), str) and calls.get(i, 0) <= 0)
    assert not unreached, "reachable instances with no call in profiles/kernel_coverage_gpu_suite.csv (re-take it with " \
                          "tools/kernel_coverage.py after adding the test):\n  " + "\n  ".join(unreached)
    unknown = sorted(set(calls) - set(instances))
    assert not unknown, f"coverage record names instances the code object does not hold: {unknown}"


def test_no_instance_declared_unreachable_was_dispatched(instances):
    """the other half of the manifest's claim: a line that says 'unreachable' while the record shows calls is stale"""
    calls = read_coverage()
    stale = sorted((i, calls[i]) for i, why in read_manifest().items() if isinstance(why, str) and calls.get(i, 0) > 0)
    assert not stale, "tests/kernel_instances.txt declares instances unreachable that profiles/kernel_coverage_gpu_suite.csv shows " \
                      "dispatched (name the GPU tests that reach them):\n  " + "\n  ".join(f"{i}: {n} calls" for i, n in stale)


def _record_commit():
    head = [l for l in open(COVERAGE) if l.startswith("#")]
    found = [m.group(1) for l in head for m in [re.search(r"\bcommit ([0-9a-f]{7,})", l)] if m]
    assert found, "the coverage record must name the commit it was taken at"
    return found[0]


def test_coverage_record_states_where_it_was_taken():
    _record_commit()


def test_coverage_record_was_taken_on_this_history():
    """the commit the record names is HEAD or one of its ancestors: a record from another branch says nothing about this tree"""
    sha = _record_commit()
    if not os.path.exists(os.path.join(ROOT, ".git")):
        pytest.skip("no .git here (a source archive): the record's commit cannot be placed in the history")
    head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--verify", "HEAD"], capture_output=True, text=True)
    if head.returncode != 0:
        pytest.skip(f"git cannot read this checkout ({head.stderr.strip()}): the record's commit cannot be placed in the history")
    r = subprocess.run(["git", "-C", ROOT, "merge-base", "--is-ancestor", sha, "HEAD"], capture_output=True, text=True)
    assert r.returncode == 0, f"the coverage record was taken at commit {sha}, which is not HEAD or an ancestor of it " \
                              f"(git: {r.stderr.strip() or 'exit ' + str(r.returncode)}); re-take it with tools/kernel_coverage.py"


# ---- tuning keys ---------------------------------------------------------------------------------------------------------------

def shipped_tuning_keys():
    """the keys lk_set_tuning's strcmp chain accepts outside #ifdef LK_DIAGNOSTICS"""
    src = open(os.path.join(ROOT, "lightkrylov_amd", "csrc", "lk_engine.hip")).read()
    body = src[src.index("int lk_set_tuning(lk_context_t c, const char *key, int value)"):]
    body = body[:body.index("unknown key")]
    body = re.sub(r"#ifdef LK_DIAGNOSTICS.*?#endif", "", body, flags=re.S)
    return re.findall(r'strcmp\(key, "(\w+)"\)', body)


def documented_tuning_keys():
    """(keys, stated count) of the comment above lk_set_tuning in the public header, without the diagnostics build's keys"""
    hdr = open(os.path.join(ROOT, "include", "lightkrylov_hip.h")).read()
    end = hdr.index("int lk_set_tuning(")
    block = hdr[hdr.rindex("/* Tuning keys", 0, end):end]
    count = int(re.search(r"\((?:integers; )?(\d+) of them", block).group(1))
    block = block[:block.index("A build made with -DLK_DIAGNOSTICS")]
    return re.findall(r'"(\w+)"', block), count


def test_documented_tuning_keys_are_the_shipped_ones():
    shipped = shipped_tuning_keys()
    documented, count = documented_tuning_keys()
    assert len(shipped) == len(set(shipped)), "a key is tested twice in lk_set_tuning"
    assert sorted(set(documented)) == sorted(shipped), (sorted(set(documented) - set(shipped)), sorted(set(shipped) - set(documented)))
    assert count == len(shipped), f"the header says {count} keys, lk_set_tuning accepts {len(shipped)}"


def test_every_tuning_key_is_set_in_a_gpu_test():
    text = ""
    for f in sorted(os.listdir(os.path.join(ROOT, "tests"))):
        if f.startswith("test_gpu_") and f.endswith(".py"):
            text += open(os.path.join(ROOT, "tests", f)).read()
    unnamed = [k for k in shipped_tuning_keys() if not re.search(r"""["']%s["']""" % k, text)]
    assert not unnamed, f"tuning keys no GPU test sets: {unnamed}"
