"""fortran/test_cg_iso_c: lk_cg through the ISO_C_BINDING interface module from a Fortran host program, on the diagonal SPD system
d_i = 1 + (i - 1) / n, b_i = sin i, n = 1000, at rtol = 1e-12."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FDIR = os.path.join(ROOT, "fortran")


def test_fortran_host_program_solves_through_lk_cg():
    exe = os.path.join(FDIR, "test_cg_iso_c")
    assert os.path.exists(exe), "run __graft_entry__.build() first (fortran/Makefile builds test_cg_iso_c)"
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(ROOT, "lightkrylov_amd") + ":/opt/rocm/lib:/opt/rocm/lib/llvm/lib:" + env.get("LD_LIBRARY_PATH", "")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    vals = {}
    for line in out.stdout.splitlines():
        parts = line.split()
        if len(parts) == 2:
            vals[parts[0]] = float(parts[1])
    info, nres = int(vals["info"]), int(vals["nres"])
    print(out.stdout)
    assert info > 0 and nres == info + 1, (info, nres)
    assert vals["res_last"] < vals["tol"] < vals["res_first"]
    assert vals["err"] <= 1e-9 * vals["bmax"], vals
