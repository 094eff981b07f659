"""csrc/mfs_vcg_form.h decides which kernel a stencil launch of the viscosity engine takes -- for the march its geometry, LDS
bytes, grid and template arguments -- and which loop mfs_vcg3d_iterate runs.  tests/c_abi/vcg_form_check.cpp (stand-alone
C++17, the header alone, no HIP) holds vmarch_form and vloop_form against the decision code they replaced -- transcribed
there as plain functions -- over every row length from 1 to 1200 for the geometry and the full product of knobs for the rest,
and vmarch_reachable against the set of forms that come out: equal in both directions, 16 march forms per dtype and 8 loop
forms.  Built with the host compiler under AddressSanitizer and UBSan; no GPU."""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_vmarch_form_and_vloop_form_agree_with_the_decision_code_they_replaced_on_every_input(tmp_path):
    exe = str(tmp_path / "vcg_form_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(REPO, "python-fluid-simulation_amd", "csrc"), os.path.join(REPO, "tests", "c_abi", "vcg_form_check.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    m = re.fullmatch(r"ok (\d+) cases, 16 march forms, 8 loop forms\n", r.stdout)
    assert m and int(m.group(1)) > 1000000, r.stdout
