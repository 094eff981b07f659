"""csrc/mfs_pcg_form.h decides which instantiation of the pressure march a stencil launch takes.  tests/c_abi/pcg_form_check.cpp
(stand-alone C++17, the header alone, no HIP) holds march_form against the decision tree it replaced -- transcribed there as a
plain function -- over the full product of inputs, and march_reachable against the set of forms that come out: equal in both
directions, 67 forms with whole vectors and 13 on the scalar path, each satisfying the kernel's static_asserts.  Built with
the host compiler under AddressSanitizer and UBSan; no GPU."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_march_form_agrees_with_the_decision_tree_it_replaced_on_every_input(tmp_path):
    exe = str(tmp_path / "pcg_form_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(REPO, "python-fluid-simulation_amd", "csrc"), os.path.join(REPO, "tests", "c_abi", "pcg_form_check.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.startswith("ok ") and "67 vector forms, 13 scalar forms" in r.stdout, r.stdout
