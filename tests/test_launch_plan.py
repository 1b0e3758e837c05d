"""The launch plan of a general insert / mixed batch (pmdfc_amd/csrc/launch_plan.h): no GPU.

tests/cpp/test_launch_plan.cpp walks every input the engine can produce and
compares plan_launches' result with the launch table written out as data,
plus the invariants the kernels rely on (k_apply_fb only behind a lean first
pass, gates 2 and 1 in pairs, no gate on the coarse-partition pass).  Built
here as a program of its own with the address and undefined-behaviour
sanitizers where their runtimes are usable; nothing sanitized is loaded into
this process.
"""
import os
import shutil
import subprocess

import pytest

from conftest import REPO

SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_every_plan_against_the_table(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    src = os.path.join(REPO, "tests", "cpp", "test_launch_plan.cpp")
    tried = []
    for how, flags in (("static sanitizers", SANITIZE + ["-static-libasan", "-static-libubsan"]),
                       ("sanitizers", SANITIZE), ("unsanitized", [])):
        exe = str(tmp_path / ("plan_" + how.split()[0]))
        b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-o", exe, src] + flags,
                           capture_output=True, text=True)
        if b.returncode != 0:
            tried.append((how, "does not build", b.stderr[-2000:]))
            continue
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        if flags and "runtime does not come first" in r.stderr:
            tried.append((how, "its runtime must be loaded first"))
            continue
        assert r.returncode == 0, (how, r.stdout[-4000:], r.stderr[-2000:])
        word, count = r.stdout.split()
        # 5 bucket resolutions x {fb} x {ramp} x the 21 producible kinds, the
        # coarse partition only at the three resolutions past kCpSbb
        assert word == "OK" and int(count) == 4 * (5 * 20 + 3), (how, r.stdout)
        return
    raise AssertionError(tried)
