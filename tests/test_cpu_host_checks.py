"""Sanitizers on the library's host logic (SURVEY.md §5 "race detection / sanitizers"): GPU AddressSanitizer is not available on the MI355X
pool, so the NON-KERNEL code of libmatcha_hip -- argument validation, workspace sizing and carving, the option table, the step's kernel route
and its record -- is compiled for the host only with -fsanitize=address,undefined and driven by the stand-alone programs of tests/host/ (what
they share is tests/host/host_driver.hpp; what each one covers is its file's header).  One build (`make host-asan`), one case per driver.  Runs
in the CPU container; nothing is loaded into Python and no kernel is launched (launch attempts must come back as MATCHA_EHIP)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# driver (csrc/Makefile: HOST_DRIVERS) -> the line it prints when every check held
DRIVERS = {
    "host_checks": "ALL HOST CHECKS PASSED",
    "route_node_dx": "ALL NODE_DX ROUTE CHECKS PASSED",
    "route_pairs": "ALL LAUNCH PAIR ROUTE CHECKS PASSED",
    "complete_checks": "ALL CLUSTER COMPLETION HOST CHECKS PASSED",
    "subsets_checks": "ALL CLUSTER DECOMPOSITION HOST CHECKS PASSED",
    "grow_checks": "ALL CLUSTER GROWTH HOST CHECKS PASSED",
    "region_checks": "ALL MULTI-REGION HOST CHECKS PASSED",
    "outlier_checks": "ALL OUTLIER HOST CHECKS PASSED",
    "expected_checks": "ALL EXPECTATION HOST CHECKS PASSED",
    "walk_checks": "ALL WALK HOST CHECKS PASSED",
}


@pytest.fixture(scope="module")
def host_asan():
    csrc = os.path.join(ROOT, "matcha_amd", "csrc")
    build = subprocess.run(["make", "-C", csrc, "-j", str(min(8, os.cpu_count() or 1)), "host-asan"], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout[-3000:] + build.stderr[-3000:]
    return os.path.join(ROOT, "build", "host_asan")


@pytest.mark.parametrize("driver", list(DRIVERS))
def test_host_side_under_asan_ubsan(host_asan, driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for k in list(env):
        if k.startswith("MATCHA_DISABLE") or k == "MATCHA_FUSED_DBG":
            env.pop(k)
    if driver == "host_checks":
        env["MATCHA_FUSED_DBG"] = "3"      # its option checks read the environment's spelling once, at first use
    run = subprocess.run([os.path.join(host_asan, driver)], capture_output=True, text=True, env=env, timeout=600)
    out = run.stdout + run.stderr
    assert run.returncode == 0, out[-4000:]
    assert DRIVERS[driver] in out
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
