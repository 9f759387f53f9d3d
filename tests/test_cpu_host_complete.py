"""Cluster completion's host side (csrc/sweep_rows.hip: matcha_kway_complete_count, the argument checks of matcha_kway_complete_rows) under
AddressSanitizer + UndefinedBehaviorSanitizer on the host: tests/host/complete_checks.hip, a stand-alone driver on the host-only objects of
tests/test_cpu_host_sanitizers.py -- the count against a 128-bit restatement over a grid that includes every integer extreme, every
refusal with its message, the no-op forms.  No kernel is launched."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_completion_host_side_under_asan_ubsan():
    csrc = os.path.join(ROOT, "matcha_amd", "csrc")
    build = subprocess.run(["make", "-C", csrc, "-j", str(min(8, os.cpu_count() or 1)), "host-asan-complete"], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout[-3000:] + build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for k in list(env):
        if k.startswith("MATCHA_DISABLE") or k == "MATCHA_FUSED_DBG":
            env.pop(k)
    run = subprocess.run([os.path.join(ROOT, "build", "host_asan", "complete_checks")], capture_output=True, text=True, env=env, timeout=600)
    out = run.stdout + run.stderr
    assert run.returncode == 0, out[-4000:]
    assert "ALL CLUSTER COMPLETION HOST CHECKS PASSED" in out
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
