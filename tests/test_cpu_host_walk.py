"""The argument validation of the hypergraph walk and of the skip-gram pass (csrc/walk.hip: matcha_hyper_walk; csrc/sgns.hip:
matcha_sgns_epoch) under AddressSanitizer + UndefinedBehaviorSanitizer on the host: tests/host/walk_checks.hip, a stand-alone driver on the
host-only objects of tests/test_cpu_host_sanitizers.py -- every refusal of the two entries with its message, the integer extremes of the walk
range and of the position counter, the no-op forms.  No kernel is launched."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_walk_host_side_under_asan_ubsan():
    import matcha_amd.walk  # noqa: F401  (the feature under test)
    csrc = os.path.join(ROOT, "matcha_amd", "csrc")
    build = subprocess.run(["make", "-C", csrc, "-j", str(min(8, os.cpu_count() or 1)), "host-asan-walk"], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout[-3000:] + build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for k in list(env):
        if k.startswith("MATCHA_DISABLE") or k == "MATCHA_FUSED_DBG":
            env.pop(k)
    run = subprocess.run([os.path.join(ROOT, "build", "host_asan", "walk_checks")], capture_output=True, text=True, env=env, timeout=600)
    out = run.stdout + run.stderr
    assert run.returncode == 0, out[-4000:]
    assert "ALL WALK HOST CHECKS PASSED" in out
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
