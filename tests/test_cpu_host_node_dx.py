"""decide_route's node_dx field (model.hip: the encoder's input gradients summed per node at their producers) under AddressSanitizer +
UndefinedBehaviorSanitizer on the host: tests/host/route_node_dx.hip, a driver of its own on the host-only objects of
tests/test_cpu_host_sanitizers.py -- what the field implies over shapes, per-call options and every switch, that its switch takes out this
field alone, that the per-node replicas fit the buffer they are carved in, the sizes the rule fixes, the record.  No kernel is launched."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_node_dx_route_under_asan_ubsan():
    csrc = os.path.join(ROOT, "matcha_amd", "csrc")
    build = subprocess.run(["make", "-C", csrc, "-j", str(min(8, os.cpu_count() or 1)), "host-asan-node-dx"], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout[-3000:] + build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for k in list(env):
        if k.startswith("MATCHA_DISABLE") or k == "MATCHA_FUSED_DBG":
            env.pop(k)
    run = subprocess.run([os.path.join(ROOT, "build", "host_asan", "route_node_dx")], capture_output=True, text=True, env=env, timeout=600)
    out = run.stdout + run.stderr
    assert run.returncode == 0, out[-4000:]
    assert "ALL NODE_DX ROUTE CHECKS PASSED" in out
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
