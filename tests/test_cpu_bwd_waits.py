"""The waits behind fused_bwdh_kernel's per-node float atomics, read off the build's device assembly (fused_bwd.hip, the rotated walk;
DESIGN.md 4.3) -- in the manner of tests/test_cpu_isa_audit.py.

vmcnt retires in order, and when the compiler waits for a staged load it counts the memory operations it KNOWS to be newer.  A float atomic
stays counted for ~1.2 us with the chip busy, so a wait of the next half tile's staging that leaves fewer operations in flight than the d x_hat
phase's adds drains them in front of a barrier, once per half tile.  The walk of the per-node adds is shaped so that the compiler's own count
includes them: eight straight-line atomics, nothing the staging consumes issued behind them, the staging reachable from the loop body only.
Checked for the headline instance <5, true, true> and for <8, true, true>:
  * the walk holds exactly eight float atomics in ONE basic block (none behind a branch of its own);
  * from the last of them to the barrier that closes the staging -- down to the loop's back edge, then from the loop's head to its first
    barrier -- every s_waitcnt that names vmcnt leaves at least eight operations in flight.  (Every one, also those that only one wavefront
    executes: stricter than needed, and it holds.)
The adds are buffer_atomic_add_f32 (a lane past the half tile's tokens is dropped by the descriptor's range check); global_atomic_add_f32, the
same memory-side operation, is accepted as well.  Skips when the assembly is absent (a tree that was never built).
"""
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDS = 8
ATOMIC = re.compile(r"^(global|buffer)_atomic_add_f32\b")
BRANCH = re.compile(r"^s_c?branch\w*\s+(\.LBB\d+_\d+)")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
VMCNT = re.compile(r"^s_waitcnt\b.*\bvmcnt\((\d+)\)")


def _kernel(stem, mangled):
    """The instructions (comments stripped) of the one kernel of build/csrc/<stem>-...gfx950.s whose symbol contains `mangled`."""
    paths = glob.glob(os.path.join(ROOT, "build", "csrc", f"{stem}-hip-amdgcn-amd-amdhsa-gfx950.s"))
    if not paths:
        pytest.skip("no device assembly: the library was not built in this tree")
    lines = open(paths[0]).read().split("\n")
    starts = [i for i, l in enumerate(lines) if re.match(r"^_Z\w+:", l) and mangled in l]
    assert len(starts) == 1, (mangled, len(starts))
    out = []
    for l in lines[starts[0] + 1:]:
        s = l.split(";")[0].strip()
        if s:
            out.append(s)
        if s == "s_endpgm":
            break
    return out


def _node_walk(ins):
    """(head, first add, last add, back edge) of the loop whose body holds the straight-line run of atomics."""
    at = [i for i, s in enumerate(ins) if ATOMIC.match(s)]
    runs, run = [], []
    for i in at:                                               # runs of atomics with neither a label nor a branch between two of them
        if run and any(LABEL.match(s) or BRANCH.match(s) for s in ins[run[-1]:i]):
            runs.append(run)
            run = []
        run.append(i)
    runs.append(run)
    straight = [r for r in runs if len(r) == ADDS]
    assert len(straight) == 1, [len(r) for r in runs]
    first, last = straight[0][0], straight[0][-1]
    label_at = {LABEL.match(s).group(1): i for i, s in enumerate(ins) if LABEL.match(s)}
    for i in range(last + 1, len(ins)):                        # the back edge: the first branch behind the adds to a label in front of them
        m = BRANCH.match(ins[i])
        if m and label_at.get(m.group(1), len(ins)) < first:
            head = label_at[m.group(1)]
            assert [j for j in at if head <= j <= i] == straight[0], "the walk's body holds other atomics than the eight"
            return head, first, last, i
    raise AssertionError("no back edge behind the adds")


@pytest.mark.parametrize("ml", [5, 8])
def test_no_wait_of_the_staging_drains_the_adds(ml):
    ins = _kernel("fused_bwd", f"fused_bwdh_kernelILi{ml}ELb1ELb1EE")
    head, first, last, back = _node_walk(ins)
    barrier = next(i for i in range(head, first) if ins[i].startswith("s_barrier"))
    region = ins[last + 1:back + 1] + ins[head:barrier + 1]
    assert sum(1 for s in ins[last + 1:back + 1] if s.startswith("s_barrier")) == 1      # the barrier in front of the staging
    waits = [int(VMCNT.match(s).group(1)) for s in region if VMCNT.match(s)]
    assert waits, "the staging waits for nothing?"
    assert min(waits) >= ADDS, waits
    # nothing the staging consumes is issued behind the adds: no load between them and the back edge
    assert not [s for s in ins[last + 1:back + 1] if re.match(r"^(global|buffer|flat)_load", s)]


def test_the_other_walk_keeps_its_branches():
    """The per-token adds (dx_atomic without dx_node) keep their text: one branch per add, in a loop of their own."""
    ins = _kernel("fused_bwd", "fused_bwdh_kernelILi5ELb1ELb1EE")
    assert sum(1 for s in ins if ATOMIC.match(s)) == 2 * ADDS
    assert sum(1 for s in ins if s.startswith("buffer_atomic_add_f32")) == ADDS
