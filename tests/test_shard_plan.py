"""The planning of the host protein call (kmers.anno_amd/csrc/kma_shard_plan.h: the pieces of
whole proteins, one kernel each, and the copy segments and packing chunks of the streamed
pipeline) on the host: kmers.anno_amd/host/shard_plan_check.cpp is a stand-alone program built
with -fsanitize=address,undefined that plans offsets arrays alone (one protein, less than a group,
no residues, whole groups and one residue more, piece boundaries on group edges and one residue
to either side, empty proteins, one giant protein with empty pieces behind it, piece limits of
1 to 16 and beyond, and the library's own shape on 40M residues), each with equal and with ramped
pieces, and checks every plan: the piece boundaries against a linear scan, the segments' tiling,
sizes and owners, the chunk maps, and that no piece's kernel would be launched before every
group holding its residues has been queued. The group-edge and empty-protein cases also assert
that their plans reach what they are named for (a middle boundary at residue 8192, 8193 and
8191; a boundary on the first of several empty proteins). A failed check ends its case only, so
the program lists every failing case. The test builds and runs it."""
import os
import subprocess

from conftest import PKG

# 24 offsets arrays / limits (5 tiny, 2 whole-group, 3 group-edge, 2 with empty proteins, 4 with a
# giant protein, 6 piece limits, 64 KiB pieces, the defaults), each with and without the ramp
CASES = 2 * (5 + 2 + 3 + 2 + 4 + 6 + 1 + 1)


def test_shard_plans_hold_their_invariants_under_sanitizers():
    subprocess.run(["make", "-s", "-C", PKG, "build/kma_shard_plan_check"], check=True)
    exe = os.path.join(PKG, "build", "kma_shard_plan_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert CASES == 48 and f"shard_plan_check ok: {CASES} cases" in r.stdout
