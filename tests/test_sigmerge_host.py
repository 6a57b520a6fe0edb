"""Host side of the streamed signature build's union merge (no GPU).

kmers.anno_amd/host/sigmerge_check.cpp is a stand-alone program built with
-fsanitize=address,undefined that runs a serial model of the merge kernel from the pieces the
kernel itself is made of (csrc/kma_sigmerge.h: the combine, the merge-path split in its binary and
its 64-probe form, the A-first tie rule, the head rule for a merged position), tile by tile on heap
arrays of exactly the sizes a block stages, then the scan of the tiles' head counts and the write
pass, against a std::map fold. The cases are the tile edges: run lengths 0, 1, tile - 1, tile,
tile + 1 and 3 tile + 1 on both sides, for disjoint, interleaved, identical and shifted-identical
key sets (an equal pair then straddles a tile boundary at either parity) and random ones."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from conftest import PKG

EXE = os.path.join(PKG, "build", "kma_sigmerge_check")
PATTERNS = {0: "disjoint, B low", 1: "disjoint, B high", 2: "interleaved", 3: "identical",
            4: "identical, one more in front of A", 5: "identical, one more in front of B",
            6: "random, 30% shared"}


@pytest.fixture(scope="module")
def check_program():
    subprocess.run(["make", "-s", "-C", PKG, "build/kma_sigmerge_check"], check=True)
    return EXE


def run_check(*args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, env=env,
                          timeout=120)


@pytest.mark.parametrize("tile", [4, 8, 2048])
def test_merge_model_against_map_fold_under_sanitizers(check_program, tile):
    sizes = [0, 1, tile - 1, tile, tile + 1, 3 * tile + 1]
    cases = [(na, nb, tile, 1000 * p + 7 * ia + ib, p) for p in PATTERNS
             for ia, na in enumerate(sizes) for ib, nb in enumerate(sizes)]
    assert len(cases) == 36 * 7
    with ThreadPoolExecutor(8) as pool:
        results = list(pool.map(lambda c: run_check(*c), cases))
    shared_pairs = 0
    for c, r in zip(cases, results):
        assert r.returncode == 0, (c, PATTERNS[c[4]], r.stdout + r.stderr)
        assert r.stdout.startswith(f"sigmerge_check ok: {c[0]} + {c[1]} keys, "), (c, r.stdout)
        shared = int(r.stdout.split(" keys, ")[1].split(" shared")[0])
        if c[4] == 3:
            assert shared == min(c[0], c[1]), c
        if c[4] in (0, 1, 2):
            assert shared == 0, c
        shared_pairs += shared
    assert shared_pairs > 10 * tile  # the equal-pair path was walked


def test_merge_check_refuses_bad_arguments(check_program):
    assert run_check(1, 2, 3).returncode == 2
    assert run_check(4, 4, 0, 1, 0).returncode == 2
    assert run_check(4, 4, 8, 1, 9).returncode == 2
