"""Measurements of the streamed signature build, on one GPU.

  1. The stages of one add (hipEvent times from the library's measurement hook
     kma_debug_sig_builder_ms: windows, sort, reduce, merge count pass + scan, merge write pass,
     counts) for an add of --add-residues random residues into a run of --run-keys keys. The same
     batch is added again and again: the combine is idempotent, so the run keeps its size and every
     repeat does the whole work. Warm, median of --repeats.
  2. The merge's bytes moved over its time, 12 (nA + nB) read and 12 n_out written per pass that
     moves them, next to a device-to-device copy of the run's size (read + written bytes over its
     event time).
  3. The whole build of --build-residues residues: kma_build_signatures against the builder in 1
     and in 8 adds, wall time of the calls (host buffers in, rows out), median of --build-repeats.

    python scripts/sigbuild_rate.py [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kmers.anno_amd", "python"))
import kmeranno as kma  # noqa: E402

AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
STAGES = ("windows", "sort", "reduce", "merge_count", "merge_write", "counts")


def proteins(rng, n_residues, length=320, n_roles=500):
    n = n_residues // length
    res = np.r_[AA[rng.integers(0, 20, n * length)], np.zeros(32, np.uint8)]
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(length)
    roles = rng.integers(0, n_roles, n).astype(np.int32)
    roles[rng.random(n) < 0.1] = -1
    return res, off, roles


def stage_ms(b):
    out = (C.c_double * 6)()
    assert kma.load().kma_debug_sig_builder_ms(b.handle, out) == 0
    return list(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run-keys", type=int, default=100_000_000)
    ap.add_argument("--add-residues", type=int, default=16_000_000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--build-residues", type=int, default=64_000_000)
    ap.add_argument("--build-repeats", type=int, default=5)
    ap.add_argument("--json")
    a = ap.parse_args()
    kma.load().kma_debug_sig_builder_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    rng = np.random.default_rng(1)
    out = {}

    with kma.SigBuilder(8) as b:
        while b.info().n_keys < a.run_keys:
            b.add(*proteins(rng, a.add_residues))
        batch = proteins(rng, a.add_residues)
        b.add(*batch)
        n_a = int(b.info().n_keys)
        rows, walls = [], []
        for _ in range(a.repeats + 2):
            t0 = time.perf_counter()
            b.add(*batch)
            walls.append((time.perf_counter() - t0) * 1e3)
            rows.append(stage_ms(b))
        assert int(b.info().n_keys) == n_a
        med = {s: statistics.median(r[i] for r in rows[2:]) for i, s in enumerate(STAGES)}
        i = b.info()
        out["add"] = {"run_keys": n_a, "add_residues": a.add_residues, "stage_ms": med,
                      "wall_ms": statistics.median(walls[2:]), "bytes_held": int(i.bytes),
                      "by_state": [int(i.n_role), int(i.n_conflict), int(i.n_buffered)]}
    # the batch's reduced size: one add of it alone
    with kma.SigBuilder(8) as b1:
        b1.add(*batch)
        n_b = int(b1.info().n_keys)
    moved = 12 * (n_a + n_b)
    out["merge"] = {"n_a": n_a, "n_b": n_b, "n_out": n_a,
                    "count_pass_GBps": moved / med["merge_count"] / 1e6,
                    "write_pass_GBps": (moved + 12 * n_a) / med["merge_write"] / 1e6}
    # a device-to-device copy of the run's size
    src = torch.empty(12 * n_a, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    times = []
    for _ in range(a.repeats + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    copy_gbps = 2 * 12 * n_a / statistics.median(times[2:]) / 1e6
    out["merge"]["d2d_copy_GBps"] = copy_gbps
    out["merge"]["write_pass_fraction_of_copy"] = out["merge"]["write_pass_GBps"] / copy_gbps
    del src, dst

    res, off, roles = proteins(rng, a.build_residues)
    n = len(roles)

    def one_shot():
        return kma.build_signatures(res, off, roles, 8)

    def streamed(parts):
        with kma.SigBuilder(8) as b:
            cuts = np.linspace(0, n, parts + 1).astype(int)
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                lo_r, hi_r = int(off[lo]), int(off[hi])
                b.add(np.r_[res[lo_r:hi_r], np.zeros(32, np.uint8)], off[lo:hi + 1] - off[lo],
                      roles[lo:hi])
            return b.finish()

    want = one_shot()
    build = {}
    for name, fn in (("one_shot", one_shot), ("builder_1_add", lambda: streamed(1)),
                     ("builder_8_adds", lambda: streamed(8))):
        t = []
        for _ in range(a.build_repeats + 1):
            t0 = time.perf_counter()
            got = fn()
            t.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        build[name + "_ms"] = statistics.median(t[1:])
    build["rows"] = len(want[0])
    build["residues"] = int(off[-1])
    build["ratio_1_add"] = build["builder_1_add_ms"] / build["one_shot_ms"]
    build["ratio_8_adds"] = build["builder_8_adds_ms"] / build["one_shot_ms"]
    out["build"] = build
    print(json.dumps(out, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
