#!/usr/bin/env python3
"""Measures the sequence MD5 and the duplicate check on one GPU, on c5's batch
(kmeranno.synth: 1M proteins, ~310M residues; the build's stored copy where there is one):

  - kma_sequence_md5_device in its four kernel forms (refill or static lanes x per-lane 16-byte
    loads or loads through LDS; csrc/kma_md5.hip), flag 0, and the shipped form with
    KMA_MD5_UPPER: hipEvents around the launch, best of --repeat after a warm-up round. The
    forms take turns inside every round (A B C D, A B C D, ...), so a drifting clock falls on
    all of them alike;
  - the refill form at 4 .. 32 waves per compute unit;
  - the longest-sequence floor: a batch that is one 70,000-residue sequence, every form;
  - kma_check_sequences (host buffers: copy in, digests, two sorts, run heads, reductions,
    copy out), by hipEvents on the null stream around the call, and by the host clock;
  - hashlib.md5 over the same batch on --workers processes (before the GPU is initialised: the
    workers are forked), which also gives every digest the forms are compared with.

Prints one JSON document; --out writes it to a file as well. No threshold: the record is the
baseline.

    python scripts/md5_rate.py [--out profiles/md5/NAME.json] [--repeat 5] [--workers 16]
"""
import argparse
import hashlib
import json
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kmers.anno_amd", "python")]

import torch  # noqa: E402  (torch's HIP runtime first; libkmeranno binds it by SONAME)

import kmeranno as kma  # noqa: E402
from kmeranno import synth, synth_cache  # noqa: E402

FORMS = {"refill_lane": 0, "static_lane": kma.MD5_STATIC, "refill_lds": kma.MD5_COOP,
         "static_lds": kma.MD5_STATIC | kma.MD5_COOP}
_BATCH = None


def c5_batch(n_seq=None):
    n, t_size, n_fid, seed = synth.CONFIGS["c5"]
    qseed = seed * 1_000_003 + 17
    q = synth_cache.load_queries(t_size, n_fid, seed, 8, n, qseed) if n_seq is None else None
    if q is None:
        sig = synth.make_table(t_size, n_fid, seed, 8, protos_only=True)
        q = synth.make_queries(sig, n_seq or n, qseed)
    return np.ascontiguousarray(q[0], np.uint8), np.ascontiguousarray(q[1], np.uint64)


def _hash_range(span):
    res, off = _BATCH
    lo, hi = span
    buf = memoryview(res)
    return b"".join(hashlib.md5(buf[int(off[i]):int(off[i + 1])]).digest() for i in range(lo, hi))


def cpu_digests(res, off, workers):
    """hashlib over the batch on forked workers: (seconds, (n, 16) digests)."""
    global _BATCH
    _BATCH = (res, off)
    n = len(off) - 1
    cuts = np.linspace(0, n, 8 * workers + 1).astype(np.int64)
    spans = [(int(a), int(b)) for a, b in zip(cuts[:-1], cuts[1:])]
    with multiprocessing.get_context("fork").Pool(workers) as pool:
        pool.map(_hash_range, spans[:workers])  # (workers started and warm)
        t = time.perf_counter()
        parts = pool.map(_hash_range, spans, chunksize=1)
        dt = time.perf_counter() - t
    return dt, np.frombuffer(b"".join(parts), np.uint8).reshape(n, 16)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def time_forms(calls, repeat):
    """calls: {name: fn}. One warm-up round, then `repeat` rounds in which the calls take turns;
    {name: [ms per round]}."""
    ms = {k: [] for k in calls}
    for r in range(repeat + 1):
        for name, fn in calls.items():
            t = event_ms(fn)
            if r:
                ms[name].append(t)
    return ms


def on_device(res, off):
    return torch.from_numpy(res).cuda(), torch.from_numpy(off.view(np.int64)).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--n-seq", type=int, help="a smaller batch of the same generator (trials)")
    a = ap.parse_args()
    t0 = time.perf_counter()
    res, off = c5_batch(a.n_seq)
    n, n_res = len(off) - 1, int(off[-1] - off[0])
    lens = np.diff(off).astype(np.int64)
    blocks = int(((lens + 8) // 64 + 1).sum())
    load_s = time.perf_counter() - t0
    cpu_s, want = cpu_digests(res, off, a.workers)
    assert kma.device_count() >= 1, "no HIP device: nothing is measured without one"
    stream = torch.cuda.current_stream().cuda_stream
    d_res, d_off = on_device(res, off)
    d_dig = torch.zeros((n, 16), dtype=torch.uint8, device="cuda")

    def md5(form, flags=0, waves=0, d=(d_res, d_off, n, n_res, d_dig)):
        return lambda: kma.sequence_md5_device(d[0].data_ptr(), d[1].data_ptr(), d[2], d[3],
                                               d[4].data_ptr(), flags, stream=stream, form=form,
                                               waves_per_cu=waves)

    for name, form in FORMS.items():  # every form gives hashlib's digests before it is timed
        d_dig.zero_()
        md5(form)()
        torch.cuda.synchronize()
        assert (d_dig.cpu().numpy() == want).all(), name
    calls = {k: md5(f) for k, f in FORMS.items()}
    calls["refill_lane_upper"] = md5(0, kma.MD5_UPPER)
    forms_ms = time_forms(calls, a.repeat)
    waves_ms = time_forms({f"waves_{w}": md5(0, 0, w) for w in (4, 8, 16, 32)}, a.repeat)
    # the floor: one sequence of 70,000 residues
    one = np.ascontiguousarray(res[:70_000 + 32])
    one_off = np.array([0, 70_000], np.uint64)
    d_one = on_device(one, one_off) + (1, 70_000, torch.zeros((1, 16), dtype=torch.uint8,
                                                               device="cuda"))
    floor_ms = time_forms({k: md5(f, d=d_one) for k, f in FORMS.items()}, a.repeat)
    torch.cuda.synchronize()
    assert bytes(d_one[4].cpu().numpy()[0]) == hashlib.md5(one[:70_000].tobytes()).digest()
    # the duplicate check, host buffers
    fun = (np.arange(n) % 7).astype(np.uint32)
    check_ms, check_wall = [], []
    for r in range(a.repeat + 1):
        t = time.perf_counter()
        ms = event_ms(lambda: kma.check_sequences(res, off, fun))
        if r:
            check_ms.append(ms)
            check_wall.append((time.perf_counter() - t) * 1e3)
    rep, size, mixed, stats = kma.check_sequences(res, off, fun)
    groups = {}
    for i in range(n):
        if lens[i]:
            groups.setdefault(want[i].tobytes(), []).append(i)
    assert int(stats[0]) == len(groups)
    assert all(rep[m[-1]] == m[0] and size[m[0]] == len(m) for m in groups.values())

    def best(v):
        return {"best": min(v), "all": v}
    lane = min(forms_ms["refill_lane"])
    doc = {
        "device": torch.cuda.get_device_name(0), "batch": "c5" if a.n_seq is None else "trial",
        "sequences": n, "residues": n_res, "blocks": blocks, "blocks_per_sequence": blocks / n,
        "longest_sequence": int(lens.max()), "batch_load_s": load_s, "repeat": a.repeat,
        "md5_device_ms": {k: best(v) for k, v in forms_ms.items()},
        "md5_device_gb_per_s": {k: n_res / (min(v) * 1e-3) / 1e9 for k, v in forms_ms.items()},
        "md5_device_blocks_per_s": blocks / (lane * 1e-3),
        "refill_waves_per_cu_ms": {k: best(v) for k, v in waves_ms.items()},
        "one_sequence_of_70000_ms": {k: best(v) for k, v in floor_ms.items()},
        "check_sequences_event_ms": best(check_ms), "check_sequences_wall_ms": best(check_wall),
        "check_sequences_stats": [int(x) for x in stats],
        "hashlib_workers": a.workers, "hashlib_s": cpu_s,
        "hashlib_gb_per_s": n_res / cpu_s / 1e9,
        "ratio_hashlib_over_kernel": cpu_s * 1e3 / lane,
    }
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
