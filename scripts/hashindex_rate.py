#!/usr/bin/env python3
"""Measures the hash annotator against a resident prototype index on one GPU.

Prototypes: c5's batch (kmeranno.synth: 1M proteins, ~310M residues; the build's stored copy
where there is one). Genomes: batches of --genome-proteins proteins from synth.make_queries over
the same families with other seeds. Reported, by the host clock around the synchronous calls:

  - kma_proto_index_create, once (and the index's sizes);
  - kma_hash_annotate per genome (both sides sent with every call: what there was before) and
    kma_hash_annotate_indexed per genome, best of --repeat after a warm-up round, the two forms
    taking turns inside every round (A B, A B, ...), so a drifting clock falls on both alike;
  - the indexed call at KMA_OPT_HASH_CAP 512 / 1024 / 2048 (LDS tables of 8 / 16 / 32 KiB), and
    at a CAP low enough to split proteins into prototype ranges;
  - per genome: proteins with a candidate, proteins split, ranges scored (out_stats).

Every genome's three outputs are checked equal between the two forms (and between the CAPs)
before anything is timed. Prints one JSON document; --out writes it to a file as well. No
threshold beyond "no slower than kma_hash_annotate": the record is the baseline.

    python scripts/hashindex_rate.py [--out profiles/hashindex/NAME.json] [--repeat 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kmers.anno_amd", "python")]

import torch  # noqa: E402  (torch's HIP runtime first; libkmeranno binds it by SONAME)

import kmeranno as kma  # noqa: E402
from kmeranno import synth, synth_cache  # noqa: E402

CAPS = (512, 1024, 2048)


def inputs(n_proto, n_genomes, genome_proteins):
    """(prototype residues, offsets), [(genome residues, offsets)]."""
    n, t_size, n_fid, seed = synth.CONFIGS["c5"]
    qseed = seed * 1_000_003 + 17
    q = synth_cache.load_queries(t_size, n_fid, seed, 8, n, qseed) if n_proto is None else None
    sig = synth.make_table(t_size, n_fid, seed, 8, protos_only=True)
    if q is None:
        q = synth.make_queries(sig, n_proto or n, qseed)
    genomes = [synth.make_queries(sig, genome_proteins, qseed + 7919 * (i + 1))[:2]
               for i in range(n_genomes)]
    c = np.ascontiguousarray
    return (c(q[0], np.uint8), c(q[1], np.uint64)), \
        [(c(g[0], np.uint8), c(g[1], np.uint64)) for g in genomes]


def wall_ms(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def same(a, b):
    return all((x == y).all() for x, y in zip(a[:3], b[:3]))


def take_turns(calls, repeat):
    """calls: {name: fn}. One warm-up round, then `repeat` rounds in which the calls take turns;
    {name: [ms per round]}."""
    ms = {k: [] for k in calls}
    for r in range(repeat + 1):
        for name, fn in calls.items():
            t = wall_ms(fn)[0]
            if r:
                ms[name].append(t)
    return ms


def best(v):
    return {"best": min(v), "spread": max(v) - min(v), "all": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--genomes", type=int, default=3)
    ap.add_argument("--genome-proteins", type=int, default=4000)
    ap.add_argument("--low-cap", type=int, default=16)
    ap.add_argument("--n-proto", type=int, help="a smaller prototype batch of the same generator "
                    "(trials)")
    a = ap.parse_args()
    t0 = time.perf_counter()
    (pr, po), genomes = inputs(a.n_proto, a.genomes, a.genome_proteins)
    load_s = time.perf_counter() - t0
    assert kma.device_count() >= 1, "no HIP device: nothing is measured without one"
    torch.cuda.synchronize()
    create_ms, idx = wall_ms(lambda: kma.ProtoIndex(pr, po, k=8))
    info = idx.info()
    doc = {
        "device": torch.cuda.get_device_name(0), "batch": "c5" if a.n_proto is None else "trial",
        "prototypes": int(info.n_proto), "prototype_residues": int(po[-1] - po[0]),
        "input_load_s": load_s, "repeat": a.repeat, "clock": "host, around the synchronous call",
        "index_create_ms": create_ms, "index_unique_keys": int(info.n_keys),
        "index_postings": int(info.n_postings), "index_device_bytes": int(info.bytes),
        "default_cap": 1024, "genomes": [],
    }
    with idx:
        for gi, (gr, go) in enumerate(genomes):
            plain = kma.hash_annotate(gr, go, pr, po, 8, 0.0125)
            ref = kma.hash_annotate_indexed(idx, gr, go, 0.0125, stats=True)
            assert same(ref, plain), f"genome {gi}: the indexed call differs"
            stats = {"default": [int(x) for x in ref[3]]}
            for cap in CAPS + (a.low_cap,):  # every CAP gives the same outputs before it is timed
                with kma.options(hash_cap=cap):
                    got = kma.hash_annotate_indexed(idx, gr, go, 0.0125, stats=True)
                assert same(got, plain), f"genome {gi}: CAP {cap} differs"
                stats[f"cap_{cap}"] = [int(x) for x in got[3]]

            def indexed(cap=0, gr=gr, go=go):
                def run():
                    with kma.options(hash_cap=cap):
                        kma.hash_annotate_indexed(idx, gr, go, 0.0125)
                return run

            forms = take_turns({"hash_annotate": lambda: kma.hash_annotate(gr, go, pr, po, 8,
                                                                           0.0125),
                                "hash_annotate_indexed": indexed()}, a.repeat)
            caps = take_turns({f"cap_{c}": indexed(c) for c in CAPS + (a.low_cap,)}, a.repeat)
            lens = np.diff(go).astype(np.int64)
            doc["genomes"].append({
                "proteins": len(go) - 1, "residues": int(lens.sum()),
                "proteins_with_a_best": int((ref[0] >= 0).sum()),
                "stats_candidates_split_ranges": stats,
                "call_ms": {k: best(v) for k, v in forms.items()},
                "indexed_by_cap_ms": {k: best(v) for k, v in caps.items()},
                "ratio_plain_over_indexed": min(forms["hash_annotate"]) /
                min(forms["hash_annotate_indexed"]),
            })
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
