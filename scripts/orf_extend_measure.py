#!/usr/bin/env python3
"""Measures the projector's ORF-extension stage ("ORF extension"): for small.gto
projected onto itself and for a synthetic 5 Mbp genome (config 3's generator) with ~10^6
proposals, on one GPU:

  - kma_orf_index_create: wall time of the call (allocation, H2D copy of the DNA, the classify
    kernel and the two scans, synchronised) and the device bytes it keeps;
  - kma_extend_proposals: wall time per call (H2D of the proposals, the kernel, D2H of the three
    output arrays, synchronised);
  - the host path it replaces: kmeranno.projector.extend, the per-proposal codon walk, timed on
    a sample of the same proposals (all of them when there are fewer than --sample) and scaled
    to the whole set.

Both library calls are synchronous, so a host clock around them is a device-synchronised time.
Every figure is the median of --repeat calls after one warm-up call. The GPU results are checked
against the host walk on the sample before anything is reported.

    python scripts/orf_extend_measure.py [--out FILE.json] [--proposals 1000000] [--sample 10000]
"""
import argparse
import gzip
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kmers.anno_amd", "python")]

import torch  # noqa: E402,F401  (torch's HIP runtime first; libkmeranno binds it by SONAME)

import kmeranno as kma  # noqa: E402
from kmeranno import projector, synth  # noqa: E402

K = 8


def median_ms(fn, repeat):
    fn()  # warm-up: code objects, allocator
    out = []
    for _ in range(repeat):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out), min(out), max(out)


def small_gto_case():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "small.gto.gz"), "rt") as f:
        gto = json.load(f)
    rng = np.random.default_rng(9)
    prots = [f["protein_translation"] for f in gto["features"] if f.get("protein_translation")]
    aa = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
    close = []
    for p in prots:
        b = np.frombuffer(p.encode(), np.uint8).copy()
        m = rng.random(len(b)) < 0.05
        b[m] = aa[rng.integers(0, 20, int(m.sum()))]
        close.append(b.tobytes().decode())
    res, off = kma.pack_strings(close)
    contigs = [c["dna"] for c in gto["contigs"]]
    dna, doff = kma.pack_strings(contigs)
    t, _ = kma.SignatureTable.from_pegs(res, off, K)
    with t:
        hits = kma.connect_pegs(t, dna, doff, 11, False)
    props, _ = kma.propose_pegs(hits, np.array([len(p) for p in close], np.uint32), K)
    return "small.gto onto itself", contigs, dna, doff, props


def synthetic_case(n_props, seed=3):
    """Config 3's genome (5 Mbp, 20 contigs, genes planted on both strands) and n_props
    proposals as the sweep shapes them: in a gene's frame, from a random codon of the gene to a
    later one, with a random evidence."""
    wl = synth.make_contig_workload(table_size=100_000, n_fid=1000, seed=seed)
    rng = np.random.default_rng(seed + 100)
    lens = np.diff(wl.offsets).astype(np.int64)
    g = wl.genes[rng.integers(0, len(wl.genes), n_props)]
    # the gene's extent: to the next gene start on its contig is not recorded; walk to its stop
    first = rng.integers(0, 60, n_props) * 3
    span = rng.integers(8, 120, n_props) * 3
    left0 = g[:, 1] + first  # 0-based forward left edge, in the gene's frame on either strand
    right0 = np.minimum(left0 + span - 1, lens[g[:, 0]] - 1)
    keep = right0 - left0 + 1 >= 24
    props = np.zeros(int(keep.sum()), kma.PROPOSAL_DTYPE)
    props["contig"] = g[keep, 0]
    props["left"] = left0[keep] + 1
    props["right"] = right0[keep] + 1
    props["strand"] = np.where(g[keep, 2] > 0, ord("+"), ord("-"))
    props["evidence"] = rng.integers(1, 80, len(props))
    dna = np.ascontiguousarray(wl.dna)
    text = dna[:int(wl.offsets[-1])].tobytes().decode()
    contigs = [text[int(wl.offsets[c]):int(wl.offsets[c + 1])] for c in range(wl.n_contig)]
    return "synthetic 5 Mbp (config 3)", contigs, dna, wl.offsets, props


def measure(name, contigs, dna, doff, props, repeat, sample, min_strength=0.5 / 3, min_evidence=10):
    bases = int(doff[-1] - doff[0])
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    idx = kma.OrfIndex(dna, doff)
    free1 = torch.cuda.mem_get_info()[0]
    idx.close()
    slots = 2 * sum(3 * ((len(c) + 2) // 3) for c in contigs)
    layout_bytes = 8 * slots + 12 * len(contigs) + 8

    def build():
        kma.OrfIndex(dna, doff).close()
    build_ms = median_ms(build, repeat)
    with kma.OrfIndex(dna, doff) as idx:
        ext_ms = median_ms(lambda: kma.extend_proposals(idx, props, min_strength, min_evidence),
                           repeat)
        left, right, status, stats = kma.extend_proposals(idx, props, min_strength, min_evidence)
    # the host path: projector.extend per proposal, on a sample
    rng = np.random.default_rng(1)
    pick = np.arange(len(props)) if len(props) <= sample else \
        np.sort(rng.choice(len(props), sample, replace=False))
    locs = [projector.Location(int(p["contig"]), chr(p["strand"]), int(p["left"]),
                               int(p["right"])) for p in props[pick]]
    t = time.perf_counter()
    real = [projector.extend(contigs[loc.contig], loc, 11) for loc in locs]
    host_s = time.perf_counter() - t
    for i, r in zip(pick.tolist(), real):  # the sample agrees before anything is reported
        want = (0, 0) if r is None else (r.left, r.right)
        assert (int(left[i]), int(right[i])) == want, (i, want, int(left[i]), int(right[i]))
        assert (status[i] == kma.ORF_REJECTED) == (r is None)
    host_ms = host_s * 1e3 * len(props) / len(pick)
    return {
        "case": name, "bases": bases, "contigs": len(contigs), "proposals": len(props),
        "status_counts": {"made": int(stats[0]), "rejected": int(stats[1]),
                          "weak": int(stats[2]), "small": int(stats[3])},
        "index_build_ms": {"median": build_ms[0], "min": build_ms[1], "max": build_ms[2]},
        "extend_call_ms": {"median": ext_ms[0], "min": ext_ms[1], "max": ext_ms[2]},
        "host_extend_ms_scaled": host_ms, "host_sample": len(pick),
        "host_us_per_proposal": host_s * 1e6 / len(pick),
        "ratio_host_over_extend_call": host_ms / ext_ms[0],
        "ratio_host_over_build_plus_extend": host_ms / (build_ms[0] + ext_ms[0]),
        "index_bytes_layout": layout_bytes, "index_bytes_per_base_layout": layout_bytes / bases,
        "index_bytes_allocator": int(free0 - free1),
        "index_bytes_per_base_allocator": (free0 - free1) / bases,
        "repeat": repeat,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--proposals", type=int, default=1_000_000)
    ap.add_argument("--sample", type=int, default=10_000)
    ap.add_argument("--repeat", type=int, default=9)
    a = ap.parse_args()
    assert kma.device_count() >= 1, "no HIP device: nothing is measured without one"
    results = [measure(*small_gto_case(), a.repeat, a.sample),
               measure(*synthetic_case(a.proposals), a.repeat, a.sample)]
    doc = {"device": torch.cuda.get_device_name(0), "results": results}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
