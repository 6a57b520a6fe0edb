#!/usr/bin/env python3
"""Measures the projector's translation stage: kma_translate_locations on one
GPU, for small.gto's 712 pegs and for the synthetic 5 Mbp genome (config 3's generator) with
every extended ORF of its ~10^6 proposals (scripts/orf_extend_measure.py's case, through
OrfIndex / extend_proposals; the rejected ones have no ORF):

  - the whole call from Python (kmeranno.translate_locations: sizing, validation, allocation, H2D
    of the DNA, the locations and the offsets, the kernel, D2H of the residues), synchronous, by
    the host clock: the median of --repeat calls after one warm-up call, with min and max;
  - the kernel alone by hipEvents around its launch (kmeranno.translate_kernel_ms), over the
    same calls;
  - the same locations through the host restatement kmeranno.projector.peg_translate, and
    through the C oracle's orc_translate (one thread; the '-' strand through its
    orc_reverse_complement first), each on a sample of --sample locations (all of them when
    there are fewer) and scaled by residues to the whole set.

The GPU's residues are compared with the host restatement's on the sample before anything is
reported. No threshold: the record is the baseline.

    python scripts/translate_measure.py [--out FILE.json] [--proposals 1000000] [--sample 10000]
"""
import argparse
import ctypes as C
import gzip
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kmers.anno_amd", "python"), os.path.join(ROOT, "scripts")]

import torch  # noqa: E402,F401  (torch's HIP runtime first; libkmeranno binds it by SONAME)

import kmeranno as kma  # noqa: E402
from kmeranno import projector  # noqa: E402
from oracle import c_oracle  # noqa: E402
from orf_extend_measure import synthetic_case  # noqa: E402


def small_gto_case():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "small.gto.gz"), "rt") as f:
        gto = json.load(f)
    ids = [c["id"] for c in gto["contigs"]]
    rows = []
    for f in gto["features"]:
        if f.get("protein_translation") and len(f["location"]) == 1:
            cid, begin, strand, length = f["location"][0]
            begin, length = int(begin), int(length)
            rows.append((ids.index(cid), strand, begin, begin + length - 1) if strand == "+"
                        else (ids.index(cid), strand, begin - length + 1, begin))
    contigs = [c["dna"] for c in gto["contigs"]]
    dna, doff = kma.pack_strings(contigs)
    return "small.gto's pegs", contigs, dna, doff, kma.make_locations(rows)


def synthetic_orfs(n_props):
    name, contigs, dna, doff, props = synthetic_case(n_props)
    with kma.OrfIndex(dna, doff) as idx:
        left, right, status, _ = kma.extend_proposals(idx, props, 0.0, 0)
    keep = status != kma.ORF_REJECTED
    locs = np.zeros(int(keep.sum()), kma.LOCATION_DTYPE)
    locs["contig"] = props["contig"][keep]
    locs["strand"] = props["strand"][keep]
    locs["left"] = left[keep]
    locs["right"] = right[keep]
    return name + ", every extended ORF", contigs, dna, doff, locs


def measure(name, contigs, dna, doff, locs, repeat, sample):
    call_ms, kernel_ms = [], []
    for i in range(repeat + 1):  # the first call warms up: code objects, allocator
        t = time.perf_counter()
        res, off = kma.translate_locations(dna, doff, locs, 11, peg=True)
        dt = (time.perf_counter() - t) * 1e3
        if i:
            call_ms.append(dt)
            kernel_ms.append(kma.translate_kernel_ms())
    residues = int(off[-1])
    rng = np.random.default_rng(1)
    pick = np.arange(len(locs)) if len(locs) <= sample else \
        np.sort(rng.choice(len(locs), sample, replace=False))
    plocs = [projector.Location(int(x["contig"]), chr(x["strand"]), int(x["left"]),
                                int(x["right"])) for x in locs[pick]]
    t = time.perf_counter()
    host = [projector.peg_translate(contigs[p.contig], p, 11, True) for p in plocs]
    host_s = time.perf_counter() - t
    text = res.tobytes()
    for i, h in zip(pick.tolist(), host):  # the sample agrees before anything is reported
        assert text[int(off[i]):int(off[i + 1])].decode() == h, i
    sample_res = sum(len(h) for h in host)
    # the C oracle, one thread: substring (reverse complemented on '-'), orc_translate; the trim
    # and the M rule are not its work and are left out of its time
    lib = c_oracle.lib()
    lib.orc_reverse_complement.argtypes = [C.c_char_p, C.c_int64, C.c_char_p]
    raw = [c.encode() for c in contigs]
    buf = C.create_string_buffer(max((p.length for p in plocs), default=0) + 8)
    out = C.create_string_buffer(len(buf) // 3 + 8)
    t = time.perf_counter()
    n_orc = 0
    for p in plocs:
        sub = raw[p.contig][p.left - 1:p.right]
        if p.strand == "-":
            lib.orc_reverse_complement(sub, len(sub), buf)
            sub = buf.raw[:len(sub)]
        n_orc += lib.orc_translate(sub, len(sub), 1, 11, out)
    orc_s = time.perf_counter() - t
    assert n_orc == sample_res + sum(p.length >= 3 for p in plocs)
    scale = residues / max(sample_res, 1)
    bases = int(np.maximum(locs["right"].astype(np.int64) - locs["left"] + 1, 0).sum())

    def stat(v):
        return {"median": statistics.median(v), "min": min(v), "max": max(v)}
    return {
        "case": name, "genome_bases": int(doff[-1] - doff[0]), "locations": len(locs),
        "location_bases": bases, "residues": residues,
        "call_ms": stat(call_ms), "kernel_ms": stat(kernel_ms),
        "kernel_gb_per_s": (bases + residues) / (statistics.median(kernel_ms) * 1e-3) / 1e9,
        "host_sample": len(pick), "host_sample_residues": sample_res,
        "host_peg_translate_ms_scaled": host_s * 1e3 * scale,
        "host_peg_translate_ns_per_residue": host_s * 1e9 / max(sample_res, 1),
        "c_oracle_ms_scaled": orc_s * 1e3 * scale,
        "c_oracle_ns_per_residue": orc_s * 1e9 / max(sample_res, 1),
        "ratio_host_over_call": host_s * 1e3 * scale / statistics.median(call_ms),
        "ratio_c_oracle_over_call": orc_s * 1e3 * scale / statistics.median(call_ms),
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
               measure(*synthetic_orfs(a.proposals), a.repeat, a.sample)]
    doc = {"device": torch.cuda.get_device_name(0), "results": results}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
