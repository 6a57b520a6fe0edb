#!/usr/bin/env python3
"""What the protein probe's early exit can skip, sized on the CPU.

    python scripts/early_exit_model.py c5 [--sample N]

A protein with two different fids on its record ends AMBIGUOUS whatever else it hits, and
annotate_kernel stops probing it from the next step of its block on. This script takes a bench
workload's table and batch (kmeranno.synth_cache's copy where the build stored one, else the
generator), looks every window up in the table on the CPU (a sorted-key search: the fid of
every window, -1 for a miss) and applies the library's own block assignment: proteins
[g P, g P + P) form block g (P = 6 for c5, 4 for c4 and c2: kma_abi.cpp's block_proteins),
window i of a protein that starts `base` residues into its block's span is span position
base + i. "Library order" below is the probe's order up to DESIGN 5.7: a step takes 512
consecutive span positions (256 threads x 2). The order the kernel has now is the
strided one: a block of T = ceil(span / 512) steps has 64-position chunks [0, 8 T), and step s
takes chunks r T + s, r = 0..7, so span position x is probed in step (x // 64) % T.

Per protein: i2 = the first window whose fid differs from the protein's first hit's (none: the
protein is not AMBIGUOUS). Under complete visibility (every hit of steps <= s is on record at
the top of step s + 1; the kernel has no barrier there, so a late wave skips less) the probe
skips the protein's windows in the steps after i2's.

Printed (one JSON line), as shares of the batch's windows unless said otherwise:
  ambiguous_proteins / ambiguous_windows  proteins (of all) and windows of AMBIGUOUS proteins
  skipped_windows                         windows in a step after the one that holds i2
  dropped_walk_windows                    windows of proteins dead at their block's end that
                                          were still probed: their queued walks are dropped if
                                          the queue is flushed at the block's end (a wave's
                                          queue holds 192 walks and is flushed above 64: at
                                          ~0.046 walks per window and 128 windows per wave
                                          and step, not before ~11 steps; c5's blocks have ~4)
  walk_share                              skipped + dropped: the share of deferred walks that
                                          is not walked (walks taken as uniform over windows)
  strided_skipped_windows                 the kernel's order (built): a protein's
                                          dead step is the second smallest, over its distinct
                                          fids, of the earliest step in which that fid is hit
                                          (two fids inside one step make it the dead step);
                                          skipped are its windows in later steps
  interleaved_skipped_windows             for sizing only, not built: the same skip if a block's
                                          steps took every protein's windows in proportion
                                          (window i of w in step floor(i S / w), S the block's
                                          steps) instead of protein after protein
  called                                  proteins CALLED (distinct keys >= 5, one fid): equals
                                          bench.py's called_per_batch, which checks the pass
--sample N models every N-th block only.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "kmers.anno_amd", "python")]
from kmeranno import synth, synth_cache  # noqa: E402

K, MIN_HITS, STEP = 8, 5, 512
BLOCK_PROTEINS = {"c5": 6, "c4": 4, "c2": 4, "c1": 4}
_CODE = np.zeros(256, np.uint64)
_CODE[65:91] = np.arange(1, 27)
_CODE[42] = 27


def strided_skipped(base, w, T, hp, hi, hf):
    """Per protein, the windows the strided step order skips under complete visibility, and the
    protein's dead step (-1: it never has two fids on record). base, w, T: per protein, its
    first span position, its windows and its block's steps (>= 1); hp, hi, hf: per hit, its
    protein, its window index in the protein and its fid."""
    base, w, T = (np.asarray(v, np.int64) for v in (base, w, T))
    hp, hi, hf = (np.asarray(v, np.int64) for v in (hp, hi, hf))
    n = len(base)
    hs = ((base[hp] + hi) // 64) % T[hp]  # the step that probes the hit's window
    o = np.lexsort((hs, hf, hp))  # by protein, fid, step: each (protein, fid)'s earliest step
    p1, f1, s1 = hp[o], hf[o], hs[o]
    lead = np.ones(len(o), bool)
    lead[1:] = (p1[1:] != p1[:-1]) | (f1[1:] != f1[:-1])
    p1, s1 = p1[lead], s1[lead]
    o = np.lexsort((s1, p1))  # by protein, step: the second row of a protein is its dead step
    p1, s1 = p1[o], s1[o]
    second = (np.arange(len(p1)) - np.searchsorted(p1, p1, "left")) == 1
    dead = np.full(n, -1, np.int64)
    dead[p1[second]] = s1[second]
    wstart = np.zeros(n + 1, np.int64)
    wstart[1:] = np.cumsum(w)
    pid = np.repeat(np.arange(n), w)
    ws = ((base[pid] + np.arange(wstart[-1]) - wstart[pid]) // 64) % T[pid]
    late = (dead[pid] >= 0) & (ws > dead[pid])
    return np.bincount(pid[late], minlength=n), dead


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", choices=sorted(BLOCK_PROTEINS))
    ap.add_argument("--sample", type=int, default=1)
    ap.add_argument("--block-proteins", type=int, default=0)
    args = ap.parse_args()
    t0 = time.time()
    n_seq, t_size, n_fid, seed = synth.CONFIGS[args.workload]
    qseed = seed * 1_000_003 + 17
    sig = synth_cache.load_table(t_size, n_fid, seed, K) or synth.make_table(t_size, n_fid, seed, K)
    q = synth_cache.load_queries(t_size, n_fid, seed, K, n_seq, qseed) or \
        synth.make_queries(sig, n_seq, qseed)
    residues, offsets = q[0], np.asarray(q[1], np.int64)
    order = np.argsort(sig.keys, kind="stable")
    skeys, sfids = sig.keys[order], sig.fids[order].astype(np.int64)
    last = np.ones(len(skeys), bool)  # duplicate keys: the last row wins
    last[:-1] = skeys[1:] != skeys[:-1]
    skeys, sfids = skeys[last], sfids[last]
    del order, last
    P = args.block_proteins or BLOCK_PROTEINS[args.workload]
    n_blocks = (n_seq + P - 1) // P
    tot = dict.fromkeys(("proteins", "windows", "amb_p", "amb_w", "skip", "drop", "inter",
                         "strided", "called"), 0)
    chunk = 4096 * args.sample  # blocks per pass
    for b0 in range(0, n_blocks, chunk):
        blocks = np.arange(b0, min(b0 + chunk, n_blocks), args.sample)
        prot = (blocks[:, None] * P + np.arange(P)[None, :]).ravel()
        prot = prot[prot < n_seq]
        lo, hi = offsets[prot], offsets[prot + 1]
        w = np.maximum(hi - lo - K + 1, 0)
        base = lo - offsets[prot - prot % P]
        bend = offsets[np.minimum(prot - prot % P + P, n_seq)] - offsets[prot - prot % P]
        S = np.maximum((bend + STEP - 1) // STEP, 1)  # the block's steps
        # every window's fid
        wstart = np.zeros(len(prot) + 1, np.int64)
        wstart[1:] = np.cumsum(w)
        pid = np.repeat(np.arange(len(prot)), w)
        idx = np.arange(wstart[-1]) - wstart[pid]  # window index in its protein
        pos = lo[pid] + idx
        key = np.zeros(len(pos), np.uint64)
        for j in range(K):
            key = (key << np.uint64(5)) | _CODE[residues[pos + j]]
        at = np.searchsorted(skeys, key)
        at[at == len(skeys)] = 0
        hit = np.flatnonzero((skeys[at] == key) & (key != 0))
        hp, hi_, hf, hk = pid[hit], idx[hit], sfids[at[hit]], key[hit]
        del pos, key, at
        # first hit's fid per protein, then the first hit with another fid
        first = np.full(len(prot), -1, np.int64)
        u, ui = np.unique(hp, return_index=True)  # hits are in window order
        first[u] = hf[ui]
        other = hf != first[hp]
        i2 = np.full(len(prot), -1, np.int64)
        u2, ui2 = np.unique(hp[other], return_index=True)
        i2[u2] = hi_[other][ui2]
        amb = i2 >= 0
        # CALLED: one fid, >= MIN_HITS distinct keys
        pk = np.unique(np.stack([hp.astype(np.uint64), hk]), axis=1)
        distinct = np.bincount(pk[0].astype(np.int64), minlength=len(prot))
        tot["called"] += int(((first >= 0) & ~amb & (distinct >= MIN_HITS)).sum())
        # library order: windows of the protein in steps after i2's
        kept = np.minimum(w, ((base + i2) // STEP + 1) * STEP - base)
        skip = np.where(amb, w - kept, 0)
        # interleaved order
        si = np.where(w > 0, i2 * S // np.maximum(w, 1), 0)
        kept_i = np.minimum(w, -((-(si + 1) * w) // S))  # first i with floor(i S / w) > si
        inter = np.where(amb, w - kept_i, 0)
        strided, _ = strided_skipped(base, w, S, hp, hi_, hf)
        tot["proteins"] += len(prot)
        tot["windows"] += int(w.sum())
        tot["amb_p"] += int(amb.sum())
        tot["amb_w"] += int(w[amb].sum())
        tot["skip"] += int(skip.sum())
        tot["drop"] += int((w[amb] - skip[amb]).sum())
        tot["inter"] += int(inter.sum())
        tot["strided"] += int(strided.sum())
    W = tot["windows"]
    out = {"workload": args.workload, "block_proteins": P, "sample_every": args.sample,
           "proteins": tot["proteins"], "windows": W,
           "ambiguous_proteins": tot["amb_p"] / tot["proteins"],
           "ambiguous_windows": tot["amb_w"] / W,
           "skipped_windows": tot["skip"] / W,
           "dropped_walk_windows": tot["drop"] / W,
           "walk_share": (tot["skip"] + tot["drop"]) / W,
           "strided_skipped_windows": tot["strided"] / W,
           "interleaved_skipped_windows": tot["inter"] / W,
           "called": tot["called"], "seconds": round(time.time() - t0, 1)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
