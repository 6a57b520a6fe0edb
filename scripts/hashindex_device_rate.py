#!/usr/bin/env python3
"""Measures the indexed hash annotator on a device-resident genome against the
host entry, on one GPU, at §5.10's shape: c5's 1M prototypes (kmeranno.synth; the build's stored
copy where there is one) and 4,000-protein genomes from synth.make_queries.

Per genome, every output of kma_hash_annotate_indexed_device (best, sim, count, stats[0..2];
stats[3] == 0) is first asserted equal to kma_hash_annotate_indexed's. Then the two forms take
turns inside every round (A B, A B, ...), best of --repeat after a warm-up round:

  (a) kma_hash_annotate_indexed from host buffers, by the host clock around the synchronous call
      (its code is the parent commit's: the yardstick);
  (b) kma_hash_annotate_indexed_device on torch buffers that already hold the genome, by events
      around the call on its stream.

The kernels of (b) are timed separately from a kernel trace: `--trace-calls N` makes N device
calls per genome and nothing else (run it under `rocprofv3 --kernel-trace --output-format csv`),
and `--merge-trace CSV --into JSON` adds each kernel's durations from that trace to a record
written earlier, with the sets kernel's registers, LDS and occupancy from the build's resource
report (kmers.anno_amd/build/kma_hashsets.o.res).

    python scripts/hashindex_device_rate.py --out profiles/hashindex/device_rate.json
"""
import argparse
import csv
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kmers.anno_amd", "python")]
KERNELS = ("hash_reset_kernel", "genome_sets_kernel", "index_score_kernel")


def merge_trace(trace, into, calls):
    """Per kernel of the device call: durations (us) of its last 3 x `calls` dispatches, by
    genome, from a rocprofv3 kernel trace; and the sets kernel's resource report."""
    doc = json.load(open(into))
    runs = {k: [] for k in KERNELS}
    for r in csv.DictReader(open(trace)):
        for k in KERNELS:
            if k in r["Kernel_Name"]:
                runs[k].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    n_g = len(doc["genomes"])
    for k, v in runs.items():
        v.sort()
        assert len(v) >= n_g * calls, (k, len(v))
        v = v[-n_g * calls:]
        for g in range(n_g):
            us = [(e - s) / 1e3 for s, e in v[g * calls:(g + 1) * calls]]
            doc["genomes"][g].setdefault("kernel_us", {})[k] = {
                "best": min(us), "mean": sum(us) / len(us), "calls": len(us)}
    res = os.path.join(ROOT, "kmers.anno_amd", "build", "kma_hashsets.o.res")
    if os.path.exists(res):
        text = open(res).read()
        text = text[text.index("genome_sets_kernel"):]
        grab = lambda pat: int(re.search(pat + r": (\d+)", text).group(1))  # noqa: E731
        lds = grab(r"LDS Size \[bytes/block\]")
        doc["genome_sets_kernel_resources"] = {
            "vgprs": grab("VGPRs"), "scratch_bytes_per_lane": grab(r"ScratchSize \[bytes/lane\]"),
            "lds_bytes_per_block": lds, "occupancy_waves_per_simd": grab(r"Occupancy \[waves/SIMD\]"),
            "blocks_per_cu_by_lds": (160 * 1024) // lds}
    doc["kernel_clock"] = "rocprofv3 --kernel-trace, a run of its own"
    with open(into, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--genomes", type=int, default=3)
    ap.add_argument("--genome-proteins", type=int, default=4000)
    ap.add_argument("--n-proto", type=int, help="a smaller prototype batch (trials)")
    ap.add_argument("--trace-calls", type=int, default=0)
    ap.add_argument("--merge-trace")
    ap.add_argument("--into")
    a = ap.parse_args()
    if a.merge_trace:
        return merge_trace(a.merge_trace, a.into, a.trace_calls or 20)

    import torch  # (torch's HIP runtime first; libkmeranno binds it by SONAME)
    import kmeranno as kma
    from hashindex_rate import inputs

    t0 = time.perf_counter()
    (pr, po), genomes = inputs(a.n_proto, a.genomes, a.genome_proteins)
    load_s = time.perf_counter() - t0
    assert kma.device_count() >= 1, "no HIP device: nothing is measured without one"
    idx = kma.ProtoIndex(pr, po, k=8)
    info = idx.info()
    doc = {"device": torch.cuda.get_device_name(0), "prototypes": int(info.n_proto),
           "index_unique_keys": int(info.n_keys), "index_postings": int(info.n_postings),
           "input_load_s": load_s, "repeat": a.repeat,
           "clocks": {"hash_annotate_indexed": "host, around the synchronous call",
                      "hash_annotate_indexed_device": "events around the call on its stream"},
           "genomes": []}
    stream = torch.cuda.current_stream().cuda_stream
    traced = []
    with idx:
        for gi, (gr, go) in enumerate(genomes):
            n_g, n_r = len(go) - 1, int(go[-1] - go[0])
            res = np.zeros(int(go[-1]) + 32, np.uint8)  # 32 readable bytes past the last residue
            res[:int(go[-1])] = gr[:int(go[-1])]
            d_res = torch.from_numpy(res).cuda()
            d_off = torch.from_numpy(go.view(np.int64)).cuda()
            sbytes = kma.hash_scratch_bytes(n_r, n_g)
            scratch = torch.full((sbytes,), 0xEE, dtype=torch.uint8, device="cuda")
            best = torch.full((n_g,), -7, dtype=torch.int32, device="cuda")
            sim = torch.full((n_g,), -7.0, dtype=torch.float64, device="cuda")
            cnt = torch.full((info.n_proto,), -7, dtype=torch.int32, device="cuda")
            st = torch.full((4,), -7, dtype=torch.int64, device="cuda")

            def device(d_res=d_res, d_off=d_off, n_g=n_g, n_r=n_r, scratch=scratch,
                       sbytes=sbytes, best=best, sim=sim, cnt=cnt, st=st):
                kma.hash_annotate_indexed_device(idx, d_res.data_ptr(), d_off.data_ptr(), n_g, n_r,
                                                 scratch.data_ptr(), sbytes, best.data_ptr(),
                                                 sim.data_ptr(), cnt.data_ptr(), st.data_ptr(),
                                                 0.0125, stream=stream)

            def host(gr=gr, go=go):
                return kma.hash_annotate_indexed(idx, gr, go, 0.0125, stats=True)

            ref = host()
            device()
            torch.cuda.synchronize()
            got = (best.cpu().numpy(), sim.cpu().numpy(), cnt.cpu().numpy().view(np.uint32),
                   st.cpu().numpy().view(np.uint64))
            assert int(got[3][3]) == 0 and got[3][:3].tolist() == ref[3].tolist(), f"genome {gi}"
            for x, y in zip(got[:3], ref[:3]):
                assert x.dtype == y.dtype and (x == y).all(), f"genome {gi}: the entries differ"
            if a.trace_calls:  # (traced below, after every genome's check: the trace's last
                traced.append(device)  # genomes x N dispatches of each kernel are these calls)
                doc["genomes"].append({"proteins": n_g, "traced_calls": a.trace_calls})
                continue
            ms = {"hash_annotate_indexed": [], "hash_annotate_indexed_device": []}
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            for r in range(a.repeat + 1):
                torch.cuda.synchronize()
                t = time.perf_counter()
                host()
                t_host = (time.perf_counter() - t) * 1e3
                torch.cuda.synchronize()
                ev[0].record()
                device()
                ev[1].record()
                torch.cuda.synchronize()
                if r:
                    ms["hash_annotate_indexed"].append(t_host)
                    ms["hash_annotate_indexed_device"].append(ev[0].elapsed_time(ev[1]))
            lens = np.diff(go).astype(np.int64)
            doc["genomes"].append({
                "proteins": n_g, "residues": int(lens.sum()), "median_length": int(np.median(lens)),
                "longest": int(lens.max()), "scratch_bytes": int(sbytes),
                "stats_candidates_split_ranges": [int(x) for x in ref[3]],
                "call_ms": {k: {"best": min(v), "spread": max(v) - min(v), "all": v}
                            for k, v in ms.items()},
                "ratio_host_over_device": min(ms["hash_annotate_indexed"]) /
                min(ms["hash_annotate_indexed_device"])})
        for device in traced:
            for _ in range(a.trace_calls):
                device()
            torch.cuda.synchronize()
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
