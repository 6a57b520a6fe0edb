"""Host side of the hash annotator (§8(f)3) above kma_hash_annotate and the resident prototype
index (kma_proto_index, kma_hash_annotate_indexed): the per-genome report of
HashAnnotationProcessor.processGenome (HashAnnotationProcessor.java:221-328) and the command
`hashAnno` (:137-213).

    python -m kmeranno.hashanno annoFile inDir [-K 8] [-D Annotations] [--minSim 0.0125]
                                [--minLen 50] [--missing] [--clear]

The role annotation file has headers and is read by its columns `protein` and `annotation`; rows
with a blank annotation or a protein shorter than minLen are dropped (:159-168), and minLen < K
is refused (:150). The prototype index is built once; every genome inDir/*.gto (.gz allowed)
then goes through annotate_genome, and <genomeId>.anno.tbl is written to the output directory
with the header below. changes.tbl there holds the header and this run's new annotations
(:201-204, :320-323). --missing skips genomes whose (\\d+\\.\\d+)\\.anno\\.tbl is already in the
output directory (:184-197); --clear erases the output directory first. Genomes are processed in
file-name order (the reference's parallel stream leaves the order of changes.tbl unspecified:
DESIGN.md §7).

  - proteins are keyed by sequence (Feature.getMD5 is the MD5 of the translation); blank
    proteins and proteins holding '*' are skipped (:237-241) but still get report lines;
  - the prototypes of the role annotation file are those with a non-blank annotation and a
    protein of at least minLen residues (default 50), in file order (:142-153);
  - a genome protein's proposal is the GPU's best prototype (similarity >= minSim, default
    0.0125), else the default proposal: its own annotation with score 0.0 (GenomeProteinKmers
    restated; parity unpinned). When features share a protein, the first one's annotation is
    the default;
  - report lines "fid\\tscore\\tnew_annotation\\told_annotation" (:281-293; a feature without a
    proposal gets a blank score and its old annotation twice); score 0.0 counts as a default,
    an equal annotation as confirmed, anything else as a change (:295-304).
"""
from __future__ import annotations

import argparse
import glob
import gzip
import json
import os
import re
import shutil
import sys

import numpy as np

from . import ProtoIndex, hash_annotate, hash_annotate_indexed

HEADER = "fid\tscore\tnew_annotation\told_annotation"


def prototypes_from_rows(rows, min_len: int = 50):
    """(protein, annotation) rows of the role annotation file -> the kept prototypes."""
    return [(p, a) for p, a in rows if a and a.strip() and len(p) >= min_len]


def _pack(strs):
    b = [s.encode() for s in strs]
    off = np.zeros(len(b) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in b])
    return np.frombuffer(b"".join(b) or b"\0", np.uint8).copy(), off


def build_index(prototypes, k: int = 8, device: int = 0) -> ProtoIndex:
    """The resident index of the kept prototypes [(protein, annotation)] (annotate_genome's
    `index`)."""
    return ProtoIndex(*_pack([p for p, _ in prototypes]), k=k, device=device)


def annotate_genome(features, prototypes, k: int = 8, min_sim: float = 0.0125,
                    device: int = 0, index: ProtoIndex | None = None):
    """features: [(fid, protein or '', function)]; prototypes: [(protein, annotation)]; index:
    build_index(prototypes, k) to score against (its K and device are used), else both sides are
    sent with the call. Returns (report lines without the header, counts {default, confirmed,
    new}, change lines)."""
    by_seq, default = {}, []
    for fid, prot, func in features:
        if prot and "*" not in prot and prot not in by_seq:
            by_seq[prot] = len(default)
            default.append(func)
    seqs = list(by_seq)
    gres, goff = _pack(seqs)
    if index is not None:
        best, sim, _ = hash_annotate_indexed(index, gres, goff, min_sim)
    else:
        pres, poff = _pack([p for p, _ in prototypes])
        best, sim, _ = hash_annotate(gres, goff, pres, poff, k, min_sim, device)
    lines, changes = [], []
    counts = {"default": 0, "confirmed": 0, "new": 0}
    for fid, prot, func in features:
        g = by_seq.get(prot) if prot else None
        if g is None:
            lines.append(f"{fid}\t\t{func}\t{func}")
            continue
        b = int(best[g])
        score = float(sim[g]) if b >= 0 else 0.0
        new = prototypes[b][1] if b >= 0 else default[g]
        line = f"{fid}\t{score!r}\t{new}\t{func}"
        lines.append(line)
        if score == 0.0:
            counts["default"] += 1
        elif new == func:
            counts["confirmed"] += 1
        else:
            counts["new"] += 1
            changes.append(line)
    return lines, counts, changes


ANNO_FILE_PATTERN = re.compile(r"(\d+\.\d+)\.anno\.tbl")


def read_annotation_file(path: str):
    """(protein, annotation) rows of a role annotation file, by its header's columns."""
    with open(path) as f:
        head = f.readline().rstrip("\r\n").split("\t")
        for name in ("annotation", "protein"):
            if name not in head:
                raise ValueError(f'Field "{name}" not found in {path}.')
        a, p = head.index("annotation"), head.index("protein")
        rows = []
        for line in f:
            cols = line.rstrip("\r\n").split("\t")
            if len(cols) > max(a, p):
                rows.append((cols[p], cols[a]))
    return rows


def _load(path: str) -> dict:
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "rt") as f:
        return json.load(f)


def genome_features(genome: dict):
    """[(fid, protein, function)] of every feature of a GTO, in its order (:234-247)."""
    return [(f.get("id", ""), f.get("protein_translation") or "", f.get("function") or "")
            for f in genome.get("features", [])]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m kmeranno.hashanno", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("annoFile", help="input role annotation file")
    ap.add_argument("inDir", help="input GTO directory")
    ap.add_argument("-K", "--kmer", type=int, default=8, help="protein kmer size")
    ap.add_argument("-D", "--outDir", default="Annotations", help="output directory")
    ap.add_argument("--minSim", type=float, default=0.0125)
    ap.add_argument("--minLen", type=int, default=50)
    ap.add_argument("--missing", action="store_true",
                    help="only annotate genomes without an output file")
    ap.add_argument("--clear", action="store_true", help="erase the output directory first")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if a.kmer < 2:
        ap.error("Kmer Size must be at least 2.")
    if not 0.0 <= a.minSim < 1.0:
        ap.error("Minimum similarity score must be between 0 and 1.")
    if not os.path.isdir(a.inDir):
        ap.error(f"Input directory {a.inDir} is not found or invalid.")
    if a.minLen < a.kmer:
        ap.error("Minimum protein length cannot be less than kmer size.")
    if not os.path.isfile(a.annoFile):
        ap.error(f"Role annotation file {a.annoFile} is not found or unreadable.")
    protos = prototypes_from_rows(read_annotation_file(a.annoFile), a.minLen)
    print(f"{len(protos)} annotations found.", file=sys.stderr)
    if a.clear and os.path.isdir(a.outDir):
        shutil.rmtree(a.outDir)
    os.makedirs(a.outDir, exist_ok=True)
    paths = sorted(glob.glob(os.path.join(a.inDir, "*.gto")) +
                   glob.glob(os.path.join(a.inDir, "*.gto.gz")), key=os.path.basename)
    done = set()
    if a.missing:
        for name in os.listdir(a.outDir):
            m = ANNO_FILE_PATTERN.fullmatch(name)
            if m:
                done.add(m.group(1))
    totals = {"default": 0, "confirmed": 0, "new": 0}
    n_genomes = n_features = 0
    with build_index(protos, a.kmer, a.device) as index, \
            open(os.path.join(a.outDir, "changes.tbl"), "w") as change_file:
        change_file.write(HEADER + "\n")
        for path in paths:
            genome = _load(path)
            gid = str(genome.get("id", ""))
            if gid in done:
                continue
            feats = genome_features(genome)
            lines, counts, changes = annotate_genome(feats, protos, a.kmer, a.minSim, a.device,
                                                     index=index)
            with open(os.path.join(a.outDir, gid + ".anno.tbl"), "w") as f:
                f.write("\n".join([HEADER] + lines) + "\n")
            change_file.writelines(line + "\n" for line in changes)
            n_genomes += 1
            n_features += len(feats)
            for key in totals:
                totals[key] += counts[key]
    print(f"{n_features} features processed for {n_genomes} genomes.  {totals['confirmed']} "
          f"annotations confirmed, {totals['new']} updated, {totals['default']} defaulted.",
          file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
