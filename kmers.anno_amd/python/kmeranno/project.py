"""The projector as a command (the reference's `kmers`, KmerProcessor.annotateGenome):

    python -m kmeranno.project -i new.gto --close DIR -o out.gto

projects the pegs of the close genomes DIR/*.gto (sorted by name; the first -n of them) onto
new.gto's contigs with kmeranno.projector.project_genome, appends the features to the genome's
`features` and writes it as JSON. The options and their defaults are KmerProcessor's (:62-94,
:144-150). Fetching close genomes from PATRIC (--cache) is not part of this command: they are
read from DIR. GTOs may be gzipped (.gz).
"""
from __future__ import annotations

import argparse
import glob
import gzip
import json
import os
import sys


def _load(path: str) -> dict:
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "rt") as f:
        return json.load(f)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m kmeranno.project", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-i", "--input", required=True, help="the new genome (GTO)")
    ap.add_argument("--close", required=True, metavar="DIR", help="directory of close genomes")
    ap.add_argument("-o", "--output", required=True, help="the annotated genome (GTO)")
    ap.add_argument("-m", "--minStrength", "--min", type=float, default=0.5)
    ap.add_argument("-f", "--fuzz", "--maxLength", "--max", type=float, default=1.5)
    ap.add_argument("--minLength", "--minFuzz", type=float, default=0.8)
    ap.add_argument("-e", "--minEvidence", type=int, default=10)
    ap.add_argument("-K", "--kmer", type=int, default=8)
    ap.add_argument("-n", "--nGenomes", "--num", type=int, default=10)
    ap.add_argument("--algorithm", choices=("AGGRESSIVE", "STRICT"), default="AGGRESSIVE")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    # KmerProcessor.validateParms :117-122
    if a.minStrength >= 1.0:
        ap.error("Minimum strength must be less than 1.")
    if a.fuzz <= 1.0:
        ap.error("Max length factor must be greater than 1.")
    if a.minLength > 1.0:
        ap.error("Min length factor must be less than or equal to 1.")
    if not os.path.isdir(a.close):
        ap.error(f"{a.close} is not a directory.")
    from kmeranno import projector
    genome = _load(a.input)
    paths = sorted(glob.glob(os.path.join(a.close, "*.gto")), key=os.path.basename)
    close = [_load(p) for p in paths[:max(a.nGenomes, 0)]]
    feats, counters = projector.project_genome(
        genome, close, k=a.kmer, strict=a.algorithm == "STRICT", min_strength=a.minStrength,
        max_fuzz=a.fuzz, min_fuzz=a.minLength, min_evidence=a.minEvidence,
        max_genomes=a.nGenomes, device=a.device)
    print("%d proposals made, %d merged, %d rejected, %d too weak, %d too little evidence, "
          "%d kept." % tuple(counters[c] for c in ("made", "merged", "rejected", "weak", "small",
                                                   "kept")), file=sys.stderr)
    genome.setdefault("features", []).extend(feats)
    with open(a.output, "w") as f:
        json.dump(genome, f)
    return 0


if __name__ == "__main__":
    sys.exit(main())
