"""Host side of the duplicate-protein check above kma_check_sequences: the reference's
`seqCheck` (anno/SequenceCheckProcessor.java:83-135).

    python -m kmeranno.seqcheck DIR [--roles FILE]

Every peg of the genomes DIR/*.gto (sorted by name; .gz allowed) that has a non-empty protein is
keyed by the MD5 of its sequence on the GPU; the groups whose members carry more than one
function are reported:

  - the header "num\\tfid\\tfunction\\tinteresting", then per mixed group one line per member,
    "%8d\\t%s\\t%s\\t%s" with the group's number (1-based, badCount), the feature id, its function
    and "*" when it is interesting, and a blank line after the group (:106, :128-130);
  - function ids are the exact function strings unless `normalize` maps a function to its key
    (FunctionMap.findOrInsert is external; a peg without a function has the id of "");
  - `interesting` comes with the feature: Feature.isInteresting(RoleMap) is external. The
    command restates it as: some role of the function (split at " / ", " @ " and "; ", comment
    after " #" or " !" dropped) is named, case-insensitively, in the last column of --roles
    (parity unpinned); without --roles nothing is interesting, as with the empty RoleMap;
  - the order is canonical: groups by their first member's input index, members in input order
    (Java prints HashMap / HashSet order: compare as sets of groups);
  - the counts are {groups, multiple, mixed}: proteinMap.size(), protCount and badCount (:103,
    :134). The sequence is hashed with KMA_MD5_UPPER by default (taken to be
    MD5Hex.sequenceMD5's normalisation: DESIGN.md §7).
"""
from __future__ import annotations

import argparse
import glob
import gzip
import json
import os
import re
import sys

import numpy as np

from . import MD5_UPPER, check_sequences, pack_strings

HEADER = "num\tfid\tfunction\tinteresting"


def check_features(features, normalize=None, flags: int = MD5_UPPER, device: int = 0):
    """features: [(fid, protein or '', function, interesting)] in input order. Returns (report
    lines without the header, HEADER, counts {groups, multiple, mixed})."""
    features = list(features)
    fun_ids, fun = {}, np.zeros(len(features), np.uint32)
    for i, (_, _, func, _) in enumerate(features):
        key = normalize(func) if normalize else func
        fun[i] = fun_ids.setdefault(key, len(fun_ids))
    res, off = pack_strings([p or "" for _, p, _, _ in features])
    rep, _, mixed, stats = check_sequences(res, off, fun, flags, device)
    members = {}
    for i in np.flatnonzero(mixed):  # ascending: groups by first member, members in order
        members.setdefault(int(rep[i]), []).append(int(i))
    lines = []
    for num, group in enumerate(members.values(), 1):
        for i in group:
            fid, _, func, interesting = features[i]
            lines.append("%8d\t%s\t%s\t%s" % (num, fid, func, "*" if interesting else ""))
        lines.append("")
    counts = {"groups": int(stats[0]), "multiple": int(stats[1]), "mixed": int(stats[2])}
    return lines, HEADER, counts


def roles_of(function: str):
    """The roles of a function string (Feature.rolesOfFunction, external, restated)."""
    text = re.split(r"\s+[#!]", function or "", maxsplit=1)[0]
    return [r.strip() for r in re.split(r"\s+/\s+|\s+@\s+|;\s+", text) if r.strip()]


def load_roles(path: str):
    """The role names of a role definition file: the last tab-separated column of each line."""
    with open(path) as f:
        return {line.rstrip("\n").split("\t")[-1].strip().lower() for line in f if line.strip()}


def _load(path: str) -> dict:
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "rt") as f:
        return json.load(f)


def genome_pegs(genome: dict):
    """(fid, protein, function) of a GTO's pegs (Genome.getPegs: the CDS features)."""
    for f in genome.get("features", []):
        if f.get("type") in ("CDS", "peg") or ".peg." in f.get("id", ""):
            yield f.get("id", ""), f.get("protein_translation") or "", f.get("function") or ""


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m kmeranno.seqcheck", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("inDir", metavar="DIR", help="input GTO directory")
    ap.add_argument("--roles", metavar="FILE", help="role definition file of interesting roles")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if not os.path.isdir(a.inDir):
        ap.error(f"Input directory {a.inDir} is not found or invalid.")
    roles = load_roles(a.roles) if a.roles else set()
    paths = sorted(glob.glob(os.path.join(a.inDir, "*.gto")) +
                   glob.glob(os.path.join(a.inDir, "*.gto.gz")), key=os.path.basename)
    features = []
    for p in paths:
        for fid, prot, func in genome_pegs(_load(p)):
            features.append((fid, prot, func,
                             any(r.lower() in roles for r in roles_of(func)) if roles else False))
    lines, header, counts = check_features(features, device=a.device)
    sys.stdout.write("\n".join([header] + lines) + "\n")
    print("%d inconsistent proteins found.  %d proteins occurred multiple times.  %d distinct "
          "proteins in %d genomes." % (counts["mixed"], counts["multiple"], counts["groups"],
                                       len(paths)), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
