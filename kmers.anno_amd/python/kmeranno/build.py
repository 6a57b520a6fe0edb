"""The reference's `build` command (anno/BuildKmerProcessor.java:137-223) above the streamed
signature build (kmeranno.SigBuilder, kma_sig_builder):

    python -m kmeranno.build roleFile goodRoleFile gtoDir [-g genomeFile] [-K 8]
                             [--batch-residues N] [--device D]

Every peg of the genomes gtoDir/*.gto and *.gto.gz (file-name order; with -g only the genomes whose
id the file names) is resolved to "interesting with one good role", "buffered" or "skipped"
(resolve_roles, :157-165), the pegs are appended to a batch until it holds --batch-residues
residues, and every batch is one SigBuilder.add. The discriminating kmers are written to stdout as
`kmer\\troleId` lines in key order (the reference prints its HashMap's order: compare as sets), so
the file is what `apply` and kma_table_create_from_tsv read.

--batch-residues defaults to 2^26 (67,108,864): an add holds about 33 bytes of device scratch per
residue plus the staged batch, so the default keeps the per-add scratch near 2.3 GB, and one add
stays below the 2^31 residues an add may hold whatever the value given. -K is the window size
actually used (1..12); the reference's -K sets KmerReference's K, which ProteinKmers never reads
(DESIGN.md §7).

stderr carries the reference's log counts: per genome "N interesting pegs found, N buffered."
(:177; its third figure, the hits that agreed with a kmer's first role, depends on the order of the
pegs and is not produced), then "N discriminating kmers remaining." (:209) and, per good role
without a kmer, "No kmers found for ID: NAME." (:217-221).

External to the reference's repository and restated here (parity unpinned):

  - RoleMap.load(roleFile): one role per line, tab-separated, the first column the role id, the
    last column the role name. A name is matched case-insensitively after collapsing runs of
    whitespace (the rule seqcheck.load_roles uses); a name that occurs again keeps its first id.
  - LineReader.readSet(goodRoleFile): the set of the file's lines (trailing white space dropped,
    empty lines skipped); each is a role id.
  - TabbedLineReader.readSet(genomeFile, "1"): a header line, then the first column of every line.
  - Feature.getUsefulRoles(roleMap): the roles of the function (seqcheck.roles_of:
    Feature.rolesOfFunction restated) that the role map knows.
  - GenomeDirectory: the *.gto files of the directory in name order (gzipped ones as well here).
"""
from __future__ import annotations

import argparse
import glob
import os
import sys

import numpy as np

from . import SigBuilder
from .seqcheck import _load, genome_pegs, roles_of

DEFAULT_BATCH_RESIDUES = 1 << 26
MAX_ADD_RESIDUES = (1 << 31) - 1  # an add holds fewer than 2^31 residues


_SYMBOLS = "?ABCDEFGHIJKLMNOPQRSTUVWXYZ*????"  # the standard 5-bit codes (std_codes)


def kmer_of(key: int, k: int) -> str:
    """The kmer of a packed key: 5 bits per residue, the first residue highest."""
    return "".join(_SYMBOLS[(key >> (5 * (k - 1 - j))) & 31] for j in range(k))


def role_key(name: str) -> str:
    """The form in which role names are compared: white space collapsed, lower case."""
    return " ".join(name.split()).lower()


def load_role_map(path: str):
    """RoleMap.load restated: ({role_key(name): id}, {id: name})."""
    by_name, names = {}, {}
    with open(path) as f:
        for line in f:
            cols = line.rstrip("\r\n").split("\t")
            if not cols[0].strip() or not cols[-1].strip():
                continue
            by_name.setdefault(role_key(cols[-1]), cols[0].strip())
            names.setdefault(cols[0].strip(), cols[-1].strip())
    return by_name, names


def read_set(path: str):
    """LineReader.readSet restated: the file's non-empty lines, in order, each once."""
    seen = {}
    with open(path) as f:
        for line in f:
            if line.strip():
                seen.setdefault(line.strip(), len(seen))
    return list(seen)


def read_genome_ids(path: str):
    """TabbedLineReader.readSet(file, "1") restated: the header line is skipped; column 1."""
    with open(path) as f:
        lines = f.read().splitlines()[1:]
    return {ln.split("\t")[0].strip() for ln in lines if ln.strip()}


def resolve_roles(function: str, role_map, good) -> int:
    """BuildKmerProcessor.java:158-165: the roles of `function` that role_map ({role_key(name):
    id}) knows and whose id is in good ({id: dense index}). None kept: -1 (the protein is
    buffered); exactly one: its dense index; more: -2 (the peg is skipped)."""
    ids = [role_map[k] for k in map(role_key, roles_of(function)) if k in role_map]
    kept = [good[i] for i in ids if i in good]
    if not kept:
        return -1
    return kept[0] if len(kept) == 1 else -2


def genome_paths(gto_dir: str):
    return sorted(glob.glob(os.path.join(gto_dir, "*.gto")) +
                  glob.glob(os.path.join(gto_dir, "*.gto.gz")), key=os.path.basename)


class _Batch:
    def __init__(self):
        self.prots, self.roles, self.residues = [], [], 0

    def flush(self, builder: SigBuilder):
        if not self.prots:
            return
        lens = np.fromiter((len(p) for p in self.prots), np.uint64, len(self.prots))
        off = np.zeros(len(lens) + 1, np.uint64)
        np.cumsum(lens, out=off[1:])
        res = np.frombuffer(b"".join(self.prots) + b"\0" * 32, np.uint8)
        builder.add(res, off, np.asarray(self.roles, np.int32))
        self.__init__()


def build(role_file: str, good_file: str, gto_dir: str, genome_file: str | None = None,
          k: int = 8, batch_residues: int = DEFAULT_BATCH_RESIDUES, device: int = 0,
          out=None, log=None):
    """The command's body: writes the rows to `out` and the counts to `log`; returns the
    builder's final info."""
    out = out or sys.stdout
    log = log or sys.stderr
    role_map, names = load_role_map(role_file)
    good_ids = read_set(good_file)
    good = {rid: i for i, rid in enumerate(good_ids)}
    genomes = read_genome_ids(genome_file) if genome_file else None
    batch_residues = max(1, min(int(batch_residues), MAX_ADD_RESIDUES))
    with SigBuilder(k, 0, device) as builder:
        batch = _Batch()
        for path in genome_paths(gto_dir):
            genome = _load(path)
            if genomes is not None and str(genome.get("id", "")) not in genomes:
                continue
            n_role = n_buffered = 0
            for _, prot, func in genome_pegs(genome):
                r = resolve_roles(func, role_map, good)
                n_role += r >= 0
                n_buffered += r == -1
                p = prot.encode()
                if batch.residues + len(p) > MAX_ADD_RESIDUES:
                    batch.flush(builder)
                batch.prots.append(p)
                batch.roles.append(r)
                batch.residues += len(p)
                if batch.residues >= batch_residues:
                    batch.flush(builder)
            print(f"{os.path.basename(path)}: {n_role} interesting pegs found, {n_buffered} "
                  "buffered.", file=log)
        batch.flush(builder)
        keys, roles = builder.finish()
        info = builder.info()
    out.write("".join(f"{kmer_of(key, k)}\t{good_ids[r]}\n"
                      for key, r in zip(keys.tolist(), roles.tolist())))
    print(f"{len(keys)} discriminating kmers remaining.", file=log)
    have = set(roles.tolist())
    for i, rid in enumerate(good_ids):
        if i not in have:
            print(f"No kmers found for {rid}: {names.get(rid, '')}.", file=log)
    return info


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m kmeranno.build", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("roleFile", help="role definition file (roles.in.subsystems)")
    ap.add_argument("goodRoleFile", help="interesting role ids (roles.to.use)")
    ap.add_argument("gtoDir", help="input genome directory")
    ap.add_argument("-g", "--genomes", metavar="genomeFile.tbl",
                    help="file of acceptable genome ids (header line, ids in column 1)")
    ap.add_argument("-K", "--kmer", type=int, default=8, help="protein kmer length (default 8)")
    ap.add_argument("--batch-residues", type=int, default=DEFAULT_BATCH_RESIDUES,
                    help="residues per add (default 2^26)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if not os.path.isdir(a.gtoDir):
        ap.error(f"Genome directory {a.gtoDir} not found or invalid.")
    for f in (a.roleFile, a.goodRoleFile) + ((a.genomes,) if a.genomes else ()):
        if not os.path.isfile(f):
            ap.error(f"{f} not found or unreadable.")
    if len(read_set(a.goodRoleFile)) >= (1 << 24) - 1:
        ap.error("2^24 - 1 good roles or more")
    build(a.roleFile, a.goodRoleFile, a.gtoDir, a.genomes, a.kmer, a.batch_residues, a.device)
    return 0


if __name__ == "__main__":
    sys.exit(main())
