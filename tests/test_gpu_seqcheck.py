"""Duplicate-protein grouping on the GPU (kma_check_sequences; kmeranno.seqcheck, the reference's
seqCheck, anno/SequenceCheckProcessor.java:92-133) against a dict-of-lists grouping over
hashlib.md5 written here: rep, size, mixed and the three counts; then the report of
check_features and of the command on small.gto's pegs beside a copy with altered functions."""
import gzip
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu
UPPER = 1
AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)


@pytest.fixture(scope="module")
def kma(native_lib):
    import kmeranno
    assert kmeranno.device_count() >= 1
    return kmeranno


def fold(b: bytes) -> bytes:
    return bytes(c - 32 if 97 <= c <= 122 else c for c in b)


def grouping(seqs, fun, flags):
    """SequenceCheckProcessor's map restated: md5 -> members (empty sequences join none)."""
    groups = {}
    for i, s in enumerate(seqs):
        if s:
            groups.setdefault(hashlib.md5(fold(s) if flags & UPPER else s).digest(), []).append(i)
    n = len(seqs)
    rep, size, mixed = np.full(n, -1, np.int32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    stats = [len(groups), 0, 0]
    for members in groups.values():
        bad = fun is not None and len(members) > 1 and len({fun[i] for i in members}) > 1
        stats[1] += len(members) > 1
        stats[2] += bad
        for i in members:
            rep[i], size[i], mixed[i] = members[0], len(members), bad
    return rep, size, mixed, stats


def check(kma, seqs, fun=None, flags=0):
    res, off = kma.pack_strings(seqs)
    rep, size, mixed, stats, dig = kma.check_sequences(res, off, fun, flags, digests=True)
    erep, esize, emixed, estats = grouping(seqs, fun, flags)
    assert (rep == erep).all() and (size == esize).all() and (mixed == emixed).all()
    assert stats.tolist() == estats
    for i, s in enumerate(seqs):
        assert bytes(dig[i]) == hashlib.md5(fold(s) if flags & UPPER else s).digest()
    return rep, size, mixed, stats


def rand_seqs(rng, n, lo=1, hi=300):
    return [AA[rng.integers(0, 20, rng.integers(lo, hi))].tobytes() for _ in range(n)]


def test_all_distinct(kma):
    rng = np.random.default_rng(1)
    seqs = [s + b"%d" % i for i, s in enumerate(rand_seqs(rng, 700))]
    rep, size, mixed, stats = check(kma, seqs, rng.integers(0, 5, 700))
    assert (rep == np.arange(700)).all() and (size == 1).all() and not mixed.any()
    assert stats.tolist() == [700, 0, 0]


@pytest.mark.parametrize("n", [1, 2, 64, 1500])
def test_all_identical(kma, n):
    seqs = [b"MKVLAAGIVALLLAAGCSSA"] * n
    rep, size, mixed, stats = check(kma, seqs, np.full(n, 7))
    assert (rep == 0).all() and (size == n).all() and not mixed.any()
    fun = np.full(n, 7)
    fun[-1] = 8
    rep, size, mixed, stats = check(kma, seqs, fun)
    assert stats.tolist() == [1, int(n > 1), int(n > 1)] and mixed.all() == (n > 1)


def test_duplicates_adjacent_and_far_apart(kma):
    rng = np.random.default_rng(2)
    seqs = rand_seqs(rng, 2400)
    seqs[11] = seqs[10]                    # adjacent
    seqs[1500] = seqs[500]                 # 1,000 apart
    seqs[2399] = seqs[2000] = seqs[0]      # three members, first and last of the batch
    fun = rng.integers(0, 3, len(seqs))
    fun[10], fun[11] = 4, 4                # one function
    fun[500], fun[1500] = 5, 6             # two
    rep, size, mixed, stats = check(kma, seqs, fun)
    assert rep[11] == 10 and rep[1500] == 500 and rep[2399] == rep[2000] == 0 and size[0] == 3
    assert not mixed[10] and mixed[500] and mixed[1500]
    check(kma, seqs)  # without function ids nothing is mixed


def test_empty_sequences_join_no_group(kma):
    seqs = [b"", b"MKV", b"", b"MKV", b"", b"A"]
    rep, size, mixed, stats = check(kma, seqs, [1, 2, 3, 4, 5, 6])
    assert rep.tolist() == [-1, 1, -1, 1, -1, 5] and size.tolist() == [0, 2, 0, 2, 0, 1]
    assert mixed.tolist() == [0, 1, 0, 1, 0, 0] and stats.tolist() == [2, 1, 1]
    check(kma, [b"", b""], [1, 2])
    check(kma, [b""])


@pytest.mark.parametrize("flags", [0, UPPER])
def test_near_pairs(kma, flags):
    """Pairs that differ only in the last byte, only in length, and only in case."""
    base = b"MSTNPKPQRKTKRNTNRRPQDVKFPGGGQIVGGVYLLPRRGPRLGVRATRKTSERSQPRGRRQPIPKARRPEGRTWAQPGYPWPLYGNE"
    seqs = [base, base[:-1] + b"Q", base, base[:-1], base + b"A", base.lower(),
            base[:40] + base[40:].lower(), base[:64], base[:64], base[:63], base[:65]]
    fun = list(range(len(seqs)))
    rep, size, mixed, stats = check(kma, seqs, fun, flags)
    assert rep[2] == 0 and rep[1] == 1 and rep[3] == 3 and rep[4] == 4 and rep[8] == 7
    assert rep[5] == (0 if flags else 5) and rep[6] == (0 if flags else 6)


def test_function_patterns(kma):
    """(1, 1, 2) is mixed, (5, 5) is not, singletons never are."""
    a, b, c, d = b"AAAAKL", b"CCCCKL", b"DDDDKL", b"EEEEKL"
    seqs = [a, b, a, c, b, a, d]
    fun = [1, 5, 1, 9, 5, 2, 0xFFFFFFFF]
    rep, size, mixed, stats = check(kma, seqs, np.array(fun, np.uint32))
    assert mixed.tolist() == [1, 0, 1, 0, 0, 1, 0] and stats.tolist() == [4, 2, 1]
    assert size.tolist() == [3, 2, 3, 1, 2, 3, 1]


@pytest.fixture(scope="module")
def two_genomes(small_gto):
    """small.gto and a copy (another genome id) in which the functions of 10 pegs are altered."""
    copy = json.loads(json.dumps(small_gto))
    copy["id"] = "97478.31"
    pegs = [f for f in copy["features"] if f.get("protein_translation")]
    altered = []
    for j, f in enumerate(pegs):
        f["id"] = f["id"].replace("97478.30", "97478.31")
        if j % 71 == 3:
            f["function"] = (f.get("function") or "") + " (altered)"
            altered.append(j)
    assert len(altered) == 10
    return small_gto, copy, altered


def pegs_of(g):
    return [(f["id"], f["protein_translation"], f.get("function") or "", j % 2 == 0)
            for j, f in enumerate(x for x in g["features"] if x.get("protein_translation"))]


def test_check_features_reports_the_altered_groups(kma, two_genomes):
    from kmeranno import seqcheck
    a, b, altered = two_genomes
    feats = pegs_of(a) + pegs_of(b)
    lines, header, counts = seqcheck.check_features(feats)
    assert header == "num\tfid\tfunction\tinteresting"
    assert counts == {"groups": 712, "multiple": 712, "mixed": 10}
    want = []
    for num, j in enumerate(altered, 1):  # canonical order: by first member, members in order
        for fid, _, func, interesting in (feats[j], feats[712 + j]):
            want.append("%8d\t%s\t%s\t%s" % (num, fid, func, "*" if interesting else ""))
        want.append("")
    assert lines == want
    # a normalize callable makes the function ids: dropping the alteration leaves nothing mixed
    lines, _, counts = seqcheck.check_features(feats, lambda f: f.replace(" (altered)", ""))
    assert lines == [] and counts["mixed"] == 0 and counts["multiple"] == 712
    # lower-case copies are the same proteins under the default flag, other proteins under 0
    low = [(fid, p.lower(), f, i) for fid, p, f, i in pegs_of(b)]
    assert seqcheck.check_features(pegs_of(a) + low)[2]["groups"] == 712
    assert seqcheck.check_features(pegs_of(a) + low, flags=0)[2] == {
        "groups": 1424, "multiple": 0, "mixed": 0}


def test_seqcheck_command(kma, two_genomes, tmp_path):
    from kmeranno import seqcheck
    a, b, altered = two_genomes
    with open(tmp_path / "a.gto", "w") as f:
        json.dump(a, f)
    with gzip.open(tmp_path / "b.gto.gz", "wt") as f:
        json.dump(b, f)
    feats = [(fid, p, fn, False) for fid, p, fn, _ in pegs_of(a) + pegs_of(b)]
    lines, header, _ = seqcheck.check_features(feats)
    env = dict(os.environ, PYTHONPATH=os.path.join(PKG, "python"))
    r = subprocess.run([sys.executable, "-m", "kmeranno.seqcheck", str(tmp_path)],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "\n".join([header] + lines) + "\n" and len(lines) == 30
    assert "10 inconsistent proteins found.  712 proteins occurred multiple times." in r.stderr
    # --roles marks the members whose function names a listed role
    role = seqcheck.roles_of(feats[altered[0]][2])[0]
    (tmp_path / "roles.tbl").write_text(f"RoleA\t{role}\n")
    r = subprocess.run([sys.executable, "-m", "kmeranno.seqcheck", str(tmp_path), "--roles",
                        str(tmp_path / "roles.tbl")],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr
    out = r.stdout.split("\n")
    assert out[1] == lines[0] + "*" and [x.rstrip("*") for x in out[1:-1]] == lines
