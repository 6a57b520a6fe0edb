"""§8(f)2, makeFeature's protein on the GPU: kma_translate_locations (kma_translate.hip) against
the oracle composition — oracle_py.reverse_complement and oracle_py.translate on the location's
substring (the C oracle's orc_translate for the genetic codes oracle_py does not carry), the trim
and the 'M' rule composed here — bit-exact on residues and offsets; then make_features,
project_genome and `python -m kmeranno.project` end to end on the reference's own fixture against
the oracle's literal PegProposalList. The kernel splits the flat output over threads and finds
each thread's location by a search of the offsets, so the cases here are the places that can go
wrong: location borders inside a thread's four residues, a block's range, runs of empty
locations, contig borders, both strands, and the tail of the stream."""
import ctypes as C
import json
import os
import subprocess
import sys
from decimal import ROUND_HALF_UP, Decimal

import numpy as np
import pytest

from conftest import PKG
from oracle import oracle_py
from oracle.proposal_list import Loc, ProposalList

pytestmark = pytest.mark.gpu
K = 8
STARTS = ("ATG", "GTG", "TTG")
ALL_CODES = (1, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13, 14, 16, 21, 22, 23, 24, 25)


@pytest.fixture(scope="module")
def kma(native_lib):
    import kmeranno
    assert kmeranno.device_count() >= 1
    return kmeranno


def text(contig) -> str:
    return contig.decode("latin-1") if isinstance(contig, bytes) else contig


def raw_and_peg(contig: str, strand, left, right, gcode, translate=oracle_py.translate):
    """The expected proteins of one location, raw and peg mode: the substring (reverse
    complemented on '-') through the oracle's translate; peg mode drops the last whole codon and
    turns a first ATG / GTG / TTG into M."""
    sub = contig[left - 1:right]
    if strand == "-":
        sub = oracle_py.reverse_complement(sub)
    raw = translate(sub, 1, gcode)
    assert len(raw) == len(sub) // 3
    peg = raw[:max(len(raw) - 1, 0)]
    if peg and sub[:3].upper().replace("U", "T") in STARTS:
        peg = "M" + peg[1:]
    return raw, peg


def expect(contigs, rows, gcode, translate=oracle_py.translate):
    """([raw proteins], [peg proteins]) of rows (contig, strand, left, right)."""
    strs = [text(c) for c in contigs]
    both = [raw_and_peg(strs[c], s, lft, rgt, gcode, translate) for c, s, lft, rgt in rows]
    return [b[0] for b in both], [b[1] for b in both]


def gpu(kma, contigs, rows, gcode=11, peg=False):
    """translate_locations' answer as (list of proteins, offsets)."""
    dna, off = kma.pack_strings(contigs)
    res, ooff = kma.translate_locations(dna, off, kma.make_locations(rows), gcode, peg)
    assert len(res) == int(ooff[-1]) + 32 and not res[int(ooff[-1]):].any()
    raw = res.tobytes()
    return [raw[int(a):int(b)].decode("latin-1") for a, b in zip(ooff[:-1], ooff[1:])], ooff


def check(kma, contigs, rows, want, gcode=11, peg=False):
    got, ooff = gpu(kma, contigs, rows, gcode, peg)
    assert ooff.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    bad = [(r, g, w) for r, g, w in zip(rows, got, want) if g != w]
    assert not bad, (len(bad), bad[:3])


def random_contig(rng, n, ambiguous=0.01, lower=0.2, odd=0.0):
    b = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy()
    b[rng.random(n) < ambiguous] = ord("N")
    if odd:
        m = rng.random(n) < odd
        b[m] = np.frombuffer(b"Uu\xff\x80-", np.uint8)[rng.integers(0, 5, int(m.sum()))]
    b[(rng.random(n) < lower) & (b < 128)] |= 0x20
    return b.tobytes()


# ---- 1. exhaustive small genome -----------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    """6 contigs (0, 2, 3, 5, 700, 3001 bases; ~1% N, ~1% U / bytes >= 128 / '-', ~20% lower
    case) and every span of 0..9, 24 and 25 bases at every left on both strands."""
    rng = np.random.default_rng(20)
    contigs = [random_contig(rng, n, odd=0.01) for n in (0, 2, 3, 5, 700, 3001)]
    rows = [(c, s, lft, lft + ln - 1) for c, x in enumerate(contigs)
            for ln in (*range(10), 24, 25) for lft in range(1, len(x) - ln + 2) for s in "+-"]
    return contigs, rows


@pytest.mark.parametrize("gcode", [11, 4, 1])
def test_every_span_of_a_small_genome(kma, small, gcode):
    contigs, rows = small
    raw, peg = expect(contigs, rows, gcode)
    assert len(rows) > 80_000
    check(kma, contigs, rows, raw, gcode, False)
    check(kma, contigs, rows, peg, gcode, True)
    assert any("X" in p for p in raw) and any(p[:1] == "M" != r[:1] for r, p in zip(raw, peg))
    assert any("W" in p for p in raw) and any("*" in p for p in raw)


# ---- 2. code tables -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def codon_contig():
    """3,000 bases: all 64 codons in each frame's reach (every codon, then every codon shifted by
    one and by two bases), codons with N / U / lower case, random filler."""
    rng = np.random.default_rng(22)
    codons = "".join(a + b + c for a in "TCAG" for b in "TCAG" for c in "TCAG")
    s = codons + "A" + codons + "C" + codons + "ANGNNNTNAUGAugauuGGuN" + codons.lower()
    s += random_contig(rng, 3000 - len(s)).decode()
    assert len(s) == 3000
    return s


@pytest.mark.parametrize("gcode", ALL_CODES)
def test_every_genetic_code(kma, oracle_c, codon_contig, gcode):
    """oracle_py carries codes 1, 4, 11 and 25; the others are checked against the C oracle's
    orc_translate, and those four against both."""
    rows = [(0, s, 1 + f, 3000 - g) for s in "+-" for f in range(3) for g in range(3)]
    rows += [(0, s, lft, lft + 8) for s in "+-" for lft in range(1, 700)]
    oracles = [oracle_c.translate] + ([oracle_py.translate] if gcode in (1, 4, 11, 25) else [])
    for tr in oracles:
        raw, peg = expect([codon_contig], rows, gcode, tr)
        check(kma, [codon_contig], rows, raw, gcode, False)
        check(kma, [codon_contig], rows, peg, gcode, True)
    assert len(set(raw[0])) >= 20


def test_unknown_genetic_code_is_invalid(kma, codon_contig):
    for bad in (0, 7, 8, 15, 17, 20, 26, -1, 111):
        with pytest.raises(kma.KmerAnnoError) as e:
            gpu(kma, [codon_contig], [(0, "+", 1, 30)], bad)
        assert e.value.code == kma.E_INVALID and "genetic code" in str(e.value)


# ---- 3. decomposition ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch():
    """One contig of 61,000 bases and one batch: a 20,000-codon location on each strand,
    locations of 2^i - 1, 2^i and 2^i + 1 codons for i = 0..12, 5,000 one-codon locations in a
    row, runs of 1, 63, 64 and 1,500 empty locations (0, 1 or 2 bases) between non-empty ones,
    an empty location first and last; with the oracle's answer in both modes."""
    rng = np.random.default_rng(23)
    contig = random_contig(rng, 61_000, ambiguous=0.002)
    n = len(contig)

    def at(codons, extra=0, strand=None):
        ln = 3 * codons + extra
        left = int(rng.integers(1, n - ln + 2))
        return (0, strand or "+-"[int(rng.integers(0, 2))], left, left + ln - 1)

    def empties(k):
        return [at(0, int(rng.integers(0, 3))) for _ in range(k)]
    rows = empties(1)
    rows += [(0, "+", 5, 4 + 60_000), (0, "-", 17, 16 + 60_000)]
    for i in range(13):
        for codons in (2 ** i - 1, 2 ** i, 2 ** i + 1):
            rows.append(at(codons, int(rng.integers(0, 3))))
    rows += [(0, "+-"[j & 1], 100 + j, 102 + j) for j in range(5000)]
    for run in (1, 63, 64, 1500):
        rows += empties(run) + [at(int(rng.integers(1, 40)))]
    rows += empties(1)
    raw, peg = expect([contig], rows, 11)
    assert sum(len(r) for r in raw) > 69_000  # 40,000 + 3 (2^13 - 1) + 5,000 and the fillers
    return contig, rows, raw, peg


@pytest.mark.parametrize("peg", [False, True], ids=["raw", "peg"])
@pytest.mark.parametrize("order", ["given", "shuffled"])
def test_decomposition(kma, batch, order, peg):
    contig, rows, raw, pg = batch
    want = pg if peg else raw
    idx = np.arange(len(rows))
    if order == "shuffled":
        np.random.default_rng(24).shuffle(idx)
    check(kma, [contig], [rows[i] for i in idx], [want[i] for i in idx], 11, peg)


# ---- 4. edges and isolation ------------------------------------------------------------------------------
def test_contig_ends(kma):
    rng = np.random.default_rng(25)
    contigs = [random_contig(rng, n) for n in (31, 30, 1, 64)]
    rows = []
    for c, x in enumerate(contigs):
        n = len(x)
        for s in "+-":
            rows += [(c, s, 1, n), (c, s, 1, min(n, 7)), (c, s, max(1, n - 6), n), (c, s, 1, 0),
                     (c, s, n + 1, n), (c, s, 1, 1), (c, s, n, n)]
    raw, peg = expect(contigs, rows, 11)
    check(kma, contigs, rows, raw, 11, False)
    check(kma, contigs, rows, peg, 11, True)


def test_contigs_are_isolated(kma):
    """Whole-contig locations of neighbours filled with bytes that change the answer if one base
    across a border is read."""
    for contigs in (["ATG" * 10, "N" * 30, "ATG" * 10], ["N" * 30, "ATG" * 10, "N" * 30],
                    ["N" * 31, "ATG" * 10 + "AT", "N" * 29]):
        rows = [(c, s, 1, len(x)) for c, x in enumerate(contigs) for s in "+-"]
        raw, peg = expect(contigs, rows, 11)
        check(kma, contigs, rows, raw, 11, False)
        check(kma, contigs, rows, peg, 11, True)
        got, _ = gpu(kma, contigs, rows)
        for (c, s, _, _), g in zip(rows, got):
            if len(contigs[c]) == 30:  # the answers spelled out: ATG -> M, its complement CAT -> H
                assert g == ("X" if "N" in contigs[c] else "M" if s == "+" else "H") * 10


def test_peg_start_rule(kma, oracle_c):
    firsts = {"atg": "M", "gTg": "M", "TTG": "M", "CTG": "L", "NTG": "X", "ATA": "I", "UUG": "M"}
    contigs = [f + "GCTGTGATGTTGTAA" for f in firsts]
    rows = [(c, "+", 1, len(x)) for c, x in enumerate(contigs)]
    rc = [oracle_py.reverse_complement(x) for x in contigs]
    raw, peg = expect(contigs, rows, 11)
    assert peg == [m + "AVML" for m in firsts.values()]  # the internal GTG / ATG / TTG stay
    assert raw == [r + "AVML*" for r in "MVLLXIL"]
    check(kma, contigs, rows, raw, 11, False)
    check(kma, contigs, rows, peg, 11, True)
    rows = [(c, "-", 1, len(x)) for c, x in enumerate(rc)]
    assert expect(rc, rows, 11)[1] == peg
    check(kma, rc, rows, peg, 11, True)
    # the start set is the same under every genetic code
    rows = [(c, "+", 1, len(x)) for c, x in enumerate(contigs)]
    for gcode in (4, 2, 25):
        want = expect(contigs, rows, gcode,
                      oracle_py.translate if gcode != 2 else oracle_c.translate)[1]
        table = dict(firsts, ATA="M") if gcode == 2 else firsts  # code 2 reads ATA as M itself
        assert [w[0] for w in want] == list(table.values())
        check(kma, contigs, rows, want, gcode, True)


# ---- 5. errors --------------------------------------------------------------------------------------
def test_invalid_arguments(kma):
    lib = kma.load()
    contigs = ["ATGGCTTAAC", "ATGGCTGCTTAA"]  # 10 and 12 bases
    dna, off = kma.pack_strings(contigs)
    ok = (1, "+", 1, 12)

    def call(rows, flags=0, gcode=11, dna_p=dna.ctypes.data, off_a=off, cap=64, out=True,
             ooff=True, locs=True, n_contig=2):
        la = kma.make_locations(rows)
        res, oo = np.zeros(cap + 32, np.uint8), np.full(len(la) + 1, 99, np.uint64)
        rc = lib.kma_translate_locations(
            dna_p, off_a.ctypes.data if off_a is not None else None, n_contig, gcode, 0,
            la.ctypes.data if locs else None, len(la), flags, res.ctypes.data if out else None,
            cap, oo.ctypes.data if ooff else None)
        return rc, oo, lib.kma_last_error().decode()

    assert call([ok, ok])[0] == kma.OK
    bad = {"contig 2 >= 2": (2, "+", 1, 3), "strand": (0, "x", 1, 3), "left 0 < 1": (0, "+", 0, 3),
           "right 11 past": (0, "-", 1, 11), "right 3 < left 5 - 1": (1, "+", 5, 3)}
    for word, row in bad.items():
        for where in (0, 2):
            rows = [ok, ok, ok]
            rows[where] = row
            rc, _, msg = call(rows)
            assert rc == kma.E_INVALID and f"location {where}:" in msg and word in msg, msg
    rc, oo, _ = call([(1, "+", 5, 4), (0, "-", 11, 10), ok])  # right == left - 1: legal, empty
    assert rc == kma.OK and oo.tolist() == [0, 0, 0, 4]
    assert call([ok], off_a=np.array([0, 10, 9], np.uint64))[0] == kma.E_INVALID
    assert "decrease" in lib.kma_last_error().decode()
    rc, _, msg = call([(0, "+", 1, 3)], off_a=np.array([0, 1 << 31], np.uint64), n_contig=1)
    assert rc == kma.E_INVALID and "2^31" in msg
    for flags in (2, 3, 0x100, -2):
        rc, _, msg = call([ok], flags=flags)
        assert rc == kma.E_INVALID and "flag" in msg
    assert call([ok], off_a=None)[0] == kma.E_INVALID
    assert call([ok], ooff=False)[0] == kma.E_INVALID
    assert call([ok], locs=False)[0] == kma.E_INVALID
    assert call([ok], dna_p=None)[0] == kma.E_INVALID
    assert call([ok], out=False)[0] == kma.E_INVALID
    assert call([ok], gcode=7)[0] == kma.E_INVALID
    with pytest.raises(kma.KmerAnnoError) as e:
        kma.translate_locations(dna, off, kma.make_locations([ok, (0, "+", 1, 11)]))
    assert e.value.code == kma.E_INVALID and "location 1:" in str(e.value)


def test_capacity_and_empty_batches(kma):
    lib = kma.load()
    dna, off = kma.pack_strings(["ATGGCTTAAC", "ATGGCTGCTTAA"])
    rows = [(1, "+", 1, 12), (0, "-", 1, 10), (0, "+", 2, 1)]
    la = kma.make_locations(rows)
    oo = np.full(4, 99, np.uint64)
    res = np.full(16, 0xEE, np.uint8)
    args = (dna.ctypes.data, off.ctypes.data, 2, 11, 0, la.ctypes.data, 3)
    assert lib.kma_translate_locations(*args, 0, res.ctypes.data, 6, oo.ctypes.data) \
        == kma.E_CAPACITY
    assert oo.tolist() == [0, 4, 7, 7] and (res == 0xEE).all()  # the need is readable
    assert lib.kma_translate_locations(*args, 0, None, 0, oo.ctypes.data) == kma.E_CAPACITY
    assert lib.kma_translate_locations(*args, kma.TR_PEG, res.ctypes.data, 5, oo.ctypes.data) \
        == kma.OK
    assert oo.tolist() == [0, 3, 5, 5] and res[:5].tobytes() == b"MAAVK" and (res[5:] == 0xEE).all()
    assert lib.kma_translate_locations(*args, 0, res.ctypes.data, 7, oo.ctypes.data) == kma.OK
    assert res[:7].tobytes() == b"MAA*VKP" and (res[7:] == 0xEE).all()
    # no location, and no residue at all: OK, offsets filled, nothing written
    res[:] = 0xEE
    one = np.full(1, 99, np.uint64)
    assert lib.kma_translate_locations(dna.ctypes.data, off.ctypes.data, 2, 11, 0, None, 0, 0,
                                       None, 0, one.ctypes.data) == kma.OK
    assert one.tolist() == [0]
    e = kma.make_locations([(0, "+", 1, 2), (1, "-", 13, 12)])
    two = np.full(3, 99, np.uint64)
    assert lib.kma_translate_locations(dna.ctypes.data, off.ctypes.data, 2, 11, 0, e.ctypes.data,
                                       2, 0, None, 0, two.ctypes.data) == kma.OK
    assert two.tolist() == [0, 0, 0]
    r, o = kma.translate_locations(dna, off, np.zeros(0, kma.LOCATION_DTYPE))
    assert len(r) == 32 and o.tolist() == [0]
    r, o = kma.translate_locations(dna, off, kma.make_locations([(0, "+", 1, 5)]), peg=True)
    assert len(r) == 32 and o.tolist() == [0, 0]


# ---- 6. the output feeds the signature vote ---------------------------------------------------------
def peg_rows(gto):
    ids = [c["id"] for c in gto["contigs"]]
    rows, pegs = [], []
    for f in gto["features"]:
        if f.get("protein_translation") and len(f["location"]) == 1:
            cid, begin, strand, length = f["location"][0]
            begin, length = int(begin), int(length)
            rows.append((ids.index(cid), strand, begin, begin + length - 1) if strand == "+"
                        else (ids.index(cid), strand, begin - length + 1, begin))
            pegs.append(f)
    return rows, pegs


def test_output_feeds_annotate_proteins(kma, small_gto):
    """small.gto's 712 peg proteins straight from translate_locations(peg=True) into
    annotate_proteins, against the same proteins packed by pack_strings."""
    rows, pegs = peg_rows(small_gto)
    contigs = [c["dna"] for c in small_gto["contigs"]]
    dna, off = kma.pack_strings(contigs)
    res, ooff = kma.translate_locations(dna, off, kma.make_locations(rows), 11, peg=True)
    prots = [res[int(a):int(b)].tobytes().decode() for a, b in zip(ooff[:-1], ooff[1:])]
    assert len(prots) == 712
    assert sum(p == f["protein_translation"] for p, f in zip(prots, pegs)) == 711
    rng = np.random.default_rng(26)
    kmers = sorted({p[i:i + K] for p in prots for i in range(0, len(p) - K + 1, 7)
                    if "X" not in p[i:i + K]})
    kmers = [kmers[i] for i in rng.choice(len(kmers), 2000, replace=False)]
    fids = rng.integers(0, 50, len(kmers)).astype(np.uint32)
    with kma.SignatureTable.from_rows(kmers, fids, K) as t:
        got = kma.annotate_proteins(t, res, ooff, min_hits=2)
        want = kma.annotate_proteins(t, *kma.pack_strings(prots), min_hits=2)
    for g, w in zip(got[:3], want[:3]):
        assert np.array_equal(g, w)
    # the table is hit and the vote has more than one outcome: not a comparison of empty answers
    assert (got[1] > 0).any() and len(set(got[2].tolist())) > 1


# ---- 7. end to end on the reference's fixture -------------------------------------------------------------
def close_genome(small_gto, seed, gid):
    """small.gto's pegs mutated 5% as a close genome (the recipe of tests/test_gpu_orf.py)."""
    rng = np.random.default_rng(seed)
    aa = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
    feats = []
    for f in small_gto["features"]:
        if not f.get("protein_translation"):
            continue
        b = np.frombuffer(f["protein_translation"].encode(), np.uint8).copy()
        m = rng.random(len(b)) < 0.05
        b[m] = aa[rng.integers(0, 20, int(m.sum()))]
        feats.append({"id": f["id"].replace("97478.30", gid), "type": "CDS",
                      "function": f.get("function", ""),
                      "protein_translation": b.tobytes().decode()})
    return {"id": gid, "genetic_code": 11, "contigs": [], "features": feats}


def java_4f(x):
    return str(Decimal(repr(x)).quantize(Decimal("0.0001"), rounding=ROUND_HALF_UP))


STAMP = 1549493540.5


@pytest.fixture(scope="module")
def projected(kma, small_gto):
    from kmeranno import projector
    close = close_genome(small_gto, 9, "1000.1")
    feats, counters = projector.project_genome(small_gto, [close], timestamp=STAMP)
    return close, feats, counters


def test_project_genome_matches_the_oracle_chain(kma, projected, small_gto):
    close, feats, counters = projected
    contigs = [c["dna"] for c in small_gto["contigs"]]
    ids = [c["id"] for c in small_gto["contigs"]]
    dna, doff = kma.pack_strings(contigs)
    prots = [f["protein_translation"] for f in close["features"]]
    funcs = [f["function"] for f in close["features"]]
    t, _ = kma.SignatureTable.from_pegs(*kma.pack_strings(prots), K)
    with t:
        hits = kma.connect_pegs(t, dna, doff, 11, False)
    props, _ = kma.propose_pegs(hits, np.array([len(p) for p in prots], np.uint32), K)
    olist = ProposalList(dict(zip(ids, contigs)), 0.5 / 3, 10)
    for p in props:
        olist.propose(Loc(ids[int(p["contig"])], chr(p["strand"]), int(p["left"]),
                          int(p["right"])), funcs[int(p["peg"])], int(p["evidence"]))
    want = []
    for i, q in enumerate(olist, start=1):
        loc = q.loc
        _, prot = raw_and_peg(contigs[ids.index(loc.contig_id)], loc.dir, loc.left, loc.right, 11)
        note = "Annotated with evidence %d and strength %s" % (q.evidence, java_4f(q.strength()))
        want.append({"id": f"fig|{small_gto['id']}.peg.{i}", "type": "CDS",
                     "function": q.function,
                     "location": [[loc.contig_id, str(loc.begin()), loc.dir, loc.length()]],
                     "protein_translation": prot,
                     "annotations": [[note, "kmers.anno", STAMP, ""],
                                     ["Set function to " + q.function, "kmers.anno", STAMP, ""]]})
    assert len(feats) > 400 and len(feats) == len(want)
    bad = [(g, w) for g, w in zip(feats, want) if g != w]
    assert not bad, (len(bad), bad[:2])
    assert counters == {"made": olist.made, "merged": olist.merged, "rejected": olist.rejected,
                        "weak": olist.weak, "small": olist.small, "kept": len(want)}
    assert counters["made"] == len(props) and counters["kept"] == len(feats)
    print("projected features:", len(feats), counters)
    # a projected peg that lands on a peg of small.gto carries the translation stored there
    stored = {json.dumps(f["location"]): f["protein_translation"] for f in peg_rows(small_gto)[1]}
    same = [f for f in feats if json.dumps(f["location"]) in stored]
    print("features on a stored peg's location:", len(same))
    assert len(same) >= 1
    assert all(f["protein_translation"] == stored[json.dumps(f["location"])] for f in same)
    assert all(f["protein_translation"] and "*" not in f["protein_translation"] for f in feats)


def test_project_command_in_a_child_process(kma, projected, small_gto, tmp_path):
    close, feats, _ = projected
    (tmp_path / "close").mkdir()
    with open(tmp_path / "new.gto", "w") as f:
        json.dump(small_gto, f)
    with open(tmp_path / "close" / "1000.1.gto", "w") as f:
        json.dump(close, f)
    (tmp_path / "close" / "notes.txt").write_text("not a genome")
    env = dict(os.environ, PYTHONPATH=os.path.join(PKG, "python"))
    r = subprocess.run([sys.executable, "-m", "kmeranno.project", "-i", str(tmp_path / "new.gto"),
                        "--close", str(tmp_path / "close"), "-o", str(tmp_path / "out.gto")],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert f"{len(feats)} kept" in r.stderr
    with open(tmp_path / "out.gto") as f:
        out = json.load(f)
    n_old = len(small_gto["features"])
    assert out["features"][:n_old] == small_gto["features"]
    assert {k: v for k, v in out.items() if k != "features"} == \
        {k: v for k, v in small_gto.items() if k != "features"}

    def unstamped(fs):
        return [dict(f, annotations=[[a[0], a[1], a[3]] for a in f["annotations"]]) for f in fs]
    assert unstamped(out["features"][n_old:]) == unstamped(feats)
    assert all(isinstance(a[2], float) for f in out["features"][n_old:]
               for a in f["annotations"])


def test_max_genomes_limits_the_close_genomes(kma, projected, small_gto):
    from kmeranno import projector
    close, feats, counters = projected
    second = close_genome(small_gto, 10, "1000.2")
    one = projector.project_genome(small_gto, [close, second], max_genomes=1, timestamp=STAMP)
    assert one == (feats, counters)
    two, c2 = projector.project_genome(small_gto, [close, second], max_genomes=2, timestamp=STAMP)
    assert c2["made"] > counters["made"] and c2["merged"] >= counters["merged"]
    assert [f["id"] for f in two] == [f"fig|{small_gto['id']}.peg.{i + 1}" for i in range(len(two))]
