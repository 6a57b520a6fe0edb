"""§8(f)2, ORF extension of the projector's peg proposals on the GPU (kma_orf_index_create /
kma_extend_proposals, kma_orf.hip) against oracle/proposal_list.py:extend, the independent
restatement of Location.extend (external to the reference, parity-unpinned), and end to end on
the reference's own fixture against the oracle's literal PegProposalList. The index answers a
proposal from two scans over the genome (next in-frame stop, farthest start since the previous
stop); the cases here are the places a scan can go wrong: contig ends, segment borders between
frames, strands and contigs, carries across every tile of a 20,000-codon ORF, ambiguous bases,
and the three filters with their counters."""
import threading

import numpy as np
import pytest

from oracle.proposal_list import Loc, ProposalList, extend

pytestmark = pytest.mark.gpu
K = 8
KEPT, REJECTED, WEAK, SMALL = 0, 1, 2, 3
_COMP = str.maketrans("ACGTacgt", "TGCAtgca")


def revcomp(s):
    return s.translate(_COMP)[::-1]


@pytest.fixture(scope="module")
def kma(native_lib):
    import kmeranno
    assert kmeranno.device_count() >= 1
    return kmeranno


def make_props(kma, rows):
    """rows of (contig, strand, left, right, evidence) -> PROPOSAL_DTYPE."""
    arr = np.zeros(len(rows), kma.PROPOSAL_DTYPE)
    for i, (c, s, lft, rgt, ev) in enumerate(rows):
        arr[i] = (0, c, lft, rgt, ev, ord(s), 0, 0)
    return arr


def oracle_rows(contigs, rows, gcode=11, min_strength=0.0, min_evidence=0):
    """(status, left, right) per row from the oracle's extend and PegProposalList.propose's
    filter order (PegProposalList.java:71-76)."""
    out = []
    for c, s, lft, rgt, ev in rows:
        real = extend(contigs[c], Loc(str(c), s, lft, rgt), gcode)
        if real is None:
            out.append((REJECTED, 0, 0))
        elif ev / real.length() < min_strength:
            out.append((WEAK, real.left, real.right))
        elif ev < min_evidence:
            out.append((SMALL, real.left, real.right))
        else:
            out.append((KEPT, real.left, real.right))
    return out


def gpu_rows(kma, contigs, rows, gcode=11, min_strength=0.0, min_evidence=0):
    dna, off = kma.pack_strings(contigs)
    with kma.OrfIndex(dna, off, gcode) as idx:
        left, right, status, stats = kma.extend_proposals(idx, make_props(kma, rows),
                                                          min_strength, min_evidence)
    return list(zip(status.tolist(), left.tolist(), right.tolist())), stats.tolist()


def mirror(contigs, c, a, b):
    """The '-' strand twin of strand span [a, b] (0-based) on contig c: every contig reverse
    complemented, the same strand coordinates, as forward 1-based edges."""
    n = len(contigs[c])
    return [revcomp(x) for x in contigs], (c, "-", n - b, n - a)


# ---- 1. exhaustive small genome -----------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    """6 contigs (0, 2, 3, 5, 700, 3001 bases; ~1% N, ~20% lower case), every 24-base span on
    both strands, and the oracle's answer under genetic codes 11, 4 and 1."""
    rng = np.random.default_rng(20)
    contigs = []
    for n in (0, 2, 3, 5, 700, 3001):
        b = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy()
        b[rng.random(n) < 0.01] = ord("N")
        low = rng.random(n) < 0.2
        b[low] |= 0x20
        contigs.append(b.tobytes().decode())
    rows = [(c, s, lft, lft + 23, 1) for c, x in enumerate(contigs)
            for lft in range(1, len(x) - 22) for s in "+-"]
    return contigs, rows, {g: oracle_rows(contigs, rows, g) for g in (11, 4, 1)}


@pytest.mark.parametrize("gcode", [11, 4, 1])
def test_every_span_of_a_small_genome(kma, small, gcode):
    contigs, rows, exp = small
    got, stats = gpu_rows(kma, contigs, rows, gcode)
    assert len(rows) > 7000
    bad = [(r, g, e) for r, g, e in zip(rows, got, exp[gcode]) if g != e]
    assert not bad, (len(bad), bad[:5])
    n_rej = sum(e[0] == REJECTED for e in exp[gcode])
    assert n_rej >= 0.1 * len(rows) and len(rows) - n_rej >= 0.1 * len(rows)  # not a constant
    assert stats == [len(rows), n_rej, 0, 0]
    # code 4 reads through TGA: some proposal ends at a different stop than under code 11
    assert exp[1] == exp[11]
    assert any(a != b for a, b in zip(exp[4], exp[11]))


# ---- 2. hand-built edges --------------------------------------------------------------------------
# (name, contig, strand span [a, b] 0-based, expected (status, start, stop_end) in strand coords)
_A = "ATG" + "GCT" * 4 + "TAA" + "GCT" * 2
EDGES = [
    ("stop_is_own_last_codon", _A, 3, 17, (KEPT, 0, 17)),
    ("stop_is_contig_end", "ATG" + "GCT" * 4 + "TAA", 3, 8, (KEPT, 0, 17)),
    ("stop_cut_by_contig_end", "ATG" + "GCT" * 4 + "TA", 3, 8, (REJECTED,)),
    ("start_at_a", "CCC" + "ATG" + "GCT" * 3 + "TAG" + "CC", 3, 8, (KEPT, 3, 17)),
    ("stop_at_a", "ATG" + "TAA" + "GCT" * 2 + "TAA", 3, 8, (REJECTED,)),
    ("start_before_previous_stop", "ATG" + "TAA" + "GCT" + "GTG" + "GCT" * 2 + "TGA", 12, 17,
     (KEPT, 9, 20)),
    ("farthest_of_three_starts", "CC" + "TTG" + "GCT" + "GTG" + "ATG" + "GCT" * 2 + "TAG" + "C",
     14, 19, (KEPT, 2, 22)),
    ("no_start", "GCT" * 4 + "TAA", 3, 8, (REJECTED,)),
    ("out_of_frame_stop", "ATG" + "GCT" + "GTA" + "AGC" + "GCT" + "TAA", 3, 8, (KEPT, 0, 17)),
    ("ambiguous_codons", "ANG" + "ATG" + "GCT" + "TNA" + "GCT" + "TAA", 6, 11, (KEPT, 3, 17)),
    ("span_not_multiple_of_3", _A, 3, 16, (KEPT, 0, 17)),
]
EDGE_CASES = [(name, "+", *rest) for name, *rest in EDGES] + [
    (name, "-", *rest) for name, *rest in EDGES
    if name in ("stop_is_own_last_codon", "stop_is_contig_end", "start_at_a")]


@pytest.fixture(scope="module")
def edge_results(kma):
    """Every edge case as one contig of one genome, answered by one index."""
    contigs, rows, want = [], [], []
    for c, (name, strand, seq, a, b, exp) in enumerate(EDGE_CASES):
        n = len(seq)
        if strand == "+":
            contigs.append(seq)
            rows.append((c, "+", a + 1, b + 1, 1))
            want.append((KEPT, exp[1] + 1, exp[2] + 1) if exp[0] == KEPT else (REJECTED, 0, 0))
        else:
            contigs.append(revcomp(seq))
            rows.append((c, "-", n - b, n - a, 1))
            want.append((KEPT, n - exp[2], n - exp[1]) if exp[0] == KEPT else (REJECTED, 0, 0))
    got, _ = gpu_rows(kma, contigs, rows)
    return got, want, oracle_rows(contigs, rows)


@pytest.mark.parametrize("i", range(len(EDGE_CASES)),
                         ids=[f"{c[0]}{c[1]}" for c in EDGE_CASES])
def test_edge(edge_results, i):
    got, want, ora = edge_results
    assert got[i] == want[i] == ora[i]


def test_minus_stop_at_forward_base_1(edge_results):
    i = [c[:2] for c in EDGE_CASES].index(("stop_is_contig_end", "-"))
    assert edge_results[0][i] == (KEPT, 1, 18)


# ---- 3. segment isolation ---------------------------------------------------------------------------
# (name, contigs, contig, strand, span [a, b] in strand coordinates): all REJECTED, each for one
# reason only (a start but no stop, or a stop but no start), with the missing codon present in a
# neighbouring segment: the next / previous contig, the other strand, the next / previous frame.
_OPEN = "ATG" + "GCT" * 5                       # frame 0: a start, no stop
_NOSTART = "GCT" * 4 + "TAA"                    # frame 0: a stop, no start
_STARTS_BOTH = "ATG" + "GCT" * 3 + "CAT" + "GC"  # '+' frame 0 and '-' frame 2: a start, no stop
_MINUS_F2_OPEN = revcomp("GC" + "ATG" + "GCT" * 4)
_PLUS_F2_START = "GC" + "ATG" + "TTA" + "AGC" * 4  # '-' strand: GCT x 4, TAA, CAT, GC
ISOLATION = [
    ("stop_in_next_contig", [_OPEN, "TAA" + "GCT" * 3], 0, "+", 3, 17),
    ("stop_in_next_frame", ["CTAA" + "GC" + "ATG" + "GCT" * 3], 0, "+", 9, 14),
    ("start_in_previous_contig", [_STARTS_BOTH, _NOSTART], 1, "+", 3, 8),
    ("minus_stop_in_next_contig", [_MINUS_F2_OPEN, "TAA" + "GCT" * 3], 0, "-", 5, 10),
    ("stop_on_other_strand", ["GC" + "ATG" + "GCT" * 3 + "TTA"], 0, "+", 5, 10),
    ("start_on_other_strand", [_PLUS_F2_START], 0, "-", 3, 8),
]


def _isolation_cases():
    out = []
    for name, contigs, c, strand, a, b in ISOLATION:
        n = len(contigs[c])
        row = (c, "+", a + 1, b + 1, 1) if strand == "+" else (c, "-", n - b, n - a, 1)
        out.append((name, contigs, row))
        if name in ("stop_in_next_contig", "start_in_previous_contig"):  # the '-' strand twins
            mc, mrow = mirror(contigs, c, a, b)
            out.append((name + "_mirrored", mc, mrow + (1,)))
    return out


@pytest.mark.parametrize("name,contigs,row", _isolation_cases(),
                         ids=[c[0] for c in _isolation_cases()])
def test_segments_are_isolated(kma, name, contigs, row):
    got, _ = gpu_rows(kma, contigs, [row])
    assert got == oracle_rows(contigs, [row]) == [(REJECTED, 0, 0)]


# ---- 4. long carries ----------------------------------------------------------------------------------
def test_carries_across_a_20000_codon_orf(kma):
    """ATG + 20,000 x GCT + TAA in random flanks, and its reverse complement further down the
    contig: 2,000 proposals inside each extend to the one known (start, stop), whatever scan
    tile or block they sit in. The oracle walks three of each strand only (20,000 steps)."""
    rng = np.random.default_rng(21)

    def flank(n):
        return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes().decode()
    orf = "ATG" + "GCT" * 20000 + "TAA"
    f1, f2, f3 = flank(1001), flank(777), flank(500)
    contig = f1 + "TAA" + orf + f2 + revcomp("TAA" + orf) + f3
    n = len(contig)
    p0 = len(f1) + 3                      # '+' ORF: forward 0-based [p0, p0 + len(orf))
    m0 = len(f1) + 3 + len(orf) + len(f2)  # revcomp(orf): forward 0-based [m0, m0 + len(orf))
    steps = np.linspace(0, 20000 - 7, 2000).astype(int).tolist()
    rows = [(0, "+", p0 + 3 * k + 1, p0 + 3 * k + 24, 1) for k in steps]
    rows += [(0, "-", m0 + 3 * k + 1, m0 + 3 * k + 24, 1) for k in steps]
    want = [(KEPT, p0 + 1, p0 + len(orf))] * 2000 + [(KEPT, m0 + 1, m0 + len(orf))] * 2000
    got, stats = gpu_rows(kma, [contig], rows)
    assert got == want and stats == [4000, 0, 0, 0]
    some = [0, 1000, 1999, 2000, 3000, 3999]
    assert oracle_rows([contig], [rows[i] for i in some]) == [want[i] for i in some]
    assert n > 120_000


# ---- 5. filters and counters ----------------------------------------------------------------------------
_ORF300 = "ATG" + "GCT" * 98 + "TAA"


def test_filters_in_the_reference_order(kma):
    contigs = ["CC" + _ORF300 + "C", "GCT" * 10]
    span = (0, "+", 33, 56)
    rows = [span + (29,), span + (30,), span + (31,), span + (35,), (1, "+", 4, 27, 50)]
    got, stats = gpu_rows(kma, contigs, rows, 11, 0.1, 0)
    assert got == oracle_rows(contigs, rows, 11, 0.1, 0)
    assert [g[0] for g in got] == [WEAK, KEPT, KEPT, KEPT, REJECTED]
    assert got[0][1:] == got[1][1:] == (3, 302)  # weak and small keep their edges
    got, stats = gpu_rows(kma, contigs, rows, 11, 0.1, 40)
    assert got == oracle_rows(contigs, rows, 11, 0.1, 40)
    # 29: weak as well as small counts as weak; 35: strong enough but small
    assert [g[0] for g in got] == [WEAK, SMALL, SMALL, SMALL, REJECTED]
    assert stats == [5, 1, 1, 3]
    hist = np.bincount([g[0] for g in got], minlength=4)
    assert stats[0] == len(rows) and stats[1:] == hist[1:].tolist()


def test_no_proposals(kma):
    dna, off = kma.pack_strings([_ORF300])
    with kma.OrfIndex(dna, off) as idx:
        left, right, status, stats = kma.extend_proposals(idx, np.zeros(0, kma.PROPOSAL_DTYPE),
                                                          0.1, 10)
    assert len(left) == len(right) == len(status) == 0 and stats.tolist() == [0, 0, 0, 0]


def test_invalid_arguments(kma):
    import ctypes as C
    lib = kma.load()
    dna, off = kma.pack_strings([_ORF300, _ORF300])
    h = C.c_void_p()
    for code in (0, 2, 3, 25):
        assert lib.kma_orf_index_create(dna.ctypes.data, off.ctypes.data, 2, code, 0,
                                        C.byref(h)) == kma.E_INVALID
        with pytest.raises(kma.KmerAnnoError):
            kma.OrfIndex(dna, off, code)
    big = np.array([0, 1 << 31], np.uint64)  # refused on the offsets alone
    assert lib.kma_orf_index_create(dna.ctypes.data, big.ctypes.data, 1, 11, 0,
                                    C.byref(h)) == kma.E_INVALID
    assert lib.kma_orf_index_create(dna.ctypes.data, None, 2, 11, 0, C.byref(h)) == kma.E_INVALID
    assert lib.kma_orf_index_create(dna.ctypes.data, off.ctypes.data, 2, 11, 0,
                                    None) == kma.E_INVALID
    assert lib.kma_orf_index_create(None, off.ctypes.data, 2, 11, 0, C.byref(h)) == kma.E_INVALID
    ok = (0, "+", 4, 27, 5)
    with kma.OrfIndex(dna, off) as idx:
        for bad in ((2, "+", 4, 27, 5), (0, "x", 4, 27, 5), (0, "+", 4, 5, 5), (0, "-", 9, 4, 5)):
            with pytest.raises(kma.KmerAnnoError) as e:
                kma.extend_proposals(idx, make_props(kma, [ok, bad]), 0.0, 0)
            assert e.value.code == kma.E_INVALID
        p = make_props(kma, [ok])
        out = [np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.uint8),
               np.zeros(4, np.uint64)]
        ptrs = [x.ctypes.data for x in out]
        assert lib.kma_extend_proposals(idx._h, p.ctypes.data, 1, 0.0, 0, *ptrs) == kma.OK
        assert lib.kma_extend_proposals(None, p.ctypes.data, 1, 0.0, 0, *ptrs) == kma.E_INVALID
        assert lib.kma_extend_proposals(idx._h, None, 1, 0.0, 0, *ptrs) == kma.E_INVALID
        for k in range(4):
            q = list(ptrs)
            q[k] = None
            assert lib.kma_extend_proposals(idx._h, p.ctypes.data, 1, 0.0, 0,
                                            *q) == kma.E_INVALID


# ---- 6. end to end on the reference's fixture --------------------------------------------------------------
@pytest.fixture(scope="module")
def joined(kma, oracle_c, small_gto):
    """small.gto's pegs mutated 5% as the close genome, projected onto small.gto's contigs (the
    recipe of tests/test_gpu_proposals.py): (AGGRESSIVE hits, peg protein lengths, dna, offsets)."""
    rng = np.random.default_rng(9)
    prots = [f["protein_translation"] for f in small_gto["features"]
             if f.get("protein_translation")]
    aa = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
    close = []
    for p in prots:
        b = np.frombuffer(p.encode(), np.uint8).copy()
        m = rng.random(len(b)) < 0.05
        b[m] = aa[rng.integers(0, 20, int(m.sum()))]
        close.append(b.tobytes().decode())
    res, off = oracle_c.pack_strings(close)
    dna, doff = oracle_c.pack_strings([c["dna"] for c in small_gto["contigs"]])
    t, _ = kma.SignatureTable.from_pegs(res, off, K)
    with t:
        agg = kma.connect_pegs(t, dna, doff, 11, False)
    return agg, np.array([len(p) for p in close], np.uint32), dna, doff


def test_projection_of_small_gto_end_to_end(kma, joined, small_gto):
    """propose_pegs -> OrfIndex -> extend_proposals -> annotate_proposals(extended=...) gives the
    features, order and counters of the oracle's literal PegProposalList fed the same proposals."""
    from kmeranno import projector
    hits, peg_len, dna, doff = joined
    props, _ = kma.propose_pegs(hits, peg_len, K)
    with kma.OrfIndex(dna, doff) as idx:
        left, right, status, stats = kma.extend_proposals(idx, props, 0.5 / 3, 10)
    contigs = [c["dna"] for c in small_gto["contigs"]]
    ids = [c["id"] for c in small_gto["contigs"]]
    funcs = [f.get("function", "") for f in small_gto["features"]
             if f.get("protein_translation")]
    feats, plist = projector.annotate_proposals(props, funcs, contigs, small_gto["id"], ids,
                                                extended=(left, right, status))
    olist = ProposalList(dict(zip(ids, contigs)), 0.5 / 3, 10)
    for p in props:
        c = int(p["contig"])
        olist.propose(Loc(ids[c], chr(p["strand"]), int(p["left"]), int(p["right"])),
                      funcs[int(p["peg"])], int(p["evidence"]))
    exp = [(q.function, q.loc.contig_id, q.loc.dir, q.loc.left, q.loc.right, q.evidence)
           for q in olist]
    got = [(f[1], ids[f[2].contig], f[2].strand, f[2].left, f[2].right, f[3]) for f in feats]
    assert len(got) > 400 and got == exp
    assert [f[0] for f in feats] == [f"fig|{small_gto['id']}.peg.{i + 1}" for i in range(len(got))]
    counters = (olist.made, olist.rejected, olist.weak, olist.small, olist.merged)
    assert (plist.made, plist.rejected, plist.weak, plist.small, plist.merged) == counters
    assert stats.tolist() == list(counters[:4])


# ---- 7. index reuse and concurrency ----------------------------------------------------------------------------
def test_one_index_four_threads(kma, small):
    contigs, rows, exp = small
    props = make_props(kma, rows)
    dna, off = kma.pack_strings(contigs)
    cut = [len(props) * i // 4 for i in range(5)]
    got, errors = [None] * 4, []
    with kma.OrfIndex(dna, off) as idx:
        single = kma.extend_proposals(idx, props, 0.0, 0)

        def run(i):
            try:
                for _ in range(5):
                    got[i] = kma.extend_proposals(idx, props[cut[i]:cut[i + 1]], 0.0, 0)
            except Exception as e:  # noqa: BLE001 (reported below)
                errors.append(e)
        threads = [threading.Thread(target=run, args=(i,)) for i in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=120)
        assert not errors and not any(t.is_alive() for t in threads)
    assert list(zip(single[2].tolist(), single[0].tolist(), single[1].tolist())) == exp[11]
    for i in range(4):
        for k in range(3):
            assert np.array_equal(got[i][k], single[k][cut[i]:cut[i + 1]]), (i, k)
        assert got[i][3][0] == cut[i + 1] - cut[i]
