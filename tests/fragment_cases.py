"""Fragmented genomes: thousands of contigs per call, many shorter than one probe window.

Every genome-side operator finds a position's contig by a search of the offsets array, each with
code of its own (the 6-frame probe's ballot / 64-ary wave search / per-lane binary search, the
ORF index's search of its segment offsets, the proposal sweep's contig runs, the translation's
search of its output offsets, the host call's replica shards). The builders here cut the
reference's fixture small.gto into draft-assembly shapes that take those searches through every
branch; tests/test_fragment_workload.py shows on the oracle alone that each workload meets the
conditions tests/test_gpu_fragments.py relies on.

  frag4k(gto)      small.gto's bases, unchanged and in order, re-cut into more than 4,200 contigs
  boundary(gto, n) the first n pieces of frag4k, the last lengthened by a gene (n around 64, 4096)
  frag262k(gto)    262,145 contigs (64^3 + 1): tiny ones and 20 gene-bearing ones

Every builder is deterministic (fixed seeds) and cached; the arrays are read-only.
"""
from __future__ import annotations

import types

import numpy as np

# the oracle composition of a location's protein, the close genome and the timestamp: one copy
from test_gpu_translate import STAMP, close_genome, java_4f, raw_and_peg  # noqa: F401

K = 8
CONTIG_TILE = 1024  # forward positions per 6-frame probe block: kContigTile (csrc/kma_internal.h)
OFF_CACHE = 64      # offsets a probe block caches: kOffCache (csrc/kma_contigs.hip)
TR_TILE = 1024      # residues per translate block: kTrTile (csrc/kma_translate.h)
BOUNDARY_COUNTS = (63, 64, 65, 4095, 4096, 4097)
PAST = (0, 1, 3 * K - 1, 3 * K, 3 * K + 2)  # a contig's last base, in bases past a tile boundary
N_FID = 300
N_262K = 64 ** 3 + 1
GENE_POSITIONS_262K = (0, 1, 4095, 4096, 4097, 20_000, 41_000, 62_000, 83_000, 104_000, 131_072,
                       150_000, 170_000, 190_000, 210_000, 230_000, 250_000, 262_142, 262_143,
                       262_144)

_cache: dict = {}


def _frozen(a):
    a.flags.writeable = False
    return a


def source_bases(gto) -> np.ndarray:
    """small.gto's contigs concatenated in order (768,718 bases)."""
    if "source" not in _cache:
        text = "".join(c["dna"] for c in gto["contigs"])
        _cache["source"] = _frozen(np.frombuffer(text.encode(), np.uint8).copy())
    return _cache["source"]


def _genome(name, dna_bytes, lens, ids=None, **marks):
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens, dtype=np.uint64)
    assert int(off[-1]) == len(dna_bytes)
    dna = np.concatenate([dna_bytes, np.zeros(32, np.uint8)])
    g = types.SimpleNamespace(name=name, dna=_frozen(dna), off=_frozen(off), n_contig=len(lens),
                              n_bases=len(dna_bytes), lens=_frozen(np.asarray(lens, np.int64)),
                              ids=ids, **marks)
    g._contigs = None
    return g


def contig_strings(g):
    """The contigs of a genome as Python strings (built on first use)."""
    if g._contigs is None:
        text = g.dna[:g.n_bases].tobytes().decode("latin-1")
        o = g.off.astype(np.int64).tolist()
        g._contigs = [text[a:b] for a, b in zip(o[:-1], o[1:])]
    return g._contigs


# ---- frag4k ---------------------------------------------------------------------------------------

def _frag4k_lengths(total):
    """Piece lengths summing to `total`, emitted left to right so that a piece's length can be
    chosen from the running offset (the alignments below). Returns (lengths, marks)."""
    rng = np.random.default_rng(4200)
    n_short, n_empty = 3900, 60
    # 36% of the short pieces hold no whole codon (1 or 2 bases): empty translate locations
    short = np.where(rng.random(n_short) < 0.36, rng.integers(1, 3, n_short),
                     rng.integers(3, 48, n_short))
    # the dense run: 84 contigs of 1..14 bases, every third long enough (12..14) for K = 3 hits
    dense = rng.integers(1, 12, 84)
    dense[::3] = rng.integers(12, 15, len(dense[::3]))
    tiny_run = rng.integers(1, 3, 56)  # 56 contigs in a row without a whole codon
    tail_short = [5, 31, 2]
    d_sum = int(dense.sum())
    assert 5 + d_sum + 200 <= CONTIG_TILE
    # the gene-bearing piece after the dense run: sized so that the run starts 5 bases into a tile
    tail_long = 1500 + (total - sum(tail_short) - d_sum - 1500 - 5) % CONTIG_TILE
    specials = [("pair", p) for p in PAST] + [("before", 0), ("at", 0), ("after", 0)]
    budget = (total - int(short.sum()) - 4400 * len(specials) - int(tiny_run.sum()) - d_sum
              - tail_long - sum(tail_short))
    longs, rem = [], budget
    while rem > 4000:
        x = int(rng.integers(400, 4001))
        if rem - x < 400:
            x = rem - 400
        longs.append(x)
        rem -= x
    assert 400 <= rem <= 4000
    items = ([("s", int(x)) for x in short] + [("e", 0)] * n_empty + [("l", x) for x in longs]
             + specials + [("tiny", 0)])
    items = [items[i] for i in rng.permutation(len(items))]
    lens, marks = [], {"pair_ends": {}, "empty_at_boundary": {}}
    pos = 0

    def put(n):
        nonlocal pos
        lens.append(int(n))
        pos += int(n)

    for kind, v in items:
        if kind in ("s", "l", "e"):
            put(v)
        elif kind == "tiny":
            marks["tiny_run"] = (len(lens), len(tiny_run))
            for x in tiny_run:
                put(x)
        elif kind == "pair":  # two long pieces, the first ending v bases past a tile boundary
            d = (v - (pos + 1200)) % CONTIG_TILE
            marks["pair_ends"][v] = len(lens)
            put(1200 + d)
            put(3200 - d)
        elif kind == "before":  # an empty contig one base before a boundary
            d = (-1 - (pos + 1200)) % CONTIG_TILE
            put(1200 + d)
            marks["empty_at_boundary"]["before"] = len(lens)
            put(0)
            put(1)
            put(3199 - d)
        elif kind == "at":  # an empty contig on a boundary, a gene-bearing contig after it
            d = (-(pos + 1200)) % CONTIG_TILE
            put(1200 + d)
            marks["empty_at_boundary"]["at"] = len(lens)
            put(0)
            put(3200 - d)
        else:  # "after": an empty contig one base after a boundary
            d = (-(pos + 1200)) % CONTIG_TILE
            put(1200 + d)
            put(1)
            marks["empty_at_boundary"]["after"] = len(lens)
            put(0)
            put(3199 - d)
    put(rem)
    marks["dense_run"] = (len(lens), len(dense))
    for x in dense:
        put(x)
    put(tail_long)
    for x in tail_short:
        put(x)
    put(0)
    put(0)
    assert pos == total
    return np.array(lens, np.int64), marks


def frag4k(gto):
    if "frag4k" not in _cache:
        src = source_bases(gto)
        lens, marks = _frag4k_lengths(len(src))
        ids = [f"frag_{i}" for i in range(len(lens))]  # unpadded: string order != index order
        _cache["frag4k"] = _genome("frag4k", src, lens, ids, **marks)
    return _cache["frag4k"]


def frag4k_half_empty(gto):
    """frag4k with the contig that holds the half-way base split there and 50 empty contigs put
    between the halves: the host call's two replica shards then meet inside a run of empties."""
    if "frag4k_half" not in _cache:
        g = frag4k(gto)
        half = g.n_bases // 2
        off = g.off.astype(np.int64)
        c = int(np.searchsorted(off, half, side="right")) - 1
        assert off[c] < half < off[c + 1]
        lens = np.concatenate([g.lens[:c], [half - off[c]], np.zeros(50, np.int64),
                               [off[c + 1] - half], g.lens[c + 1:]])
        _cache["frag4k_half"] = _genome("frag4k_half", g.dna[:g.n_bases], lens, None,
                                        empties=(c + 1, 50))
    return _cache["frag4k_half"]


def planted_gene(gto) -> np.ndarray:
    """The bases of small.gto's first '+' strand peg of 600 to 1,200 bases."""
    ids = [c["id"] for c in gto["contigs"]]
    for f in gto["features"]:
        if f.get("protein_translation") and len(f["location"]) == 1:
            cid, begin, strand, length = f["location"][0]
            begin, length = int(begin), int(length)
            if strand == "+" and 600 <= length <= 1200:
                dna = gto["contigs"][ids.index(cid)]["dna"][begin - 1:begin - 1 + length]
                return np.frombuffer(dna.encode(), np.uint8)
    raise AssertionError("no such peg")


def boundary(gto, n):
    """The first n pieces of frag4k, the last one lengthened by planted_gene."""
    if ("boundary", n) not in _cache:
        g = frag4k(gto)
        gene = planted_gene(gto)
        lens = g.lens[:n].copy()
        lens[-1] += len(gene)
        dna = np.concatenate([g.dna[:int(g.off[n])], gene])
        _cache["boundary", n] = _genome(f"n{n}", dna, lens, None)
    return _cache["boundary", n]


# ---- frag262k -------------------------------------------------------------------------------------

def frag262k(gto):
    if "frag262k" not in _cache:
        src = source_bases(gto)
        rng = np.random.default_rng(262_145)
        n = N_262K
        # 30% empty; of the rest 58% have 6 bases (the one length that keeps a residue once peg
        # mode drops the last codon, so that both modes fill more than 100 translate tiles), the
        # others 1..5
        tiny = np.where(rng.random(n) < 0.58, 6, rng.integers(1, 6, n))
        lens = np.where(rng.random(n) < 0.3, 0, tiny).astype(np.int64)
        lens[200_000:200_060] = rng.integers(0, 3, 60)  # 60 contigs in a row without a codon
        genes = np.array(GENE_POSITIONS_262K)
        lens[genes] = rng.integers(600, 2001, len(genes))
        off = np.zeros(n + 1, np.int64)
        off[1:] = np.cumsum(lens)
        dna = np.empty(int(off[-1]), np.uint8)
        is_gene = np.zeros(n, bool)
        is_gene[genes] = True
        tiny_base = ~np.repeat(is_gene, lens)
        dna[tiny_base] = np.resize(src, int(tiny_base.sum()))
        for i, p in enumerate(genes):  # gene-dense stretches of small.gto, 30 kb apart
            s = 5000 + 30_000 * i
            dna[off[p]:off[p + 1]] = src[s:s + lens[p]]
        _cache["frag262k"] = _genome("frag262k", dna, lens, None, genes=tuple(genes.tolist()))
    return _cache["frag262k"]


# ---- what the offsets say about the probe ------------------------------------------------------------

def wave_search_rounds(n_contig) -> int:
    """The most rounds the probe's 64-ary wave search takes over n_contig offsets
    (contig_of_wave); a position in the last, shorter slot of a round can finish sooner."""
    span, rounds = n_contig, 0
    while span > 1:
        span = (span + 63) // 64  # the widest span a round can leave
        rounds += 1
    return rounds


def wave_search_rounds_at(off, g) -> int:
    """The rounds contig_of_wave takes for position g of these offsets (its arithmetic, lane by
    lane collapsed to the count of candidates <= g)."""
    off = np.asarray(off, np.int64)
    lo, span, rounds = 0, len(off) - 1, 0
    while span > 1:
        step = (span + 63) // 64
        cand = lo + np.arange(64) * step
        le = (np.arange(64) * step < span) & (off[np.minimum(cand, len(off) - 1)] <= g)
        nlo = lo + (int(le.sum()) - 1) * step
        span = min(step, lo + span - nlo)
        lo = nlo
        rounds += 1
    assert lo == np.searchsorted(off[:-1], g, side="right") - 1  # the plain search's contig
    return rounds


def tile_search_rounds(off):
    """{rounds: tiles} of the wave search for every tile's first position."""
    off = np.asarray(off, np.int64)
    out = {}
    for r0 in range(0, int(off[-1] - off[0]), CONTIG_TILE):
        r = wave_search_rounds_at(off, int(off[0]) + r0)
        out[r] = out.get(r, 0) + 1
    return dict(sorted(out.items()))


def probe_tiles(off):
    """Per probe tile of a genome's offsets: (first contig, contigs met), as the kernel finds them
    (the largest c < n with off[c] <= the tile's first / last position)."""
    off = np.asarray(off, np.int64)
    n = len(off) - 1
    base, total = off[0], off[-1] - off[0]
    r0 = np.arange(0, max(total, 1), CONTIG_TILE)
    last = np.minimum(r0 + CONTIG_TILE, total)
    lo = np.searchsorted(off[:n], base + r0, side="right") - 1
    hi = np.searchsorted(off[:n], base + np.maximum(last - 1, 0), side="right") - 1
    return lo, hi - lo + 1


def probe_paths(off):
    """How many tiles take each of the probe's three ways to a position's contig: 'ballot'
    (n_contig < 64), 'window' (a wave search and the cached offsets[c .. c + 64]), 'global' (more
    than 64 contigs meet the tile: a binary search per lane); 'clamped': the window tiles whose
    cached window is cut short at n_contig."""
    n = len(off) - 1
    lo, nc = probe_tiles(off)
    if n < OFF_CACHE:
        return {"ballot": len(lo), "window": 0, "global": 0, "clamped": 0}
    window = nc <= OFF_CACHE
    return {"ballot": 0, "window": int(window.sum()), "global": int((~window).sum()),
            "clamped": int((window & (lo + OFF_CACHE > n)).sum())}


def hit_tiles(off, contig, left):
    """The probe tile of each hit (contig, 1-based left)."""
    off = np.asarray(off, np.int64)
    return (off[np.asarray(contig, np.int64)] - off[0] + np.asarray(left, np.int64) - 1) \
        // CONTIG_TILE


# ---- tables and the close genome ---------------------------------------------------------------------

def sample_table(oracle_c, g, k, gcode=11):
    """Half of the genome's own K-mers with random fids below N_FID, rows in file order (the last
    row of a kmer wins): half of its kmer records at K = 8, half of its distinct kmers at K = 3
    (where half the records would hold nearly every 3-mer). (rows (n, k) u8, fids i32)."""
    key = ("table", g.name, k, gcode)
    if key not in _cache:
        km = oracle_c.contig_kmers(g.dna, g.off, gcode, k)[0]
        rng = np.random.default_rng([sum(g.name.encode()), k, gcode])
        if k <= 4:  # distinct kmers, in the order of their packed bytes
            packed = np.zeros(len(km), np.uint32)
            for j in range(k):
                packed = (packed << np.uint32(8)) | km[:, j]
            km = km[np.unique(packed, return_index=True)[1]]
        rows = np.ascontiguousarray(km[rng.random(len(km)) < 0.5])
        fids = rng.integers(0, N_FID, len(rows)).astype(np.int32)
        _cache[key] = (_frozen(rows), _frozen(fids))
    return _cache[key]


def oracle_table(oracle_c, rows, fids):
    k = rows.shape[1]
    return oracle_c.Table.from_buffer(rows.tobytes(), np.arange(len(rows) + 1, dtype=np.uint64) * k,
                                      fids)


def expect_contigs(oracle_c, g, k, gcode=11):
    """oracle_c.annotate_contigs of the genome against its sample_table, once per (genome, K)."""
    key = ("hits", g.name, k, gcode)
    if key not in _cache:
        rows, fids = sample_table(oracle_c, g, k, gcode)
        e = oracle_c.annotate_contigs(oracle_table(oracle_c, rows, fids), g.dna, g.off, gcode, k)
        _cache[key] = tuple(_frozen(a) for a in e)
    return _cache[key]


def close_proteins(gto, seed=9):
    """small.gto's pegs mutated 5% (test_gpu_translate.close_genome's; seed 9 gives the close
    genome of tests/test_gpu_proposals.py)."""
    return [f["protein_translation"] for f in close_genome(gto, seed, "close")["features"]]


def expect_join(oracle_c, gto, strict=False):
    """The oracle's peg join of close_proteins with frag4k: ((contig, left, strand, frame, peg),
    peg lengths)."""
    key = ("join", strict)
    if key not in _cache:
        g = frag4k(gto)
        close = close_proteins(gto)
        res, off = oracle_c.pack_strings(close)
        e = oracle_c.peg_connect(res, off, g.dna, g.off, 11, K, strict)
        _cache[key] = (tuple(_frozen(a) for a in e),
                       _frozen(np.array([len(p) for p in close], np.uint32)))
    return _cache[key]


LOOSE = dict(min_strength=0.05, max_fuzz=2.5, min_fuzz=0.3)  # test_gpu_proposals.py's "loose"


def expect_proposals(oracle_c, gto, loose=False):
    """oracle_c.propose on the AGGRESSIVE join: (proposal arrays, stats)."""
    key = ("proposals", loose)
    if key not in _cache:
        (ct, lf, sd, _, pg), peg_len = expect_join(oracle_c, gto)
        _cache[key] = oracle_c.propose(ct, lf, sd, pg, peg_len, K, **(LOOSE if loose else {}))
    return _cache[key]


# test_proposals_synthetic_dense's second parameter set
SYNTHETIC_LOOSE = dict(min_strength=0.01, max_fuzz=3.0, min_fuzz=0.1)


def synthetic_connections(hit_dtype):
    """200,000 connections of 300 pegs over 5,000 contigs in canonical order: a peg's list then
    crosses hundreds of contig runs, most of them 1 to 3 connections long."""
    rng = np.random.default_rng(5000)
    n, n_peg, n_ctg = 200_000, 300, 5000
    h = np.zeros(n, hit_dtype)
    h["contig"] = rng.integers(0, n_ctg, n)
    h["left"] = rng.integers(1, 3000, n)
    h["strand"] = np.where(rng.random(n) < 0.5, ord("+"), ord("-"))
    h["fid"] = rng.integers(0, n_peg, n)
    h = np.unique(h)
    h = h[np.lexsort((h["left"], h["contig"]))]
    return h, rng.integers(30, 900, n_peg).astype(np.uint32)


# ---- ORF rows ---------------------------------------------------------------------------------------

def short_contig_spans(g, max_rows=30_000, seed=48):
    """Rows (contig, strand, left, right, evidence) of every span of 3 to 24 bases on both strands
    of every contig shorter than 48 bases, sampled down to max_rows (evidence 1..40)."""
    short = np.flatnonzero((g.lens >= 3) & (g.lens < 48))
    rows = [(int(c), s, lft, lft + ln - 1) for c in short
            for ln in range(3, min(24, int(g.lens[c])) + 1)
            for lft in range(1, int(g.lens[c]) - ln + 2) for s in "+-"]
    rng = np.random.default_rng(seed)
    if len(rows) > max_rows:
        rows = [rows[i] for i in np.sort(rng.choice(len(rows), max_rows, replace=False))]
    ev = rng.integers(1, 41, len(rows)).tolist()
    return [r + (e,) for r, e in zip(rows, ev)]


def frag4k_orf_rows(oracle_c, gto):
    """short_contig_spans of frag4k, then the oracle's real proposals from the join."""
    if "orf_rows" not in _cache:
        _cache["orf_rows"] = short_contig_spans(frag4k(gto)) + proposal_rows(
            expect_proposals(oracle_c, gto)[0])
    return _cache["orf_rows"]


KEPT, REJECTED, WEAK, SMALL = 0, 1, 2, 3


def oracle_orf_rows(contigs, rows, gcode=11, min_strength=0.0, min_evidence=0):
    """(status, left, right) per row (contig, strand, left, right, evidence) from the oracle's
    extend and PegProposalList.propose's filter order (as tests/test_gpu_orf.py composes them)."""
    from oracle.proposal_list import Loc, extend
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


def proposal_rows(prop):
    """oracle_c.propose's arrays as rows (contig, strand, left, right, evidence)."""
    return [(int(c), chr(s), int(a), int(b), int(e)) for c, s, a, b, e in
            zip(prop["contig"], prop["strand"], prop["left"], prop["right"], prop["evidence"])]


def whole_contig_locations(g):
    """One location per contig (contig, strand, left, right): the whole contig, strands
    alternating, an empty contig as left = 1, right = 0."""
    c = np.arange(g.n_contig)
    return c, np.where(c % 2 == 0, ord("+"), ord("-")).astype(np.uint8), \
        np.ones(g.n_contig, np.int32), g.lens.astype(np.int32)


# ---- translation -------------------------------------------------------------------------------------

def expect_whole_contigs(g):
    """([raw proteins], [peg proteins]) of whole_contig_locations(g), once per genome."""
    key = ("translate", g.name)
    if key not in _cache:
        contigs = contig_strings(g)
        both = [raw_and_peg(x, "+-"[c & 1], 1, len(x), 11) if len(x) >= 3 else ("", "")
                for c, x in enumerate(contigs)]
        _cache[key] = ([b[0] for b in both], [b[1] for b in both])
    return _cache[key]


# ---- the projection end to end ----------------------------------------------------------------------

CLOSE_GENOMES = ((9, "1000.1"), (10, "1000.2"))


def new_genome(gto):
    """frag4k as the GTO of a new genome: small.gto's id, the unpadded contig ids, no feature."""
    g = frag4k(gto)
    return {"id": gto["id"], "genetic_code": 11, "features": [],
            "contigs": [{"id": i, "dna": d} for i, d in zip(g.ids, contig_strings(g))]}


def expect_projection(oracle_c, gto):
    """The oracle chain of project_genome(new_genome, both close genomes): the C oracle's join
    and sweep per close genome, the literal PegProposalList over all their proposals in order,
    the oracle's translation of every kept ORF. (features, counters, contig index per feature)."""
    if "projection" not in _cache:
        from oracle.proposal_list import Loc, ProposalList
        g = frag4k(gto)
        contigs, ids = contig_strings(g), g.ids
        olist = ProposalList(dict(zip(ids, contigs)), 0.5 / 3, 10)
        made = 0
        for seed, gid in CLOSE_GENOMES:
            close = close_genome(gto, seed, gid)
            prots = [f["protein_translation"] for f in close["features"]]
            funcs = [f["function"] for f in close["features"]]
            res, off = oracle_c.pack_strings(prots)
            ct, lf, sd, _, pg = oracle_c.peg_connect(res, off, g.dna, g.off, 11, K, False)
            prop, _ = oracle_c.propose(ct, lf, sd, pg, np.array([len(p) for p in prots]), K)
            made += len(prop["peg"])
            for c, s, a, b, e, p in zip(prop["contig"].tolist(), prop["strand"].tolist(),
                                        prop["left"].tolist(), prop["right"].tolist(),
                                        prop["evidence"].tolist(), prop["peg"].tolist()):
                olist.propose(Loc(ids[c], chr(s), a, b), funcs[p], e)
        index = {cid: i for i, cid in enumerate(ids)}
        want, where = [], []
        for i, q in enumerate(olist, start=1):
            loc = q.loc
            c = index[loc.contig_id]
            prot = raw_and_peg(contigs[c], loc.dir, loc.left, loc.right, 11)[1]
            note = "Annotated with evidence %d and strength %s" % (q.evidence,
                                                                   java_4f(q.strength()))
            want.append({"id": f"fig|{gto['id']}.peg.{i}", "type": "CDS", "function": q.function,
                         "location": [[loc.contig_id, str(loc.begin()), loc.dir, loc.length()]],
                         "protein_translation": prot,
                         "annotations": [[note, "kmers.anno", STAMP, ""],
                                         ["Set function to " + q.function, "kmers.anno", STAMP,
                                          ""]]})
            where.append(c)
        counters = {"made": olist.made, "merged": olist.merged, "rejected": olist.rejected,
                    "weak": olist.weak, "small": olist.small, "kept": len(want)}
        assert olist.made == made
        _cache["projection"] = (want, counters, where)
    return _cache["projection"]


def features_out_of_index_order(where, ids):
    """How many features sit on a contig whose rank by id string, among the contigs that carry a
    feature, differs from its rank by index."""
    used = sorted(set(where))
    by_id = sorted(used, key=lambda c: ids[c])
    moved = {c for c, d in zip(used, by_id) if c != d}
    return sum(c in moved for c in where)
