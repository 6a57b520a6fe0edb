"""Inputs and ordered step lists of the long-lived-object sessions, shared by
tests/test_session_workload.py (CPU, the oracle alone) and tests/test_gpu_sessions.py.

A JNI host creates a table once and calls it for every genome, with proteins and contigs in
turn and batches of very different sizes; the pooled host contexts, the workspaces and the strict
join's counters survive every call. The sessions here run many kinds of call on ONE table (or
workspace) in a fixed order, and every step's expected value is the oracle's answer on that step's
input alone, so a step that inherits anything from the step before it is caught.

One K = 8 table serves every protein and contig step. Its rows are
  - the 20,000 rows of synth.make_table(20_000, 300, SEED): what synth.make_workload and
    synth.make_contig_workload of that seed both build their inputs against;
  - every window of one 12,000-residue prototype, all on function LONG_FID: a protein cut from it
    is CALLED with a count as large as its window count (the LDS pool and the workspace hash set
    of step 8);
  - about half of the 6-frame kmers of the 20 kb genome g20 under each of the 18 genetic codes
    (step 11; a kmer is in or out by a hash of its key, whatever the code), fid = key mod 300.
Plain numpy and the C oracle; no GPU.
"""
import functools
import types

import numpy as np

from kmeranno import synth

K = 8
MIN_HITS = 5
N_FID = 300
SEED = 61
LONG_FID = 7
ALL_CODES = (1, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13, 14, 16, 21, 22, 23, 24, 25)
F_END_EXCLUSIVE, F_MULTISET = 1, 2
CONTIG_TILE = 1024          # forward positions per probe block
EMIT_GROUP = 256            # probe blocks per emit-offset group
PIECE_MIN = 60_000          # KMA_OPT_HOST_PIECE_MIN of the p1500 steps: >= 4 pipeline pieces
DEGENERATE_LENGTHS = [0, 3, 7, 8, 0, 0, 9, 120, 1, 0, 640, 5, 0]  # test_degenerate_proteins'
HIT_FIELDS = ("contig", "left", "strand", "frame", "fid")


# ---- the table ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def signatures():
    """synth's 20,000-row table and its 300 prototypes."""
    return synth.make_table(20_000, N_FID, SEED, K)


@functools.lru_cache(maxsize=None)
def long_proto():
    return synth.AA[np.random.default_rng(SEED + 1).integers(0, 20, 12_000)]


def _pack_rows(kmers_u8):
    """Standard packed keys of an (n, K) uint8 array of kmers over A-Z."""
    keys = np.zeros(len(kmers_u8), np.uint64)
    for j in range(K):
        keys = (keys << np.uint64(5)) | (kmers_u8[:, j].astype(np.uint64) - np.uint64(64))
    return keys


@functools.lru_cache(maxsize=None)
def table_rows():
    """(keys, fids) of the long-lived signature table, in file order."""
    from oracle import c_oracle
    sig = signatures()
    rng = np.random.default_rng(SEED + 2)
    long_keys = np.unique(synth.window_keys(long_proto(), K))
    keys, fids = [sig.keys, long_keys], [sig.fids, np.full(len(long_keys), LONG_FID, np.uint32)]
    dna, off = genome("g20")
    code_keys = []
    for code in ALL_CODES:
        km = c_oracle.contig_kmers(dna, off, code, K)[0]
        ck = np.unique(_pack_rows(km))
        code_keys.append(ck[(ck * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(63) == 0])
    ck = rng.permutation(np.unique(np.concatenate(code_keys)))
    keys.append(ck)
    fids.append((ck % np.uint64(N_FID)).astype(np.uint32))
    return np.concatenate(keys), np.concatenate(fids).astype(np.uint32)


def table_kmers():
    """The rows' kmers as strings (the row-text creators)."""
    from helpers import unpack_keys
    return [r.tobytes().decode() for r in unpack_keys(table_rows()[0], K)]


_ORACLE = {}


def oracle_table(oracle_c):
    if "t" not in _ORACLE:
        from helpers import full_oracle_table
        _ORACLE["t"] = full_oracle_table(oracle_c, *table_rows(), K)
    return _ORACLE["t"]


# ---- protein batches ----------------------------------------------------------------------------
def _pack(prots):
    off = np.zeros(len(prots) + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for p in prots], dtype=np.uint64)
    res = np.concatenate([np.asarray(p, np.uint8) for p in prots] + [np.zeros(32, np.uint8)])
    return res, off


def _hits(prot, keys_sorted):
    return int(np.isin(np.unique(synth.window_keys(prot, K)), keys_sorted).sum())


def _mutate(rng, prot, rate):
    out = prot.copy()
    m = rng.random(len(out)) < rate
    out[m] = synth.AA[rng.integers(0, 20, int(m.sum()))]
    return out


@functools.lru_cache(maxsize=None)
def protein_batch(name):
    """(residues padded by 32 bytes, offsets) of a named batch.
    p13   : the 13 lengths of test_degenerate_proteins. The length-8 protein is a table row (one
            hit: BELOW_MIN), the 120 one the head of a prototype (CALLED), the 640 one the heads of
            two prototypes (AMBIGUOUS), the rest random (NONE).
    p1500 : 1,480 synthetic queries (copies, random proteins, chimeras) and 20 prototypes followed
            by their own first 100 residues (windows that occur twice: KMA_F_MULTISET counts them
            twice).
    p200  : the first 200 proteins of p1500.
    plong : step 8's three long proteins between short ones.
    pbig  : p1500 twice over, for the device session's larger reservation."""
    sig = signatures()
    rng = np.random.default_rng(SEED + 3 + sum(map(ord, name)))
    ks = np.sort(sig.keys)
    rich = [p for p in sig.protos if len(p) >= 320 and _hits(p[:120], ks) >= 2 * MIN_HITS]
    if name == "p13":
        prots = []
        for n in DEGENERATE_LENGTHS:
            if n == 8:
                prots.append(np.frombuffer(synth.unpack_key(sig.keys[0], K).encode(), np.uint8))
            elif n == 120:
                prots.append(rich[0][:120])
            elif n == 640:
                prots.append(np.concatenate([rich[1][:320], rich[2][:320]]))
            else:
                prots.append(synth.AA[rng.integers(0, 20, n)])
        return _pack(prots)
    if name == "p1500":
        res, off, _, _ = synth.make_queries(sig, 1480, SEED * 1_000_003 + 17)
        prots = [res[int(a):int(b)] for a, b in zip(off[:-1], off[1:])]
        prots += [np.concatenate([p, p[:100]]) for p in rich[3:23]]
        assert len(prots) == 1500
        return _pack(prots)
    if name == "p200":
        from helpers import take_proteins
        return take_proteins(*protein_batch("p1500"), np.arange(200))
    if name == "pbig":
        res, off = protein_batch("p1500")
        n = int(off[-1])
        return (np.concatenate([res[:n], res]), np.concatenate([off, off[1:] + np.uint64(n)]))
    if name == "plong":
        lp = long_proto()
        shorts = [rich[i][:n] for i, n in zip(range(4, 13), (50, 60, 70, 80, 90, 40, 33, 0, 100))]
        prots = [shorts[0], lp[3000:5807]] + shorts[1:5] + [lp, shorts[5],
                                                             _mutate(rng, lp[7000:10_000], 0.10)]
        return _pack(prots + shorts[6:])
    raise KeyError(name)


PLONG_AT = {"lds": 1, "gset": 6, "third": 8}  # indices of step 8's long proteins in plong


def expect_proteins(oracle_c, name, min_hits=MIN_HITS, flags=0, lo=0, hi=None):
    """The oracle's (fid, count, status, tally) of proteins [lo, hi) of a batch."""
    key = ("p", name, min_hits, flags, lo, hi)
    if key not in _ORACLE:
        res, off = protein_batch(name)
        off = np.ascontiguousarray(off[lo:None if hi is None else hi + 1])
        fid, cnt, st = oracle_c.apply_mt(oracle_table(oracle_c), res, off, K, min_hits, flags, 4)
        tally = np.bincount(fid[st == 1], minlength=N_FID).astype(np.uint32)
        _ORACLE[key] = (fid, cnt, st, tally)
    return _ORACLE[key]


# ---- genomes ------------------------------------------------------------------------------------
_BASES = np.frombuffer(b"acgt", np.uint8)
_COMP = np.full(256, ord("n"), np.uint8)
for _a, _b in zip(b"acgtACGT", b"tgcaTGCA"):
    _COMP[_a] = _b


def _revcomp(dna):
    """Reverse complement (synth.reverse_complement maps c to a and g to t, so the minus-strand
    genes synth.make_contig_workload plants never hit; the genomes here plant their own)."""
    return _COMP[dna[::-1]]


def _plant(rng, proteins, ids, n_contig, mutation, gap):
    """Contigs of random bases with a coding sequence (random synonymous codons of code 11, a
    stop codon last) of each protein ids[j], mutated per residue, on either strand, dealt round
    robin over the contigs; genes: (contig, start, length) of each."""
    contigs, genes = [[] for _ in range(n_contig)], []
    for j, p in enumerate(ids):
        cds = synth.reverse_translate(rng, _mutate(rng, proteins[int(p)], mutation))
        if rng.random() < 0.5:
            cds = _revcomp(cds)
        c = contigs[j % n_contig]
        c.append(_BASES[rng.integers(0, 4, int(rng.integers(*gap)))])
        genes.append((j % n_contig, sum(len(z) for z in c), len(cds)))
        c.append(cds)
    return [np.concatenate(c + [_BASES[rng.integers(0, 4, 50)]]) for c in contigs], genes


def _pack_dna(contigs):
    off = np.zeros(len(contigs) + 1, np.uint64)
    off[1:] = np.cumsum([len(z) for z in contigs], dtype=np.uint64)
    return np.concatenate(list(contigs) + [np.zeros(64, np.uint8)]), off


@functools.lru_cache(maxsize=None)
def _planted(name):
    """(dna, offsets, genes) of g60 / g300: the table's prototypes at 10% mutation, 'n' bases."""
    rng = np.random.default_rng(SEED + 5 + len(name))
    n_gene, nc, total = (36, 5, 60_000) if name == "g60" else (190, 3, 300_000)
    contigs, genes = _plant(rng, signatures().protos, rng.integers(0, N_FID, n_gene), nc, 0.10,
                            (100, 1200))
    short = total - sum(len(c) for c in contigs)
    if short > 0:
        contigs[-1] = np.concatenate([contigs[-1], _BASES[rng.integers(0, 4, short)]])
    dna, off = _pack_dna(contigs)
    dna[:int(off[-1])][rng.random(int(off[-1])) < 0.0005] = ord("n")
    return dna, off, genes


@functools.lru_cache(maxsize=None)
def genome(name):
    """(dna padded by 64 bytes, offsets) of a named genome.
    g60 / g300 : random contigs with mutated copies of the table's prototypes planted as genes on
                 both strands, and 'n' bases: 5 contigs of 60 kb in all (one emit group), 3 of
                 300 kb (two).
    g40        : 40 bases from inside a planted gene of g60: less than one probe tile.
    none       : no contig at all; empty: three empty contigs.
    g20        : 20 kb in two contigs with 'n', upper case and 'u' / 'U' for t (step 11)."""
    if name in ("g60", "g300"):
        return _planted(name)[:2]
    if name == "g40":
        dna, off, genes = _planted("g60")
        c, start, _ = genes[1]
        at = int(off[c]) + start + 30
        return (np.concatenate([dna[at:at + 40], np.zeros(64, np.uint8)]),
                np.array([0, 40], np.uint64))
    if name == "none":
        return np.zeros(64, np.uint8), np.zeros(1, np.uint64)
    if name == "empty":
        return np.zeros(64, np.uint8), np.zeros(4, np.uint64)
    if name == "g20":
        rng = np.random.default_rng(SEED + 4)
        n = 20_000
        dna = np.frombuffer(b"acgt", np.uint8)[rng.integers(0, 4, n)].copy()
        dna[(dna == ord("t")) & (rng.random(n) < 0.05)] = ord("u")
        dna[rng.random(n) < 0.002] = ord("n")
        dna[rng.random(n) < 0.3] -= 32  # upper case ('N' and 'U' among them)
        return np.concatenate([dna, np.zeros(64, np.uint8)]), np.array([0, 12_001, n], np.uint64)
    raise KeyError(name)


def n_bases(name):
    off = genome(name)[1]
    return int(off[-1] - off[0])


def expect_contigs(oracle_c, name, code=11):
    """The oracle's ((contig, left, strand, frame, fid) arrays, tally[n_contig, N_FID])."""
    key = ("g", name, code)
    if key not in _ORACLE:
        dna, off = genome(name)
        nc = len(off) - 1
        if nc == 0:
            e = (np.zeros(0, np.uint32), np.zeros(0, np.int32), np.zeros(0, np.uint8),
                 np.zeros(0, np.uint8), np.zeros(0, np.uint32))
        else:
            e = oracle_c.annotate_contigs(oracle_table(oracle_c), dna, off, code, K)
        tally = np.zeros((nc, N_FID), np.uint32)
        np.add.at(tally, (e[0], e[4]), 1)
        _ORACLE[key] = (e, tally)
    return _ORACLE[key]


# ---- the host session ---------------------------------------------------------------------------
def _step(name, kind, inp, same_as=None, **kw):
    return types.SimpleNamespace(name=name, kind=kind, inp=inp, same_as=same_as, **kw)


def _p(name, inp, same_as=None, flags=0, min_hits=MIN_HITS, opts=None, bad_offsets=False):
    o = dict(opts or {})
    if inp == "p1500":
        o.setdefault("host_piece_min", PIECE_MIN)
    return _step(name, "proteins", inp, same_as, flags=flags, min_hits=min_hits, opts=o,
                 bad_offsets=bad_offsets)


def _c(name, inp, same_as=None, code=11, opts=None):
    return _step(name, "contigs", inp, same_as, code=code, opts=dict(opts or {}))


def host_steps():
    """The ordered steps of the host session. kind: 'proteins' / 'contigs' (the Python wrapper;
    all of fid, count, status, tally / of the hits, the total, the tally compared),
    'proteins_fail' / 'contigs_fail' (KMA_E_INVALID expected), 'contigs_abi' (the C ABI through
    ctypes: cap relative to the needed count, a prefilled hit buffer and tally). same_as: an earlier step with the same input, whose output
    this one must also equal. opts: library options set for this call alone."""
    s = [_p("1", "p13"),
         _c("2", "g60"),
         _p("3", "p1500"),
         _c("4-40", "g40"), _c("4-none", "none"), _c("4-empty", "empty"),
         _c("5-300k", "g300"), _c("5-again", "g60", "2"),
         _step("6-short", "contigs_abi", "g60", cap=-1),   # needed - 1: KMA_E_CAPACITY
         _step("6-fits", "contigs_abi", "g60", cap=0),     # needed
         _step("6-null", "contigs_abi", "g60", cap=None)]  # out_hits = NULL
    for tag, kw in (("minhits0", dict(min_hits=0)), ("offsets", dict(bad_offsets=True)),
                    ("flagbit", dict(flags=4))):
        f = _p("7-" + tag, "p13", **kw)
        f.kind = "proteins_fail"
        s += [f, _p("7-after-" + tag, "p13", "1")]
    s += [_p("8", "plong", opts=dict(block_proteins=6)),
          _p("8-p13", "p13", "1"), _p("8-p1500", "p1500", "3")]
    for i, fl in enumerate((0, F_MULTISET, F_END_EXCLUSIVE, F_MULTISET | F_END_EXCLUSIVE, 0)):
        s.append(_p(f"9-{i}-flags{fl}", "p1500", "3" if fl == 0 else None, flags=fl))
    for i, mode in enumerate((1, 0, 2, 1)):
        s.append(_p(f"10-{i}-packed{mode}", "p1500", "3", opts=dict(packed_input=mode)))
        if i < 3:
            s.append(_c(f"10-{i}-g60", "g60", "2"))
    for code in ALL_CODES:
        s.append(_c(f"11-code{code}", "g20", "11-code1" if code == 11 else None, code=code))
    bad = _c("11-code7", "g20", code=7)
    bad.kind = "contigs_fail"
    s += [bad, _c("11-after", "g20", "11-code11", code=11)]
    return s


# ---- the peg session ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def peg_case():
    """About 300 pegs (prototype proteins, an empty one, one shorter than K and one with an 'X'
    run) and two genomes: A (three contigs with 60 of the pegs planted at 5% mutation on either
    strand, and a fourth contig of segments copied from inside those genes: 27 = 3K + 3, 60, 90,
    200 and 400 bases, one of them reverse complemented, so that their kmers have two locations
    and the strict join drops both) and B (two contigs, 20 other pegs, no copies)."""
    rng = np.random.default_rng(SEED + 6)
    protos = synth.make_table(1, 297, SEED + 7, K, protos_only=True).protos
    x = protos[5].copy()
    x[40:43] = ord("X")
    pegs = list(protos[:5]) + [x] + list(protos[6:]) + [np.zeros(0, np.uint8), protos[0][:7],
                                                       protos[1][:9]]
    ca, genes = _plant(rng, protos, range(60), 3, 0.05, (30, 400))
    dups = []
    for (c, at, n), seg in zip([g for g in genes if g[2] > 600][:5], (27, 60, 90, 200, 400)):
        piece = ca[c][at + 60:at + 60 + seg]
        dups += [_revcomp(piece) if seg == 90 else piece, _BASES[rng.integers(0, 4, 50)]]
    ca.append(np.concatenate(dups))
    cb, _ = _plant(rng, protos, range(60, 80), 2, 0.05, (30, 400))

    res, off = _pack(pegs)
    return types.SimpleNamespace(residues=res, offsets=off, n_peg=len(pegs),
                                 genomes={"A": _pack_dna(ca), "B": _pack_dna(cb)})


PEG_STEPS = (("A", True), ("A", True), ("A", False), ("B", True), ("A", True), ("B", False))


def expect_pegs(oracle_c, g, strict):
    """The oracle's (contig, left, strand, frame, peg) connections of genome g."""
    key = ("peg", g, strict)
    if key not in _ORACLE:
        pc = peg_case()
        _ORACLE[key] = oracle_c.peg_connect(pc.residues, pc.offsets, *pc.genomes[g], 11, K, strict)
    return _ORACLE[key]


# ---- the device session -------------------------------------------------------------------------
def device_steps():
    """The ordered calls of the device session (one workspace, one stream). Protein steps: the
    proteins [lo, hi) of a batch (lo > 0: d_offsets[0] is nonzero), entry 'ascii' or 'packed' (a
    stream of kma_pack_residues); ws_opts: workspace options set before the call. Contig steps:
    lead bytes before the genome in its device buffer (d_offsets[0] = lead), cap (None: the
    total; an int below it: only that many records are written). 'reserve' / 'reserve_contigs'
    grow the workspace; 'over' passes n_bases above the reservation (KMA_E_CAPACITY)."""
    P, C = "proteins", "contigs"
    return [
        _step("1", P, "p200", lo=3, hi=200, entry="ascii", ws_opts=None),
        _step("2", C, "g60", lead=5, cap=None),
        _step("3", P, "p200", lo=40, hi=200, entry="packed", ws_opts=None),
        _step("4", C, "g60", lead=0, cap=100),
        _step("5", C, "g60", lead=0, cap=None),
        _step("6-bp1-defer2", P, "p200", lo=0, hi=200, entry="ascii",
              ws_opts=dict(block_proteins=1, defer=2)),
        _step("6-defaults", P, "p200", lo=0, hi=200, entry="ascii",
              ws_opts=dict(block_proteins=None, defer=None)),
        _step("7-reserve", "reserve", "pbig"),
        _step("7", P, "pbig", lo=0, hi=3000, entry="ascii", ws_opts=None),
        _step("8-reserve", "reserve_contigs", "g300"),
        _step("8-300k", C, "g300", lead=0, cap=None),
        _step("8-40", C, "g40", lead=0, cap=None),
        _step("9-over", "over", "g300"),
        _step("9-after", C, "g60", lead=5, cap=None),
    ]
