"""Edge and scale parity of the four sort-and-scan operators: kma_protein_distances /
kma_protein_best_match, kma_hash_annotate, kma_build_signatures and kma_propose_pegs against
the C oracle, bit-exact (integers, and doubles by ==), with the Python twins of oracle_py on the
small cases.

One generator (shared_input) feeds all four: the full alphabet A-Z and '*', windows that start
and end with '*' and 'Z' (the top and bottom five key bits), lengths aimed at K and at the
64-lane stride of the wave-per-protein kernels, a 40,000-residue protein for the segmented
sort's long-segment path, empty proteins first, last and adjacent, and the same batch passed as
a view with offsets[0] = 37. The scale cases cross each launcher's grid cap, so that every
grid-stride loop takes a second trip. tests/test_set_ops_workload.py shows on the oracle alone
that each case meets the condition it is built for."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

from helpers import take_proteins
from oracle import oracle_py

pytestmark = pytest.mark.gpu

SYMS = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZ*", np.uint8)
NEXT_SYM = np.zeros(256, np.uint8)
NEXT_SYM[SYMS] = np.roll(SYMS, -1)
BASE = 37  # offsets[0] of the nonzero-base calls
E_INVALID, E_CAPACITY = -1, -4
HASH_MIN_SIMS = (0.0, 0.0125, 0.5, float(np.nextafter(1.0, 0.0)))
PROPOSAL_PARAMS = {"defaults": dict(), "strength0.2": dict(min_strength=0.2),
                   "loose": dict(min_strength=0.05, max_fuzz=2.5, min_fuzz=0.3)}
PROP_FIELDS = ("peg", "contig", "strand", "left", "right", "evidence", "frame")


@pytest.fixture(scope="module")
def kma(native_lib):
    import kmeranno
    assert kmeranno.device_count() >= 1
    return kmeranno


# ---- shared inputs -----------------------------------------------------------------------------
def rand_prot(rng, n):
    return SYMS[rng.integers(0, 27, int(n))].tobytes()


def mutate(p, every, start=0):
    """p with the residues at start, start + every, ... replaced by the alphabet's next symbol
    ('Z' -> '*' -> 'A')."""
    b = np.frombuffer(p, np.uint8).copy()
    pos = np.arange(start, len(b), every)
    b[pos] = NEXT_SYM[b[pos]]
    return b.tobytes()


def pack(prots, base=0):
    """(residues padded by 32 bytes, offsets) of byte strings. base > 0: the batch as a view into
    a larger buffer (offsets[0] = base, other residues before and after it)."""
    off = np.zeros(len(prots) + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for p in prots], dtype=np.uint64)
    buf = b"W" * base + b"".join(prots) + b"W" * base + b"\0" * 32
    return np.frombuffer(buf, np.uint8).copy(), off + np.uint64(base)


def shared_lengths(k):
    return [0, 1, k - 1, k, k + 1, 63, 64, 65, 64 + k - 2, 64 + k - 1, 64 + k, 127, 128, 129]


@functools.lru_cache(maxsize=None)
def shared_input(k):
    """The proteins every operator is run on at kmer size k.
    prots: two empty proteins; per length of shared_lengths a random full-alphabet protein and
    its relative (every 4k-th residue changed, from the first: 0 < similarity < 1 where the
    length allows); two empty proteins; three pairs that differ by '*' against 'Z' at the first,
    the last and an inner position; an all-'A' window inside a protein and alone; one letter x
    200; a 40,000-residue protein and its relative; an empty protein.
    rel / star_z: index pairs; by_len: length -> index of the random protein; small: the indices
    without the two long proteins; roles: per protein a role >= 0, -1 (buffered) or -2 (skipped)
    for the signature build (relatives in the same role, another role, buffered, skipped)."""
    rng = np.random.default_rng(7100 + k)
    prots, rel, by_len = [b"", b""], [], {}
    for n in shared_lengths(k):
        p = rand_prot(rng, n)
        by_len[n] = len(prots)
        rel.append((len(prots), len(prots) + 1))
        prots += [p, mutate(p, 4 * k)]
    prots += [b"", b""]
    core = rand_prot(rng, 30 + k)
    h = k + 3
    star_z = []
    for a, b in ((b"*" + core, b"Z" + core), (core + b"*", core + b"Z"),
                 (core[:h] + b"*" + core[h:], core[:h] + b"Z" + core[h:])):
        star_z.append((len(prots), len(prots) + 1))
        prots += [a, b]
    prots += [core[:5] + b"A" * k + core[5:], b"A" * k, b"Q" * 200]
    small = list(range(len(prots))) + [len(prots) + 2]
    long_p = rand_prot(rng, 40_000)
    rel.append((len(prots), len(prots) + 1))
    prots += [long_p, mutate(long_p, 4 * k), b""]
    roles = [i % 5 for i in range(len(prots))]
    for j, (a, b) in enumerate(rel):
        roles[b] = (roles[a], (roles[a] + 1) % 5, -1, -2)[j % 4]
    for j, (a, b) in enumerate(star_z):
        roles[b] = (roles[a], (roles[a] + 1) % 5, -1)[j]
    return types.SimpleNamespace(prots=prots, rel=rel, star_z=star_z, by_len=by_len, small=small,
                                 roles=roles, long=(len(prots) - 3, len(prots) - 2))


def batch_shapes(k):
    """Batches of 1, 2, 3, 5 and 7 proteins (an empty protein first, last, two adjacent), a batch
    of only empty proteins and one in which no protein reaches k."""
    si = shared_input(k)
    p = si.prots
    g = si.by_len
    return [[p[g[65]]], [b"", p[g[64]]], [p[g[k + 1]], p[g[63]], b""],
            [p[g[64]], b"", b"", p[g[65]], p[g[k]]],
            [p[g[63]], p[g[63] + 1], p[g[64]], p[g[64] + 1], b"", p[g[65]], p[g[65] + 1]],
            [b"", b"", b""], [b"", b"A" * (k - 1), p[g[65]][:k - 1]]]


def shared_pairs(k):
    """Pairs over shared_input(k): every (i, i), each relative and each '*' / 'Z' pair both ways,
    200 random pairs, and the two leading empty proteins."""
    si = shared_input(k)
    n = len(si.prots)
    rng = np.random.default_rng(7200 + k)
    both = np.array(si.rel + si.star_z)
    pa = np.concatenate([np.arange(n), both[:, 0], both[:, 1], rng.integers(0, n, 200), [0, 1]])
    pb = np.concatenate([np.arange(n), both[:, 1], both[:, 0], rng.integers(0, n, 200), [1, 0]])
    return pa.astype(np.uint32), pb.astype(np.uint32)


# ---- distances and best match -------------------------------------------------------------------
def check_distances(kma, oracle_c, res, off, pa, pb, k, flags):
    sim, size, dist = kma.protein_distances(res, off, pa, pb, k, flags)
    esim, esa, esb, edist = oracle_c.protein_distances(res, off, pa, pb, k, flags)
    assert (sim == esim).all() and (dist == edist).all()
    assert (size[pa] == esa).all() and (size[pb] == esb).all()
    return sim, size, dist


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("k", range(2, 13))
def test_distances_shared_inputs(kma, oracle_c, k, flags):
    si = shared_input(k)
    pa, pb = shared_pairs(k)
    res, off = pack(si.prots)
    sim, size, dist = check_distances(kma, oracle_c, res, off, pa, pb, k, flags)
    # the same batch as a view at offsets[0] = 37
    res37, off37 = pack(si.prots, BASE)
    for got, ref in zip(check_distances(kma, oracle_c, res37, off37, pa, pb, k, flags),
                        (sim, size, dist)):
        assert (got == ref).all()
    # no pairs, sizes requested; pair counts 1, 2 and 3 (mod 4)
    s0, z0, d0 = kma.protein_distances(res, off, [], [], k, flags)
    assert len(s0) == 0 and len(d0) == 0 and (z0 == size).all()
    n = len(si.prots)
    for m in (5, 6, 7, 1):  # from the relatives on
        sm, zm, dm = check_distances(kma, oracle_c, res, off, pa[n:n + m], pb[n:n + m], k, flags)
        assert (sm == sim[n:n + m]).all() and (zm == size).all() and (dm == dist[n:n + m]).all()
    # batch shapes: every pair of each small batch
    for batch in batch_shapes(k):
        n = len(batch)
        qa, qb = np.repeat(np.arange(n), n), np.tile(np.arange(n), n)
        for base in (0, BASE):
            check_distances(kma, oracle_c, *pack(batch, base), qa.astype(np.uint32),
                            qb.astype(np.uint32), k, flags)
    # the Python twin (strings and sets: no 5-bit packing) on the pairs without a long protein
    small = set(si.small)
    for i, (a, b) in enumerate(zip(pa.tolist(), pb.tolist())):
        if a in small and b in small:
            d = oracle_py.distance(si.prots[a].decode(), si.prots[b].decode(), k, flags == 1)
            assert d == dist[i], (a, b)


@pytest.mark.parametrize("k", [1, 13])
def test_distances_refuse_k(kma, k):
    res, off = pack([b"ACDEFGHIKLMNPQRSTVWY", b"ACDEFGHIKLMNPQRSTVWY"])
    with pytest.raises(kma.KmerAnnoError) as e:
        kma.protein_distances(res, off, [0], [1], k)
    assert e.value.code == E_INVALID
    with pytest.raises(kma.KmerAnnoError) as e:
        kma.protein_best_match(res, off, [0], [0, 1], [1], 0.5, k)
    assert e.value.code == E_INVALID


@functools.lru_cache(maxsize=None)
def distance_scale_case():
    """70,001 proteins of 0..23 residues and 70,003 pairs at K = 2 (both above the 65,536 the
    wave-per-item grids cover in one trip); the last 10 pairs are (i, i) of the last proteins."""
    rng = np.random.default_rng(41)
    n = 70_001
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(rng.integers(0, 24, n))
    res = np.concatenate([SYMS[rng.integers(0, 27, int(off[-1]))], np.zeros(32, np.uint8)])
    last = np.arange(n - 10, n)
    pa = np.concatenate([rng.integers(0, n, 69_993), last]).astype(np.uint32)
    pb = np.concatenate([rng.integers(0, n, 69_993), last]).astype(np.uint32)
    return res, off, pa, pb


def test_distances_scale(kma, oracle_c):
    res, off, pa, pb = distance_scale_case()
    sim, size, dist = check_distances(kma, oracle_c, res, off, pa, pb, 2, 0)
    assert (sim > 0).mean() > 0.10
    assert (dist[-10:][size[pa[-10:]] > 0] == 0.0).all()


def java_best(edist, cand, cand_off, max_dist):
    """GeneCopyProcessor.java:135-146 over the oracle's distances (edist[i] of cand[i])."""
    best, bd = [], []
    for q in range(len(cand_off) - 1):
        fdist, found = max_dist, -1
        for i in range(int(cand_off[q]), int(cand_off[q + 1])):
            if edist[i] <= fdist:
                fdist, found = edist[i], int(cand[i])
        best.append(found)
        bd.append(fdist)
    return np.array(best, np.int32), np.array(bd, np.float64)


def best_match_case(k):
    """shared_input(k) twice over (so that each protein has an identical later copy) as the
    proteins; every protein of the first half is a query. Candidates, in order: its copy, its
    relative or '*' / 'Z' partner, three random proteins, itself, one random protein. The first,
    the middle and the last query have no candidates."""
    si = shared_input(k)
    n = len(si.prots)
    rng = np.random.default_rng(7400 + k)
    partner = {}
    for a, b in si.rel + si.star_z:
        partner[a], partner[b] = b, a
    cands = []
    for q in range(n):
        r = rng.integers(0, 2 * n, 4).tolist()
        cands.append([] if q in (0, n // 2, n - 1) else
                     [q + n] + ([partner[q]] if q in partner else []) + r[:3] + [q, r[3]])
    cand_off = np.zeros(n + 1, np.uint64)
    cand_off[1:] = np.cumsum([len(c) for c in cands])
    cand = np.array([x for c in cands for x in c], np.uint32)
    return si.prots + si.prots, np.arange(n, dtype=np.uint32), cand_off, cand, cands


@pytest.mark.parametrize("max_dist", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("k", [2, 3, 8, 12])
def test_best_match_shared_inputs(kma, oracle_c, k, max_dist):
    prots, query, cand_off, cand, cands = best_match_case(k)
    res, off = pack(prots)
    pa = np.repeat(query, np.diff(cand_off).astype(np.int64))
    edist = oracle_c.protein_distances(res, off, pa, cand, k, 0)[3]
    ebest, ebd = java_best(edist, cand, cand_off, max_dist)
    best, bd = kma.protein_best_match(res, off, query, cand_off, cand, max_dist, k)
    assert (best == ebest).all() and (bd == ebd).all()
    # cand_off[0] != 0 and offsets[0] != 0
    res37, off37 = pack(prots, BASE)
    best, bd = kma.protein_best_match(res37, off37, query, cand_off + np.uint64(3),
                                      np.concatenate([[7, 7, 7], cand]).astype(np.uint32),
                                      max_dist, k)
    assert (best == ebest).all() and (bd == ebd).all()
    # no queries
    best, bd = kma.protein_best_match(res, off, [], [0], [], max_dist, k)
    assert len(best) == 0 and len(bd) == 0
    # the Python twin on the queries without a long protein among the candidates
    n = len(query)
    for q in range(n):
        if cands[q] and all(c % n in shared_input(k).small for c in cands[q] + [q]):
            f, d = oracle_py.best_match(prots[q].decode(), [prots[c].decode() for c in cands[q]],
                                        max_dist, k)
            assert ebest[q] == (cands[q][f] if f >= 0 else -1) and ebd[q] == d


BEST_EDGE_PROTS = [b"ACD", b"ACDE", b"WWWW", b"ACD", b"", b"AAAA", b"AAAAAA"]
# (query, candidates, max_dist, best, its distance) at K = 3
BEST_EDGE_CASES = [
    (0, [1], 0.5, 1, 0.5),        # one shared kmer, union of two: exactly max_dist, kept
    (0, [2, 4], 1.0, 4, 1.0),     # nothing shared: distance 1.0 <= 1.0, the last one wins
    (0, [3, 1, 2], 1.0, 3, 0.0),  # ... but not after a closer one
    (5, [1, 6, 0], 0.0, 6, 0.0),  # max_dist 0: only the identical set {AAA}
    (0, [1, 2], 0.0, -1, 0.0),    # max_dist 0 and no identical set
    (1, [3, 0], 0.5, 0, 0.5),     # equal distances: the last of them
    (1, [0, 3], 0.5, 3, 0.5),
]


def test_best_match_edges(kma, oracle_c):
    res, off = pack(BEST_EDGE_PROTS)
    strs = [p.decode() for p in BEST_EDGE_PROTS]
    for q, cands, max_dist, want, want_d in BEST_EDGE_CASES:
        cand_off = np.array([0, len(cands)], np.uint64)
        best, bd = kma.protein_best_match(res, off, [q], cand_off, cands, max_dist, 3)
        assert (int(best[0]), float(bd[0])) == (want, want_d), (q, cands, max_dist)
        f, d = oracle_py.best_match(strs[q], [strs[c] for c in cands], max_dist, 3)
        assert (cands[f] if f >= 0 else -1, d) == (want, want_d)
        edist = oracle_c.protein_distances(res, off, [q] * len(cands), cands, 3, 0)[3]
        ebest, ebd = java_best(edist, cands, cand_off, max_dist)
        assert (int(ebest[0]), float(ebd[0])) == (want, want_d)


# ---- hash annotator ------------------------------------------------------------------------------
def check_hash(kma, oracle_c, genome, protos, k, min_sim, base=0, twin=False):
    """genome / protos: lists of byte strings, or (residues, offsets)."""
    g, go = pack(genome, base) if isinstance(genome, list) else genome
    p, po = pack(protos, base) if isinstance(protos, list) else protos
    got = kma.hash_annotate(g, go, p, po, k, min_sim)
    exp = oracle_c.hash_annotate(g, go, p, po, k, min_sim)
    for a, b in zip(got, exp):
        assert (a == b).all()
    if twin:
        pb, ps, pc = oracle_py.hash_annotate([x.decode() for x in genome],
                                             [x.decode() for x in protos], k, min_sim)
        assert exp[0].tolist() == pb and exp[1].tolist() == ps and exp[2].tolist() == pc
    return got


@functools.lru_cache(maxsize=None)
def hash_shared_case(k):
    """Genome: shared_input(k). Prototypes: an empty one, a mutated copy of every genome protein
    that reaches k, an empty one and one of k - 1 residues in the middle, exact copies (one of
    them twice: the earlier wins), an empty one."""
    si = shared_input(k)
    protos = [mutate(p, 3 * k + i % 5, i % (k + 1)) for i, p in enumerate(si.prots)
              if len(p) >= k]
    mid = len(protos) // 2
    copies = [si.prots[si.by_len[65]], si.prots[si.by_len[129]], si.prots[si.star_z[0][0]],
              si.prots[si.by_len[65]]]
    protos = [b""] + protos[:mid] + [b"", b"A" * (k - 1)] + protos[mid:] + copies + [b""]
    return si.prots, protos


@pytest.mark.parametrize("min_sim", HASH_MIN_SIMS, ids=["0", "0.0125", "0.5", "below1"])
@pytest.mark.parametrize("k", range(2, 13))
def test_hash_shared_inputs(kma, oracle_c, k, min_sim):
    genome, protos = hash_shared_case(k)
    ref = check_hash(kma, oracle_c, genome, protos, k, min_sim)
    got = check_hash(kma, oracle_c, genome, protos, k, min_sim, base=BASE)
    for a, b in zip(got, ref):
        assert (a == b).all()
    si = shared_input(k)
    small_g = [genome[i] for i in si.small]
    small_p = [p for p in protos if len(p) < 1000]
    check_hash(kma, oracle_c, small_g, small_p, k, min_sim, twin=True)
    # batch shapes on either side
    for batch in batch_shapes(k):
        check_hash(kma, oracle_c, batch, [mutate(p, 3 * k, 1) for p in batch] + batch[:1], k,
                   min_sim, twin=True)
        check_hash(kma, oracle_c, batch, small_p, k, min_sim)
        check_hash(kma, oracle_c, small_g, batch, k, min_sim, base=BASE)


def hash_tie_case(order):
    """K = 3: ACDE shares one of three kmers with ACDW (1/3) and two of six with ACDEFGHI (2/6):
    equal doubles from different fractions."""
    protos = [b"ACDW", b"ACDEFGHI"]
    return [b"ACDE"], protos if order == 0 else protos[::-1]


@pytest.mark.parametrize("slice_cand", [0, 1])
@pytest.mark.parametrize("order", [0, 1])
def test_hash_tie_of_equal_doubles(kma, oracle_c, order, slice_cand):
    genome, protos = hash_tie_case(order)
    third = 1.0 / 3.0
    assert third == 2.0 / 6.0
    kma.set_option(kma.OPT_HASH_SLICE, slice_cand)
    for min_sim in (0.0, 0.0125, third):  # the threshold is inclusive
        best, sim, cnt = check_hash(kma, oracle_c, genome, protos, 3, min_sim, twin=True)
        assert best.tolist() == [0] and sim.tolist() == [third] and cnt.tolist() == [1, 1]
    # every similarity below min_sim
    best, sim, cnt = check_hash(kma, oracle_c, genome, protos, 3,
                                float(np.nextafter(third, 1.0)), twin=True)
    assert best.tolist() == [-1] and sim.tolist() == [0.0] and cnt.tolist() == [0, 0]


def test_hash_thresholds_and_disjoint(kma, oracle_c):
    best, sim, cnt = check_hash(kma, oracle_c, [b"ACD"], [b"ACDE"], 3, 0.5, twin=True)
    assert best.tolist() == [0] and sim.tolist() == [0.5] and cnt.tolist() == [1]
    best, sim, cnt = check_hash(kma, oracle_c, [b"ACD"], [b"ACDE"], 3,
                                float(np.nextafter(0.5, 1.0)), twin=True)
    assert best.tolist() == [-1] and sim.tolist() == [0.0] and cnt.tolist() == [0]
    rng = np.random.default_rng(5)
    lo, hi = np.frombuffer(b"ACDEFGHIKL", np.uint8), np.frombuffer(b"MNPQRSTVWY", np.uint8)
    genome = [lo[rng.integers(0, 10, 40)].tobytes() for _ in range(9)]
    protos = [hi[rng.integers(0, 10, 40)].tobytes() for _ in range(7)]
    best, sim, cnt = check_hash(kma, oracle_c, genome, protos, 3, 0.0, twin=True)
    assert (best == -1).all() and (sim == 0.0).all() and (cnt == 0).all()


HASH_EMPTY_GENOME = [b"", b"ACDEFGHIK", b"AC", b"ACDEFW", b"FGHIKLMN", b""]
HASH_EMPTY_PROTOS = [b"", b"ACDEFG", b"GHIKLM", b"", b"ACDEFGHIK", b"AC", b"FGHIK", b""]


def cand_counts(genome, protos, k):
    """Candidates (shared distinct kmers summed over the genome proteins) per prototype."""
    def kset(p):
        return {p[i:i + k] for i in range(len(p) - k + 1)}
    gs = [kset(g) for g in genome]
    return [sum(len(kset(p) & g) for g in gs) for p in protos]


@pytest.mark.parametrize("slicing", ["one", "each", "after_empty"])
def test_hash_empty_and_short_prototypes(kma, oracle_c, slicing):
    """Prototypes and genome proteins that are empty or shorter than K first, in the middle and
    last, in one slice, in slices of one candidate (slices without candidates) and with a slice
    size that ends a slice right after the empty prototype 3."""
    cc = cand_counts(HASH_EMPTY_GENOME, HASH_EMPTY_PROTOS, 3)
    kma.set_option(kma.OPT_HASH_SLICE, {"one": 0, "each": 1, "after_empty": sum(cc[:4])}[slicing])
    for min_sim in (0.0, 0.3, 0.5):
        best, sim, cnt = check_hash(kma, oracle_c, HASH_EMPTY_GENOME, HASH_EMPTY_PROTOS, 3,
                                    min_sim, twin=True)
    # at 0.5: FGHIK against FGHIKLMN is 3 / 6, on the threshold
    assert best.tolist() == [-1, 4, -1, 1, 2, -1] and cnt.tolist() == [0, 2, 1, 0, 1, 0, 1, 0]
    for base in (0, BASE):  # no prototype, or no genome protein, reaches K
        short = [b"", b"AC", b"A"]
        for g, p in ((HASH_EMPTY_GENOME, short), (short, HASH_EMPTY_PROTOS), (short, short)):
            best, sim, cnt = check_hash(kma, oracle_c, g, p, 3, 0.0, base=base, twin=True)
            assert (best == -1).all() and (cnt == 0).all()


def hash_count_case(n_pt):
    """K = 3: 40 genome proteins; n_pt prototypes, mutated copies of them, the last one an exact
    copy of genome protein 0 (the prototype index with the top bit of the sort key set)."""
    rng = np.random.default_rng(53)
    genome = [rand_prot(rng, rng.integers(20, 60)) for _ in range(40)]
    pool = [mutate(genome[i % 40], 5 + i // 40, i % 5) for i in range(n_pt)]
    return genome, pool[:-1] + [genome[0]]


@pytest.mark.parametrize("n_pt", [1, 2, 3, 4, 5, 256, 257])
def test_hash_prototype_counts(kma, oracle_c, n_pt):
    genome, protos = hash_count_case(n_pt)
    for slice_cand in (0, 40):
        kma.set_option(kma.OPT_HASH_SLICE, slice_cand)
        best, sim, cnt = check_hash(kma, oracle_c, genome, protos, 3, 0.0125, twin=n_pt < 10)
        assert best[0] == n_pt - 1 and sim[0] == 1.0 and cnt[-1] >= 1


def hash_shared_sets_case():
    """K = 5: 500 identical genome proteins and 40 variants (long protein ranges per key)."""
    rng = np.random.default_rng(59)
    p = rand_prot(rng, 120)
    genome = [p] * 500 + [mutate(p, 6 + j, j % 6) for j in range(40)]
    protos = [mutate(p, 7), rand_prot(rng, 90), p, mutate(p, 9, 3), p, b""]
    return genome, protos


def test_hash_shared_sets(kma, oracle_c):
    genome, protos = hash_shared_sets_case()
    for slice_cand in (0, 5000):
        kma.set_option(kma.OPT_HASH_SLICE, slice_cand)
        best, sim, cnt = check_hash(kma, oracle_c, genome, protos, 5, 0.0125)
        assert (best[:500] == 2).all() and (sim[:500] == 1.0).all() and cnt[2] == cnt[4] >= 500


def random_batch(rng, lens):
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    return np.concatenate([SYMS[rng.integers(0, 27, int(off[-1]))], np.zeros(32, np.uint8)]), off


@functools.lru_cache(maxsize=None)
def hash_scale_case(name):
    """(genome, prototypes, K, min_sim), each side as (residues, offsets):
    runs       1,500 x 1,500 proteins of 40..79 residues at K = 2: above 2,097,152 (prototype,
               protein) runs (score, choose)
    positions  30,000 prototypes (20%-mutated copies of the genome) x 50 genome proteins of
               50..99 residues at K = 4: above 2,097,152 prototype positions (cand_count,
               cand_emit, proto_cum's input)
    pairs      the same two swapped: above 2,097,152 genome (key, protein) pairs (run_heads)
    proteins   2,200,001 genome proteins of 6..12 residues cut from 36 12-mers x 6 prototypes at
               K = 8 (merge_best and the wave-per-protein kernels)
    prototypes the same two swapped: above 2,097,152 prototypes (proto_cum)"""
    rng = np.random.default_rng(61)
    if name == "runs":
        return (random_batch(rng, rng.integers(40, 80, 1500)),
                random_batch(rng, rng.integers(40, 80, 1500)), 2, 0.0)
    if name in ("positions", "pairs"):
        g = random_batch(rng, rng.integers(50, 100, 50))
        pres, poff = take_proteins(g[0], g[1], np.arange(30_000) % 50)
        m = rng.random(len(pres) - 32) < 0.2
        pres[:-32][m] = SYMS[rng.integers(0, 27, int(m.sum()))]
        return (g, (pres, poff), 4, 0.0125) if name == "positions" else ((pres, poff), g, 4, 0.0125)
    if name == "prototypes":
        g, p, k, min_sim = hash_scale_case("proteins")
        return p, g, k, min_sim
    n = 2_200_001
    pool = SYMS[rng.integers(0, 27, (36, 12))]
    lens = rng.integers(6, 13, n)
    start = (rng.random(n) * (13 - lens)).astype(np.int64)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    src = np.repeat(rng.integers(0, 36, n) * 12 + start - off[:-1].astype(np.int64), lens)
    src += np.arange(int(off[-1]))
    gres = np.concatenate([pool.ravel()[src], np.zeros(32, np.uint8)])
    protos = [pool[2 * i].tobytes() + pool[2 * i + 1].tobytes() for i in range(5)]
    return (gres, off), pack(protos + [mutate(pool[20].tobytes(), 11, 10)]), 8, 0.0125


HASH_SCALE_CASES = ["runs", "positions", "pairs", "proteins", "prototypes"]


@pytest.mark.parametrize("name", HASH_SCALE_CASES)
def test_hash_scale(kma, oracle_c, name):
    genome, protos, k, min_sim = hash_scale_case(name)
    best, sim, cnt = check_hash(kma, oracle_c, genome, protos, k, min_sim)
    assert (best >= 0).sum() >= 6 and cnt.sum() > 1000


# ---- signature build -----------------------------------------------------------------------------
def check_build(kma, oracle_c, res, off, roles, k, flags=0):
    """Rows equal the oracle's as a set; keys strictly increase. Returns {packed key: role}."""
    keys, groles = kma.build_signatures(res, off, roles, k, flags)
    km, rl = oracle_c.build_signatures(res, off, roles, k, flags)
    ekeys = kma.pack_std(km)
    order = np.argsort(ekeys)
    assert (keys[1:] > keys[:-1]).all()
    assert len(keys) == len(ekeys) and (keys == ekeys[order]).all()
    assert (groles.astype(np.int64) == rl[order]).all()
    return keys, groles


def key_of(kma, kmer):
    return int(kma.pack_std(np.frombuffer(kmer, np.uint8)[None, :])[0])


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("k", range(1, 13))
def test_build_shared_inputs(kma, oracle_c, k, flags):
    si = shared_input(k)
    keys, roles = check_build(kma, oracle_c, *pack(si.prots), si.roles, k, flags)
    k37, r37 = check_build(kma, oracle_c, *pack(si.prots, BASE), si.roles, k, flags)
    assert (k37 == keys).all() and (r37 == roles).all()
    for batch in batch_shapes(k):
        for base in (0, BASE):
            check_build(kma, oracle_c, *pack(batch, base), list(range(len(batch))), k, flags)
    # the Python twin on the proteins without the long ones
    small = [si.prots[i] for i in si.small]
    sroles = [si.roles[i] for i in si.small]
    keys, roles = check_build(kma, oracle_c, *pack(small), sroles, k, flags)
    twin = oracle_py.build_signatures([p.decode() for p in small], sroles, k, flags == 1)
    assert {key_of(kma, km.encode()): r for km, r in twin.items()} == \
        dict(zip(keys.tolist(), roles.tolist()))


# K = 1, flags 0 and no skipped protein: every position is a window, so a real key ('A') sits at
# sorted index 0, whose head index equals the "no head" value of the max-scan.
BUILD_K1_PROTS = [b"AB", b"AC", b"BD", b"A"]
BUILD_K1_CASES = [([0, 0, 1, 0], {"A": 0, "C": 0, "D": 1}),   # A kept, B counted for two roles
                  ([0, 1, 1, 0], {"C": 1, "D": 1}),           # A counted for two roles
                  ([0, 0, 1, -1], {"C": 0, "D": 1})]          # A removed by a buffered protein


@pytest.mark.parametrize("case", range(len(BUILD_K1_CASES)))
def test_build_k1_key_at_sorted_index_0(kma, oracle_c, case):
    roles, want = BUILD_K1_CASES[case]
    keys, groles = check_build(kma, oracle_c, *pack(BUILD_K1_PROTS), roles, 1, 0)
    assert dict(zip(keys.tolist(), groles.tolist())) == \
        {key_of(kma, km.encode()): r for km, r in want.items()}


LONG_RUN_KMER = b"MKV*LZGH"
LONG_RUN_VARIANTS = {"as_is": (None, True), "other_role_first": (4, False),
                     "other_role_last": (4, False), "buffered": (-1, False), "skipped": (-2, True)}


@functools.lru_cache(maxsize=None)
def long_run_case(variant):
    """K = 8: 70,000 proteins of role 3, each the shared 8-mer followed by 8..12 random
    residues (one key run across many scan blocks; above the 32,768 proteins that
    build_windows covers in one trip), and one more protein holding the 8-mer whose role is
    the variant's. Returns (residues, offsets, roles, whether the 8-mer stays a signature)."""
    rng = np.random.default_rng(67)
    n = 70_000
    lens = 8 + rng.integers(8, 13, n)
    role, kept = LONG_RUN_VARIANTS[variant]
    roles = np.full(n, 3, np.int32)
    if role is not None:
        at = 0 if variant == "other_role_first" else n
        lens = np.insert(lens, at, 16)
        roles = np.insert(roles, at, role)
    res, off = random_batch(rng, lens)
    head = off[:-1].astype(np.int64)[:, None] + np.arange(8)
    res[head] = np.frombuffer(LONG_RUN_KMER, np.uint8)
    return res, off, roles, kept


@pytest.mark.parametrize("variant", list(LONG_RUN_VARIANTS))
def test_build_long_run(kma, oracle_c, variant):
    res, off, roles, kept = long_run_case(variant)
    keys, groles = check_build(kma, oracle_c, res, off, roles, 8)
    at = np.searchsorted(keys, key_of(kma, LONG_RUN_KMER))
    found = at < len(keys) and keys[at] == key_of(kma, LONG_RUN_KMER)
    assert found == kept and (not kept or groles[at] == 3)
    assert len(keys) > 500_000


# ---- proposal sweep ------------------------------------------------------------------------------
def as_hits(kma, conns):
    """conns: (contig, left, strand, peg) arrays -> HIT_DTYPE in canonical order, no duplicates."""
    ct, lf, sd, pg = conns
    h = np.zeros(len(ct), kma.HIT_DTYPE)
    h["contig"], h["left"], h["strand"], h["fid"] = ct, lf, sd, pg
    return np.unique(h)  # sorts by (contig, left, fid, strand)


def check_propose(kma, oracle_c, hits, peg_len, k, **kw):
    got, gst = kma.propose_pegs(hits, peg_len, k, **kw)
    exp, est = oracle_c.propose(hits["contig"], hits["left"], hits["strand"], hits["fid"],
                                peg_len, k, **kw)
    assert (gst == est).all(), (gst, est)
    assert len(got) == len(exp["peg"])
    for f in PROP_FIELDS:
        assert (got[f] == exp[f]).all(), f
    return got, gst


EDGE_PARAMS = dict(min_strength=0.375, max_fuzz=1.6875, min_fuzz=0.796875)
EDGE_PEG_LEN = np.array([20, 23, 21], np.uint32)
# per peg (maxLen, minLen, minKmers) under EDGE_PARAMS: every product is exact in double
EDGE_LIMITS = [(102, 47, 7), (117, 54, 8), (107, 50, 7)]


def proposal_edge_case(k):
    """Seven lists (one per peg, strand and phase) aimed at the sweep's comparisons. Locations of
    one list are 3 apart (one frame), so right - left_i = 3m + 3k - 1 for a later location.
    Returns ((contig, left, strand, peg) arrays, the proposals that must appear as (peg, contig,
    strand, left, right, evidence), the (peg, contig, strand, left) starts that must not)."""
    rows = []

    def add(peg, strand, contig, lefts):
        rows.extend((contig, left, ord(strand), peg) for left in lefts)
    # peg 0, '+', phase 0: 7 = minKmers locations, so one start. The 6th has right == left +
    # maxLen - 1 (counted), the 7th is 3 further (not counted)
    far = 300 + 102 - 3 * k
    add(0, "+", 0, [300, 303, 306, 309, 312, far, far + 3])
    # peg 0, '+', phase 1: 6 = minKmers - 1 locations: too few
    add(0, "+", 0, [301 + 3 * i for i in range(6)])
    # peg 0, '+', phase 2: the list goes on on contig 1; on contig 0 the second location gives
    # best == left + minLen exactly (kept), evidence 2
    add(0, "+", 0, [302, 302 + 48 - 3 * k])
    add(0, "+", 1, [302 + 3 * i for i in range(5)])
    # peg 0, '-', phase 0: 9 locations, starts 0..2, the first alone on its contig
    add(0, "-", 0, [600])
    add(0, "-", 1, [600 + 9 * i for i in range(8)])
    # peg 1, '+', phase 0: 8 = minKmers locations; the second gives best == left + minLen - 1:
    # too short
    add(1, "+", 0, [900, 900 + 54 - 3 * k] + [1500 + 3 * i for i in range(6)])
    # peg 1, '-', phase 0: 9 = minKmers + 1 locations: two starts
    add(1, "-", 0, [900 + 9 * i for i in range(9)])
    # peg 2, '+', phase 0: the second location has right == left + maxLen - 3 (counted), the
    # third right == left + maxLen (not counted)
    near = 1200 + 105 - 3 * k
    add(2, "+", 0, [1200, near, near + 3, near + 6, near + 9, near + 12, near + 15])
    a = np.array(rows, np.int64)
    conns = (a[:, 0].astype(np.uint32), a[:, 1].astype(np.int32), a[:, 2].astype(np.uint8),
             a[:, 3].astype(np.uint32))
    must = [(0, 0, "+", 300, 401, 6), (0, 0, "+", 302, 349, 2), (2, 0, "+", 1200, 1304, 2)]
    must_not = [(0, 0, "+", 301), (1, 0, "+", 900)]
    return conns, must, must_not


def proposal_tuples(p):
    return [(int(a), int(b), chr(c), int(d), int(e), int(f)) for a, b, c, d, e, f in
            zip(p["peg"], p["contig"], p["strand"], p["left"], p["right"], p["evidence"])]


@pytest.mark.parametrize("k", [1, 3, 8, 12])
def test_proposal_list_edges(kma, oracle_c, k):
    conns, must, must_not = proposal_edge_case(k)
    hits = as_hits(kma, conns)
    got, st = check_propose(kma, oracle_c, hits, EDGE_PEG_LEN, k, **EDGE_PARAMS)
    tup = proposal_tuples(got)
    assert set(must) <= set(tup)
    assert not set(must_not) & {t[:4] for t in tup}
    assert st[0] == 7 and st[1] == 1 and st[2] >= 1
    exp, est = oracle_py.propose([(int(h["contig"]), int(h["left"]), chr(h["strand"]),
                                   int(h["fid"])) for h in hits], EDGE_PEG_LEN.tolist(), k,
                                 EDGE_PARAMS["min_strength"], EDGE_PARAMS["max_fuzz"],
                                 EDGE_PARAMS["min_fuzz"])
    assert list(st) == est and [t + (int(f),) for t, f in zip(tup, got["frame"])] == exp


def random_conns(rng, n, n_peg, n_ctg, reach):
    """n distinct connections (distinct (contig, left))."""
    left = np.sort(rng.choice(np.arange(1, reach), n, replace=False)).astype(np.int32)
    ct = np.sort(rng.integers(0, n_ctg, n)).astype(np.uint32)
    sd = np.where(rng.random(n) < 0.5, ord("+"), ord("-")).astype(np.uint8)
    return ct, left, sd, rng.integers(0, n_peg, n).astype(np.uint32)


@pytest.mark.parametrize("k", [1, 3, 8, 12])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_proposal_connection_counts(kma, oracle_c, n, k):
    """n connections around the block size: the sweep rounds its trip count up to whole blocks."""
    rng = np.random.default_rng(1000 * k + n)
    hits = as_hits(kma, random_conns(rng, n, 3, 2, 40 * n + 50))
    assert len(hits) == n
    got, st = check_propose(kma, oracle_c, hits, np.array([5, 9, 30], np.uint32), k,
                            **PROPOSAL_PARAMS["loose"])
    assert st[0] >= 1 and st[2] + st[3] >= 1


def test_proposal_capacity(kma, native_lib, oracle_c):
    """A direct call with room for none and for all but one proposal: KMA_E_CAPACITY, the count
    needed, and the proposals that fit."""
    conns, _, _ = proposal_edge_case(8)
    hits = as_hits(kma, conns)
    exp, est = oracle_c.propose(hits["contig"], hits["left"], hits["strand"], hits["fid"],
                                EDGE_PEG_LEN, 8, **EDGE_PARAMS)
    need = len(exp["peg"])
    assert need == est[3] and need >= 4
    for cap in (0, need - 1, need):
        out = np.zeros(max(cap, 1), kma.PROPOSAL_DTYPE)
        n, stats = C.c_uint64(), np.zeros(4, np.uint64)
        rc = native_lib.kma_propose_pegs(hits.ctypes.data, len(hits), EDGE_PEG_LEN,
                                         len(EDGE_PEG_LEN), 8, EDGE_PARAMS["min_strength"],
                                         EDGE_PARAMS["max_fuzz"], EDGE_PARAMS["min_fuzz"], 0,
                                         out.ctypes.data if cap else None, cap, C.byref(n), stats)
        assert rc == (kma.OK if cap == need else E_CAPACITY)
        assert n.value == need and (stats == est).all()
        for f in PROP_FIELDS:
            assert (out[f][:cap] == exp[f][:cap]).all(), f


@functools.lru_cache(maxsize=None)
def proposal_scale_case():
    """About 1.27M distinct connections (above the 1,048,576 the proposal kernels cover in one
    trip): 40,000 pegs of 3..119 aa with a home contig and position, 32 hits each, 90% of them
    within 9 x the peg's length of home and 10% strays, both strands, 5 contigs. Returns
    ((contig, left, strand, peg) arrays, peg lengths)."""
    rng = np.random.default_rng(71)
    n_peg, per = 40_000, 32
    peg_len = rng.integers(3, 120, n_peg).astype(np.uint32)
    peg = np.repeat(np.arange(n_peg), per)
    n = len(peg)
    home_ct, home_pos = rng.integers(0, 5, n_peg), rng.integers(2_000, 3_000_000, n_peg)
    reach = 9 * peg_len[peg].astype(np.int64)
    left = home_pos[peg] + rng.integers(-reach, reach + 1)
    ct = home_ct[peg]
    stray = rng.random(n) < 0.1
    left[stray] = rng.integers(1, 3_000_000, int(stray.sum()))
    ct[stray] = rng.integers(0, 5, int(stray.sum()))
    sd = np.where(rng.random(n) < 0.5, ord("+"), ord("-")).astype(np.uint8)
    return (ct.astype(np.uint32), left.astype(np.int32), sd, peg.astype(np.uint32)), peg_len


@pytest.mark.parametrize("params", list(PROPOSAL_PARAMS))
def test_proposal_scale(kma, oracle_c, params):
    conns, peg_len = proposal_scale_case()
    hits = as_hits(kma, conns)
    got, st = check_propose(kma, oracle_c, hits, peg_len, 8, **PROPOSAL_PARAMS[params])
    assert len(hits) > 1_048_576 and (st >= 500).all(), st
