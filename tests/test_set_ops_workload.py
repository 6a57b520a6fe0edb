"""The inputs of tests/test_gpu_set_ops.py meet the conditions its GPU tests rely on, shown on the
oracle alone (no GPU): the scale cases are above the grid caps they are meant to cross, the tie
ties, every threshold and list edge falls where it is aimed, and the C oracle equals its Python
twin on the small cases."""
import numpy as np
import pytest

from oracle import oracle_py
from test_gpu_set_ops import (HASH_SCALE_CASES, BEST_EDGE_CASES, BEST_EDGE_PROTS, BUILD_K1_CASES, BUILD_K1_PROTS,
                              EDGE_LIMITS, EDGE_PARAMS, EDGE_PEG_LEN, HASH_EMPTY_GENOME,
                              HASH_EMPTY_PROTOS, HASH_MIN_SIMS, LONG_RUN_KMER, LONG_RUN_VARIANTS,
                              PROPOSAL_PARAMS, batch_shapes, best_match_case, cand_counts,
                              distance_scale_case, hash_count_case, hash_scale_case,
                              hash_shared_case, hash_shared_sets_case, hash_tie_case, java_best,
                              long_run_case, pack, proposal_edge_case, proposal_scale_case,
                              random_conns, shared_input, shared_lengths, shared_pairs)

GRID1_CAP = 8192 * 256       # kma_kmersets.h grid1: items per trip
WAVE_CAP = 16384 * 4         # kma_kmersets.h grid_waves: proteins or pairs per trip
BUILD_CAP = 8192 * 4         # launch_build_windows: proteins per trip
PROPOSAL_CAP = 4096 * 256    # kma_proposals.hip grid_of: connections per trip


def _sizes(oracle_c, res, off, k):
    """Distinct kmers per protein (the oracle's |A| of the pair (i, i))."""
    idx = np.arange(len(off) - 1, dtype=np.uint32)
    return oracle_c.protein_distances(res, off, idx, idx, k, 0)[1].astype(np.int64)


@pytest.mark.parametrize("k", range(1, 13))
def test_shared_input_shape(oracle_c, k):
    si = shared_input(k)
    lens = [len(p) for p in si.prots]
    assert set(shared_lengths(k)) | {200, 40_000} <= set(lens)
    assert lens[0] == lens[1] == 0 and lens[-1] == 0 and lens.count(0) >= 7
    assert set(b"".join(si.prots)) == set(b"ABCDEFGHIJKLMNOPQRSTUVWXYZ*")
    assert any(p[:1] == b"*" for p in si.prots) and any(p[:1] == b"Z" for p in si.prots)
    assert any(p[-1:] == b"*" for p in si.prots) and any(p[-1:] == b"Z" for p in si.prots)
    assert b"A" * k in si.prots and set(si.roles) >= {-2, -1, 0, 1, 2, 3, 4}
    assert [len(b) for b in batch_shapes(k)] == [1, 2, 3, 5, 7, 3, 3]
    assert all(len(p) < k for p in batch_shapes(k)[-1]) and not any(batch_shapes(k)[-2])
    if k == 1:
        return  # the pair operators take K >= 2
    res, off = pack(si.prots)
    pa, pb = shared_pairs(k)
    for flags in (0, 1):
        sim, sa, sb, dist = oracle_c.protein_distances(res, off, pa, pb, k, flags)
        between = (sim > 0) & (sim < np.minimum(sa, sb))
        print(f"K={k} flags={flags}: pairs {len(pa)} with 0 < sim < 1: {int(between.sum())}")
        assert between.sum() >= 20
        assert (sa > sb).sum() >= 10 and (sa < sb).sum() >= 10 and (sa == sb).sum() >= 10
        assert ((sa == 0) & (sb == 0) & (dist == 1.0)).sum() >= 2
        # '*' against 'Z' at one position: the sets differ (at the last position only when the
        # last window counts)
        for j, (a, b) in enumerate(si.star_z):
            s, za = oracle_c.protein_distances(res, off, [a], [b], k, flags)[:2]
            assert (s[0] < za[0]) == (flags == 0 or j != 1)
    size = _sizes(oracle_c, res, off, k)
    assert size[si.long[0]] > (700 if k == 2 else 10_000) and size[lens.index(200)] == 1


def test_distance_scale_shape(oracle_c):
    res, off, pa, pb = distance_scale_case()
    assert len(off) - 1 > WAVE_CAP and len(pa) > WAVE_CAP and len(pa) % 4 == 3
    sim = oracle_c.protein_distances(res, off, pa, pb, 2, 0)[0]
    print(f"pairs sharing a kmer: {(sim > 0).mean():.3f}")
    assert (sim > 0).mean() > 0.10
    assert (pa[-10:] == pb[-10:]).all() and pa[-1] == len(off) - 2


@pytest.mark.parametrize("k", [2, 3, 8, 12])
def test_best_match_case_shape(oracle_c, k):
    """Each max_dist decides differently, empty candidate lists come first, in the middle and
    last, and at max_dist 0 the later of two identical candidates is the answer."""
    prots, query, cand_off, cand, cands = best_match_case(k)
    n = len(query)
    assert not cands[0] and not cands[n // 2] and not cands[n - 1]
    res, off = pack(prots)
    pa = np.repeat(query, np.diff(cand_off).astype(np.int64))
    edist = oracle_c.protein_distances(res, off, pa, cand, k, 0)[3]
    b0, d0 = java_best(edist, cand, cand_off, 0.0)
    b5, d5 = java_best(edist, cand, cand_off, 0.5)
    b1, d1 = java_best(edist, cand, cand_off, 1.0)
    size = _sizes(oracle_c, res, off, k)
    has = np.array([bool(c) for c in cands]) & (size[:n] > 0)
    # max_dist 0: an identical set is found, nearly always the query itself, which comes after
    # its copy; queries without kmers or without candidates find nothing
    assert (d0[has] == 0.0).all() and (b0[has] == query[has]).mean() > 0.8
    assert (b0[~has] == -1).all() and (~has).sum() >= 8
    assert (b1 >= 0).sum() == sum(bool(c) for c in cands)
    assert ((d1 == 1.0) & (b1 >= 0)).sum() >= 3  # a last candidate accepted at distance 1.0
    assert ((edist > 0) & (edist < 0.5)).sum() >= 3 and (edist == 1.0).sum() >= 50
    assert (b5 == b0)[has].all() and (b1 == b0)[has].all()


def test_best_match_edge_expectations(oracle_c):
    res, off = pack(BEST_EDGE_PROTS)
    for q, cands, max_dist, want, want_d in BEST_EDGE_CASES:
        edist = oracle_c.protein_distances(res, off, [q] * len(cands), cands, 3, 0)[3]
        best, bd = java_best(edist, cands, np.array([0, len(cands)]), max_dist)
        assert (int(best[0]), float(bd[0])) == (want, want_d)
    assert oracle_c.protein_distances(res, off, [0], [1], 3, 0)[3][0] == 0.5


@pytest.mark.parametrize("k", range(2, 13))
def test_hash_shared_case_shape(oracle_c, k):
    genome, protos = hash_shared_case(k)
    assert protos[0] == b"" and protos[-1] == b"" and b"" in protos[1:-1]
    assert b"A" * (k - 1) in protos
    g, p = pack(genome), pack(protos)
    counts = []
    for min_sim in HASH_MIN_SIMS:
        best, sim, cnt = oracle_c.hash_annotate(*g, *p, k, min_sim)
        counts.append(int(cnt.sum()))
        if min_sim == HASH_MIN_SIMS[-1]:
            assert (sim[best >= 0] == 1.0).all() and (best >= 0).sum() >= 3
    print(f"K={k}: matches per min_sim {counts}")
    assert counts[0] >= counts[1] > counts[2] > counts[3] >= 4
    best, sim, cnt = oracle_c.hash_annotate(*g, *p, k, 0.0125)
    assert ((sim > 0) & (sim < 1)).sum() >= 15
    assert best[shared_input(k).by_len[65]] == len(protos) - 5  # the earlier of two exact copies


def test_hash_tie_and_thresholds(oracle_c):
    third = 1.0 / 3.0
    assert np.float64(third).tobytes() == np.float64(2.0 / 6.0).tobytes()
    for order in (0, 1):
        genome, protos = hash_tie_case(order)
        for min_sim in (0.0, third):
            best, sim, cnt = oracle_c.hash_annotate(*pack(genome), *pack(protos), 3, min_sim)
            assert best.tolist() == [0] and sim.tolist() == [third] and cnt.tolist() == [1, 1]
            assert oracle_py.hash_annotate([b"ACDE".decode()], [p.decode() for p in protos], 3,
                                           min_sim) == ([0], [third], [1, 1])
        best, sim, cnt = oracle_c.hash_annotate(*pack(genome), *pack(protos), 3,
                                                float(np.nextafter(third, 1.0)))
        assert best.tolist() == [-1] and cnt.tolist() == [0, 0]
    best, sim, cnt = oracle_c.hash_annotate(*pack([b"ACD"]), *pack([b"ACDE"]), 3, 0.5)
    assert best.tolist() == [0] and sim.tolist() == [0.5] and cnt.tolist() == [1]


def test_hash_empty_case_shape(oracle_c):
    cc = cand_counts(HASH_EMPTY_GENOME, HASH_EMPTY_PROTOS, 3)
    assert cc == [0, 7, 6, 0, 13, 0, 6, 0]
    # a slice size of 13 candidates: prototypes 0..3 fill a slice exactly, the cut falls right
    # after the empty prototype 3, and prototype 4 alone fills the next
    assert sum(cc[:4]) == 13 and sum(cc[:5]) > 13 and cc[4] == 13 and cc[4] + cc[6] > 13
    best, sim, cnt = oracle_c.hash_annotate(*pack(HASH_EMPTY_GENOME), *pack(HASH_EMPTY_PROTOS), 3,
                                            0.5)
    assert best.tolist() == [-1, 4, -1, 1, 2, -1] and cnt.tolist() == [0, 2, 1, 0, 1, 0, 1, 0]
    assert sim.tolist() == [0.0, 1.0, 0.0, 0.6, 4 / 6, 0.0]


@pytest.mark.parametrize("n_pt", [1, 2, 3, 4, 5, 256, 257])
def test_hash_count_case_shape(oracle_c, n_pt):
    genome, protos = hash_count_case(n_pt)
    assert len(protos) == n_pt
    best, sim, cnt = oracle_c.hash_annotate(*pack(genome), *pack(protos), 3, 0.0125)
    assert best[0] == n_pt - 1 and sim[0] == 1.0
    if n_pt > 40:
        assert len(set(best.tolist())) >= 30 and (cnt > 0).sum() >= n_pt - 5


def test_hash_shared_sets_shape(oracle_c):
    genome, protos = hash_shared_sets_case()
    assert len(set(genome[:500])) == 1 and len(set(genome)) == 41
    best, sim, cnt = oracle_c.hash_annotate(*pack(genome), *pack(protos), 5, 0.0125)
    assert (best[:500] == 2).all() and cnt[2] == cnt[4] >= 500


@pytest.mark.parametrize("name", HASH_SCALE_CASES)
def test_hash_scale_shape(oracle_c, name):
    genome, protos, k, min_sim = hash_scale_case(name)
    best, sim, cnt = oracle_c.hash_annotate(*genome, *protos, k, min_sim)
    n_gp, n_pt = len(genome[1]) - 1, len(protos[1]) - 1
    positions = int(protos[1][-1] - protos[1][0])
    pairs = int(_sizes(oracle_c, *genome, k).sum())
    print(f"{name}: genome {n_gp} prototypes {n_pt} positions {positions} genome pairs {pairs} "
          f"matches {int(cnt.sum())} annotated {int((best >= 0).sum())}")
    if name == "runs":
        assert cnt.sum() > GRID1_CAP  # min_sim 0: every run is a match
    elif name == "positions":
        assert positions > GRID1_CAP
    elif name == "pairs":
        assert pairs > GRID1_CAP and n_gp <= WAVE_CAP
    elif name == "proteins":
        assert n_gp > GRID1_CAP and (best >= 0).sum() > 100_000 and (cnt > 0).all()
    else:
        assert n_pt > GRID1_CAP and (best >= 0).all() and (cnt > 0).sum() > 100_000
    assert (best >= 0).sum() >= 6 and cnt.sum() > 1000


def test_build_k1_expectations(oracle_c):
    for roles, want in BUILD_K1_CASES:
        res, off = pack(BUILD_K1_PROTS)
        assert min(roles) >= -1 and int(off[-1]) == 7  # nothing skipped: 7 positions, 7 windows
        km, rl = oracle_c.build_signatures(res, off, roles, 1, 0)
        assert {bytes(r).decode(): int(v) for r, v in zip(km, rl)} == want
        assert oracle_py.build_signatures([p.decode() for p in BUILD_K1_PROTS], roles, 1) == want


@pytest.mark.parametrize("variant", list(LONG_RUN_VARIANTS))
def test_build_long_run_shape(oracle_c, variant):
    res, off, roles, kept = long_run_case(variant)
    lens = np.diff(off.astype(np.int64))
    assert len(lens) > BUILD_CAP and lens.min() >= 16
    has = np.array([res[int(o):int(o) + 8].tobytes() == LONG_RUN_KMER for o in off[:-1]])
    assert has.all() and (roles == 3).sum() == 70_000
    km, rl = oracle_c.build_signatures(res, off, roles, 8, 0)
    rows = {bytes(r) for r in km}
    assert (LONG_RUN_KMER in rows) == kept and len(rows) > 500_000


@pytest.mark.parametrize("k", [1, 3, 8, 12])
def test_proposal_edge_expectations(oracle_c, k):
    """The edge lists under EDGE_PARAMS: the limits are the ones the lists are laid out for, and
    the oracle counts the location at maxLen - 1, drops the one at maxLen, keeps best == left +
    minLen, and calls minLen - 1 too short and minKmers - 1 locations too few."""
    for n, (max_len, min_len, min_kmers) in zip(EDGE_PEG_LEN.tolist(), EDGE_LIMITS):
        bp = 3 * n
        assert (int(bp * EDGE_PARAMS["max_fuzz"] + 1), int(bp * EDGE_PARAMS["min_fuzz"]),
                int(bp * (EDGE_PARAMS["min_strength"] / 3))) == (max_len, min_len, min_kmers)
    (ct, lf, sd, pg), must, must_not = proposal_edge_case(k)
    assert len(set(zip(ct.tolist(), lf.tolist(), sd.tolist(), pg.tolist()))) == len(ct)
    exp, st = oracle_c.propose(ct, lf, sd, pg, EDGE_PEG_LEN, k, **EDGE_PARAMS)
    tup = [(int(a), int(b), chr(c), int(d), int(e), int(f)) for a, b, c, d, e, f in
           zip(exp["peg"], exp["contig"], exp["strand"], exp["left"], exp["right"],
               exp["evidence"])]
    print(f"K={k}: stats {st.tolist()} proposals {tup}")
    assert set(must) <= set(tup) and not set(must_not) & {t[:4] for t in tup}
    assert st[0] == 7 and st[1] == 1 and st[2] >= 2 and st[3] == len(tup) >= 7
    span = 3 * k - 1
    lefts = set(lf.tolist())
    assert 300 + 102 - 1 - span in lefts and 300 + 102 + 2 - span in lefts   # maxLen - 1, + 2
    assert 1200 + 107 - span in lefts and 1200 + 107 - 3 - span in lefts     # maxLen, - 3
    assert 302 + 47 - span in lefts and 900 + 54 - 1 - span in lefts         # minLen, minLen - 1
    # the list that goes on on a second contig: one start, on contig 0
    assert sum(t[:3] == (0, 1, "+") for t in tup) == 0


def test_proposal_count_and_scale_shape(oracle_c):
    for n in (1, 255, 256, 257):
        ct, lf, sd, pg = random_conns(np.random.default_rng(n), n, 3, 2, 40 * n + 50)
        assert len(set(zip(ct.tolist(), lf.tolist()))) == n
    (ct, lf, sd, pg), peg_len = proposal_scale_case()
    conns = np.unique(np.stack([ct.astype(np.int64), lf, pg, sd]), axis=1)
    assert conns.shape[1] > PROPOSAL_CAP and len(peg_len) == 40_000
    assert set(np.unique(ct).tolist()) == {0, 1, 2, 3, 4} and lf.min() >= 1
    assert 0.4 < (sd == ord("+")).mean() < 0.6
    for name, kw in PROPOSAL_PARAMS.items():
        exp, st = oracle_c.propose(*conns[[0, 1, 3, 2]], peg_len, 8, **kw)
        print(f"{name}: connections {conns.shape[1]} stats {st.tolist()}")
        assert (st >= 500).all()


@pytest.mark.parametrize("k", [2, 8, 12])
def test_python_twin_on_shared_input(oracle_c, k):
    """The C oracle's distances equal the string-and-set twin's on the shared pairs without a
    long protein, under both window conventions."""
    si = shared_input(k)
    pa, pb = shared_pairs(k)
    keep = np.isin(pa, si.small) & np.isin(pb, si.small)
    res, off = pack(si.prots)
    for flags in (0, 1):
        edist = oracle_c.protein_distances(res, off, pa[keep], pb[keep], k, flags)[3]
        twin = [oracle_py.distance(si.prots[a].decode(), si.prots[b].decode(), k, flags == 1)
                for a, b in zip(pa[keep].tolist(), pb[keep].tolist())]
        assert edist.tolist() == twin
