"""kma_hash_annotate_indexed where index_score_kernel's LDS table carries load
(tests/hashindex_cases.py has the cases and the set model; tests/test_hashindex_workload.py shows
on the CPU that they aim right):

 (a) candidate counts of exactly CAP - 1, CAP, CAP + 1 for CAP 512, 1024 (the default) and 2048
     (kHashCapMax, 32 KiB of LDS), and 2,600; ties across ranges on a best; 4,993 postings of one
     prototype into one slot;
 (b) holders whose first slots are the table's last few: one probe chain of hundreds of slots
     through slot T - 1 into slot 0, below CAP and overflowing inside the chain, at CAP 256, 1024
     and 2048;
 (c) 2^20, 2^20 + 1 and 2^20 + 517 genome proteins: blocks that score a second protein after a
     first that differs from it in best, candidates and splitting;
 (d) min_sim at a similarity's own double and one ulp above; an index wholly above or below the
     genome's keys.

Every comparison is equality on best, sim, count and on all three out_stats, against the set
model, against kma_hash_annotate (the unindexed call) and, where it takes the CPU under a few
seconds, against the C oracle (all of (a), (b) and (d); for (c) its all-pairs loop takes 14 s
per call and is left out)."""
import time

import numpy as np
import pytest

import hashindex_cases as hc
from hashindex_cases import GRID, K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kma(native_lib):
    import kmeranno
    assert kmeranno.device_count() >= 1
    return kmeranno


def same(got, want, what):
    for name, g, w in zip(("best", "sim", "count"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        wrong = np.flatnonzero(g != w)
        assert len(wrong) == 0, (f"{what}: {name} wrong at {len(wrong)} of {len(w)}, first "
                                 f"{wrong[:5].tolist()}: {g[wrong[:5]].tolist()} for "
                                 f"{w[wrong[:5]].tolist()}")


def indexed(kma, index, g, go, min_sim, cap):
    """(best, sim, count), stats of the indexed call at this CAP option (0: the default)."""
    try:
        kma.set_option(kma.OPT_HASH_CAP, cap)
        best, sim, cnt, st = kma.hash_annotate_indexed(index, g, go, min_sim, stats=True)
    finally:
        kma.set_option(kma.OPT_HASH_CAP, 0)
    assert best.dtype == np.int32 and sim.dtype == np.float64 and cnt.dtype == np.uint32
    return (best, sim, cnt), [int(x) for x in st]


class Loaded:
    """A case with its index resident and the unindexed call's and the oracle's answers, each
    asserted equal to the set model once."""

    def __init__(self, kma, oracle_c, case, what):
        t0 = time.perf_counter()
        self.kma, self.case, self.what = kma, case, what
        self.want = (case.ref.best, case.ref.sim, case.ref.count)
        self.index = kma.ProtoIndex(case.p, case.po, k=K)
        same(kma.hash_annotate(case.g, case.go, case.p, case.po, K, case.min_sim), self.want,
             what + ", unindexed call")
        same(oracle_c.hash_annotate(case.g, case.go, case.p, case.po, K, case.min_sim), self.want,
             what + ", C oracle")
        print(f"fixture {what}: {time.perf_counter() - t0:.2f} s")

    def run(self, cap):
        got, st = indexed(self.kma, self.index, self.case.g, self.case.go, self.case.min_sim, cap)
        same(got, self.want, f"{self.what}, CAP option {cap}")
        assert st == self.case.stats(cap), (self.what, cap)
        return st


# ---- (a)
@pytest.fixture(scope="module")
def bounds(kma, oracle_c):
    loaded = Loaded(kma, oracle_c, hc.bounds_case(), "bounds")
    yield loaded
    loaded.index.close()


@pytest.mark.parametrize("cap", hc.BOUND_CAPS)
def test_candidate_counts_at_the_cap_bounds(bounds, cap):
    """A protein splits exactly when it has more than CAP candidates, all three stats are the
    set model's, and nothing of the results depends on CAP."""
    st = bounds.run(cap)
    assert st[0] == 11 and st[1] == sum(n > (cap or hc.CAP_DEFAULT) for n in hc.BOUND_N)
    assert st[1] == {512: 8, 0: 5, 2048: 2}[cap]


# ---- (b)
@pytest.fixture(scope="module", params=sorted(hc.CLUSTER))
def cluster(request, kma, oracle_c):
    loaded = Loaded(kma, oracle_c, hc.cluster_case(request.param), f"cluster {request.param}")
    yield loaded
    loaded.index.close()


def test_probe_chain_across_the_table_end(cluster):
    """At the CAP the holders were chosen for: three proteins overflow inside the chain and are
    scored in halves, three stay at or below CAP and are scored in one range."""
    cap = cluster.case.cap
    st = cluster.run(cap)
    assert st[:2] == [6, 3]
    # the proteins at or below CAP alone, several blocks at once: no split, one range each
    case, below = cluster.case, (2, 3, 4, 3, 2, 4, 4, 3)
    g, go = hc.pack([case.genome[q] for q in below])
    got, st = indexed(cluster.kma, cluster.index, g, go, case.min_sim, cap)
    same(got[:2], (case.ref.best[list(below)], case.ref.sim[list(below)]), "below CAP")
    count = np.zeros(len(case.protos), np.uint32)
    for q in below:
        count[case.ref.passed[q]] += 1
    same(got[2:], (count,), "below CAP")
    assert st == [len(below), 0, len(below)]


def test_cluster_at_the_other_caps(cluster):
    """The same index at the other table sizes (the holders then start all over the table)."""
    for cap in (256, 0, 2048, 16):
        cluster.run(cap)


# ---- (c)
class Scale:
    def __init__(self, kma):
        t0 = time.perf_counter()
        self.kma, self.case = kma, hc.scale_case()
        self.index = kma.ProtoIndex(self.case.p, self.case.po, k=K)
        print(f"fixture scale: {time.perf_counter() - t0:.2f} s")


@pytest.fixture(scope="module")
def scale(kma):
    loaded = Scale(kma)
    yield loaded
    loaded.index.close()


@pytest.mark.parametrize("n", hc.SCALE_SIZES)
def test_blocks_that_score_a_second_protein(scale, n):
    """2^20 proteins: one per block. 2^20 + 1: block 0 scores protein 2^20 (no candidate) after
    protein 0 (a strong best, 302 candidates, splitting at CAP 128). 2^20 + 517: 517 blocks score
    two, 39 of them a crafted pair. Nothing of a block's first protein shows in its second."""
    s = scale.case
    g, go = s.genome(n)
    t0 = time.perf_counter()
    plain = scale.kma.hash_annotate(g, go, s.p, s.po, K, s.min_sim)
    t1 = time.perf_counter()
    same(plain, s.expected(n)[:3], f"n = {n}, unindexed call")
    for cap in (0, hc.SCALE_LOW_CAP):
        want = s.expected(n, cap)
        t2 = time.perf_counter()
        got, st = indexed(scale.kma, scale.index, g, go, s.min_sim, cap)
        print(f"n = {n}, CAP option {cap}: indexed call {time.perf_counter() - t2:.2f} s "
              f"(unindexed {t1 - t0:.2f} s)")
        same(got, want[:3], f"n = {n}, CAP option {cap}")
        assert st == want[3], (n, cap)
        assert (st[1] > 0) == (cap == hc.SCALE_LOW_CAP)
    if n > GRID:
        assert got[0][0] == s.s1_id and got[0][GRID] == -1 and got[1][GRID] == 0.0


# ---- (d)
def test_min_sim_at_the_similarity_itself(kma, oracle_c):
    """shared 1, union 80: the pair proposes and counts at min_sim = 0.0125 and does neither one
    ulp above, in the indexed and in the unindexed call."""
    genome, protos = hc.threshold_case()
    (g, go), (p, po) = hc.pack(genome), hc.pack(protos)
    above = float(np.nextafter(hc.THRESHOLD, 1))
    assert above > hc.THRESHOLD
    with kma.ProtoIndex(p, po, k=K) as idx:
        for min_sim, want in ((hc.THRESHOLD, ([0], [0.0125], [1])), (above, ([-1], [0.0], [0]))):
            got, st = indexed(kma, idx, g, go, min_sim, 0)
            same(got, want, f"indexed, min_sim {min_sim!r}")
            assert st == [1, 0, 1]
            same(kma.hash_annotate(g, go, p, po, K, min_sim), want, f"unindexed, {min_sim!r}")
            same(oracle_c.hash_annotate(g, go, p, po, K, min_sim), want, f"oracle, {min_sim!r}")
            ref = hc.set_model(genome, protos, K, min_sim)
            same(got, (ref.best, ref.sim, ref.count), "set model")


@pytest.mark.parametrize("index_above", [True, False])
def test_index_keys_all_above_or_all_below_the_genome(kma, oracle_c, index_above):
    """The lookup's lower bound lands at 0 (at n_u) for every genome key: no match, no proposal."""
    genome, protos = hc.disjoint_keys_case(index_above)
    (g, go), (p, po) = hc.pack(genome), hc.pack(protos)
    want = (np.full(len(genome), -1), np.zeros(len(genome)), np.zeros(len(protos)))
    with kma.ProtoIndex(p, po, k=K) as idx:
        assert idx.info().n_keys > 1000
        got, st = indexed(kma, idx, g, go, 0.0125, 0)
    same(got, want, "indexed")
    assert st == [0, 0, 0]
    same(kma.hash_annotate(g, go, p, po, K, 0.0125), want, "unindexed")
    same(oracle_c.hash_annotate(g, go, p, po, K, 0.0125), want, "oracle")
