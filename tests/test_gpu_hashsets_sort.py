"""genome_sets_kernel (csrc/kma_hashsets.hip) where its sort and its head rule decide the result:
the cases of tests/hashsets_cases.py (duplicate-heavy proteins at every network size 2 .. 4096,
every W, every K, several runs, a block's second protein, bytes without a code);
tests/test_hashsets_workload.py shows on the CPU that every network step and every narrowed head
rule is seen in them.

End to end, every comparison is equality: best, sim, count and stats[0..2] of
kma_hash_annotate_indexed_device against kma_hash_annotate_indexed on the same index, against the
set model (hashindex_cases.set_model) and, except for the 2^20 case, against the C oracle.

The scratch is read back after the call and checked against the plain reference. This is a
white-box check of an internal layout (hash_scratch_layout, csrc/kma_hashsets.h, mirrored by
hashsets_cases.scratch_layout; the mirror's total must equal kma_hash_scratch_bytes, so a layout
change fails here loudly): gsize is the number of distinct windows, a protein's gmatch segment
holds the index position of each of its distinct keys that the index holds exactly once and
kHashEmpty everywhere else, no 0xEE poison stays in it, and every run of a protein of more than W
windows is its chunk's keys in ascending order."""
import time

import numpy as np
import pytest

import hashsets_cases as sc
from hashindex_cases import GRID, kmers
from test_gpu_hashindex_device import DeviceBatch

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
POISON32 = 0xEEEEEEEE


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


class Scratch:
    """The three parts of a call's scratch, read back."""

    def __init__(self, kma, batch):
        gmatch, gsize, runs, total = sc.scratch_layout(batch.n_res, batch.n_g)
        assert total == kma.hash_scratch_bytes(batch.n_res, batch.n_g) == batch.sbytes
        raw = batch.scratch.cpu().numpy()
        assert len(raw) == total
        self.gmatch = raw[gmatch:gmatch + 4 * batch.n_res].view(np.uint32)
        self.gsize = raw[gsize:gsize + 4 * batch.n_g].view(np.uint32)
        self.runs = raw[runs:runs + 8 * batch.n_res].view(np.uint64)

    def check_protein(self, what, at, seg, s, matches, k, w):
        """Protein number `at` of the call, whose residues start at position seg: the string s,
        with `matches` the ascending index positions of its distinct keys in the index."""
        n_win = sc.n_windows(s, k)
        assert self.gsize[at] == len(kmers(s, k)), (what, "gsize", int(self.gsize[at]))
        mine = self.gmatch[seg:seg + len(s)]
        assert not (mine == POISON32).any(), (what, "poison left in gmatch")
        assert (mine[n_win:] == sc.EMPTY).all(), (what, "a trailing position holds a match")
        found = np.sort(mine[mine != sc.EMPTY]).tolist()
        assert found == matches, (what, "gmatch", len(found), len(matches))
        if n_win > w:
            keys = sc.window_keys(sc.LUT[np.frombuffer(s.encode(), np.uint8)], k)
            for c0 in range(0, n_win, w):
                run = self.runs[seg + c0:seg + min(c0 + w, n_win)]
                assert (run == np.sort(keys[c0:c0 + w])).all(), (what, "run", c0 // w)


def check_case_scratch(kma, batch, case, w):
    scratch = Scratch(kma, batch)
    for g, s in enumerate(case.genome):
        scratch.check_protein((case.name, w, g), g, int(case.go[g]), s, case.matches(g), case.k, w)


def run_case(kma, oracle_c, case):
    """The case at every W it names: results against the host entry, the set model and the
    oracle; the scratch against the plain reference."""
    ref = case.ref
    want = (ref.best, ref.sim, ref.count)
    oracle = oracle_c.hash_annotate(case.g, case.go, case.p, case.po, case.k, case.min_sim)
    same(oracle, want, f"{case.name}: C oracle against the set model")
    with kma.ProtoIndex(case.p, case.po, k=case.k) as idx:
        assert idx.info().n_keys == len(case.index)
        best, sim, cnt, st = kma.hash_annotate_indexed(idx, case.g, case.go, case.min_sim,
                                                       stats=True)
        same((best, sim, cnt), want, f"{case.name}: host entry against the set model")
        assert st.tolist() == case.stats()
        for w in case.lds_keys:
            with kma.options(hash_lds_keys=w):
                batch = DeviceBatch(kma, case.g, case.go, len(case.protos))
                batch.call(idx, case.min_sim)
                got = batch.results()
            what = f"{case.name}, W option {w}"
            for a, b in zip(got[:3], (best, sim, cnt)):
                assert a.dtype == b.dtype
            same(got[:3], (best, sim, cnt), what + ": device entry against the host entry")
            same(got[:3], want, what + ": device entry against the set model")
            same(got[:3], oracle, what + ": device entry against the C oracle")
            assert got[3].tolist() == case.stats() + [0], what
            check_case_scratch(kma, batch, case, w or sc.W_MAX)


def test_every_network_size(kma, oracle_c):
    """n2 = 2 .. 4096 at the default W: proteins of n2, n2 - 1 and n2 / 2 + 1 windows whose every
    network step decides some protein's heads (364 steps over 12 sizes), and the run the size-2
    network leaves."""
    run_case(kma, oracle_c, sc.network_case())


def test_runs_at_every_w(kma, oracle_c):
    """3W + 17 and 2W windows built for W = 64 .. 2048, each at all six W options."""
    run_case(kma, oracle_c, sc.every_w_case())


def test_runs_at_the_default_w(kma, oracle_c):
    """2 * 4096 + 41 and 3 * 4096 + 17 windows at W = 4096."""
    run_case(kma, oracle_c, sc.default_w_case())


@pytest.mark.parametrize("k", sc.EVERY_K)
def test_runs_at_every_k(kma, oracle_c, k):
    """Three runs and a partial one at W = 64 for K = 2 .. 12; from K = 7 keys that differ in
    the high word alone, the low word alone and both, up to bit 59."""
    run_case(kma, oracle_c, sc.every_k_case(k))


# ---- more than 2^20 proteins
class Scale:
    """The 2^20 + 517 case: index, the host entry's answers and one device call, made once."""

    def __init__(self, kma):
        t0 = time.perf_counter()
        self.kma, self.case = kma, sc.scale_case()
        s = self.case
        t1 = time.perf_counter()
        self.index = kma.ProtoIndex(s.p, s.po, k=s.k)
        self.host = kma.hash_annotate_indexed(self.index, s.g, s.go, s.min_sim, stats=True)
        t2 = time.perf_counter()
        with kma.options(hash_lds_keys=sc.SCALE_W):
            self.batch = DeviceBatch(kma, s.g, s.go, len(s.protos))
            self.batch.call(self.index, s.min_sim)
            self.got = self.batch.results()
        t3 = time.perf_counter()
        print(f"fixture scale: case {t1 - t0:.2f} s, index and host entry {t2 - t1:.2f} s, "
              f"device entry {t3 - t2:.2f} s")


@pytest.fixture(scope="module")
def scale(kma):
    loaded = Scale(kma)
    yield loaded
    loaded.index.close()


def test_second_protein_of_a_block_end_to_end(scale):
    """517 blocks take a second protein at W = 64: three runs then a short one and the reverse,
    an empty or a K - 1 protein on either side, a duplicate-heavy pair. The whole call equals
    the host entry and the set model."""
    s, got = scale.case, scale.got
    want = s.expected()
    assert scale.index.info().n_keys == len(s.index)
    same(scale.host[:3], want[:3], "host entry against the set model")
    assert scale.host[3].tolist() == want[3]
    same(got[:3], scale.host[:3], "device entry against the host entry")
    same(got[:3], want[:3], "device entry against the set model")
    assert got[3].tolist() == want[3] + [0]
    for g, pair in s.pairs:                 # (said once more for the crafted pairs)
        for at, name in ((g, pair[0]), (g + GRID, pair[1])):
            item = s.item_of[name]
            assert got[0][at] == s.ref.best[item] and got[1][at] == s.ref.sim[item], (g, pair)


def test_second_protein_of_a_block_in_the_scratch(scale):
    """gsize of all 2^20 + 517 proteins; no poison and the right number of matches in every
    protein's gmatch segment; and protein by protein for the 517 pairs and 2,000 others."""
    s = scale.case
    scratch = Scratch(scale.kma, scale.batch)
    assert (scratch.gsize == s.item_size[s.idx]).all()
    assert not (scratch.gmatch == POISON32).any()
    n_match = np.array([len(s.matches_of_item(i)) for i in range(len(s.items))])
    filled = np.concatenate([[0], np.cumsum(scratch.gmatch != sc.EMPTY)])
    off = s.go.astype(np.int64)
    assert (filled[off[1:]] - filled[off[:-1]] == n_match[s.idx]).all()
    matches = {}
    for g in s.checked().tolist():
        i = int(s.idx[g])
        if i not in matches:
            matches[i] = s.matches_of_item(i)
        scratch.check_protein(("scale", g), g, int(off[g]), s.items[i], matches[i], s.k, sc.SCALE_W)


def test_alphabet_flag_from_a_blocks_second_protein(scale):
    """A byte without a code in chunk 1 of protein 2^20 + 1 (three runs; the second protein of
    block 1, after a short one) sets stats[3]."""
    s = scale.case
    g = GRID + 1
    assert s.protein(g) == s.crafted["three_run"] and s.protein(1) == s.crafted["short"]
    res = s.g.copy()
    res[int(s.go[g]) + sc.SCALE_W + 20] = sc.FLAG_BYTE
    with scale.kma.options(hash_lds_keys=sc.SCALE_W):
        batch = DeviceBatch(scale.kma, res, s.go, len(s.protos))
        batch.call(scale.index, s.min_sim)
        assert int(batch.results()[3][3]) != 0
    assert int(scale.got[3][3]) == 0


# ---- the alphabet flag
def test_alphabet_flag_positions(kma):
    """stats[3] is set by a byte without a code at a protein's first byte, at its last byte (read
    by the tail of the last chunk's code loop alone), at each of the K - 1 bytes chunks 0 and 1
    both read, and in chunk 2 of four; it stays 0, with results equal to the host entry's on the
    clean genome, for such a byte just before offsets[0] of a view and just after its last
    protein."""
    f = sc.flag_case()
    with kma.ProtoIndex(f.p, f.po, k=f.k) as idx:
        for w in f.lds_keys:
            for name, res, lo, hi, flagged in f.variants:
                with kma.options(hash_lds_keys=w):
                    batch = DeviceBatch(kma, res, f.go, len(f.protos), lo, hi)
                    batch.call(idx, f.min_sim)
                    got = batch.results()
                assert (int(got[3][3]) != 0) == flagged, (name, w)
                if not flagged:
                    view = f.genome[lo:hi]
                    g, go = kma.pack_strings(view)
                    host = kma.hash_annotate_indexed(idx, g, go, f.min_sim, stats=True)
                    ref = sc.set_model(view, f.protos, f.k, f.min_sim)
                    same(got[:3], host[:3], f"{name}, W option {w}: against the host entry")
                    same(got[:3], (ref.best, ref.sim, ref.count), f"{name}: against the set model")
                    assert got[3][:3].tolist() == host[3].tolist()
                    assert ref.best[1] == 0          # the long protein finds its mutated copy


# ---- a captured call
def test_replayed_graph_on_duplicate_heavy_runs(kma, oracle_c):
    """One call captured at W = 64 on a genome of three runs and a partial one, two runs, and
    two single chunks, all duplicate-heavy; replayed, then replayed on a second such genome
    written over the residues in place. Each replay's outputs equal the host entry's, the set
    model's and the oracle's for its genome, and its scratch is that genome's."""
    cases = sc.graph_cases()
    first = cases[0]
    with kma.ProtoIndex(first.p, first.po, k=first.k) as idx, kma.options(hash_lds_keys=64):
        batch = DeviceBatch(kma, first.g, first.go, len(first.protos))
        batch.call(idx, first.min_sim)       # (the module is loaded before the capture)
        batch.results()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            batch.call(idx, first.min_sim)
        seen = []
        for case in (first, cases[1], first):
            batch.d_res.copy_(torch.from_numpy(case.g))
            batch.poison()
            graph.replay()
            got = batch.results()
            host = kma.hash_annotate_indexed(idx, case.g, case.go, case.min_sim, stats=True)
            want = (case.ref.best, case.ref.sim, case.ref.count)
            same(got[:3], host[:3], f"{case.name}: replay against the host entry")
            same(got[:3], want, f"{case.name}: replay against the set model")
            same(got[:3], oracle_c.hash_annotate(case.g, case.go, case.p, case.po, case.k,
                                                 case.min_sim), f"{case.name}: the C oracle")
            assert got[3].tolist() == case.stats() + [0] == host[3].tolist() + [0]
            check_case_scratch(kma, batch, case, 64)
            seen.append(got[1])
    assert not (seen[0] == seen[1]).all() and (seen[0] == seen[2]).all()
