"""GPU parity on fragmented genomes: thousands of contigs per call, many shorter than one window.

Every genome-side operator locates a position's contig by a search of the offsets array with code
of its own, and the rest of the suite gives those searches a handful of contigs. Here the 6-frame
probe runs its three ways to a contig (offsets cached by ballot below 64 contigs; a 64-ary wave
search of 1, 2, 3 and 4 rounds with a cached window of 64 offsets, clamped at the end of the array;
a binary search per lane where more than 64 contigs meet one tile) at the contig counts where they
switch (63 / 64 / 65, 4,095 / 4,096 / 4,097, 64^3 + 1); the host call shards 4,400 contigs over two
replicas; the ORF index, the proposal sweep and the translation search offsets of thousands to
hundreds of thousands of entries with runs of equal values; and the projector orders its features
by contig ids whose string order is not their index order. Every comparison is bit-exact against
the checker the operator's own tests use (the C oracle, oracle/proposal_list.py, the oracle's
translate). The genomes are tests/fragment_cases.py's; tests/test_fragment_workload.py shows on the
oracle alone that they reach those branches."""
import ctypes as C

import numpy as np
import pytest

import fragment_cases as fc

pytestmark = pytest.mark.gpu
K = fc.K
HIT_FIELDS = ("contig", "left", "strand", "frame", "fid")
PROPOSAL_FIELDS = ("peg", "contig", "strand", "left", "right", "evidence", "frame")


@pytest.fixture(scope="module")
def kma(native_lib):
    import kmeranno
    assert kmeranno.device_count() >= 1
    return kmeranno


@pytest.fixture(params=["auto", "chained"])
def layout(request):
    """The size rule's table with two-choice placement, or with overflow chains (read per table
    creation, reset after the test by conftest)."""
    import kmeranno
    kmeranno.load()
    kmeranno.set_option(kmeranno.OPT_LAYOUT, -1)
    kmeranno.set_option(kmeranno.OPT_PLACEMENT, 0 if request.param == "chained" else -1)
    return request.param


def make_table(kma, rows, fids, devices=None):
    """kma_table_create (kma_table_create_replicated with devices) on (n, k) kmer bytes."""
    n, k = rows.shape
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(k)
    h = C.c_void_p()
    if devices is None:
        kma._check(kma.load().kma_table_create(rows.tobytes(), off, fids.astype(np.uint32), n, k, 0,
                                               0.5, C.byref(h)))
    else:
        dv = np.ascontiguousarray(devices, np.int32)
        kma._check(kma.load().kma_table_create_replicated(rows.tobytes(), off,
                                                          fids.astype(np.uint32), n, k, len(dv),
                                                          dv, 0.5, C.byref(h)))
    return kma.SignatureTable(h)


def assert_hits_equal(hits, e):
    assert len(hits) == len(e[0])
    for f, b in zip(HIT_FIELDS, e):
        assert (hits[f] == b).all(), f


def expected_tally(g, e):
    t = np.zeros((g.n_contig, fc.N_FID), np.uint32)
    np.add.at(t, (e[0], e[4]), 1)
    return t


def genome(small_gto, case):
    return fc.frag4k(small_gto) if case == "frag4k" else fc.boundary(small_gto, case)


# ---- 1. the 6-frame probe ---------------------------------------------------------------------------

@pytest.mark.parametrize("k", [8, 3])
@pytest.mark.parametrize("case", ["frag4k", *fc.BOUNDARY_COUNTS], ids=str)
def test_probe_vs_oracle(kma, oracle_c, small_gto, case, k, layout):
    """frag4k and the boundary contig counts against half of their own K-mers (random fids, the
    last row wins) at K = 8 and K = 3: the host call with a tally and the device call on buffers
    whose offsets[0] is not 0 both give the oracle's hits in canonical order and its tally rows.
    The oracle's own hits show that the branches are exercised: hits in a tile that meets more
    than 64 contigs and on the contig just after the empty one on a tile boundary (frag4k), on
    the last three non-empty contigs (the boundary counts)."""
    torch = pytest.importorskip("torch")
    g = genome(small_gto, case)
    rows, fids = fc.sample_table(oracle_c, g, k)
    e = fc.expect_contigs(oracle_c, g, k)
    off = g.off.astype(np.int64)
    if case == "frag4k":
        _, nc = fc.probe_tiles(g.off)
        d0, dn = g.dense_run
        assert (nc[fc.hit_tiles(off, e[0], e[1])] > fc.OFF_CACHE).sum() >= 1
        assert (e[0] == g.empty_at_boundary["at"] + 1).sum() >= 20 and len(e[0]) >= 100_000
        if k == 3:
            assert ((e[0] >= d0) & (e[0] < d0 + dn)).sum() >= 20
    else:
        assert np.isin(e[0], np.flatnonzero(g.lens > 0)[-3:]).sum() >= 20
        assert (fc.probe_paths(g.off)["ballot"] > 0) == (case < 64)
    want_tally = expected_tally(g, e)
    lead = 777  # bases of another call in front of this one's: offsets[0] = 777
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    with make_table(kma, rows, fids) as t:
        assert t.info.k == k and (layout != "chained" or t.info.two_choice == 0)
        hits, tally = kma.annotate_contigs(t, g.dna, g.off, 11, n_fid=fc.N_FID)
        assert_hits_equal(hits, e)
        assert (tally == want_tally).all()
        ws = kma.Workspace(0)
        ws.reserve_contigs(g.n_bases)
        d_dna = torch.from_numpy(np.concatenate([np.full(lead, ord("G"), np.uint8), g.dna])).to(dev)
        d_off = torch.from_numpy((g.off + np.uint64(lead)).view(np.int64)).to(dev)
        cap = len(e[0]) + 16
        d_hits = torch.zeros(cap * kma.HIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_nh = torch.zeros(1, dtype=torch.int64, device=dev)
        d_tally = torch.zeros(g.n_contig * fc.N_FID, dtype=torch.int32, device=dev)
        kma.annotate_contigs_device(t, ws, d_dna.data_ptr(), d_off.data_ptr(), g.n_contig,
                                    g.n_bases, 11, d_hits.data_ptr(), cap, d_nh.data_ptr(),
                                    d_tally.data_ptr(), fc.N_FID, stream)
        torch.cuda.synchronize()
        assert int(d_nh.item()) == len(e[0])
        raw = d_hits.cpu().numpy()
        assert not raw[len(e[0]) * kma.HIT_DTYPE.itemsize:].any()
        assert_hits_equal(raw.view(kma.HIT_DTYPE)[:len(e[0])], e)
        got_tally = d_tally.cpu().numpy().view(np.uint32).reshape(g.n_contig, fc.N_FID)
        assert (got_tally == want_tally).all()
        ws.close()


# ---- 2. replica shards ------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [8, 3])
@pytest.mark.parametrize("variant", ["frag4k", "half_empty"])
def test_probe_two_replicas(kma, oracle_c, small_gto, variant, k):
    """The host call on a table with two replicas on device 0 shards the contigs at the half-way
    base, rebases each shard's contig indices and writes its tally rows at contig * n_fid: hits
    and tally identical to the single replica's and the oracle's. half_empty: the half-way base
    lies on a run of 50 empty contigs, where the second shard then starts."""
    g = fc.frag4k(small_gto) if variant == "frag4k" else fc.frag4k_half_empty(small_gto)
    rows, fids = fc.sample_table(oracle_c, g, k)
    e = fc.expect_contigs(oracle_c, g, k)
    # both shards carry hits, also on the contigs next to the cut
    cut = int(np.searchsorted(g.off[1:], g.n_bases // 2, side="left")) + 1
    assert (e[0] < cut).sum() >= 10_000 and (e[0] >= cut).sum() >= 10_000
    if variant == "half_empty":
        e0, en = g.empties
        assert e0 <= cut <= e0 + en and (e[0] == e0 - 1).sum() >= 1 and (e[0] == e0 + en).sum() >= 1
    with make_table(kma, rows, fids) as t1:
        h1, y1 = kma.annotate_contigs(t1, g.dna, g.off, 11, n_fid=fc.N_FID)
    with make_table(kma, rows, fids, devices=[0, 0]) as t2:
        assert t2.replicas == [0, 0]
        h2, y2 = kma.annotate_contigs(t2, g.dna, g.off, 11, n_fid=fc.N_FID)
    assert_hits_equal(h2, e)
    assert (h1 == h2).all() and (y1 == y2).all() and (y2 == expected_tally(g, e)).all()


# ---- 3. the peg join ----------------------------------------------------------------------------------

@pytest.mark.parametrize("strict", [False, True], ids=["aggressive", "strict"])
def test_peg_join_vs_oracle(kma, oracle_c, small_gto, strict):
    g = fc.frag4k(small_gto)
    e, peg_len = fc.expect_join(oracle_c, small_gto, strict)
    assert len(e[0]) >= 50_000 and len(np.unique(e[0])) >= 500 and (e[0] > 4096).sum() >= 100
    res, off = kma.pack_strings(fc.close_proteins(small_gto))
    t, _ = kma.SignatureTable.from_pegs(res, off, K)
    with t:
        hits = kma.connect_pegs(t, g.dna, g.off, 11, strict)
    assert_hits_equal(hits, e)


# ---- 4. 262,145 contigs ----------------------------------------------------------------------------------

def make_props(kma, rows):
    """rows of (contig, strand, left, right, evidence) -> PROPOSAL_DTYPE."""
    arr = np.zeros(len(rows), kma.PROPOSAL_DTYPE)
    arr["contig"] = [r[0] for r in rows]
    arr["strand"] = [ord(r[1]) for r in rows]
    arr["left"] = [r[2] for r in rows]
    arr["right"] = [r[3] for r in rows]
    arr["evidence"] = [r[4] for r in rows]
    return arr


def check_extension(kma, g, rows, gcode, min_strength, min_evidence):
    """kma_orf_index_create + kma_extend_proposals against the oracle's extend and filters:
    status, left, right per row and the four counters. Returns the oracle's status histogram."""
    want = fc.oracle_orf_rows(fc.contig_strings(g), rows, gcode, min_strength, min_evidence)
    with kma.OrfIndex(g.dna, g.off, gcode) as idx:
        left, right, status, stats = kma.extend_proposals(idx, make_props(kma, rows), min_strength,
                                                          min_evidence)
    got = list(zip(status.tolist(), left.tolist(), right.tolist()))
    bad = [(r, a, b) for r, a, b in zip(rows, got, want) if a != b]
    assert not bad, (len(bad), bad[:5])
    hist = np.bincount([w[0] for w in want], minlength=4)
    assert stats.tolist() == [len(rows), hist[fc.REJECTED], hist[fc.WEAK], hist[fc.SMALL]]
    return hist


def test_frag262k_probe_vs_oracle(kma, oracle_c, small_gto):
    """64^3 + 1 contigs through the host 6-frame call: the wave search takes four rounds, nearly
    every tile meets hundreds of contigs, the last gene-bearing contigs' window is clamped."""
    g = fc.frag262k(small_gto)
    rows, fids = fc.sample_table(oracle_c, g, K)
    e = fc.expect_contigs(oracle_c, g, K)
    per = [int((e[0] == p).sum()) for p in g.genes]
    assert min(per) >= 20 and fc.wave_search_rounds(g.n_contig) == 4
    paths = fc.probe_paths(g.off)
    assert paths["global"] >= 100 and paths["clamped"] >= 1
    with make_table(kma, rows, fids) as t:
        hits, _ = kma.annotate_contigs(t, g.dna, g.off, 11)
    assert_hits_equal(hits, e)


def test_frag262k_orf_extension(kma, small_gto):
    """The ORF index over 262,145 contigs: every 24-base span of the 20 gene-bearing contigs on
    both strands and 2,000 spans of 3 to 6 bases on the tiny contigs."""
    g = fc.frag262k(small_gto)
    rows = [(p, s, lft, lft + 23, 1) for p in g.genes
            for lft in range(1, int(g.lens[p]) - 22) for s in "+-"]
    rng = np.random.default_rng(262)
    tiny = np.setdiff1d(np.flatnonzero(g.lens >= 3), g.genes)
    for c in rng.choice(tiny, 2000, replace=False).tolist():
        n = int(g.lens[c])
        ln = int(rng.integers(3, n + 1))
        lft = int(rng.integers(1, n - ln + 2))
        rows.append((c, "+-"[int(rng.integers(0, 2))], lft, lft + ln - 1, 1))
    hist = check_extension(kma, g, rows, 11, 0.0, 0)
    assert len(rows) >= 40_000
    assert hist[fc.KEPT] >= 0.05 * len(rows) and hist[fc.REJECTED] >= 0.05 * len(rows)


# ---- 5. the ORF index on frag4k ------------------------------------------------------------------------------

@pytest.mark.parametrize("gcode", [11, 4])
def test_frag4k_orf_extension(kma, oracle_c, small_gto, gcode):
    """Up to 30,000 spans of 3 to 24 bases on the contigs shorter than 48 bases (evidence 1..40)
    and the oracle's real proposals from the join, under the projector's default filters."""
    g = fc.frag4k(small_gto)
    rows = fc.frag4k_orf_rows(oracle_c, small_gto)
    assert 35_000 <= len(rows) <= 45_000
    hist = check_extension(kma, g, rows, gcode, 0.5 / 3, 10)
    assert hist[fc.KEPT] >= 0.05 * len(rows) and hist[fc.REJECTED] >= 0.05 * len(rows)
    assert hist[fc.WEAK] >= 1 and hist[fc.SMALL] >= 1


# ---- 6. the proposal sweep -------------------------------------------------------------------------------------

def check_sweep(kma, oracle_c, hits, peg_len, **kw):
    got, gst = kma.propose_pegs(hits, peg_len, K, **kw)
    exp, est = oracle_c.propose(hits["contig"], hits["left"], hits["strand"], hits["fid"], peg_len,
                                K, **kw)
    assert (gst == est).all(), (gst, est)
    assert len(got) == len(exp["peg"])
    for f in PROPOSAL_FIELDS:
        assert (got[f] == exp[f]).all(), f
    return got, gst


@pytest.mark.parametrize("params", [dict(), fc.LOOSE], ids=["defaults", "loose"])
@pytest.mark.parametrize("strict", [False, True], ids=["aggressive", "strict"])
def test_sweep_on_the_join(kma, oracle_c, small_gto, strict, params):
    """The oracle's connections of frag4k (1,000 contigs carry some): a peg's list crosses many
    contig runs."""
    e, peg_len = fc.expect_join(oracle_c, small_gto, strict)
    hits = np.zeros(len(e[0]), kma.HIT_DTYPE)
    for f, a in zip(HIT_FIELDS, e):
        hits[f] = a
    got, st = check_sweep(kma, oracle_c, hits, peg_len, **params)
    assert len(got) >= 5000 and len(np.unique(got["contig"])) >= 100 and st[0] > 500


@pytest.mark.parametrize("params", [dict(), fc.SYNTHETIC_LOOSE], ids=["defaults", "loose"])
def test_sweep_synthetic_many_contigs(kma, oracle_c, params):
    """200,000 connections of 300 pegs over 5,000 contigs: a list crosses hundreds of contig
    runs of 1 to 3 connections. Under the defaults nearly every start is turned down (too few
    kmers in 1,518 of the 1,800 lists, too short at 14,834 starts, 16 proposals), so that case
    is mostly about the rejection counters; the loose parameters propose at 12,632 starts."""
    hits, peg_len = fc.synthetic_connections(kma.HIT_DTYPE)
    got, st = check_sweep(kma, oracle_c, hits, peg_len, **params)
    assert st[0] >= 500 and len(got) >= (1000 if params else 10)
    if not params:
        assert st[1] >= 1000 and st[2] >= 10_000


# ---- 7. translation ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("peg", [False, True], ids=["raw", "peg"])
@pytest.mark.parametrize("order", ["index", "shuffled"])
@pytest.mark.parametrize("name", ["frag4k", "frag262k"])
def test_translate_whole_contigs(kma, small_gto, name, order, peg):
    """One whole-contig location per contig, strands alternating, empty contigs as left = 1,
    right = 0: the search of the output offsets steps over runs of 50 and more locations without
    a residue; on frag262k the flat output spans more than 100 translate tiles in either mode."""
    from kmeranno import projector
    g = fc.frag4k(small_gto) if name == "frag4k" else fc.frag262k(small_gto)
    want = fc.expect_whole_contigs(g)[1 if peg else 0]
    c, strand, left, right = fc.whole_contig_locations(g)
    idx = np.arange(g.n_contig)
    if order == "shuffled":
        np.random.default_rng(77).shuffle(idx)
    locs = np.zeros(g.n_contig, kma.LOCATION_DTYPE)
    locs["contig"], locs["strand"], locs["left"], locs["right"] = c[idx], strand[idx], left[idx], \
        right[idx]
    want_len = np.array([len(w) for w in want], np.int64)[idx]
    empty = want_len == 0
    assert empty.mean() >= 0.30
    if order == "index":
        runs = np.diff(np.flatnonzero(np.concatenate([[True], ~empty, [True]]))) - 1
        assert runs.max() >= 50
    if name == "frag262k":
        assert want_len.sum() // fc.TR_TILE >= 100
    res, ooff = kma.translate_locations(g.dna, g.off, locs, 11, peg)
    assert (ooff.astype(np.int64) == np.concatenate([[0], np.cumsum(want_len)])).all()
    flat = "".join([want[i] for i in idx.tolist()]).encode("latin-1")
    assert len(res) == len(flat) + 32 and not res[len(flat):].any()
    got = res[:len(flat)]
    exp = np.frombuffer(flat, np.uint8)
    bad = np.flatnonzero(got != exp)
    assert len(bad) == 0, (len(bad), bad[:5])
    # the host restatement the projector documents agrees on a sample of the contigs
    contigs = fc.contig_strings(g)
    for j in idx[:300].tolist():
        loc = projector.Location(j, chr(strand[j]), 1, int(g.lens[j]))
        assert projector.peg_translate(contigs[j], loc, 11, peg) == want[j]


# ---- 8. end to end --------------------------------------------------------------------------------------------------

def test_project_genome_on_fragments(kma, oracle_c, small_gto):
    """project_genome with frag4k as the new genome (contig ids frag_0, frag_1, ...) and two close
    genomes: features, order, fig|...peg.N numbering, proteins and counters equal the oracle
    chain (C oracle join and sweep, the literal PegProposalList, the oracle's translation). The
    TreeSet orders by contig id string: frag_1000's features come before frag_2's."""
    from kmeranno import projector
    g = fc.frag4k(small_gto)
    want, counters, where = fc.expect_projection(oracle_c, small_gto)
    assert len(want) >= 200 and fc.features_out_of_index_order(where, g.ids) >= 2
    assert where != sorted(where)
    close = [fc.close_genome(small_gto, seed, gid) for seed, gid in fc.CLOSE_GENOMES]
    feats, got_counters = projector.project_genome(fc.new_genome(small_gto), close,
                                                   timestamp=fc.STAMP)
    assert len(feats) == len(want)
    bad = [(a, b) for a, b in zip(feats, want) if a != b]
    assert not bad, (len(bad), bad[:2])
    assert got_counters == counters
    assert [f["id"] for f in feats] == [f"fig|{small_gto['id']}.peg.{i + 1}"
                                        for i in range(len(feats))]
