"""The fragmented genomes of tests/fragment_cases.py meet the conditions tests/test_gpu_fragments.py
relies on, shown on the oracle alone (no GPU): every search branch the GPU tests are about is
reached by the offsets, and every comparison has enough expected hits, proposals and kept / rejected
ORFs to mean something. Each test prints the figures its conditions are about (pytest -s shows
them). A seed that misses a condition is a bug in the builder."""
import numpy as np

import fragment_cases as fc

TILE = fc.CONTIG_TILE


def test_frag4k_shape(small_gto):
    g = fc.frag4k(small_gto)
    src = fc.source_bases(small_gto)
    lens, off = g.lens, g.off.astype(np.int64)
    n = g.n_contig
    assert g.n_bases == len(src) == 768_718 and (g.dna[:g.n_bases] == src).all()
    short = ((lens >= 1) & (lens <= 47)).sum()
    empty = (lens == 0).sum()
    long_ = ((lens >= 400) & (lens <= 4000)).sum()
    print(f"frag4k: {n} contigs; 1..47 bases {short} ({short / n:.1%}), empty {empty} "
          f"({empty / n:.1%}), 400..4,000 bases {long_}")
    assert n >= 4200 and n > 4096 and short + empty + long_ == n
    assert 0.88 <= short / n <= 0.93 and 0.012 <= empty / n <= 0.02
    assert g.ids[17] == "frag_17" and sorted(g.ids) != g.ids
    assert lens[-1] == 0 and lens[-2] == 0
    # a dense run of >= 80 non-empty contigs of 1..14 bases from an index >= 4,096 on, inside one
    # tile: that tile meets more than 64 contigs, its neighbour's cached window is clamped
    d0, dn = g.dense_run
    run = lens[d0:d0 + dn]
    assert dn >= 80 and d0 >= 4096 and run.min() >= 1 and run.max() <= 14
    assert off[d0] // TILE == (off[d0 + dn] - 1) // TILE
    lo, nc = fc.probe_tiles(g.off)
    tile = int(off[d0] // TILE)
    assert nc[tile] > fc.OFF_CACHE and lo[tile + 1] + fc.OFF_CACHE > n and nc[tile + 1] <= fc.OFF_CACHE
    assert ((run >= 12).sum()) >= 20  # long enough for a K = 3 window on either strand
    print(f"dense run: contigs {d0}..{d0 + dn - 1} in tile {tile}, which meets {nc[tile]} contigs; "
          f"the next tile's window starts at contig {lo[tile + 1]} of {n}")
    # empty contigs around a tile boundary: one base before it, on it, one base after it
    eb = g.empty_at_boundary
    for name, rel in (("before", TILE - 1), ("at", 0), ("after", 1)):
        c = eb[name]
        assert lens[c] == 0 and off[c] % TILE == rel and 0 < off[c] < g.n_bases, name
        assert lens[c - 1] >= 1 and lens[c + 1] >= 1
    assert lens[eb["at"] + 1] >= 400  # a gene-bearing contig starts on that boundary
    # contigs whose last base lies 0, 1, 3K-1, 3K, 3K+2 bases past a tile boundary
    ends = off[1:][lens > 0] % TILE
    for past in fc.PAST:
        assert (ends == past).any(), past
        assert off[g.pair_ends[past] + 1] % TILE == past
    # translate locations: one per contig
    no_codon = lens < 3
    runs = np.diff(np.flatnonzero(np.concatenate([[True], ~no_codon, [True]]))) - 1
    print(f"whole-contig locations without a residue: {no_codon.mean():.1%}, longest run {runs.max()}")
    assert no_codon.mean() >= 0.30 and runs.max() >= 50
    paths = fc.probe_paths(g.off)
    print("probe paths (tiles):", paths, "wave search rounds:", fc.wave_search_rounds(n))
    assert paths["global"] >= 1 and paths["window"] >= 100 and paths["clamped"] >= 1
    assert fc.wave_search_rounds(n) == 3


def test_frag4k_half_empty(small_gto):
    g, h = fc.frag4k(small_gto), fc.frag4k_half_empty(small_gto)
    e0, en = h.empties
    off = h.off.astype(np.int64)
    assert h.n_contig == g.n_contig + 51 and (h.dna == g.dna).all()
    assert en == 50 and (h.lens[e0:e0 + en] == 0).all() and off[e0] == h.n_bases // 2
    # the host call cuts its two shards at the first offset >= half the bases: the run's first
    cut = int(np.searchsorted(off[1:], h.n_bases // 2, side="left")) + 1
    print(f"half-way base {h.n_bases // 2}: 50 empty contigs {e0}..{e0 + en - 1}, shard cut at {cut}")
    assert e0 <= cut <= e0 + en


def test_frag4k_join_and_proposals(oracle_c, small_gto):
    g = fc.frag4k(small_gto)
    (ct, lf, sd, fr, pg), peg_len = fc.expect_join(oracle_c, small_gto)
    on = np.unique(ct)
    high = int((ct > 4096).sum())
    print(f"join: {len(ct)} connections on {len(on)} contigs, {high} on contigs above index 4,096")
    assert len(ct) >= 50_000 and len(on) >= 500 and high >= 100
    strict = fc.expect_join(oracle_c, small_gto, True)[0]
    print(f"strict join: {len(strict[0])} connections")
    assert 1000 <= len(strict[0]) < len(ct)
    prop, stats = fc.expect_proposals(oracle_c, small_gto)
    pc = np.unique(prop["contig"])
    print(f"sweep: {len(prop['peg'])} proposals on {len(pc)} contigs, stats {stats.tolist()}")
    assert len(prop["peg"]) >= 5000 and len(pc) >= 100
    loose = fc.expect_proposals(oracle_c, small_gto, True)[0]
    print(f"loose sweep: {len(loose['peg'])} proposals")
    assert len(loose["peg"]) > len(prop["peg"])
    rows = fc.proposal_rows(prop)
    ext = fc.oracle_orf_rows(fc.contig_strings(g), rows)
    kept = sum(e[0] == fc.KEPT for e in ext)
    print(f"ORF extension: {kept} kept, {len(ext) - kept} rejected")
    assert kept >= 0.05 * len(ext) and len(ext) - kept >= 0.05 * len(ext)


def test_frag4k_probe_hits(oracle_c, small_gto):
    """K = 8 and K = 3 against half the genome's own kmers: expected hits in the tile that meets
    more than 64 contigs and on the contig just after the empty one on a tile boundary."""
    g = fc.frag4k(small_gto)
    off = g.off.astype(np.int64)
    _, nc = fc.probe_tiles(g.off)
    d0, dn = g.dense_run
    after_empty = g.empty_at_boundary["at"] + 1
    for k in (8, 3):
        ct, lf, sd, fr, fid = fc.expect_contigs(oracle_c, g, k)
        in_crowded = int((nc[fc.hit_tiles(off, ct, lf)] > fc.OFF_CACHE).sum())
        on_dense = int(((ct >= d0) & (ct < d0 + dn)).sum())
        print(f"K = {k}: {len(ct)} hits on {len(np.unique(ct))} contigs; {in_crowded} in tiles of more "
              f"than 64 contigs, {on_dense} on the dense run, {int((ct == after_empty).sum())} on the "
              f"contig after the boundary's empty one")
        assert len(ct) >= 100_000 and in_crowded >= 1 and (ct == after_empty).sum() >= 20
        assert set(sd.tolist()) == {ord("+"), ord("-")} and set(fr.tolist()) == {1, 2, 3}
        if k == 3:
            assert on_dense >= 20
    assert off[after_empty] % TILE == 0


def test_boundary_counts(oracle_c, small_gto):
    for n in fc.BOUNDARY_COUNTS:
        g = fc.boundary(small_gto, n)
        assert g.n_contig == n and g.lens[-1] >= 600
        last3 = np.flatnonzero(g.lens > 0)[-3:]
        paths = fc.probe_paths(g.off)
        rounds = fc.wave_search_rounds(n)
        for k in (8, 3):
            ct = fc.expect_contigs(oracle_c, g, k)[0]
            on_last = int(np.isin(ct, last3).sum())
            print(f"n = {n}, K = {k}: {g.n_bases} bases, {len(ct)} hits, {on_last} on the last three "
                  f"non-empty contigs; tiles {paths}, wave rounds {rounds}")
            assert on_last >= 20 and len(ct) >= 500
        assert (paths["ballot"] > 0) == (n < 64)
        assert rounds == (1 if n <= 64 else 2 if n <= 4096 else 3)


def test_frag262k(oracle_c, small_gto):
    g = fc.frag262k(small_gto)
    lens = g.lens
    genes = np.array(g.genes)
    tiny = np.delete(lens, genes)
    print(f"frag262k: {g.n_contig} contigs, {g.n_bases} bases, empty {np.mean(tiny == 0):.1%}, "
          f"tiny 1..6 bases {np.mean((tiny >= 1) & (tiny <= 6)):.1%}")
    assert g.n_contig == 64 ** 3 + 1 and tiny.max() <= 6
    assert 0.28 <= np.mean(tiny == 0) <= 0.32
    assert len(genes) == 20 and (lens[genes] >= 600).all() and (lens[genes] <= 2000).all()
    for p in (0, 1, 4095, 4096, 4097, 131_072, 262_142, 262_143, 262_144):
        assert p in g.genes
    assert fc.wave_search_rounds(g.n_contig) == 4 and fc.wave_search_rounds(64 ** 3) == 3
    # 4 is the most: a position in the first round's last slot (34 contigs wide) ends in 3
    rounds = fc.tile_search_rounds(g.off)
    print("wave search rounds per tile {rounds: tiles}:", rounds)
    assert set(rounds) == {3, 4} and rounds[4] >= 100 and rounds[3] >= 1
    paths = fc.probe_paths(g.off)
    print("probe paths (tiles):", paths)
    assert paths["global"] >= 100 and paths["window"] >= 5 and paths["clamped"] >= 1
    ct = fc.expect_contigs(oracle_c, g, 8)[0]
    per = [int((ct == p).sum()) for p in genes]
    print(f"K = 8: {len(ct)} hits; per gene-bearing contig {per}")
    assert per[0] >= 20 and per[-1] >= 20 and min(per) >= 20
    # translate: one location per contig
    no_codon = lens < 3
    runs = np.diff(np.flatnonzero(np.concatenate([[True], ~no_codon, [True]]))) - 1
    residues = int((lens // 3).sum())
    peg_residues = int(np.maximum(lens // 3 - 1, 0).sum())  # peg mode drops the last codon
    print(f"whole-contig locations without a residue: {no_codon.mean():.1%}, longest run "
          f"{runs.max()}; {residues} residues = {residues // fc.TR_TILE} translate tiles, in peg "
          f"mode {peg_residues} = {peg_residues // fc.TR_TILE} tiles")
    assert no_codon.mean() >= 0.30 and runs.max() >= 50
    assert residues // fc.TR_TILE >= 100 and peg_residues // fc.TR_TILE >= 100
    raw, peg = fc.expect_whole_contigs(g)
    assert sum(map(len, raw)) == residues and sum(map(len, peg)) == peg_residues


def test_synthetic_connections(oracle_c):
    dt = np.dtype([("contig", "<u4"), ("left", "<i4"), ("fid", "<u4"), ("strand", "u1"),
                   ("frame", "u1"), ("pad", "<u2")])
    h, peg_len = fc.synthetic_connections(dt)
    # contig runs inside one peg-and-strand list
    order = np.lexsort((h["left"], h["contig"], h["strand"], h["fid"]))
    s = h[order]
    new_list = np.concatenate([[True], (s["fid"][1:] != s["fid"][:-1])
                               | (s["strand"][1:] != s["strand"][:-1])])
    new_run = new_list | np.concatenate([[True], s["contig"][1:] != s["contig"][:-1]])
    run_len = np.diff(np.flatnonzero(np.concatenate([new_run, [True]])))
    runs_per_list = new_run.sum() / new_list.sum()
    print(f"synthetic: {len(h)} connections, {len(np.unique(h['contig']))} contigs, "
          f"{runs_per_list:.0f} contig runs per list, {np.mean(run_len <= 3):.1%} of 1..3")
    assert len(h) >= 190_000 and len(np.unique(h["contig"])) >= 4900
    assert runs_per_list >= 200 and np.mean(run_len <= 3) >= 0.9
    prop, stats = oracle_c.propose(h["contig"], h["left"], h["strand"], h["fid"], peg_len, fc.K)
    print(f"synthetic sweep: {len(prop['peg'])} proposals, stats {stats.tolist()}")
    assert stats[0] >= 500
    prop, stats = oracle_c.propose(h["contig"], h["left"], h["strand"], h["fid"], peg_len, fc.K,
                                   **fc.SYNTHETIC_LOOSE)
    print(f"synthetic sweep, loose: {len(prop['peg'])} proposals, stats {stats.tolist()}")
    assert len(prop["peg"]) >= 1000


def test_projection_chain(oracle_c, small_gto):
    """The oracle chain of the end-to-end test: enough kept features, and features on contigs
    whose id order ("frag_1000" < "frag_2") differs from their index order."""
    g = fc.frag4k(small_gto)
    want, counters, where = fc.expect_projection(oracle_c, small_gto)
    moved = fc.features_out_of_index_order(where, g.ids)
    print(f"projection: {len(want)} features on {len(set(where))} contigs, counters {counters}; "
          f"{moved} features on contigs whose id order differs from their index order")
    assert len(want) >= 200 and counters["merged"] >= 1 and counters["rejected"] >= 100
    # the default sweep proposes nothing with fewer than 10 kmers of evidence here, so the
    # min-evidence filter stays idle end to end (small = 0); the ORF tests' rows of evidence
    # 1..40 exercise it (test_frag4k_orf_extension asserts SMALL rows)
    assert counters["weak"] >= 100 and counters["small"] == 0
    assert moved >= 2 and where != sorted(where)
    assert [g.ids[c] for c in where] == sorted(g.ids[c] for c in where)
    assert all(f["protein_translation"] for f in want)
