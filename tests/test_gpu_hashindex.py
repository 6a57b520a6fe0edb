"""§8(f)3 against a resident prototype index: kma_proto_index_create once, then
kma_hash_annotate_indexed per genome (one workgroup per genome protein counting shared kmers per
prototype in an LDS table; csrc/kma_hashindex.hip). Its three outputs must equal, exactly, the C
oracle's (orc_hash_annotate, all pairs) and kma_hash_annotate's, on the shapes of
tests/test_gpu_hashanno.py, with one index reused over several genomes, with the table forced to
overflow (KMA_OPT_HASH_CAP low: proteins scored in halved prototype ranges, ties across ranges),
and on the edges; out_stats is checked against a plain Python set model. Then the per-genome
report with an index, and the command `python -m kmeranno.hashanno` on a directory of genomes."""
import gzip
import json
import os

import numpy as np
import pytest

from oracle import oracle_py
from test_gpu_set_ops import BASE, batch_shapes, hash_shared_case, mutate, pack, shared_input

pytestmark = pytest.mark.gpu
AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)


@pytest.fixture(scope="module")
def kma(native_lib):
    import kmeranno
    assert kmeranno.device_count() >= 1
    return kmeranno


def _mut(rng, p, rate):
    b = np.frombuffer(p.encode(), np.uint8).copy()
    m = rng.random(len(b)) < rate
    b[m] = AA[rng.integers(0, 20, int(m.sum()))]
    return b.tobytes().decode()


def _rand(rng, n):
    return AA[rng.integers(0, 20, n)].tobytes().decode()


def distinct_candidates(genome, protos, k):
    """Per genome protein, the number of prototypes sharing at least one K-mer (set model)."""
    holders = {}
    for p, s in enumerate(protos):
        for kmer in {s[i:i + k] for i in range(len(s) - k + 1)}:
            holders.setdefault(kmer, []).append(p)
    out = []
    for s in genome:
        cand = set()
        for kmer in {s[i:i + k] for i in range(len(s) - k + 1)}:
            cand.update(holders.get(kmer, ()))
        out.append(len(cand))
    return np.array(out)


class Shape:
    """A genome and prototypes with the oracle's and kma_hash_annotate's answers, computed once
    and asserted equal; indexed() runs the indexed call and asserts its outputs equal both."""

    def __init__(self, kma, oracle_c, genome, protos, k, min_sim):
        self.kma, self.genome, self.protos, self.k, self.min_sim = kma, genome, protos, k, min_sim
        self.g, self.go = oracle_c.pack_strings(genome)
        self.p, self.po = oracle_c.pack_strings(protos)
        self.exp = oracle_c.hash_annotate(self.g, self.go, self.p, self.po, k, min_sim)
        self.plain = kma.hash_annotate(self.g, self.go, self.p, self.po, k, min_sim)
        for a, b in zip(self.plain, self.exp):
            assert (a == b).all()
        self._cand = None

    @property
    def cand(self):
        if self._cand is None:
            self._cand = distinct_candidates(self.genome, self.protos, self.k)
        return self._cand

    def index(self):
        return self.kma.ProtoIndex(self.p, self.po, k=self.k)

    def indexed(self, index=None, cap=None):
        """(best, sim, count, stats) of the indexed call: equal to the oracle and to
        kma_hash_annotate, stats against the set model at this CAP (None: the default)."""
        kma = self.kma
        own = index is None
        index = self.index() if own else index
        try:
            if cap is not None:
                kma.set_option(kma.OPT_HASH_CAP, cap)
            best, sim, cnt, st = kma.hash_annotate_indexed(index, self.g, self.go, self.min_sim,
                                                           stats=True)
        finally:
            kma.set_option(kma.OPT_HASH_CAP, 0)
            if own:
                index.close()
        for got, exp, plain in zip((best, sim, cnt), self.exp, self.plain):
            assert got.dtype == plain.dtype and (got == exp).all() and (got == plain).all()
        assert int(st[0]) == int((self.cand > 0).sum())
        assert int(st[1]) == int((self.cand > (cap or 1024)).sum())
        assert int(st[2]) >= int(st[0]) + int(st[1])
        if cap is None:  # no shape of this file has a protein of more than 1024 candidates
            assert int(st[1]) == 0
        return best, sim, cnt, st


def _small_gto_protos(small_gto):
    rng = np.random.default_rng(7)
    prots = [f["protein_translation"] for f in small_gto["features"]
             if f.get("protein_translation")]
    protos = [_mut(rng, p, rng.uniform(0.1, 0.4)) for p in prots]
    rng.shuffle(protos)
    return prots, protos + prots[:20] + prots[:5]


@pytest.mark.parametrize("k,min_sim", [(8, 0.0125), (8, 0.3), (5, 0.05), (12, 0.0)])
def test_indexed_small_gto_vs_oracle(kma, oracle_c, small_gto, k, min_sim):
    """test_gpu_hashanno.py's small.gto shape: prototypes = the proteins mutated 10-40%,
    shuffled, with exact copies and duplicates (the earlier prototype wins a tie)."""
    prots, protos = _small_gto_protos(small_gto)
    shape = Shape(kma, oracle_c, prots, protos, k, min_sim)
    best, sim, cnt, st = shape.indexed()
    assert (best[:5] >= len(protos) - 25).all() and (sim[:5] == 1.0).all()
    assert shape.cand.max() <= 281  # (K = 5: 281, the largest of this file)
    with shape.index() as idx:
        info = idx.info()
        assert info.n_proto == len(protos) and info.k == k and info.n_keys <= info.n_postings
        assert info.bytes == info.n_keys * 8 + (info.n_keys + 1) * 4 + info.n_postings * 4 \
            + info.n_proto * 4


def test_indexed_python_twin(kma, oracle_c):
    rng = np.random.default_rng(3)
    base = [_rand(rng, rng.integers(60, 300)) for _ in range(80)]
    genome = [_mut(rng, p, 0.05) for p in base[:50]] + ["ACDEFG", ""]
    protos = [_mut(rng, p, 0.25) for p in base] + [base[3], base[3], "MMMMMMMMMMMMMMMMMMMMMMMMMMMM"]
    best, sim, cnt, _ = Shape(kma, oracle_c, genome, protos, 8, 0.0125).indexed()
    pb, ps, pc = oracle_py.hash_annotate(genome, protos, 8, 0.0125)
    assert best.tolist() == pb and sim.tolist() == ps and cnt.tolist() == pc
    assert best[3] == 80 and best[-1] == -1 and best[-2] == -1


@pytest.fixture(scope="module")
def low_complexity(kma, oracle_c):
    """1,500 genome proteins x 3,000 prototypes with a low-complexity motif shared by a third of
    them (long postings, hundreds of candidates per protein)."""
    rng = np.random.default_rng(11)
    motif = "GGSGGSGGSGGSGGSGGS"
    base = [_rand(rng, rng.integers(50, 500)) + (motif if i % 3 == 0 else "") for i in range(1500)]
    protos = [_mut(rng, base[i % 1500], 0.3) for i in rng.permutation(3000)]
    return Shape(kma, oracle_c, base, protos, 8, 0.0125)


def test_indexed_low_complexity_and_scale(low_complexity):
    st = low_complexity.indexed()[3]
    assert int(st[0]) > 1400 and int(st[2]) == int(st[0])  # one range per protein with candidates


@pytest.mark.parametrize("cap,split", [(256, 458), (64, 500), (4, None)])
def test_forced_splitting_low_complexity(low_complexity, cap, split):
    """CAP below the motif proteins' candidate counts: they are scored in halved prototype ranges
    and nothing changes. The number of proteins that split is the set model's."""
    ref = low_complexity.indexed()
    got = low_complexity.indexed(cap=cap)
    for a, b in zip(got[:3], ref[:3]):
        assert (a == b).all()
    if split is not None:
        assert int(got[3][1]) == split
    assert int(got[3][1]) >= 458 and int(got[3][2]) > int(ref[3][2])


@pytest.fixture(scope="module")
def ties(kma, oracle_c, small_gto):
    """The ties shape of test_hash_scores_in_prototype_slices: exact copies of the first ten
    proteins at prototype indices 150..159 and again at the end."""
    rng = np.random.default_rng(21)
    prots = [f["protein_translation"] for f in small_gto["features"]
             if f.get("protein_translation")][:300]
    protos = [_mut(rng, p, rng.uniform(0.1, 0.4)) for p in prots]
    protos = protos[:150] + prots[:10] + protos[150:] + prots[:10]
    return Shape(kma, oracle_c, prots, protos, 8, 0.0125)


@pytest.mark.parametrize("cap", [4, 1])
def test_forced_splitting_ties_across_ranges(ties, cap):
    """The equal copies fall in different prototype ranges: a later range's equal similarity
    does not replace the running best, and the result equals the default-CAP run."""
    ref = ties.indexed()
    got = ties.indexed(cap=cap)
    for a, b in zip(got[:3], ref[:3]):
        assert (a == b).all()
    assert (got[0][:10] == np.arange(150, 160)).all() and (got[1][:10] == 1.0).all()
    # (no protein of this shape has more than 3 candidate prototypes: only CAP 1 splits)
    assert int(got[3][1]) == (14 if cap == 1 else 0)


def test_index_reuse_over_genomes(kma, oracle_c, small_gto):
    """One index, three different genomes, then the first again: every result equals the
    oracle's for that genome, and out_count is per call."""
    prots, protos = _small_gto_protos(small_gto)
    genomes = [prots[:200], prots[200:450], prots[450:], prots[:200]]
    shapes = [Shape(kma, oracle_c, g, protos, 8, 0.0125) for g in genomes[:3]]
    shapes.append(shapes[0])
    with shapes[0].index() as idx:
        counts = [s.indexed(index=idx)[2] for s in shapes]
    assert (counts[0] == counts[3]).all() and counts[0].sum() > 0
    assert not (counts[0] == counts[1]).all()


def test_indexed_edges(kma, oracle_c):
    """A prototype shorter than K, a genome protein sharing no kmer, an exact copy (1.0), an
    empty protein, and one protein of ~20,000 residues built from concatenated prototypes (78
    chunks of 256 keys, a candidate in most of them)."""
    rng = np.random.default_rng(17)
    protos = [_rand(rng, 200) for _ in range(100)]
    protos[7] = "ACDEF"
    protos[40] = protos[12]  # the earlier of two equal prototypes wins
    long_one = "".join(protos)
    assert 19_000 < len(long_one) < 20_100
    genome = [long_one, _rand(rng, 300), protos[12], "", protos[60][:150], "W" * 30]
    shape = Shape(kma, oracle_c, genome, protos, 8, 0.0125)
    best, sim, cnt, st = shape.indexed()
    assert best.tolist()[1:4] == [-1, 12, -1] and sim[2] == 1.0 and best[4] == 60 and best[5] == -1
    assert cnt[7] == 0 and shape.cand[0] == 99 and int(st[0]) == 3
    for cap in (16, 1):
        got = shape.indexed(cap=cap)
        assert (got[0] == best).all() and (got[1] == sim).all() and (got[2] == cnt).all()
        assert int(got[3][1]) == (1 if cap == 16 else 2)  # the long one; at CAP 1 also the copy


@pytest.mark.parametrize("k", [2, 8, 12])
def test_indexed_views_and_edge_batches(kma, oracle_c, k):
    """Both sides as views into larger buffers (offsets[0] = 37, other residues around them), on
    test_gpu_set_ops.py's shared proteins (a few dozen short ones) and its batch shapes on either
    side: an empty protein first, last and two adjacent, a side of only empty proteins, a side in
    which no protein reaches K. The index built from a view and queried with a view gives the
    oracle's and kma_hash_annotate's results on the same views, and those of the base-0 run."""
    genome, protos = hash_shared_case(k)
    small_g = [genome[i] for i in shared_input(k).small]
    small_p = [p for p in protos if len(p) < 1000]
    assert 30 <= len(small_g) <= 60 and 30 <= len(small_p) <= 60
    sides = [(small_g, small_p)]
    for batch in batch_shapes(k):
        sides += [(batch, [mutate(p, 3 * k, 1) for p in batch] + batch[:1]), (batch, small_p),
                  (small_g, batch)]
    annotated = 0
    for g, p in sides:
        runs = []
        for base in (BASE, 0):
            (gr, go), (pr, po) = pack(g, base), pack(p, base)
            assert int(go[0]) == int(po[0]) == base
            with kma.ProtoIndex(pr, po, k=k) as idx:
                got = kma.hash_annotate_indexed(idx, gr, go, 0.0125)
            for other in (oracle_c.hash_annotate(gr, go, pr, po, k, 0.0125),
                          kma.hash_annotate(gr, go, pr, po, k, 0.0125)):
                for a, b in zip(got, other):
                    assert (a == b).all(), (len(g), len(p), base)
            runs.append(got)
        for a, b in zip(*runs):
            assert (a == b).all(), (len(g), len(p))
        annotated += int((runs[0][0] >= 0).sum())
    assert annotated > 60  # (the shapes are not all empty: most short proteins find their copy)


def test_indexed_rejects_lowercase_on_either_side(kma):
    good = "ACDEFGHIKLMNPQRSTVWY"
    with pytest.raises(kma.KmerAnnoError) as e:
        kma.ProtoIndex.from_strings([good, "acdefghiklmnpqrstvwy"])
    assert e.value.code == kma.E_ALPHABET
    with kma.ProtoIndex.from_strings([good, good[::-1]]) as idx:
        res, off = kma.pack_strings([good, "acdefghiklmnpqrstvwy"])
        with pytest.raises(kma.KmerAnnoError) as e:
            kma.hash_annotate_indexed(idx, res, off)
        assert e.value.code == kma.E_ALPHABET
        best, sim, cnt = kma.hash_annotate_indexed(idx, *kma.pack_strings([good]))  # still usable
        assert best.tolist() == [0] and sim.tolist() == [1.0] and cnt.tolist() == [1, 0]


def _report_inputs(small_gto):
    from kmeranno import hashanno
    rng = np.random.default_rng(5)
    feats = [(f["id"], f.get("protein_translation", ""), f.get("function", ""))
             for f in small_gto["features"]]
    rows = [(_mut(rng, p, 0.1), func if i % 4 else f"renamed {i}")
            for i, (fid, p, func) in enumerate(feats) if p]
    rows.append(("ACDEFGHIKL" * 3, "too short"))
    rows.append((rows[0][0], " "))  # blank annotation: dropped
    return feats, rows, hashanno


def test_report_with_index_equals_report_without(kma, small_gto):
    feats, rows, hashanno = _report_inputs(small_gto)
    protos = hashanno.prototypes_from_rows(rows)
    plain = hashanno.annotate_genome(feats, protos)
    with hashanno.build_index(protos) as idx:
        assert hashanno.annotate_genome(feats, protos, index=idx) == plain
        assert hashanno.annotate_genome(feats[:100], protos, index=idx) == \
            hashanno.annotate_genome(feats[:100], protos)
    assert plain[1]["new"] == len(plain[2]) > 100


def test_command_on_a_directory_of_genomes(kma, small_gto, tmp_path):
    """python -m kmeranno.hashanno on three genomes cut from small.gto: one <id>.anno.tbl per
    genome with the header, changes.tbl with this run's changes in file-name order, and
    --missing annotating only the genome whose output is gone."""
    feats, rows, hashanno = _report_inputs(small_gto)
    in_dir, out_dir = tmp_path / "in", tmp_path / "out"
    in_dir.mkdir()
    anno = tmp_path / "roles.tbl"
    anno.write_text("id\tannotation\tprotein\n" +
                    "".join(f"r{i}\t{a}\t{p}\n" for i, (p, a) in enumerate(rows)))
    features = small_gto["features"]
    cuts = {"100.3": features[:250], "100.1": features[250:500], "100.2": features[500:]}
    for gid, part in cuts.items():
        doc = json.dumps({"id": gid, "scientific_name": "cut " + gid, "features": part})
        if gid == "100.2":
            with gzip.open(in_dir / f"{gid}.gto.gz", "wt") as f:
                f.write(doc)
        else:
            (in_dir / f"{gid}.gto").write_text(doc)
    assert hashanno.main([str(anno), str(in_dir), "-D", str(out_dir)]) == 0
    protos = hashanno.prototypes_from_rows(hashanno.read_annotation_file(str(anno)))
    assert protos == hashanno.prototypes_from_rows(rows)
    assert len(protos) == sum(len(p) >= 50 for p, _ in rows) - 1 < len(rows) - 2  # minLen, blank
    all_changes = {}
    for gid, part in cuts.items():
        f3 = [(f["id"], f.get("protein_translation", ""), f.get("function", "")) for f in part]
        lines, _, changes = hashanno.annotate_genome(f3, protos)
        text = (out_dir / f"{gid}.anno.tbl").read_text().split("\n")
        assert text[0] == hashanno.HEADER and text[1:-1] == lines and text[-1] == ""
        all_changes[gid] = changes
    want = [hashanno.HEADER] + all_changes["100.1"] + all_changes["100.2"] + all_changes["100.3"]
    assert (out_dir / "changes.tbl").read_text() == "\n".join(want) + "\n"
    assert sorted(os.listdir(out_dir)) == ["100.1.anno.tbl", "100.2.anno.tbl", "100.3.anno.tbl",
                                           "changes.tbl"]
    # --missing: only 100.2 is annotated again; the other outputs are not rewritten
    kept = (out_dir / "100.1.anno.tbl").read_text()
    (out_dir / "100.1.anno.tbl").write_text("kept\n")
    (out_dir / "100.2.anno.tbl").unlink()
    assert hashanno.main([str(anno), str(in_dir), "-D", str(out_dir), "--missing"]) == 0
    assert (out_dir / "100.1.anno.tbl").read_text() == "kept\n" and kept.startswith(hashanno.HEADER)
    assert (out_dir / "100.2.anno.tbl").read_text().split("\n")[0] == hashanno.HEADER
    assert (out_dir / "changes.tbl").read_text() == \
        "\n".join([hashanno.HEADER] + all_changes["100.2"]) + "\n"
    # --clear starts from an empty output directory
    assert hashanno.main([str(anno), str(in_dir), "-D", str(out_dir), "--clear", "-K", "8",
                          "--minSim", "0.0125", "--minLen", "50"]) == 0
    assert (out_dir / "100.1.anno.tbl").read_text() == kept
