"""§8(f)3 on a device-resident batch: kma_hash_annotate_indexed_device (genome_sets_kernel,
csrc/kma_hashsets.hip, then index_score_kernel unchanged) on torch device buffers in the layout
of annotate_proteins_device. Its best, sim, count and stats[0..2] must equal, exactly, the C
oracle's (orc_hash_annotate; it has no stats) and kma_hash_annotate_indexed's on the same index.
Before every call the scratch and all outputs are filled with 0xEE: the call reads no scratch it
has not written and writes every output itself. KMA_OPT_HASH_LDS_KEYS = 64 sends proteins of more
than 64 windows down the long-protein path (sorted runs, heads by search in the earlier runs)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)


@pytest.fixture(scope="module")
def kma(native_lib):
    import kmeranno
    assert kmeranno.device_count() >= 1
    return kmeranno


def _rand(rng, n):
    return AA[rng.integers(0, 20, n)].tobytes().decode()


def _mut(rng, p, rate):
    b = np.frombuffer(p.encode(), np.uint8).copy()
    m = rng.random(len(b)) < rate
    b[m] = AA[rng.integers(0, 20, int(m.sum()))]
    return b.tobytes().decode()


def poisoned(nbytes, dtype):
    return torch.full((max(nbytes, 16),), 0xEE, dtype=torch.uint8, device="cuda").view(dtype)


class DeviceBatch:
    """A batch on the device (res holds 32 readable bytes past off[-1]) with poisoned outputs."""

    def __init__(self, kma, res, off, n_proto, lo=0, hi=None):
        self.kma, self.off, self.lo = kma, off, lo
        self.hi = len(off) - 1 if hi is None else hi
        self.n_g, self.n_proto = self.hi - lo, n_proto
        self.n_res = int(off[self.hi] - off[lo])
        self.d_res = torch.from_numpy(np.ascontiguousarray(res)).cuda()
        self.d_off = torch.from_numpy(np.ascontiguousarray(off).view(np.int64)).cuda()
        self.sbytes = kma.hash_scratch_bytes(self.n_res, self.n_g)
        self.scratch = poisoned(self.sbytes, torch.uint8)
        self.best = poisoned(4 * self.n_g, torch.int32)
        self.sim = poisoned(8 * self.n_g, torch.float64)
        self.count = poisoned(4 * n_proto, torch.int32)
        self.stats = poisoned(32, torch.int64)

    def poison(self):
        for t in (self.scratch, self.best, self.sim, self.count, self.stats):
            t.view(torch.uint8).fill_(0xEE)

    def call(self, idx, min_sim=0.0125):
        self.kma.hash_annotate_indexed_device(
            idx, self.d_res.data_ptr(), self.d_off.data_ptr() + 8 * self.lo, self.n_g, self.n_res,
            self.scratch.data_ptr(), self.sbytes, self.best.data_ptr(), self.sim.data_ptr(),
            self.count.data_ptr(), self.stats.data_ptr(), min_sim,
            stream=torch.cuda.current_stream().cuda_stream)

    def results(self):
        torch.cuda.synchronize()
        return (self.best.cpu().numpy()[:self.n_g].copy(), self.sim.cpu().numpy()[:self.n_g].copy(),
                self.count.cpu().numpy().view(np.uint32)[:self.n_proto].copy(),
                self.stats.cpu().numpy().view(np.uint64)[:4].copy())


def device_run(kma, idx, res, off, n_proto, min_sim=0.0125, lo=0, hi=None):
    b = DeviceBatch(kma, res, off, n_proto, lo, hi)
    b.call(idx, min_sim)
    return b.results()


def assert_equal(got, host, oracle=None):
    """got = (best, sim, count, stats[4]) of the device entry; host = the host entry's four."""
    assert int(got[3][3]) == 0
    for a, b in zip(got[:3], host[:3]):
        assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all()
    assert got[3][:3].tolist() == host[3].tolist()
    if oracle is not None:
        for a, b in zip(got[:3], oracle):
            assert (a == b).all()


def check(kma, oracle_c, genome, protos, k, min_sim=0.0125, lds_keys=(0,), cap=0):
    """The device entry at every W of lds_keys against the oracle and the host entry."""
    g, go = kma.pack_strings(genome)
    p, po = kma.pack_strings(protos)
    oracle = oracle_c.hash_annotate(g, go, p, po, k, min_sim)
    with kma.ProtoIndex(p, po, k=k) as idx, kma.options(hash_cap=cap):
        host = kma.hash_annotate_indexed(idx, g, go, min_sim, stats=True)
        for w in lds_keys:
            with kma.options(hash_lds_keys=w):
                got = device_run(kma, idx, g, go, len(protos), min_sim)
            assert_equal(got, host, oracle)
    return got


def test_python_twin_shape(kma, oracle_c):
    """tests/test_gpu_hashindex.py's python-twin shape: 80 + 3 prototypes, 52 genome proteins
    with "ACDEFG" and "" among them, K = 8; at the default W and with every protein of more than
    64 windows on the long path."""
    rng = np.random.default_rng(3)
    base = [_rand(rng, rng.integers(60, 300)) for _ in range(80)]
    genome = [_mut(rng, p, 0.05) for p in base[:50]] + ["ACDEFG", ""]
    protos = [_mut(rng, p, 0.25) for p in base] + [base[3], base[3], "MMMMMMMMMMMMMMMMMMMMMMMMMMMM"]
    best, sim, cnt, st = check(kma, oracle_c, genome, protos, 8, lds_keys=(0, 64))
    assert best[3] == 80 and best[-1] == -1 and best[-2] == -1 and int(st[0]) > 40


@pytest.mark.parametrize("k", [2, 8, 12])
def test_window_count_edges_on_the_long_path(kma, oracle_c, k):
    """W = 64: proteins of exactly 63, 64, 65, 127, 128, 129 and 200 windows cut from the
    prototypes (each one's best match is the prototype it was cut from), one residue 300 times,
    a protein whose only repeat lies in chunks 0 and 2, L = K - 1, L = K, and empty proteins
    first, last and two adjacent."""
    rng = np.random.default_rng(60 + k)
    protos = [_rand(rng, 320) for _ in range(24)] + ["W" * 40]
    counts = (63, 64, 65, 127, 128, 129, 200)
    cut = [protos[i][:n + k - 1] for i, n in enumerate(counts)]
    rep = bytearray(protos[10][:3 * 64 + k - 1].encode())
    rep[2 * 64 + 9:2 * 64 + 29] = rep[3:23]
    genome = ["", cut[0], cut[1], "", "", cut[2], cut[3], "W" * 300, cut[4], rep.decode(),
              protos[11][:k - 1], protos[12][:k], cut[5], cut[6], ""]
    best, sim, cnt, st = check(kma, oracle_c, genome, protos, k, lds_keys=(64, 0, 128))
    assert best[[0, 3, 4, 10, 14]].tolist() == [-1] * 5
    if k >= 8:
        where = [1, 2, 5, 6, 8, 12, 13]
        assert best[where].tolist() == list(range(7)) and (sim[where] > 0.15).all()
        assert best[7] == 24 and best[9] == 10 and best[11] == -1  # (one window: below min_sim)


def test_long_protein_in_runs_and_in_prototype_ranges(kma, oracle_c):
    """test_indexed_edges' protein of ~20,000 residues (concatenated prototypes): 5 runs at the
    default W, and at KMA_OPT_HASH_CAP 16 the long path and range splitting together, with the
    host entry's stats[1]."""
    rng = np.random.default_rng(17)
    protos = [_rand(rng, 200) for _ in range(100)]
    protos[7] = "ACDEF"
    protos[40] = protos[12]
    long_one = "".join(protos)
    assert 4 * 4096 < len(long_one) - 7 <= 5 * 4096
    genome = [long_one, _rand(rng, 300), protos[12], "", protos[60][:150], "W" * 30]
    best, sim, cnt, st = check(kma, oracle_c, genome, protos, 8)
    assert best.tolist()[1:4] == [-1, 12, -1] and sim[2] == 1.0 and int(st[1]) == 0
    capped = check(kma, oracle_c, genome, protos, 8, cap=16, lds_keys=(0, 256))
    assert int(capped[3][1]) == 1 and (capped[0] == best).all() and (capped[2] == cnt).all()


def test_views_into_a_larger_batch(kma, oracle_c):
    """d_offsets points into the middle of a larger offsets array (offsets[0] = 37); other
    proteins' residues, lowercase bytes among them, lie before and after the view. No window of
    the view holds them: stats[3] stays 0 and the results equal the base-0 run's."""
    rng = np.random.default_rng(37)
    protos = [_rand(rng, rng.integers(40, 260)) for _ in range(40)]
    view = [_mut(rng, p, 0.1) for p in protos[:20]] + ["", "ACD", protos[30]]
    before = ["acdefghiklmnpqrstvwy", "lowercaseneighbour"[:17]]
    after = ["x" * 25, "mkvlaagivallmkv"]
    assert sum(len(s) for s in before) == 37
    res, off = kma.pack_strings(before + view + after)
    p, po = kma.pack_strings(protos)
    g0, go0 = kma.pack_strings(view)
    with kma.ProtoIndex(p, po, k=8) as idx:
        host = kma.hash_annotate_indexed(idx, g0, go0, stats=True)
        for w in (0, 64):
            with kma.options(hash_lds_keys=w):
                base0 = device_run(kma, idx, g0, go0, len(protos))
                got = device_run(kma, idx, res, off, len(protos), lo=2, hi=2 + len(view))
            assert int(off[2]) == 37
            assert_equal(base0, host, oracle_c.hash_annotate(g0, go0, p, po, 8, 0.0125))
            assert_equal(got, host)


def test_alphabet_flag_only_for_bytes_inside_windows(kma, oracle_c):
    """A lowercase byte inside a window sets stats[3]; the same byte in the 32-byte padding, or
    in a protein shorter than K, leaves it 0 and the results exact."""
    rng = np.random.default_rng(5)
    protos = [_rand(rng, 150) for _ in range(12)]
    genome = [protos[2][:100], "ACDEFG", protos[5], protos[7][20:]]
    p, po = kma.pack_strings(protos)
    g, go = kma.pack_strings(genome)
    with kma.ProtoIndex(p, po, k=8) as idx:
        host = kma.hash_annotate_indexed(idx, g, go, stats=True)
        for w in (0, 64):
            with kma.options(hash_lds_keys=w):
                inside = g.copy()
                inside[int(go[2]) + 90] = ord("k")
                assert int(device_run(kma, idx, inside, go, len(protos))[3][3]) != 0
                padding = g.copy()
                padding[int(go[-1]):] = ord("k")
                assert_equal(device_run(kma, idx, padding, go, len(protos)), host)
                short = g.copy()
                short[int(go[1]) + 2] = ord("k")
                assert_equal(device_run(kma, idx, short, go, len(protos)), host)


def test_two_calls_into_the_same_outputs(kma, oracle_c):
    """d_count is per call: a second genome into the same buffers gives its own counts."""
    rng = np.random.default_rng(9)
    protos = [_rand(rng, 120) for _ in range(30)]
    genomes = [[_mut(rng, p, 0.1) for p in protos[:12]], [_mut(rng, p, 0.1) for p in protos[8:20]]]
    p, po = kma.pack_strings(protos)
    with kma.ProtoIndex(p, po, k=8) as idx:
        packed = [kma.pack_strings(g) for g in genomes]
        assert packed[0][1].tolist() == packed[1][1].tolist()
        b = DeviceBatch(kma, packed[0][0], packed[0][1], len(protos))
        seen = []
        for g, go in packed + packed[:1]:
            b.d_res.copy_(torch.from_numpy(g))
            b.call(idx)  # (outputs as the call before left them)
            got = b.results()
            assert_equal(got, kma.hash_annotate_indexed(idx, g, go, stats=True),
                         oracle_c.hash_annotate(g, go, p, po, 8, 0.0125))
            seen.append(got[2])
    assert not (seen[0] == seen[1]).all() and (seen[0] == seen[2]).all() and seen[0].sum() >= 12


def test_no_prototypes_and_no_proteins(kma):
    g, go = kma.pack_strings(["ACDEFGHIKLMNPQ", "", "MKVLAAGIVALLMKV"])
    with kma.ProtoIndex.from_strings([]) as idx:
        b = DeviceBatch(kma, g, go, 0)
        kma.hash_annotate_indexed_device(
            idx, b.d_res.data_ptr(), b.d_off.data_ptr(), 3, b.n_res, b.scratch.data_ptr(),
            b.sbytes, b.best.data_ptr(), b.sim.data_ptr(), 0, b.stats.data_ptr(),
            stream=torch.cuda.current_stream().cuda_stream)
        best, sim, cnt, st = b.results()
        assert best.tolist() == [-1] * 3 and sim.tolist() == [0.0] * 3 and st.tolist() == [0] * 4
    with kma.ProtoIndex.from_strings(["ACDEFGHIKLMNPQ"]) as idx:
        b = DeviceBatch(kma, g, go, 1)
        kma.hash_annotate_indexed_device(idx, b.d_res.data_ptr(), b.d_off.data_ptr(), 0, 0,
                                         b.scratch.data_ptr(), b.sbytes, b.best.data_ptr(),
                                         b.sim.data_ptr(), b.count.data_ptr(), b.stats.data_ptr())
        torch.cuda.synchronize()  # nothing was enqueued: the poison is still there
        for t in (b.best, b.sim, b.count, b.stats, b.scratch):
            assert bool((t.view(torch.uint8) == 0xEE).all())
        b.call(idx)
        best, sim, cnt, st = b.results()
        assert best.tolist() == [0, -1, -1] and sim[0] == 1.0 and cnt.tolist() == [1]


def test_device_entry_in_a_captured_graph(kma):
    """One call captured on a side stream, replayed; then the residues are overwritten in place
    with a second genome of the same offsets and the graph is replayed again: each replay's
    outputs equal the host entry's for that genome."""
    rng = np.random.default_rng(23)
    protos = [_rand(rng, 180) for _ in range(60)]
    first = [_mut(rng, p, 0.1) for p in protos[:25]] + [_rand(rng, 4400)]
    second = [_mut(rng, p, 0.15) for p in protos[30:55]] + [_rand(rng, 4400)]
    p, po = kma.pack_strings(protos)
    (g1, go1), (g2, go2) = kma.pack_strings(first), kma.pack_strings(second)
    assert go1.tolist() == go2.tolist()
    with kma.ProtoIndex(p, po, k=8) as idx:
        hosts = [kma.hash_annotate_indexed(idx, g, go1, stats=True) for g in (g1, g2)]
        b = DeviceBatch(kma, g1, go1, len(protos))
        b.call(idx)  # (the module is loaded before the capture)
        assert_equal(b.results(), hosts[0])
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            b.call(idx)
        for g, host in ((g1, hosts[0]), (g2, hosts[1])):
            b.d_res.copy_(torch.from_numpy(g))
            b.poison()
            graph.replay()
            assert_equal(b.results(), host)
    assert not (hosts[0][0] == hosts[1][0]).all()


def test_low_complexity_scale(kma, oracle_c):
    """tests/test_gpu_hashindex.py's low-complexity shape (1,500 genome proteins x 3,000
    prototypes, a motif shared by a third of them), once at the defaults."""
    rng = np.random.default_rng(11)
    motif = "GGSGGSGGSGGSGGSGGS"
    base = [_rand(rng, rng.integers(50, 500)) + (motif if i % 3 == 0 else "") for i in range(1500)]
    protos = [_mut(rng, base[i % 1500], 0.3) for i in rng.permutation(3000)]
    st = check(kma, oracle_c, base, protos, 8)[3]
    assert int(st[0]) > 1400 and int(st[2]) == int(st[0])
