"""GPU parity at K = 1..7: the protein kernel, the 6-frame probe and the peg join at the narrow
kmer sizes below ProteinKmers' default 8.

K is a property of the data (ApplyKmerProcessor.java:108 takes it from kmerdb.tbl's last row,
BuildKmerProcessor / KmerProcessor take -K, AppTest runs K = 4), and the library instantiates a
kernel per (K, layout). Below 8 the layout codes collapse (min(K, 6) = min(K, 7) up to K = 6),
tables shrink to a handful of buckets, a protein's windows are mostly duplicates, and the 6-frame
probe's halo, validity bounds and '-' frame all move with 3K. Every assertion here compares the
HIP path with the C oracle (or its Python twin), bit for bit.

The workload of `narrow_workload` is built over four disjoint five-letter alphabets so that
proteins are still called, ambiguous, below the minimum or unmatched at every K (the 20-letter
generator of kmeranno.synth calls nothing at K <= 2 and almost nothing at K = 5);
tests/test_narrow_k_workload.py checks that on the oracle alone.
"""
import functools
import types

import numpy as np
import pytest

from oracle import oracle_py

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 4, 5, 6, 7)
ROLE_ALPHABETS = ("ACDEF", "GHIKL", "MNPQR", "STVWY")
N_FID = len(ROLE_ALPHABETS)
MIN_HITS = 5
N_PROTEINS = 600
ROLE_SAMPLE = 20_000  # table rows drawn per role when 5^K is larger
AA20 = "ACDEFGHIKLMNPQRSTVWY"
# Forward positions per 6-frame probe block: kContigTile (csrc/kma_internal.h).
CONTIG_TILE = 1024


# ---- §1: a workload that works at every K -------------------------------------------------------

def _kmers_over(alphabet, idx, k):
    """The k-mers over a 5-letter alphabet with the base-5 indices idx."""
    a = np.frombuffer(alphabet.encode(), np.uint8)
    digits = (idx[:, None] // 5 ** np.arange(k - 1, -1, -1, dtype=np.int64)) % 5
    return [bytes(r).decode() for r in a[digits]]


def _narrow_rows(k, rng):
    """(kmer, fid) rows in file order, and the number of rows of another length."""
    rows = []
    for r, alphabet in enumerate(ROLE_ALPHABETS):
        n = 5 ** k
        idx = np.arange(n) if n <= ROLE_SAMPLE else np.sort(rng.choice(n, ROLE_SAMPLE, replace=False))
        if k > 1:
            idx = idx[rng.random(len(idx)) < 0.6]
        rows += [(km, r) for km in _kmers_over(alphabet, idx, k)]
    rows = [rows[i] for i in rng.permutation(len(rows))]
    # Every 50th row once more under another role; the last row of a kmer wins. The first such
    # copy and the copies of the last role's rows are appended (the kmer changes role, so the
    # last role's longer proteins turn ambiguous); the others go somewhere before their row (the
    # kmer keeps its role, unless a table takes the first row). Appending them all would leave
    # every role with foreign kmers among its own, and no protein of a hundred residues called.
    later, earlier = [], []
    for j, i in enumerate(range(0, len(rows), 50)):
        km, fid = rows[i]
        other = (fid + 1 + j % 3) % N_FID
        if j == 0 or fid == N_FID - 1:
            later.append((km, other))
        else:
            earlier.append((int(rng.integers(0, i + 1)), (km, other)))
    for at, row in sorted(earlier, reverse=True):
        rows.insert(at, row)
    rows += later
    off_length = [("ACDEFGHI"[:k - 1], 0), ("STVWYSTV"[:k + 1], 3), ("GHIKLGHI"[:k + 1], 1),
                  ("MNPQRMNP"[:k - 1], 2)]
    for j, row in enumerate(off_length):  # spread through the file, one of them last but one
        rows.insert(min(len(rows) - 1, (j * len(rows)) // 3), row)
    return rows, len(off_length)


def _narrow_proteins(k, rng):
    lengths = (0, k - 1, k, k + 1, k + 3, 30, 120, 400, 1500)
    weights = (0.07, 0.07, 0.09, 0.09, 0.09, 0.09, 0.13, 0.15, 0.22)
    letters = [np.frombuffer(a.encode(), np.uint8) for a in ROLE_ALPHABETS]
    foreign = np.frombuffer(b"BJOUZ", np.uint8)  # codable, never in the table
    noise = np.frombuffer(b"x*-X#", np.uint8)    # uncodable bytes and symbols the table lacks
    prots, kinds = [], []
    for _ in range(N_PROTEINS):
        n = int(rng.choice(lengths, p=weights))
        kind = int(rng.choice(5, p=(0.35, 0.2, 0.1, 0.2, 0.15)))
        r = int(rng.integers(0, N_FID))
        if kind == 0:    # one role: many repeated windows
            p = letters[r][rng.integers(0, 5, n)]
        elif kind == 1:  # a role-r stretch, then a role-(r+1) stretch: ambiguous
            cut = int(rng.integers(0, n + 1))
            p = np.concatenate([letters[r][rng.integers(0, 5, cut)],
                                letters[(r + 1) % N_FID][rng.integers(0, 5, n - cut)]])
        elif kind == 2:
            p = foreign[rng.integers(0, 5, n)]
        elif kind == 3:  # one role with about 10% of the bytes replaced
            p = letters[r][rng.integers(0, 5, n)].copy()
            m = rng.random(n) < 0.1
            p[m] = noise[rng.integers(0, 5, int(m.sum()))]
        else:            # a period-7 repeat of one 7-mer of the role
            p = np.tile(letters[r][rng.integers(0, 5, 7)], n // 7 + 1)[:n]
        prots.append(p.astype(np.uint8).tobytes().decode())
        kinds.append(kind)
    return prots, kinds


@functools.lru_cache(maxsize=None)
def narrow_workload(k, seed=7):
    """Table rows and 600 proteins over the four role alphabets, seeded per (seed, K)."""
    from oracle import c_oracle
    rng = np.random.default_rng([seed, k])
    rows, n_skipped = _narrow_rows(k, rng)
    prots, kinds = _narrow_proteins(k, rng)
    res, off = c_oracle.pack_strings(prots)
    for a in (res, off):
        a.flags.writeable = False
    return types.SimpleNamespace(
        k=k, rows=rows, kmers=[km for km, _ in rows], prots=prots, kinds=kinds,
        fids=np.array([f for _, f in rows], np.int32), res=res, off=off, n_skipped=n_skipped,
        n_entries=len({km for km, _ in rows if len(km) == k}))


_expected = {}


def oracle_apply(oracle_c, k, flags):
    """oracle_c.apply on narrow_workload(k), computed once per (K, flags) and left unchanged."""
    if (k, flags) not in _expected:
        wl = narrow_workload(k)
        e = oracle_c.apply(oracle_c.Table(wl.kmers, wl.fids), wl.res, wl.off, k, MIN_HITS, flags)
        for a in e:
            a.flags.writeable = False
        _expected[k, flags] = e
    return _expected[k, flags]


# ---- fixtures ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def kma(native_lib):
    import kmeranno
    assert kmeranno.device_count() >= 1
    return kmeranno


def _layouts(k):
    """The layout parameters that build different tables at this K: the size rule with two-choice
    placement, the size rule with overflow chains, flat; min(K, 6) and min(K, 7) differ at K = 7
    only (below it the minimizer is the whole key under both), so forcing them is a case of its
    own there alone."""
    return ["auto", "chained", "flat"] + (["m6", "m7"] if min(k, 6) != min(k, 7) else [])


K_LAYOUTS = [(k, name) for k in KS for name in _layouts(k)]


@pytest.fixture(params=K_LAYOUTS, ids=[f"k{k}-{name}" for k, name in K_LAYOUTS])
def k_layout(request):
    """(K, layout name) with KMA_OPT_LAYOUT / KMA_OPT_PLACEMENT set for the tables the test
    creates (read per table creation, reset after the test by conftest)."""
    import kmeranno
    kmeranno.load()
    k, name = request.param
    kmeranno.set_option(kmeranno.OPT_LAYOUT, {"auto": -1, "chained": -1, "flat": 0, "m6": 6,
                                              "m7": 7}[name])
    kmeranno.set_option(kmeranno.OPT_PLACEMENT, 0 if name == "chained" else -1)
    return k, name


@pytest.fixture(params=["direct", "defer"])
def path(request):
    """The protein kernel's grids: every group in block order, or short groups deferred to a
    second pass (forced on every batch)."""
    import kmeranno
    kmeranno.load()
    kmeranno.set_option(kmeranno.OPT_DEFER, 0 if request.param == "direct" else 2)
    return request.param


@pytest.fixture(params=["packed", "ascii"])
def input_mode(request):
    """Residues packed to 5 bits before the probe (KMA_OPT_PACKED_INPUT = 2), or ASCII packed by
    the probe itself (0)."""
    import kmeranno
    kmeranno.load()
    kmeranno.set_option(kmeranno.OPT_PACKED_INPUT, 2 if request.param == "packed" else 0)
    return request.param


def _check_layout_info(info, k, name):
    assert info.k == k
    assert info.minimizer_order == 0  # the mod-sampling order is K = 8's alone
    forced = {"flat": 0, "m6": min(k, 6), "m7": min(k, 7)}
    if name in forced:
        assert info.minimizer_len == forced[name]
    else:  # the size rule's code is one a kernel is instantiated for
        assert info.minimizer_len in (0, min(k, 6), min(k, 7))
    if name == "chained":
        assert info.two_choice == 0


def _assert_apply_equal(got, want, n_fid=None):
    fid, cnt, st = got[:3]
    efid, ecnt, est = want
    assert (st == est).all() and (fid == efid).all() and (cnt == ecnt).all()
    if n_fid is not None:
        assert (got[3] == np.bincount(efid[est == 1], minlength=n_fid)).all()


# ---- §2: protein apply ---------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, 1, 2])
def test_apply_narrow_k_vs_oracle(kma, oracle_c, k_layout, flags, path, input_mode):
    """600 proteins against the role-alphabet table at K = 1..7 under every layout distinct at
    that K, both grids, both input forms, both window conventions and multiset counting:
    status, fid, count and tally equal the oracle's; the table reports its K, a layout code a
    kernel takes, the distinct K-mers as entries and the rows of other lengths as skipped."""
    k, name = k_layout
    wl = narrow_workload(k)
    want = oracle_apply(oracle_c, k, flags)
    with kma.SignatureTable.from_rows(wl.kmers, wl.fids.astype(np.uint32), k) as t:
        i = t.info
        _check_layout_info(i, k, name)
        assert (i.n_rows, i.n_entries, i.n_skipped) == (len(wl.rows), wl.n_entries, wl.n_skipped)
        got = kma.annotate_proteins(t, wl.res, wl.off, MIN_HITS, flags, n_fid=N_FID)
    _assert_apply_equal(got, want, N_FID)


@pytest.mark.parametrize("k", [3, 7])
@pytest.mark.parametrize("defer", [1, 64])
def test_apply_narrow_k_block_capacities(kma, oracle_c, k, defer):
    """K != 8 has one kernel capacity (P = kBlockProteins): calls in a row on one table at 1, 4,
    5 and 8 proteins per block (partial and full blocks of it), with no group deferred (1 step)
    and every group deferred (64), each equal to the oracle."""
    wl = narrow_workload(k)
    want = oracle_apply(oracle_c, k, 0)
    kma.set_option(kma.OPT_DEFER, defer)
    with kma.SignatureTable.from_rows(wl.kmers, wl.fids.astype(np.uint32), k) as t:
        for bp in (1, 4, 5, 8):
            kma.set_option(kma.OPT_BLOCK_PROTEINS, bp)
            got = kma.annotate_proteins(t, wl.res, wl.off, MIN_HITS, 0, n_fid=N_FID)
            _assert_apply_equal(got, want, N_FID)


def _distinct_windows(p, k):
    b = np.frombuffer(p.encode(), np.uint8)
    w = np.lib.stride_tricks.sliding_window_view(b, k)
    return len(np.unique(w, axis=0))


@pytest.mark.parametrize("lf", [0.5, 0.95])
@pytest.mark.parametrize("k,keys", [(1, "all20"), (2, "all20"), (1, "one-fid"), (1, "eight")])
def test_apply_narrow_k_saturated_table(kma, oracle_c, k, keys, lf, path, input_mode):
    """A table holding every K-mer over the 20 standard residues (fid = the first residue's index
    mod 3): every codable window hits, so a protein over one fid's residues counts all its
    windows under KMA_F_MULTISET and its distinct windows (numpy) otherwise, including a
    70,000-residue one whose set lives in workspace memory. one-fid: the K = 1 table of fid 0's
    seven residues alone, which is a single bucket at load factor 0.95 and two at 0.5 (the
    creators then build it chained, or pair the two buckets); the 20 residues themselves do
    not fit two eight-slot buckets (they take 3 at load factor 0.95, 5 at 0.5). eight: the first
    eight residues, which at load factor 0.95 fill the single bucket's every slot, so that a
    miss finds no empty slot and ends at the table's size."""
    rng = np.random.default_rng(70 + k)
    aa = np.frombuffer(AA20.encode(), np.uint8)
    by_fid = [aa[f::3] for f in range(3)]
    table_aa = {"all20": aa, "one-fid": by_fid[0], "eight": aa[:8]}[keys]
    fid0_hits = set(by_fid[0].tolist()) <= set(table_aa.tolist())  # fid 0's residues all in the table
    grid = np.stack(np.meshgrid(*[np.arange(len(table_aa))] * k, indexing="ij"), -1).reshape(-1, k)
    kmers = [bytes(r).decode() for r in table_aa[grid]]
    fids = [AA20.index(km[0]) % 3 for km in kmers]
    prots = []
    for n in (0, k - 1, k, k + 1, 7, 64, 300, 1500):
        for f in range(3):
            prots.append(by_fid[f][rng.integers(0, len(by_fid[f]), n)].tobytes().decode())
        prots.append(aa[rng.integers(0, 20, n)].tobytes().decode())
    giant = by_fid[0][rng.integers(0, len(by_fid[0]), 70_000)].tobytes().decode()
    prots.insert(5, giant)
    noisy = np.frombuffer(prots[-4].encode(), np.uint8).copy()
    noisy[::9] = np.frombuffer(b"x*-X#bB", np.uint8)[np.arange(len(noisy[::9])) % 7]
    prots.append(noisy.tobytes().decode())
    res, off = oracle_c.pack_strings(prots)
    ot = oracle_c.Table(kmers, fids)
    with kma.SignatureTable.from_rows(kmers, fids, k, load_factor=lf) as t:
        i = t.info
        assert i.k == k and i.n_entries == len(table_aa) ** k and i.minimizer_order == 0
        assert i.n_buckets == kma.buckets_for(len(kmers), lf, k)
        if keys != "all20":
            assert i.n_buckets <= 2 and i.two_choice == (0 if i.n_buckets == 1 else 1)
        if kma.bucket_slots(k) == 8 and lf == 0.95:
            assert i.n_buckets == {"all20": 3 if k == 1 else 53, "one-fid": 1, "eight": 1}[keys]
        for flags in (0, 1, 2):
            got = kma.annotate_proteins(t, res, off, MIN_HITS, flags, n_fid=3)
            _assert_apply_equal(got, oracle_c.apply(ot, res, off, k, MIN_HITS, flags), 3)
            for j, p in enumerate(prots):
                if not fid0_hits:
                    break
                if set(p) <= set(by_fid[0].tobytes().decode()) and len(p) >= k + (flags == 1):
                    windows = len(p) - k + 1 - (flags == 1)
                    hits = windows if flags == 2 else _distinct_windows(p[:k - 1 + windows], k)
                    assert got[1][j] == hits and got[0][j] == 0, (j, flags)
    assert _distinct_windows(giant, k) <= 20 ** k and prots[5] is giant


def test_apply_narrow_k_device_entry_packed_equals_ascii(kma, oracle_c):
    """The _device entry on torch buffers at K = 5 with the ASCII probe (KMA_OPT_PACKED_INPUT 0)
    and the pack kernel first (2), on the whole batch and on a sub-batch whose first offset is
    not 0, and the packed-stream entry on that sub-batch packed on the host: all equal the
    oracle."""
    torch = pytest.importorskip("torch")
    k, k0 = 5, 7
    wl = narrow_workload(k)
    efid, ecnt, est = oracle_apply(oracle_c, k, 0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    n, n_res = len(wl.prots), int(wl.off[-1])
    assert wl.off[k0] > 0
    with kma.SignatureTable.from_rows(wl.kmers, wl.fids.astype(np.uint32), k) as t:
        ws = kma.Workspace(0, n_res, n)
        res = torch.from_numpy(wl.res.copy()).to(dev)
        off = torch.from_numpy(wl.off.view(np.int64).copy()).to(dev)
        for mode in (0, 2):
            kma.set_option(kma.OPT_PACKED_INPUT, mode)
            for lo in (0, k0):
                fid = torch.full((n,), -7, dtype=torch.int32, device=dev)
                cnt = torch.full((n,), -7, dtype=torch.int32, device=dev)
                st = torch.full((n,), 9, dtype=torch.uint8, device=dev)
                tally = torch.zeros(N_FID, dtype=torch.int32, device=dev)
                kma.annotate_proteins_device(t, ws, res.data_ptr(), off.data_ptr() + 8 * lo, n - lo,
                                             int(wl.off[-1] - wl.off[lo]), MIN_HITS, 0,
                                             fid.data_ptr(), cnt.data_ptr(), st.data_ptr(),
                                             tally.data_ptr(), N_FID, stream)
                torch.cuda.synchronize()
                got = (fid.cpu().numpy()[:n - lo], cnt.cpu().numpy()[:n - lo],
                       st.cpu().numpy()[:n - lo], tally.cpu().numpy())
                _assert_apply_equal(got, (efid[lo:], ecnt[lo:], est[lo:]), N_FID)
        # the sub-batch as a stream packed on the host (kma_annotate_packed_device)
        r0 = int(wl.off[k0])
        d_stream = torch.from_numpy(kma.pack_residues(t, wl.res[r0:n_res])).to(dev)
        outs = [torch.full((n,), 9, dtype=d, device=dev)
                for d in (torch.int32, torch.int32, torch.uint8)]
        kma.annotate_packed_device(t, ws, d_stream.data_ptr(), off.data_ptr() + 8 * k0, n - k0,
                                   n_res - r0, MIN_HITS, 0, *[o.data_ptr() for o in outs], 0, 0,
                                   stream)
        torch.cuda.synchronize()
        _assert_apply_equal([o.cpu().numpy()[:n - k0] for o in outs],
                            (efid[k0:], ecnt[k0:], est[k0:]))
        ws.close()


def test_table_from_tsv_takes_k_from_last_row(kma, oracle_c, tmp_path):
    """kma_table_create_from_tsv on the K = 5 rows written as a kmerdb.tbl (CRLF line ends, a
    third column on odd rows): the same roles, counts and apply outputs as the rows handed to
    kma_table_create (both equal to the oracle's), and the last row's kmer length reported as
    ApplyKmerProcessor.java:108 would use it, whatever that row's length."""
    k = 5
    wl = narrow_workload(k)
    names = [f"Role{chr(65 + f)}" for f in range(N_FID)]
    ids = {}
    for _, f in wl.rows:
        ids.setdefault(names[f], len(ids))
    first_seen = np.array([ids[names[f]] for f in range(N_FID)], np.int32)

    def write(path, rows):
        path.write_bytes("".join(
            f"{km}\t{names[f]}" + ("\tthird column" if j % 2 else "") + "\r\n"
            for j, (km, f) in enumerate(rows)).encode())

    write(tmp_path / "kmerdb.tbl", wl.rows)
    t, roles, last = kma.SignatureTable.from_tsv(str(tmp_path / "kmerdb.tbl"), k)
    assert roles == list(ids) and last == len(wl.rows[-1][0]) == k
    efid, ecnt, est = oracle_apply(oracle_c, k, 0)
    with t, kma.SignatureTable.from_rows(wl.kmers, first_seen[wl.fids].astype(np.uint32), k) as ref:
        a, b = t.info, ref.info
        assert (a.n_rows, a.n_skipped, a.n_entries, a.n_extra_syms, a.k) == \
            (b.n_rows, b.n_skipped, b.n_entries, b.n_extra_syms, b.k) == \
            (len(wl.rows), wl.n_skipped, wl.n_entries, 0, k)
        for tab in (t, ref):
            got = kma.annotate_proteins(tab, wl.res, wl.off, MIN_HITS, 0, n_fid=N_FID)
            want_fid = np.where(efid < 0, efid, first_seen[np.maximum(efid, 0)]).astype(np.int32)
            _assert_apply_equal(got, (want_fid, ecnt, est), N_FID)
    for tail in ("ACD", "ACDEFGH", "ACDEFGHIKL"):
        write(tmp_path / "other.tbl", wl.rows + [(tail, 0)])
        with_tail, _, last = kma.SignatureTable.from_tsv(str(tmp_path / "other.tbl"), k)
        with with_tail:
            assert last == len(tail)
            assert with_tail.info.n_skipped == wl.n_skipped + 1


# ---- §3: 6-frame probe ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _contig_strings(k):
    """About 70 kb of small.gto's DNA cut to this K's edges (see test_contigs_narrow_k_vs_oracle)."""
    import gzip
    import json
    import os
    from conftest import GOLDEN
    with gzip.open(os.path.join(GOLDEN, "small.gto.gz"), "rt") as f:
        src = [c["dna"] for c in json.load(f)["contigs"]]
    a, b = src[0][2000:32000], src[1][5000:35000]
    contigs = [a, b[:17000] + "nnnNacgtRYk" + b[17000:]]
    contigs += [src[0][100:100 + n] for n in range(max(0, 3 * k - 4), 3 * k + 12)]
    contigs += ["n" * (3 * k + 40), ""]
    # 90 short contigs from a tile boundary on, under 1,024 bases together: all of them meet one
    # tile (more than the 64 whose offsets a block caches); every third is long enough for hits
    total = sum(len(c) for c in contigs)
    contigs.append(src[2][:CONTIG_TILE + (-total) % CONTIG_TILE])
    short = [3 * k + 3 + i % 4 if i % 3 == 0 else i % 7 for i in range(90)]
    assert sum(short) < CONTIG_TILE
    contigs += [src[2][2000 + 50 * i:2000 + 50 * i + n] for i, n in enumerate(short)]
    # contigs whose last base lies 0, 1, 3K-1, 3K and 3K+2 bases past a tile boundary of the
    # concatenated bases (the probe tiles them, not each contig)
    total = sum(len(c) for c in contigs)
    for past in (0, 1, 3 * k - 1, 3 * k, 3 * k + 2):
        n = CONTIG_TILE + 200 + (past - (total + CONTIG_TILE + 200)) % CONTIG_TILE
        contigs.append(src[3][3000:3000 + n])
        total += n
        assert total % CONTIG_TILE == past % CONTIG_TILE
    return tuple(contigs)


_contig_cases = {}


def _contig_case(oracle_c, k, gcode):
    """DNA, the oracle's kmer records, the sampled and (K <= 4) saturated tables and the oracle's
    hits on each, once per (K, genetic code)."""
    if (k, gcode) not in _contig_cases:
        contigs = _contig_strings(k)
        dna, off = oracle_c.pack_strings(contigs)
        km = oracle_c.contig_kmers(dna, off, gcode, k)[0]
        rng = np.random.default_rng([k, gcode])
        tables = {}
        pick = np.flatnonzero(rng.random(len(km)) < 0.5)
        tables["sample"] = ([bytes(r).decode() for r in km[pick]],
                            rng.integers(0, 300, len(pick)).astype(np.int32))
        if k <= 4:
            uniq = np.unique(km, axis=0)
            tables["saturated"] = ([bytes(r).decode() for r in uniq],
                                   rng.integers(0, 300, len(uniq)).astype(np.int32))
        expected = {name: oracle_c.annotate_contigs(oracle_c.Table(kmers, fids), dna, off, gcode, k)
                    for name, (kmers, fids) in tables.items()}
        _contig_cases[k, gcode] = types.SimpleNamespace(
            contigs=contigs, dna=dna, off=off, n_records=len(km), tables=tables, expected=expected)
    return _contig_cases[k, gcode]


def _assert_hits_equal(hits, e):
    assert len(hits) == len(e[0])
    for a, b in zip((hits["contig"], hits["left"], hits["strand"], hits["frame"], hits["fid"]), e):
        assert (a == b).all()


@pytest.mark.parametrize("gcode", [11, 4])
def test_contigs_narrow_k_vs_oracle(kma, oracle_c, k_layout, gcode):
    """The 6-frame probe at K = 1..7 on 30 kb slices of two small.gto contigs (ambiguous bases
    spliced into one), contigs of every length from 3K-4 to 3K+11 bases, 70 short contigs (more
    than 64 contigs, and more than 64 in one tile: the offset search), an all-'n' and an empty
    contig, and contigs ending 0, 1, 3K-1, 3K and 3K+2 bases past a tile boundary; against half
    of their own kmer records (random fids, last row wins) and, for K <= 4, against every kmer
    they hold, where each probed window hits (full staging records, and more hits than the host
    wrapper's first capacity, so it regrows): hits and tally equal the oracle's, and a hit's
    kmer is the translation of the DNA at its location (AppTest.java:131-138)."""
    k, name = k_layout
    c = _contig_case(oracle_c, k, gcode)
    windows = kma.contig_window_count(c.off, k)
    assert len(c.contigs) > 100 and c.n_records > 100_000
    assert len(c.dna) - 32 == c.off[-1] <= 80_000
    for tname, (kmers, fids) in c.tables.items():
        e = c.expected[tname]
        with kma.SignatureTable.from_rows(kmers, fids.astype(np.uint32), k) as t:
            _check_layout_info(t.info, k, name)
            assert t.info.n_entries == len(set(kmers))
            hits, tally = kma.annotate_contigs(t, c.dna, c.off, gcode, n_fid=300)
        _assert_hits_equal(hits, e)
        expect = np.zeros((len(c.contigs), 300), np.uint32)
        np.add.at(expect, (e[0], e[4]), 1)
        assert (tally == expect).all()
        if tname == "saturated":
            assert len(hits) == c.n_records and len(hits) > windows // 8
        tab = set(kmers)
        rng = np.random.default_rng(k)
        for h in hits[rng.choice(len(hits), 300, replace=False)]:
            seq = c.contigs[h["contig"]][h["left"] - 1:h["left"] - 1 + 3 * k]
            if h["strand"] == ord("-"):
                seq = oracle_py.reverse_complement(seq)
            assert oracle_py.translate(seq, 1, gcode) in tab


def test_contigs_narrow_k_device_cap(kma, oracle_c):
    """kma_annotate_contigs_device at K = 2 with the saturated table: the published total is
    the oracle's whether the hits fit (cap = total + 5) or not (cap = 100), the first
    min(cap, total) hits are the oracle's, and the 16 records past cap stay untouched."""
    torch = pytest.importorskip("torch")
    k = 2
    c = _contig_case(oracle_c, k, 11)
    kmers, fids = c.tables["saturated"]
    e = c.expected["saturated"]
    total = len(e[0])
    assert total == c.n_records
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    n_bases = int(c.off[-1])
    with kma.SignatureTable.from_rows(kmers, fids.astype(np.uint32), k) as t:
        ws = kma.Workspace(0)
        ws.reserve_contigs(n_bases)
        d_dna = torch.from_numpy(c.dna).to(dev)
        d_off = torch.from_numpy(c.off.view(np.int64)).to(dev)
        d_nh = torch.zeros(1, dtype=torch.int64, device=dev)
        for cap in (total + 5, 100):
            d_hits = torch.zeros((cap + 16) * kma.HIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            kma.annotate_contigs_device(t, ws, d_dna.data_ptr(), d_off.data_ptr(), len(c.contigs),
                                        n_bases, 11, d_hits.data_ptr(), cap, d_nh.data_ptr(), 0, 0,
                                        stream)
            torch.cuda.synchronize()
            assert int(d_nh.item()) == total
            assert not d_hits[cap * kma.HIT_DTYPE.itemsize:].any()
            n = min(cap, total)
            hits = d_hits.cpu().numpy().view(kma.HIT_DTYPE)[:n]
            for a, b in zip((hits["contig"], hits["left"], hits["strand"], hits["frame"],
                             hits["fid"]), e):
                assert (a == b[:n]).all()
        ws.close()


# ---- §4: peg join --------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [4, 6])
@pytest.mark.parametrize("strict", [False, True])
def test_peg_connect_narrow_vs_oracle(kma, oracle_c, small_gto, k, strict):
    """KmerProcessor.java:195-207 at -K 4 (AppTest's size) and 6: singleton peg kmers of a
    mutated copy of small.gto's pegs joined with the 6-frame kmer map of 60 kb of
    its contigs, AGGRESSIVE and STRICT, equal to the oracle's connections."""
    rng = np.random.default_rng(100 + k)
    aa = np.frombuffer(AA20.encode(), np.uint8)
    prots = [f["protein_translation"] for f in small_gto["features"]
             if f.get("protein_translation")]
    close = []
    for p in prots:
        b = np.frombuffer(p.encode(), np.uint8).copy()
        m = rng.random(len(b)) < 0.04
        b[m] = aa[rng.integers(0, 20, int(m.sum()))]
        close.append(b.tobytes().decode())
    close[3] = close[3][:40] + "XXX" + close[3][40:]
    close += prots[:4] + ["", "ACDEFGHIKLMN"[:k], "ACDEFGHIKLMN"[:k + 1], "XXXXXXXXXXXXXXXX"]
    res, off = oracle_c.pack_strings(close)
    dna, doff = oracle_c.pack_strings([c["dna"][:30000] for c in small_gto["contigs"][:2]])
    e = oracle_c.peg_connect(res, off, dna, doff, 11, k, strict)
    assert len(e[0]) > 5_000
    t, n_win = kma.SignatureTable.from_pegs(res, off, k)
    assert n_win == sum(max(len(p) - k, 0) for p in close)
    with t:
        assert t.info.k == k and t.info.minimizer_order == 0
        hits = kma.connect_pegs(t, dna, doff, 11, strict)
    _assert_hits_equal(hits, e)
