"""GPU parity over the whole 5-bit residue field.

Every packed key is built from 5-bit residue codes ('A'..'Z' -> 1..26, '*' -> 27, up to four
other table bytes -> 28..31, 0 = no code), and each kernel family has its own byte-to-code step:
the ASCII staged probe, the device pack kernel, the host packer, kma_pack_kmers, the peg, build,
distance and hash-annotate window packers. The other GPU workloads draw from the twenty letters
ACDEFGHIKLMNPQRSTVWY. Here the tables and proteins of tests/alphabet_cases.py hold all 27
standard symbols and the extra symbols '-', '1', 'a' and 0xC3 (codes 28..31: a lower-case letter
that must not fold into 'A', and a byte >= 128 as the all-ones code), keys up to 2^(5K) - 1, key
bytes 0xF8..0xFF next to the slot's fid, mod-sampling ties, and windows whose key is not 0 but
has a zero low dword (the empty-slot test). tests/test_alphabet_workload.py shows on the oracle
alone that these workloads are not degenerate. Expected values are the C oracle's, numpy
restatements of the documented formats, or the input rows; never the library's.
"""
import numpy as np
import pytest

import alphabet_cases as ac
from helpers import unpack_keys
from test_gpu_id_range import decode_slots

pytestmark = pytest.mark.gpu

F_MULTISET = 2
MIN_HITS = ac.MIN_HITS


@pytest.fixture(scope="module")
def kma(native_lib):
    import kmeranno
    assert kmeranno.device_count() >= 1
    return kmeranno


@pytest.fixture(params=["auto", "6", "7", "0", "chained"],
                ids=["m-auto", "m6-random", "m7", "flat", "chained"])
def layout(request):
    """The size rule's layout with two-choice placement (at K = 8 the mod-sampling order), m = 6 in
    the smallest-hash order, m = 7, flat, and the size rule's layout with overflow chains
    (KMA_OPT_PLACEMENT = 0); at K = 5 the minimizer lengths 6 and 7 both mean 5."""
    import kmeranno
    kmeranno.load()
    p = request.param
    kmeranno.set_option(kmeranno.OPT_LAYOUT, -1 if p in ("auto", "chained") else int(p))
    kmeranno.set_option(kmeranno.OPT_PLACEMENT, 0 if p == "chained" else -1)
    return p


@pytest.fixture(params=["direct", "defer"])
def path(request):
    """The protein kernel's grids: every group in block order, or short groups deferred to a
    second pass (forced on every batch)."""
    import kmeranno
    kmeranno.load()
    kmeranno.set_option(kmeranno.OPT_DEFER, 0 if request.param == "direct" else 2)
    return request.param


@pytest.fixture(params=[0, 1, 2], ids=["ascii", "default", "packed"])
def input_mode(request):
    """KMA_OPT_PACKED_INPUT: ASCII packed by the probe itself through the LDS LUT (0), the
    default (1: the host call packs while it stages), residues packed to 5 bits first (2)."""
    import kmeranno
    kmeranno.load()
    kmeranno.set_option(kmeranno.OPT_PACKED_INPUT, request.param)
    return request.param


def _assert_apply_equal(got, want, n_fid=None):
    fid, cnt, st = got[:3]
    efid, ecnt, est = want
    assert (st == est).all() and (fid == efid).all() and (cnt == ecnt).all()
    assert not (fid == 0).any()  # a false match on an empty slot would show as fid 0
    if n_fid is not None:
        assert (got[3] == np.bincount(efid[est == 1], minlength=n_fid)).all()


def _check_info(info, wl):
    assert info.k == wl.k
    assert (info.n_rows, info.n_entries, info.n_skipped) == (len(wl.rows), len(wl.table),
                                                             wl.n_skipped)
    want = ac.EXTRA if wl.extra else b""
    assert info.n_extra_syms == len(want) and bytes(info.extra_syms)[:len(want)] == want


# ---- a. apply parity -------------------------------------------------------------------------------

@pytest.mark.parametrize("lf", [0.5, 0.95])
@pytest.mark.parametrize("extra", [False, True], ids=["std", "extra"])
@pytest.mark.parametrize("k", ac.KS)
def test_apply_alphabet_vs_oracle(kma, oracle_c, layout, path, input_mode, k, extra, lf):
    """The 1,500 proteins against the table over all 27 (31) symbols under every layout and
    placement, both grids, the three input forms, at load factor 0.5 and 0.95, set and multiset
    counting, 1 and 6 proteins per block: status, fid, count and tally equal the oracle's, no
    output has fid 0, and the table reports its rows, its distinct K-length kmers and the four
    extra symbols in byte order."""
    wl = ac.workload(k, extra)
    forced = [None]
    if layout == "auto" and k == 8:  # the creators may leave the size rule's order: force it too
        forced.append(6 | kma.LAYOUT_MOD_SAMPLING)
    for code in forced:
        if code is not None:
            kma.set_option(kma.OPT_LAYOUT, code)
        with kma.SignatureTable.from_rows(wl.kmers, wl.fids.astype(np.uint32), k,
                                          load_factor=lf) as t:
            info = t.info
            _check_info(info, wl)
            if code is not None:
                assert info.minimizer_len == 6 and info.minimizer_order != 0
            if layout == "chained":
                assert info.two_choice == 0
            if layout == "0":
                assert info.minimizer_len == 0
            for flags in (0, F_MULTISET):
                want = ac.oracle_apply(oracle_c, k, extra, flags)
                for bp in (1, 6):
                    kma.set_option(kma.OPT_BLOCK_PROTEINS, bp)
                    got = kma.annotate_proteins(t, wl.res, wl.off, MIN_HITS, flags, n_fid=ac.N_FID)
                    _assert_apply_equal(got, want, ac.N_FID)


# ---- b. device entries, the packed stream and kma_pack_kmers ---------------------------------------

def stream_bytes(codes, n_bytes):
    """The packed residue stream of include/kmeranno.h restated: residue j is the 5-bit code at
    bits [5j, 5j + 5) of a big-endian bit stream (8 residues = 5 bytes, the first residue most
    significant), zero to the end of its n_bytes."""
    c = np.zeros(-(-len(codes) // 8) * 8, np.uint64)
    c[:len(codes)] = codes
    c = c.reshape(-1, 8)
    v = np.zeros(len(c), np.uint64)
    for j in range(8):
        v = (v << np.uint64(5)) | c[:, j]
    out = np.zeros(n_bytes, np.uint8)
    for b in range(5):
        out[b:5 * len(c):5] = ((v >> np.uint64(32 - 8 * b)) & np.uint64(0xFF)).astype(np.uint8)
    return out


def packed_rows(rows, k, lut):
    """kma_pack_kmers restated: the key of a K-length row whose bytes all have codes, else 0."""
    keys = np.zeros(len(rows), np.uint64)
    for i, r in enumerate(rows):
        c = lut[np.frombuffer(r, np.uint8)]
        if len(r) == k and (c != 0).all():
            keys[i] = int(ac.pack_codes(c[None, :])[0])
    return keys


@pytest.mark.parametrize("k,extra", [(8, True), (8, False), (7, True), (5, True)],
                         ids=["k8-extra", "k8-std", "k7-extra", "k5-extra"])
def test_device_entries_and_packed_stream(kma, oracle_c, k, extra):
    """kma_annotate_proteins_device on torch buffers with the ASCII probe and with the pack kernel
    first, and kma_annotate_packed_device on the kma_pack_residues stream of the same residues,
    each on uneven sub-batches whose d_offsets[0] is not 0: all equal the oracle; the stream
    equals the numpy restatement of its format byte for byte, and kma_pack_kmers the restated
    keys of the table's rows and of rows that hold bytes without a code."""
    torch = pytest.importorskip("torch")
    wl = ac.workload(k, extra)
    lut = ac.code_of(extra)
    want = ac.oracle_apply(oracle_c, k, extra, 0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    n, n_res = len(wl.prots), int(wl.off[-1])
    cuts = [0, 1, 2, 7, 300, 301, 811, 1100, n]
    assert wl.off[1] > 0 and cuts == sorted(set(cuts))
    with kma.SignatureTable.from_rows(wl.kmers, wl.fids.astype(np.uint32), k) as t:
        _check_info(t.info, wl)
        rows = wl.kmers + [b"acdefghi"[:k], b"ACDE#GHI"[:k], b"\xc3" * k, b"-1a\xc3-1a\xc3"[:k],
                           b"A" * (k + 1), b""]
        keys = t.pack(rows)
        assert (keys == packed_rows(rows, k, lut)).all()
        assert (keys != 0).sum() == len(rows) - wl.n_skipped - (6 if not extra else 4)
        if extra:
            assert int(keys.max()) == (1 << (5 * k)) - 1
        ws = kma.Workspace(0, n_res, n)
        d_res = torch.from_numpy(wl.res.copy()).to(dev)
        d_off = torch.from_numpy(wl.off.view(np.int64).copy()).to(dev)
        for mode in (0, 2, "stream"):
            if mode != "stream":
                kma.set_option(kma.OPT_PACKED_INPUT, mode)
            outs = [torch.full((n,), 9, dtype=d, device=dev)
                    for d in (torch.int32, torch.int32, torch.uint8)]
            tally = torch.zeros(ac.N_FID, dtype=torch.int32, device=dev)
            keep = []
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                r0, r1 = int(wl.off[lo]), int(wl.off[hi])
                ptrs = (outs[0].data_ptr() + 4 * lo, outs[1].data_ptr() + 4 * lo,
                        outs[2].data_ptr() + lo, tally.data_ptr(), ac.N_FID, stream)
                if mode == "stream":
                    host = kma.pack_residues(t, wl.res[r0:r1])
                    assert len(host) == kma.packed_bytes(r1 - r0) == 40 * (-(-(r1 - r0) // 64)) + 16
                    assert (host == stream_bytes(lut[wl.res[r0:r1]], len(host))).all(), (lo, hi)
                    d_stream = torch.from_numpy(host).to(dev)
                    keep.append(d_stream)
                    kma.annotate_packed_device(t, ws, d_stream.data_ptr(), d_off.data_ptr() + 8 * lo,
                                               hi - lo, r1 - r0, MIN_HITS, 0, *ptrs)
                else:
                    kma.annotate_proteins_device(t, ws, d_res.data_ptr(), d_off.data_ptr() + 8 * lo,
                                                 hi - lo, r1 - r0, MIN_HITS, 0, *ptrs)
            torch.cuda.synchronize()
            got = [o.cpu().numpy() for o in outs] + [tally.cpu().numpy()]
            _assert_apply_equal(got, want, ac.N_FID)
        ws.close()


# ---- c. slot dump ----------------------------------------------------------------------------------

def _dump_proteins(keys, k):
    """One protein per key (its text under the EXTRA symbols) and chains of six keys."""
    text = ac.codes_text(ac.key_codes(keys, k))
    prots = [r.tobytes() for r in text]
    prots += [text[i:i + 6].tobytes() for i in range(0, len(text) - 6, 41)]
    return prots


@pytest.mark.parametrize("k,layout_name", [(8, "two-choice"), (8, "two-choice-mod"),
                                           (8, "chained"), (8, "flat"), (12, "chained")])
def test_build_device_slot_dump_all_codes(kma, oracle_c, k, layout_name):
    """kma_table_build_device at load factor 0.9 on keys over all 31 residue codes (2^(5K) - 1,
    first residues of code 31 whose key byte next to the fid is 0xF8..0xFF, mod-sampling ties,
    repeated keys): the decoded slots hold exactly the last-wins (key, fid) pairs. At K = 8 the
    wrapped table, probed through the packed-stream entry with one protein per key and chains of
    keys, and through the ASCII entry (a wrapped table has the standard alphabet: windows with a
    code above 27 miss), equals the oracle on the keys' text."""
    torch = pytest.importorskip("torch")
    keys, fids, want = ac.dump_keys(k)
    S = kma.bucket_slots(k)
    nb = kma.buckets_for(len(want), 0.9, k)
    m = kma.layout_for(k, nb) & 0xFF
    code = {"two-choice": 6 | kma.LAYOUT_TWO_CHOICE,
            "two-choice-mod": 6 | kma.LAYOUT_MOD_SAMPLING | kma.LAYOUT_TWO_CHOICE,
            "chained": m, "flat": 0}[layout_name]
    assert m != 0
    if k == 8:
        assert m == 6 | kma.LAYOUT_MOD_SAMPLING  # the size rule's order at K = 8
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    words = 2 if k > 8 else 1  # u64 per slot
    slots = torch.empty(nb * S * words, dtype=torch.int64, device=dev)
    winner = torch.empty(nb * S, dtype=torch.int32, device=dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    d_keys = torch.from_numpy(keys.view(np.int64)).to(dev)
    d_fids = torch.from_numpy(fids.view(np.int32)).to(dev)
    kma.build_device(slots.data_ptr(), nb, winner.data_ptr(), d_keys.data_ptr(),
                     d_fids.data_ptr(), len(keys), status.data_ptr(), stream, k=k, layout=code)
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    assert st[0] == 0 and st[1] == len(want), st.tolist()
    got_keys, got_fids = decode_slots(slots.cpu().numpy().view(np.uint64), k)
    assert len(got_keys) == len(want)
    got = dict(zip(got_keys.tolist(), got_fids.tolist()))
    assert len(got) == len(want) and got == want
    assert got[(1 << (5 * k)) - 1] == len(keys)  # the all-ones key: the last row's fid
    if k != 8:
        return
    wkeys = np.fromiter(want, np.uint64, len(want))
    wfids = np.fromiter(want.values(), np.int32, len(want))
    prots = _dump_proteins(wkeys, k)
    res, off = oracle_c.pack_strings(prots)
    n, n_res = len(prots), int(off[-1])
    rows = ac.codes_text(ac.key_codes(wkeys, k))
    table_of = lambda keep: oracle_c.Table.from_buffer(  # noqa: E731
        rows[keep].tobytes(), np.arange(int(keep.sum()) + 1, dtype=np.uint64) * k, wfids[keep])
    standard = (ac.key_codes(wkeys, k) <= 27).all(axis=1)
    assert 1000 < standard.sum() < len(wkeys) - 1000
    d_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
    with kma.SignatureTable.wrap_device(slots.data_ptr(), nb, k, 0, code) as t:
        ws = kma.Workspace(0, n_res, n)
        for entry in ("stream", "ascii"):
            outs = [torch.full((n,), 9, dtype=d, device=dev)
                    for d in (torch.int32, torch.int32, torch.uint8)]
            if entry == "stream":
                host = stream_bytes(ac.code_of(True)[res[:n_res]], kma.packed_bytes(n_res))
                d_in = torch.from_numpy(host).to(dev)
                keep = np.ones(len(wkeys), bool)
                call = kma.annotate_packed_device
            else:
                kma.set_option(kma.OPT_PACKED_INPUT, 0)
                d_in = torch.from_numpy(res.copy()).to(dev)
                keep = standard
                call = kma.annotate_proteins_device
            call(t, ws, d_in.data_ptr(), d_off.data_ptr(), n, n_res, 1, 0,
                 *[o.data_ptr() for o in outs], 0, 0, stream)
            torch.cuda.synchronize()
            efid, ecnt, est = oracle_c.apply(table_of(keep), res, off, k, 1, 0)
            fid, cnt, stt = (o.cpu().numpy() for o in outs)
            assert (stt == est).all() and (fid == efid).all() and (cnt == ecnt).all(), entry
            single = np.flatnonzero(keep)
            assert (est[single] == 1).all() and (efid[single] == wfids[keep]).all()
        ws.close()


# ---- d. peg tables ---------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [4, 8, 12])
def test_peg_table_all_symbols(kma, oracle_c, k):
    """kma_peg_table_create on pegs over 'A'..'Z' and '*' with 'X' runs, lower case, EXTRA bytes,
    repeated kmers and pegs of length 0, K and K + 1: the counted windows, the entries (the
    oracle's peg kmers that hold standard symbols only and occur once: a numpy count), and, for
    K <= 8, the pegs annotated against their own table (every window counted, one hit enough)
    equal to the oracle on the table of those singletons with the peg index as fid. That probe
    reads the 'Z' and '*' kmers that no translated contig can reach."""
    pegs = ac.peg_case(k)
    res, off = oracle_c.pack_strings(pegs)
    kmers, owner = ac.peg_singletons(oracle_c, k, pegs)
    t, n_win = kma.SignatureTable.from_pegs(res, off, k)
    with t:
        assert n_win == sum(max(len(p) - k, 0) for p in pegs)
        info = t.info
        assert info.k == k and info.n_entries == len(kmers) and info.n_extra_syms == 0
        if k > 8:
            return
        want = oracle_c.apply(oracle_c.Table(kmers, owner.astype(np.int32)), res, off, k, 1,
                              F_MULTISET)
        assert (want[2] == 1).sum() > 100 and (want[2] == 2).sum() > 10
        for mode in (0, 2):
            kma.set_option(kma.OPT_PACKED_INPUT, mode)
            fid, cnt, st, _ = kma.annotate_proteins(t, res, off, 1, F_MULTISET)
            assert (st == want[2]).all() and (fid == want[0]).all() and (cnt == want[1]).all()


# ---- e. set operators ------------------------------------------------------------------------------

_set_case = []


def set_case(oracle_c):
    if not _set_case:
        prots = ac.set_op_proteins()
        res, off = oracle_c.pack_strings(prots)
        for a in (res, off):
            a.flags.writeable = False
        _set_case.append((prots, res, off))
    return _set_case[0]


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("k", [1, 8, 12])
def test_build_signatures_all_symbols(kma, oracle_c, k, flags):
    """kma_build_signatures on 200 proteins over the 27 standard symbols, half of the residues
    from BJOUXZ* (seven roles, buffered and skipped proteins): the (kmer, role) rows equal the
    oracle's, '*' * K among the kmers seen."""
    prots, res, off = set_case(oracle_c)
    roles = (np.arange(len(prots)) % 9 - 2).astype(np.int32)  # -2 skipped, -1 buffered, 0..6
    km, rl = oracle_c.build_signatures(res, off, roles, k, flags)
    keys, groles = kma.build_signatures(res, off, roles, k, flags)
    got = dict(zip((bytes(r) for r in unpack_keys(np.asarray(keys, np.uint64), k)),
                   groles.tolist()))
    exp = {bytes(r): int(v) for r, v in zip(km, rl)}
    assert got == exp and len(keys) == len(exp)
    if k > 1:  # (every 1-mer occurs under several roles: no row survives at K = 1)
        assert len(exp) > 1000 and sum(b"Z" in r or b"*" in r for r in exp) > 300


@pytest.mark.parametrize("k", [2, 8, 12])
def test_distances_and_best_match_all_symbols(kma, oracle_c, k):
    """kma_protein_distances (both window conventions) and kma_protein_best_match on the same
    proteins: similarity, set sizes and distances equal the oracle's, and the closest-source
    choice equals the rule of GeneCopyProcessor applied to the oracle's distances."""
    prots, res, off = set_case(oracle_c)
    n = len(prots)
    rng = np.random.default_rng(k)
    pa = np.concatenate([rng.integers(0, n, 3000), np.arange(n)]).astype(np.uint32)
    pb = np.concatenate([rng.integers(0, n, 3000), np.arange(n)]).astype(np.uint32)
    for flags in (0, 1):
        sim, size, dist = kma.protein_distances(res, off, pa, pb, k, flags)
        esim, esa, esb, edist = oracle_c.protein_distances(res, off, pa, pb, k, flags)
        assert (sim == esim).all() and (size[pa] == esa).all() and (size[pb] == esb).all()
        assert (dist == edist).all()
    assert (esim > 0).sum() > 150
    query = np.arange(n, dtype=np.uint32)
    cand = rng.integers(0, n, 12 * n).astype(np.uint32)
    cand[12 * query[::2] + query[::2] % 12] = query[::2]  # the query itself: distance 0
    cand[12 * np.arange(0, 36, 3) + 5] = 150 + np.arange(0, 36, 3)  # its mutated copy
    cand_off = np.arange(n + 1, dtype=np.uint64) * 12
    best, bd = kma.protein_best_match(res, off, query, cand_off, cand, 0.9, k)
    edist = oracle_c.protein_distances(res, off, np.repeat(query, 12), cand, k, 0)[3]
    for q in range(n):
        fdist, found = 0.9, -1
        for c, x in zip(cand[12 * q:12 * q + 12], edist[12 * q:12 * q + 12]):
            if x <= fdist:
                fdist, found = x, int(c)
        assert best[q] == found and bd[q] == fdist, q
    assert (best >= 0).sum() > 80 and (best != query)[best >= 0].sum() > 5


@pytest.mark.parametrize("k", [2, 8, 12])
def test_hash_annotate_all_symbols(kma, oracle_c, k):
    """kma_hash_annotate with the first 130 of those proteins as the genome and the proteins from
    the 70th on as prototypes: best prototype, similarity and match counts equal the oracle's."""
    prots, _, _ = set_case(oracle_c)
    g, go = oracle_c.pack_strings(prots[:130])
    p, po = oracle_c.pack_strings(prots[70:])
    got = kma.hash_annotate(g, go, p, po, k, 0.0125)
    exp = oracle_c.hash_annotate(g, go, p, po, k, 0.0125)
    for a, b in zip(got, exp):
        assert (a == b).all()
    assert (exp[0] >= 0).sum() > 60
