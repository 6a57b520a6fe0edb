"""The staged ASCII probe (annotate_kernel<K, M, P, false>): a block packs its span's residues
into an LDS stage of C + 7 residues at a time (C = kStageRes, kma_internal.h) and reads its
window keys from there. Device calls run it under KMA_OPT_PACKED_INPUT 0 and 1 (the default)
at every batch size; 2 keeps the pack kernel and the stream probe.

Every case compares fid, count, status and the tally of kma_annotate_proteins_device with the
oracle (oracle.c_oracle.apply_mt) and checks that options 0, 1 and 2 agree bit for bit. The
library exports no C, so the chunk-edge lengths are derived for all three stage sizes the
design considers (1,024, 2,048 and 4,096 residues): the cases hold whichever one is built.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
K = 8
MIN_HITS = 5
N_FID = 300
STAGES = (1024, 2048, 4096)
PAD = 32  # bytes the ABI header promises readable past offsets[n_seq]


@pytest.fixture(scope="module")
def kma(native_lib):
    import kmeranno
    assert kmeranno.device_count() >= 1
    return kmeranno


class _Case:
    """A ~20k-row table (device + oracle) and the residues of its synthetic queries, used as
    the source text of every protein here (copies of table functions: their windows hit)."""

    def __init__(self, kma, oracle_c, k=K, seed=41, one_fid=False):
        from kmeranno import synth
        wl = synth.make_workload(400, 20_000, N_FID, seed=seed, k=k)
        self.k = k
        # one_fid: every row carries function 7, so a protein cut across many source proteins is
        # CALLED (not AMBIGUOUS, count 0) and its count, the size of its set, is compared
        self.keys, self.fids = wl.keys, np.full_like(wl.fids, 7) if one_fid else wl.fids
        self.text = wl.residues[:int(wl.offsets[-1])].copy()
        kmers = [synth.unpack_key(x, k) for x in wl.keys]
        self.oracle = oracle_c.Table(kmers, self.fids.astype(np.int32))

    def take(self, lengths, at=0):
        """Proteins of these lengths cut consecutively from the source text (cyclically)."""
        total = int(sum(lengths))
        res = np.resize(np.roll(self.text, -at), total) if total else np.zeros(0, np.uint8)
        off = np.zeros(len(lengths) + 1, np.uint64)
        off[1:] = np.cumsum(np.asarray(lengths, np.uint64))
        return res, off


@pytest.fixture(scope="module")
def case(kma, oracle_c):
    return _Case(kma, oracle_c)


@pytest.fixture(scope="module")
def case1(kma, oracle_c):
    return _Case(kma, oracle_c, one_fid=True)


def _expected(oracle_c, case, res, off, flags, min_hits=MIN_HITS):
    efid, ecnt, est = oracle_c.apply_mt(case.oracle, res, off, case.k, min_hits, flags, 4)
    tally = np.bincount(efid[est == 1], minlength=N_FID).astype(np.uint32)
    return efid, ecnt, est, tally


def _device_call(kma, t, res, off, flags=0, mis=0, lead=8, pad=None, min_hits=MIN_HITS):
    """kma_annotate_proteins_device on a device buffer whose first residue sits at byte
    lead + mis (offsets[0] = lead + mis != 0; the buffer is 8-byte aligned) and that ends PAD
    bytes after the last residue; `pad` fills those bytes (default: zeros)."""
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    n, n_res, first = len(off) - 1, len(res), lead + mis
    buf = np.zeros(first + n_res + PAD, np.uint8)
    buf[:first] = ord("A")
    buf[first:first + n_res] = res
    if pad is not None:
        buf[first + n_res:] = np.resize(pad, PAD)
    d_res = torch.from_numpy(buf).to(dev)
    assert d_res.data_ptr() % 8 == 0
    d_off = torch.from_numpy((off + np.uint64(first)).view(np.int64).copy()).to(dev)
    fid = torch.full((n,), -7, dtype=torch.int32, device=dev)
    cnt = torch.full((n,), -7, dtype=torch.int32, device=dev)
    st = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    tally = torch.zeros(N_FID, dtype=torch.int32, device=dev)
    ws = kma.Workspace(0, max(n_res, 1), n)
    try:
        kma.annotate_proteins_device(t, ws, d_res.data_ptr(), d_off.data_ptr(), n, n_res, min_hits,
                                     flags, fid.data_ptr(), cnt.data_ptr(), st.data_ptr(),
                                     tally.data_ptr(), N_FID, stream)
        torch.cuda.synchronize()
    finally:
        ws.close()
    return (fid.cpu().numpy(), cnt.cpu().numpy(), st.cpu().numpy(),
            tally.cpu().numpy().astype(np.uint32))


def _check(kma, oracle_c, case, t, res, off, flags=0, **kw):
    """Options 0, 1 and 2 agree bit for bit, and equal the oracle."""
    want = _expected(oracle_c, case, res, off, flags)
    got = {}
    for mode in (1, 0, 2):
        with kma.options(packed_input=mode):
            got[mode] = _device_call(kma, t, res, off, flags, **kw)
    for mode in (0, 2):
        for a, b, name in zip(got[mode], got[1], ("fid", "count", "status", "tally")):
            assert (a == b).all(), (mode, name)
    for a, b, name in zip(got[1], want, ("fid", "count", "status", "tally")):
        assert (a == b).all(), name
    return got[1]


def _edge_spans():
    spans = []
    for c in STAGES:
        spans += [c - 1, c, c + 1, c + 7, c + 8, 2 * c + 3]
    return spans


@pytest.mark.parametrize("block_proteins", [1, 6])
def test_chunk_edges(kma, oracle_c, case, case1, block_proteins):
    """Group spans of C - 1, C, C + 1, C + 7, C + 8 and 2C + 3 residues and one protein of
    3C + 5 (for C = 1,024, 2,048 and 4,096): the stage reload, its 7-residue overlap and windows
    that straddle two stages. One protein per block, and groups of 6 (five short proteins, one
    of them empty, then the one that fills the span)."""
    lengths = []
    for s in _edge_spans():
        lengths += [s] if block_proteins == 1 else [20, 9, 0, 31, 40, s - 100]
    for c in STAGES:
        lengths += [3 * c + 5] + ([] if block_proteins == 1 else [11, 0, 8, 7, 300])
    res, off = case.take(lengths)
    for c in (case, case1):
        with kma.SignatureTable.from_packed(c.keys, c.fids, K) as t, \
                kma.options(block_proteins=block_proteins):
            fid, cnt, st, _ = _check(kma, oracle_c, c, t, res, off)
    # (one function: long proteins cut from copies are called, with counts; the source text also
    # holds random proteins, which hit nothing)
    called = (np.asarray(lengths) > 900) & (st == kma.STATUS_CALLED)
    assert called.sum() >= 12 and cnt[called].max() > 100


@pytest.mark.parametrize("mis", range(8))
def test_alignment(kma, oracle_c, case, mis):
    """The call's first residue at every byte offset 0..7 of the 8-byte aligned device buffer,
    offsets[0] != 0; spans on both sides of the stage size."""
    res, off = case.take([300, 1500, 7, 1030, 0, 2060, 4100, 64, 8, 9], at=mis * 101)
    with kma.SignatureTable.from_packed(case.keys, case.fids, K) as t:
        _check(kma, oracle_c, case, t, res, off, mis=mis)
        with kma.options(block_proteins=1):
            _check(kma, oracle_c, case, t, res, off, mis=mis)


def test_degenerate_proteins(kma, oracle_c, case):
    """Proteins shorter than K, empty proteins, n_seq not a multiple of the block's protein
    count (4 by default here, 6 forced), and a batch of 7 empty proteins."""
    lengths = [0, 3, 7, 8, 0, 0, 9, 120, 1, 0, 640, 5, 0]  # 13 proteins
    res, off = case.take(lengths)
    with kma.SignatureTable.from_packed(case.keys, case.fids, K) as t:
        for bp in (0, 6, 1):
            with kma.options(block_proteins=bp):
                _, cnt, st, _ = _check(kma, oracle_c, case, t, res, off)
                assert (st[np.asarray(lengths) < K] == kma.STATUS_NONE).all()
        res0, off0 = case.take([0] * 7)
        _, cnt, st, tally = _check(kma, oracle_c, case, t, res0, off0)
        assert (st == kma.STATUS_NONE).all() and not cnt.any() and not tally.any()


def test_bytes_without_a_code(kma, oracle_c, case, case1):
    """'*' (a code, but in no table row here), a digit, a lower-case letter, 0x00 and 0xFF inside
    windows and at their edges, a window whose eight bytes all lack codes (key 0: not probed) and
    longer runs of them, also across the first stage's end."""
    lengths = [400, 1100, 2100, 4200, 100]
    res, off = case.take(lengths)
    res = res.copy()
    bad = np.frombuffer(b"*7q\x00\xff", np.uint8)
    for p in range(len(lengths)):
        lo, hi = int(off[p]), int(off[p + 1])
        res[lo] = bad[p % 5]               # a protein's first byte
        res[hi - 1] = bad[(p + 1) % 5]     # and its last
        res[lo + 40:lo + 48] = np.resize(bad[1:], 8)   # a whole window without codes
        res[lo + 70:lo + 70 + 23] = np.resize(bad, 23)  # a run: every window inside is key 0
        res[lo + 20] = bad[p % 5]          # one byte inside otherwise good windows
    for c in STAGES:  # around the stage ends of the long proteins
        for p in range(len(lengths)):
            if lengths[p] > c + 16:
                res[int(off[p]) + c - 3:int(off[p]) + c + 6] = np.resize(bad, 9)
    for c in (case, case1):
        with kma.SignatureTable.from_packed(c.keys, c.fids, K) as t:
            for bp in (0, 1):
                with kma.options(block_proteins=bp):
                    _check(kma, oracle_c, c, t, res, off)


@pytest.mark.parametrize("flags", [1, 2, 3], ids=["end-exclusive", "multiset", "both"])
def test_flags(kma, oracle_c, case1, flags):
    case = case1  # one function: counts (distinct keys, or every hit) are reported
    """KMA_F_END_EXCLUSIVE and KMA_F_MULTISET on spans below and above the stage size."""
    res, off = case.take([8, 9, 500, 1024, 1031, 2050, 4099, 0, 77], at=5000)
    with kma.SignatureTable.from_packed(case.keys, case.fids, K) as t:
        _check(kma, oracle_c, case, t, res, off, flags=flags)


@pytest.mark.parametrize("layout", ["auto", "6", "7", "0", "chained"],
                         ids=["m6-mod-two-choice", "m6-two-choice", "m7", "flat", "chained"])
def test_layouts(kma, oracle_c, case, layout):
    """Every table layout the library builds at K = 8: m = 6 in the mod-sampling order (the
    size rule's choice), m = 6 in the smallest-hash order, m = 7 and flat, each with two-choice
    placement, and the size rule's layout with overflow chains."""
    kma.set_option(kma.OPT_LAYOUT, -1 if layout in ("auto", "chained") else int(layout))
    kma.set_option(kma.OPT_PLACEMENT, 0 if layout == "chained" else -1)
    res, off = case.take([300, 1023, 1025, 2049, 4097, 5, 0, 3100], at=777)
    with kma.SignatureTable.from_packed(case.keys, case.fids, K) as t:
        info = t.info
        assert info.two_choice == (0 if layout == "chained" else 1)
        assert info.minimizer_len == {"auto": 6, "chained": 6, "6": 6, "7": 7, "0": 0}[layout]
        _check(kma, oracle_c, case, t, res, off)
        with kma.options(block_proteins=1):
            _check(kma, oracle_c, case, t, res, off)


def test_narrow_k(kma, oracle_c):
    """K = 5: windows of 25 stream bits from the same stage."""
    c5 = _Case(kma, oracle_c, k=5, seed=43)
    res, off = c5.take([4, 5, 6, 300, 1020, 1028, 2047, 2052, 4100, 0, 12300], at=99)
    with kma.SignatureTable.from_packed(c5.keys, c5.fids, 5) as t:
        for flags in (0, 1):
            _check(kma, oracle_c, c5, t, res, off, flags=flags)


def test_lds_pool_pressure(kma, oracle_c, case1):
    case = case1  # one function: the counts are reported and compared
    """A group whose sets no longer fit beside the stage: one protein of 2,800 windows
    (a set of 4,200 entries; the pool has 4,096, less the stage) beside five short ones keeps
    its hits in its workspace list, and the counts still equal the oracle's. Then two proteins
    whose sets would fit the whole pool together (2 x 1,340 windows -> 4,024 entries) but not
    what the stage leaves of it."""
    with kma.SignatureTable.from_packed(case.keys, case.fids, K) as t, kma.options(block_proteins=6):
        for lengths in ([50, 2807, 60, 70, 80, 90], [1347, 1347, 0, 0, 0, 0]):
            res, off = case.take(lengths, at=1234)
            _, cnt, st, _ = _check(kma, oracle_c, case, t, res, off)
            assert cnt.max() > 50  # the long protein is called with many distinct keys


def test_buffer_end(kma, oracle_c, case1):
    case = case1  # one function: a leaked window changes a reported count
    """The batch's last residue is the last byte of a device buffer that carries only the
    padding the ABI header promises (kmeranno.h: d_residues is "readable for 32 bytes past
    offsets[n_seq]"). The staged loads stay inside it: a block reads the aligned 8-byte words
    around whole 8-residue groups that start below its span's end, so the last word read is the
    one after the word holding the last residue, at most 15 bytes past it, which is also the
    last word the per-window ASCII loads of earlier releases read. The padding holds table
    kmers: a window that took residues from it would change a count. Every length modulo 8 of
    the tail protein, at every misalignment that moves the end across a word."""
    with kma.SignatureTable.from_packed(case.keys, case.fids, K) as t:
        for tail in (1017, 1024, 1025, 2055, 61):
            for mis in (0, 3, 7):
                res, off = case.take([40, 0, tail], at=PAD)
                pad = np.resize(np.roll(case.text, -(PAD + len(res))), PAD)  # the text goes on
                with kma.options(block_proteins=1):
                    _check(kma, oracle_c, case, t, res, off, mis=mis, pad=pad)
                _check(kma, oracle_c, case, t, res, off, mis=mis, pad=pad)
