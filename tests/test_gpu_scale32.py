"""Protein device calls of 2^31 to 2^32 - 128 residues against the oracle, bit-exact.

kma_annotate_proteins_device, kma_annotate_packed_device and kma_workspace_reserve_batch accept
up to 2^32 - 128 residues in one call; the kernels hold positions inside a call in 32 bits and
form addresses (residue bytes, the packed stream's bit offsets, a long protein's workspace list at
2 u32 per residue) in 64. The batches are tests/scale_cases.py's: one base tile of 105 proteins
repeated on the device, so the expected outputs are the oracle's on one tile, tiled
(tests/test_scale_workload.py shows that on the CPU). Every comparison is `==` over all proteins
of the call, tally included.

One module-scoped fixture holds the table(s), the 2^32 - 128-residue device buffer, its offsets
and one workspace reserved for the limit: about 42 GB of device memory, computed from the
library's own formulas before anything is allocated (the module skips, with both numbers, if less
than that plus 2 GiB is free). The protein path takes tables of K <= 8 only (a K = 10 table is
refused with KMA_E_INVALID, tests/test_gpu_wide.py), so the second table here is K = 7.

The batch sits LEAD bytes (16 MiB) into its allocation. Calls pass the batch's own first byte
as d_residues, except test_c_buffer_positions_past_2_32, which passes the allocation's and
offsets larger by LEAD: a buffer of 2^32 - 128 bytes addressed from its first byte never forms
offsets[0] + position >= 2^32, and a residue address truncated to 32 bits went unnoticed
without that case.
"""
import time

import numpy as np
import pytest

import scale_cases as sc

pytestmark = pytest.mark.gpu
K = 8
MIN_HITS = sc.MIN_HITS
PAD = 64           # bytes after the last residue (the header asks for 32 readable ones)
LEAD = (1 << 24) + 40   # bytes before the batch in its device buffer (a multiple of 8): with
                        # them as offsets[0] the batch's last 16 MiB lie past byte 2^32
RES_PAD = 64       # the workspace's positions past the last residue (kma_abi_proteins.cpp)
GIB = 1 << 30
TWO31 = 1 << 31
SUB = 3000         # proteins of a high sub-batch: 28 tiles, 4.6M residues
N_HOST = TWO31 + (8 << 20)   # the host call: one default slice of 2^31 residues and a rest


@pytest.fixture(scope="module")
def kma(native_lib):
    import kmeranno
    assert kmeranno.device_count() >= 1
    return kmeranno


def _device_need(kma, lay, lay_d):
    """Bytes of device memory the module's fixtures hold at once (the library's formulas)."""
    n = sc.N_MAX
    n_seq = max(lay.n_seq, lay_d.n_seq)
    return {
        "residues": LEAD + n + PAD,
        "workspace lists (8 B per residue)": 8 * (n + RES_PAD),
        "workspace packed stream": kma.packed_bytes(n + RES_PAD),
        "pre-packed stream": kma.packed_bytes(n),
        "offsets": 16 * (lay.n_seq + 1) + 8 * (lay_d.n_seq + 1),
        "outputs": 9 * n_seq + 4 * sc.N_FID,
    }


def _host_call_need(kma):
    """Device bytes of the host call's pooled context(s): the lists and the staged stream of one
    2^31-residue slice (two replicas hold half of it each)."""
    return 8 * (TWO31 + RES_PAD) + kma.packed_bytes(TWO31) + 16 * (N_HOST // 1000)


def _require_free(need, what):
    import torch
    free, total = torch.cuda.mem_get_info(0)
    print(f"\n{what}: needs {need / GIB:.2f} GiB of device memory, {free / GIB:.2f} GiB free of "
          f"{total / GIB:.2f}")
    if free < need + 2 * GIB:
        pytest.skip(f"{what} needs {need} bytes of device memory and 2 GiB of margin; "
                    f"{free} bytes are free")


def _tiled_on_device(torch, dev, tile, reps, tail, n_bytes, lead=0):
    """tile x reps, then tail, in one device buffer of n_bytes (zero after the tail) that follows
    `lead` bytes of 'A'; returns the whole allocation and the buffer."""
    whole = torch.empty(lead + n_bytes, dtype=torch.uint8, device=dev)
    whole[:lead].fill_(ord("A"))
    buf = whole[lead:]
    assert whole.data_ptr() % 8 == 0 and buf.data_ptr() % 8 == 0
    t = torch.from_numpy(np.array(tile)).to(dev)
    body = reps * len(tile)
    buf[:body].view(reps, len(tile)).copy_(t.expand(reps, len(tile)))  # (Tensor.repeat in place)
    buf[body:body + len(tail)].copy_(torch.from_numpy(np.array(tail)).to(dev))
    buf[body + len(tail):].zero_()
    return whole, buf


class _Big:
    """The tables, the N_MAX-residue device batch, its offsets, the outputs and one workspace."""

    def __init__(self, kma, oracle_c):
        import torch
        self.kma, self.oracle_c, self.torch = kma, oracle_c, torch
        self.dev = torch.device("cuda", 0)
        self.lay = sc.layout(sc.N_MAX)
        self.lay_d = sc.layout(sc.N_MAX, aligned=True)
        need = _device_need(kma, self.lay, self.lay_d)
        self.need = sum(need.values())
        for name, v in need.items():
            print(f"\n  {name}: {v / GIB:.3f} GiB", end="")
        _require_free(self.need, "the 2^32 - 128-residue fixtures")
        self.free_before = torch.cuda.mem_get_info(0)[0]
        self.tables = {}
        lay, b = self.lay, self.lay.base
        t0 = time.perf_counter()
        self.whole, self.buf = _tiled_on_device(torch, self.dev, b.res, lay.reps,
                                                sc.tail_residues(lay), sc.N_MAX + PAD, LEAD)
        self.d_off = torch.from_numpy(lay.offsets.view(np.int64)).to(self.dev)
        self.d_off_lead = self.d_off + LEAD  # the same batch seen from the allocation's start
        n_seq = max(self.lay.n_seq, self.lay_d.n_seq)
        self.fid = torch.empty(n_seq, dtype=torch.int32, device=self.dev)
        self.cnt = torch.empty(n_seq, dtype=torch.int32, device=self.dev)
        self.st = torch.empty(n_seq, dtype=torch.uint8, device=self.dev)
        self.tally = torch.zeros(sc.N_FID, dtype=torch.int32, device=self.dev)
        self.ws = kma.Workspace(0)
        self.ws.reserve(sc.N_MAX, n_seq)
        torch.cuda.synchronize()
        print(f"fixture built in {time.perf_counter() - t0:.2f} s: {lay.n_seq} proteins, "
              f"{lay.reps} tiles of {b.T} residues, partial tile of {lay.m}, filler {lay.filler}")
        self._stream_d = None

    def table(self, placement="two-choice", k=K):
        """The table of scale_cases.table_rows(k), two-choice placement or overflow chains."""
        kma = self.kma
        if (placement, k) not in self.tables:
            kmers, fids = sc.table_rows(k)
            with kma.options(placement=0 if placement == "chained" else -1):
                t = kma.SignatureTable.from_rows(kmers, fids, k)
            assert t.info.two_choice == (0 if placement == "chained" else 1)
            assert t.info.n_extra_syms == 4 and t.info.k == k
            self.tables[(placement, k)] = t
        return self.tables[(placement, k)]

    def stream_d(self):
        """The pre-packed stream of the batch of tiles of whole 64-residue groups, and its
        offsets: the host-packed base tile's 40-byte groups tiled on the device, then the
        host-packed tail (which starts at a multiple of 64 residues)."""
        if self._stream_d is None:
            kma, torch, lay, t = self.kma, self.torch, self.lay_d, self.table()
            b = lay.base
            assert b.T % 64 == 0 and lay.tail0 % 64 == 0
            g = 40 * (b.T // 64)
            tile = kma.pack_residues(t, b.res)[:g]
            tail = kma.pack_residues(t, sc.tail_residues(lay))
            total = kma.packed_bytes(sc.N_MAX)
            assert lay.reps * g + len(tail) == total
            stream = _tiled_on_device(torch, self.dev, tile, lay.reps, tail, total)[1]
            d_off = torch.from_numpy(lay.offsets.view(np.int64)).to(self.dev)
            self._stream_d = (stream, d_off)
        return self._stream_d

    def call(self, t, lo, hi, flags=0, entry="ascii", k=K):
        """One device call on proteins [lo, hi) (the offsets pointer advanced by lo entries, the
        residue pointer the buffer's base; entry "lead": the allocation's base, LEAD bytes before
        it, and offsets larger by LEAD); returns what the call wrote and what it should."""
        kma, torch = self.kma, self.torch
        lay = self.lay_d if entry == "stream" else self.lay
        n, n_res = hi - lo, int(lay.offsets[hi] - lay.offsets[lo])
        self.fid[:n].fill_(-7)
        self.cnt[:n].fill_(-7)
        self.st[:n].fill_(9)
        self.tally.zero_()
        out = (self.fid.data_ptr(), self.cnt.data_ptr(), self.st.data_ptr(),
               self.tally.data_ptr(), sc.N_FID, torch.cuda.current_stream().cuda_stream)
        if entry == "stream":
            stream, d_off = self.stream_d()
            first = int(lay.offsets[lo])
            assert first % 64 == 0  # stream residue 0 is residue offsets[lo]: a whole group
            kma.annotate_packed_device(t, self.ws, stream.data_ptr() + 40 * (first // 64),
                                       d_off.data_ptr() + 8 * lo, n, n_res, MIN_HITS, flags, *out)
        else:
            base, d_off = (self.whole, self.d_off_lead) if entry == "lead" else \
                (self.buf, self.d_off)
            kma.annotate_proteins_device(t, self.ws, base.data_ptr(), d_off.data_ptr() + 8 * lo,
                                         n, n_res, MIN_HITS, flags, *out)
        torch.cuda.synchronize()
        got = (self.fid[:n].cpu().numpy(), self.cnt[:n].cpu().numpy(), self.st[:n].cpu().numpy(),
               self.tally.cpu().numpy().astype(np.uint32))
        return got, sc.expected(self.oracle_c, lay, k, flags, lo, hi), lay

    def check(self, t, lo, hi, flags=0, entry="ascii", k=K, what=""):
        t0 = time.perf_counter()
        got, want, lay = self.call(t, lo, hi, flags, entry, k)
        dt = time.perf_counter() - t0
        for name, a, b in zip(("status", "fid", "count"), (got[2], got[0], got[1]),
                              (want[2], want[0], want[1])):
            bad = np.flatnonzero(a != b)
            if bad.size:
                i = lo + int(bad[0])
                raise AssertionError(
                    f"{what}: {name} differs for {bad.size} of {hi - lo} proteins, first protein "
                    f"{i} (tile protein {i % lay.base.n}, residues [{int(lay.offsets[i])}, "
                    f"{int(lay.offsets[i + 1])}) of the buffer, {int(lay.offsets[i] - lay.offsets[lo])} "
                    f"into the call): got {a[bad[0]]}, expected {b[bad[0]]}")
        assert (got[3] == want[3]).all(), f"{what}: tally"
        assert want[3].sum() > 0 or hi - lo < lay.base.n
        return dt

    def close(self):
        for t in self.tables.values():
            t.close()
        self.ws.close()


@pytest.fixture(scope="module")
def big(kma, oracle_c):
    b = _Big(kma, oracle_c)
    yield b
    b.close()


def _first_at_or_past(lay, x):
    return int(np.searchsorted(lay.offsets, np.uint64(x), side="left"))


def test_buffer_is_the_tiled_batch(big):
    """The device buffer holds the batch residues_at describes: its first bytes, 1 MiB on either
    side of 2^31 and its last MiB with the padding."""
    lay = big.lay
    for lo, hi in ((0, 1 << 20), (TWO31 - (1 << 20), TWO31 + (1 << 20)),
                   (sc.N_MAX - (1 << 20), sc.N_MAX)):
        assert (big.buf[lo:hi].cpu().numpy() == sc.residues_at(lay, lo, hi)).all()
    assert not big.buf[sc.N_MAX:].cpu().numpy().any()
    assert big.buf.data_ptr() == big.whole.data_ptr() + LEAD
    assert (big.whole[:LEAD].cpu().numpy() == ord("A")).all()
    assert (big.d_off_lead.cpu().numpy().view(np.uint64) == lay.offsets + np.uint64(LEAD)).all()
    assert int(big.d_off[-1].item()) == sc.N_MAX and big.d_off.numel() == lay.n_seq + 1


@pytest.mark.parametrize("flags", [0, 3])
@pytest.mark.parametrize("packed_input", [0, 2], ids=["ascii-staged", "pack-kernel"])
def test_a_whole_batch_at_the_limit(kma, big, packed_input, flags):
    """A. One call of 2^32 - 128 residues, n_fid tally on: the ASCII probe staged in LDS and the
    device pack kernel with the stream probe, flags 0 and END_EXCLUSIVE | MULTISET."""
    with kma.options(packed_input=packed_input):
        dt = big.check(big.table(), 0, big.lay.n_seq, flags, what="whole batch")
    print(f"\nwhole batch, packed_input {packed_input}, flags {flags}: {dt:.3f} s")


@pytest.mark.parametrize("side", ["below", "above"])
@pytest.mark.parametrize("packed_input", [0, 2], ids=["ascii-staged", "pack-kernel"])
def test_b_prefixes_on_either_side_of_2_31(kma, big, packed_input, side):
    """B. Proteins [0, n) for the largest n with offsets[n] < 2^31 and the smallest with
    offsets[n] > 2^31."""
    off = big.lay.offsets
    n = _first_at_or_past(big.lay, TWO31) - 1 if side == "below" else \
        int(np.searchsorted(off, np.uint64(TWO31), side="right"))
    assert int(off[n]) < TWO31 <= int(off[n + 1]) if side == "below" else \
        int(off[n - 1]) <= TWO31 < int(off[n])
    with kma.options(packed_input=packed_input):
        dt = big.check(big.table(), 0, n, 0, what=f"prefix {side} 2^31")
    print(f"\nprefix of {int(off[n])} residues, packed_input {packed_input}: {dt:.3f} s")


def _sub_range(lay, name):
    i0 = _first_at_or_past(lay, TWO31)
    if name == "from-2^31":
        lo = i0
    elif name == "last":
        lo = lay.n_seq - SUB
    else:  # straddling 2^31
        lo = i0 - SUB // 2
    hi = lo + SUB
    off = lay.offsets
    if name == "from-2^31":
        assert int(off[lo]) >= TWO31 > int(off[lo - 1])
    elif name == "last":
        assert hi == lay.n_seq and int(off[lo]) > (1 << 32) - (1 << 24)
    else:
        assert int(off[lo]) < TWO31 < int(off[hi])
    for long_one in ("g30", "l60", "a30"):
        assert sc.proteins_holding(lay, long_one, lo, hi) >= 1
    return lo, hi


@pytest.mark.parametrize("placement", ["two-choice", "chained"])
@pytest.mark.parametrize("name", ["from-2^31", "last", "straddle"])
def test_c_high_sub_batches(kma, big, name, placement):
    """C. Small calls whose offsets[0] is large: 3,000 proteins from the first one at or past
    2^31, the buffer's last 3,000 (offsets[0] > 2^32 - 2^24) and 3,000 around 2^31, each with
    30,000- and 60,000-residue proteins, under both inputs, flags 0..3, 1 and 8 proteins per
    block, the one-pass and the two-pass grid, on a two-choice and a chained table."""
    lo, hi = _sub_range(big.lay, name)
    t = big.table(placement)
    for packed_input in (0, 2):
        for flags in (0, 1, 2, 3):
            for bp in (1, 8):
                for defer in (0, 2):
                    with kma.options(packed_input=packed_input, block_proteins=bp, defer=defer):
                        big.check(t, lo, hi, flags, what=f"{name} packed_input {packed_input} "
                                  f"flags {flags} block_proteins {bp} defer {defer}")


def test_c_high_sub_batch_k7(kma, big):
    """C, another key width: the buffer's last 3,000 proteins against the K = 7 table (the
    protein path refuses wide tables, K > 8)."""
    lo, hi = _sub_range(big.lay, "last")
    t = big.table("two-choice", 7)
    for packed_input in (0, 2):
        for flags in (0, 1, 2, 3):
            with kma.options(packed_input=packed_input):
                big.check(t, lo, hi, flags, k=7, what=f"K = 7 packed_input {packed_input} "
                          f"flags {flags}")


@pytest.mark.parametrize("packed_input", [0, 2], ids=["ascii-staged", "pack-kernel"])
def test_c_buffer_positions_past_2_32(kma, big, packed_input):
    """C, residues past byte 2^32 of their buffer: the same batch addressed from LEAD bytes before
    it (offsets[0] = LEAD for the whole batch), so offsets[0] + a position inside the call passes
    2^32 for the last 16 MiB. The whole batch, and its last 3,000 proteins (all of them past
    2^32) under flags 0..3 with 1 and 8 proteins per block."""
    lay = big.lay
    t = big.table()
    lo, hi = _sub_range(lay, "last")
    assert int(lay.offsets[lo]) + LEAD >= 1 << 32
    with kma.options(packed_input=packed_input):
        big.check(t, 0, lay.n_seq, 0, entry="lead", what="whole batch behind a lead")
        for flags in (0, 1, 2, 3):
            for bp in (1, 8):
                with kma.options(block_proteins=bp):
                    big.check(t, lo, hi, flags, entry="lead",
                              what=f"past 2^32, flags {flags} block_proteins {bp}")


def test_d_pre_packed_stream(kma, big):
    """D. kma_annotate_packed_device on a stream of 2^32 - 128 residues packed on the host one
    tile at a time: the whole batch, and its last 28 tiles with the tail (stream residue 0 is
    residue d_offsets[0], past 2^32 - 2^24) under flags 0..3."""
    lay = big.lay_d
    t = big.table()
    t0 = time.perf_counter()
    big.stream_d()
    big.torch.cuda.synchronize()
    print(f"\nstream built in {time.perf_counter() - t0:.2f} s")
    for flags in (0, 3):
        dt = big.check(t, 0, lay.n_seq, flags, entry="stream", what="whole stream")
        print(f"whole stream, flags {flags}: {dt:.3f} s")
    lo = (lay.reps - 28) * lay.base.n
    assert int(lay.offsets[lo]) > (1 << 32) - (1 << 24)
    for long_one in ("g30", "l60", "a30"):
        assert sc.proteins_holding(lay, long_one, lo, lay.n_seq) >= 28
    for flags in (0, 1, 2, 3):
        for bp in (1, 8):
            with kma.options(block_proteins=bp):
                big.check(t, lo, lay.n_seq, flags, entry="stream",
                          what=f"stream tail flags {flags} block_proteins {bp}")


@pytest.fixture(scope="module")
def host_batch():
    lay = sc.layout(N_HOST)
    return lay, sc.materialise(lay)


@pytest.mark.parametrize("devs", [[0], [0, 0]], ids=["one-replica", "two-replicas"])
def test_e_host_call_cut_at_the_default_slice(kma, oracle_c, host_batch, devs):
    """E. kma_annotate_proteins on 2^31 + 8 MiB residues with default options: one replica's share
    is cut at the library's own 2^31-residue slice (two device calls, tallies summed); two
    replicas on device 0 take about 2^30 each."""
    lay, res = host_batch
    _require_free(_host_call_need(kma), "the host call's contexts")
    assert kma.get_option(kma.OPT_HOST_SLICE) == 0 and kma.get_option(kma.OPT_PACKED_INPUT) == 1
    kmers, fids = sc.table_rows(K)
    with kma.SignatureTable.from_rows_replicated(kmers, fids, devs, K) as t:
        t0 = time.perf_counter()
        fid, cnt, st, tally = kma.annotate_proteins(t, res, lay.offsets, MIN_HITS, 0,
                                                    n_fid=sc.N_FID)
        print(f"\nhost call of {lay.n_total} residues, {lay.n_seq} proteins, {len(devs)} "
              f"replica(s): {time.perf_counter() - t0:.2f} s")
    efid, ecnt, est, etally = sc.expected(oracle_c, lay, K, 0)
    for name, a, b in (("status", st, est), ("fid", fid, efid), ("count", cnt, ecnt)):
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, (f"{name} differs for {bad.size} proteins, first {bad[0]} at "
                               f"residue {int(lay.offsets[bad[0]])}")
    assert (tally == etally).all() and tally.sum() > 0


def test_f_past_the_limit_is_refused(kma):
    """F. 2^32 - 127 residues: both reservations and both device entries answer KMA_E_INVALID
    before they touch device memory; the workspace stays usable."""
    import torch
    dev = torch.device("cuda", 0)
    n = (1 << 32) - 127
    msg = f"{n} residues in one call (limit 2^32 - 128)"
    ws = kma.Workspace(0)
    d = torch.zeros(64, dtype=torch.int64, device=dev)
    kmers, fids = sc.table_rows(K)
    try:
        with kma.SignatureTable.from_rows(kmers[:50], fids[:50], K) as t:
            calls = [lambda: ws.reserve(n), lambda: ws.reserve(n, 1000)]
            for entry in (kma.annotate_proteins_device, kma.annotate_packed_device):
                calls.append(lambda entry=entry: entry(t, ws, d.data_ptr(), d.data_ptr(), 1, n,
                                                       MIN_HITS, 0, d.data_ptr(), d.data_ptr(),
                                                       d.data_ptr()))
            for call in calls:
                with pytest.raises(kma.KmerAnnoError) as e:
                    call()
                assert e.value.code == kma.E_INVALID and msg in str(e.value)
            ws.reserve(1000)
            fid = torch.full((3,), -7, dtype=torch.int32, device=dev)
            cnt = torch.full((3,), -7, dtype=torch.int32, device=dev)
            st = torch.full((3,), 9, dtype=torch.uint8, device=dev)
            kma.annotate_proteins_device(t, ws, d.data_ptr(), d[8:].data_ptr(), 3, 0, MIN_HITS, 0,
                                         fid.data_ptr(), cnt.data_ptr(), st.data_ptr())
            torch.cuda.synchronize()
            assert st.cpu().tolist() == [kma.STATUS_NONE] * 3 and cnt.cpu().tolist() == [0] * 3
    finally:
        ws.close()


def test_small_call_after_the_giant_ones(kma, oracle_c, big):
    """The workspace and the table the giant calls used answer a small call exactly: the 13
    lengths of test_gpu_staged_probe.py's test_degenerate_proteins, cut from the base tile's
    called proteins, in a buffer of their own."""
    import torch
    b = big.lay.base
    lengths = [0, 3, 7, 8, 0, 0, 9, 120, 1, 0, 640, 5, 0]
    efid0, _, est0 = sc.base_expected(oracle_c, K, 0)
    src = [i for i in b.ordinary if est0[i] == sc.CALLED and int(b.off[i + 1] - b.off[i]) >= 640]
    prots = [b.res[int(b.off[src[j % len(src)]]):][:n] for j, n in enumerate(lengths)]
    off = np.zeros(len(lengths) + 1, np.uint64)
    off[1:] = np.cumsum(lengths)
    res = np.concatenate(prots + [np.zeros(32, np.uint8)])
    efid, ecnt, est = oracle_c.apply(sc.oracle_table(oracle_c, K), res, off, K, MIN_HITS, 0)
    assert (est == sc.CALLED).sum() >= 2
    d_res = torch.from_numpy(res).to(big.dev)
    d_off = torch.from_numpy(off.view(np.int64)).to(big.dev)
    n = len(lengths)
    for packed_input in (0, 2):
        big.fid[:n].fill_(-7)
        big.cnt[:n].fill_(-7)
        big.st[:n].fill_(9)
        big.tally.zero_()
        with kma.options(packed_input=packed_input):
            kma.annotate_proteins_device(big.table(), big.ws, d_res.data_ptr(), d_off.data_ptr(),
                                         n, int(off[-1]), MIN_HITS, 0, big.fid.data_ptr(),
                                         big.cnt.data_ptr(), big.st.data_ptr(),
                                         big.tally.data_ptr(), sc.N_FID)
        torch.cuda.synchronize()
        assert (big.st[:n].cpu().numpy() == est).all()
        assert (big.fid[:n].cpu().numpy() == efid).all()
        assert (big.cnt[:n].cpu().numpy() == ecnt).all()
        assert (big.tally.cpu().numpy() == np.bincount(efid[est == 1], minlength=sc.N_FID)).all()
