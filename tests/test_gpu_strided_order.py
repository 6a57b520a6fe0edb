"""The protein probe's strided step order: a block's span of T steps is cut into 64-position
chunks, and slot r = 4 j + wave takes chunk r T + s in step s, so that every step samples the
whole span (kma_internal.h). The ASCII probe reads the residues of two steps from an
LDS stage of one 136-residue region per slot. The order changes which windows the early exit
skips and nothing else: every fid, count, status and tally here equals oracle.c_oracle.apply_mt
by ==.

The batches (tests/strided_order_cases.py, and the early-exit batches) run at block capacities
1, 4, 6 and 8, through the device entry and the host entry, with KMA_OPT_PACKED_INPUT 0 (the
staged ASCII probe) and 2 (the stream probe), extraction flags 0, 1 and 2, and on three tables:
two-choice placement at load factor 0.5, and two-choice and chained placement at load factor
0.9. The device entry gets a batch whose first residue is at byte 11 of its buffer
(offsets[0] = 11: the stage's funnel shift is 3 bytes) and whose last protein ends at the
batch's last byte, followed by the 32 readable bytes the ABI asks for, filled with table kmers.

What fails if the map or the stage is wrong: a chunk probed twice or not at all, a region read
at the wrong offset or a stage group left unread changes a single-role protein's exact count; a
window across two proteins that is probed, or a window past the span that is not masked, turns
a CALLED protein AMBIGUOUS; a dead mask applied to the wrong protein loses a live one's hits."""
import numpy as np
import pytest

import early_exit_cases as ec
import strided_order_cases as sc

pytestmark = pytest.mark.gpu
PAD = 32  # bytes the ABI header promises readable past offsets[n_seq]
FIRST = 11
NAMES = ("fid", "count", "status", "tally")


@pytest.fixture(scope="module")
def kma(native_lib):
    import kmeranno
    assert kmeranno.device_count() >= 1
    return kmeranno


@pytest.fixture(scope="module")
def otable(oracle_c):
    from helpers import full_oracle_table
    return full_oracle_table(oracle_c, *ec.table_rows(), ec.K)


_WANT = {}


def _want(oracle_c, otable, name, flags):
    """The oracle's (fid, count, status, tally), computed once per batch and flags."""
    if (name, flags) not in _WANT:
        res, off, _ = sc.batch(name)
        fid, cnt, st = oracle_c.apply_mt(otable, res, off, ec.K, ec.MIN_HITS, flags, 4)
        tally = np.bincount(fid[st == ec.CALLED], minlength=ec.N_FID).astype(np.uint32)
        for a in (fid, cnt, st, tally):
            a.setflags(write=False)
        _WANT[name, flags] = (fid, cnt, st, tally)
    return _WANT[name, flags]


@pytest.fixture(scope="module", params=["two-choice", "two-choice-lf0.9", "chained-lf0.9"])
def table(request, kma):
    chained = request.param.startswith("chained")
    lf = 0.9 if request.param.endswith("0.9") else 0.5
    kma.set_option(kma.OPT_PLACEMENT, 0 if chained else -1)
    try:
        t = kma.SignatureTable.from_packed(*ec.table_rows(), ec.K, load_factor=lf)
    finally:
        kma.set_option(kma.OPT_PLACEMENT, -1)
    assert t.info.two_choice == (0 if chained else 1)
    yield t
    t.close()


def _device(kma, t, res, off, flags):
    """The device entry on a buffer whose first residue is at byte FIRST (unaligned) and that
    ends PAD bytes after the batch's last residue; those bytes hold kmers of both roles."""
    import torch
    dev = torch.device("cuda", 0)
    n, n_res = len(off) - 1, int(off[-1])
    buf = np.empty(FIRST + n_res + PAD, np.uint8)
    buf[:FIRST] = np.resize(ec.role_kmer("B", 7), FIRST)
    buf[FIRST:FIRST + n_res] = res[:n_res]
    buf[FIRST + n_res:] = np.concatenate([ec.role_kmer("B", 8), ec.role_kmer("A", 9)] * 2)
    d_res = torch.from_numpy(buf).to(dev)
    assert d_res.data_ptr() % 8 == 0
    d_off = torch.from_numpy((off + np.uint64(FIRST)).view(np.int64).copy()).to(dev)
    fid = torch.full((n,), -7, dtype=torch.int32, device=dev)
    cnt = torch.full((n,), -7, dtype=torch.int32, device=dev)
    st = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    tally = torch.zeros(ec.N_FID, dtype=torch.int32, device=dev)
    ws = kma.Workspace(0, n_res, n)
    try:
        kma.annotate_proteins_device(t, ws, d_res.data_ptr(), d_off.data_ptr(), n, n_res,
                                     ec.MIN_HITS, flags, fid.data_ptr(), cnt.data_ptr(),
                                     st.data_ptr(), tally.data_ptr(), ec.N_FID,
                                     torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        ws.close()
    return (fid.cpu().numpy(), cnt.cpu().numpy(), st.cpu().numpy(),
            tally.cpu().numpy().astype(np.uint32))


def _host(kma, t, res, off, flags):
    fid, cnt, st, tally = kma.annotate_proteins(t, res, off, ec.MIN_HITS, flags, ec.N_FID)
    return fid, cnt, st, tally.astype(np.uint32)


def _run(kma, oracle_c, otable, t, name, capacity, entry, modes=(0, 2), all_flags=(0, 1, 2)):
    res, off, names = sc.batch(name)
    for flags in all_flags:
        want = _want(oracle_c, otable, name, flags)
        for mode in modes:
            with kma.options(block_proteins=capacity, packed_input=mode):
                got = (_device if entry == "device" else _host)(kma, t, res, off, flags)
            for g, w, what in zip(got, want, NAMES):
                bad = np.flatnonzero(g != w)
                assert not len(bad), (what, flags, mode, [(int(i), names[i] if what != "tally"
                                                           else "", int(g[i]), int(w[i]))
                                                          for i in bad[:5]])


@pytest.mark.parametrize("entry", ["device", "host"])
@pytest.mark.parametrize("capacity", [1, 4, 6, 8])
def test_span_lengths_and_chunk_edges(kma, oracle_c, otable, table, capacity, entry):
    """Spans of T = 1, 2, 3, 4, 5 and 12 steps, lengths that are and are not multiples of 64 and
    of 512 (the last slots own chunks wholly past the span), a kmer at the last window of a
    chunk and the first of another in both steps of a stage pair and at both ends of every
    slot's part of the span; two roles in different slots of one step."""
    _run(kma, oracle_c, otable, table, "spans", capacity, entry)


@pytest.mark.parametrize("entry", ["device", "host"])
@pytest.mark.parametrize("capacity", [1, 4, 6, 8])
def test_early_exit_across_the_span(kma, oracle_c, otable, table, capacity, entry):
    """A two-role protein late in the span, dead in step 0 through a high slot, beside
    single-role proteins early in the span that hit in the last two steps only."""
    _run(kma, oracle_c, otable, table, "across", capacity, entry)


@pytest.mark.parametrize("entry", ["device", "host"])
@pytest.mark.parametrize("capacity", [1, 4, 6, 8])
def test_windows_across_two_proteins(kma, oracle_c, otable, table, capacity, entry):
    """Short proteins, several per chunk, with a table kmer across every border."""
    _run(kma, oracle_c, otable, table, "straddle", capacity, entry)


@pytest.mark.parametrize("entry", ["device", "host"])
@pytest.mark.parametrize("capacity", [1, 4, 6, 8])
def test_early_exit_batches(kma, oracle_c, otable, table, capacity, entry):
    """The early-exit tests' planted proteins (600 to 1,600 windows, dead and live in one
    block), from an unaligned buffer."""
    _run(kma, oracle_c, otable, table, "main", capacity, entry)


@pytest.mark.parametrize("entry", ["device", "host"])
@pytest.mark.parametrize("capacity", [1, 6])
def test_workspace_lists(kma, oracle_c, otable, table, capacity, entry):
    """Proteins of 3,000 windows, whose sets overflow the LDS pool; at capacity 1 the single-role
    one with repeated kmers is a span of its own, and its exact distinct count is reported."""
    _run(kma, oracle_c, otable, table, "big", capacity, entry)
    want = _want(oracle_c, otable, "big", 0)
    i = ec.BIG_ORDER.index("w3000-single-role")
    assert want[2][i] == ec.CALLED and want[1][i] > 60


@pytest.mark.parametrize("capacity", [4, 6, 8])
def test_mixed_batch(kma, oracle_c, otable, table, capacity):
    """1,500 mixed proteins with a tally, device and host entry."""
    for entry in ("device", "host"):
        _run(kma, oracle_c, otable, table, "mixed", capacity, entry, all_flags=(0, 2))
