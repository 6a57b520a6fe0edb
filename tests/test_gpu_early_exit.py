"""The protein probe's early exit: a protein with two different fids on its record is dead, and
from the next 512-window step of its block on its windows are not probed, its queued walks are
dropped and its workspace list is not deduplicated. None of that may change an output: every
fid, count, status and tally here equals oracle.c_oracle.apply_mt by ==.

The batches (tests/early_exit_cases.py; their statuses and steps are shown on the oracle in
tests/test_early_exit_workload.py) run with each protein alone in its block (capacity 1) and
packed at capacities 4, 6 and 8, through the device entry and the host entry, with
KMA_OPT_PACKED_INPUT 0 (the staged ASCII probe) and 2 (the stream probe), extraction flags 0, 1
and 2, and on three tables: two-choice placement at load factor 0.5, and two-choice and chained
placement at load factor 0.9, where many of the planted keys sit in alternate buckets, so that
walks are queued for dead and live proteins alike.

What fails if the skip is wrong: a single-role protein that is skipped loses hits (its count
falls, or CALLED turns BELOW_MIN / NONE); a mask indexed by step or shifted by one protein
skips the live neighbour of a dead protein."""
import numpy as np
import pytest

import early_exit_cases as ec

pytestmark = pytest.mark.gpu
PAD = 32
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
        res, off, _ = ec.batch(name)
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
    if lf == 0.9:  # keys in alternate buckets: their windows queue walks
        assert t.info.n_displaced > 1000
    yield t
    t.close()


def _device(kma, t, res, off, flags):
    import torch
    dev = torch.device("cuda", 0)
    n, n_res = len(off) - 1, int(off[-1])
    d_res = torch.from_numpy(res[:n_res + PAD].copy()).to(dev)
    d_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
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
    res, off, names = ec.batch(name)
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
def test_planted_proteins(kma, oracle_c, otable, table, capacity, entry):
    """600, 1,030 and 1,600 windows; B's only kmer at the last window of step 0, the first of
    step 1, in the last step only, or absent; single-role proteins with hits in every step and
    with none in step 0; dead proteins before and after live ones in one block."""
    _run(kma, oracle_c, otable, table, "main", capacity, entry)


@pytest.mark.parametrize("entry", ["device", "host"])
@pytest.mark.parametrize("capacity", [1, 6])
def test_workspace_lists(kma, oracle_c, otable, table, capacity, entry):
    """Proteins of 3,000 windows, whose sets overflow the LDS pool: one turns ambiguous midway
    (its list is dropped), one stays single-role with repeated kmers (its list is deduplicated
    and its exact count reported)."""
    _run(kma, oracle_c, otable, table, "big", capacity, entry)
    want = _want(oracle_c, otable, "big", 0)
    i = ec.BIG_ORDER.index("w3000-single-role")
    assert want[2][i] == ec.CALLED and want[1][i] > 60


@pytest.mark.parametrize("capacity", [4, 6, 8])
def test_mixed_batch(kma, oracle_c, otable, table, capacity):
    """1,500 mixed proteins with a tally, device and host entry."""
    for entry in ("device", "host"):
        _run(kma, oracle_c, otable, table, "mixed", capacity, entry, all_flags=(0, 2))
    assert _want(oracle_c, otable, "mixed", 0)[3].sum() >= 100
