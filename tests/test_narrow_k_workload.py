"""The K = 1..7 workloads of tests/test_gpu_narrow_k.py meet the conditions its GPU tests rely on,
shown on the oracle alone (no GPU): enough proteins of every status, duplicate windows that make
set and multiset counts differ, last windows that make the two window conventions differ, and
the C oracle equal to its Python twin on them."""
import numpy as np
import pytest

from oracle import oracle_py
from test_gpu_narrow_k import (CONTIG_TILE, KS, MIN_HITS, N_FID, _contig_strings, narrow_workload,
                               oracle_apply)

F_END_EXCLUSIVE, F_MULTISET = 1, 2


@pytest.mark.parametrize("k", KS)
def test_narrow_workload_conditions(oracle_c, k):
    wl = narrow_workload(k)
    fid, cnt, st = oracle_apply(oracle_c, k, 0)
    cnt_x = oracle_apply(oracle_c, k, F_END_EXCLUSIVE)[1]
    cnt_m = oracle_apply(oracle_c, k, F_MULTISET)[1]
    by_status = np.bincount(st, minlength=4)
    called = st == oracle_py.STATUS_CALLED
    more = int((called & (cnt_m > cnt)).sum())
    differ = int((cnt_x != cnt).sum())
    print(f"K={k}: rows {len(wl.rows)} entries {wl.n_entries} none {by_status[0]} called "
          f"{by_status[1]} ambiguous {by_status[2]} below-min {by_status[3]} max count "
          f"{cnt.max()} multiset {cnt_m.max()} multiset>set {more} end-exclusive differs {differ}")
    assert by_status[oracle_py.STATUS_CALLED] >= 100
    assert by_status[oracle_py.STATUS_AMBIGUOUS] >= 20
    assert by_status[oracle_py.STATUS_NONE] >= 100
    assert by_status[oracle_py.STATUS_BELOW_MIN] >= 50
    assert more >= 30
    assert differ >= 30
    # table file: duplicates under another role (the last row wins), rows of other lengths
    by_kmer = {}
    for km, f in wl.rows:
        by_kmer.setdefault(km, []).append(f)
    assert sum(len(set(v)) > 1 for v in by_kmer.values()) >= 1
    assert sum(len(km) != k for km, _ in wl.rows) == wl.n_skipped > 0
    assert len(wl.rows[-1][0]) == k and set(wl.fids.tolist()) == set(range(N_FID))


@pytest.mark.parametrize("k", KS)
def test_narrow_workload_python_twin(oracle_c, k):
    """oracle_py (str / dict / set) equals the C oracle on the first 60 proteins, for both window
    conventions and multiset counting."""
    wl = narrow_workload(k)
    table = oracle_py.load_table(wl.rows)
    for flags in (0, F_END_EXCLUSIVE, F_MULTISET):
        fid, cnt, st = oracle_apply(oracle_c, k, flags)
        for j, p in enumerate(wl.prots[:60]):
            s, role, n = oracle_py.apply_protein(table, p, MIN_HITS, k, flags == F_END_EXCLUSIVE,
                                                 flags == F_MULTISET)
            assert (s, -1 if role is None else role, n) == (int(st[j]), int(fid[j]), int(cnt[j])), \
                (k, flags, j)


@pytest.mark.parametrize("k", range(1, 13))
def test_size_rule_layout_is_a_dispatched_code(native_lib, k):
    """The creators' layout code (kma_table_layout_for: kma::minimizer_len and the placement) for
    every K, forced layout, placement and table size is one the kernels are instantiated for
    (dispatch_m: 0, min(K, 6), min(K, 7); the mod-sampling order at K = 8, m = 6 alone) and one
    the layout check of kma_table_wrap_device accepts; two-choice placement needs a narrow
    table of two buckets or more."""
    import ctypes as C
    import kmeranno as kma
    for forced in (-1, 0, 6, 7, 6 | kma.LAYOUT_MOD_SAMPLING):
        for placement in (-1, 0):
            for nb in (1, 2, 3, 1000, 1 << 25, (1 << 25) + 1, 1 << 27):
                with kma.options(layout=forced, placement=placement):
                    code = kma.layout_for(k, nb)
                m, order = code & 0x3F, code & kma.LAYOUT_MOD_SAMPLING
                assert code & ~(0x3F | kma.LAYOUT_MOD_SAMPLING | kma.LAYOUT_TWO_CHOICE) == 0
                assert m in (0, min(k, 6), min(k, 7)), (forced, placement, nb, code)
                assert not order or (k == 8 and m == 6)
                if forced in (0, 6, 7):
                    assert m == (0 if forced == 0 else min(k, forced)) and not order
                assert bool(code & kma.LAYOUT_TWO_CHOICE) == (k <= 8 and placement != 0 and nb >= 2)
                h = C.c_void_p()
                rc = native_lib.kma_table_wrap_device(C.c_void_p(4096), nb, k, code, 0, C.byref(h))
                assert rc in (kma.E_DEVICE, kma.OK), (forced, placement, nb, code)
                if rc == kma.OK:
                    native_lib.kma_table_destroy(h)


@pytest.mark.parametrize("k", KS)
def test_narrow_contigs_shape(k):
    """The 6-frame inputs: about 70 kb, every length from 3K-4 to 3K+11, more than 64 contigs
    inside one tile, an all-'n' and an empty contig, and ends 0, 1, 3K-1, 3K and 3K+2 bases past
    a tile boundary."""
    contigs = _contig_strings(k)
    lens = np.array([len(c) for c in contigs])
    off = np.concatenate([[0], np.cumsum(lens)])
    assert 60_000 <= off[-1] <= 80_000
    assert set(range(max(0, 3 * k - 4), 3 * k + 12)) <= set(lens.tolist())
    first_tile, last_tile = off[:-1] // CONTIG_TILE, np.maximum(off[1:] - 1, off[:-1]) // CONTIG_TILE
    per_tile = [int(((first_tile <= t) & (last_tile >= t) & (lens > 0)).sum())
                for t in range(int(off[-1]) // CONTIG_TILE + 1)]
    assert max(per_tile) > 64
    assert "" in contigs and any(c and set(c) == {"n"} for c in contigs)
    ends = {int(e) % CONTIG_TILE for e, n in zip(off[1:], lens) if n > CONTIG_TILE}
    assert {p % CONTIG_TILE for p in (0, 1, 3 * k - 1, 3 * k, 3 * k + 2)} <= ends
