"""The tiled batches of tests/scale_cases.py, shown on the oracle alone (no GPU): the oracle run on
an explicit batch of 3 and of 5 tiles (plus the partial tile and the filler) equals the tiled
expectation that tests/test_gpu_scale32.py holds the 2^32 - 128-residue calls to, and the base
tile meets the conditions those tests rely on. Each test prints the counts its conditions are
about (pytest -s shows them)."""
import numpy as np
import pytest

import scale_cases as sc


@pytest.mark.parametrize("aligned", [False, True], ids=["odd-tile", "tile-of-64s"])
def test_base_tile_conditions(oracle_c, aligned):
    b = sc.base(aligned)
    lens = np.diff(b.off.view(np.int64))
    fid, cnt, st = sc.base_expected(oracle_c, 8, 0, aligned)
    by = np.bincount(st[b.ordinary], minlength=4)
    print(f"tile: {b.n} proteins, {b.T} residues; ordinary none {by[0]} called {by[1]} "
          f"ambiguous {by[2]} below-min {by[3]}")
    assert 90 <= b.n <= 120 and (lens[b.ordinary] >= 50).all() and (lens[b.ordinary] <= 900).all()
    assert by[sc.CALLED] >= 20 and by[sc.AMBIGUOUS] >= 10 and by[sc.NONE] >= 10
    assert by[sc.BELOW_MIN] >= 5
    if aligned:
        assert b.T % 64 == 0
    else:
        assert b.T % 2 == 1 and b.T % 8 != 0 and b.T % 64 != 0
    # empty proteins and K - 1, K, K + 1 residues for K = 8 and K = 7
    assert sorted(lens[b.tiny].tolist()) == [0, 0, 0, 1, 6, 7, 8, 8, 8, 9]
    assert (st[b.tiny][lens[b.tiny] < 8] == sc.NONE).all()
    assert (st[b.tiny][lens[b.tiny] >= 8] == sc.BELOW_MIN).all()
    # the long proteins: present, single-role where they are meant to be
    assert lens[b.g30] == 30_000 and st[b.g30] == sc.CALLED and fid[b.g30] == 3
    assert cnt[b.g30] == sc.PROTO_LEN - 7  # ten copies of one prototype: its windows, once each
    assert lens[b.l60] == 60_000 and st[b.l60] == sc.CALLED and fid[b.l60] == sc.FID_LONG
    assert cnt[b.l60] == sc.LONG_LEN       # every window a row; 3,000 distinct ones
    assert lens[b.a30] == 30_000 and st[b.a30] == sc.AMBIGUOUS
    assert st[b.high] == sc.CALLED and fid[b.high] == sc.FID_HIGH
    # every window counts under KMA_F_MULTISET: more hits than the LDS pool's 4,096 entries for
    # l60 (its list takes the hash-set branch), fewer for g30 (deduplicated in the pool)
    mfid, mcnt, mst = sc.base_expected(oracle_c, 8, 2, aligned)
    print(f"hits: g30 {mcnt[b.g30]}, l60 {mcnt[b.l60]}")
    assert mcnt[b.l60] == 60_000 - 7 and 0 < mcnt[b.g30] < 4096
    # K = 7: the same residues against the 7-window table
    fid7, cnt7, st7 = sc.base_expected(oracle_c, 7, 0, aligned)
    assert st7[b.l60] == sc.CALLED and st7[b.g30] == sc.CALLED and st7[b.a30] == sc.AMBIGUOUS
    assert (st7[b.tiny][lens[b.tiny] == 7] == sc.BELOW_MIN).all()


def test_table_rows():
    for k in sc.KS:
        kmers, fids = sc.table_rows(k)
        print(f"K = {k}: {len(kmers)} rows")
        assert 5000 <= len(kmers) <= 10_000 and len(set(kmers)) == len(kmers)
        assert fids.min() == 1 and fids.max() == sc.N_FID - 1
        assert all(len(km) == k for km in kmers)


@pytest.mark.parametrize("n_total", [12_345, sc.N_MAX, (1 << 31) + (8 << 20)])
@pytest.mark.parametrize("aligned", [False, True])
def test_filler_arithmetic(n_total, aligned):
    """offsets[-1] is exactly the requested N; the tail is whole proteins and a filler of at
    least MIN_FILLER residues; one more protein would not leave room for it."""
    lay = sc.layout(n_total, aligned)
    b = lay.base
    off = lay.offsets
    assert off.dtype == np.uint64 and int(off[0]) == 0 and int(off[-1]) == n_total
    assert lay.n_seq == lay.reps * b.n + lay.m + 1 == len(off) - 1
    assert int(off[-1] - off[-2]) == lay.filler >= sc.MIN_FILLER
    assert int(off[-2]) == lay.reps * b.T + int(b.off[lay.m])
    if lay.m < b.n:
        assert lay.reps * b.T + int(b.off[lay.m + 1]) + sc.MIN_FILLER > n_total
    # tile r repeats the base tile's lengths
    for r in (0, lay.reps // 2, lay.reps - 1):
        if r >= 0 and lay.reps:
            seg = off[r * b.n:(r + 1) * b.n + 1]
            assert (seg - seg[0] == b.off).all()


def test_remainder_too_short_drops_a_tile():
    b = sc.base()
    lay = sc.layout(3 * b.T + 5)  # 5 residues cannot hold the filler
    # one tile fewer; the partial tile then drops its last protein too, which would again leave 5
    assert lay.reps == 2 and lay.m == b.n - 1
    assert lay.filler == 5 + b.T - int(b.off[b.n - 1]) >= sc.MIN_FILLER
    lay = sc.layout(3 * b.T + sc.MIN_FILLER)
    assert lay.reps == 3 and lay.filler >= sc.MIN_FILLER and int(lay.offsets[-1]) == 3 * b.T + 16


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("reps,aligned,k", [(3, False, 8), (5, False, 8), (3, True, 8),
                                            (5, False, 7)])
def test_oracle_equals_tiled_expectation(oracle_c, reps, aligned, k, flags):
    """The oracle on the materialised batch (reps tiles, a partial tile, the filler) equals the
    tiled expectation, tally included; so does any sub-range of it."""
    b = sc.base(aligned)
    lay = sc.layout(reps * b.T + int(b.off[b.n // 2]) + 777, aligned)
    assert lay.reps == reps and 0 < lay.m < b.n
    res = sc.materialise(lay)
    assert len(res) == lay.n_total + 32
    fid, cnt, st = oracle_c.apply_mt(sc.oracle_table(oracle_c, k), res, lay.offsets, k,
                                     sc.MIN_HITS, flags, 4)
    tally = np.bincount(fid[st == sc.CALLED], minlength=sc.N_FID).astype(np.uint32)
    efid, ecnt, est, etally = sc.expected(oracle_c, lay, k, flags)
    assert (st == est).all() and (fid == efid).all() and (cnt == ecnt).all()
    assert (tally == etally).all() and tally.sum() > 0
    assert st[-1] == sc.NONE and cnt[-1] == 0
    # the whole tiles' share of the tally is reps x the base tile's
    bfid, _, bst = sc.base_expected(oracle_c, k, flags, aligned)
    whole = sc.expected(oracle_c, lay, k, flags, 0, reps * b.n)[3]
    assert (whole == reps * np.bincount(bfid[bst == sc.CALLED], minlength=sc.N_FID)).all()
    lo, hi = b.n + 7, lay.n_seq - 3
    sfid, scnt, sst, stally = sc.expected(oracle_c, lay, k, flags, lo, hi)
    assert (sst == st[lo:hi]).all() and (sfid == fid[lo:hi]).all() and (scnt == cnt[lo:hi]).all()
    assert (stally == np.bincount(fid[lo:hi][st[lo:hi] == sc.CALLED], minlength=sc.N_FID)).all()
    assert sc.proteins_holding(lay, "l60", 0, lay.n_seq) in (reps, reps + 1)
