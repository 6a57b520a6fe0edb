"""The workloads of tests/alphabet_cases.py meet the conditions tests/test_gpu_alphabet.py relies
on, shown on the oracle alone (no GPU): every status often enough, called proteins that owe
counted hits to kmers holding the codes 26..31 and the all-ones code 31, the special rows and the
zero-low-word windows present, no protein near the fid-0 row, and the C oracle equal to its
Python twin. Each test prints the counts the conditions are about (pytest -s shows them)."""
import numpy as np
import pytest

import alphabet_cases as ac
from oracle import oracle_py

F_MULTISET = 2
CASES = [(k, extra) for k in ac.KS for extra in (False, True)]
IDS = [f"k{k}-{'extra' if e else 'std'}" for k, e in CASES]


def _windows(p, k):
    return [p[i:i + k] for i in range(len(p) - k + 1)]


def _holds(kmer, lut, lo):
    return max(lut[c] for c in kmer) >= lo


@pytest.mark.parametrize("k,extra", CASES, ids=IDS)
def test_alphabet_workload_conditions(oracle_c, k, extra):
    wl = ac.workload(k, extra)
    lut = ac.code_of(extra)
    assert 1400 <= len(wl.prots) <= 1600 and max(len(p) for p in wl.prots) <= 600
    assert min(len(p) for p in wl.prots) == 0 and 2000 <= len(wl.rows) <= 6000
    for flags in (0, F_MULTISET):
        fid, cnt, st = ac.oracle_apply(oracle_c, k, extra, flags)
        by_status = np.bincount(st, minlength=4)
        called = np.flatnonzero(st == oracle_py.STATUS_CALLED)
        high = top = 0
        hits_high = hits_top = 0
        for j in called:
            hit = [w for w in _windows(wl.prots[j], k) if w in wl.table]
            if not flags:
                hit = list(dict.fromkeys(hit))
            assert len(hit) == cnt[j] and {wl.table[w] for w in hit} == {int(fid[j])}
            h = sum(_holds(w, lut, 26) for w in hit)
            t = sum(_holds(w, lut, 31) for w in hit)
            high, top, hits_high, hits_top = high + (h > 0), top + (t > 0), hits_high + h, hits_top + t
        print(f"K={k} extra={int(extra)} flags={flags}: rows {len(wl.rows)} entries {len(wl.table)} "
              f"none {by_status[0]} called {by_status[1]} ambiguous {by_status[2]} below-min "
              f"{by_status[3]}; called with a hit on a code >= 26: {high} ({hits_high} hits), on "
              f"code 31: {top} ({hits_top} hits)")
        assert by_status.min() >= 50
        assert high >= 200
        if extra:  # a table without extra symbols has no code above 27
            assert top >= 50
        else:
            assert top == 0
        assert not (fid == 0).any()
    cnt_s, cnt_m = (ac.oracle_apply(oracle_c, k, extra, f)[1] for f in (0, F_MULTISET))
    assert (cnt_m > cnt_s).sum() >= 30
    k0 = ac.fid0_kmer(k)
    assert wl.table[k0] == 0 and list(wl.table.values()).count(0) == 1
    assert not any(k0 in p for p in wl.prots)


@pytest.mark.parametrize("k,extra", CASES, ids=IDS)
def test_alphabet_table_rows(k, extra):
    """The table file: all symbols present (the four extra ones exactly when asked for), the
    stratum of codes 26..31, the special rows with their roles and each inside a protein,
    duplicate kmers under another fid, rows of other lengths."""
    wl = ac.workload(k, extra)
    lut = ac.code_of(extra)
    klen = [km for km in wl.kmers if len(km) == k]
    seen = set(b"".join(klen))
    assert seen == set(ac.STD + (ac.EXTRA if extra else b""))
    assert sum(min(lut[c] for c in km) >= 26 for km in wl.table) >= (100 if extra else 20)
    top = ac.EXTRA[3:] if extra else b"*"
    special = ac.special_rows(k, extra)
    for fid, kmers in special.items():
        assert kmers and len(set(kmers)) == len(kmers)
        for km in kmers:
            assert len(km) == k and wl.table[km] == fid
            assert any(km in p for p in wl.prots), km
    for km in (b"Z" * k, b"*" * k, top + b"A" * (k - 1)) + ((top * k,) if extra else ()):
        assert km in special[ac.FID_TOP]
    assert all(km[-1:] == top and top not in km[:-1] for km in special[ac.FID_LAST])
    if k == 8:
        for x in range(5):
            ties = [km for km in special[ac.FID_TIE]
                    if [i for i in range(8) if lut[km[i]] == max(lut[c] for c in km)] == [x, x + 3]]
            assert len(ties) >= 3
    by_kmer = {}
    for km, f in wl.rows:
        by_kmer.setdefault(km, []).append(f)
    changed = sum(len(set(v)) > 1 for v in by_kmer.values())
    assert 0.01 * len(wl.rows) <= changed <= 0.04 * len(wl.rows)
    assert sum(v[-1] != v[0] for v in by_kmer.values()) >= 10  # the last row wins, and differs
    assert 3 <= wl.n_skipped <= 10 and len(wl.rows[-1][0]) == k
    assert set(wl.fids.tolist()) == set(range(ac.N_FID))


@pytest.mark.parametrize("k,extra", [(7, False), (7, True), (8, False), (8, True)])
def test_zero_low_word_windows(k, extra):
    """Every zero-low-word window packs to a key that is not 0 and has a zero low dword, is a
    protein of exactly K residues, and sits in a protein with at least 5 table kmers of one role
    on either side."""
    wl = ac.workload(k, extra)
    lut = ac.code_of(extra)
    wins = ac.zero_low_windows(k, extra)
    assert len(wins) == 2 * (6 + extra)
    for s, w in wins:
        assert len(w) == k
        key = int(ac.pack_codes(lut[np.frombuffer(w, np.uint8)][None, :])[0])
        assert key != 0 and key & 0xFFFFFFFF == 0
        if k == 8 and extra and s == ac.EXTRA[3:]:
            assert key >> 35 == 31
        assert w in wl.prots
        hosts = [p for p in wl.prots if w in p and len(p) > k]
        assert hosts
        for p in hosts[:1]:
            at = p.index(w)
            for side in (p[:at], p[at + k:]):
                hit = {x for x in _windows(side, k) if x in wl.table}
                assert len(hit) >= 5 and len({wl.table[x] for x in hit}) == 1


@pytest.mark.parametrize("k,extra", CASES, ids=IDS)
def test_alphabet_workload_python_twin(oracle_c, k, extra):
    """oracle_py (bytes / dict) equals the C oracle on a 100-protein sample, set and multiset."""
    wl = ac.workload(k, extra)
    table = oracle_py.load_table(wl.rows)
    sample = np.random.default_rng(k).choice(len(wl.prots), 100, replace=False)
    for flags in (0, F_MULTISET):
        fid, cnt, st = ac.oracle_apply(oracle_c, k, extra, flags)
        for j in sample:
            s, role, n = oracle_py.apply_protein(table, wl.prots[j], ac.MIN_HITS, k, False,
                                                 flags == F_MULTISET)
            assert (s, -1 if role is None else role, n) == (int(st[j]), int(fid[j]), int(cnt[j])), j


@pytest.mark.parametrize("k", [8, 12])
def test_dump_keys_shape(k):
    """The slot-dump keys: all 31 codes, the all-ones key, first residues of code 31 (at K = 8 a
    top key byte of 0xFF too), mod-sampling ties, repeated keys whose last row wins."""
    keys, fids, want = ac.dump_keys(k)
    codes = ac.key_codes(keys, k)
    assert set(np.unique(codes).tolist()) == set(range(1, 32)) and (keys != 0).all()
    assert (1 << (5 * k)) - 1 in want and len(want) < len(keys) - 300
    assert (codes[:, 0] == 31).sum() > 500
    if k == 8:
        assert (keys >> np.uint64(32) == 0xFF).sum() > 20
    mx = codes.max(axis=1, keepdims=True)
    for x in range(5):
        at = np.zeros(k, bool)
        at[[x, x + 3]] = True
        assert (((codes == mx) == at).all(axis=1) & (mx[:, 0] == 31)).sum() >= 5
    last = {}
    for key, f in zip(keys.tolist(), fids.tolist()):
        last[key] = f
    assert last == want
    print(f"K={k} slot dump: {len(want)} keys, {int((codes.max(axis=1) >= 26).sum())} rows hold a "
          f"code >= 26, {int((codes == 31).any(axis=1).sum())} hold code 31")


@pytest.mark.parametrize("k", [4, 8, 12])
def test_peg_case_shape(oracle_c, k):
    """The pegs: lengths 0, K and K + 1, 'X' runs, lower case and EXTRA bytes, kmers repeated
    inside a peg and across pegs; singletons that hold 'Z' and '*'."""
    pegs = ac.peg_case(k)
    lens = {len(p) for p in pegs}
    assert {0, k, k + 1} <= lens and any(b"X" * k in p for p in pegs)
    assert all(any(bytes([c]) in p for p in pegs) for c in ac.EXTRA + b"xz")
    res, off = oracle_c.pack_strings(pegs)
    km, pg, _ = oracle_c.peg_kmers(res, off, k)
    rows = [r.tobytes() for r in km]
    kmers, owner = ac.peg_singletons(oracle_c, k, pegs)
    assert len(set(kmers)) == len(kmers) < len(set(rows))
    count = {}
    for r, p in zip(rows, pg.tolist()):
        count.setdefault(r, []).append(p)
    inside = sum(len(v) > 1 and len(set(v)) == 1 for v in count.values())
    across = sum(len(set(v)) > 1 for v in count.values())
    assert inside >= 5 and across >= 5
    std = set(ac.STD)
    assert set(kmers) == {r for r, v in count.items() if len(v) == 1 and set(r) <= std}
    assert all(count[r] == [p] for r, p in zip(kmers, owner.tolist()))
    high = sum(b"Z" in r or b"*" in r for r in kmers)
    assert high >= 1000 and sum(b"*" in r for r in kmers) >= 300
    print(f"K={k} pegs: {len(rows)} windows, {len(kmers)} singletons, {high} hold a code >= 26")


def test_set_op_proteins_shape():
    prots = ac.set_op_proteins()
    lut = ac.code_of(False)
    assert len(prots) == 200 and all(set(p) <= set(ac.STD) for p in prots)
    text = b"".join(prots)
    assert sum(c in ac.RARE for c in text) > 0.4 * len(text)
    assert b"*" * 12 in prots and any(len(p) == 0 for p in prots)
    for k in (1, 2, 8, 12):
        wins = [w for p in prots for w in _windows(p, k)]
        print(f"K={k} set operators: {len(wins)} windows, {sum(_holds(w, lut, 26) for w in wins)} "
              f"hold a code >= 26")
        assert b"*" * k in wins
