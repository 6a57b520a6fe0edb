"""The early-exit cases on the oracle alone (CPU): every planted protein has the status it is
meant to have, and its second fid is found in the step it is meant to be found in, by the
library's block assignment (early_exit_cases.protein_steps). tests/test_gpu_early_exit.py runs
the same batches through the probe."""
import numpy as np
import pytest

import early_exit_cases as ec


@pytest.fixture(scope="module")
def otable(oracle_c):
    from helpers import full_oracle_table
    return full_oracle_table(oracle_c, *ec.table_rows(), ec.K)


def _apply(oracle_c, otable, name, flags=0):
    res, off, names = ec.batch(name)
    fid, cnt, st = oracle_c.apply_mt(otable, res, off, ec.K, ec.MIN_HITS, flags, 4)
    return res, off, names, fid, cnt, st


def test_table():
    keys, fids = ec.table_rows()
    assert len(keys) == len(np.unique(keys)) == 78_000
    assert (fids == ec.FID_A).sum() == (fids == ec.FID_B).sum() == ec.N_ROLE


@pytest.mark.parametrize("name", ["main", "big"])
def test_statuses_and_steps_alone(oracle_c, otable, name):
    """Each protein alone in its block (capacity 1): the spec's status, the spec's steps."""
    res, off, names, fid, cnt, st = _apply(oracle_c, otable, name)
    steps = ec.protein_steps(res, off, 1)
    specs = {**ec.SPECS, **ec.BIG_SPECS}
    for p, n in enumerate(names):
        w, a, b, status, (dead, last) = specs[n]
        assert int(off[p + 1] - off[p]) == w + ec.K - 1
        assert st[p] == status, (n, st[p])
        assert steps[p] == (0, last, -1 if dead is None else dead), (n, steps[p])
        if status == ec.AMBIGUOUS:
            assert fid[p] == -1 and cnt[p] == 0
        elif status in (ec.CALLED, ec.BELOW_MIN):
            planted = {x for x in a if not isinstance(x, tuple)}  # (i, j): a repeat of j's kmer
            assert fid[p] == ec.FID_A and cnt[p] == len(planted), (n, cnt[p])
    # what the cases are for
    s = {n: steps[names.index(n)] for n in names}
    if name == "main":
        for w in (600, 1030, 1600):
            assert s[f"w{w}-b-last-of-step0"][2] == 0 and s[f"w{w}-b-first-of-step1"][2] == 1
            assert s[f"w{w}-b-last-step-only"][2] == s[f"w{w}-b-last-step-only"][1]
        assert st[names.index("w1600-b-absent")] == ec.CALLED
        assert cnt[names.index("w1600-b-absent")] >= 16  # hits in each of its four steps
        wf = ec.window_fids(res[int(off[names.index("w1600-late-single-role")]):][:1607])
        assert (wf[:512] < 0).all() and (wf[512:] >= 0).sum() >= 15
    else:
        assert s["w3000-ambiguous-midway"] == (0, 5, 2) and s["w3000-single-role"][2] == -1
        i = names.index("w3000-single-role")
        m = oracle_c.apply_mt(otable, res, off, ec.K, ec.MIN_HITS, ec.F_MULTISET, 4)[1]
        assert m[i] == cnt[i] + 3  # three kmers occur twice: the list is deduplicated


@pytest.mark.parametrize("capacity", [4, 6, 8])
def test_steps_packed(oracle_c, otable, capacity):
    """Packed in blocks of 4, 6 and 8: dead and live proteins share blocks in both orders, some
    proteins die before their last step (the skip has windows to take) and some in it."""
    res, off, names, fid, cnt, st = _apply(oracle_c, otable, "main")
    steps = ec.protein_steps(res, off, capacity)
    dead = np.array([d for _, _, d in steps])
    last = np.array([l for _, l, _ in steps])
    assert ((dead >= 0) == (st == ec.AMBIGUOUS)).all()
    assert ((dead >= 0) & (dead < last)).sum() >= 4 and ((dead >= 0) & (dead == last)).sum() >= 2
    block = np.arange(len(names)) // capacity
    pairs = set()
    for p in range(len(names) - 1):
        if block[p] == block[p + 1]:
            pairs.add((bool(dead[p] >= 0 and dead[p] < last[p + 1]), st[p + 1] == ec.CALLED))
            pairs.add((st[p] == ec.CALLED, bool(dead[p + 1] >= 0)))
    assert (True, True) in pairs  # a dead protein before a live one, and the reverse


def test_mixed_batch(oracle_c, otable):
    res, off, names, fid, cnt, st = _apply(oracle_c, otable, "mixed")
    assert len(names) == 1500
    for status in (ec.NONE, ec.CALLED, ec.BELOW_MIN, ec.AMBIGUOUS):
        assert (st == status).sum() >= 100, status
    steps = ec.protein_steps(res, off, 6)
    assert sum(1 for f, l, d in steps if 0 <= d < l) >= 50


@pytest.mark.parametrize("flags", [1, 2])
def test_flags_change_the_answer(oracle_c, otable, flags):
    """End-exclusive drops a protein's last window; the multiset counts repeats."""
    res, off, names, fid, cnt, st = _apply(oracle_c, otable, "main")
    _, _, _, fid2, cnt2, st2 = _apply(oracle_c, otable, "main", flags)
    if flags == ec.F_MULTISET:
        i = names.index("w600-live")
        assert cnt2[i] == cnt[i] + 1 and (st2 == st).all()
    else:
        assert (st2 == st).all()  # no planted kmer sits in a last window
