"""CPU checks of the strided step order's test inputs and of its model.

scripts/early_exit_model.py's strided_skipped_windows figure comes from a closed form (a
protein's dead step is the second smallest, over its distinct fids, of the earliest step in
which that fid is hit; skipped are its windows in later steps). Here it is checked, protein by
protein, against a window-by-window simulation of the step order
(strided_order_cases.brute_force_dead_steps) on small synthetic batches, and the new batches of
tests/test_gpu_strided_order.py are shown on the oracle to be what their docstrings say."""
import importlib.util
import os

import numpy as np
import pytest

import early_exit_cases as ec
import strided_order_cases as sc

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


@pytest.fixture(scope="module")
def model():
    spec = importlib.util.spec_from_file_location(
        "early_exit_model", os.path.join(ROOT, "scripts", "early_exit_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def otable(oracle_c):
    from helpers import full_oracle_table
    return full_oracle_table(oracle_c, *ec.table_rows(), ec.K)


def _model_inputs(res, off, capacity):
    off = np.asarray(off, np.int64)
    n = len(off) - 1
    first = np.arange(n) - np.arange(n) % capacity
    base = off[:-1] - off[first]
    span = off[np.minimum(first + capacity, n)] - off[first]
    T = np.maximum((span + sc.STEP - 1) // sc.STEP, 1)
    w = np.maximum(off[1:] - off[:-1] - ec.K + 1, 0)
    hp, hi, hf = [], [], []
    for p in range(n):
        wf = ec.window_fids(res[off[p]:off[p + 1]]) if w[p] else np.zeros(0, np.int64)
        at = np.flatnonzero(wf >= 0)
        hp += [p] * len(at)
        hi += list(at)
        hf += list(wf[at])
    return base, w, T, hp, hi, hf


@pytest.mark.parametrize("capacity", [1, 4, 6])
@pytest.mark.parametrize("name", ["across", "spans", "mixed"])
def test_model_matches_simulation(model, name, capacity):
    res, off, _ = sc.batch(name)
    n = min(len(off) - 1, 48)  # (mixed: its first 48 proteins)
    off = off[:n + 1]
    skipped, dead = model.strided_skipped(*_model_inputs(res, off, capacity))
    want = sc.brute_force_dead_steps(res, off, capacity)
    assert [int(d) for d in dead] == [d for d, _ in want]
    assert [int(s) for s in skipped] == [s for _, s in want]
    if name != "spans" or capacity > 1:
        assert sum(s for _, s in want) > 0  # the case skips something


def test_batches_are_what_they_claim(oracle_c, otable):
    def want(name):
        res, off, _ = sc.batch(name)
        return oracle_c.apply_mt(otable, res, off, ec.K, ec.MIN_HITS, 0, 4)

    _, cnt, st = want("spans")
    for i, name in enumerate(sc.batch("spans")[2]):
        if name.endswith("single-role") or name == "n2000-last-step-only":
            assert st[i] == ec.CALLED and cnt[i] >= 8, name
        else:
            assert st[i] == ec.AMBIGUOUS, name
    st = want("straddle")[2]
    assert (st == ec.CALLED).sum() >= 40 and (st != ec.AMBIGUOUS).all()
    assert list(want("across")[2]) == [ec.CALLED] * 3 + [ec.AMBIGUOUS]
    dead = sc.brute_force_dead_steps(*sc.batch("across")[:2], 4)
    assert [d for d, _ in dead] == [-1, -1, -1, 0] and dead[3][1] > 700


def test_span_lengths_cover_the_step_counts():
    assert sorted({sc.steps_of(n) for n in sc.SPAN_LENGTHS}) == [1, 2, 3, 4, 5, 12]
    assert any(n % 64 == 0 and n % 512 for n in sc.SPAN_LENGTHS)
    assert any(n % 512 == 0 for n in sc.SPAN_LENGTHS) and any(n % 64 for n in sc.SPAN_LENGTHS)
    for n in (513, 1100):  # the last slot's chunks lie wholly past the span
        assert 64 * 7 * sc.steps_of(n) >= n
    assert 64 * (7 * 12 + 5) <= 5700 < 64 * (7 * 12 + 6)  # the last slot's last six chunks do
