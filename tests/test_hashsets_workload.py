"""The inputs of tests/test_gpu_hashsets_sort.py see what they claim to see, shown on the block
model of tests/hashsets_cases.py alone (no GPU): the unmodified model gives the set reference on
every protein of every case and the set sizes of tests/test_hashsets_host.py's cases; every
compare-exchange step of every network size 2 .. 4096, skipped or inverted, changes the heads of
a protein of the network case (the size-2 step: the run it leaves); every narrowed head rule
changes the heads of a protein of the run cases; models of the value-changing kernel mutants
disagree with the reference on the cases; and a full chunk of 4,096 distinct keys, the kind of
input the device entry's first tests use, sees no skipped step at all."""
import numpy as np
import pytest

import hashsets_cases as sc
from hashindex_cases import GRID, kmers
from test_hashsets_host import cases_for, in_windows, set_size


def heads_changed(case, proteins, **hooks):
    """Whether the hooked model's heads differ (number or multiset) from the reference on any of
    the proteins, at the case's first W."""
    w = case.lds_keys[0] or sc.W_MAX
    for g in proteins:
        got = sc.block_model(case.genome[g], case.k, w, **hooks)
        if sorted(got.heads.tolist()) != sc.ref_keys(case.genome[g], case.k):
            return True
    return False


def only_step(n2, m, j, mode):
    return lambda a, b, c: mode if (a, b, c) == (n2, m, j) else None


# ---- the model itself
@pytest.mark.parametrize("case", sc.all_sets_cases(), ids=lambda c: c.name)
def test_model_heads_are_the_set_reference(case):
    """Every protein, at every W the case names: the heads are the distinct keys, each once; the
    vectorised window keys are key_of's; the runs are stored sorted; the index is sorted unique."""
    for g, s in enumerate(case.genome):
        want = sc.ref_keys(s, case.k)
        assert len(want) == len(kmers(s, case.k))
        for w in case.lds_keys:
            w = w or sc.W_MAX
            got = sc.block_model(s, case.k, w)
            assert sorted(got.heads.tolist()) == want and got.gsize == len(want), (case.name, g, w)
            assert not any(got.bad)
            assert (got.runs is None) == (sc.n_windows(s, case.k) <= w)
            if got.runs is not None:
                for c0 in range(0, len(got.runs), w):
                    assert (np.diff(got.runs[c0:c0 + w].astype(object)) >= 0).all()
    keys = sc.index_keys(case.protos, case.k)
    assert keys == sorted(set(keys)) and len(case.index) == len(keys) and max(keys) < 1 << 60
    # every protein with a window has a candidate at min_sim: an error in gsize or in the
    # matched heads moves its sim
    for g, s in enumerate(case.genome):
        assert (case.ref.best[g] >= 0) == (len(s) >= case.k), (case.name, g)


def test_model_on_the_scale_and_flag_cases():
    s = sc.scale_case()
    for i, item in enumerate(s.items):
        got = sc.block_model(item, s.k, sc.SCALE_W)
        assert sorted(got.heads.tolist()) == sc.ref_keys(item, s.k) and not any(got.bad)
        assert got.gsize == s.item_size[i]
    f = sc.flag_case()
    for g, item in enumerate(f.genome):
        for w in f.lds_keys:
            got = sc.block_model(item, f.k, w or sc.W_MAX)
            assert sorted(got.heads.tolist()) == sc.ref_keys(item, f.k) and not any(got.bad)


@pytest.mark.parametrize("w", [64, 256, 4096])
def test_model_is_faithful_on_the_host_check_cases(w):
    """The cases host/hashsets_check.cpp runs under sanitizers: the same set sizes and flags."""
    n = 0
    for w_, k, s in cases_for(w, 100 + w):
        got = sc.block_model(s, k, w_)
        assert int(any(got.bad)) == in_windows(s, k)
        if not any(got.bad):
            assert got.gsize == set_size(s, k), (w, k, len(s))
            n += 1
    assert n > 20


def test_scratch_layout_mirror():
    for n_res, n_g in ((0, 1), (1, 1), (3, 2), (4, 4), (5, 5), (1000, 7), (1 << 20, 1 << 20)):
        gmatch, gsize, runs, total = sc.scratch_layout(n_res, n_g)
        assert gmatch == 0 and gsize >= 4 * n_res and runs >= gsize + 4 * n_g
        assert total >= runs + 8 * n_res + 16 and gsize % 16 == runs % 16 == total % 16 == 0
        assert total <= 12 * n_res + 4 * n_g + 64


# ---- (a) every step of every network size
def test_network_case_is_what_it_is_named():
    c = sc.network_case()
    assert sorted(c.sizes) == list(sc.NETWORK_SIZES) and len(sc.NETWORK_SIZES) == 12
    for n2, proteins in c.sizes.items():
        counts = {sc.n_windows(c.genome[g], c.k) for g in proteins}
        assert counts == {n2, n2 - 1, n2 // 2 + 1}
        assert all(sc.padded_size(n) == n2 for n in counts if n > 1)
        if 4 < n2 < 128:
            assert len(proteins) == 3 * sc.SMALL_SEEDS
    for g in c.focused:                                   # the condition, again
        assert 2 * len(kmers(c.genome[g], c.k)) <= sc.n_windows(c.genome[g], c.k)
    outside = set(range(len(c.genome))) - set(c.focused)
    assert all(sc.n_windows(c.genome[g], c.k) == 1 for g in outside)
    tail = c.genome[c.tail]
    assert sc.n_windows(tail, c.k) == sc.W_MAX + 2 and tail[-3:] == "CAA"
    assert sum(len(sc.network_steps(n2)) for n2 in sc.NETWORK_SIZES) == 364
    assert len(sc.network_steps(4096)) == 78 and len(sc.network_steps(64)) == 21


# One step of a merge that is not the network's last, with every pair's direction inverted,
# leaves a network that still sorts: the blocks of width m come out of their merge rearranged
# (for j = m / 2 as a rotation of the sorted block), and the merges that follow sort them all the
# same. That is shown below by the 0-1 principle at n2 = 4, 8, 16 and on the case's chunks at
# every size. Only the last merge's steps (m = n2; 78 over the twelve sizes) are wrong when
# inverted. Nothing can see the others, and no test should claim to.
def harmless_inversion(n2, m, j):
    return n2 > m


def zeros_and_ones(n2):
    return (np.arange(1 << n2, dtype=np.int64)[None, :] >> np.arange(n2)[:, None]) & 1


@pytest.mark.parametrize("n2", [4, 8, 16])
def test_harmless_inversions_are_exactly_these(n2):
    """By the 0-1 principle: a network that sorts all 2^n2 inputs of zeros and ones sorts every
    input. At n2 = 4, 8 and 16 the network with one step inverted does so exactly for the steps
    of harmless_inversion. For sizes beyond what 2^n2 inputs can show, the chunks of the
    network case stand in: test_every_network_step_is_seen asserts that a harmless inversion
    leaves every chunk sorted and that every other one changes some protein's heads."""
    bits = zeros_and_ones(n2)
    for m, j in sc.network_steps(n2):
        got = sc.sort_network(bits.copy(), step=only_step(n2, m, j, "invert"))
        assert (got.sum(axis=0) == bits.sum(axis=0)).all()
        assert (np.diff(got, axis=0) >= 0).all() == harmless_inversion(n2, m, j), (n2, m, j)


@pytest.mark.parametrize("n2", sc.NETWORK_SIZES)
@pytest.mark.parametrize("mode", ["skip", "invert"])
def test_every_network_step_is_seen(n2, mode):
    """Each (m, j) step of the size-n2 network, skipped or with every pair's direction inverted,
    changes the heads of a protein of that size. n2 = 2 is one exchange of two keys, whose heads
    are the same in either order: it is seen in the run it leaves, by the 4,098-window protein.
    An inversion of harmless_inversion is no wrong network: it must leave every chunk sorted."""
    c = sc.network_case()
    for m, j in sc.network_steps(n2):
        hook = only_step(n2, m, j, mode)
        if n2 == 2:
            s = c.genome[c.tail]
            got = sc.block_model(s, c.k, sc.W_MAX, step=hook)
            assert not heads_changed(c, c.sizes[2], step=hook)
            assert got.runs[-2] > got.runs[-1] and sc.block_model(s, c.k).runs[-2] < got.runs[-2]
        elif mode == "invert" and harmless_inversion(n2, m, j):
            assert not heads_changed(c, c.sizes[n2], step=hook)
            for g in c.sizes[n2]:
                got = sc.block_model(c.genome[g], c.k, step=hook).heads
                assert (np.diff(got.astype(object)) > 0).all()
        else:
            assert heads_changed(c, c.sizes[n2], step=hook), (n2, m, j, mode)


def test_all_distinct_keys_see_no_step():
    """The negative control: one full chunk of 4,096 windows at K = 8 over 20 letters, all keys
    distinct, as the device entry's first tests have them. No skipped step of the 78 changes its
    heads - an unsorted chunk of distinct keys has the heads of a sorted one. This is why the
    duplicate-heavy cases exist."""
    rng = np.random.default_rng(8)
    s = sc.draw(rng, sc.LETTERS, 4096 + 7)
    assert len(kmers(s, 8)) == 4096
    want = sc.ref_keys(s, 8)
    steps = sc.network_steps(4096)
    assert len(steps) == 78
    for m, j in steps:
        got = sc.block_model(s, 8, step=only_step(4096, m, j, "skip"))
        assert sorted(got.heads.tolist()) == want
    none = sc.block_model(s, 8, step=lambda *a: "skip")   # no network at all
    assert sorted(none.heads.tolist()) == want


# ---- (b), (c), (d) the head rule across runs
RUN_RULES = {"previous run only": dict(searched=lambda c: range(max(c - 1, 0), c)),
             "first two runs only": dict(searched=lambda c: range(min(c, 2))),
             "w - 1 keys per run": None}


def rule_hooks(rule, w):
    return dict(run_keys=w - 1) if RUN_RULES[rule] is None else RUN_RULES[rule]


def runs_groups():
    """(name, case, proteins, w): the proteins built for each W, the default W, each K."""
    out = []
    e = sc.every_w_case()
    for w in sc.EVERY_W:
        out.append((f"W = {w}", e, [g for g, (w_, _) in enumerate(e.runs_of) if w_ == w], w))
    d = sc.default_w_case()
    out.append(("default W", d, list(range(len(d.genome))), sc.W_MAX))
    for k in sc.EVERY_K:
        c = sc.every_k_case(k)
        out.append((c.name, c, [g for g, r in enumerate(c.runs_of) if r is not None], 64))
    return out


@pytest.mark.parametrize("rule", sorted(RUN_RULES))
@pytest.mark.parametrize("group", runs_groups(), ids=lambda g: g[0])
def test_every_narrowed_head_rule_is_seen(group, rule):
    name, case, proteins, w = group
    hooks = rule_hooks(rule, w)
    changed = [g for g in proteins
               if not sc.block_model(case.genome[g], case.k, w, **hooks).same_heads(
                   sc.block_model(case.genome[g], case.k, w))]
    assert changed, (name, rule)


def test_run_cases_are_what_they_are_named():
    for name, case, proteins, w in runs_groups():
        counts = sorted(sc.n_windows(case.genome[g], case.k) for g in proteins)
        assert counts == ([2 * w + 41, 3 * w + 17] if w == sc.W_MAX else [2 * w, 3 * w + 17])
        for g in proteins:
            s, (w_, marks) = case.genome[g], case.runs_of[g]
            assert w_ == w
            sc.assert_run_properties(s, case.k, w, marks)
            assert 2 * len(kmers(s, case.k)) <= sc.n_windows(s, case.k)
            if sc.n_windows(s, case.k) == 3 * w + 17:
                assert set(marks) == {"X", "V", "Y"}
    for k in sc.EVERY_K:
        keys = [sc.key_of(x) for s in sc.every_k_case(k).genome for x in kmers(s, k)]
        assert max(keys) < 1 << 5 * k
        if k >= 7:                       # pairs that differ in one word alone, and in both
            arr = np.array(sorted(set(keys)), np.uint64)
            hi, lo = arr >> np.uint64(32), arr & np.uint64(0xFFFFFFFF)
            same_hi = (hi[1:] == hi[:-1]).any()
            same_lo = len(set(lo.tolist())) < len(lo)
            both = len(set(hi.tolist())) > 1 and len(set(lo.tolist())) > 1
            assert same_hi and same_lo and both, k
        if k == 12:
            assert max(keys) >> 59 == 1 and sc.key_of("*" * 12) in keys


# ---- (e) a block's second protein
def test_scale_case_pairs():
    s = sc.scale_case()
    assert sc.SCALE_N == GRID + 517 and len(s.idx) == sc.SCALE_N and len(s.go) == sc.SCALE_N + 1
    assert max(sc.SCALE_BLOCKS) == 516 and len(set(sc.SCALE_BLOCKS)) == len(sc.SCALE_BLOCKS)
    seen = set()
    for g, pair in s.pairs:
        assert (s.protein(g), s.protein(g + GRID)) == (s.crafted[pair[0]], s.crafted[pair[1]])
        seen.add(pair)
    assert seen == set(sc.SCALE_PAIRS)
    k, w = s.k, sc.SCALE_W
    three = s.crafted["three_run"]
    assert sc.n_windows(three, k) == 3 * w + 17 and len(s.crafted["k_minus_1"]) == k - 1
    assert 0 < sc.n_windows(s.crafted["short"], k) <= w and s.crafted["empty"] == ""
    lens = np.diff(s.go.astype(np.int64))
    pool = s.idx < sc.SCALE_POOL
    assert lens[pool].max() <= 40 and 0.03 < (lens == 0).mean() < 0.07
    assert 0.03 < (lens == k - 1).mean() < 0.07
    sample = np.random.default_rng(1).integers(0, sc.SCALE_N, 2000).tolist()
    sample += [0, GRID - 1, GRID, sc.SCALE_N - 1]
    assert all(s.protein(g) == s.items[s.idx[g]] for g in sample)
    checked = s.checked()
    assert set(range(GRID, sc.SCALE_N)) <= set(checked.tolist()) and len(checked) > 2900
    best = s.ref.best
    assert best[s.item_of["three_run"]] == 6 and best[s.item_of["heavy_a"]] == 7
    assert best[s.item_of["empty"]] == best[s.item_of["k_minus_1"]] == -1


def test_model_heads_counter_carried_into_a_blocks_second_protein():
    """s_heads zeroed once per block: the second protein's gsize is its own plus the first's.
    Wrong for every second protein whose first has a window."""
    s = sc.scale_case()
    size = s.item_size[s.idx].astype(np.int64)
    second = np.arange(GRID, sc.SCALE_N)
    wrong = np.flatnonzero(size[second - GRID] > 0)
    print(f"{len(wrong)} of 517 second proteins get a wrong gsize")
    assert len(wrong) > 400
    by_pair = {pair: size[g] for g, pair in s.pairs}
    for pair in sc.SCALE_PAIRS:
        assert (by_pair[pair] > 0) == (pair[0] not in ("empty", "k_minus_1"))


# ---- (f) the alphabet flag
def test_flag_case_positions():
    f = sc.flag_case()
    k, w = f.k, sc.FLAG_W
    lo, hi = f.long_at
    assert hi - lo == 3 * w + 17 + k - 1
    names = [v[0] for v in f.variants]
    assert len(names) == 3 + (k - 1) + 2
    for name, res, first, last, flagged in f.variants:
        at = np.flatnonzero(res != f.g)
        assert len(at) == 1 and res[at[0]] == sc.FLAG_BYTE
        at = int(at[0])
        protein = res[lo:hi].tobytes()
        bad = sc.block_model(protein, k, w).bad
        assert any(bad) == flagged == (lo <= at < hi), name
        if name == "first byte":
            assert at == lo and bad == [True, False, False, False]
        if name == "last byte":
            # the last code the tail of the last chunk's loop reads, and no other chunk
            assert at == hi - 1 and bad == [False, False, False, True]
        if name.startswith("shared"):
            assert bad == [True, True, False, False]
        if name == "chunk 2":
            assert bad == [False, False, True, False]
        if not flagged:
            assert at in (int(f.go[first]) - 1, int(f.go[last])) and 0 < first and last < 5
    # `bad` reset at every chunk: only a protein's last chunk could set the flag - the first
    # byte, the shared bytes and chunk 2 would go unseen
    unseen = [v[0] for v in f.variants
              if v[4] and not sc.block_model(v[1][lo:hi].tobytes(), k, w).bad[-1]]
    assert len(unseen) == 2 + (k - 1)


# ---- models of the kernel mutants the GPU file must fail on
MUTANT_STEPS = {"stride 1 never applied": lambda n2, m, j: "skip" if j == 1 else None,
                "stride 128 dropped": lambda n2, m, j: "skip" if j == 128 else None,
                "direction from low & (m << 1)": lambda n2, m, j: "m2"}


@pytest.mark.parametrize("mutant", sorted(MUTANT_STEPS))
def test_model_of_the_network_mutants(mutant):
    c = sc.network_case()
    hook = MUTANT_STEPS[mutant]
    wrong = [n2 for n2 in sc.NETWORK_SIZES if heads_changed(c, c.sizes[n2], step=hook)]
    print(f"{mutant}: sizes with a changed protein {wrong}")
    if mutant == "stride 128 dropped":
        assert wrong == [256, 512, 1024, 2048, 4096]
    else:
        assert wrong == list(sc.NETWORK_SIZES[1:])
    # the barrier path taking stride 64 as well leaves every value where it was: nothing to model
