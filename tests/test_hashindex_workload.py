"""The inputs of tests/test_gpu_hashindex_load.py meet the conditions its GPU tests rely on, shown
on the set model and on the host check program alone (no GPU): the Python mirror of the slot hash
and the table size equals the header's, every protein of the bounds case has exactly its planted
candidate count and splits exactly above CAP, the cluster's holders start in the table's last
slots and form one chain of more than 256 slots that passes from slot T - 1 to slot 0 (by the
mirror, and by the serial block model of host/hashindex_check.cpp under sanitizers, which also
agrees with brute force on the case), the scale case's crafted pairs are what they are named,
and models of the broken kernels the cases aim at disagree with the reference where they should."""
import re
import subprocess

import numpy as np
import pytest

import hashindex_cases as hc
from hashindex_cases import GRID, K
from test_hashindex_host import EXE, check_program, run_check  # noqa: F401 (a fixture)


def caps_of(option):
    return option or hc.CAP_DEFAULT


# ---- the mirror
@pytest.mark.parametrize("cap", [1, 4, 256, 511, 512, 513, 1024, 1536, 1537, 2048])
def test_python_mirror_equals_the_header(check_program, cap):
    rng = np.random.default_rng(cap)
    ids = [0, 1, 2, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1] + rng.integers(0, 2 ** 32, 200).tolist()
    if cap in hc.CLUSTER:
        ids += hc.cluster_ids(cap)[::7]
    r = subprocess.run([EXE, "--hash", str(cap)] + [str(i) for i in ids], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    bits = hc.hash_bits(cap)
    assert lines[0] == f"slots {hc.hash_table_slots(cap)} bits {bits}"
    assert lines[1:-1] == [f"{i} {hc.hash_slot(i, bits)}" for i in ids]
    assert hc.hash_slots_of(ids, bits).tolist() == [hc.hash_slot(i, bits) for i in ids]
    # at most half full at CAP, and room for a block's inserts in flight
    assert hc.hash_table_slots(cap) >= max(2 * cap, cap + 2 * hc.BLOCK)


def test_hash_mode_refuses_a_bad_cap(check_program):
    for cap in ("0", "2049"):
        assert subprocess.run([EXE, "--hash", cap, "1"], capture_output=True).returncode == 2


def test_table_sizes_of_the_caps_in_use():
    assert [hc.hash_table_slots(c) for c in (128, 256, 512, 1024, 2048)] == \
        [1024, 1024, 1024, 2048, 4096]
    assert hc.hash_table_slots(hc.CAP_MAX) * 8 == 32 * 1024     # the largest dynamic LDS


# ---- (a)
def test_bounds_case_has_exactly_its_candidate_counts():
    a = hc.bounds_case()
    cand = [len(c) for c in a.ref.cand]
    assert cand == list(hc.BOUND_N) + [1, 0, 0]
    assert len(a.protos) == hc.BOUND_PROTOS and len(set(a.ids)) == hc.BOUND_HOLDERS
    for j, n in enumerate(hc.BOUND_N):                       # nested: the first n holders
        assert a.ref.cand[j] == sorted(a.ids[:n])
    for cap in (512, 1024, 2048):                            # both sides of every CAP
        assert {cap - 1, cap, cap + 1} <= set(hc.BOUND_N)
    for option in hc.BOUND_CAPS:
        cap = caps_of(option)
        st = a.stats(option)
        assert st[0] == 11 and st[1] == sum(n > cap for n in hc.BOUND_N)
        assert st[2] >= sum(-(-n // cap) for n in cand)
    assert [a.stats(o)[1] for o in hc.BOUND_CAPS] == [8, 5, 2]
    # at CAP 512 more ranges than an even spread of the holders would need: halves of a range
    # hold unequal numbers of them, and some split again while their siblings do not
    assert a.stats(512)[2] > sum(-(-n // 512) for n in cand)


def test_bounds_case_similarities_ties_and_the_long_copy():
    a = hc.bounds_case()
    ref = a.ref
    for j in range(len(hc.BOUND_N)):                         # about half pass, none all-or-nothing
        assert 0.4 < len(ref.passed[j]) / len(ref.cand[j]) < 0.6, j
    held = ref.count[a.ids]
    assert (held == 0).any() and (held > 0).any() and len(set(held.tolist())) > 5
    sizes = {len(hc.kmers(a.protos[p])) for p in a.ids}
    assert len(sizes) > 200                                  # psize differs
    motif_kmers = [len(hc.kmers(a.genome[j]) & hc.kmers(a.protos[a.ids[0]])) for j in range(10)]
    assert len(set(motif_kmers)) >= 8                        # shared counts differ by protein
    shared0 = {len(hc.kmers(a.genome[9]) & hc.kmers(a.protos[p])) for p in a.ids[:500]}
    assert len(shared0) >= 5                                 # ... and by holder
    # the tie on the best of protein 9, which splits at every CAP: two equal prototypes in
    # different halves of the id range, the earlier one wins
    lo, hi = sorted(a.ids[i] for i in a.champs)
    assert a.protos[lo] == a.protos[hi] and lo < hc.BOUND_PROTOS // 2 <= hi
    assert ref.best[9] == lo and len(ref.cand[9]) > hc.CAP_MAX
    assert hi in ref.passed[9] and ref.count[lo] == ref.count[hi] == 1
    # three equal holders far apart, among the candidates of every protein
    trio = [a.ids[i] for i in (3, 77, 400)]
    assert len({a.protos[p] for p in trio}) == 1 and max(trio) - min(trio) > 2000
    assert all(set(trio) <= set(ref.cand[j]) for j in range(10))
    assert len(set(ref.count[trio].tolist())) == 1
    # the copy: 4,993 postings of one prototype, all into one slot
    assert ref.cand[10] == [a.long_id] and ref.sim[10] == 1.0 and ref.best[10] == a.long_id
    assert len(hc.kmers(a.genome[10])) == 5000 - K + 1
    assert ref.best[11] == ref.best[12] == -1
    assert max(len(s) for s in a.genome[:10]) > 8 * hc.BLOCK  # several chunks of 256 keys


# ---- (b)
@pytest.mark.parametrize("cap", sorted(hc.CLUSTER))
def test_cluster_holders_form_one_chain_across_the_table_end(cap):
    c = hc.cluster_case(cap)
    last, count, sizes = hc.CLUSTER[cap]
    bits, T = hc.hash_bits(cap), hc.hash_table_slots(cap)
    assert len(c.hold) == count > cap and sizes[0] == count
    assert all(hc.hash_slot(p, bits) >= T - last for p in c.hold)
    held = set(c.hold)
    assert all(len(s) < K for p, s in enumerate(c.protos) if p not in held)
    assert sum(len(s) > 0 for s in c.protos) > count + 100   # some fillers are not empty
    assert [len(x) for x in c.ref.cand] == list(sizes) + [count, 0, 0]
    assert sizes[1] == cap + 1 and sizes[2] == cap and all(2 * n >= cap for n in sizes)
    for q, n in enumerate(sizes):
        _, chain, wraps = hc.occupied_slots(c.ref.cand[q], cap)
        assert chain == n and wraps, (q, chain)              # one chain, through slot T - 1 to 0
    assert sum(n > 256 for n in sizes) >= (5 if cap > 256 else 2)
    st = c.stats(cap)
    assert st[:2] == [6, 3] and st[2] == sum(hc.ranges_scored(x, len(c.protos), cap)
                                             for x in c.ref.cand)
    for q in (2, 3, 4):                                      # at or below CAP: one range
        assert hc.ranges_scored(c.ref.cand[q], len(c.protos), cap) == 1
    for q in range(6):                                       # about half pass
        assert 0.4 < len(c.ref.passed[q]) / len(c.ref.cand[q]) < 0.6
    twin = c.hold[sizes[3] - 1]
    assert c.protos[twin] == c.protos[c.hold[0]] and twin - c.hold[0] > len(c.protos) // 20


@pytest.mark.parametrize("cap", sorted(hc.CLUSTER))
def test_cluster_through_the_block_model_under_sanitizers(check_program, tmp_path, cap):
    """The serial block model equals brute force and the set model on the cluster case; its
    longest probe is longer than 256 slots and a probe passed from slot T - 1 to slot 0."""
    c = hc.cluster_case(cap)
    path = tmp_path / "cluster.bin"
    hc.write_check_case(path, c, cap)
    r = run_check(path)
    assert r.returncode == 0, r.stdout + r.stderr
    st = c.stats(cap)
    m = re.search(r"hashindex_check ok: (\d+) prototypes, (\d+) proteins, (\d+) split, "
                  r"(\d+) ranges, longest probe (\d+), wrapped (\d)\n", r.stdout)
    assert m, r.stdout
    n_proto, n_genome, split, ranges, longest, wrapped = map(int, m.groups())
    assert (n_proto, n_genome, split, ranges) == (len(c.protos), len(c.genome), st[1], st[2])
    assert longest > 256 and wrapped == 1
    assert longest <= hc.hash_table_slots(cap)


def test_block_model_reports_short_probes_on_a_light_table(check_program, tmp_path):
    """The two new fields are measured, not constants: a dozen scattered candidates give a probe
    of a few slots and no wrap."""
    rng = np.random.default_rng(9)
    motif = hc.rand(rng, 12)
    protos = [motif + hc.rand(rng, 20) if p % 5 == 0 else hc.rand(rng, 30) for p in range(60)]
    case = hc.Case([motif + hc.rand(rng, 40)], protos, 0.0125)
    assert len(case.ref.cand[0]) == 12
    hc.write_check_case(tmp_path / "light.bin", case, 1024)
    r = run_check(tmp_path / "light.bin")
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"longest probe (\d+), wrapped (\d)\n", r.stdout)
    assert m and 1 <= int(m.group(1)) <= 3 and m.group(2) == "0"


# ---- (c)
def test_scale_case_is_what_it_is_named():
    s = hc.scale_case()
    assert hc.SCALE_N == GRID + 517 and hc.SCALE_SIZES == (GRID, GRID + 1, GRID + 517)
    assert len(s.idx) == hc.SCALE_N and len(s.go) == hc.SCALE_N + 1
    lens = np.diff(s.go.astype(np.int64))
    tiny = s.idx < hc.SCALE_POOL
    assert (~tiny).sum() == sum(x is not None for g in range(len(hc.SCALE_BLOCKS))
                                for x in hc.SCALE_PAIRS[g % len(hc.SCALE_PAIRS)])
    assert 0.09 < (lens < K).mean() < 0.11 and (lens == 0).mean() > 0.04
    assert set(lens[tiny & (lens >= K)].tolist()) == {8, 9, 10}          # 1 to 3 windows
    # the residues are the items' (a sample, the crafted ones and both ends)
    sample = np.random.default_rng(1).integers(0, hc.SCALE_N, 3000).tolist()
    sample += np.flatnonzero(~tiny).tolist() + [0, GRID - 1, GRID, hc.SCALE_N - 1]
    assert all(s.protein(g) == s.items[s.idx[g]] for g in sample)
    res, off = s.genome(GRID + 1)
    assert len(off) == GRID + 2 and len(res) == int(off[-1]) + 32 and off[0] == 0
    # prototypes: the hub K-mer in a dozen, the miss strings in none
    hub = s.protos[0][20:]
    assert len(hub) == K and sum(hub in p for p in s.protos) == 12
    cands = np.array([len(c) for c in s.ref.cand])
    pool = cands[:hc.SCALE_POOL]
    assert (pool == 0).mean() > 0.25 and (pool == 12).sum() > 300 and (pool[pool > 0] < 12).any()
    assert 0.25 < (s.ref.best[:hc.SCALE_POOL] >= 0).mean() < 0.6          # min_sim cuts the pool
    with_cand = (pool > 0) & (s.ref.best[:hc.SCALE_POOL] < 0)
    assert with_cand.sum() > 300                              # candidates, none at min_sim
    # the crafted proteins
    it = s.item_of
    low = hc.SCALE_LOW_CAP
    assert cands[it["strong_many"]] == 302 > low and s.ref.best[it["strong_many"]] == s.s1_id
    assert s.protos[-1] == s.protos[s.s1_id] and len(s.protos) - 1 in s.ref.passed[it["strong_many"]]
    assert s.ref.sim[it["strong_many"]] > 0.7
    assert cands[it["second_best"]] == 101 <= low and s.ref.best[it["second_best"]] == s.s2_id
    assert cands[it["crowd"]] == 300 and cands[it["few"]] == 100 and cands[it["none"]] == 0
    assert s.ref.best[it["crowd"]] != s.ref.best[it["few"]] and s.ref.best[it["none"]] == -1
    # every kind of pair sits in some block, and block 0 is (strong best and many, none)
    kinds = set()
    for g in hc.SCALE_BLOCKS:
        a, b = s.items[s.idx[g]], s.items[s.idx[g + GRID]]
        kinds.add((cands[s.idx[g]] > low, cands[s.idx[g + GRID]] > low,
                   cands[s.idx[g]] > 0, cands[s.idx[g + GRID]] > 0))
        assert len(a) > 100 or len(b) > 100 or s.idx[g] >= hc.SCALE_POOL
    assert {(True, False, True, False), (False, True, False, True), (True, False, True, True),
            (False, True, True, True)} <= kinds
    assert s.idx[0] == it["strong_many"] and s.idx[GRID] == it["none"]
    assert max(hc.SCALE_BLOCKS) == 516 and len(hc.SCALE_BLOCKS) >= 36


@pytest.mark.parametrize("n", hc.SCALE_SIZES)
def test_scale_expectations_follow_from_the_items(n):
    s = hc.scale_case()
    best, sim, count, st = s.expected(n, hc.SCALE_LOW_CAP)
    assert len(best) == len(sim) == n and count.sum() == sum(len(s.ref.passed[i]) for i in s.idx[:n])
    st0 = s.expected(n)[3]
    assert st[0] == st0[0] == sum(len(s.ref.cand[i]) > 0 for i in s.idx[:n])
    assert st0[1] == 0 and st0[2] == st0[0] and st[2] > st[0] and st[1] > 0
    # a direct run of the set model on a slice around the grid size
    lo, hi = GRID - 40, min(n, GRID + 40)
    direct = hc.set_model([s.protein(g) for g in range(lo, hi)], s.protos, K, s.min_sim)
    assert (direct.best == best[lo:hi]).all() and (direct.sim == sim[lo:hi]).all()


# ---- (d)
def test_threshold_pair_and_disjoint_keys():
    genome, protos = hc.threshold_case()
    ref = hc.set_model(genome, protos, K, hc.THRESHOLD)
    assert len(hc.kmers(genome[0])) == 41 and len(hc.kmers(protos[0])) == 40
    assert len(hc.kmers(genome[0]) & hc.kmers(protos[0])) == 1
    assert ref.sim[0] == 0.0125 == 1 / 80 and ref.best[0] == 0 and ref.count[0] == 1
    above = hc.set_model(genome, protos, K, float(np.nextafter(hc.THRESHOLD, 1)))
    assert above.best[0] == -1 and above.count[0] == 0 and above.cand[0] == [0]
    for index_above in (True, False):
        genome, protos = hc.disjoint_keys_case(index_above)
        gk = [hc.kmer_key(k) for s in genome for k in hc.kmers(s)]
        pk = [hc.kmer_key(k) for s in protos for k in hc.kmers(s)]
        assert (max(gk) < min(pk)) if index_above else (min(gk) > max(pk))


# ---- models of the broken kernels the cases aim at
def _better(sa, ia, sb, ib):
    """hash_better over (similarity, prototype); -1 is none."""
    return ia >= 0 and (ib < 0 or sa > sb or (sa == sb and ia < ib))


@pytest.mark.parametrize("n", hc.SCALE_SIZES)
def test_model_best_carried_into_a_blocks_second_protein(n):
    """best_bits / best_id initialised once per block: the second protein of a block starts from
    the first one's best. Wrong for more than 2^20 proteins, right at 2^20."""
    s = hc.scale_case()
    best, sim = s.expected(n)[:2]
    wrong = [g for g in range(GRID, n) if _better(sim[g - GRID], best[g - GRID], sim[g], best[g])]
    print(f"n = {n}: {len(wrong)} of {max(n - GRID, 0)} second proteins take the first one's best")
    assert (len(wrong) > 0) == (n > GRID)
    if n == hc.SCALE_N:
        assert len(wrong) > 100 and GRID in wrong


@pytest.mark.parametrize("n", hc.SCALE_SIZES)
def test_model_split_and_ranges_carried_into_a_blocks_second_protein(n):
    """split / ranges initialised once per block (`has` is assigned at every protein's first
    range): the second protein reports the first one's split flag and adds its ranges again."""
    s = hc.scale_case()
    for cap in (hc.CAP_DEFAULT, hc.SCALE_LOW_CAP):
        split = np.array([len(c) > cap for c in s.ref.cand])[s.idx[:n]]
        ranges = np.array([hc.ranges_scored(c, len(s.protos), cap) for c in s.ref.cand])[s.idx[:n]]
        second = np.arange(GRID, n)
        more_split = int((split[second - GRID] & ~split[second]).sum())
        more_ranges = int(ranges[second - GRID].sum())
        print(f"n = {n}, CAP {cap}: +{more_split} split, +{more_ranges} ranges")
        assert (more_ranges > 0) == (n > GRID)
        assert (more_split > 0) == (n > GRID and cap == hc.SCALE_LOW_CAP)   # block 0 at 2^20 + 1


def test_model_claims_refused_at_cap_instead_of_above_it():
    """table_add refusing a new prototype at distinct >= CAP while the split test stays
    distinct > CAP: without a race the table never passes CAP, nothing splits, and every
    protein of more than CAP candidates loses some (at CAP + 1 exactly one). The bounds case has
    such a protein at every CAP in use, the cluster case three; no shape at CAP + 1 existed."""
    a = hc.bounds_case()
    for option in hc.BOUND_CAPS:
        cap = caps_of(option)
        lost = [n - cap for n in hc.BOUND_N if n > cap]
        assert 1 in lost and a.stats(option)[1] == len(lost) > 0
    for cap in hc.CLUSTER:
        assert sum(len(x) == cap + 1 for x in hc.cluster_case(cap).ref.cand) == 1


def probes_over(ids, cap, limit):
    """How many of the ids, inserted in ascending order, need more than `limit` probe steps."""
    bits = hc.hash_bits(cap)
    T = 1 << bits
    taken, over = np.zeros(T, bool), 0
    for p in ids:
        h, steps = hc.hash_slot(p, bits), 1
        while taken[h]:
            h, steps = (h + 1) & (T - 1), steps + 1
        taken[h] = True
        over += steps > limit
    return over


def test_model_probe_cut_to_16_steps():
    """A probe that gives up after 16 slots and drops the posting: the cluster loses nearly all
    of its holders at every CAP. The bounds case's scattered ids, inserted in ascending order, lose
    none even in a half-full table (printed): only a cluster aims at the probe's length."""
    for cap in hc.CLUSTER:
        c = hc.cluster_case(cap)
        for q in (2, 3, 4):                                  # the proteins that do not split
            over = probes_over(c.ref.cand[q], cap, 16)
            print(f"cluster CAP {cap}, protein {q}: {over} of {len(c.ref.cand[q])} dropped")
            assert over > len(c.ref.cand[q]) - 40
    a = hc.bounds_case()
    for option in hc.BOUND_CAPS:
        cap = caps_of(option)
        over = [probes_over(a.ref.cand[j], cap, 16) for j, n in enumerate(hc.BOUND_N) if n <= cap]
        print(f"bounds CAP {cap}: dropped per unsplit protein {over}")
