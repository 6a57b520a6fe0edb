"""The inputs of tests/test_gpu_seqcheck_scale.py meet the conditions its GPU tests rely on, shown
on the references alone (no GPU): the id-to-sequence map is injective, the sizes stand on the
intended sides of rocPRIM's limits and of the MD5 grid cap, the crafted digests hold the pairs
they are there for, every planted group has its planted size and mixedness, the dict and the
numpy reference agree, and a numpy model of each broken grouping disagrees with the reference
where it should."""
import hashlib

import numpy as np
import pytest

import seqcheck_cases as sc
from seqcheck_cases import NO_FUN, UPPER


def same(a, b):
    return all((x == y).all() for x, y in zip(a[:3], b[:3])) and list(a[3]) == list(b[3])


def test_id_map_is_injective():
    """Different ids give different bytes (same length: different digits; else another length),
    equal ids equal bytes, and build_batch writes id_bytes."""
    rng = np.random.default_rng(1)
    ids = np.unique(np.concatenate([np.arange(5000), [sc.BIG_ID, sc.TAIL_ID, 20 ** 7 - 1],
                                    rng.integers(0, 20 ** 7, 5000)]))
    res, off = sc.build_batch(ids)
    seqs = [res[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(ids))]
    assert len(set(seqs)) == len(ids)
    assert all(s == sc.id_bytes(int(g)) for s, g in zip(seqs[::37], ids[::37]))
    lens = np.diff(off.astype(np.int64))
    assert lens.min() == 9 and lens.max() == 70 and set(lens) == set(range(9, 71))
    assert len(sc.id_bytes(sc.BIG_ID)) == 70 and len(sc.id_bytes(sc.TAIL_ID)) == 56
    assert set(b"".join(seqs)) <= set(sc.AA.tobytes())
    # vectorised: on the whole range of one digit position the digits are a bijection, and the
    # length is a function of the id
    g = np.arange(0, 3_000_000)
    digits = np.stack([g // 20 ** d % 20 for d in range(sc.ID_DIGITS)])
    assert ((digits * (20 ** np.arange(sc.ID_DIGITS))[:, None]).sum(axis=0) == g).all()


def test_sizes_stand_where_they_are_aimed():
    assert sc.SCALE_SIZES[0] == sc.MERGE_SORT_LIMIT == 1 << 20       # the last merge-sort size
    assert sc.SCALE_SIZES[1] == sc.MERGE_SORT_LIMIT + 1              # the first onesweep size
    assert sc.SCALE_SIZES[2] == 2_500_000
    assert all(n > sc.MD5_GRID_CAP == 131_072 for n in sc.SCALE_SIZES)
    assert sc.SINGLE_SORT_LIMIT == 256 * 4
    assert {sc.SINGLE_SORT_LIMIT, sc.SINGLE_SORT_LIMIT + 1} <= set(sc.COUNT_EDGES)
    for edge in (64, 256, 1024, 4096, 65_536):                      # wave, block, scan blocks
        assert {edge - 1, edge, edge + 1} <= set(sc.COUNT_EDGES)
    assert {1, 2} <= set(sc.COUNT_EDGES)
    for r in (sc.same_half("low"), sc.same_half("high")):
        assert len(r.digest) == 300_000 and sc.SINGLE_SORT_LIMIT < 300_000 < sc.MERGE_SORT_LIMIT
        assert len(r.digest) > (1 << 17) + 70_000                    # merge path, not odd-even
    assert len(sc.stability().digest) == 200_000
    assert len(sc.upper_case().g) == 200_000 > sc.MD5_GRID_CAP


def test_lattice_holds_pairs_equal_in_one_half():
    r = sc.lattice()
    low, high = sc.halves_of(r.digest[r.lengths != 0])
    pairs = set(zip(low.tolist(), high.tolist()))
    assert len(pairs) == 81 and set(low.tolist()) == set(high.tolist()) == set(sc.LATTICE_HALVES)
    for a in sc.LATTICE_HALVES:
        assert len({h for l, h in pairs if l == a}) == 9     # equal low, nine different highs
        assert len({l for l, h in pairs if h == a}) == 9     # equal high, nine different lows
    sizes = {(int(l), int(h)): int(s) for l, h, s in zip(low, high, r.size[r.lengths != 0])}
    assert set(sizes.values()) == {1, 2, 3, 5} and sizes[(0, 0)] == 3
    multi = r.size > 1
    assert r.mixed[multi].any() and not r.mixed[multi].all() and not r.mixed[~multi].any()
    assert (r.lengths == 0).sum() == 5 and (r.rep[r.lengths == 0] == -1).all()
    assert r.stats[0] == 81
    # 0 and NO_FUN, the accumulators' initial values, inside groups of several members
    for f in (0, NO_FUN):
        assert ((r.fun == f) & multi & (r.mixed == 0)).any()
        assert ((r.fun == f) & (r.mixed == 1)).any()
    # the words of the 32-bit model: halves that agree in their low word and differ above it
    z = {h & 0xFFFFFFFF for h in sc.LATTICE_HALVES}
    assert len(z) < len(sc.LATTICE_HALVES)


def test_neighbours_swaps_and_stability_shapes():
    r = sc.neighbours()
    assert r.stats[:2] == [129, 129] and (r.size == 2).all() and 0 < r.stats[2] < 129
    vals = sorted({int.from_bytes(bytes(d), "little") for d in r.digest})
    base = [v for v in vals if sum(bin(v ^ u).count("1") == 1 for u in vals) == 128]
    assert len(vals) == 129 and len(base) == 1
    assert {base[0] ^ v for v in vals} == {0} | {1 << b for b in range(128)}
    r = sc.swaps()
    words = np.sort(r.digest.view("<u4").reshape(-1, 4), axis=1)
    assert (words == words[0]).all() and len(set(words[0].tolist())) == 4
    assert r.stats[:2] == [24, 24] and (r.size == 2).all() and 0 < r.stats[2] < 24
    r = sc.stability()
    assert (r.rep[0::2] == 0).all() and (r.size[0::2] == 100_000).all() and r.mixed[0::2].all()
    assert (r.rep[1::2] == np.arange(1, 200_000, 2)).all() and (r.size[1::2] == 1).all()
    assert r.stats == [100_001, 1, 1] and (r.fun[:-2] == 6).all()
    for which in ("low", "high"):
        r = sc.same_half(which)
        low, high = sc.halves_of(r.digest)
        few, many = (low, high) if which == "low" else (high, low)
        assert len(np.unique(few)) == 7 and 49_000 < len(np.unique(many)) <= 50_000
        # 300,000 draws from 350,000 pairs: about 350,000 (1 - e^(-6/7)) = 201,000 groups
        assert 190_000 < r.stats[0] < 210_000 and r.stats[1] > 50_000
        assert 0 < r.stats[2] < r.stats[1]


@pytest.mark.parametrize("n,empties", [(sc.SCALE_SIZES[0], False), (sc.SCALE_SIZES[1], False),
                                       (sc.SCALE_SIZES[2], True)])
def test_scale_case_has_its_planted_groups(n, empties):
    c = sc.scale_case(n, empties)
    assert len(c.g) == n and c.offsets[0] == 0 and len(c.residues) == int(c.offsets[-1]) + 32
    live = np.ones(n, bool) if c.empty is None else ~c.empty
    # the big group: about n / 3 members from the batch's first non-empty index to its end,
    # mixed by its last member alone
    big = c.big
    assert big[0] == (1 if empties else 0) and (c.g[big] == sc.BIG_ID).all()
    assert abs(len(big) - n / 3) < (0.04 * n if empties else 1)
    assert big[-1] > 0.9 * (n - sc.TAIL_MEMBERS) and (np.diff(big) < n // 1000).all()
    assert (c.rep[big] == big[0]).all() and (c.size[big] == len(big)).all() and c.mixed[big].all()
    assert (c.fun[big[:-1]] == 77).all() and c.fun[big[-1]] == 78
    # the tail group: adjacent at the end, one function id, NO_FUN
    tail = np.arange(c.tail0, n)[live[c.tail0:]]
    assert len(tail) == (sc.TAIL_MEMBERS if not empties else live[c.tail0:].sum()) > 60_000
    assert (c.g[c.tail0:] == sc.TAIL_ID).all() and (c.fun[c.tail0:] == NO_FUN).all()
    assert (c.rep[tail] == tail[0]).all() and (c.size[tail] == len(tail)).all()
    assert not c.mixed[tail].any()
    # the small groups
    assert len(c.small_sizes) == n // 10 and set(c.small_sizes.tolist()) == {2, 3, 4, 5}
    m, grp = c.small_members, c.small_group
    if not empties:
        assert (c.size[m] == c.small_sizes[grp]).all()
        assert (c.mixed[m] == grp % 2).all()                 # every other one mixed
    else:
        assert (c.size[m][live[m]] <= c.small_sizes[grp][live[m]]).all()
        assert 0.3 < c.mixed[m].mean() < 0.5
    for kind, ids in ((0, {0}), (2, {NO_FUN}), (1, {0, NO_FUN})):
        sel = m[grp % 8 == kind]
        assert set(c.fun[sel].tolist()) == ids and (c.mixed[sel][live[sel]] <= kind % 2).all()
        assert (c.size[sel] > 1).sum() > 1000
    # singletons for the rest; counts
    single = (c.size == 1)
    assert single.sum() > 0.2 * n and not c.mixed[single].any()
    if empties:
        assert c.empty[0] and c.empty[n - 1] and abs(c.empty.sum() - n / 10) <= 2
        assert (c.rep[c.empty] == -1).all() and (c.size[c.empty] == 0).all()
        assert not c.mixed[c.empty].any() and (c.rep[live] >= 1).all()
        assert c.stats[0] == len(np.unique(c.g[live]))
    else:
        assert c.empty is None
        assert c.stats == [2 + n // 10 + int(single.sum()), 2 + n // 10,
                           1 + int((np.arange(n // 10) % 2).sum())]
    # lengths cross one MD5 block
    lens = np.diff(c.offsets.astype(np.int64))
    assert lens[live].min() == 9 and lens[live].max() == 70 and (lens[~live] == 0).all()
    assert (lens >= 56).sum() > n // 3


def test_dict_and_numpy_references_agree():
    """On 5,000 sequences: the ids' grouping (np.unique) equals the dict grouping over hashlib's
    digests of the sequences' bytes."""
    c = sc.random_case(5000, 77)
    assert c.empty.sum() > 100 and c.stats[1] > 500 and 0 < c.stats[2] < c.stats[1]
    seqs = [sc.sequence_bytes(c, i) for i in range(5000)]
    assert all(s == (b"" if c.empty[i] else sc.id_bytes(int(c.g[i]))) for i, s in enumerate(seqs))
    dig = np.frombuffer(b"".join(hashlib.md5(s).digest() for s in seqs), np.uint8).reshape(-1, 16)
    lengths = np.array([len(s) for s in seqs], np.uint32)
    assert same(sc.dict_grouping(dig, lengths, c.fun), (c.rep, c.size, c.mixed, c.stats))
    assert not any(bytes(d) == sc.EMPTY_MD5 for d in dig[lengths != 0])


def test_edge_view_upper_and_pattern_cases():
    for n in sc.COUNT_EDGES:
        c = sc.edge_case(n)
        assert len(c.g) == n and (n < 63 or c.empty.any()) and (n < 63 or c.stats[2] > 0)
    c = sc.view_case()
    assert len(c.g) == sc.VIEW_N == 65_537
    for k in sc.VIEW_STARTS:
        (res, off, fun), want = sc.view_of(c, k)
        assert off[0] != 0 and len(off) == sc.VIEW_N - k + 1 and len(fun) == len(off) - 1
        assert want[0].max() < sc.VIEW_N - k and not same(want, (c.rep[k:], c.size[k:],
                                                                  c.mixed[k:], c.stats))
    assert any(int(c.offsets[k]) % 4 for k in sc.VIEW_STARTS)       # a misaligned residue start
    u = sc.upper_case()
    assert u.expected[UPPER][3][0] < u.expected[0][3][0] - 10_000
    low = np.flatnonzero(u.lower)
    # (an id has 3.3 sequences on average: about 0.7 of the lower-case ones are not its first)
    assert (u.expected[UPPER][0][low] < low).sum() > 40_000          # joined an earlier group
    joined = u.expected[UPPER][0][low]
    assert (~u.lower[joined]).sum() > 30_000                         # ... led by an upper-case one
    assert (u.lower[u.expected[0][0]] == u.lower).all()              # apart under flag 0
    body = u.residues[:int(u.offsets[-1])]
    assert set(body.tolist()) <= set(sc.AA.tobytes() + sc.AA.tobytes().lower())
    c, want = sc.fun_pattern_case()
    assert (c.mixed == want).all() and c.stats == [8, 8, 5]
    assert sorted(c.size.tolist()) == [2] * 8 + [3] * 12


@pytest.mark.parametrize("record", ["lattice", "neighbours", "swaps", "same_low", "same_high",
                                    "stability"])
def test_model_of_the_grouping_equals_the_reference(record):
    r = {x.name: x for x in sc.probe_records()}[record]
    rep, size = sc.model_grouping(r.digest, r.lengths)
    assert (rep == r.rep).all() and (size == r.size).all()


# Which crafted records each broken form must get wrong.
#  - No first sort: equal high halves keep their input order, so every record with two digests
#    of one high half and shuffled copies breaks; with 7 high values, nearly every group.
#  - Two-word compare: merges neighbours of the final order (by high, then low) that share the
#    low half across a change of the high half. The one-bit flips of the high half all share the
#    base's low half; with 7 low values one boundary in a few does. Not the lattice: there every
#    high half's run starts at low 0 and ends at 2^64 - 1.
#  - 32-bit second key, low key from x twice: need halves that agree in their low word and
#    differ above it (0, 2^32 and 2^63 in the lattice; the flips of w and of y). Random halves
#    never do.
CAUGHT_BY = {
    "no first sort": ("lattice", "neighbours", "swaps", "same_low", "same_high"),
    "two-word compare": ("neighbours", "same_low"),
    "32-bit second key": ("lattice", "neighbours"),
    "low key from x twice": ("lattice", "neighbours"),
}


@pytest.mark.parametrize("broken", sorted(sc.BROKEN_MODELS))
def test_broken_models_disagree_with_the_reference(broken):
    records = {x.name: x for x in sc.probe_records()}
    for name in CAUGHT_BY[broken]:
        r = records[name]
        rep, size = sc.model_grouping(r.digest, r.lengths, **sc.BROKEN_MODELS[broken])
        wrong = int(((rep != r.rep) | (size != r.size)).sum())
        print(f"{broken}: {name}: {wrong} of {len(rep)} entries wrong")
        assert wrong > 0, (broken, name)
        if broken == "no first sort" and name.startswith("same_"):
            assert wrong > 100_000, (broken, name)                   # a third of the record
