"""GPU parity of the streamed signature build (kma_sig_builder: csrc/kma_sigmerge.hip, the
builder in csrc/kma_abi_ops.cpp) against the one-shot build, the C oracle and a dict / numpy model
of the per-key state and its combine rule (csrc/kma_sigmerge.h).

A protein of exactly K residues is one window, so a batch of such proteins is a set of keys the
test chooses: key number m (base-26 digits, most significant first, as residues 'A' + digit) is
monotone in m, which gives the tests the numeric order of the packed keys."""
import ctypes as C
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
K = 8
CONF, BUF = 1 << 30, 1 << 31  # the model's states above every role


@pytest.fixture(scope="module")
def kma(native_lib):
    import kmeranno
    assert kmeranno.device_count() >= 1
    return kmeranno


# ---- the model ------------------------------------------------------------------------------
def combine(a, b):
    if a == b:
        return a
    hi = max(a, b)
    return hi if hi >= CONF else CONF


def fold(keys, states):
    """Per distinct key the join of its states: (ascending keys, states). With role < CONF < BUF
    the join of a group is its largest state when that is CONF or BUF, CONF when two roles
    differ, else the one role."""
    keys, states = np.asarray(keys, np.uint64), np.asarray(states, np.int64)
    if not len(keys):
        return keys, states
    order = np.argsort(keys, kind="stable")
    keys, states = keys[order], states[order]
    starts = np.flatnonzero(np.r_[True, keys[1:] != keys[:-1]])
    lo, hi = np.minimum.reduceat(states, starts), np.maximum.reduceat(states, starts)
    return keys[starts], np.where(hi >= CONF, hi, np.where(lo != hi, CONF, lo))


def counts_of(states):
    states = np.asarray(states, np.int64)
    return (len(states), int((states < CONF).sum()), int((states == CONF).sum()),
            int((states == BUF).sum()))


def info_counts(b):
    i = b.info()
    return (i.n_keys, i.n_role, i.n_conflict, i.n_buffered)


def key_batch(m, k=K):
    """Proteins of exactly k residues for the key numbers m: (residues, offsets, packed keys)."""
    m = np.asarray(m, np.int64)
    digits = np.stack([(m // 26 ** (k - 1 - j)) % 26 for j in range(k)], axis=1) if len(m) \
        else np.zeros((0, k), np.int64)
    codes = (digits + 1).astype(np.uint64)
    keys = np.zeros(len(m), np.uint64)
    for j in range(k):
        keys = (keys << np.uint64(5)) | codes[:, j]
    res = np.r_[(codes + 64).astype(np.uint8).reshape(-1), np.zeros(32, np.uint8)]
    return res, np.arange(len(m) + 1, dtype=np.uint64) * np.uint64(k), keys


def spec_batch(m, spec, a_role=3, b_role=7):
    """Key numbers m with wanted states spec (0 role A, 1 role B, 2 conflict, 3 buffered) as one
    batch: a conflict is two proteins of the kmer with different roles. Returns (residues,
    offsets, roles, model keys, model states)."""
    m, spec = np.asarray(m, np.int64), np.asarray(spec, np.int64)
    twice = np.flatnonzero(spec == 2)
    mm = np.r_[m, m[twice]]
    roles = np.r_[np.choose(spec, [a_role, b_role, a_role, -1]), np.full(len(twice), b_role)]
    perm = np.random.default_rng(len(mm)).permutation(len(mm))
    res, off, keys = key_batch(mm[perm])
    _, _, mkeys = key_batch(m)
    return res, off, roles[perm].astype(np.int32), mkeys, np.choose(spec, [a_role, b_role, CONF, BUF])


def check_builder(b, want_keys, want_states, what=""):
    """info()'s counts and finish() against the model's rows."""
    assert info_counts(b) == counts_of(want_states), what
    keys, roles = b.finish()
    kept = want_states < CONF
    assert np.array_equal(keys, want_keys[kept]), what
    assert np.array_equal(roles, want_states[kept].astype(np.uint32)), what
    return keys, roles


# ---- 1. split invariance ----------------------------------------------------------------------
def _family_proteins(rng, n_fam=80, n=1500):
    """Proteins drawn from families (mutated 8%), roles from the families with mixing: several
    roles share families (non-discriminating kmers), some proteins are buffered (-1) or
    skipped (-2). (The generator of test_gpu_build.py.)"""
    aa = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
    fams = [aa[rng.integers(0, 20, int(rng.integers(20, 400)))] for _ in range(n_fam)]
    prots, roles = [], []
    for _ in range(n):
        f = int(rng.integers(0, n_fam))
        p = fams[f].copy()
        m = rng.random(len(p)) < 0.08
        p[m] = aa[rng.integers(0, 20, int(m.sum()))]
        prots.append(p.tobytes().decode())
        u = rng.random()
        roles.append(-1 if u < 0.1 else -2 if u < 0.13 else f % 50)
    return prots, roles


def _stream(kma, k, flags, batches):
    """batches: [(prots, roles)] -> (keys, roles) after adding them in order."""
    with kma.SigBuilder(k, flags) as b:
        for prots, roles in batches:
            res, off = kma.pack_strings(prots)
            b.add(res, off, roles)
        i = b.info()
        assert i.n_adds == len(batches) and i.k == k and i.flags == flags
        assert i.n_residues == sum(len(p) for ps, _ in batches for p in ps)
        assert i.n_keys == i.n_role + i.n_conflict + i.n_buffered
        return b.finish()


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("k", [5, 8, 12])
def test_split_invariance(kma, oracle_c, flags, k):
    """However the proteins are split into adds, and in whatever order the adds come, the rows
    are the oracle's and, bit for bit, kma_build_signatures' on the whole list."""
    from kmeranno import synth
    rng = np.random.default_rng(17 + flags + k)
    prots, roles = _family_proteins(rng)
    edge = "ACDEFGHIKLMNPQRSTVWY"
    prots += ["", edge[:k - 1], edge[:k], edge[:k + 1], edge[1:k], edge[1:k + 1], edge[2:k + 3]]
    roles += [3, 3, 4, 5, -1, -1, 6]
    n = len(prots)
    res, off = oracle_c.pack_strings(prots)
    km, rl = oracle_c.build_signatures(res, off, roles, k, flags)
    exp = {bytes(r).decode(): int(v) for r, v in zip(km, rl)}
    assert len(exp) > 10_000
    one_keys, one_roles = kma.build_signatures(res, off, roles, k, flags)

    def cut(bounds):
        bounds = [0] + list(bounds) + [n]
        return [(prots[a:b], roles[a:b]) for a, b in zip(bounds[:-1], bounds[1:])]

    cuts7 = sorted(int(x) for x in rng.choice(np.arange(1, n), 7, replace=False))
    extra = [([], []), (["MKVLAAGIVALLMKVLAAGIW", prots[0], prots[1]], [-2, -2, -7]),
             (["", "", ""], [1, -1, 2])]
    interleaved = cut(cuts7)
    for at, e in zip((1, 4, 8), extra):
        interleaved.insert(at, e)
    splits = {"one batch": cut([]), "40 single proteins, then the rest": cut(range(1, 41)),
              "7 random cuts": cut(cuts7), "7 random cuts, reversed": cut(cuts7)[::-1],
              "with empty, all-skipped and only-empty-protein adds": interleaved}
    assert len(splits["40 single proteins, then the rest"]) == 41
    for what, batches in splits.items():
        keys, groles = _stream(kma, k, flags, batches)
        got = {synth.unpack_key(x, k): int(r) for x, r in zip(keys.tolist(), groles)}
        assert got == exp, what
        assert keys.dtype == one_keys.dtype and groles.dtype == one_roles.dtype
        assert np.array_equal(keys, one_keys) and np.array_equal(groles, one_roles), what
        assert (np.diff(keys.astype(np.int64)) > 0).all(), what


# ---- 2. the state lattice across batches ----------------------------------------------------
def test_state_lattice_across_batches(kma):
    """Every sequence of 1..4 events over {role A, role B, buffered, skipped} on its own kmer,
    event j in add j: the kmer survives iff the model's fold says so, with the right role, and
    info()'s counts follow the model after every add."""
    A, B = 2, 5
    events = {"A": A, "B": B, "-1": -1, "-2": -2}
    seqs = [s for n in range(1, 5) for s in itertools.product(events, repeat=n)]
    assert len(seqs) == 340
    numbers = np.arange(len(seqs), dtype=np.int64) * 7919 + 5
    _, _, all_keys = key_batch(numbers)
    state = {}
    with kma.SigBuilder(K) as b:
        for j in range(4):
            rows = [i for i, s in enumerate(seqs) if len(s) > j]
            roles = np.array([events[seqs[i][j]] for i in rows], np.int32)
            res, off, keys = key_batch(numbers[rows])
            b.add(res, off, roles)
            for key, r in zip(keys.tolist(), roles.tolist()):
                if r != -2:
                    s = BUF if r == -1 else r
                    state[key] = combine(state[key], s) if key in state else s
            assert info_counts(b) == counts_of(list(state.values())), f"after add {j}"
        keys, roles = b.finish()
    got = dict(zip(keys.tolist(), roles.tolist()))
    for s, key in zip(seqs, all_keys.tolist()):
        want = state.get(key)
        name = ",".join(s)
        if want is not None and want < CONF:
            assert got.get(key) == want, f"{name}: kept for role {want}"
        else:
            assert key not in got, f"{name}: not a discriminating kmer"
    by_name = {",".join(s): got.get(key) for s, key in zip(seqs, all_keys.tolist())}
    assert by_name["A,B,A"] is None, "A,B,A: two roles hit it in adds 1 and 2; it stays dead"
    assert by_name["A,-1,A"] is None, "A,-1,A: a buffered protein between two hits deletes it"
    assert by_name["-1,A"] is None, "-1,A: a buffered protein seen early deletes a later kmer"
    assert by_name["B,-1"] is None, "B,-1: a buffered protein seen later deletes it"
    assert by_name["A,-2,A"] == A, "A,-2,A: a skipped peg counts for nothing"
    assert by_name["-2,-2,B"] == B and by_name["A,A,A,A"] == A and by_name["A,A,A,B"] is None
    assert len(got) == sum(1 for v in state.values() if v < CONF)


# ---- 3. merge tile edges on the device ------------------------------------------------------
def _pattern_numbers(pattern, na, nb, rng):
    if pattern == "disjoint, B low":
        return np.arange(nb, nb + na), np.arange(nb)
    if pattern == "disjoint, B high":
        return np.arange(na), np.arange(na, na + nb)
    if pattern == "interleaved":
        return 2 * np.arange(na), 2 * np.arange(nb) + 1
    if pattern == "identical":
        return 3 * np.arange(na) + 10, 3 * np.arange(nb) + 10
    if pattern == "identical, one more in front of A":
        return np.r_[5, 3 * np.arange(max(na - 1, 0)) + 10][:na], 3 * np.arange(nb) + 10
    if pattern == "identical, one more in front of B":
        return 3 * np.arange(na) + 10, np.r_[5, 3 * np.arange(max(nb - 1, 0)) + 10][:nb]
    assert pattern == "random, 30% shared"
    n = 16 * max(na, nb) + 16
    a = np.sort(rng.choice(n, na, replace=False))
    take = min(int(0.3 * nb), na)
    shared = rng.choice(a, take, replace=False) if take else np.zeros(0, np.int64)
    rest = np.setdiff1d(np.arange(n), a)
    b = np.sort(np.r_[shared, rng.choice(rest, nb - take, replace=False)])
    return a, b


@pytest.mark.parametrize("pattern", ["disjoint, B low", "disjoint, B high", "interleaved",
                                     "identical", "identical, one more in front of A",
                                     "identical, one more in front of B", "random, 30% shared"])
def test_merge_tile_edges(kma, pattern):
    """Run lengths 0, 1, T - 1, T, T + 1 and 3T + 1 on both sides of one merge (T = the merge
    kernel's tile): rows and counts equal the model, and adding A again changes nothing."""
    rng = np.random.default_rng(len(pattern))
    with kma.SigBuilder(K) as probe:
        T = int(probe.info().tile)
    assert T >= 64 and T % 64 == 0
    sizes = [0, 1, T - 1, T, T + 1, 3 * T + 1]
    shared = in_both = 0
    for na, nb in itertools.product(sizes, sizes):
        what = f"{pattern}: nA = {na}, nB = {nb}"
        ma, mb = _pattern_numbers(pattern, na, nb, rng)
        assert len(ma) == na and len(mb) == nb and len(set(ma)) == na and len(set(mb)) == nb
        batch_a = spec_batch(ma, rng.integers(0, 4, na))
        batch_b = spec_batch(mb, rng.integers(0, 4, nb))
        with kma.SigBuilder(K) as b:
            b.add(*batch_a[:3])
            ka, sa = fold(batch_a[3], batch_a[4])
            check_builder(b, ka, sa, what + " (A alone)")
            b.add(*batch_b[:3])
            ku, su = fold(np.r_[batch_a[3], batch_b[3]], np.r_[batch_a[4], batch_b[4]])
            first = check_builder(b, ku, su, what)
            b.add(*batch_a[:3])
            again = check_builder(b, ku, su, what + " (A again)")
            assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
            assert b.info().n_adds == 3
        shared += na + nb - len(ku)
        in_both += len(np.intersect1d(ma, mb))
    # the equal-pair path was walked as often as the key sets say (never for the disjoint ones)
    assert shared == in_both
    assert in_both > 3 * T if pattern.startswith(("identical", "random")) else in_both == 0


# ---- 4. growth and a grid of many tiles -------------------------------------------------------
def test_growth_over_many_tiles(kma):
    """Three adds of 2^20 distinct random keys, 10% shared between consecutive adds (with roles
    drawn anew, so shared keys mostly conflict): the run buffers are reallocated, finish is
    repeatable, and an add after finish continues."""
    rng = np.random.default_rng(2024)
    n = 1 << 20
    pool = rng.permutation(np.unique(rng.integers(0, 26 ** K, 3 * n + n // 2)))[:3 * n]
    all_keys, all_states, bytes_after, keys_after = [], [], [], []
    with kma.SigBuilder(K) as b:
        for j in range(3):
            lo = j * (n - n // 10)
            m = pool[lo:lo + n]
            roles = rng.integers(0, 10, n).astype(np.int32)
            roles[rng.random(n) < 0.05] = -1
            res, off, keys = key_batch(m)
            b.add(res, off, roles)
            all_keys.append(keys)
            all_states.append(np.where(roles < 0, BUF, roles.astype(np.int64)))
            want = fold(np.concatenate(all_keys), np.concatenate(all_states))
            assert info_counts(b) == counts_of(want[1]), f"after add {j}"
            bytes_after.append(b.info().bytes)
            keys_after.append(b.info().n_keys)
            if j >= 1:
                first = check_builder(b, *want, f"finish after add {j}")
                second = b.finish()
                assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
                assert b.info().bytes == bytes_after[-1]  # finish holds nothing afterwards
        assert b.info().n_conflict > n // 20 and b.info().n_buffered > n // 10
        assert b.info().n_keys > 1000 * b.info().tile  # a merge grid of more than 1000 tiles
    # The run more than doubled after the first add, so no buffer of that time holds it: the run
    # buffers were reallocated, and the memory held grew by at least the new rows' 12 bytes each.
    assert keys_after[0] == n and keys_after[2] > 2 * keys_after[0]
    assert bytes_after[0] < bytes_after[1] < bytes_after[2]
    assert bytes_after[2] - bytes_after[0] >= 12 * (keys_after[2] - keys_after[0])


# ---- 5. all-or-nothing ------------------------------------------------------------------------
def test_failed_adds_and_finish_capacity(kma):
    rng = np.random.default_rng(5)
    prots, roles = _family_proteins(rng, n_fam=20, n=200)
    with kma.SigBuilder(K) as b:
        res, off = kma.pack_strings(prots)
        b.add(res, off, roles)
        info0, (keys0, roles0) = info_counts(b), b.finish()
        adds0, res0 = b.info().n_adds, b.info().n_residues
        n = len(keys0)
        assert n > 1000

        def unchanged(what):
            i = b.info()
            assert info_counts(b) == info0 and (i.n_adds, i.n_residues) == (adds0, res0), what
            k1, r1 = b.finish()
            assert np.array_equal(k1, keys0) and np.array_equal(r1, roles0), what

        bad = [prots[3], "ACDEFGHIKLmNPQRS", prots[4]]
        with pytest.raises(kma.KmerAnnoError) as e:
            b.add(*kma.pack_strings(bad), [1, 2, 3])
        assert e.value.code == kma.E_ALPHABET
        unchanged("after an add with a lower-case residue in a counted window")
        with pytest.raises(kma.KmerAnnoError) as e:
            b.add(*kma.pack_strings(bad), [1, -1, 3])  # ... of a buffered protein
        assert e.value.code == kma.E_ALPHABET
        unchanged("after an add with a lower-case residue in a buffered protein")
        r2, o2 = kma.pack_strings(bad)
        with pytest.raises(kma.KmerAnnoError) as e:
            b.add(r2, o2[[0, 2, 1, 3]], [1, 2, 3])
        assert e.value.code == kma.E_INVALID and "offsets decrease" in str(e.value)
        unchanged("after an add with decreasing offsets")
        with pytest.raises(kma.KmerAnnoError) as e:
            b.add(*kma.pack_strings([prots[3]]), [(1 << 24) - 1])
        assert e.value.code == kma.E_INVALID
        unchanged("after an add with a role of 2^24 - 1")
        # finish's capacity rule, through the raw entry
        L = kma.load()
        ok, orl, n_out = np.zeros(n, np.uint64), np.zeros(n, np.uint32), C.c_uint64()
        rc = L.kma_sig_builder_finish(b.handle, ok.ctypes.data, orl.ctypes.data, n - 1,
                                      C.byref(n_out))
        assert rc == kma.E_CAPACITY and n_out.value == n and not ok.any()
        assert L.kma_sig_builder_finish(b.handle, None, None, n, C.byref(n_out)) == kma.E_CAPACITY
        assert n_out.value == n
        rc = L.kma_sig_builder_finish(b.handle, ok.ctypes.data, orl.ctypes.data, n, C.byref(n_out))
        assert rc == kma.OK and n_out.value == n
        assert np.array_equal(ok, keys0) and np.array_equal(orl, roles0)
        # the residue is not counted in a skipped peg: that add succeeds and changes no row
        b.add(*kma.pack_strings(bad[1:2]), [-2])
        assert info_counts(b) == info0 and b.info().n_adds == adds0 + 1
        # and the builder goes on: the top role next to the buffered tag
        b.add(*kma.pack_strings(["WWWWHHHHWWWW"]), [(1 << 24) - 2])
        keys1, roles1 = b.finish()
        assert len(keys1) == n + 5 and int(roles1.max()) == (1 << 24) - 2
