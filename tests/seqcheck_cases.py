"""Inputs and expected outputs of the duplicate check at the places its first suite could not
reach, shared by tests/test_seqcheck_workload.py (CPU, the references alone) and
tests/test_gpu_seqcheck_scale.py.

Two kinds of case.

Crafted digests, for the probe program kmers.anno_amd/host/seqcheck_probe.hip, which runs the
library's grouping (kma::launch_seq_check: two stable 64-bit radix sorts, low half then high
half, run heads by a four-word compare, max-scan, per-run atomics) on digests of the caller's
choice. Real MD5 digests never share a 64-bit half, so only chosen digests reach "equal in one
half, different in the other". A digest is 16 bytes: bytes 0..7 little-endian are the low sort key
(words x, y), bytes 8..15 the high one (z, w). The reference is `dict_grouping`: a Python dict
over bytes(digest), members in input order, the first one the rep. Records:
  lattice     (low, high) for all pairs of LATTICE_HALVES (0, 1, 2^31, 2^32 - 1, 2^32, 2^63,
              2^64 - 1, two random values), each 1, 2, 3 or 5 times, shuffled; plus five empty
              entries with the empty message's MD5. (0, 0) is there three times: a head at
              sorted position 0, which is also `start`'s value for a non-head.
  neighbours  a random digest and its 128 one-bit flips, each twice: 129 groups of 2.
  swaps       the 24 orders of four different words, each twice.
  same_low / same_high   300,000 digests, one half from 7 values, the other from 50,000.
  stability   one digest 100,000 times, interleaved 1:1 with 100,000 distinct ones.
Precondition of the grouping kernels (sc_reduce, sc_emit), kept by every record: no non-empty
entry carries the digest of an empty one.

Sequences, for kmeranno.check_sequences. Sequence i is a function of a group id g(i) alone
(`id_bytes`): the seven base-20 digits of g over ACDEFGHIKLMNPQRSTVWY, lowest first, then 'A' up
to the length 9 + g % 62 (9..70 residues; from 56 on a second MD5 block). Equal ids give equal
bytes, different ids different bytes, so the expected grouping comes from the ids with np.unique
(`id_grouping`) and owes nothing to MD5. Residues and offsets are built as numpy arrays.
`scale_case(n)` plants: BIG_ID (70 residues) on about n / 3 sequences all over the batch, the
first at index 0, one function id but for its last member; TAIL_ID (56 residues) on the last
70,000 sequences, every function id 0xFFFFFFFF; n / 10 groups of 2..5 (every other one mixed,
some all 0, some {0, 0xFFFFFFFF}); singletons elsewhere; and, where asked, 10% empty sequences,
indices 0 and n - 1 among them.

rocPRIM's radix_sort_pairs for u64 keys with u32 values, read from the installed headers
(rocprim/device/device_radix_sort.hpp, device_radix_sort_config.hpp, detail/
device_config_helper.hpp): one block up to 256 threads x 4 items = 1,024 (SINGLE_SORT_LIMIT),
merge sort up to merge_sort_limit = 1,048,576 (MERGE_SORT_LIMIT; inside it the odd-even merge up
to 2^17 + 70,000 = 201,072, merge path above), onesweep beyond. The MD5 kernel's grid is capped at
8 waves on each of 256 compute units: above MD5_GRID_CAP = 64 x 8 x 256 sequences a wave owns
more than 64 sequences by count.
Plain numpy; no GPU.
"""
import functools
import hashlib
import itertools
import struct
import types

import numpy as np

AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
UPPER = 1
NO_FUN = 0xFFFFFFFF             # fmin's initial value; 0 is fmax's
SINGLE_SORT_LIMIT = 1024
MERGE_SORT_LIMIT = 1 << 20
MD5_GRID_CAP = 64 * 8 * 256
SCALE_SIZES = (MERGE_SORT_LIMIT, MERGE_SORT_LIMIT + 1, 2_500_000)
COUNT_EDGES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 65_535,
               65_536, 65_537, SINGLE_SORT_LIMIT, SINGLE_SORT_LIMIT + 1)
VIEW_N, VIEW_STARTS = 65_537, (1, 3, 64)
EMPTY_MD5 = hashlib.md5(b"").digest()


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


# ---- crafted digests ---------------------------------------------------------------------------
def digests_of(low, high):
    """(n, 16) uint8 from the two 64-bit halves."""
    d = np.empty((len(low), 2), "<u8")
    d[:, 0], d[:, 1] = low, high
    return d.view(np.uint8).reshape(len(low), 16)


def halves_of(dig):
    d = np.ascontiguousarray(dig).view("<u8").reshape(len(dig), 2)
    return d[:, 0].copy(), d[:, 1].copy()


def dict_grouping(dig, lengths, fun):
    """The map of SequenceCheckProcessor over given digests: (rep, size, mixed, stats)."""
    groups = {}
    for i in range(len(dig)):
        if lengths[i]:
            groups.setdefault(bytes(dig[i]), []).append(i)
    n = len(dig)
    rep, size, mixed = np.full(n, -1, np.int32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    stats = [len(groups), 0, 0]
    for members in groups.values():
        bad = fun is not None and len(members) > 1 and len({int(fun[i]) for i in members}) > 1
        stats[1] += len(members) > 1
        stats[2] += bad
        for i in members:
            rep[i], size[i], mixed[i] = members[0], len(members), bad
    return rep, size, mixed, stats


def _record(name, dig, lengths, fun):
    dig = np.ascontiguousarray(dig, np.uint8)
    lengths = np.ascontiguousarray(lengths, np.uint32)
    fun = None if fun is None else np.ascontiguousarray(fun, np.uint32)
    empty = {bytes(d) for d in dig[lengths == 0]}   # the precondition
    assert not empty or not any(bytes(d) in empty for d in dig[lengths != 0]), name
    rep, size, mixed, stats = dict_grouping(dig, lengths, fun)
    _frozen(dig, lengths, fun, rep, size, mixed)
    return types.SimpleNamespace(name=name, digest=dig, lengths=lengths, fun=fun, rep=rep,
                                 size=size, mixed=mixed, stats=stats)


LATTICE_HALVES = (0, 1, 1 << 31, (1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 1,
                  0x9E3779B97F4A7C15, 0x6A09E667F3BCC908)
LATTICE_REPS = (3, 1, 2, 5)


def _shuffled(rng, dig, lengths, fun):
    p = rng.permutation(len(dig))
    return dig[p], lengths[p], fun[p]


def _group_funs(g, r):
    """Function ids of group number g with r members: even g one id (0 and NO_FUN among them),
    odd g one member apart (among them {0, NO_FUN})."""
    base = (0, 7, NO_FUN, 9)[g // 2 % 4] if g % 2 == 0 else (0, 11, 12, NO_FUN)[g // 2 % 4]
    f = [base] * r
    if g % 2 == 1:
        f[g % r] = NO_FUN if base == 0 else 0 if base == NO_FUN else base + 1
    return f


@functools.lru_cache(maxsize=None)
def lattice():
    low, high, fun = [], [], []
    for g, (ia, ib) in enumerate(itertools.product(range(9), repeat=2)):
        r = LATTICE_REPS[(ia + 2 * ib + ia * ib) % 4]
        low += [LATTICE_HALVES[ia]] * r
        high += [LATTICE_HALVES[ib]] * r
        fun += _group_funs(g, r)
    dig = digests_of(np.array(low, np.uint64), np.array(high, np.uint64))
    lengths = np.full(len(dig), 20, np.uint32)
    dig = np.concatenate([dig, np.tile(np.frombuffer(EMPTY_MD5, np.uint8), (5, 1))])
    lengths = np.concatenate([lengths, np.zeros(5, np.uint32)])
    fun = np.array(fun + [3, 0, NO_FUN, 4, 5], np.uint32)
    return _record("lattice", *_shuffled(np.random.default_rng(5901), dig, lengths, fun))


@functools.lru_cache(maxsize=None)
def neighbours():
    rng = np.random.default_rng(5902)
    base = int.from_bytes(rng.bytes(16), "little")
    vals = [base] + [base ^ (1 << b) for b in range(128)]
    dig = np.frombuffer(b"".join(v.to_bytes(16, "little") for v in vals), np.uint8)
    dig = np.repeat(dig.reshape(129, 16), 2, axis=0)
    fun = np.repeat(np.arange(129, dtype=np.uint32), 2)
    fun[1::4] += 1000           # every other group mixed
    return _record("neighbours",
                   *_shuffled(rng, dig, np.full(258, 1, np.uint32), fun))


@functools.lru_cache(maxsize=None)
def swaps():
    words = (0x01234567, 0x89ABCDEF, 0x0F1E2D3C, 0xF0E1D2C3)
    dig = np.array([p for p in itertools.permutations(words)], "<u4").view(np.uint8)
    dig = np.repeat(dig.reshape(24, 16), 2, axis=0)
    fun = np.repeat(np.arange(24, dtype=np.uint32), 2)
    fun[1::6] = NO_FUN
    return _record("swaps", *_shuffled(np.random.default_rng(5903), dig,
                                       np.full(48, 300, np.uint32), fun))


@functools.lru_cache(maxsize=None)
def same_half(which):
    """which = 'low': the low halves come from 7 values, the high ones from 50,000."""
    rng = np.random.default_rng(5904 + (which == "low"))
    n = 300_000
    few = rng.integers(0, 1 << 64, 7, dtype=np.uint64, endpoint=False)
    many = rng.integers(0, 1 << 64, 50_000, dtype=np.uint64, endpoint=False)
    a, b = few[rng.integers(0, 7, n)], many[rng.integers(0, 50_000, n)]
    dig = digests_of(a, b) if which == "low" else digests_of(b, a)
    fun = rng.integers(0, 3, n).astype(np.uint32)
    return _record("same_" + which, dig, np.full(n, 40, np.uint32), fun)


@functools.lru_cache(maxsize=None)
def stability():
    rng = np.random.default_rng(5906)
    n = 100_000
    dig = rng.integers(0, 256, (2 * n, 16), dtype=np.uint8)
    dig[0::2] = dig[0]
    fun = np.full(2 * n, 6, np.uint32)
    fun[2 * n - 2] = 0          # mixed by its last copy alone
    return _record("stability", dig, np.full(2 * n, 9, np.uint32), fun)


def probe_records():
    return [lattice(), neighbours(), swaps(), same_half("low"), same_half("high"), stability()]


def write_records(path, records):
    with open(path, "wb") as f:
        for r in records:
            f.write(struct.pack("<II", len(r.digest), r.fun is not None))
            f.write(r.digest.tobytes())
            f.write(r.lengths.astype("<u4").tobytes())
            if r.fun is not None:
                f.write(r.fun.astype("<u4").tobytes())


def read_results(path, records):
    """[(rep, size, mixed, stats)] of the probe's output file, one per record."""
    out = []
    with open(path, "rb") as f:
        for r in records:
            n = len(r.digest)
            assert struct.unpack("<I", f.read(4))[0] == n, r.name
            rep = np.frombuffer(f.read(4 * n), "<i4")
            size = np.frombuffer(f.read(4 * n), "<u4")
            mixed = np.frombuffer(f.read(n), np.uint8)
            stats = list(struct.unpack("<3Q", f.read(24)))
            assert len(mixed) == n, r.name
            out.append((rep, size, mixed, stats))
        assert f.read() == b""
    return out


# ---- numpy models of the device grouping, whole and broken -------------------------------------
def model_grouping(dig, lengths, first_sort=True, words=4, high_bits=64, x_twice=False):
    """The device's steps in numpy: stable sort by the low key, stable sort by the high key, heads
    where a neighbour's words differ, members counted at the head. The defaults are the code as
    it is; each argument switches in one wrong form: no first sort, a compare of the first
    `words` words, a second sort over `high_bits` bits, a low key made of x twice."""
    w = np.ascontiguousarray(dig).view("<u4").reshape(len(dig), 4).astype(np.uint64)
    low = (w[:, 0] if x_twice else w[:, 1]) << np.uint64(32) | w[:, 0]
    high = w[:, 3] << np.uint64(32) | w[:, 2]
    if high_bits < 64:
        high = high & np.uint64((1 << high_bits) - 1)
    order = np.argsort(low, kind="stable") if first_sort else np.arange(len(dig))
    order = order[np.argsort(high[order], kind="stable")]
    s = w[order][:, :words]
    head = np.ones(len(dig), bool)
    head[1:] = (s[1:] != s[:-1]).any(axis=1)
    start = np.maximum.accumulate(np.where(head, np.arange(len(dig)), 0))
    live = lengths[order] != 0
    count = np.bincount(start[live], minlength=len(dig))
    rep, size = np.full(len(dig), -1, np.int32), np.zeros(len(dig), np.uint32)
    rep[order[live]] = order[start[live]]
    size[order[live]] = count[start[live]]
    return rep, size


BROKEN_MODELS = {
    "no first sort": dict(first_sort=False),
    "two-word compare": dict(words=2),
    "32-bit second key": dict(high_bits=32),
    "low key from x twice": dict(x_twice=True),
}


# ---- sequences from group ids ------------------------------------------------------------------
ID_DIGITS = 7
BIG_ID, TAIL_ID, SMALL_ID0 = 61, 47, 1000
TAIL_MEMBERS = 70_000


def id_length(g):
    return 9 + np.asarray(g, np.int64) % 62


def id_bytes(g: int) -> bytes:
    """One id's sequence (the scalar statement of `build_batch`)."""
    digits = bytes(AA[g // 20 ** d % 20] for d in range(ID_DIGITS))
    return digits + b"A" * (int(id_length(g)) - ID_DIGITS)


def build_batch(g, empty=None, lower=None):
    """(residues padded by 32 bytes, offsets) of the ids g; empty[i]: sequence i has no residue;
    lower[i]: its residues are in lower case."""
    g = np.asarray(g, np.int64)
    assert g.min() >= 0 and g.max() < 20 ** ID_DIGITS
    lens = id_length(g)
    if empty is not None:
        lens = np.where(empty, 0, lens)
    off = np.zeros(len(g) + 1, np.uint64)
    np.cumsum(lens, out=off[1:])
    res = np.full(int(off[-1]) + 32, ord("A"), np.uint8)
    res[int(off[-1]):] = 0
    live = np.flatnonzero(lens)
    at = off[:-1][live].astype(np.int64)
    for d in range(ID_DIGITS):
        res[at + d] = AA[g[live] // 20 ** d % 20]
    if lower is not None:
        res[:int(off[-1])] |= np.repeat(np.where(lower, 0x20, 0).astype(np.uint8), lens)
    return res, off


def id_grouping(key, empty, fun):
    """Expected (rep, size, mixed, stats) from group keys alone: np.unique over the non-empty
    sequences' keys; a group's rep is its first index."""
    n = len(key)
    rep, size, mixed = np.full(n, -1, np.int32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    live = np.arange(n) if empty is None else np.flatnonzero(~np.asarray(empty))
    if len(live) == 0:
        return rep, size, mixed, [0, 0, 0]
    _, first, inv, counts = np.unique(np.asarray(key)[live], return_index=True,
                                      return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    rep[live] = live[first[inv]]
    size[live] = counts[inv]
    bad = np.zeros(len(counts), bool)
    if fun is not None:
        by_group = np.argsort(inv, kind="stable")
        starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
        f = np.asarray(fun, np.uint32)[live][by_group]
        bad = (counts > 1) & (np.minimum.reduceat(f, starts) != np.maximum.reduceat(f, starts))
        mixed[live] = bad[inv]
    return rep, size, mixed, [len(counts), int((counts > 1).sum()), int(bad.sum())]


def _case(g, empty, fun, lower=None, **planted):
    res, off = build_batch(g, empty, lower)
    rep, size, mixed, stats = id_grouping(g, empty, fun)
    _frozen(g, empty, fun, lower, res, off, rep, size, mixed)
    return types.SimpleNamespace(g=g, empty=empty, fun=fun, lower=lower, residues=res,
                                 offsets=off, rep=rep, size=size, mixed=mixed, stats=stats,
                                 **planted)


@functools.lru_cache(maxsize=None)
def scale_case(n, empties=False):
    rng = np.random.default_rng(5910 + n % 1000)
    tail0 = n - TAIL_MEMBERS
    g = np.full(n, -1, np.int64)
    fun = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    fun[rng.integers(0, n, 1000)] = 0
    fun[rng.integers(0, n, 1000)] = NO_FUN
    g[tail0:] = TAIL_ID
    fun[tail0:] = NO_FUN
    free = rng.permutation(np.arange(2 if empties else 1, tail0))
    n_big = n // 3
    big = np.concatenate([[1 if empties else 0], free[:n_big - 1]])
    g[big] = BIG_ID
    sizes = rng.integers(2, 6, n // 10)
    members = free[n_big - 1:n_big - 1 + int(sizes.sum())]
    group = np.repeat(np.arange(len(sizes)), sizes)
    rank = np.arange(len(members)) - np.repeat(np.cumsum(sizes) - sizes, sizes)
    g[members] = SMALL_ID0 + group
    # small group j: even j one id (j % 8 == 0: all 0, j % 8 == 2: all NO_FUN), odd j its
    # member of rank 0 apart (j % 8 == 1: 0 against NO_FUN)
    kind = group % 8
    f = (group + 10).astype(np.uint32)
    f[(kind == 0) | (kind == 1)] = 0
    f[kind == 2] = NO_FUN
    odd = (group % 2 == 1) & (rank == 0)
    f[odd] = np.where(kind[odd] == 1, NO_FUN, f[odd] + 1)
    fun[members] = f
    rest = np.flatnonzero(g < 0)
    g[rest] = SMALL_ID0 + len(sizes) + np.arange(len(rest))
    empty = None
    if empties:
        empty = np.zeros(n, bool)
        empty[rng.choice(n, n // 10, replace=False)] = True
        empty[[0, n - 1]] = True
        empty[1] = False
    live_big = big if empty is None else big[~empty[big]]
    fun[live_big] = 77
    fun[live_big.max()] = 78    # the big group is mixed by its last member alone
    return _case(g, empty, fun, big=np.sort(live_big), small_sizes=sizes, small_members=members,
                 small_group=group, tail0=tail0)


def random_case(n, seed, empties=True):
    """n sequences over about n / 2 ids, function ids from {0, 1, NO_FUN}, one in 16 empty."""
    rng = np.random.default_rng(seed)
    g = SMALL_ID0 + rng.integers(0, max(1, n // 2), n)
    fun = np.array([0, 1, NO_FUN], np.uint32)[rng.integers(0, 3, n)]
    empty = rng.random(n) < 1 / 16 if empties and n >= 63 else None
    return _case(g, empty, fun)


@functools.lru_cache(maxsize=None)
def edge_case(n):
    return random_case(n, 5920 + n)


@functools.lru_cache(maxsize=None)
def view_case():
    return random_case(VIEW_N, 5930)


def view_of(case, k):
    """The batch from sequence k on, as a caller passes it (the residue buffer whole, offsets[k:])
    and what it must give: the grouping of the suffix, rep counted from k."""
    empty = None if case.empty is None else case.empty[k:]
    return (case.residues, case.offsets[k:], case.fun[k:]), id_grouping(case.g[k:], empty,
                                                                         case.fun[k:])


@functools.lru_cache(maxsize=None)
def upper_case():
    """200,000 sequences over 60,000 ids, a third in lower case: under KMA_MD5_UPPER a lower-case
    copy joins its id's group, under flag 0 the two cases of an id are two groups."""
    rng = np.random.default_rng(5940)
    n = 200_000
    g = SMALL_ID0 + rng.integers(0, 60_000, n)
    lower = rng.random(n) < 1 / 3
    fun = rng.integers(0, 4, n).astype(np.uint32)
    res, off = build_batch(g, None, lower)
    folded = id_grouping(g, None, fun)
    apart = id_grouping(2 * g + lower, None, fun)
    _frozen(g, lower, fun, res, off, *folded[:3], *apart[:3])
    return types.SimpleNamespace(g=g, lower=lower, fun=fun, residues=res, offsets=off,
                                 expected={UPPER: folded, 0: apart})


# (function ids of one group, its expected mixed)
FUN_PATTERNS = [((0, 0), 0), ((0, 1), 1), ((NO_FUN, NO_FUN), 0), ((0, NO_FUN), 1),
                ((5, 5, 5), 0), ((6, 5, 5), 1), ((5, 6, 5), 1), ((5, 5, 6), 1)]


def fun_pattern_case():
    """One group per pattern, members interleaved over the batch, and the expected mixed."""
    g, fun, want = [], [], []
    for rank in range(3):
        for j, (ids, bad) in enumerate(FUN_PATTERNS):
            if rank < len(ids):
                g.append(SMALL_ID0 + j)
                fun.append(ids[rank])
                want.append(bad)
    case = _case(np.array(g, np.int64), None, np.array(fun, np.uint32))
    return case, np.array(want, np.uint8)


def sequence_bytes(case, i):
    return case.residues[int(case.offsets[i]):int(case.offsets[i + 1])].tobytes()
