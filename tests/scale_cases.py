"""Protein batches of up to 2^32 - 128 residues and their expected outputs, shared by
tests/test_scale_workload.py (CPU, the oracle alone) and tests/test_gpu_scale32.py.

A batch of N residues is one small base tile of about 100 proteins repeated: windows that straddle
two proteins are never probed, so a protein's outputs depend on that protein alone, and the
expected outputs of the big batch are the oracle's outputs on the base tile, tiled. The oracle runs
on a few hundred kB; the big buffers are built from the tile (np.tile on the host,
torch.Tensor.repeat on the device). After the last whole tile comes a partial tile of whole
proteins, then one filler protein without a table hit (NONE) whose length makes offsets[-1] equal
the requested N exactly.

The base tile (fixed seed; the residues do not depend on K, the table's rows are the K-windows of
its prototypes, so one residue buffer serves a K = 8 and a K = 7 table):
  - ordinary proteins of 50..900 residues: mutated copies of one prototype (CALLED), halves of two
    prototypes (AMBIGUOUS), random residues (NONE), nine residues of a prototype inside random ones
    (BELOW_MIN);
  - empty proteins and proteins of 6, 7, 8 and 9 residues (K - 1, K, K + 1 for both K), cut from
    prototypes;
  - HIGH: a prototype over the symbols of codes 26..31 ('Z', '*' and the four extra bytes of
    alphabet_cases.EXTRA) with bytes that have no code (alphabet_cases.NOISE) inside it;
  - G30: 30,000 random residues with ten clean copies of one prototype: one role, fewer hits than
    the LDS pool has entries. Its set of 1.5 x windows entries exceeds any LDS pool, so it keeps a
    list in workspace memory that is deduplicated in the pool;
  - L60: the 3,000-residue prototype LONG twenty times over, 60,000 residues: every window is a
    table row (the table holds LONG's cyclic windows), more hits than the pool has entries, so
    its list is deduplicated in a hash set in the second half of its workspace region;
  - A30: 15,000 residues of LONG, then 15,000 of another prototype: a workspace list that is
    dropped when the protein turns AMBIGUOUS midway.
The tile's length is odd (so successive tiles start at every byte alignment and at every position
of a 64-residue packed group); `aligned` gives a second tile of the same proteins whose length is a
multiple of 64, so that its host-packed stream can be tiled as 40-byte groups.
Plain numpy and the C oracle; no GPU.
"""
import functools
import types

import numpy as np

from alphabet_cases import EXTRA, NOISE

KS = (8, 7)
MIN_HITS = 5
SEED = 83
N_PROTO = 30                    # roles 1..30: prototypes of PROTO_LEN residues
PROTO_LEN = 200
FID_HIGH, FID_LONG = 31, 32
N_FID = 33                      # fid 0 belongs to no row
LONG_LEN = 3000
N_ORDINARY = 90
MIN_FILLER = 16                 # the filler protein has windows of its own
NONE, CALLED, AMBIGUOUS, BELOW_MIN = 0, 1, 2, 3
AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
HIGH_SYMS = np.frombuffer(b"Z*" + EXTRA, np.uint8)   # codes 26..31
N_MAX = (1 << 32) - 128         # the device entries' limit (include/kmeranno.h)


@functools.lru_cache(maxsize=None)
def protos():
    """Prototype 0 is unused; 1..30 ordinary, FID_HIGH over codes 26..31, FID_LONG the long one."""
    rng = np.random.default_rng(SEED)
    p = [np.zeros(0, np.uint8)] + [AA[rng.integers(0, 20, PROTO_LEN)] for _ in range(N_PROTO)]
    p.append(HIGH_SYMS[rng.integers(0, len(HIGH_SYMS), 150)])
    p.append(AA[rng.integers(0, 20, LONG_LEN)])
    return p


@functools.lru_cache(maxsize=None)
def filler_pattern():
    return AA[np.random.default_rng(SEED + 1).integers(0, 20, 997)]


def _windows(text, k):
    return {text[i:i + k].tobytes() for i in range(len(text) - k + 1)}


@functools.lru_cache(maxsize=None)
def table_rows(k):
    """(kmers as bytes, fids int32) in file order: every K-window of every prototype, LONG's
    cyclic ones included (a copy of LONG followed by another has no window outside the table).
    No kmer has two roles, and no window of the cyclic filler pattern is a row."""
    p = protos()
    rows = {}
    for fid in range(1, N_FID):
        text = np.concatenate([p[fid], p[fid][:k - 1]]) if fid == FID_LONG else p[fid]
        for km in sorted(_windows(text, k)):
            assert rows.setdefault(km, fid) == fid, "a kmer with two roles"
    fp = filler_pattern()
    assert not (_windows(np.concatenate([fp, fp[:k - 1]]), k) & rows.keys())
    order = np.random.default_rng(SEED + 2).permutation(len(rows))
    items = list(rows.items())
    return [items[i][0] for i in order], np.array([items[i][1] for i in order], np.int32)


_ORACLE = {}


def oracle_table(oracle_c, k):
    if k not in _ORACLE:
        _ORACLE[k] = oracle_c.Table(*table_rows(k))
    return _ORACLE[k]


def _mutate(rng, text, rate):
    out = text.copy()
    m = rng.random(len(out)) < rate
    out[m] = AA[rng.integers(0, 20, int(m.sum()))]
    return out


def _copy_of(rng, proto, n):
    """n residues of a prototype read cyclically from a random start."""
    return np.resize(np.roll(proto, -int(rng.integers(0, len(proto)))), n)


@functools.lru_cache(maxsize=None)
def base(aligned=False):
    """The base tile: res (no padding), off (uint64), n proteins, T residues, and the indices of
    the special proteins (g30, l60, a30, high, tuner) and of the empty and tiny ones."""
    rng = np.random.default_rng(SEED + 3)
    p = protos()
    prots, kinds = [], []
    for i in range(N_ORDINARY):
        n = int(rng.integers(50, 901))
        f, g = (int(x) for x in 1 + rng.choice(N_PROTO, 2, replace=False))
        kind = (CALLED, AMBIGUOUS, NONE, CALLED, BELOW_MIN, CALLED, NONE, AMBIGUOUS, CALLED)[i % 9]
        if kind == CALLED:
            t = _mutate(rng, _copy_of(rng, p[f], n), 0.05)
        elif kind == AMBIGUOUS:
            t = np.concatenate([_copy_of(rng, p[f], n // 2), _copy_of(rng, p[g], n - n // 2)])
        elif kind == NONE:
            t = AA[rng.integers(0, 20, n)]
        else:
            t = AA[rng.integers(0, 20, n)]
            at = int(rng.integers(0, n - 9))
            t[at:at + 9] = p[f][20:29]
        if i % 10 == 3:  # bytes without a code inside ordinary proteins
            t = t.copy()
            t[rng.integers(0, n, 3)] = np.frombuffer(NOISE, np.uint8)[rng.integers(0, len(NOISE), 3)]
        prots.append(t)
        kinds.append("ordinary")
    tiny = [p[1][:0], p[2][:6], p[3][:7], p[4][:8], p[5][:9], p[1][:0], p[6][40:48], p[1][:0],
            p[FID_HIGH][:8], p[7][:1]]
    prots += tiny
    kinds += ["tiny"] * len(tiny)
    high = p[FID_HIGH].copy()
    high[[20, 77, 78, 120]] = np.frombuffer(NOISE, np.uint8)[[0, 3, 4, 1]]
    g30 = AA[rng.integers(0, 20, 30_000)]
    for j in range(10):
        g30[1500 + 2900 * j:1500 + 2900 * j + PROTO_LEN] = p[3]
    l60 = np.tile(p[FID_LONG], 20)
    a30 = np.concatenate([np.tile(p[FID_LONG], 5), np.resize(p[4], 15_000)])
    special = {"high": high, "g30": g30, "l60": l60, "a30": a30,
               "tuner": AA[rng.integers(0, 20, 400)]}
    prots += list(special.values())
    kinds += list(special)
    order = rng.permutation(len(prots))
    prots, kinds = [prots[i] for i in order], [kinds[i] for i in order]
    # the tuner's length sets the tile's: odd, or a multiple of 64
    total = sum(len(t) for t in prots)
    cut = total % 64 if aligned else 1 - total % 2
    at = kinds.index("tuner")
    prots[at] = prots[at][:len(prots[at]) - cut]
    off = np.zeros(len(prots) + 1, np.uint64)
    off[1:] = np.cumsum([len(t) for t in prots], dtype=np.uint64)
    res = np.concatenate(prots)
    for a in (res, off):
        a.flags.writeable = False
    T = int(off[-1])
    assert T % 64 == 0 if aligned else T % 2 == 1
    where = {name: kinds.index(name) for name in special}
    return types.SimpleNamespace(res=res, off=off, n=len(prots), T=T, aligned=aligned,
                                 tiny=[i for i, x in enumerate(kinds) if x == "tiny"],
                                 ordinary=[i for i, x in enumerate(kinds) if x == "ordinary"],
                                 **where)


def base_expected(oracle_c, k, flags, aligned=False):
    """The oracle's (fid, count, status) on the base tile alone, computed once and frozen."""
    key = (k, flags, aligned)
    if key not in _ORACLE:
        b = base(aligned)
        res = np.concatenate([b.res, np.zeros(32, np.uint8)])
        e = oracle_c.apply_mt(oracle_table(oracle_c, k), res, np.ascontiguousarray(b.off), k,
                              MIN_HITS, flags, 4)
        for a in e:
            a.flags.writeable = False
        _ORACLE[key] = e
    return _ORACLE[key]


def layout(n_total, aligned=False):
    """The batch of exactly n_total residues: `reps` whole tiles, the first `m` proteins of one
    more, and the filler. offsets: the full uint64 array (n_seq + 1 entries, built vectorised)."""
    b = base(aligned)
    assert n_total >= MIN_FILLER
    reps = n_total // b.T
    while True:
        rem = n_total - reps * b.T
        # the most whole proteins that leave the filler MIN_FILLER residues or more
        m = int(np.searchsorted(b.off, rem - MIN_FILLER, side="right")) - 1 if rem >= MIN_FILLER \
            else -1
        if m >= 0:
            break
        reps -= 1  # the remainder is too short for a filler: one tile fewer
    m = min(m, b.n)
    tiles = (np.arange(reps, dtype=np.uint64)[:, None] * np.uint64(b.T) + b.off[None, :-1]).ravel()
    tail0 = np.uint64(reps * b.T)
    offsets = np.concatenate([tiles, tail0 + b.off[:m + 1], np.array([n_total], np.uint64)])
    n_seq = reps * b.n + m + 1
    filler = n_total - reps * b.T - int(b.off[m])
    assert len(offsets) == n_seq + 1 and filler >= MIN_FILLER and int(offsets[-1]) == n_total
    assert not (np.diff(offsets.view(np.int64)) < 0).any()
    return types.SimpleNamespace(base=b, n_total=n_total, reps=reps, m=m, filler=filler,
                                 n_seq=n_seq, offsets=offsets, tail0=int(tail0))


def tail_residues(lay):
    """The residues after the last whole tile: the partial tile and the filler."""
    b = lay.base
    return np.concatenate([b.res[:int(b.off[lay.m])], np.resize(filler_pattern(), lay.filler)])


def materialise(lay, pad=32):
    """The whole batch on the host, `pad` zero bytes after it."""
    return np.concatenate([np.tile(lay.base.res, lay.reps), tail_residues(lay),
                           np.zeros(pad, np.uint8)])


def residues_at(lay, lo, hi):
    """Residues [lo, hi) of the batch without building it."""
    pos = np.arange(lo, hi, dtype=np.int64)
    tail = tail_residues(lay)
    out = lay.base.res[pos % lay.base.T]
    past = pos >= lay.tail0
    out[past] = tail[pos[past] - lay.tail0]
    return out


def expected(oracle_c, lay, k, flags, lo=0, hi=None):
    """(fid, count, status, tally) of proteins [lo, hi) of the batch: the base tile's, tiled, and
    the filler's (-1, 0, NONE), which does not touch the tally."""
    hi = lay.n_seq if hi is None else hi
    efid, ecnt, est = base_expected(oracle_c, k, flags, lay.base.aligned)
    idx = np.arange(lo, hi)
    at = idx % lay.base.n
    fid, cnt, st = efid[at], ecnt[at], est[at]
    last = idx == lay.n_seq - 1
    fid[last], cnt[last], st[last] = -1, 0, NONE
    tally = np.bincount(fid[st == CALLED], minlength=N_FID).astype(np.uint32)
    return fid, cnt, st, tally


def proteins_holding(lay, name, lo, hi):
    """How many copies of the base tile's special protein `name` lie in proteins [lo, hi)."""
    idx = np.arange(lo, min(hi, lay.n_seq - 1))
    return int((idx % lay.base.n == getattr(lay.base, name)).sum())
