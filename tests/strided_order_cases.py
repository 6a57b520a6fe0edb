"""Inputs of tests/test_gpu_strided_order.py: batches that aim at the protein probe's step order.

A block's span of T = ceil(span / 512) probe steps is cut into 64-position chunks [0, 8 T). The
pair (window j of a lane, wave) is slot r = 4 j + wave, and slot r takes chunk r T + s in step s:
span position x is probed in step (x // 64) % T by slot x // (64 T). The ASCII probe keeps the
residues of two steps (s, s + 1, s even) in an LDS stage of one region per slot. The cases put
table kmers where that map or that stage can go wrong; every other window is no table row, so
a window that is lost, probed twice or probed for the wrong protein changes a count or a status.

The table and the protein builder are those of tests/early_exit_cases.py (roles A and B).
Plain numpy; no GPU.
"""
import functools

import numpy as np

import early_exit_cases as ec

K = ec.K
STEP, CHUNK, SLOTS = 512, 64, 8


def steps_of(span):
    return (span + STEP - 1) // STEP


def step_at(x, T):
    """The step that probes span position x of a span of T steps."""
    return (x // CHUNK) % T


def slot_at(x, T):
    return x // (CHUNK * T)


def spaced(xs, windows, taken=()):
    """Of xs (window indices, in order of priority) those that lie in [0, windows) and at least
    K from every one kept before and from `taken`; sorted."""
    out = []
    for x in xs:
        x = int(x)
        if 0 <= x < windows and all(abs(x - y) >= K for y in out + list(taken)):
            out.append(x)
    return tuple(sorted(out))


def edge_windows(windows, T, base=0):
    """Window indices of a protein that starts at span position `base`: for every slot r and the
    steps 0, 1 (the two steps of the first stage), 2 and T - 1, the last window of chunk
    r T + s (offset 63) or the first (offset 0), in turn; s = T - 1 with offset 63 is the last
    window of the slot's part of the span, s = 0 with offset 0 the first."""
    xs = []
    for r in range(SLOTS):
        for s in sorted({0, 1 % T, 2 % T, T - 1}):
            c = r * T + s
            xs.append(CHUNK * c + (63 if (r + s) % 2 == 0 else 0) - base)
            if s in (0, T - 1):  # both sides of the border between two slots' parts
                xs.append(CHUNK * c + (0 if s == 0 else 63) - base)
    return spaced(xs, windows)


def by_step(windows, T, base, steps, gap=11, slots=None):
    """Window indices (gap apart) of a protein at span position `base` that are probed in one
    of `steps` (and, if given, by one of `slots`)."""
    xs = [i for i in range(windows)
          if step_at(base + i, T) in steps and (slots is None or slot_at(base + i, T) in slots)]
    return spaced(xs[::gap], windows)


# ---- spans: one protein per span at capacity 1 --------------------------------------------------
# residues of the protein = the span's length at capacity 1
SPAN_LENGTHS = (
    300,    # T = 1: the identity map; slots 5..7 hold nothing
    512,    # T = 1, a whole step
    513,    # T = 2: 16 chunks for 9 used; slots 5..7 wholly past the span
    1024,   # T = 2, whole steps
    1100,   # T = 3 (odd: the last stage serves one step); slots 6, 7 wholly past the span
    1280,   # T = 3, a multiple of 64 but not of 512
    2048,   # T = 4
    2055,   # T = 5
    2560,   # T = 5, whole steps
    5700,   # T = 12: slot 7 owns chunks 84..95, the span ends in chunk 89
    6144,   # T = 12, whole steps
)


@functools.lru_cache(maxsize=None)
def spans_batch():
    """Single-role proteins with a kmer at every chunk edge that matters and on a grid between
    them: CALLED, the count is the number of planted kmers. Then two-role proteins whose only
    kmers sit in different slots of one step, and in a late slot's early step and an early
    slot's late step."""
    rng = np.random.default_rng(ec.SEED + 101)
    prots, names = [], []
    for n in SPAN_LENGTHS:
        w, T = n - K + 1, steps_of(n)
        edges = edge_windows(w, T)
        a = spaced(list(edges) + [w - 1] + list(range(3, w, 37)), w)
        prots.append(ec.protein(w, a, (), rng))
        names.append(f"n{n}-single-role")
    # two roles, same step, different slots (T = 4: slot r owns span [256 r, 256 r + 256))
    n, T = 2000, 4
    w = n - K + 1
    prots.append(ec.protein(w, by_step(w, T, 0, {2}, slots={1})[:1],
                            by_step(w, T, 0, {2}, slots={5})[:1], rng))
    names.append("n2000-two-roles-one-step")
    # role B late in the span but in step 0, role A early in the span but in the last step
    a = by_step(w, T, 0, {3}, slots={0, 1})
    prots.append(ec.protein(w, a, by_step(w, T, 0, {0}, slots={7})[:1], rng))
    names.append("n2000-late-slot-early-step")
    # the same A windows alone: every one of them counts
    prots.append(ec.protein(w, a, (), rng))
    names.append("n2000-last-step-only")
    return ec.pack(prots) + (tuple(names),)


# ---- across: one block at capacities 4, 6 and 8 -------------------------------------------------
@functools.lru_cache(maxsize=None)
def across_batch():
    """Four proteins of 700, 700, 700 and 900 residues: at capacity 4 and above one block, span
    3,000, T = 6, slot r owns span [384 r, 384 r + 384). The last protein (span 2100..2999) has
    both roles in chunk 36 (slot 6, step 0) and more kmers of both after it: dead from step 1 on.
    The first three hit role A only, and only in steps 4 and 5: they are probed after the dead
    one is known, keep every hit and are CALLED."""
    rng = np.random.default_rng(ec.SEED + 102)
    lens, T = (700, 700, 700, 900), 6
    assert steps_of(sum(lens)) == T
    prots, base = [], 0
    for n in lens[:3]:
        w = n - K + 1
        a = by_step(w, T, base, {4, 5}, gap=9)
        assert len(a) >= ec.MIN_HITS
        prots.append(ec.protein(w, a, (), rng))
        base += n
    w = lens[3] - K + 1
    first = 36 * CHUNK - base  # chunk 36 = 6 T: slot 6, step 0
    assert step_at(base + first, T) == 0 and slot_at(base + first, T) == 6
    a = spaced([first + 5] + list(range(first + 70, w, 23)), w)
    b = spaced([first + 30] + list(range(first + 81, w, 23)), w, taken=a)
    prots.append(ec.protein(w, a, b, rng))
    names = ("early-late-steps",) * 3 + ("late-two-roles-step0",)
    return ec.pack(prots) + (names,)


# ---- straddle: windows that lie across two proteins ---------------------------------------------
@functools.lru_cache(maxsize=None)
def straddle_batch():
    """64 proteins of 30..140 residues (several per chunk) with role A kmers inside, and across
    every border between two of them a role B kmer: 4 residues at the end of one protein, 4 at
    the start of the next. No window of a protein holds it: probing it would turn both
    neighbours AMBIGUOUS."""
    rng = np.random.default_rng(ec.SEED + 103)
    prots = []
    for i in range(64):
        n = int(rng.integers(30, 141))
        w = n - K + 1
        a = spaced(range(6, w - 6, 9), w)
        while True:
            p = ec.protein(w, a, (), rng)
            head, tail = ec.role_kmer("B", 2 * i), ec.role_kmer("B", 2 * i + 1)
            p = p.copy()
            p[:4] = head[4:]
            p[-4:] = tail[:4]
            if set(np.flatnonzero(ec.window_fids(p) >= 0)) == set(a):
                break
        prots.append(p)
    for i in range(1, 64):  # the kmer across border i: the tail of i - 1 and the head of i agree
        kmer = ec.role_kmer("B", 2 * i)
        prots[i - 1][-4:] = kmer[:4]
        prots[i][:4] = kmer[4:]
    for i, p in enumerate(prots):
        hits = np.flatnonzero(ec.window_fids(p) >= 0)
        assert len(hits) and (ec.window_fids(p)[hits] == ec.FID_A).all(), i
    res, off = ec.pack(prots)
    joined = ec.window_fids(res[:int(off[-1])])
    assert (joined == ec.FID_B).sum() >= 60  # the kmers are there for a probe that ignores borders
    return res, off, ("straddled",) * 64


def batch(name):
    """(residues padded by 32 bytes, offsets, names)."""
    if name in ("main", "big", "mixed"):
        return ec.batch(name)
    return {"spans": spans_batch, "across": across_batch, "straddle": straddle_batch}[name]()


def brute_force_dead_steps(residues, offsets, capacity):
    """Per protein, by simulating the step order window by window: (dead step, windows probed
    after it). A step's hits are all on record at the top of the next step."""
    off = np.asarray(offsets, np.int64)
    n = len(off) - 1
    out = []
    for g0 in range(0, n, capacity):
        ps = range(g0, min(g0 + capacity, n))
        span = int(off[ps[-1] + 1] - off[g0])
        T = steps_of(span)
        seen = {p: set() for p in ps}
        dead, late = {p: -1 for p in ps}, {p: 0 for p in ps}
        fids = {p: ec.window_fids(residues[off[p]:off[p + 1]]) for p in ps}
        for s in range(T):
            hits = []
            for r in range(SLOTS):
                for x in range(CHUNK * (r * T + s), CHUNK * (r * T + s) + CHUNK):
                    for p in ps:
                        i = x - int(off[p] - off[g0])
                        if 0 <= i < len(fids[p]):
                            late[p] += dead[p] >= 0
                            if fids[p][i] >= 0:
                                hits.append((p, int(fids[p][i])))
            for p, f in hits:
                seen[p].add(f)
                if len(seen[p]) > 1 and dead[p] < 0:
                    dead[p] = s
        out += [(dead[p], late[p]) for p in ps]
    return out
