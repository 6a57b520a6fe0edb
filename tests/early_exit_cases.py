"""Inputs of the early-exit tests, shared by tests/test_early_exit_workload.py (CPU, the oracle
alone) and tests/test_gpu_early_exit.py.

The protein probe stops probing a protein once two different fids are on its record (it ends
AMBIGUOUS whatever else it hits): at the top of every 512-window step of a block, a protein that
is dead by then loses its remaining windows. The cases plant kmers of two roles, A and B, at
chosen windows of otherwise random proteins (no other window is a table row), so that the step
in which a protein's second fid is found is known, and so is every protein that must NOT be
skipped: one role only, however late or however often it hits.

One K = 8 table of 78,000 rows: 30,000 kmers of role A (fid 11), 30,000 of role B (fid 23) and
18,000 of other fids that no protein here contains. Plain numpy; no GPU.
"""
import functools

import numpy as np

from kmeranno import synth

K = 8
MIN_HITS = 5
N_FID = 64
SEED = 97
FID_A, FID_B = 11, 23
N_ROLE, N_OTHER = 30_000, 18_000
STEP = 512          # windows per probe step of a block (256 threads x 2)
F_END_EXCLUSIVE, F_MULTISET = 1, 2
NONE, CALLED, AMBIGUOUS, BELOW_MIN = 0, 1, 2, 3  # kmeranno.STATUS_*


@functools.lru_cache(maxsize=None)
def table_rows():
    """(keys, fids): the A rows, the B rows, the others; distinct keys."""
    rng = np.random.default_rng(SEED)
    kmers = synth.AA[rng.integers(0, 20, (N_ROLE * 2 + N_OTHER + 2000, K))]
    keys = np.zeros(len(kmers), np.uint64)
    for j in range(K):
        keys = (keys << np.uint64(5)) | (kmers[:, j].astype(np.uint64) - np.uint64(64))
    _, first = np.unique(keys, return_index=True)
    keys = keys[np.sort(first)][:N_ROLE * 2 + N_OTHER]
    assert len(keys) == N_ROLE * 2 + N_OTHER
    fids = np.empty(len(keys), np.uint32)
    fids[:N_ROLE] = FID_A
    fids[N_ROLE:2 * N_ROLE] = FID_B
    others = np.array([f for f in range(N_FID) if f not in (FID_A, FID_B)], np.uint32)
    fids[2 * N_ROLE:] = others[rng.integers(0, len(others), N_OTHER)]
    return keys, fids


def _kmer(key):
    return np.frombuffer(synth.unpack_key(key, K).encode(), np.uint8)


def role_kmer(role, i):
    """The i-th kmer (K bytes) of role 'A' or 'B'."""
    keys, _ = table_rows()
    return _kmer(keys[(0 if role == "A" else N_ROLE) + i % N_ROLE])


def window_fids(prot):
    """fid of every window of a protein (-1: not a table row)."""
    skeys, sfids = _sorted_rows()
    wk = synth.window_keys(np.asarray(prot, np.uint8), K)
    at = np.searchsorted(skeys, wk)
    at[at == len(skeys)] = 0
    return np.where(skeys[at] == wk, sfids[at], -1)


@functools.lru_cache(maxsize=None)
def _sorted_rows():
    keys, fids = table_rows()
    order = np.argsort(keys)
    return keys[order], fids[order].astype(np.int64)


def protein(windows, a, b, rng):
    """A random protein of `windows` windows (windows + K - 1 residues) none of which is a table
    row, then a fresh kmer of role A at each window index in `a` and of role B at each in `b`
    (indices at least K apart). A pair (i, j) in `a` or `b` plants at i the kmer planted at j:
    a kmer that occurs twice (one key of the set, two hits of the multiset)."""
    while True:  # (drawn again if a window beside a planted kmer turns out to be a row)
        prot = _protein(windows, a, b, rng)
        if prot is not None:
            return prot


def _protein(windows, a, b, rng):
    n = windows + K - 1
    prot = synth.AA[rng.integers(0, 20, n)].copy()
    while True:
        bad = np.flatnonzero(window_fids(prot) >= 0)
        if not len(bad):
            break
        prot[bad] = synth.AA[rng.integers(0, 20, len(bad))]
    used = {}
    spots = sorted([(x, "A") for x in a] + [(x, "B") for x in b],
                   key=lambda s: s[0][0] if isinstance(s[0], tuple) else s[0])
    last = -K
    fresh = {r: iter(rng.choice(N_ROLE, len(spots), replace=False)) for r in "AB"}  # distinct
    for spot, role in spots:
        i, same = spot if isinstance(spot, tuple) else (spot, None)
        assert 0 <= i < windows and i - last >= K, (i, last)
        last = i
        if same is None:
            used[i] = role_kmer(role, int(next(fresh[role])))
        else:
            used[i] = used[same]
        prot[i:i + K] = used[i]
    wf = window_fids(prot)
    planted = {(s[0][0] if isinstance(s[0], tuple) else s[0]) for s in spots}
    return prot if set(np.flatnonzero(wf >= 0)) == planted else None


def pack(prots):
    """(residues padded by 32 bytes, offsets)."""
    off = np.zeros(len(prots) + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for p in prots], dtype=np.uint64)
    res = np.concatenate([np.asarray(p, np.uint8) for p in prots] + [np.zeros(32, np.uint8)])
    return res, off


def every(step, lo, hi):
    return tuple(range(lo, hi, step))


# name -> (windows, A windows, B windows, status, steps alone: (second fid found, last step))
# `alone`: the protein is the only one of its block (block capacity 1), so window i is span
# position i and lies in step i // 512. second fid found = None: never (not AMBIGUOUS).
def _specs():
    s = {}
    for w in (600, 1030, 1600):
        last = (w - 1) // STEP
        a = every(97, 5, w - 20)  # role A in every step
        s[f"w{w}-b-last-of-step0"] = (w, tuple(x for x in a if abs(x - 511) >= K), (511,),
                                      AMBIGUOUS, (0, last))
        s[f"w{w}-b-first-of-step1"] = (w, tuple(x for x in a if abs(x - 512) >= K), (512,),
                                       AMBIGUOUS, (1, last))
        s[f"w{w}-b-last-step-only"] = (w, tuple(x for x in a if abs(x - (w - 3)) >= K), (w - 3,),
                                       AMBIGUOUS, (last, last))
        s[f"w{w}-b-absent"] = (w, a, (), CALLED, (None, last))
    # (w1600-b-absent is the single-role protein with hits in every step: CALLED, exact count)
    s["w1600-late-single-role"] = (1600, every(61, 530, 1590), (), CALLED, (None, 3))
    s["w1600-late-two-roles"] = (1600, every(61, 530, 1000), (1100,), AMBIGUOUS, (2, 3))
    s["w600-dead-at-once"] = (600, (3, 40), (20,), AMBIGUOUS, (0, 1))
    s["w600-live"] = (600, every(53, 2, 590) + ((595, 2),), (), CALLED, (None, 1))
    s["w300-below-min"] = (300, (10, 100, 200), (), BELOW_MIN, (None, 0))
    s["w200-none"] = (200, (), (), NONE, (None, 0))
    return s


SPECS = _specs()
# The main batch: every spec once, the dead protein before the live one and after it, so that
# at block capacities 4, 6 and 8 dead and live proteins share blocks in both orders.
MAIN_ORDER = ["w600-dead-at-once", "w600-live", "w600-dead-at-once", "w200-none"] + \
    [n for n in SPECS if n not in ("w600-dead-at-once", "w600-live", "w200-none")] + \
    ["w600-live", "w600-dead-at-once", "w300-below-min", "w600-live"]
# Proteins whose set does not fit the block's LDS pool (4,096 entries less the ASCII stage, a
# set takes 1.5 entries per window: ~2,700 windows): hits go to the workspace list. One turns
# ambiguous midway, one stays single-role with repeated kmers (the list is deduplicated).
BIG_SPECS = {
    "w3000-ambiguous-midway": (3000, every(41, 7, 2990), (1503,), AMBIGUOUS, (2, 5)),
    "w3000-single-role": (3000, every(41, 7, 2900) + ((2950, 7), (2960, 48), (2975, 1442)), (),
                          CALLED, (None, 5)),
}
BIG_ORDER = ["w300-below-min", "w3000-ambiguous-midway", "w600-live", "w3000-single-role",
             "w600-dead-at-once", "w3000-ambiguous-midway"]


@functools.lru_cache(maxsize=None)
def _built(name):
    w, a, b = (SPECS.get(name) or BIG_SPECS[name])[:3]
    a = tuple(x for x in a if not any(abs((x[0] if isinstance(x, tuple) else x) - y) < K
                                      for y in b))
    return protein(w, a, b, np.random.default_rng(SEED + sum(map(ord, name))))


@functools.lru_cache(maxsize=None)
def batch(name):
    """(residues, offsets, names) of 'main', 'big' or 'mixed'.
    mixed: 1,500 proteins of 20..900 windows: 40% one role, 35% both roles (the second at a
    random window), 15% no hit, 10% fewer hits than MIN_HITS."""
    if name == "main":
        return pack([_built(n) for n in MAIN_ORDER]) + (tuple(MAIN_ORDER),)
    if name == "big":
        return pack([_built(n) for n in BIG_ORDER]) + (tuple(BIG_ORDER),)
    assert name == "mixed"
    rng = np.random.default_rng(SEED + 5)
    prots, names = [], []
    for i in range(1500):
        w = int(rng.integers(20, 900))
        kind = rng.choice(4, p=[0.40, 0.35, 0.15, 0.10])
        grid = np.arange(0, w, 9)  # candidate windows, K apart or more
        if kind == 0:
            a, b = rng.choice(grid, min(len(grid), int(rng.integers(5, 30))), replace=False), ()
        elif kind == 1:
            pick = rng.choice(grid, min(len(grid), int(rng.integers(3, 30))), replace=False)
            a, b = pick[1:], pick[:1]
        elif kind == 2:
            a, b = (), ()
        else:
            a, b = rng.choice(grid, min(len(grid), int(rng.integers(1, 5))), replace=False), ()
        prots.append(protein(w, tuple(int(x) for x in a), tuple(int(x) for x in b), rng))
        names.append(("one-role", "two-roles", "no-hit", "few-hits")[kind])
    return pack(prots) + (tuple(names),)


def protein_steps(residues, offsets, capacity, flags=0):
    """The library's block assignment, on the CPU: proteins [g P, g P + P) form a block (P =
    `capacity`); window i of a protein that starts `base` residues into its block's span is
    span position base + i and is probed in step (base + i) // 512. Per protein (first, last,
    dead): the steps of its first and last window, and the step in which its second fid is
    found from its windows' fids (-1: never; a protein without windows: all -1). A protein with
    0 <= dead < last has windows the probe may skip; one with dead == -1 keeps them all."""
    off = np.asarray(offsets, np.int64)
    out = []
    for p in range(len(off) - 1):
        base = int(off[p] - off[p - p % capacity])
        wf = window_fids(residues[off[p]:off[p + 1]])
        if flags & F_END_EXCLUSIVE:
            wf = wf[:-1]
        if not len(wf):
            out.append((-1, -1, -1))
            continue
        seen = {}
        for i in np.flatnonzero(wf >= 0):
            seen.setdefault(int(wf[i]), (base + int(i)) // STEP)
        steps = sorted(seen.values())
        out.append((base // STEP, (base + len(wf) - 1) // STEP,
                    steps[1] if len(steps) > 1 else -1))
    return out
