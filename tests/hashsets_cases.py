"""Cases for genome_sets_kernel (csrc/kma_hashsets.hip): the in-block bitonic sort, the head rule
across a long protein's sorted runs, and a block's second protein; with a plain reference and a
numpy model of one block. tests/test_hashsets_workload.py shows on the CPU that the cases aim
where they claim; tests/test_gpu_hashsets_sort.py runs them.

Reference: a protein's key set is the Python set of its K-byte substrings (hashindex_cases.kmers,
set_model); the index is the sorted list of distinct keys over all prototypes, a key being 5 bits
per residue, first residue highest, A-Z as 1..26 and '*' as 27 (key_of).

block_model() walks one protein the way one workgroup does: chunks of W windows, keys padded with
the sentinel to the next power of two, the sets_step_low / sets_step_ascending network step by
step, the head rule with its binary search on the runs as they were stored (sorted or not), the
per-chunk alphabet flag. Hooks alter one (m, j) step or the runs the head rule searches. The model
shows that a wrong kernel would be seen on these inputs; it is not the GPU test's reference.

Why the inputs are duplicate-heavy: when all window keys of a protein differ, an unsorted chunk
has exactly the heads of a sorted one and the network is not observed. Every sort-focused protein
here has at most half as many distinct keys as windows (asserted where it is built).

 (a) network_case():  every network size n2 = 2 .. 4096 at the default W: proteins of n2, n2 - 1
                      and n2 / 2 + 1 windows (several per size below 128), K = 2.
 (b) every_w_case():  W = 64 .. 2048: 3W + 17 and 2W windows; keys of run 0 again in runs 1 and 2,
                      keys in runs 0 and 2 only, keys in run 2 and the partial run only, keys in
                      the partial run only, and the largest key of run 0 once there and again later.
 (c) default_w_case(): the same at W = 4096 (2W + 41 and 3W + 17 windows).
 (d) every_k_case(k): K = 2 .. 12 on 3W + 17 windows at W = 64; from K = 7 over 2 or 3 letters
                      that include Z and '*' (codes 26 and 27).
 (e) scale_case():    2^20 + 517 proteins at W = 64: 517 blocks take a second protein.
 (f) flag_case():     a byte without a code at the positions where the code loop could miss it."""
import functools

import numpy as np

import hashindex_cases as hc
from hashindex_cases import GRID, kmers, pack, set_model

BLOCK = 256                      # kSetsBlock
W_MIN, W_MAX = 64, 4096          # kSetsKeysMin, kSetsKeysMax (the default W)
EMPTY = 0xFFFFFFFF               # kHashEmpty
SENTINEL = np.uint64(2 ** 64 - 1)  # kKeySentinel
MIN_SIM = 0.0125
LETTERS = "ACDEFGHIKLMNPQRSTVWY"

LUT = np.zeros(256, np.uint8)    # sets_code
LUT[65:91] = np.arange(1, 27)
LUT[ord("*")] = 27


# ---- the plain reference
def key_of(kmer):
    v = 0
    for ch in kmer:
        v = v << 5 | (27 if ch == "*" else ord(ch) - 64)
    return v


def ref_keys(s, k):
    """The protein's distinct keys, ascending."""
    return sorted(key_of(x) for x in kmers(s, k))


def index_keys(protos, k):
    """The index's unique keys: position -> key."""
    return sorted({key_of(x) for p in protos for x in kmers(p, k)})


def scratch_layout(n_residues, n_genome):
    """Mirror of hash_scratch_layout (csrc/kma_hashsets.h): byte offsets of gmatch (uint32 per
    position), gsize (uint32 per protein) and the runs (uint64 per position), and the total."""
    def up16(v):
        return (v + 15) & ~15
    gsize = up16(4 * n_residues)
    runs = gsize + up16(4 * n_genome)
    return 0, gsize, runs, runs + up16(8 * n_residues) + 16


# ---- the block model
def window_keys(codes, k):
    n = len(codes) - k + 1
    v = np.zeros(max(n, 0), np.uint64)
    for j in range(k):
        v = (v << np.uint64(5)) | codes[j:j + n].astype(np.uint64)
    return v


def padded_size(n):
    p = 1
    while p < n:
        p <<= 1
    return p


def network_steps(n2):
    """The (m, j) compare-exchange steps of the size-n2 network, in order."""
    out, m = [], 2
    while m <= n2:
        j = m >> 1
        while j:
            out.append((m, j))
            j >>= 1
        m <<= 1
    return out


@functools.lru_cache(maxsize=None)
def step_pairs(n2, m, j):
    t = np.arange(n2 // 2, dtype=np.int64)
    lo = ((t & ~(j - 1)) << 1) | (t & (j - 1))       # sets_step_low
    return lo, lo | j, (lo & m) == 0                 # sets_step_ascending


def sort_network(key, step=None):
    """The network on key (its length a power of two; 2-D: one input per column), in place.
    step(n2, m, j) -> None (the step as it is), "skip", "invert" (every pair's direction) or "m2"
    (direction from low & (m << 1))."""
    n2 = len(key)
    for m, j in network_steps(n2):
        mode = step(n2, m, j) if step else None
        if mode == "skip":
            continue
        lo, hi, asc = step_pairs(n2, m, j)
        if mode == "invert":
            asc = ~asc
        elif mode == "m2":
            asc = (lo & (m << 1)) == 0
        x, y = key[lo], key[hi]
        swap = (x > y) == asc.reshape((-1,) + (1,) * (key.ndim - 1))
        key[lo], key[hi] = np.where(swap, y, x), np.where(swap, x, y)
    return key


def run_holds(run, n, v):
    """sets_run_holds for every v at once: the same binary search, whatever the run holds."""
    lo = np.zeros(len(v), np.int64)
    hi = np.full(len(v), n, np.int64)
    if n == 0:
        return np.zeros(len(v), bool)
    while (lo < hi).any():
        act = lo < hi
        mid = lo + ((hi - lo) >> 1)
        less = run[np.minimum(mid, n - 1)] < v
        lo = np.where(act & less, mid + 1, lo)
        hi = np.where(act & ~less, mid, hi)
    return (lo < n) & (run[np.minimum(lo, n - 1)] == v)


class Block:
    """heads: the keys the block counts, in the order found; runs: the key area as the block
    left it (None for a protein of at most W windows); bad: per chunk, whether its code loop met
    a byte without a code."""

    def __init__(self, heads, runs, bad):
        self.heads, self.runs, self.bad = heads, runs, bad

    @property
    def gsize(self):
        return len(self.heads)

    def same_heads(self, other):
        return sorted(self.heads.tolist()) == sorted(other.heads.tolist())


def block_model(s, k, w=W_MAX, step=None, searched=None, run_keys=None):
    """One block's walk over protein s (str or bytes). searched(c) -> the earlier runs that chunk
    c's head rule searches (default: all c of them); run_keys: keys searched per run (default w)."""
    res = np.frombuffer(s.encode() if isinstance(s, str) else bytes(s), np.uint8)
    n_win = max(len(res) - k + 1, 0)
    runs = np.zeros(n_win, np.uint64) if n_win > w else None
    heads, bad = [], []
    for c, c0 in enumerate(range(0, n_win, w)):
        nw = min(w, n_win - c0)
        codes = LUT[res[c0:c0 + nw + k - 1]]
        bad.append(bool((codes == 0).any()))
        key = np.full(padded_size(nw), SENTINEL, np.uint64)
        key[:nw] = window_keys(codes, k)
        sort_network(key, step)
        cur = key[:nw]
        head = np.ones(nw, bool)
        head[1:] = cur[1:] != cur[:-1]
        at = np.flatnonzero(head)
        for r in (range(c) if searched is None else searched(c)):
            held = run_holds(runs[r * w:(r + 1) * w], w if run_keys is None else run_keys, cur[at])
            at = at[~held]
        heads.append(cur[at])
        if runs is not None:
            runs[c0:c0 + nw] = cur
    return Block(np.concatenate(heads) if heads else np.zeros(0, np.uint64), runs, bad)


# ---- building blocks of the cases
def draw(rng, letters, n):
    return "".join(letters[i] for i in rng.integers(0, len(letters), int(n)))


def mutated(rng, s, letters, rate):
    out = list(s)
    for i in np.flatnonzero(rng.random(len(s)) < rate):
        out[i] = letters[int(rng.integers(0, len(letters)))]
    return "".join(out)


def n_windows(s, k):
    return max(len(s) - k + 1, 0)


def duplicate_heavy(s, k):
    """At most half as many distinct keys as windows."""
    return 2 * len(kmers(s, k)) <= n_windows(s, k)


class SetsCase:
    """genome and prototype strings, K, the KMA_OPT_HASH_LDS_KEYS values to run under (0: the
    default, 4096) and which proteins are sort-focused (duplicate-heavy by condition)."""

    def __init__(self, name, genome, protos, k, lds_keys, focused=None, **more):
        self.name, self.genome, self.protos, self.k = name, genome, protos, k
        self.lds_keys, self.min_sim = tuple(lds_keys), MIN_SIM
        self.focused = list(range(len(genome))) if focused is None else focused
        for g in self.focused:
            assert duplicate_heavy(genome[g], k), (name, g, n_windows(genome[g], k))
        self.g, self.go = pack(genome)
        self.p, self.po = pack(protos)
        self.__dict__.update(more)

    @functools.cached_property
    def ref(self):
        return set_model(self.genome, self.protos, self.k, self.min_sim)

    @functools.cached_property
    def index(self):
        return {key: at for at, key in enumerate(index_keys(self.protos, self.k))}

    def matches(self, g):
        """Index positions of protein g's distinct keys that the index holds, ascending."""
        return sorted(self.index[v] for v in ref_keys(self.genome[g], self.k) if v in self.index)

    def stats(self):
        return hc.stats_of(self.ref.cand, len(self.protos), hc.CAP_DEFAULT)


def with_prototypes(rng, genome, letters_of, k, unrelated=16):
    """Every protein of at least K residues, or a lightly mutated copy of it when it has 40 or
    more, as a prototype (equal strings once), then unrelated ones over 20 letters."""
    protos = []
    for s, letters in zip(genome, letters_of):
        if len(s) >= k:
            protos.append(mutated(rng, s, letters, 0.03) if len(s) >= 40 else s)
    protos = list(dict.fromkeys(protos))
    return protos + [draw(rng, LETTERS, rng.integers(60, 200)) for _ in range(unrelated)]


# ---- (a) every network size
NETWORK_SIZES = tuple(2 ** p for p in range(1, 13))
NETWORK_K = 2
SMALL_SEEDS = 12                 # proteins per window count below n2 = 128
TAIL_WINDOWS = W_MAX + 2         # its last chunk is the size-2 network, left as a run


def heavy_protein(rng, n_win, k=NETWORK_K):
    """n_win windows over the first a letters, a the largest with a^K <= n_win / 2 plus one (at
    least two), redrawn until at most half the windows are distinct; one letter for n_win <= 3."""
    if n_win <= 3:
        return LETTERS[int(rng.integers(0, 4))] * (n_win + k - 1), LETTERS[:4]
    a = min(max(int((n_win / 2) ** (1 / k)) + 1, 2), len(LETTERS))
    while True:
        s = draw(rng, LETTERS[:a], n_win + k - 1)
        if duplicate_heavy(s, k):
            return s, LETTERS[:a]
        if rng.random() < 0.25 and a > 2:
            a -= 1


@functools.lru_cache(maxsize=None)
def network_case():
    """sizes[n2]: the proteins whose only chunk runs the size-n2 network. n2 = 4: every string of
    five of two letters that meets the condition, and proteins of 3 windows; 8 .. 64: SMALL_SEEDS
    proteins per window count; from 128: one each. A protein of one window has one key and is
    outside the condition; the size-2 network orders two keys whose heads are the same either
    way, so its step shows only in the run it leaves: the last chunk of the 4,098-window protein,
    whose two keys are planted in descending order."""
    rng = np.random.default_rng(20250128)
    genome, letters_of, sizes, focused = [], [], {}, []
    for n2 in NETWORK_SIZES:
        sizes[n2] = []
        counts = sorted({n2, n2 - 1, n2 // 2 + 1}, reverse=True)
        for n_win in counts:
            if n2 == 4 and n_win == 4:
                some = ["".join("AC"[b >> i & 1] for i in range(5)) for b in range(32)]
                some = [(s, "AC") for s in some if duplicate_heavy(s, NETWORK_K)]
            else:
                reps = 1 if n2 >= 128 else (2 if n_win <= 3 else SMALL_SEEDS)
                some = [heavy_protein(rng, n_win) for _ in range(reps)]
            for s, letters in some:
                assert n_windows(s, NETWORK_K) == n_win
                assert n_win == 1 or padded_size(n_win) == n2
                if n_win > 1:
                    focused.append(len(genome))
                sizes[n2].append(len(genome))
                genome.append(s)
                letters_of.append(letters)
    tail, letters = heavy_protein(rng, TAIL_WINDOWS)
    tail = tail[:W_MAX] + "CAA"                      # windows 4096, 4097: "CA" then "AA"
    assert n_windows(tail, NETWORK_K) == TAIL_WINDOWS
    focused.append(len(genome))
    genome.append(tail)
    letters_of.append(letters)
    protos = with_prototypes(rng, genome, letters_of, NETWORK_K)
    return SetsCase("network", genome, protos, NETWORK_K, (0,), focused, sizes=sizes,
                    tail=len(genome) - 1)


# ---- (b), (c), (d) proteins of several runs
def code_of(ch):
    return 27 if ch == "*" else ord(ch) - 64


def runs_protein(rng, letters, k, w, n_win):
    """n_win windows (more than w). A base of period w / 4 + 4 over `letters`, so that every run
    holds the keys of run 0 again; then single windows are overwritten with marker K-mers that
    the base does not hold. X, the top letter K times (the largest key there is), at window 5 of
    run 0 and once in run 2 (run 1 for a protein of two runs): in runs 0 and 2 only, and the last
    key of run 0. With four chunks V sits once in run 2 and once in the partial run, and with a
    partial last run Y sits there alone. Copies of a marker lie a multiple of the period apart:
    the windows that overlap them are equal too, which keeps the protein duplicate-heavy.
    Returns (protein, {marker name: K-mer})."""
    period = w // 4 + 4
    length = n_win + k - 1
    top = max(letters, key=code_of)
    while True:
        unit = draw(rng, letters, period)
        base = (unit * (length // period + 2))[:length]
        have = kmers(base, k)
        # (X is planted at windows 5 + i * period: its neighbours there must not extend it)
        if top * k not in have and top not in (unit[4 % period], unit[(5 + k) % period]):
            break
    s = list(base)
    marks = {"X": top * k}

    def absent():
        while True:
            m = draw(rng, letters, k)
            if m not in have and m not in marks.values():
                return m

    def plant(m, at):
        assert 0 <= at and at + k <= length
        s[at:at + k] = m

    def back_into(run, at):
        """The window a multiple of the period before `at` that lies in `run`."""
        while at >= (run + 1) * w:
            at -= period
        assert at >= run * w
        return at

    n_runs = -(-n_win // w)
    last0 = (n_runs - 1) * w
    partial = n_win - last0 < w
    again = 2 if n_runs >= 3 else 1
    at = 5
    while at < again * w:
        at += period
    assert at < min((again + 1) * w, n_win)
    plant(marks["X"], 5)
    plant(marks["X"], at)
    if n_runs >= 4 and partial:
        marks["V"] = absent()
        plant(marks["V"], last0 + 1)
        plant(marks["V"], back_into(2, last0 + 1))
    if partial and n_win - last0 >= 17:
        marks["Y"] = absent()
        plant(marks["Y"], last0 + 14)
    return "".join(s), marks


def run_sets(s, k, w):
    """The key sets of the protein's runs (as substrings)."""
    n = n_windows(s, k)
    return [{s[i:i + k] for i in range(c0, min(c0 + w, n))} for c0 in range(0, n, w)]


def assert_run_properties(s, k, w, marks):
    """What the run-rule variants are seen by; asserted, not measured."""
    runs = run_sets(s, k, w)
    x = marks["X"]
    assert len(runs) >= 2 and runs[0] & runs[1] and duplicate_heavy(s, k)
    assert x in runs[0] and key_of(x) == max(key_of(m) for m in runs[0])
    assert sum(s[i:i + k] == x for i in range(w)) == 1        # once in run 0: its last key
    if len(runs) >= 3:
        assert runs[0] & runs[1] & runs[2]
        assert x in runs[2] and x not in runs[1] and (runs[0] & runs[2]) - runs[1]
    else:
        assert x in runs[1]
    if "V" in marks:
        assert marks["V"] in (runs[2] & runs[3]) - runs[0] - runs[1]
    if "Y" in marks:
        assert marks["Y"] in runs[-1] and not any(marks["Y"] in r for r in runs[:-1])


EVERY_W = (64, 128, 256, 512, 1024, 2048)
W_CASE_K = 3
W_CASE_LETTERS = "ACDEFGHIKLMW"


def word_twins(rng, letters, k):
    """For K >= 7: a + u + b + u three times over, u of K + 2 letters, a and b two letters whose
    codes as a key's first residue agree below bit 32. The windows at a and at b are keys that
    differ in the high word alone; period 2K + 6, so duplicate-heavy."""
    shift = 5 * (k - 1)
    a, b = next((a, b) for a in letters for b in letters if a < b and
                ((code_of(a) ^ code_of(b)) << shift) & 0xFFFFFFFF == 0)
    u = draw(rng, letters, k + 2)
    return (a + u + b + u) * 3


def runs_case(name, seed, k, letters, shapes, lds_keys, twins=False):
    """shapes: (w, n_win) per protein; runs_of[g] = (w, markers) of protein g (None: no such
    protein)."""
    rng = np.random.default_rng(seed)
    genome, runs_of = [], []
    for w, n_win in shapes:
        s, marks = runs_protein(rng, letters, k, w, n_win)
        assert_run_properties(s, k, w, marks)
        genome.append(s)
        runs_of.append((w, marks))
    if twins:
        genome.append(word_twins(rng, letters, k))
        runs_of.append(None)
    protos = with_prototypes(rng, genome, [letters] * len(genome), k, unrelated=8)
    protos += [draw(rng, letters, 150) for _ in range(4)]
    return SetsCase(name, genome, protos, k, lds_keys, runs_of=runs_of)


@functools.lru_cache(maxsize=None)
def every_w_case():
    shapes = [(w, n) for w in EVERY_W for n in (3 * w + 17, 2 * w)]
    return runs_case("every W", 64, W_CASE_K, W_CASE_LETTERS, shapes, EVERY_W)


@functools.lru_cache(maxsize=None)
def default_w_case():
    """2 * 4096 + 41 windows (three chunks) and 3 * 4096 + 17 (four: only there can a head rule
    that searches the first two runs alone be seen)."""
    shapes = [(W_MAX, 2 * W_MAX + 41), (W_MAX, 3 * W_MAX + 17)]
    return runs_case("default W", 4096, W_CASE_K, W_CASE_LETTERS, shapes, (0,))


EVERY_K = tuple(range(2, 13))
K_CASE_LETTERS = {2: "ACDEFGHI", 3: "ACDEFG", 4: "ACDE", 5: "ACDE", 6: "ACD", 7: "BZ*", 8: "Z*",
                  9: "MZ*", 10: "Z*", 11: "AZ*", 12: "Z*"}


@functools.lru_cache(maxsize=None)
def every_k_case(k):
    """3 * 64 + 17 and 2 * 64 windows at W = 64. From K = 7 the keys pass 32 bits and the letters
    are codes 26 and 27 (and 1, 2 or 13): keys differ in the high word alone (word_twins), the low
    word alone, or both; K = 12 reaches bit 59."""
    letters = K_CASE_LETTERS[k]
    assert k < 7 or ("Z" in letters and "*" in letters and len(letters) <= 3)
    return runs_case(f"K = {k}", 1200 + k, k, letters, [(64, 3 * 64 + 17), (64, 2 * 64)], (64,),
                     twins=k >= 7)


# ---- (e) more than 2^20 proteins
SCALE_N = GRID + 517
SCALE_K, SCALE_W = 3, 64
SCALE_POOL = 1024
SCALE_LETTERS = "ACD"
SCALE_BLOCKS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 31, 63, 64, 65, 127, 128, 200, 255, 256, 257, 300, 384,
                400, 448, 500, 511, 512, 513, 514, 515, 516)
SCALE_PAIRS = (("three_run", "short"), ("short", "three_run"), ("empty", "three_run"),
               ("three_run", "empty"), ("k_minus_1", "three_run"), ("three_run", "k_minus_1"),
               ("short", "k_minus_1"), ("k_minus_1", "short"), ("heavy_a", "heavy_b"),
               ("three_run", "three_run_b"))
SCALE_SAMPLE = 2000


class ScaleCase:
    """The genome is items[idx[g]]: a pool of 1,024 proteins of at most 40 residues over three
    letters (a tenth empty or of K - 1 residues) and the crafted ones; the set model runs once
    per item. Crafted: two proteins of 3 * 64 + 17 windows (runs_protein), `short` (12 residues),
    the empty protein, one of K - 1 residues, and two of 60 and 50 windows over two letters.
    Blocks SCALE_BLOCKS take the pairs SCALE_PAIRS in turn as proteins (g, g + 2^20)."""

    def __init__(self):
        rng = np.random.default_rng(517)
        k, w = SCALE_K, SCALE_W
        three, self.marks = runs_protein(rng, W_CASE_LETTERS, k, w, 3 * w + 17)
        three_b, marks_b = runs_protein(rng, W_CASE_LETTERS, k, w, 3 * w + 17)
        assert_run_properties(three, k, w, self.marks)
        assert_run_properties(three_b, k, w, marks_b)
        self.crafted = {"three_run": three, "three_run_b": three_b,
                        "short": draw(rng, SCALE_LETTERS, 12), "empty": "",
                        "k_minus_1": draw(rng, SCALE_LETTERS, k - 1),
                        "heavy_a": draw(rng, "AC", 60 + k - 1),
                        "heavy_b": draw(rng, "CD", 50 + k - 1)}
        for name in ("three_run", "three_run_b", "heavy_a", "heavy_b"):
            assert duplicate_heavy(self.crafted[name], k)
        seeds = [draw(rng, SCALE_LETTERS, 40) for _ in range(6)]
        pool = []
        for i in range(SCALE_POOL):
            kind = i % 20
            if kind == 0:
                s = ""
            elif kind == 1:
                s = draw(rng, SCALE_LETTERS, k - 1)
            elif kind < 12:
                src = seeds[int(rng.integers(0, 6))]
                n = int(rng.integers(k, 41))
                at = int(rng.integers(0, 40 - n + 1))
                s = src[at:at + n]
            else:
                s = draw(rng, SCALE_LETTERS[:2 + i % 2], rng.integers(k, 41))
            pool.append(s)
        self.protos = seeds + [mutated(rng, three, W_CASE_LETTERS, 0.03), self.crafted["heavy_a"],
                               mutated(rng, three_b, W_CASE_LETTERS, 0.05)]
        self.protos += [draw(rng, LETTERS, 120) for _ in range(6)]
        self.items = pool + list(self.crafted.values())
        self.item_of = {name: SCALE_POOL + i for i, name in enumerate(self.crafted)}
        idx = rng.integers(0, SCALE_POOL, SCALE_N)
        self.pairs = []
        for n, g in enumerate(SCALE_BLOCKS):
            pair = SCALE_PAIRS[n % len(SCALE_PAIRS)]
            idx[g], idx[g + GRID] = self.item_of[pair[0]], self.item_of[pair[1]]
            self.pairs.append((g, pair))
        self.idx = idx
        self.k, self.min_sim, self.lds_keys = k, MIN_SIM, (w,)
        self.ref = set_model(self.items, self.protos, k, MIN_SIM)
        self.index = {key: at for at, key in enumerate(index_keys(self.protos, k))}
        self.item_size = np.array([len(kmers(s, k)) for s in self.items], np.uint32)
        self.p, self.po = pack(self.protos)
        ibytes, ioff = pack(self.items)
        lens = np.diff(ioff.astype(np.int64))[idx]
        self.go = np.zeros(SCALE_N + 1, np.uint64)
        self.go[1:] = np.cumsum(lens)
        total = int(self.go[-1])
        within = np.arange(total, dtype=np.int64) - np.repeat(self.go[:-1].astype(np.int64), lens)
        self.g = np.zeros(total + 32, np.uint8)
        self.g[:total] = ibytes[np.repeat(ioff[:-1].astype(np.int64)[idx], lens) + within]

    def protein(self, g):
        return self.g[int(self.go[g]):int(self.go[g + 1])].tobytes().decode()

    def matches_of_item(self, i):
        return sorted(self.index[v] for v in ref_keys(self.items[i], self.k) if v in self.index)

    def expected(self):
        """(best, sim, count, stats[0..2]) of the whole call."""
        mult = np.bincount(self.idx, minlength=len(self.items))
        count = np.zeros(len(self.protos), np.int64)
        for i, ok in enumerate(self.ref.passed):
            count[ok] += mult[i]
        st = hc.stats_of(self.ref.cand, len(self.protos), hc.CAP_DEFAULT, mult.tolist())
        return self.ref.best[self.idx], self.ref.sim[self.idx], count.astype(np.uint32), st

    def checked(self):
        """The proteins looked at one by one: every second protein of a block, its first, and a
        seeded sample of the others."""
        second = np.arange(GRID, SCALE_N)
        sample = np.random.default_rng(2000).choice(GRID, SCALE_SAMPLE, replace=False)
        return np.unique(np.concatenate([second, second - GRID, sample]))


@functools.lru_cache(maxsize=None)
def scale_case():
    return ScaleCase()


# ---- (f) a byte without a code
FLAG_K, FLAG_W = 4, 64
FLAG_BYTE = ord("k")


class FlagCase:
    """A genome of five proteins at K = 4; protein 2 has 3 * 64 + 17 windows (four chunks at
    W = 64, one at the default W). variants: (name, residues, lo, hi, flagged) - the call is on
    proteins lo .. hi of the offsets; one byte of the clean residues is replaced per variant."""

    def __init__(self):
        rng = np.random.default_rng(404)
        k, w = FLAG_K, FLAG_W
        long_one, _ = runs_protein(rng, "ACDEFW", k, w, 3 * w + 17)
        self.genome = [draw(rng, "ACDE", 30), draw(rng, "ACDE", 25), long_one,
                       draw(rng, "ACDE", 50), draw(rng, "ACDE", 21)]
        self.protos = [mutated(rng, long_one, "ACDEFW", 0.03), self.genome[3]]
        self.protos += [draw(rng, LETTERS, 100) for _ in range(6)]
        self.k, self.lds_keys, self.min_sim = k, (w, 0), MIN_SIM
        self.g, self.go = pack(self.genome)
        self.p, self.po = pack(self.protos)
        lo, hi = int(self.go[2]), int(self.go[3])
        spots = [("first byte", lo), ("last byte", hi - 1), ("chunk 2", lo + 2 * w + 30)]
        spots += [(f"shared by chunks 0 and 1, byte {i}", lo + w + i) for i in range(k - 1)]
        self.variants = [(name, self.with_byte(at), 0, 5, True) for name, at in spots]
        # a view of proteins 1 .. 3: the bytes next to it belong to proteins 0 and 4
        self.variants += [("before the view", self.with_byte(int(self.go[1]) - 1), 1, 4, False),
                          ("after the view", self.with_byte(int(self.go[4])), 1, 4, False)]
        self.long_at = (lo, hi)

    def with_byte(self, at):
        res = self.g.copy()
        res[at] = FLAG_BYTE
        return res


@functools.lru_cache(maxsize=None)
def flag_case():
    return FlagCase()


# ---- a captured call replayed on a second genome
@functools.lru_cache(maxsize=None)
def graph_cases():
    """Two duplicate-heavy genomes of equal offsets against the same prototypes, at W = 64:
    3W + 17 and 2W windows (runs_protein), and 50 and 64 windows over two letters."""
    rng = np.random.default_rng(2323)
    k, w, letters = W_CASE_K, 64, W_CASE_LETTERS
    genomes = []
    for _ in range(2):
        genome = [runs_protein(rng, letters, k, w, n)[0] for n in (3 * w + 17, 2 * w)]
        genomes.append(genome + [draw(rng, "AC", 50 + k - 1), draw(rng, "AC", 64 + k - 1)])
    protos = with_prototypes(rng, genomes[0][:2] + genomes[1], [letters] * 6, k, unrelated=6)
    first, second = (SetsCase(f"graph {i}", g, protos, k, (w,)) for i, g in enumerate(genomes))
    assert first.go.tolist() == second.go.tolist() and first.genome != second.genome
    return first, second


def all_sets_cases():
    return [network_case(), every_w_case(), default_w_case()] + [every_k_case(k) for k in EVERY_K]
