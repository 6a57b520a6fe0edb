"""Cases for the resident prototype index's score kernel under load (csrc/kma_hashindex.hip,
index_score_kernel), with a plain Python set model as their reference.
tests/test_hashindex_workload.py shows on the CPU that they aim where they claim;
tests/test_gpu_hashindex_load.py runs them.

 (a) bounds_case():   candidate counts of exactly N for N on both sides of CAP 512, 1024 and 2048,
                      holders scattered over 20,000 prototype ids, ties across ranges, and one
                      5,000-residue copy whose postings all land in one slot.
 (b) cluster_case():  holders chosen by id so that their first slots are the table's last few:
                      one probe chain of more than 256 slots that passes from slot T - 1 to 0.
 (c) scale_case():    2^20 + 517 genome proteins, so that blocks score a second protein; pairs
                      (g, g + 2^20) crafted to differ in everything a block keeps.
 (d) threshold_case() and disjoint_keys_case().

The set model: distinct K-mers per protein, sim = c / (|P| + |G| - c) as one double division
(Python's int / int is correctly rounded, as is the kernel's division of two exact doubles), a
proposal needs sim >= min_sim and strictly above the current one (earlier prototypes win ties),
out_count per prototype; and out_stats for a CAP from the sorted candidate ids of each protein."""
import bisect
import functools
import struct

import numpy as np

AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
K = 8
BLOCK = 256                 # kHashBlock
GRID = 1 << 20              # launch_index_score's grid cap
CAP_DEFAULT, CAP_MAX = 1024, 2048


# ---- mirrors of csrc/kma_hashindex.h (held to the header by the host check program's --hash)
def hash_table_slots(cap):
    need = max(2 * cap, cap + 2 * BLOCK)
    t = 64
    while t < need:
        t <<= 1
    return t


def hash_bits(cap):
    return hash_table_slots(cap).bit_length() - 1


def hash_slot(proto, bits):
    return ((int(proto) * 0x9E3779B1) & 0xFFFFFFFF) >> (32 - bits)


def hash_slots_of(ids, bits):
    ids = np.asarray(ids, np.uint64)
    return ((ids * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - bits)


def occupied_slots(ids, cap):
    """Slots taken when `ids` are inserted by linear probing (without the CAP guard the set of
    slots does not depend on the order), and the run of taken slots that holds slot T - 1: its
    length and whether it goes on from T - 1 into slot 0."""
    bits = hash_bits(cap)
    T = 1 << bits
    taken = np.zeros(T, bool)
    for p in ids:
        h = hash_slot(p, bits)
        while taken[h]:
            h = (h + 1) & (T - 1)
        taken[h] = True
    assert not taken.all()
    if not taken[T - 1]:
        return taken, 0, False
    lo = T - 1
    while taken[lo - 1]:
        lo -= 1
    hi = 0
    while taken[hi]:
        hi += 1
    return taken, T - lo + hi, hi > 0


# ---- the set model
def rand(rng, n):
    return AA[rng.integers(0, 20, int(n))].tobytes().decode()


def kmers(s, k=K):
    return {s[i:i + k] for i in range(len(s) - k + 1)}


class Ref:
    """best, sim, count as the calls return them; per genome protein its sorted candidate ids
    (prototypes sharing a K-mer), the ids at or above min_sim, and the count shared with best."""

    def __init__(self, best, sim, count, cand, passed, shared):
        self.best, self.sim, self.count = best, sim, count
        self.cand, self.passed, self.shared = cand, passed, shared


def set_model(genome, protos, k, min_sim):
    gsets = [kmers(s, k) for s in genome]
    wanted = set().union(*gsets) if gsets else set()
    psize = [0] * len(protos)
    holders = {}
    for p, s in enumerate(protos):
        if len(s) < k:
            continue
        ks = kmers(s, k)
        psize[p] = len(ks)
        for kmer in ks & wanted:
            holders.setdefault(kmer, []).append(p)
    best = np.full(len(genome), -1, np.int32)
    sim = np.zeros(len(genome), np.float64)
    count = np.zeros(len(protos), np.uint32)
    cand, passed, shared_best = [], [], []
    for g, gs in enumerate(gsets):
        shared = {}
        for kmer in gs:
            for p in holders.get(kmer, ()):
                shared[p] = shared.get(p, 0) + 1
        ids = sorted(shared)
        b, b_sim, b_shared, ok = -1, 0.0, 0, []
        for p in ids:                       # file order: a later equal similarity does not win
            c = shared[p]
            s = c / (psize[p] + len(gs) - c)
            if s >= min_sim:
                ok.append(p)
                if b < 0 or s > b_sim:
                    b, b_sim, b_shared = p, s, c
        best[g], sim[g] = b, b_sim
        count[ok] += 1
        cand.append(ids)
        passed.append(ok)
        shared_best.append(b_shared)
    return Ref(best, sim, count, cand, passed, shared_best)


def ranges_scored(ids, n_proto, cap):
    """HashRangeStack's walk over the sorted candidate ids: a range of more than CAP candidates
    is replaced by its halves, one of 1..CAP counts once, an empty one counts nothing."""
    stack, n = [(0, n_proto)], 0
    while stack:
        lo, hi = stack.pop()
        c = bisect.bisect_left(ids, hi) - bisect.bisect_left(ids, lo)
        if c > cap:
            mid = lo + ((hi - lo) >> 1)
            stack += [(mid, hi), (lo, mid)]
        elif c:
            n += 1
    return n


def stats_of(cand, n_proto, cap, mult=None):
    """out_stats of a call at this CAP; mult: how often each protein occurs in the call."""
    mult = [1] * len(cand) if mult is None else mult
    st = [0, 0, 0]
    for ids, m in zip(cand, mult):
        if m and ids:
            st[0] += m
            st[1] += m * (len(ids) > cap)
            st[2] += m * ranges_scored(ids, n_proto, cap)
    return st


def with_tail(rng, core, cand_sets, min_sim):
    """core + a random tail of the length at which the share of the candidates (the K-mer sets
    sharing with core) at or above min_sim is nearest to a half."""
    ck = kmers(core)
    c = np.array([len(ck & s) for s in cand_sets], np.float64)
    ps = np.array([len(s) for s in cand_sets], np.float64)[c > 0]
    c = c[c > 0]
    t = min(range(0, 6000, 4),
            key=lambda t: abs(float(np.mean(c / (ps + len(ck) + t - c) >= min_sim)) - 0.5))
    return core + rand(rng, t)


def pack(strs):
    """kmeranno.pack_strings: (uint8 residues padded by 32 bytes, uint64 offsets)."""
    bs = [s.encode() for s in strs]
    off = np.zeros(len(bs) + 1, np.uint64)
    off[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
    return np.frombuffer(b"".join(bs) + b"\0" * 32, np.uint8).copy(), off


class Case:
    def __init__(self, genome, protos, min_sim, **more):
        self.genome, self.protos, self.min_sim = genome, protos, min_sim
        self.g, self.go = pack(genome)
        self.p, self.po = pack(protos)
        self.ref = set_model(genome, protos, K, min_sim)
        self.__dict__.update(more)

    def stats(self, cap):
        return stats_of(self.ref.cand, len(self.protos), cap or CAP_DEFAULT)


# ---- (a) candidate counts at the CAP bounds
BOUND_N = (511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 2600)
BOUND_CAPS = (512, 0, 2048)          # option values; 0 is the default, 1024
BOUND_PROTOS, BOUND_HOLDERS = 20_000, 2_600
BOUND_MIN_SIM = 0.0125


@functools.lru_cache(maxsize=None)
def bounds_case():
    """Holder number i (at prototype id ids[i], a fixed permutation) carries motif j iff
    i < BOUND_N[j], cut by 0..4 residues so that shared counts differ; genome protein j carries
    motif j alone and has exactly BOUND_N[j] candidates. Duplicates: holders 2100 and 2500 are
    both motif 9 with six more residues of protein 9 and nothing else, the best of protein 9 (2,600 candidates: it splits at every
    CAP), at ids in different halves of the id range; holders 3, 77 and 400 are one string.
    Protein 10 is a copy of a 5,000-residue prototype that shares with nothing else."""
    rng = np.random.default_rng(20240616)
    ids = rng.permutation(BOUND_PROTOS)[:BOUND_HOLDERS].tolist()
    motifs = [rand(rng, 14 + 3 * j) for j in range(len(BOUND_N))]
    protos = [rand(rng, rng.integers(0, 90)) for _ in range(BOUND_PROTOS)]
    for i, p in enumerate(ids):
        parts = [m[:len(m) - (i * 7 + j) % 5] for j, m in enumerate(motifs) if i < BOUND_N[j]]
        protos[p] = "".join(parts) + rand(rng, rng.integers(0, 200))
    half = BOUND_PROTOS // 2
    champs = (2100, next(i for i in range(2500, BOUND_HOLDERS)
                         if (ids[i] < half) != (ids[2100] < half)))
    core9 = motifs[9] + rand(rng, 6)    # (other holders share at most a residue or two of it)
    for i in champs:
        protos[ids[i]] = core9
    protos[ids[77]] = protos[ids[400]] = protos[ids[3]]
    held = set(ids)
    long_id = next(p for p in range(BOUND_PROTOS // 3, BOUND_PROTOS) if p not in held)
    protos[long_id] = rand(rng, 5000)
    hsets = [kmers(protos[p]) for p in ids]
    genome = [with_tail(rng, m, hsets, BOUND_MIN_SIM) for m in motifs[:9] + [core9]]
    genome += [protos[long_id], "", rand(rng, 300)]
    return Case(genome, protos, BOUND_MIN_SIM, ids=ids, champs=champs, long_id=long_id)


# ---- (b) one probe chain across the end of the table
# CAP: (the last slots of the table the holders start in, holders, holders per genome protein)
CLUSTER = {256: (8, 330, (330, 257, 256, 150, 200)),
           1024: (16, 1100, (1100, 1025, 1024, 600, 800)),
           2048: (16, 2100, (2100, 2049, 2048, 1100, 1500))}
CLUSTER_MIN_SIM = 0.0125


def cluster_ids(cap):
    """The smallest prototype ids whose first slot is one of the table's last few."""
    last, count, _ = CLUSTER[cap]
    bits = hash_bits(cap)
    ids = np.arange(count * (1 << bits) // last * 2, dtype=np.uint64)
    ids = ids[hash_slots_of(ids, bits) >= (1 << bits) - last]
    assert len(ids) >= count
    return ids[:count].astype(np.int64).tolist()


@functools.lru_cache(maxsize=None)
def cluster_case(cap):
    """Genome protein q carries motif q, held by sizes[q] of the holders (q = 0: all of them,
    more than CAP; then CAP + 1, CAP, and two counts between CAP / 2 and CAP; the first ranks for
    q = 3, random ranks otherwise); protein 5 carries motifs 0 and 3. Every other prototype is
    empty or shorter than K."""
    rng = np.random.default_rng(1000 + cap)
    _, count, sizes = CLUSTER[cap]
    hold = cluster_ids(cap)
    n_proto = hold[-1] + 4
    motifs = [rand(rng, 18 + 2 * q) for q in range(len(sizes))]
    twin = sizes[3] - 1          # holds what holder 0 holds: made its copy below
    others = np.array([r for r in range(count) if r not in (0, twin)])
    member = []
    for q, n in enumerate(sizes):
        ranks = range(n) if q in (0, 3) else [0, twin] + rng.choice(others, n - 2,
                                                                    replace=False).tolist()
        member.append(set(int(r) for r in ranks))
        assert len(member[q]) == n
    protos = ["ACDEFGH"[:p % 8] if p % 89 == 5 else "" for p in range(n_proto)]
    for r, p in enumerate(hold):
        parts = [m[:len(m) - (r * 3 + q) % 4] for q, m in enumerate(motifs) if r in member[q]]
        protos[p] = "".join(parts) + rand(rng, rng.integers(0, 30))
    protos[hold[twin]] = protos[hold[0]]                    # an equal pair far apart in id
    hsets = [kmers(protos[p]) for p in hold]
    genome = [with_tail(rng, m, hsets, CLUSTER_MIN_SIM) for m in motifs]
    genome += [with_tail(rng, motifs[0] + "W" + motifs[3], hsets, CLUSTER_MIN_SIM), "",
               rand(rng, 200)]
    return Case(genome, protos, CLUSTER_MIN_SIM, hold=hold, sizes=sizes, cap=cap)


def kmer_key(kmer):
    v = 0
    for ch in kmer.encode():
        v = v << 5 | (ch - 64)
    return v


def write_check_case(path, case, cap):
    """The case as host/hashindex_check.cpp reads it: key lists and the set model's answers."""
    with open(path, "wb") as f:
        f.write(struct.pack("<IIIId", len(case.protos), len(case.genome), cap, 0, case.min_sim))
        for s in case.protos + case.genome:
            keys = [kmer_key(s[i:i + K]) for i in range(len(s) - K + 1)]   # repeats kept
            f.write(struct.pack("<I", len(keys)) + np.asarray(keys, np.uint64).tobytes())
        for g in range(len(case.genome)):
            f.write(struct.pack("<iII", int(case.ref.best[g]), case.ref.shared[g],
                                len(case.ref.cand[g])))


# ---- (c) more than 2^20 genome proteins in one call
SCALE_N = GRID + 517
SCALE_SIZES = (GRID, GRID + 1, SCALE_N)
SCALE_LOW_CAP = 128
SCALE_MIN_SIM = 0.08
SCALE_POOL = 4096
# Blocks g whose two proteins (g, g + 2^20) are crafted, and what they are, in turn.
SCALE_BLOCKS = (0, 1, 2, 3, 4, 5, 6, 7, 31, 32, 63, 64, 65, 127, 128, 129, 200, 255, 256, 257,
                300, 301, 302, 303, 384, 400, 411, 448, 449, 450, 500, 509, 510, 511, 512, 513,
                514, 515, 516)
SCALE_PAIRS = (("strong_many", "none"), ("none", "strong_many"), ("strong_many", "second_best"),
               ("second_best", "strong_many"), ("crowd", None), ("none", "crowd"),
               ("few", "crowd"), ("crowd", "few"), (None, "strong_many"), ("second_best", "none"))


class ScaleCase:
    """The genome is items[idx[g]]: a pool of 4,096 tiny proteins and the crafted ones, so the
    set model runs once per item and a call's answers follow from idx.

    Prototypes: 12 short ones (4 seeds of 20 residues, each exact and with one residue changed at
    position 8 or 13, all followed by one hub K-mer, which so occurs in a dozen prototypes); the
    strong prototype S1 (180 residues, and a copy of it as the last prototype); 300 crowd
    prototypes that carry motif A, the first 100 of them also motif B; S2 (220 residues) in their
    middle. Pool: ~10% empty or shorter than K, the rest 8 to 10 residues cut from the short
    prototypes, the hub, strings that occur in no prototype, and mixtures.
    Crafted: strong_many = S1 + motif A (best S1 at 0.78, 302 candidates: splits at CAP 128),
    second_best = 150 residues of S2 + motif B (101 candidates: does not split), crowd = motif A
    alone (300), few = motif B alone (100), none = 150 random residues."""

    def __init__(self):
        rng = np.random.default_rng(77)
        seeds = [rand(rng, 20) for _ in range(4)]
        hub = rand(rng, K)
        short = []
        for p in range(12):
            s, pos = seeds[p % 4], (None, 8, 13)[p // 4]
            if pos is not None:
                s = s[:pos] + ("W" if s[pos] != "W" else "Y") + s[pos + 1:]
            short.append(s + hub)
        s1, s2 = rand(rng, 180), rand(rng, 220)
        mot_a, mot_b = rand(rng, 16), rand(rng, 16)
        crowd = [mot_a[:16 - r % 3] + (mot_b[:16 - r % 2] if r < 100 else "") +
                 rand(rng, rng.integers(0, 13)) for r in range(300)]
        self.protos = short + [s1] + crowd[:150] + [s2] + crowd[150:] + [s1]
        self.s1_id, self.s2_id = 12, 12 + 1 + 150
        misses = [rand(rng, 10) for _ in range(64)]
        pool = []
        for i in range(SCALE_POOL):
            kind, n = i % 10, int(rng.integers(8, 11))
            src = short[int(rng.integers(0, 12))]
            at = int(rng.integers(0, len(src) - n + 1))
            if kind == 0:
                s = rand(rng, rng.integers(1, K)) if i % 20 else ""
            elif kind <= 5:
                s = src[at:at + n]
            elif kind == 6:
                s = hub + rand(rng, n - K)
            elif kind == 7:
                s = src[at:at + n - 1] + rand(rng, 1)
            else:
                s = misses[int(rng.integers(0, 64))][:n]
            pool.append(s)
        self.crafted = {"strong_many": s1 + mot_a + rand(rng, 30), "none": rand(rng, 150),
                        "second_best": s2[40:190] + mot_b + rand(rng, 20),
                        "crowd": mot_a + rand(rng, 40), "few": mot_b + rand(rng, 25)}
        self.items = pool + list(self.crafted.values())
        self.item_of = {name: SCALE_POOL + i for i, name in enumerate(self.crafted)}
        idx = rng.integers(0, SCALE_POOL, SCALE_N)
        for n, g in enumerate(SCALE_BLOCKS):
            for g2, name in zip((g, g + GRID), SCALE_PAIRS[n % len(SCALE_PAIRS)]):
                if name is not None:
                    idx[g2] = self.item_of[name]
        self.idx = idx
        self.min_sim = SCALE_MIN_SIM
        self.ref = set_model(self.items, self.protos, K, SCALE_MIN_SIM)
        self.p, self.po = pack(self.protos)
        # the genome's residues: item bytes gathered by idx
        ibytes, ioff = pack(self.items)
        ilen = np.diff(ioff.astype(np.int64))
        lens = ilen[idx]
        self.go = np.zeros(SCALE_N + 1, np.uint64)
        self.go[1:] = np.cumsum(lens)
        total = int(self.go[-1])
        within = np.arange(total, dtype=np.int64) - np.repeat(self.go[:-1].astype(np.int64), lens)
        self.g = np.zeros(total + 32, np.uint8)
        self.g[:total] = ibytes[np.repeat(ioff[:-1].astype(np.int64)[idx], lens) + within]

    def genome(self, n):
        """The call of the first n proteins: a view of the residues, and n + 1 offsets."""
        return self.g[:int(self.go[n]) + 32], self.go[:n + 1]

    def protein(self, g):
        return self.g[int(self.go[g]):int(self.go[g + 1])].tobytes().decode()

    def expected(self, n, cap=0):
        """(best, sim, count, stats) of the first n proteins at this CAP option."""
        idx = self.idx[:n]
        mult = np.bincount(idx, minlength=len(self.items))
        count = np.zeros(len(self.protos), np.int64)
        for i, ok in enumerate(self.ref.passed):
            count[ok] += mult[i]
        st = stats_of(self.ref.cand, len(self.protos), cap or CAP_DEFAULT, mult.tolist())
        return self.ref.best[idx], self.ref.sim[idx], count.astype(np.uint32), st


@functools.lru_cache(maxsize=None)
def scale_case():
    return ScaleCase()


# ---- (d) the threshold itself; an index wholly above or below the genome's keys
THRESHOLD = 0.0125


@functools.lru_cache(maxsize=None)
def threshold_case():
    """One prototype of 40 distinct K-mers and one protein of 41 that share exactly the first:
    sim = 1 / 80, the double 0.0125."""
    rng = np.random.default_rng(5)
    proto = rand(rng, 47)
    return [proto[:K] + rand(rng, 40)], [proto]


def disjoint_keys_case(index_above):
    """Keys order by their first residues: prototypes over TVWY and proteins over ACDE (or the
    reverse) put every unique key of the index above (below) every genome key."""
    rng = np.random.default_rng(6)
    low = ["".join(rng.choice(list("ACDE"), 60)) for _ in range(40)]
    high = ["".join(rng.choice(list("TVWY"), 60)) for _ in range(40)]
    return (low, high) if index_above else (high, low)
