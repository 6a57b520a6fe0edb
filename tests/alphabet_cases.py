"""Workloads over the whole 5-bit residue field, shared by tests/test_alphabet_workload.py (CPU,
the oracle alone) and tests/test_gpu_alphabet.py.

A packed key is built from 5-bit residue codes: 'A'..'Z' -> 1..26, '*' -> 27, up to four other
bytes of a table's K-length rows -> 28..31 in byte order, 0 for a byte without a code. The other
GPU workloads draw from the twenty letters ACDEFGHIKLMNPQRSTVWY; the ones here use all 27
standard symbols and, with `extra`, the four bytes of EXTRA, so that codes 26..31 (and the
all-ones code 31, a byte >= 128) reach every kernel at the scale of a few thousand rows and
1,500 proteins. Rows and proteins are bytes, never str.
"""
import functools
import types

import numpy as np

STD = b"ABCDEFGHIJKLMNOPQRSTUVWXYZ*"   # codes 1..27
EXTRA = b"-1a\xc3"                     # codes 28..31 in byte order: '-', '1', 'a', 0xC3
NOISE = b" 7q\x00\xff@["               # bytes that never have a code
RARE = b"BJOUXZ*"                      # standard symbols the 20-letter workloads never hold
KS = (5, 7, 8)
MIN_HITS = 5
N_REGULAR = 24                         # roles 1..24 of random rows; 25..27 hold the special rows
ROWS_PER_ROLE = 150
FID_TOP, FID_TIE, FID_LAST = N_REGULAR + 1, N_REGULAR + 2, N_REGULAR + 3
N_FID = FID_LAST + 1                   # fid 0 belongs to one row that no protein contains
ZERO_LOW_R = b"DHLPTX"                 # codes 4, 8, .., 24: (code << 30) has a zero low dword


def code_of(extra):
    """The byte -> code table (numpy, 256 entries) of a table with or without the EXTRA symbols."""
    lut = np.zeros(256, np.uint8)
    for i, c in enumerate(STD):
        lut[c] = i + 1
    if extra:
        for i, c in enumerate(EXTRA):
            lut[c] = 28 + i
    return lut


def _alphabet(extra):
    return STD + (EXTRA if extra else b"")


def _high(extra):
    """The symbols of codes 26..31 that this table has."""
    return b"Z*" + (EXTRA if extra else b"")


def _top(extra):
    """The symbol of the largest code: 0xC3 (31) with the extra symbols, '*' (27) without."""
    return EXTRA[3:] if extra else b"*"


def _draw(rng, symbols, weights, n, k):
    a = np.frombuffer(symbols, np.uint8)
    p = np.asarray(weights, np.float64)
    return [r.tobytes() for r in a[rng.choice(len(a), (n, k), p=p / p.sum())]]


def special_rows(k, extra):
    """The hand-made rows by role: keys at the top of the residue field, the mod-sampling ties
    and the largest code in the last position."""
    top = _top(extra)
    tops = [b"Z" * k, b"*" * k, top + b"A" * (k - 1)]
    if extra:
        tops.append(top * k)  # the key 2^(5K) - 1
    tops += [top + b"A" * (k - 2) + bytes([c]) for c in b"CDHL"]          # first residue: top code
    tops += [top + b"Z" * (k - 1), b"*" + top * (k - 1), top * (k - 1) + b"A"]
    tops = list(dict.fromkeys(tops))  # without extra symbols the top symbol is '*' itself
    ties = []
    if k == 8:  # the largest code at positions x and x + 3 only: the first one is the minimizer
        for x in range(5):
            for fill in (b"ACDEFGHI", b"KLMNPQRS", b"YYYYYYYY", b"BJOUBJOU"):
                r = bytearray(fill)
                r[x] = r[x + 3] = top[0]
                ties.append(bytes(r))
    else:       # the same shapes cut to K, so that the role exists at every K
        for x in range(k - 3):
            for fill in (b"ACDEFGHI", b"KLMNPQRS", b"BJOUBJOU"):
                r = bytearray(fill[:k])
                r[x] = r[x + 3] = top[0]
                ties.append(bytes(r))
    lasts = [fill[:k - 1] + top for fill in (b"ACDEFGHI", b"KLMNPQRS", b"TVWYTVWY", b"BJOUXZBJ",
                                             b"AAAAAAAA", b"ZZZZZZZZ", b"HHHHDDDD", b"XXXXXXXX")]
    return {FID_TOP: tops, FID_TIE: ties, FID_LAST: lasts}


def fid0_kmer(k):
    return b"QWQWQWQW"[:k]


def table_rows(k, extra):
    """(kmer, fid) rows in file order: 24 roles of 150 random rows (uniform over the alphabet,
    heavy in BJOUXZ* and the extra symbols, the twenty letters with a tenth of rare symbols, and
    one role of codes 26..31 alone), every 50th row once more under another fid somewhere in the
    file (the last row of a kmer wins), rows of other lengths (one of them with a byte no K-length
    row has), the fid-0 row, and the special rows last, so that they keep their roles."""
    assert k in KS
    rng = np.random.default_rng([5, k, int(extra)])
    alpha, high = _alphabet(extra), _high(extra)
    aa20 = b"ACDEFGHIKLMNPQRSTVWY"
    rows = []
    for fid in range(1, N_REGULAR + 1):
        if fid == N_REGULAR:     # the stratum of codes 26..31 alone
            kmers = _draw(rng, high, np.ones(len(high)), ROWS_PER_ROLE, k)
        elif fid % 3 == 0:       # uniform over every symbol
            kmers = _draw(rng, alpha, np.ones(len(alpha)), ROWS_PER_ROLE, k)
        elif fid % 3 == 1:       # 60% rare symbols and extra ones
            heavy = RARE + (EXTRA if extra else b"")
            w = [0.6 / len(heavy) if c in heavy else 0.4 / (len(alpha) - len(heavy)) for c in alpha]
            kmers = _draw(rng, alpha, w, ROWS_PER_ROLE, k)
        else:                    # the twenty letters, a tenth of the residues any other symbol
            w = [0.9 / 20 if c in aa20 else 0.1 / (len(alpha) - 20) for c in alpha]
            kmers = _draw(rng, alpha, w, ROWS_PER_ROLE, k)
        rows += [(km, fid) for km in kmers]
    rows = [rows[i] for i in rng.permutation(len(rows))]
    dups = [(int(rng.integers(0, len(rows) + 1)), (rows[i][0], 1 + (rows[i][1] + j) % N_REGULAR))
            for j, i in enumerate(range(0, len(rows), 50))]
    for at, row in sorted(dups, reverse=True):
        rows.insert(at, row)
    rows.insert(len(rows) // 2, (fid0_kmer(k), 0))
    for fid, kmers in special_rows(k, extra).items():
        rows += [(km, fid) for km in kmers]
    off_length = [(b"ACDEFGHIK"[:k - 1], 3), (b"ZZZZ*ZZZZ"[:k + 1], 5), (b"ACD#EFGHI"[:k + 1], 7),
                  (b"", 2), (_top(extra) * (k - 1), FID_TOP)]
    for j, row in enumerate(off_length):  # spread through the file, one of them last but one
        rows.insert(min(len(rows) - 1, (j * len(rows)) // 3), row)
    return rows


def last_wins(k, rows):
    """{kmer: fid} of the K-length rows, the last row of a kmer winning."""
    return {km: fid for km, fid in rows if len(km) == k}


def zero_low_windows(k, extra):
    """Windows whose packed key is not 0 and has a zero low dword (K = 7, 8): residues without a
    code but one whose code is a multiple of 4 at bit 30, after a first residue `s` (K = 8: part
    of the window; K = 7: the residue before it). Returns (s, window of K bytes) pairs."""
    if k not in (7, 8):
        return []
    out = []
    for s in (b"A", EXTRA[3:]):
        for i, r in enumerate(ZERO_LOW_R + (b"-" if extra else b"")):
            pad = bytes(NOISE[(i + j) % len(NOISE)] for j in range(6))
            out.append((s, (s if k == 8 else b"") + bytes([r]) + pad))
    return out


def proteins(k, rows, extra):
    """About 1,500 proteins of 0 to 600 residues: chains of table kmers of one role (two roles:
    ambiguous; one to four kmers: below the minimum; one kmer repeated: set and multiset counts
    differ), mutated 2% over the alphabet with 1% noise bytes (NOISE, and the EXTRA bytes for a
    table that has no code for them), random and tiny proteins, one unmutated chain of every
    special role's rows, and the zero-low-word windows, each inside a protein with six distinct
    rows of one role on either side and as a protein of exactly K residues."""
    rng = np.random.default_rng([11, k, int(extra)])
    table = last_wins(k, rows)
    by_fid = {}
    for km, fid in table.items():
        if fid != 0:
            by_fid.setdefault(fid, []).append(km)
    fids = sorted(by_fid)
    alpha = np.frombuffer(_alphabet(extra), np.uint8)
    noise = np.frombuffer(NOISE + (b"" if extra else EXTRA), np.uint8)

    def chain(fid, n, distinct=False):
        pool = by_fid[fid]
        pick = rng.choice(len(pool), n, replace=not distinct) if n else []
        return b"".join(pool[i] for i in pick)

    def mutate(p, rate=0.02):
        b = np.frombuffer(p, np.uint8).copy()
        m = rng.random(len(b)) < rate
        b[m] = alpha[rng.integers(0, len(alpha), int(m.sum()))]
        m = rng.random(len(b)) < 0.01
        b[m] = noise[rng.integers(0, len(noise), int(m.sum()))]
        return b.tobytes()

    def random_protein(n):
        return alpha[rng.integers(0, len(alpha), n)].tobytes()

    prots = []
    for _ in range(1450):
        kind = int(rng.choice(7, p=(0.38, 0.12, 0.16, 0.12, 0.06, 0.08, 0.08)))
        fid = fids[int(rng.integers(0, len(fids)))]
        if kind == 0:
            p = mutate(chain(fid, int(rng.integers(5, 600 // k + 1))))
        elif kind == 1:
            other = fids[int(rng.integers(0, len(fids)))]
            n = int(rng.integers(2, 600 // k))
            cut = int(rng.integers(1, n))
            p = mutate(chain(fid, cut) + chain(other, n - cut))
        elif kind == 2:
            p = mutate(chain(fid, int(rng.integers(1, 5)), distinct=True), 0.005)
        elif kind == 3:
            p = mutate(random_protein(int(rng.integers(0, 601))))
        elif kind == 4:
            p = mutate(random_protein(int(rng.integers(0, k + 3))), 0.2)
        elif kind == 5:
            p = mutate(chain(fid, int(rng.integers(5, 600 // k + 1))), 0.15)
        else:
            p = chain(fid, 1) * int(rng.integers(1, 600 // k + 1))
        prots.append(p[:600])
    for fid, kmers in special_rows(k, extra).items():
        prots.append(b"".join(kmers)[:600])
        prots.append(b"".join(reversed(kmers))[:600])
    regular = [f for f in fids if f < N_REGULAR and len(by_fid[f]) >= 12]
    for j, (s, w) in enumerate(zero_low_windows(k, extra)):
        fid = regular[j % len(regular)]
        lead = s if k == 7 else b""
        prots.append(chain(fid, 6, distinct=True) + lead + w + chain(fid, 6, distinct=True))
        prots.append(w)
    k0 = fid0_kmer(k)
    return [p.replace(k0, k0[:-1] + b" ") for p in prots]


@functools.lru_cache(maxsize=None)
def workload(k, extra):
    """table_rows and proteins of (K, extra) with the packed batch, computed once and frozen."""
    from oracle import c_oracle
    rows = table_rows(k, extra)
    prots = proteins(k, rows, extra)
    res, off = c_oracle.pack_strings(prots)
    for a in (res, off):
        a.flags.writeable = False
    return types.SimpleNamespace(
        k=k, extra=extra, rows=rows, kmers=[km for km, _ in rows],
        fids=np.array([f for _, f in rows], np.int32), prots=prots, res=res, off=off,
        table=last_wins(k, rows), n_skipped=sum(len(km) != k for km, _ in rows))


_expected = {}


def oracle_apply(oracle_c, k, extra, flags):
    """oracle_c.apply on workload(k, extra), computed once per (K, extra, flags) and frozen."""
    key = (k, extra, flags)
    if key not in _expected:
        wl = workload(k, extra)
        e = oracle_c.apply(oracle_c.Table(wl.kmers, wl.fids), wl.res, wl.off, k, MIN_HITS, flags)
        for a in e:
            a.flags.writeable = False
        _expected[key] = e
    return _expected[key]


# ---- packed keys over all 31 codes (the slot dump) -------------------------------------------------

def pack_codes(codes):
    """(n, K) residue codes -> packed keys, first residue most significant."""
    keys = np.zeros(len(codes), np.uint64)
    for j in range(codes.shape[1]):
        keys = (keys << np.uint64(5)) | codes[:, j].astype(np.uint64)
    return keys


def key_codes(keys, k):
    """Packed keys -> (n, K) residue codes."""
    keys = np.asarray(keys, np.uint64)
    return np.stack([((keys >> np.uint64(5 * (k - 1 - j))) & np.uint64(31)).astype(np.uint8)
                     for j in range(k)], axis=1)


def codes_text(codes):
    """Residue codes 1..31 as the bytes of a table with the EXTRA symbols."""
    sym = np.frombuffer(b"\x00" + STD + EXTRA, np.uint8)
    return sym[codes]


def dump_keys(k, seed=0, n=6000):
    """(keys, fids, {key: winning fid}) for kma_table_build_device: random keys over the codes
    1..31, a stratum of codes 26..31, keys whose first residue is 31 (top key byte 0xF8..0xFF at
    K = 8), the all-ones key 2^(5K) - 1, at K = 8 the mod-sampling ties, and a tenth of the rows
    repeating an earlier key under a new fid (the last row wins). fids are the row numbers + 1."""
    rng = np.random.default_rng([23, k, seed])
    parts = [rng.integers(1, 32, (n, k)), rng.integers(26, 32, (n // 10, k))]
    first31 = rng.integers(1, 32, (n // 10, k))
    first31[:, 0] = 31
    first31[: n // 40, 1] = rng.integers(28, 32, n // 40)  # key bits 32..39 = 0xFC..0xFF
    parts.append(first31)
    fixed = [[31] * k, [31] + [1] * (k - 1), [1] * (k - 1) + [31], [26] * k, [27] * k,
             [31] * (k - 1) + [30]]
    for x in range(5):
        for fill in range(1, 31, 3):
            r = [fill] * k
            r[x] = r[x + 3] = 31
            fixed.append(r)
            r = list(rng.integers(1, 27, k))
            r[x] = r[x + 3] = 27
            fixed.append(r)
    parts.append(np.array(fixed))
    keys = pack_codes(np.concatenate(parts).astype(np.uint8))
    keys = keys[rng.permutation(len(keys))]
    keys = np.concatenate([keys, keys[rng.integers(0, len(keys), len(keys) // 10)],
                           pack_codes(np.array([[31] * k], np.uint8))])
    fids = np.arange(1, len(keys) + 1, dtype=np.uint32)
    want = {int(key): int(f) for key, f in zip(keys.tolist(), fids.tolist())}
    assert len(want) < len(keys) and (1 << (5 * k)) - 1 in want
    return keys, fids, want


# ---- pegs and set-operator proteins ----------------------------------------------------------------

def peg_case(k):
    """Pegs over 'A'..'Z' and '*' with 'X' runs, lower case, EXTRA bytes, kmers repeated inside a
    peg and across pegs, and pegs of length 0, K and K + 1."""
    rng = np.random.default_rng([31, k])
    std = np.frombuffer(STD, np.uint8)
    w = np.array([3.0 if c in RARE else 1.0 for c in STD])
    w[STD.index(b"X")] = 0.3
    w /= w.sum()
    pegs = [std[rng.choice(27, int(rng.integers(k + 2, 400)), p=w)].tobytes() for _ in range(140)]
    for i in range(0, 60, 4):       # a kmer-rich stretch once more: inside the peg, in another peg
        seg = pegs[i][5:5 + 3 * k]
        if i % 8 == 0:
            pegs[i] += b"ZZ" + seg
        else:
            pegs[i + 1] = pegs[i + 1][:20] + seg + pegs[i + 1][20:]
    for i in range(60, 80):         # 'X' runs, lower case and bytes without a standard code
        b = bytearray(pegs[i])
        at = int(rng.integers(0, len(b) - k))
        b[at:at + int(rng.integers(1, k + 2))] = b"X" * (k + 2)
        b = b[:len(pegs[i])]
        for c in b"a-1\xc3xz ":
            b[int(rng.integers(0, len(b)))] = c
        pegs[i] = bytes(b)
    for i in range(80, 100):        # a last window (never counted) that is another peg's kmer
        pegs[i] += pegs[i + 20][10:10 + k]
    pegs += [b"", b"Z*ZJOUBXZ*ZJ"[:k], b"*ZJOUB*ZJOUBZ"[:k + 1], b"X" * (2 * k), b"Z" * (k + 5),
             b"*" * (2 * k + 1), b"ZZZZZZZZZZZZ*"[-(k + 1):], b"acdefghiklmnpqrst"]
    return pegs


def peg_singletons(oracle_c, k, pegs):
    """(kmers, peg of each) of the peg windows (oracle_c.peg_kmers: i < L - K, no 'X') that hold
    standard symbols only and occur exactly once over all pegs."""
    res, off = oracle_c.pack_strings(pegs)
    km, pg, _ = oracle_c.peg_kmers(res, off, k)
    standard = (code_of(False)[km] != 0).all(axis=1)
    km, pg = km[standard], pg[standard]
    _, first, count = np.unique(km, axis=0, return_index=True, return_counts=True)
    once = first[count == 1]
    return [r.tobytes() for r in km[once]], pg[once]


def set_op_proteins(seed=3, n=200):
    """200 proteins over the 27 standard symbols, half of their residues from BJOUXZ*, with
    mutated copies, fragments and repeats (shared kmers), '*' * K and 'Z' * K runs for K up to 12,
    and empty and short ones."""
    rng = np.random.default_rng(seed)
    std = np.frombuffer(STD, np.uint8)
    w = np.array([0.5 / len(RARE) if c in RARE else 0.5 / (27 - len(RARE)) for c in STD])
    prots = [std[rng.choice(27, int(rng.integers(0, 300)), p=w)].tobytes() for _ in range(n - 50)]
    for i in range(0, 36, 3):
        b = np.frombuffer(prots[i], np.uint8).copy()
        m = rng.random(len(b)) < 0.08
        b[m] = std[rng.choice(27, int(m.sum()), p=w)]
        prots += [b.tobytes(), prots[i][len(prots[i]) // 3:], prots[i] * 2]
    prots += [b"", b"*", b"Z*", b"*" * 12, b"*" * 13, b"*" * 30, b"Z" * 12, b"Z" * 25,
              b"*" * 12 + b"Z" * 12, b"Z*" * 20, b"ZZZZZZZZZZZ*", b"BJOUXZ*BJOUXZ*", b"XXXXXXXXXXXXX",
              b"A" * 40]
    return prots[:n] if len(prots) >= n else prots + [b"*Z" * 9] * (n - len(prots))
