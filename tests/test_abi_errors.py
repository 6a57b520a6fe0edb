"""Argument errors of the projector's set operators: the return code and the whole
kma_last_error() text of every check that runs before the first device call (no GPU needed),
the hipSetDevice failure every operator reports the same way, and (gpu) the checks that need a
device first. The calls go through a plain ctypes handle so that null and dummy pointers can be
passed; a dummy payload pointer (DUMMY) is only ever given where the check fires before the
payload is read."""
import ctypes as C

import numpy as np
import pytest

import kmeranno as k

DUMMY = C.c_void_p(4096)  # non-null, never dereferenced
NULL = C.c_void_p(None)
DECREASE = [0, 3, 2]      # offsets decrease at 1
HUGE = [0, 1 << 31]       # 2^31 residues / bases by the offsets alone
NO_DEVICE = 9999          # no such HIP device, with or without a GPU


@pytest.fixture(scope="module")
def raw(native_lib):
    """The loaded library through a ctypes handle of its own (no ndpointer argtypes)."""
    lib = C.CDLL(k.LIB_PATH)
    lib.kma_last_error.restype = C.c_char_p
    vp, u64, u32, i, d = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_double
    lib.kma_peg_table_create.argtypes = [vp, vp, u32, i, i, d, vp, vp]
    lib.kma_build_signatures.argtypes = [vp, vp, vp, u32, i, u32, i, vp, vp, u64, vp]
    lib.kma_protein_distances.argtypes = [vp, vp, u32, i, u32, vp, vp, u64, i, vp, vp, vp]
    lib.kma_protein_best_match.argtypes = [vp, vp, u32, i, u32, vp, vp, vp, u32, d, i, vp, vp]
    lib.kma_hash_annotate.argtypes = [vp, vp, u32, vp, vp, u32, i, d, i, vp, vp, vp]
    lib.kma_orf_index_create.argtypes = [vp, vp, u32, i, i, vp]
    lib.kma_orf_index_destroy.argtypes = [vp]
    lib.kma_translate_locations.argtypes = [vp, vp, u32, i, i, vp, u64, i, vp, u64, vp]
    lib.kma_propose_pegs.argtypes = [vp, u64, vp, u32, i, d, d, d, i, vp, u64, vp, vp]
    lib.kma_extend_proposals.argtypes = [vp, vp, u64, d, i, vp, vp, vp, vp]
    return lib


_keep = []  # arrays whose addresses were handed out


def p(a, dtype=np.uint64):
    """Pointer to a C-contiguous copy of `a` (kept alive for the test run)."""
    arr = np.ascontiguousarray(a, dtype=dtype)
    _keep.append(arr)
    return C.c_void_p(arr.ctypes.data)


def res(text=b"ACDEFGHIKLMNPQRSTVWY"):
    return p(np.frombuffer(text, np.uint8), np.uint8)


def out(n=8):
    return p(np.zeros(n, np.uint64))


def expect(lib, rc, code, msg):
    assert rc == code
    assert lib.kma_last_error().decode() == msg


def expect_no_device(lib, rc):
    got = lib.kma_last_error().decode()
    assert rc == k.E_DEVICE and got.startswith(f"hipSetDevice({NO_DEVICE}): "), got
    assert len(got) > len(f"hipSetDevice({NO_DEVICE}): ")  # the runtime's reason follows


# ---- kma_peg_table_create (no residue limit before the device: no HUGE case) --------------------
@pytest.mark.parametrize("residues,offsets,n,kk,lf,msg", [
    (res(), p(DECREASE), 2, 8, 0.5, "offsets decrease at 1"),
    (NULL, p([0, 3]), 1, 8, 0.5, "null argument"),
    (res(), NULL, 1, 8, 0.5, "null argument"),
    (res(), p([0, 3]), 1, 0, 0.5, "kmer size 0 outside 1..12"),
    (res(), p([0, 3]), 1, 13, 0.5, "kmer size 13 outside 1..12"),
    (res(), p([0, 3]), 1, 8, 0.99, "load factor 0.990 > 0.95"),
    (DUMMY, DUMMY, (1 << 22) + 1, 8, 0.5, "more than 2^22 pegs"),
])
def test_peg_table_create(raw, residues, offsets, n, kk, lf, msg):
    h = C.c_void_p(1)
    rc = raw.kma_peg_table_create(residues, offsets, n, kk, 0, lf, C.byref(h), NULL)
    expect(raw, rc, k.E_INVALID, msg)
    assert h.value is None  # *out is cleared first


def test_peg_table_create_null_out(raw):
    expect(raw, raw.kma_peg_table_create(res(), p([0, 3]), 1, 8, 0, 0.5, NULL, NULL),
           k.E_INVALID, "null argument")


# ---- kma_build_signatures -----------------------------------------------------------------------
@pytest.mark.parametrize("residues,offsets,roles,n,kk,flags,msg", [
    (res(), p(DECREASE), p([0, 0], np.int32), 2, 8, 0, "offsets decrease at 1"),
    (NULL, p([0, 3]), p([0], np.int32), 1, 8, 0, "null argument"),
    (res(), NULL, p([0], np.int32), 1, 8, 0, "null argument"),
    (res(), p([0, 3]), NULL, 1, 8, 0, "null argument"),
    (res(), p([0, 3]), p([0], np.int32), 1, 0, 0, "kmer size 0 outside 1..12"),
    (res(), p([0, 3]), p([0], np.int32), 1, 13, 0, "kmer size 13 outside 1..12"),
    (res(), p([0, 3]), p([0], np.int32), 1, 8, 2, "bad flags"),
    (res(), p([0, 3, 6]), p([0, (1 << 24) - 1], np.int32), 2, 8, 0,
     "role 16777215 of protein 1 >= 2^24 - 1"),
    (DUMMY, p(HUGE), p([0], np.int32), 1, 8, 0, "more than 2^31 residues in one call"),
])
def test_build_signatures(raw, residues, offsets, roles, n, kk, flags, msg):
    n_out = C.c_uint64(7)
    rc = raw.kma_build_signatures(residues, offsets, roles, n, kk, flags, 0, out(), out(), 8,
                                  C.byref(n_out))
    expect(raw, rc, k.E_INVALID, msg)
    assert n_out.value == 0


def test_build_signatures_null_n_out(raw):
    rc = raw.kma_build_signatures(res(), p([0, 3]), p([0], np.int32), 1, 8, 0, 0, out(), out(), 8,
                                  NULL)
    expect(raw, rc, k.E_INVALID, "null argument")


# ---- kma_protein_distances ----------------------------------------------------------------------
DIST_CASES = [
    (res(), p(DECREASE), 2, 8, 0, "offsets decrease at 1"),
    (NULL, p([0, 3]), 1, 8, 0, "null argument"),
    (res(), NULL, 1, 8, 0, "null argument"),
    (res(), p([0, 3]), 1, 1, 0, "kmer size 1 outside 2..12"),
    (res(), p([0, 3]), 1, 13, 0, "kmer size 13 outside 2..12"),
    (res(), p([0, 3]), 1, 8, 2, "bad flags"),
    (DUMMY, p(HUGE), 1, 8, 0, "more than 2^31 residues in one call"),
]


@pytest.mark.parametrize("residues,offsets,n,kk,flags,msg", DIST_CASES)
def test_protein_distances(raw, residues, offsets, n, kk, flags, msg):
    rc = raw.kma_protein_distances(residues, offsets, n, kk, flags, NULL, NULL, 0, 0, NULL,
                                   out(), NULL)
    expect(raw, rc, k.E_INVALID, msg)


def test_protein_distances_pairs(raw):
    pa, pb = p([0], np.uint32), p([2], np.uint32)
    rc = raw.kma_protein_distances(res(), p([0, 3, 6]), 2, 8, 0, pa, pb, 1, 0, out(), NULL, NULL)
    expect(raw, rc, k.E_INVALID, "pair 0 indexes a protein >= 2")
    rc = raw.kma_protein_distances(res(), p([0, 3, 6]), 2, 8, 0, pa, NULL, 1, 0, out(), NULL, NULL)
    expect(raw, rc, k.E_INVALID, "null argument")


# ---- kma_protein_best_match (its batch checks are kma_protein_distances') -----------------------
@pytest.mark.parametrize("residues,offsets,n,kk,flags,msg", DIST_CASES)
def test_protein_best_match_batch(raw, residues, offsets, n, kk, flags, msg):
    rc = raw.kma_protein_best_match(residues, offsets, n, kk, flags, NULL, NULL, NULL, 0, 1.0, 0,
                                    NULL, NULL)
    expect(raw, rc, k.E_INVALID, msg)


def test_protein_best_match_candidates(raw):
    q, cand = p([0, 1], np.uint32), p([1, 0, 1], np.uint32)
    best = p([0, 0], np.int32)
    args = (res(), p([0, 3, 6]), 2, 8, 0)
    rc = raw.kma_protein_best_match(*args, q, p(DECREASE), cand, 2, 1.0, 0, best, NULL)
    expect(raw, rc, k.E_INVALID, "cand_off decreases at 1")
    rc = raw.kma_protein_best_match(*args, NULL, p([0, 1, 2]), cand, 2, 1.0, 0, best, NULL)
    expect(raw, rc, k.E_INVALID, "null argument")
    rc = raw.kma_protein_best_match(*args, q, p([0, 1, 2]), NULL, 2, 1.0, 0, best, NULL)
    expect(raw, rc, k.E_INVALID, "null argument")
    rc = raw.kma_protein_best_match(*args, q, p([0, 1, 2]), p([1, 2], np.uint32), 2, 1.0, 0, best,
                                    NULL)
    expect(raw, rc, k.E_INVALID, "pair 1 indexes a protein >= 2")


# ---- kma_hash_annotate: both sides --------------------------------------------------------------
@pytest.mark.parametrize("side,what", [(0, "genome protein"), (1, "prototype")])
@pytest.mark.parametrize("residues,offsets,n,msg", [
    (res(), p(DECREASE), 2, "{} offsets decrease at 1"),
    (NULL, p([0, 3]), 1, "null {}"),
    (res(), NULL, 1, "null {}"),
    (DUMMY, p(HUGE), 1, "more than 2^31 {} residues"),
])
def test_hash_annotate_batches(raw, side, what, residues, offsets, n, msg):
    good = (res(), p([0, 10]), 1)
    g, pt = ((residues, offsets, n), good) if side == 0 else (good, (residues, offsets, n))
    rc = raw.kma_hash_annotate(*g, *pt, 8, 0.5, 0, out(), out(), out())
    expect(raw, rc, k.E_INVALID, msg.format(what))


def test_hash_annotate_scalars(raw):
    g = (res(), p([0, 10]), 1)
    for kk in (1, 13):
        rc = raw.kma_hash_annotate(*g, *g, kk, 0.5, 0, out(), out(), out())
        expect(raw, rc, k.E_INVALID, f"kmer size {kk} outside 2..12")
    for bad in (1.0, -0.1, float("nan")):
        rc = raw.kma_hash_annotate(*g, *g, 8, bad, 0, out(), out(), out())
        expect(raw, rc, k.E_INVALID, "Minimum similarity score must be between 0 and 1.")
    rc = raw.kma_hash_annotate(*g, *g, 8, 0.5, 0, NULL, out(), out())
    expect(raw, rc, k.E_INVALID, "null output")
    rc = raw.kma_hash_annotate(*g, *g, 8, 0.5, 0, out(), out(), NULL)
    expect(raw, rc, k.E_INVALID, "null output")


# ---- kma_orf_index_create -----------------------------------------------------------------------
@pytest.mark.parametrize("dna,offsets,n,code,msg", [
    (res(b"ACGTACGT"), p(DECREASE), 2, 11, "offsets decrease at 1"),
    (NULL, p([0, 3]), 1, 11, "null argument"),
    (res(b"ACGTACGT"), NULL, 1, 11, "null argument"),
    (res(b"ACGTACGT"), p([0, 3]), 1, 2, "genetic code 2: the ORF index knows codes 1, 4 and 11"),
    (DUMMY, p(HUGE), 1, 11, "2^31 bases or more"),
])
def test_orf_index_create(raw, dna, offsets, n, code, msg):
    h = C.c_void_p(1)
    rc = raw.kma_orf_index_create(dna, offsets, n, code, 0, C.byref(h))
    expect(raw, rc, k.E_INVALID, msg)
    assert h.value is None


def test_orf_index_create_null_out(raw):
    rc = raw.kma_orf_index_create(res(b"ACGT"), p([0, 3]), 1, 11, 0, NULL)
    expect(raw, rc, k.E_INVALID, "null argument")


# ---- kma_translate_locations --------------------------------------------------------------------
def loc(contig=0, left=1, right=3, strand=b"+"):
    a = np.zeros(1, k.LOCATION_DTYPE)
    a["contig"], a["left"], a["right"], a["strand"] = contig, left, right, strand[0]
    _keep.append(a)
    return C.c_void_p(a.ctypes.data)


@pytest.mark.parametrize("dna,offsets,n,code,locs,flags,msg", [
    (res(b"ACGTACGT"), p(DECREASE), 2, 11, loc(), 0, "offsets decrease at 1"),
    (NULL, p([0, 3]), 1, 11, loc(), 0, "null argument"),
    (res(b"ACGTACGT"), NULL, 1, 11, loc(), 0, "null argument"),
    (res(b"ACGTACGT"), p([0, 3]), 1, 11, NULL, 0, "null argument"),
    (res(b"ACGTACGT"), p([0, 3]), 1, 11, loc(), 3, "unknown flag bits 0x2"),
    (res(b"ACGTACGT"), p([0, 3]), 1, 7, loc(), 0, "genetic code 7 is not a known NCBI table"),
    (DUMMY, p(HUGE), 1, 11, loc(), 0, "2^31 bases or more"),
    (res(b"ACGTACGT"), p([0, 3]), 1, 11, loc(contig=1), 0, "location 0: contig 1 >= 1"),
    (res(b"ACGTACGT"), p([0, 3]), 1, 11, loc(strand=b"x"), 0,
     "location 0: strand must be '+' or '-'"),
    (res(b"ACGTACGT"), p([0, 3]), 1, 11, loc(left=0), 0, "location 0: left 0 < 1"),
    (res(b"ACGTACGT"), p([0, 3]), 1, 11, loc(right=4), 0,
     "location 0: right 4 past the contig's 3 bases"),
    (res(b"ACGTACGT"), p([0, 3]), 1, 11, loc(left=3, right=1), 0,
     "location 0: right 1 < left 3 - 1"),
])
def test_translate_locations(raw, dna, offsets, n, code, locs, flags, msg):
    rc = raw.kma_translate_locations(dna, offsets, n, code, 0, locs, 1, flags, out(), 8, out())
    expect(raw, rc, k.E_INVALID, msg)


def test_translate_locations_capacity_and_outputs(raw):
    dna, off = res(b"ACGTACGT"), p([0, 6])
    rc = raw.kma_translate_locations(dna, off, 1, 11, 0, loc(right=6), 1, 0, out(), 1, out())
    expect(raw, rc, k.E_CAPACITY, "2 residues, capacity 1")
    rc = raw.kma_translate_locations(dna, off, 1, 11, 0, loc(right=6), 1, 0, NULL, 8, out())
    expect(raw, rc, k.E_INVALID, "null argument")
    rc = raw.kma_translate_locations(dna, off, 1, 11, 0, loc(right=6), 1, 0, out(), 8, NULL)
    expect(raw, rc, k.E_INVALID, "null argument")


# ---- kma_propose_pegs ---------------------------------------------------------------------------
def hits(rows):
    a = np.zeros(len(rows), k.HIT_DTYPE)
    for i, (contig, left, fid, strand) in enumerate(rows):
        a[i]["contig"], a[i]["left"], a[i]["fid"], a[i]["strand"] = contig, left, fid, strand[0]
    _keep.append(a)
    return C.c_void_p(a.ctypes.data)


@pytest.mark.parametrize("h,n_hits,peg_len,n_peg,kk,o,msg", [
    (hits([(0, 1, 0, b"+")]), 1, p([9, 9], np.uint32), 2, 0, out(), "kmer size 0 outside 1..12"),
    (hits([(0, 1, 0, b"+")]), 1, p([9, 9], np.uint32), 2, 13, out(), "kmer size 13 outside 1..12"),
    (NULL, 1, p([9, 9], np.uint32), 2, 8, out(), "null argument"),
    (hits([(0, 1, 0, b"+")]), 1, NULL, 2, 8, out(), "null argument"),
    (hits([(0, 1, 0, b"+")]), 1, p([9, 9], np.uint32), 0, 8, out(), "null argument"),
    (hits([(0, 1, 0, b"+")]), 1, p([9, 9], np.uint32), 2, 8, NULL, "null output"),
    (DUMMY, 1 << 31, p([9, 9], np.uint32), 2, 8, out(), "more than 2^31 connections"),
    (hits([(0, 1, 0, b"+")]), 1, DUMMY, 715827883, 8, out(), "too many pegs"),
    (hits([(0, 1, 5, b"+")]), 1, p([9, 9], np.uint32), 2, 8, out(), "connection 0: peg 5 >= 2"),
    (hits([(0, 1, 0, b"x")]), 1, p([9, 9], np.uint32), 2, 8, out(),
     "connection 0: strand must be '+' or '-'"),
    (hits([(1, 1, 0, b"+"), (0, 1, 0, b"+")]), 2, p([9, 9], np.uint32), 2, 8, out(),
     "connections are not in (contig, left) order at 1"),
    (hits([(0, 5, 0, b"+"), (0, 4, 0, b"-")]), 2, p([9, 9], np.uint32), 2, 8, out(),
     "connections are not in (contig, left) order at 1"),
])
def test_propose_pegs(raw, h, n_hits, peg_len, n_peg, kk, o, msg):
    n_out, stats = C.c_uint64(7), p([7, 7, 7, 7])
    rc = raw.kma_propose_pegs(h, n_hits, peg_len, n_peg, kk, 0.2, 0.5, 0.1, 0, o, 4,
                              C.byref(n_out), stats)
    expect(raw, rc, k.E_INVALID, msg)


def test_propose_pegs_null_counters(raw):
    h, pl = hits([(0, 1, 0, b"+")]), p([9, 9], np.uint32)
    rc = raw.kma_propose_pegs(h, 1, pl, 2, 8, 0.2, 0.5, 0.1, 0, out(), 4, NULL, out())
    expect(raw, rc, k.E_INVALID, "null argument")
    rc = raw.kma_propose_pegs(h, 1, pl, 2, 8, 0.2, 0.5, 0.1, 0, out(), 4, out(), NULL)
    expect(raw, rc, k.E_INVALID, "null argument")


# ---- kma_extend_proposals -----------------------------------------------------------------------
def test_extend_proposals_null_index(raw):
    rc = raw.kma_extend_proposals(NULL, DUMMY, 1, 0.2, 1, out(), out(), out(), out())
    expect(raw, rc, k.E_INVALID, "null argument")


# ---- entering a device: one message for every operator ------------------------------------------
def test_no_such_device(raw):
    """Valid arguments and a device that does not exist: KMA_E_DEVICE, 'hipSetDevice(<device>): '
    and the runtime's reason, before anything is allocated."""
    r, off, roles = res(), p([0, 10, 20]), p([0, 1], np.int32)
    h, n_out = C.c_void_p(), C.c_uint64()
    expect_no_device(raw, raw.kma_peg_table_create(r, off, 2, 8, NO_DEVICE, 0.5, C.byref(h), NULL))
    expect_no_device(raw, raw.kma_build_signatures(r, off, roles, 2, 8, 0, NO_DEVICE, out(), out(),
                                                   8, C.byref(n_out)))
    expect_no_device(raw, raw.kma_protein_distances(r, off, 2, 8, 0, NULL, NULL, 0, NO_DEVICE,
                                                    NULL, out(), NULL))
    expect_no_device(raw, raw.kma_hash_annotate(r, off, 2, r, off, 2, 8, 0.5, NO_DEVICE, out(),
                                                out(), out()))
    expect_no_device(raw, raw.kma_orf_index_create(res(b"ATGAAATAG"), p([0, 9]), 1, 11, NO_DEVICE,
                                                   C.byref(h)))
    expect_no_device(raw, raw.kma_translate_locations(res(b"ATGAAATAG"), p([0, 9]), 1, 11,
                                                      NO_DEVICE, loc(right=9), 1, 0, out(), 8,
                                                      out()))
    expect_no_device(raw, raw.kma_propose_pegs(hits([(0, 1, 0, b"+")]), 1, p([9, 9], np.uint32), 2,
                                               8, 0.2, 0.5, 0.1, NO_DEVICE, out(), 4,
                                               C.byref(n_out), out()))


# ---- checks behind a device call ----------------------------------------------------------------
ALPHABET = "a protein window holds a byte outside A-Z and '*'"


@pytest.mark.gpu
def test_alphabet_errors_gpu(raw):
    """A byte outside A-Z / '*' inside a counted window: KMA_E_ALPHABET from the three operators
    that read the device's flag back."""
    r, off, roles = res(b"ACDEFGHIKLMNPQRSTVWYACDEFGHIK1MNPQRSTVWY"), p([0, 20, 40]), p([0, 1], np.int32)
    n_out = C.c_uint64()
    rc = raw.kma_build_signatures(r, off, roles, 2, 8, 0, 0, out(64), out(64), 64, C.byref(n_out))
    expect(raw, rc, k.E_ALPHABET, ALPHABET)
    rc = raw.kma_protein_distances(r, off, 2, 8, 0, NULL, NULL, 0, 0, NULL, out(), NULL)
    expect(raw, rc, k.E_ALPHABET, ALPHABET)
    good = (res(), p([0, 20]), 1)
    for g, pt in (((r, off, 2), good), (good, (r, off, 2))):
        rc = raw.kma_hash_annotate(*g, *pt, 8, 0.5, 0, out(), out(), out())
        expect(raw, rc, k.E_ALPHABET, ALPHABET)


@pytest.mark.gpu
def test_extend_proposals_errors_gpu(raw):
    """kma_extend_proposals checks its proposals against the index's contigs before it stages
    them."""
    h = C.c_void_p()
    assert raw.kma_orf_index_create(res(b"ATGAAATAG"), p([0, 9]), 1, 11, 0, C.byref(h)) == k.OK

    def prop(contig=0, left=1, right=9, strand=b"+"):
        a = np.zeros(1, k.PROPOSAL_DTYPE)
        a["contig"], a["left"], a["right"], a["strand"] = contig, left, right, strand[0]
        _keep.append(a)
        return C.c_void_p(a.ctypes.data)

    try:
        for pr, msg in ((prop(contig=1), "proposal 0: contig 1 >= 1"),
                        (prop(strand=b"x"), "proposal 0: strand must be '+' or '-'"),
                        (prop(left=4, right=5), "proposal 0: shorter than a codon")):
            rc = raw.kma_extend_proposals(h, pr, 1, 0.2, 1, out(), out(), out(), out())
            expect(raw, rc, k.E_INVALID, msg)
        rc = raw.kma_extend_proposals(h, NULL, 1, 0.2, 1, out(), out(), out(), out())
        expect(raw, rc, k.E_INVALID, "null argument")
        rc = raw.kma_extend_proposals(h, prop(), 1, 0.2, 1, out(), out(), out(), NULL)
        expect(raw, rc, k.E_INVALID, "null argument")
    finally:
        raw.kma_orf_index_destroy(h)
