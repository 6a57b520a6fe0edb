"""GPU parity with identifiers at the top of their bit fields.

A table slot carries its fid in 22 bits that share a word with other fields: the narrow slot's
high dword is key bits 32..39 << 24 | filter bits << 22 | fid, the wide slot's .z is filter bits
<< 22 | fid, and the probe's verdict word puts its hit flag at bit 22, the slot from bit 24 and
the absent filter positions from bit 28 (kma_internal.h, kma_device.h). The other GPU tests use
at most 10,000 fids, so bits 14..21 of a fid are never set there. Here the fids are sent through
an injective map onto [0, 2^22) that includes 0, 1, 2^14 - 1, 2^14, 2^21, 2^21 + 1, 2^22 - 2 and
2^22 - 1, the peg join and the proposal sweep run with 2^22 pegs, the signature build with roles
up to 2^24 - 2 (one below its tag for buffered proteins), and a tally shorter than the fid range
must be left untouched past its end. Expected values are the C oracle's (or, for the slot dump,
the input rows'), never the library's.
"""
import types

import numpy as np
import pytest

from helpers import full_oracle_table, unpack_keys
from test_gpu_build import _family_proteins

pytestmark = pytest.mark.gpu

FID_BITS = 22
N_FID = 1 << FID_BITS          # KMA_MAX_FID + 1
FID_MASK = N_FID - 1
SPECIAL = (0, 1, (1 << 14) - 1, 1 << 14, 1 << 21, (1 << 21) + 1, N_FID - 2, N_FID - 1)
MIN_HITS = 5
F_MULTISET = 2
HIT_FIELDS = ("contig", "left", "strand", "frame", "fid")


def id_map(n, seed, first=(), special=SPECIAL, hi=N_FID):
    """An injective map of the ids 0..n-1 into [0, hi): the ids `first` get the special values in
    order, every other id a value drawn without repetition from [2^14, hi) (seeded)."""
    special = list(special)[:len(first)]
    rng = np.random.default_rng(seed)
    drawn = rng.choice(hi - (1 << 14), n + len(SPECIAL) + len(special), replace=False) + (1 << 14)
    drawn = drawn[~np.isin(drawn, special)][:n]
    m = drawn.astype(np.int64)
    m[np.asarray(first, np.int64)] = special
    assert len(np.unique(m)) == n and m.min() >= 0 and m.max() < hi
    return m


def most_frequent(ids, n):
    """The n ids that occur most often in `ids`, most frequent first."""
    c = np.bincount(ids)
    order = np.argsort(-c, kind="stable")[:n]
    assert (c[order] > 0).all(), "fewer distinct ids than special values"
    return order


@pytest.fixture(scope="module")
def kma(native_lib):
    import kmeranno
    assert kmeranno.device_count() >= 1
    return kmeranno


@pytest.fixture(params=["auto", "7", "0", "6", "chained"],
                ids=["m-auto", "m7", "flat", "m6-random", "chained"])
def layout(request):
    """The size rule's layout with two-choice placement, m = 7, flat, m = 6 in the smallest-hash
    order, and the size rule's layout with overflow chains (KMA_OPT_PLACEMENT = 0); at K = 5 the
    minimizer lengths 6 and 7 both mean 5."""
    import kmeranno
    kmeranno.load()
    p = request.param
    kmeranno.set_option(kmeranno.OPT_LAYOUT, -1 if p in ("auto", "chained") else int(p))
    kmeranno.set_option(kmeranno.OPT_PLACEMENT, 0 if p == "chained" else -1)
    return p


@pytest.fixture(params=["packed", "ascii"])
def input_mode(request):
    import kmeranno
    kmeranno.load()
    kmeranno.set_option(kmeranno.OPT_PACKED_INPUT, 2 if request.param == "packed" else 0)
    return request.param


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


# ---- 1. apply, narrow tables ----------------------------------------------------------------------

_apply_cases = {}


def apply_case(oracle_c, k):
    """synth.make_workload(1500, 60_000, 500) at this K, its fids through the id map (the special
    values on the fids the oracle calls most often unmapped), and the oracle's apply on the
    unmapped and the mapped table for flags 0 and KMA_F_MULTISET; computed once per K."""
    if k not in _apply_cases:
        from kmeranno import synth
        wl = synth.make_workload(1500, 60_000, 500, seed=41 + k, k=k)
        raw = full_oracle_table(oracle_c, wl.keys, wl.fids, k)
        plain = {f: _frozen(*oracle_c.apply(raw, wl.residues, wl.offsets, k, MIN_HITS, f))
                 for f in (0, F_MULTISET)}
        efid, _, est = plain[0]
        m = id_map(wl.n_fid, 1000 + k, most_frequent(efid[est == 1], len(SPECIAL)))
        fids = m[wl.fids].astype(np.uint32)
        mapped_table = full_oracle_table(oracle_c, wl.keys, fids, k)
        mapped = {f: _frozen(*oracle_c.apply(mapped_table, wl.residues, wl.offsets, k, MIN_HITS, f))
                  for f in (0, F_MULTISET)}
        _frozen(wl.keys, wl.residues, wl.offsets, fids, m)
        _apply_cases[k] = types.SimpleNamespace(k=k, keys=wl.keys, fids=fids, res=wl.residues,
                                                off=wl.offsets, map=m, plain=plain, mapped=mapped)
    return _apply_cases[k]


@pytest.mark.parametrize("k", [8, 5])
@pytest.mark.parametrize("flags", [0, F_MULTISET])
def test_apply_id_map_oracle_consistent(oracle_c, k, flags):
    """Both sides the oracle: the mapped table's status and count equal the unmapped table's and
    its fid is map[unmapped fid]; each special value is the fid of a CALLED protein."""
    c = apply_case(oracle_c, k)
    (pfid, pcnt, pst), (efid, ecnt, est) = c.plain[flags], c.mapped[flags]
    assert (est == pst).all() and (ecnt == pcnt).all()
    assert (efid[pfid < 0] == pfid[pfid < 0]).all()
    assert (efid[pfid >= 0] == c.map[pfid[pfid >= 0]]).all()
    called = set(efid[est == 1].tolist())
    assert set(SPECIAL) <= called and len(called) > 50
    assert (est == 2).sum() > 20  # AMBIGUOUS proteins too


@pytest.mark.parametrize("flags", [0, F_MULTISET], ids=["set", "multiset"])
@pytest.mark.parametrize("lf", [0.5, 0.95])
@pytest.mark.parametrize("k", [8, 5])
def test_apply_high_fids_vs_oracle(kma, oracle_c, layout, input_mode, k, lf, flags):
    """1,500 proteins against the 60,000-row table with fids over the whole 22-bit range, under
    every layout and placement, packed and ASCII input, set and multiset counting, at load factor
    0.5 and at 0.95 (displaced keys: the alt-bucket read and the chain walk re-extract the fid):
    (fid, count, status) and the 2^22-entry tally equal the oracle's."""
    c = apply_case(oracle_c, k)
    efid, ecnt, est = c.mapped[flags]
    with kma.SignatureTable.from_packed(c.keys, c.fids, k, load_factor=lf) as t:
        i = t.info
        assert i.k == k and i.n_entries == len(np.unique(c.keys))
        if lf == 0.95:
            assert i.n_displaced > 0
        fid, cnt, st, tally = kma.annotate_proteins(t, c.res, c.off, MIN_HITS, flags, n_fid=N_FID)
    assert (st == est).all() and (fid == efid).all() and (cnt == ecnt).all()
    expect = np.bincount(efid[est == 1], minlength=N_FID)
    assert (tally == expect).all()
    assert tally[N_FID - 1] > 0 and tally[0] > 0


# ---- 2. 6-frame, narrow and wide ------------------------------------------------------------------

_contig_cases = {}


def contig_case(oracle_c, small_gto, k):
    """The first 40 kb of four small.gto contigs, a table of a 50% sample of their 6-frame K-mers
    with fids through the id map (the special values on the fids hit most often), and the oracle's
    hits; once per K."""
    if k not in _contig_cases:
        contigs = [c["dna"][:40_000] for c in small_gto["contigs"][:4]]
        dna, off = oracle_c.pack_strings(contigs)
        km = oracle_c.contig_kmers(dna, off, 11, k)[0]
        rng = np.random.default_rng(200 + k)
        km = km[rng.random(len(km)) < 0.5]
        raw_fids = rng.integers(0, 3000, len(km)).astype(np.int32)
        text, rows = km.tobytes(), np.arange(len(km) + 1, dtype=np.uint64) * k
        raw = oracle_c.annotate_contigs(oracle_c.Table.from_buffer(text, rows, raw_fids), dna, off,
                                        11, k)
        m = id_map(3000, 2000 + k, most_frequent(raw[4].astype(np.int64), len(SPECIAL)))
        fids = m[raw_fids].astype(np.uint32)
        e = _frozen(*oracle_c.annotate_contigs(
            oracle_c.Table.from_buffer(text, rows, fids.astype(np.int32)), dna, off, 11, k))
        assert len(e[0]) == len(raw[0]) > 50_000 and (e[4] == m[raw[4]]).all()
        assert set(SPECIAL) <= set(e[4].tolist())
        _contig_cases[k] = types.SimpleNamespace(k=k, n_contig=len(contigs), dna=dna, off=off,
                                                 kmers=km, fids=fids, e=e)
    return _contig_cases[k]


def _assert_hits(hits, e):
    assert len(hits) == len(e[0])
    for f, b in zip(HIT_FIELDS, e):
        assert (hits[f] == b).all(), f


def _assert_contig_tally(tally, e, n_fid, n_contig):
    """tally[n_contig, n_fid] holds exactly the oracle's hit counts of the fids below n_fid."""
    tally = np.asarray(tally).reshape(n_contig, n_fid)
    keep = e[4] < n_fid
    flat = e[0][keep].astype(np.int64) * n_fid + e[4][keep]
    at, n = np.unique(flat, return_counts=True)
    assert (tally.ravel()[at] == n).all()
    assert int(tally.sum(dtype=np.int64)) == len(flat)  # counts are >= 0: every other entry is 0


@pytest.mark.parametrize("lf", [0.5, 0.9])
@pytest.mark.parametrize("k,placement", [(8, "two-choice"), (8, "chained"), (10, "chained"),
                                         (12, "chained")])
def test_contigs_high_fids_vs_oracle(kma, oracle_c, small_gto, k, placement, lf):
    """Every 6-frame hit (contig, left, strand, frame, fid) and the [4, 2^22] tally equal the
    oracle's through the host call and the device call, on narrow (two-choice and chained) and
    wide tables, with displaced keys at load factor 0.9."""
    torch = pytest.importorskip("torch")
    c = contig_case(oracle_c, small_gto, k)
    kma.set_option(kma.OPT_PLACEMENT, 0 if placement == "chained" else -1)
    keys = kma.pack_std(c.kmers)
    assert (keys != 0).all()
    with kma.SignatureTable.from_packed(keys, c.fids, k, load_factor=lf) as t:
        i = t.info
        assert i.k == k and i.slots_per_bucket == (4 if k > 8 else kma.bucket_slots())
        assert i.n_entries == len(np.unique(keys))
        if placement == "chained":
            assert i.two_choice == 0
        if lf == 0.9:
            assert i.n_displaced > 0
        hits, tally = kma.annotate_contigs(t, c.dna, c.off, 11, n_fid=N_FID)
        _assert_hits(hits, c.e)
        _assert_contig_tally(tally, c.e, N_FID, c.n_contig)
        del tally
        dev = torch.device("cuda", 0)
        stream = torch.cuda.current_stream().cuda_stream
        n_bases = int(c.off[-1])
        ws = kma.Workspace(0)
        ws.reserve_contigs(n_bases)
        d_dna = torch.from_numpy(c.dna.copy()).to(dev)
        d_off = torch.from_numpy(c.off.view(np.int64).copy()).to(dev)
        cap = len(c.e[0]) + 16
        d_hits = torch.zeros(cap * kma.HIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_nh = torch.zeros(1, dtype=torch.int64, device=dev)
        d_tally = torch.zeros(c.n_contig * N_FID, dtype=torch.int32, device=dev)
        kma.annotate_contigs_device(t, ws, d_dna.data_ptr(), d_off.data_ptr(), c.n_contig, n_bases,
                                    11, d_hits.data_ptr(), cap, d_nh.data_ptr(),
                                    d_tally.data_ptr(), N_FID, stream)
        torch.cuda.synchronize()
        n = int(d_nh.item())
        assert n == len(c.e[0])
        _assert_hits(d_hits.cpu().numpy().view(kma.HIT_DTYPE)[:n], c.e)
        _assert_contig_tally(d_tally.cpu().numpy(), c.e, N_FID, c.n_contig)
        ws.close()


# ---- 3. slot dump against the input rows ----------------------------------------------------------

def _dump_rows(k, seed, n=20_000):
    """n rows of random K-mer keys, a tenth of them repeating an earlier row's key, every row a
    different fid through the id map (the special values on rows that win their key), and one
    last row whose fid 2^22 + 5 the build masks to 5. Returns (keys, fids, {key: winning fid})."""
    rng = np.random.default_rng(seed)
    codes = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8).astype(np.uint64) - 64
    fresh = np.zeros(n, np.uint64)
    for _ in range(k):
        fresh = (fresh << np.uint64(5)) | codes[rng.integers(0, 20, n)]
    fresh = np.unique(fresh)
    rng.shuffle(fresh)
    assert len(fresh) > n - 50
    n_first = n - n // 10
    keys = np.concatenate([fresh[:n_first], fresh[rng.integers(0, n_first, n // 10)]])
    keys = keys[rng.permutation(n)]
    last_row = {int(key): r for r, key in enumerate(keys.tolist())}
    winners = sorted(last_row.values())
    assert len(last_row) < n - n // 20  # repeated keys exist
    fids = id_map(n, seed + 1, winners[:len(SPECIAL)]).astype(np.uint32)
    extra = int(fresh[n_first])
    assert extra not in last_row
    keys = np.concatenate([keys, np.array([extra], np.uint64)])
    fids = np.concatenate([fids, np.array([N_FID + 5], np.uint32)])
    want = {key: int(fids[r]) for key, r in last_row.items()}
    want[extra] = 5
    assert set(SPECIAL) <= set(want.values())
    return keys, fids, want


def decode_slots(raw, k):
    """The (key, fid) of every used slot of a slot array copied back as u64 words, decoded as
    include/kmeranno.h documents the slots: narrow (K <= 8) key bits 0..31 in the low dword and
    key bits 32..39 << 24 | filter bits << 22 | fid in the high one; wide .x .y the key, .z filter
    bits << 22 | fid, .w 0. A slot is used when its low key dword is not 0."""
    if k > 8:
        q = raw.view(np.uint32).reshape(-1, 4)  # .x .y .z .w
        assert (q[:, 3] == 0).all()
        used = q[:, 0] != 0
        got_keys = (q[used, 1].astype(np.uint64) << np.uint64(32)) | q[used, 0]
        got_fids = q[used, 2] & np.uint32(FID_MASK)
        assert (q[used, 2] >> np.uint32(FID_BITS + 2) == 0).all()  # fid and two filter bits only
    else:
        lo = (raw & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        hi = (raw >> np.uint64(32)).astype(np.uint32)
        used = lo != 0
        got_keys = ((hi[used] >> np.uint32(24)).astype(np.uint64) << np.uint64(32)) | lo[used]
        got_fids = hi[used] & np.uint32(FID_MASK)
    return got_keys, got_fids


@pytest.mark.parametrize("k,layout_name", [(8, "two-choice"), (8, "chained"), (8, "flat"),
                                           (10, "chained")])
def test_build_device_slot_dump_equals_rows(kma, k, layout_name):
    """kma_table_build_device into buffers the test owns, at load factor 0.9: the slots copied back
    and decoded as include/kmeranno.h documents them hold exactly the last-wins (key, fid) pairs of
    the input rows, each once (a build fault, apart from any probe); fids are masked to 22 bits."""
    torch = pytest.importorskip("torch")
    keys, fids, want = _dump_rows(k, 300 + k)
    n = len(keys)
    S = kma.bucket_slots(k)
    nb = kma.buckets_for(len(want), 0.9, k)  # 0.9 of the slots hold a key
    m = kma.layout_for(k, nb) & 0xFF
    code = {"two-choice": m | kma.LAYOUT_TWO_CHOICE, "chained": m, "flat": 0}[layout_name]
    assert m != 0
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    words = 2 if k > 8 else 1  # u64 per slot
    slots = torch.empty(nb * S * words, dtype=torch.int64, device=dev)
    winner = torch.empty(nb * S, dtype=torch.int32, device=dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    d_keys = torch.from_numpy(keys.view(np.int64)).to(dev)
    d_fids = torch.from_numpy(fids.view(np.int32)).to(dev)
    kma.build_device(slots.data_ptr(), nb, winner.data_ptr(), d_keys.data_ptr(),
                     d_fids.data_ptr(), n, status.data_ptr(), stream, k=k, layout=code)
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    assert st[0] == 0 and st[1] == len(want) and st[3] > 0, st.tolist()
    got_keys, got_fids = decode_slots(slots.cpu().numpy().view(np.uint64), k)
    assert len(got_keys) == len(want)
    got = dict(zip(got_keys.tolist(), got_fids.tolist()))
    assert len(got) == len(want)  # no key twice
    assert got == want


# ---- 4. peg join and proposals at n_peg = 2^22 ----------------------------------------------------

N_PEG = 1 << 22
PEG_SPECIAL = (0, 65535, 65536, N_PEG - 2, N_PEG - 1)
PROPOSAL_FIELDS = ("peg", "contig", "strand", "left", "right", "evidence", "frame")
_peg_case = []


def peg_case(oracle_c, small_gto):
    """small.gto's pegs, mutated 4%, at scattered indices of a close genome of 2^22 pegs (every
    other peg empty): (residues, offsets[2^22 + 1], peg_len[2^22], contig DNA, contig offsets)."""
    if not _peg_case:
        rng = np.random.default_rng(77)
        aa = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
        prots = []
        for f in small_gto["features"]:
            if f.get("protein_translation"):
                b = np.frombuffer(f["protein_translation"].encode(), np.uint8).copy()
                mut = rng.random(len(b)) < 0.04
                b[mut] = aa[rng.integers(0, 20, int(mut.sum()))]
                prots.append(b)
        at = np.union1d(PEG_SPECIAL, rng.choice(N_PEG, len(prots) - len(PEG_SPECIAL), replace=False))
        prots = prots[:len(at)]
        peg_len = np.zeros(N_PEG, np.uint32)
        peg_len[at] = [len(p) for p in prots]
        off = np.zeros(N_PEG + 1, np.uint64)
        np.cumsum(peg_len, dtype=np.uint64, out=off[1:])
        res = np.concatenate(prots + [np.zeros(32, np.uint8)])
        dna, doff = oracle_c.pack_strings([c["dna"] for c in small_gto["contigs"]])
        _peg_case.append(_frozen(res, off, peg_len, dna, doff))
    return _peg_case[0]


@pytest.mark.parametrize("k", [8, 10])
def test_peg_join_and_proposals_at_max_pegs(kma, oracle_c, small_gto, k):
    """kma_peg_table_create on 2^22 pegs (peg indices 0, 65535, 65536, 2^22 - 2 and 2^22 - 1
    among the non-empty ones), the join AGGRESSIVE and STRICT, and the proposal sweep keyed by
    frame * 2^22 + peg: connections and proposals (all fields, counters, order) equal the
    oracle's."""
    res, off, peg_len, dna, doff = peg_case(oracle_c, small_gto)
    t, n_win = kma.SignatureTable.from_pegs(res, off, k)
    assert n_win == int(np.maximum(peg_len.astype(np.int64) - k, 0).sum())
    with t:
        assert t.info.slots_per_bucket == (4 if k > 8 else kma.bucket_slots())
        for strict in (False, True):
            e = oracle_c.peg_connect(res, off, dna, doff, 11, k, strict)
            assert len(e[0]) > 10_000
            if not strict:
                assert set(PEG_SPECIAL) <= set(e[4].tolist())
            hits = kma.connect_pegs(t, dna, doff, 11, strict)
            _assert_hits(hits, e)
            got, gst = kma.propose_pegs(hits, peg_len, k)
            exp, est = oracle_c.propose(e[0], e[1], e[2], e[4], peg_len, k)
            assert (gst == est).all(), (gst, est)
            assert len(got) == len(exp["peg"]) > 100
            for f in PROPOSAL_FIELDS:
                assert (got[f] == exp[f]).all(), f
            assert (got["peg"] >= N_PEG // 2).any() and (got["peg"] < N_PEG // 2).any()


def test_peg_table_refuses_more_than_max_pegs(kma):
    res = np.zeros(32, np.uint8)
    with pytest.raises(kma.KmerAnnoError) as e:
        kma.SignatureTable.from_pegs(res, np.zeros(N_PEG + 2, np.uint64), 8)
    assert e.value.code == kma.E_INVALID and "2^22" in str(e.value)


# ---- 5. signature build with wide roles -----------------------------------------------------------

ROLE_NEG = (1 << 24) - 1  # kBuildNeg: the tag of a buffered protein
ROLE_SPECIAL = (0, 1 << 22, ROLE_NEG - 2, ROLE_NEG - 1, (1 << 22) - 1, 1 << 23, (1 << 14) - 1, 1)


def _unpack(keys, k):
    return [bytes(r).decode() for r in unpack_keys(np.asarray(keys, np.uint64), k)]


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("k", [8, 10])
def test_build_signatures_wide_roles_vs_oracle(kma, oracle_c, k, flags):
    """The family proteins of test_gpu_build with their 50 roles mapped onto {0, 2^22, 2^24 - 3,
    2^24 - 2, ...} (buffered -1 and skipped -2 proteins kept): the discriminating (kmer, role)
    rows equal the oracle's; role 2^24 - 1 is refused."""
    rng = np.random.default_rng(23 + flags + k)
    prots, roles = _family_proteins(rng)
    roles = np.asarray(roles, np.int64)
    m = id_map(50, 500 + k, most_frequent(roles[roles >= 0], len(ROLE_SPECIAL)),
               special=ROLE_SPECIAL, hi=ROLE_NEG)
    roles = np.where(roles >= 0, m[np.maximum(roles, 0)], roles).astype(np.int32)
    assert (roles == -1).any() and (roles == -2).any() and roles.max() == ROLE_NEG - 1
    res, off = oracle_c.pack_strings(prots)
    km, rl = oracle_c.build_signatures(res, off, roles, k, flags)
    keys, groles = kma.build_signatures(res, off, roles, k, flags)
    got = dict(zip(_unpack(keys, k), groles.tolist()))
    exp = {bytes(r).decode(): int(v) for r, v in zip(km, rl)}
    assert len(exp) > 10_000 and set(ROLE_SPECIAL) <= set(exp.values())
    assert got == exp and len(keys) == len(exp)
    bad = roles.copy()
    bad[int(np.flatnonzero(roles >= 0)[-1])] = ROLE_NEG
    with pytest.raises(kma.KmerAnnoError) as e:
        kma.build_signatures(res, off, bad, k, flags)
    assert e.value.code == kma.E_INVALID


@pytest.mark.parametrize("k", [8, 10])
def test_build_signatures_top_role_next_to_buffered_tag(kma, oracle_c, k):
    """RoleTests at the top of the role range: a kmer of role 2^24 - 2 alone is kept with that
    role; shared with a buffered protein (tagged 2^24 - 1 on the device) or with role 2^24 - 3 it
    is dropped; a skipped protein does not touch it. Each outcome is the oracle's too."""
    A, B = ROLE_NEG - 1, ROLE_NEG - 2
    shared = "PPMKVLAGHW"[-k:]
    prot = "QQ" + shared + "NN"
    others = {A: "CCCCDEFGHIKLMNPQ", B: "WWWWYYYYVVVVTTTT"}
    for roles, kept in (([A], True), ([A, A], True), ([A, -1], False), ([-1, A], False),
                        ([A, B], False), ([B, A], False), ([A, -2], True)):
        prots = [prot] * len(roles) + [others[A], others[B]]
        res, off = oracle_c.pack_strings(prots)
        all_roles = np.array(roles + [A, B], np.int32)
        keys, rl = kma.build_signatures(res, off, all_roles, k)
        got = dict(zip(_unpack(keys, k), rl.tolist()))
        km, erl = oracle_c.build_signatures(res, off, all_roles, k, 0)
        assert got == {bytes(r).decode(): int(v) for r, v in zip(km, erl)}, roles
        assert (shared in got) == kept, roles
        if kept:
            assert got[shared] == A
        assert got[others[A][:k]] == A and got[others[B][:k]] == B


# ---- 6. tally bound -------------------------------------------------------------------------------

SENTINEL = 0x5A5A5A5A
TALLY_N_FID = (1 << 21) + 1  # 2^21 is counted; 2^21 + 1 (== n_fid), 2^22 - 2 and 2^22 - 1 are not


def _tally_buffer(torch, dev, n):
    t = torch.zeros(n + 1024, dtype=torch.int32, device=dev)
    t[n:] = SENTINEL
    return t


@pytest.mark.parametrize("input_mode_", [0, 2], ids=["ascii", "packed"])
def test_protein_tally_stops_at_n_fid(kma, oracle_c, input_mode_):
    """The protein kernel drops a CALLED fid >= n_fid from the tally: with n_fid = 2^21 + 1 the
    head equals the oracle's counts of the fids below it and the 1,024 words after it keep their
    sentinel (the first of them is the word of the called fid n_fid itself)."""
    torch = pytest.importorskip("torch")
    c = apply_case(oracle_c, 8)
    efid, ecnt, est = c.mapped[0]
    called = efid[est == 1]
    assert (called >= TALLY_N_FID).sum() > 2 and (called == TALLY_N_FID).any()
    assert (called < TALLY_N_FID).sum() > 2 and (called == TALLY_N_FID - 1).any()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    kma.set_option(kma.OPT_PACKED_INPUT, input_mode_)
    n, n_res = len(c.off) - 1, int(c.off[-1])
    with kma.SignatureTable.from_packed(c.keys, c.fids, 8) as t:
        ws = kma.Workspace(0, n_res, n)
        res = torch.from_numpy(c.res.copy()).to(dev)
        off = torch.from_numpy(c.off.view(np.int64).copy()).to(dev)
        fid = torch.empty(n, dtype=torch.int32, device=dev)
        cnt = torch.empty(n, dtype=torch.int32, device=dev)
        st = torch.empty(n, dtype=torch.uint8, device=dev)
        tally = _tally_buffer(torch, dev, TALLY_N_FID)
        kma.annotate_proteins_device(t, ws, res.data_ptr(), off.data_ptr(), n, n_res, MIN_HITS, 0,
                                     fid.data_ptr(), cnt.data_ptr(), st.data_ptr(),
                                     tally.data_ptr(), TALLY_N_FID, stream)
        torch.cuda.synchronize()
        ws.close()
    assert (fid.cpu().numpy() == efid).all() and (st.cpu().numpy() == est).all()
    assert (cnt.cpu().numpy() == ecnt).all()
    got = tally.cpu().numpy().view(np.uint32)
    assert (got[TALLY_N_FID:] == SENTINEL).all()
    assert (got[:TALLY_N_FID] == np.bincount(called[called < TALLY_N_FID],
                                             minlength=TALLY_N_FID)).all()


@pytest.mark.parametrize("k", [8, 10])
def test_contig_tally_stops_at_n_fid(kma, oracle_c, small_gto, k):
    """The 6-frame kernel drops a hit fid >= n_fid from the [n_contig, n_fid] tally: no count
    lands in the next contig's row or past the end of the buffer."""
    torch = pytest.importorskip("torch")
    c = contig_case(oracle_c, small_gto, k)
    assert (c.e[4] >= TALLY_N_FID).sum() > 100 and (c.e[4] == TALLY_N_FID).any()
    assert (c.e[4] < TALLY_N_FID).sum() > 100 and (c.e[4] == TALLY_N_FID - 1).any()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    n_bases = int(c.off[-1])
    with kma.SignatureTable.from_packed(kma.pack_std(c.kmers), c.fids, k) as t:
        ws = kma.Workspace(0)
        ws.reserve_contigs(n_bases)
        d_dna = torch.from_numpy(c.dna.copy()).to(dev)
        d_off = torch.from_numpy(c.off.view(np.int64).copy()).to(dev)
        d_nh = torch.zeros(1, dtype=torch.int64, device=dev)
        cap = len(c.e[0]) + 16
        d_hits = torch.zeros(cap * kma.HIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        tally = _tally_buffer(torch, dev, c.n_contig * TALLY_N_FID)
        kma.annotate_contigs_device(t, ws, d_dna.data_ptr(), d_off.data_ptr(), c.n_contig, n_bases,
                                    11, d_hits.data_ptr(), cap, d_nh.data_ptr(), tally.data_ptr(),
                                    TALLY_N_FID, stream)
        torch.cuda.synchronize()
        ws.close()
    n = int(d_nh.item())
    assert n == len(c.e[0])
    _assert_hits(d_hits.cpu().numpy().view(kma.HIT_DTYPE)[:n], c.e)
    got = tally.cpu().numpy().view(np.uint32)
    assert (got[c.n_contig * TALLY_N_FID:] == SENTINEL).all()
    _assert_contig_tally(got[:c.n_contig * TALLY_N_FID], c.e, TALLY_N_FID, c.n_contig)


# ---- 7. creator limits ----------------------------------------------------------------------------

def test_creators_take_max_fid_and_refuse_the_next(kma):
    """kma_table_create / kma_table_create_packed: a fid of 2^22 is KMA_E_INVALID and the message
    names its row; 2^22 - 1 is stored and a lookup of its key returns it."""
    rows = ["ACDEFGHI", "KLMNPQRS", "TVWYACDE", "FGHIKLMN"]
    res, off = kma.pack_strings(rows + ["ACDEFGHI" + "KLMNPQRS"])
    for bad_row in (0, 2, 3):
        fids = np.array([7, N_FID - 1, 1 << 21, 3], np.uint32)
        fids[bad_row] = N_FID
        with pytest.raises(kma.KmerAnnoError) as e:
            kma.SignatureTable.from_rows(rows, fids, 8)
        assert e.value.code == kma.E_INVALID and f"row {bad_row}" in str(e.value)
        with pytest.raises(kma.KmerAnnoError) as e:
            kma.SignatureTable.from_packed(kma.pack_std(np.frombuffer(
                "".join(rows).encode(), np.uint8).reshape(4, 8)), fids, 8)
        assert e.value.code == kma.E_INVALID and f"row {bad_row}" in str(e.value)
    fids = np.array([7, N_FID - 1, 1 << 21, 3], np.uint32)
    keys = kma.pack_std(np.frombuffer("".join(rows).encode(), np.uint8).reshape(4, 8))
    for t in (kma.SignatureTable.from_rows(rows, fids, 8),
              kma.SignatureTable.from_packed(keys, fids, 8)):
        with t:
            fid, cnt, st, tally = kma.annotate_proteins(t, res, off, 1, 0, n_fid=N_FID)
        assert fid.tolist() == [7, N_FID - 1, 1 << 21, 3, -1]
        assert st.tolist() == [1, 1, 1, 1, 2] and cnt.tolist() == [1, 1, 1, 1, 0]
        assert tally[N_FID - 1] == 1 and tally.sum() == 4


def test_table_from_tsv_with_max_roles(kma, tmp_path):
    """kma_table_create_from_tsv on a kmerdb.tbl of 2^22 rows, each a new role id: 2^22 roles in
    first-seen order, the last row's kmer called with fid 2^22 - 1; one more role and the file is
    refused (KMA_E_INVALID)."""
    n, k = N_FID, 8
    aa = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
    i = np.arange(n, dtype=np.int64)
    rows = np.empty((n, k + 1 + 8 + 1), np.uint8)
    for j in range(k):  # row i's kmer: i in base 20, one residue per digit
        rows[:, k - 1 - j] = aa[(i // 20 ** j) % 20]
    rows[:, k] = ord("\t")
    rows[:, k + 1] = ord("R")
    for j in range(7):  # its role: R%07d
        rows[:, k + 8 - j] = 48 + (i // 10 ** j) % 10
    rows[:, k + 9] = ord("\n")
    path = tmp_path / "kmerdb.tbl"
    rows.tofile(path)
    first, last = rows[0, :k].tobytes().decode(), rows[-1, :k].tobytes().decode()
    del rows, i
    t, roles, last_len = kma.SignatureTable.from_tsv(str(path), k)
    with t:
        assert len(roles) == n and last_len == k
        assert roles[0] == "R0000000" and roles[-1] == f"R{n - 1:07d}"
        info = t.info
        assert (info.n_rows, info.n_entries, info.n_skipped) == (n, n, 0)
        res, off = kma.pack_strings([last, first, last + first])
        fid, cnt, st, tally = kma.annotate_proteins(t, res, off, 1, 0, n_fid=N_FID)
    assert fid.tolist() == [n - 1, 0, -1] and st.tolist() == [1, 1, 2]
    assert tally[n - 1] == 1 and tally[0] == 1 and tally.sum() == 2
    del roles
    with open(path, "ab") as f:
        f.write(b"YYYYYYYY\tone role more\n")
    with pytest.raises(kma.KmerAnnoError) as e:
        kma.SignatureTable.from_tsv(str(path), k)
    assert e.value.code == kma.E_INVALID and "roles" in str(e.value)
