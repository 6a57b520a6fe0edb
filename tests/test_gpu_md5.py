"""Sequence MD5 on the GPU (kma_sequence_md5, kma_sequence_md5_device; csrc/kma_md5.hip) against
hashlib.md5: RFC 1321 pins the digest, so the checker is the standard library and no restatement
of ours. Every case runs through the host entry and through the device entry (torch buffers in
the layout of annotate_proteins_device: 32 readable bytes after the last residue)."""
import hashlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
UPPER = 1
AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)


@pytest.fixture(scope="module")
def kma(native_lib):
    import kmeranno
    assert kmeranno.device_count() >= 1
    return kmeranno


def fold(b: bytes) -> bytes:
    return bytes(c - 32 if 97 <= c <= 122 else c for c in b)


def want(seqs, flags=0):
    out = np.zeros((len(seqs), 16), np.uint8)
    for i, s in enumerate(seqs):
        out[i] = np.frombuffer(hashlib.md5(fold(s) if flags & UPPER else s).digest(), np.uint8)
    return out


def device_md5(kma, res, off, flags=0, lo=0, hi=None, form=None):
    """The device entry on sequences lo .. hi of a batch; res holds offsets[-1] + 32 bytes."""
    hi = len(off) - 1 if hi is None else hi
    d_res = torch.from_numpy(np.ascontiguousarray(res)).cuda()
    d_off = torch.from_numpy(np.ascontiguousarray(off).view(np.int64)).cuda()
    d_dig = torch.full((max(hi - lo, 1), 16), 0xEE, dtype=torch.uint8, device="cuda")
    kma.sequence_md5_device(d_res.data_ptr(), d_off.data_ptr() + 8 * lo, hi - lo,
                            int(off[hi] - off[lo]), d_dig.data_ptr(), flags,
                            stream=torch.cuda.current_stream().cuda_stream, form=form)
    torch.cuda.synchronize()
    return d_dig.cpu().numpy()[:hi - lo]


def both(kma, seqs, flags=0):
    """Host and device digests of seqs, each equal to hashlib's."""
    exp = want(seqs, flags)
    res, off = kma.pack_strings(seqs)
    host = kma.sequence_md5(res, off, flags)
    dev = device_md5(kma, res, off, flags)
    bad = [i for i in range(len(seqs)) if (host[i] != exp[i]).any() or (dev[i] != exp[i]).any()]
    assert not bad, (bad[:10], [len(seqs[i]) for i in bad[:10]])
    return exp


def test_rfc1321_test_suite(kma):
    seqs = [b"", b"a", b"abc", b"message digest", b"abcdefghijklmnopqrstuvwxyz",
            b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789", b"1234567890" * 8]
    exp = both(kma, seqs)
    assert [bytes(d).hex() for d in exp[:3]] == ["d41d8cd98f00b204e9800998ecf8427e",
                                                 "0cc175b9c0f1b6a831c399e269772661",
                                                 "900150983cd24fb0d6963f7d28e17f72"]


def test_every_length_at_every_start_alignment(kma):
    """Lengths 0..130 (the padding edges 55 / 56 / 63 / 64 / 119 / 120 / 127 / 128 among them),
    each at every start address mod 8: a prefix sequence of 0..7 bytes shifts the starts of the
    131 that follow it (both entries read from an aligned base)."""
    rng = np.random.default_rng(5)
    seen = set()
    for shift in range(8):
        seqs = [rng.integers(0, 256, shift, dtype=np.uint8).tobytes()]
        seqs += [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in range(131)]
        starts = np.cumsum([0] + [len(s) for s in seqs[:-1]])
        seen |= {(len(s), int(a) % 8) for s, a in zip(seqs[1:], starts[1:])}
        both(kma, seqs)
    assert seen == {(n, a) for n in range(131) for a in range(8)}


def test_all_byte_values_next_to_the_padding(kma):
    every = bytes(range(256))
    seqs = [every, every[::-1], b"\x80" * 55, b"\x80" * 56, b"\x00" * 55, b"\x00" * 56,
            b"\x00" * 63 + b"\x80", b"\x80" + b"\x00" * 63, b"\xff" * 119, b"\x00" * 120,
            b"\x80\x00" * 64, b"\x00", b"\x80", b"\x00\x80\x00"]
    seqs += [every[i:] + every[:i] for i in (1, 2, 3, 127, 128, 129)]
    both(kma, seqs)
    both(kma, seqs, UPPER)


@pytest.mark.parametrize("n_seq", [0, 1, 63, 64, 65, 257])
def test_sequence_counts(kma, n_seq):
    rng = np.random.default_rng(n_seq)
    seqs = [AA[rng.integers(0, 20, rng.integers(0, 400))].tobytes() for _ in range(n_seq)]
    if n_seq:
        both(kma, seqs)
        return
    res, off = kma.pack_strings(seqs)
    assert kma.sequence_md5(res, off).shape == (0, 16)
    kma.sequence_md5_device(0, 0, 0, 0, 0)  # a no-op: nothing is read


@pytest.fixture(scope="module")
def refill_mix():
    """300 sequences of one to three blocks around one of 5,000 residues and one of 70,000."""
    rng = np.random.default_rng(70)
    seqs = [AA[rng.integers(0, 20, rng.integers(1, 184))].tobytes() for _ in range(300)]
    seqs.insert(100, AA[rng.integers(0, 20, 5000)].tobytes())
    seqs.insert(200, AA[rng.integers(0, 20, 70_000)].tobytes())
    return seqs, want(seqs)


def test_refill_mix_of_short_and_long_sequences(kma, refill_mix):
    seqs, exp = refill_mix
    res, off = kma.pack_strings(seqs)
    assert (kma.sequence_md5(res, off) == exp).all()
    assert (device_md5(kma, res, off) == exp).all()


@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_every_kernel_form_gives_the_same_digests(kma, refill_mix, form):
    """The forms kept for measurement (static lanes, loads through LDS) hash as the shipped one."""
    seqs, exp = refill_mix
    res, off = kma.pack_strings(seqs)
    assert (device_md5(kma, res, off, form=form) == exp).all()
    assert (device_md5(kma, res, off, UPPER, form=form) == want(seqs, UPPER)).all()


def test_sub_batch_inside_a_buffer_that_ends_32_bytes_after_it(kma):
    """offsets[0] != 0: sequences 3 .. n (and 3 .. 6) of a batch, through a device buffer that
    ends exactly 32 bytes past the batch's last residue."""
    rng = np.random.default_rng(32)
    seqs = [rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            for n in (5, 0, 8, 61, 64, 0, 57, 129, 1, 200, 3)]
    res, off = kma.pack_strings(seqs)
    assert len(res) == int(off[-1]) + 32 and off[3] == 13
    got = device_md5(kma, res, off, lo=3)
    assert (got == want(seqs[3:])).all()
    got = device_md5(kma, res, off, lo=3, hi=7)
    assert (got == want(seqs[3:7])).all()


def test_upper_folds_a_to_z_only(kma):
    rng = np.random.default_rng(26)
    mixed = [bytes(rng.choice(np.frombuffer(b"acdefghiklmnpqrstvwyACDEFGHIKLMNPQRSTVWY", np.uint8),
                              n)) for n in (1, 7, 55, 56, 64, 65, 300)]
    edge = [b"`{", b"`az{@AZ[", bytes(range(0x5f, 0x7d)), bytes(range(0x80, 0x100)),
            bytes(c | 0x80 for c in b"abcxyz") + b"abcxyz", bytes(range(256))]
    exp = both(kma, mixed + edge, UPPER)
    plain = both(kma, mixed + edge, 0)
    assert (exp[:len(mixed)] == want([s.upper() for s in mixed])).all()
    assert (exp[len(mixed)] == plain[len(mixed)]).all()  # ` and { are not letters
    assert (exp[len(mixed) + 3] == plain[len(mixed) + 3]).all()  # bytes >= 0x80 do not fold
    lower = [i for i, s in enumerate(mixed) if s != s.upper()]
    assert len(lower) >= 5 and (exp[lower] != plain[lower]).any(axis=1).all()


def test_small_gto_pegs(kma, small_gto):
    prots = [f["protein_translation"].encode() for f in small_gto["features"]
             if f.get("protein_translation")]
    assert len(prots) == 712
    both(kma, prots)
    both(kma, [p.lower() if i % 2 else p for i, p in enumerate(prots)], UPPER)


def test_device_entry_in_a_captured_graph(kma, refill_mix):
    """The call is one kernel with no state of its own: captured once, replayed twice into a
    cleared output, it gives the digests each time."""
    seqs, exp = refill_mix
    res, off = kma.pack_strings(seqs)
    n = len(seqs)
    d_res = torch.from_numpy(res).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    d_dig = torch.zeros((n, 16), dtype=torch.uint8, device="cuda")

    def call():
        kma.sequence_md5_device(d_res.data_ptr(), d_off.data_ptr(), n, int(off[-1]),
                                d_dig.data_ptr(), 0,
                                stream=torch.cuda.current_stream().cuda_stream)

    call()  # (the module is loaded before the capture)
    torch.cuda.synchronize()
    first = d_dig.cpu().numpy().copy()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    outs = []
    for _ in range(2):
        d_dig.zero_()
        graph.replay()
        torch.cuda.synchronize()
        outs.append(d_dig.cpu().numpy().copy())
    assert (first == exp).all() and (outs[0] == exp).all() and (outs[1] == outs[0]).all()
