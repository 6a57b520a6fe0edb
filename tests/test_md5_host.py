"""Host side of the sequence MD5 (no GPU).

kmers.anno_amd/host/md5_check.cpp is a stand-alone program built with
-fsanitize=address,undefined that runs the per-lane body of the MD5 kernel (csrc/kma_md5.h: the
aligned reads with their carried word, the branch-free message words, the 64 steps) on the CPU:
every record of a file written here with hashlib (flags, sequence, expected digest) at each start
alignment 0..7, alone and in one batch, from heap buffers of exactly the device call's contract
(32 bytes after the last residue), and the tail words of lengths of 2^29 - 1, 2^29, 2^32 + 5 and
2^35 + 3 bytes. The test builds and runs it. The entry points' argument checks come back
KMA_E_INVALID before any device is touched, and the new symbols are exported."""
import hashlib
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import PKG

UPPER = 1


def fold(b: bytes) -> bytes:
    return bytes(c - 32 if 97 <= c <= 122 else c for c in b)


def records():
    rng = np.random.default_rng(1321)
    out = []
    for s in (b"", b"a", b"abc", b"message digest", b"abcdefghijklmnopqrstuvwxyz",
              b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789",
              b"1234567890" * 8):  # RFC 1321 A.5
        out.append((0, s))
    every = bytes(range(256))
    for n in range(0, 131):  # every padding edge: 55 / 56 / 63 / 64 / 119 / 120 / 127 / 128
        out.append((0, rng.integers(0, 256, n, dtype=np.uint8).tobytes()))
        out.append((UPPER, (every * 2)[200 - n // 2:200 - n // 2 + n]))
    out.append((0, every))
    out.append((UPPER, every))
    out.append((0, b"\x80" * 55))
    out.append((0, b"\x00" * 56))
    out.append((UPPER, b"mkvLAAGiVaLL`{z@[aZ\xe1\xfa"))
    for n in (5000, 70_000):
        out.append((n & 1, rng.integers(0, 256, n, dtype=np.uint8).tobytes()))
    return out


def test_md5_body_against_hashlib_under_sanitizers(native_lib, tmp_path):
    subprocess.run(["make", "-s", "-C", PKG, "build/kma_md5_check"], check=True)
    recs = records()
    path = tmp_path / "records.bin"
    with open(path, "wb") as f:
        for flags, s in recs:
            want = hashlib.md5(fold(s) if flags & UPPER else s).digest()
            f.write(struct.pack("<II", flags, len(s)) + s + want)
    exe = os.path.join(PKG, "build", "kma_md5_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"md5_check ok: {len(recs)} records, {9 * len(recs)} digests, 10 tails" in r.stdout


def test_md5_body_check_fails_on_a_wrong_digest(native_lib, tmp_path):
    """The program compares: a record whose expected digest is off by one bit fails it."""
    subprocess.run(["make", "-s", "-C", PKG, "build/kma_md5_check"], check=True)
    want = bytearray(hashlib.md5(b"abc").digest())
    want[15] ^= 1
    path = tmp_path / "bad.bin"
    path.write_bytes(struct.pack("<II", 0, 3) + b"abc" + bytes(want))
    r = subprocess.run([os.path.join(PKG, "build", "kma_md5_check"), str(path)],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "wrong digest" in r.stderr


def test_exports_present(native_lib):
    import kmeranno
    for name in ("kma_sequence_md5_device", "kma_sequence_md5", "kma_check_sequences"):
        assert name in kmeranno.EXPORTS and hasattr(native_lib, name)
    assert native_lib.kma_abi_version() == 7


def _err(native_lib):
    return native_lib.kma_last_error().decode()


def test_invalid_arguments_come_back_without_a_device(native_lib):
    """Null arguments, decreasing offsets, unknown flag bits and more than 2^32 - 128 residues are
    KMA_E_INVALID with a message, from checks that run before the device is entered (device
    12345 does not exist: a call that got as far as the device would be KMA_E_DEVICE)."""
    import kmeranno as k
    L, dev = native_lib, 12345
    res = np.frombuffer(b"MKVLAAGIV" + b"\0" * 32, np.uint8).copy()
    off = np.array([0, 4, 9], np.uint64)
    dig = np.zeros((2, 16), np.uint8)
    rep, size = np.zeros(2, np.int32), np.zeros(2, np.uint32)
    mixed, stats = np.zeros(2, np.uint8), np.zeros(3, np.uint64)

    def p(a):
        return a.ctypes.data

    down = np.array([0, 5, 4], np.uint64)
    big = np.array([0, 4, (1 << 32) - 127], np.uint64)

    def host(r, o, n, flags, out):
        return L.kma_sequence_md5(r, o, n, flags, dev, out)

    def check(r, o, n, flags, out_rep=p(rep), out_size=p(size), out_mixed=p(mixed),
              out_stats=p(stats)):
        return L.kma_check_sequences(r, o, n, flags, None, dev, None, out_rep, out_size,
                                     out_mixed, out_stats)

    cases = [
        host(None, p(off), 2, 0, p(dig)), host(p(res), None, 2, 0, p(dig)),
        host(p(res), p(off), 2, 0, None), host(p(res), p(down), 2, 0, p(dig)),
        host(p(res), p(off), 2, 2, p(dig)), host(p(res), p(big), 2, 0, p(dig)),
        check(None, p(off), 2, 0), check(p(res), None, 2, 0),
        check(p(res), p(off), 2, 0, out_rep=None), check(p(res), p(off), 2, 0, out_size=None),
        check(p(res), p(off), 2, 0, out_mixed=None), check(p(res), p(off), 2, 0, out_stats=None),
        check(p(res), p(down), 2, 0), check(p(res), p(off), 2, 0x10),
        check(p(res), p(big), 2, 0),
        # the device entry: fake but aligned device addresses, never dereferenced
        L.kma_sequence_md5_device(dev, None, 4096, 2, 9, 0, 8192, None),
        L.kma_sequence_md5_device(dev, 4096, None, 2, 9, 0, 8192, None),
        L.kma_sequence_md5_device(dev, 4096, 4096, 2, 9, 0, None, None),
        L.kma_sequence_md5_device(dev, 4096, 4096, 2, 9, 4, 8192, None),
        L.kma_sequence_md5_device(dev, 4096, 4096, 2, (1 << 32) - 127, 0, 8192, None),
        L.kma_sequence_md5_device(dev, 4097, 4096, 2, 9, 0, 8192, None),
        L.kma_sequence_md5_device(dev, 4096, 4096, 2, 9, 0, 8200, None),
    ]
    for i, rc in enumerate(cases):
        assert rc == k.E_INVALID, i
    # (kma_last_error holds the last call's message: one case of each kind again, read at once)
    assert host(p(res), p(down), 2, 0, p(dig)) == k.E_INVALID and "decrease at 1" in _err(L)
    assert host(p(res), p(off), 2, 2, p(dig)) == k.E_INVALID and "flag" in _err(L)
    assert check(p(res), p(big), 2, 0) == k.E_INVALID and "2^32 - 128" in _err(L)
    assert check(None, p(off), 2, 0) == k.E_INVALID and "null" in _err(L)
    assert L.kma_sequence_md5_device(dev, 4097, 4096, 2, 9, 0, 8192, None) == k.E_INVALID
    assert "aligned" in _err(L)
    # the largest legal batch passes the checks and fails at the device that is not there
    assert L.kma_sequence_md5_device(dev, 4096, 4096, 2, (1 << 32) - 128, 1, 8192,
                                     None) == k.E_DEVICE
    assert _err(L)
    # n_seq == 0 is a no-op that returns KMA_OK on every entry, whatever the device
    assert L.kma_sequence_md5_device(dev, None, None, 0, 0, 0, None, None) == k.OK
    assert host(None, p(off), 0, 0, None) == k.OK
    assert check(None, p(off), 0, 0, None, None, None) == k.OK


def test_python_wrappers_refuse_before_the_device(native_lib):
    import kmeranno as k
    res, off = k.pack_strings(["MKV", "LAAG"])
    with pytest.raises(k.KmerAnnoError) as e:
        k.sequence_md5(res, off, flags=8, device=12345)
    assert e.value.code == k.E_INVALID
    with pytest.raises(k.KmerAnnoError) as e:
        k.check_sequences(res, off, fun=[1], device=12345)
    assert e.value.code == k.E_INVALID
    with pytest.raises(k.KmerAnnoError) as e:
        k.check_sequences(res, off[::-1].copy(), device=12345)
    assert e.value.code == k.E_INVALID
    assert len(k.sequence_md5(res[:0], off[:1], device=12345)) == 0
