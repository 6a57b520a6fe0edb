"""Host side of the indexed hash annotator's device entry (no GPU).

kmers.anno_amd/host/hashsets_check.cpp is a stand-alone program built with
-fsanitize=address,undefined that runs a serial model of one block of genome_sets_kernel from the
pieces the kernel itself is made of (csrc/kma_hashsets.h: the code LUT and window key, the padded
size, the compare-exchange partner and direction of a bitonic step, the head rule across the runs
of a long protein) against a brute-force set of substrings, on heap arrays of exactly the sizes
the kernel touches. The case files are written here, with the set sizes from a plain Python set;
the test builds and runs the program. The new entry's argument checks come back KMA_E_INVALID
before any device is touched, the scratch size is monotone, and the new symbols and the new
option are there."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import PKG

EXE = os.path.join(PKG, "build", "kma_hashsets_check")
AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)


def _rand(rng, n):
    return AA[rng.integers(0, 20, n)].tobytes()


def set_size(s, k):
    return len({s[i:i + k] for i in range(len(s) - k + 1)})


def in_windows(s, k):
    """Whether a byte outside A-Z / '*' lies in a window (any byte of a protein of >= k)."""
    ok = set(b"ABCDEFGHIJKLMNOPQRSTUVWXYZ*")
    return int(len(s) >= k and any(b not in ok for b in s))


def repeat_in_runs_0_and_2(rng, w, k):
    """3W windows; 20 residues of chunk 0 come again in chunk 2 and nowhere in chunk 1."""
    s = bytearray(_rand(rng, 3 * w + k - 1))
    s[2 * w + 11:2 * w + 31] = s[5:25]
    s = bytes(s)
    rep = {s[i:i + k] for i in range(5, 25 - k + 1)}
    run = [{s[i:i + k] for i in range(c * w, (c + 1) * w)} for c in range(3)]
    assert rep <= run[0] and rep <= run[2] and (k < 4 or not rep & run[1])
    return s


def cases_for(w, seed):
    rng = np.random.default_rng(seed)
    out = []
    for n_win in (0, 1, w - 1, w, w + 1, 2 * w, 2 * w + 1, 5 * w + 37):
        out.append((w, 8, _rand(rng, n_win + 7 if n_win else 5)))
    out.append((w, 8, b""))
    out.append((w, 8, b"W" * (2 * w + 50)))  # one distinct key, present in every run
    out.append((w, 8, b"GGS" * w))           # three distinct keys over three runs
    for k in (2, 8, 12):
        out.append((w, k, repeat_in_runs_0_and_2(rng, w, k)))
        out.append((w, k, _rand(rng, w + k)))             # W + 1 windows
        out.append((w, k, _rand(rng, 5 * w + 11 + k)))
        out.append((w, k, _rand(rng, k - 1)))
        out.append((w, k, _rand(rng, k)))
    out.append((w, 8, _rand(rng, 40) + b"k" + _rand(rng, w + 40)))  # a byte without a code
    out.append((w, 8, b"acd"))                                     # ... in no window
    out.append((w, 8, b"MKV*LAAG*IVALLMKV*"))
    return out


def write_cases(path, cases, sizes=None):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for i, (w, k, s) in enumerate(cases):
            size = set_size(s, k) if sizes is None else sizes[i]
            f.write(struct.pack("<IIIII", w, k, len(s), size, in_windows(s, k)) + s)


def run_check(path):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    return subprocess.run([EXE, str(path)], capture_output=True, text=True, env=env, timeout=120)


@pytest.fixture(scope="module")
def check_program(native_lib):
    subprocess.run(["make", "-s", "-C", PKG, "build/kma_hashsets_check"], check=True)
    return EXE


@pytest.mark.parametrize("w", [64, 256, 4096])
def test_block_model_against_brute_force_under_sanitizers(check_program, tmp_path, w):
    """Window counts 0, 1, W - 1, W, W + 1, 2W, 2W + 1 and ~5W; one repeated residue; a repeat
    that recurs only in runs 0 and 2; K = 2, 8, 12; bytes without a code in and out of windows."""
    cases = cases_for(w, 100 + w)
    assert set_size(cases[9][2], 8) == 1 and set_size(cases[10][2], 8) == 3
    path = tmp_path / "cases.bin"
    write_cases(path, cases)
    r = run_check(path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"hashsets_check ok: {len(cases)} cases, " in r.stdout


def test_block_model_check_fails_on_a_wrong_size(check_program, tmp_path):
    """The program compares: one expected size off by one makes it exit 1."""
    cases = cases_for(64, 7)
    sizes = [set_size(s, k) for _, k, s in cases]
    sizes[7] += 1  # the ~5W case
    path = tmp_path / "bad.bin"
    write_cases(path, cases, sizes)
    r = run_check(path)
    assert r.returncode == 1 and "case 7: wrong size" in r.stderr


def test_exports_and_option(native_lib):
    import kmeranno as k
    for name in ("kma_hash_scratch_bytes", "kma_hash_annotate_indexed_device"):
        assert name in k.EXPORTS and hasattr(native_lib, name)
    assert native_lib.kma_abi_version() == 7
    assert k.OPT_HASH_LDS_KEYS == 13 and k.get_option(13) == 0 and k.OPT_DEFAULTS[13] == 0
    for good in (64, 4096, 512, 0):
        k.set_option(k.OPT_HASH_LDS_KEYS, good)
        assert k.get_option(k.OPT_HASH_LDS_KEYS) == good
    for bad in (63, 96, 32, 8192, -64):
        with pytest.raises(k.KmerAnnoError) as e:
            k.set_option(k.OPT_HASH_LDS_KEYS, bad)
        assert e.value.code == k.E_INVALID and k.get_option(k.OPT_HASH_LDS_KEYS) == 0
    with k.options(hash_lds_keys=128):
        assert k.get_option(k.OPT_HASH_LDS_KEYS) == 128
    assert k.get_option(k.OPT_HASH_LDS_KEYS) == 0
    for call in (lambda: k.get_option(11), lambda: k.set_option(11, 0), lambda: k.get_option(14)):
        with pytest.raises(k.KmerAnnoError):
            call()  # 11 is still no option


def test_scratch_bytes_is_monotone_and_covers_its_parts(native_lib):
    import kmeranno as k
    sizes = [0, 1, 3, 4, 5, 1000, 1001, 1 << 20, (1 << 31) - 1]
    counts = [0, 1, 2, 3, 4, 5, 4000, 1 << 20, (1 << 32) - 1]
    grid = [[k.hash_scratch_bytes(r, g) for g in counts] for r in sizes]
    for i, r in enumerate(sizes):
        for j, g in enumerate(counts):
            assert grid[i][j] >= 4 * r + 4 * g
            assert grid[i][j] <= 12 * r + 4 * g + 64  # at most 8 B per position for the runs
            assert i == 0 or grid[i][j] >= grid[i - 1][j]
            assert j == 0 or grid[i][j] >= grid[i][j - 1]


def test_invalid_arguments_come_back_without_a_device(native_lib):
    """Every refusal of the device entry, from an index of no prototypes on a device that does
    not exist and fake non-null pointers: a call that got as far as the device would be
    KMA_E_DEVICE."""
    import kmeranno as k
    L = native_lib
    off = np.array([0], np.uint64)
    h = C.c_void_p()
    assert L.kma_proto_index_create(None, off.ctypes.data, 0, 8, 12345, C.byref(h)) == k.OK
    n_g, n_r = 3, 100
    need = k.hash_scratch_bytes(n_r, n_g)
    good = dict(index=h, res=0x1000, off=0x2000, n_g=n_g, n_r=n_r, min_sim=0.1, scratch=0x3000,
                sbytes=need, best=0x4000, sim=0x5000, count=0x6000, stats=0x7000)

    def call(**kw):
        a = dict(good, **kw)
        return L.kma_hash_annotate_indexed_device(
            a["index"], a["res"] or None, a["off"] or None, a["n_g"], a["n_r"], a["min_sim"],
            a["scratch"] or None, a["sbytes"], a["best"] or None, a["sim"] or None,
            a["count"] or None, a["stats"] or None, None)

    refused = [(dict(index=None), "null index"),
               (dict(res=0), "null argument"), (dict(off=0), "null argument"),
               (dict(scratch=0), "null argument"),
               (dict(best=0), "null output"), (dict(sim=0), "null output"),
               (dict(stats=0), "null output"),
               (dict(res=0x1004), "d_residues is not 8-byte aligned"),
               (dict(scratch=0x3008), "d_scratch is not 16-byte aligned"),
               (dict(sbytes=need - 1), f"scratch of {need - 1} bytes, {need} needed"),
               (dict(n_r=1 << 31, sbytes=1 << 40), "more than 2^31 genome protein residues"),
               (dict(min_sim=1.0), "between 0 and 1"), (dict(min_sim=-0.5), "between 0 and 1"),
               (dict(min_sim=float("nan")), "between 0 and 1")]
    for kw, msg in refused:
        assert call(**kw) == k.E_INVALID, kw
        assert msg in L.kma_last_error().decode(), kw
    # a well-formed request reaches the device that is not there (d_count may be null here: the
    # index has no prototypes); no protein: nothing to do, whatever the pointers
    assert call(count=0) == k.E_DEVICE
    assert call(n_g=0, n_r=0, res=0, off=0, scratch=0, sbytes=0, best=0, sim=0, count=0,
                stats=0) == k.OK
    with pytest.raises(k.KmerAnnoError) as e:
        with k.ProtoIndex.from_strings([], device=12345) as idx:
            k.hash_annotate_indexed_device(idx, 0x1000, 0x2000, n_g, n_r, 0x3008, need, 0x4000,
                                           0x5000, 0, 0x7000)
    assert e.value.code == k.E_INVALID and "16-byte" in str(e.value)
    assert L.kma_proto_index_destroy(h) == k.OK
