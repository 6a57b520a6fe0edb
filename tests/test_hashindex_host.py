"""Host side of the hash annotator's resident prototype index (no GPU).

kmers.anno_amd/host/hashindex_check.cpp is a stand-alone program built with
-fsanitize=address,undefined that runs a serial model of one block of the score kernel from the
pieces the kernel itself is made of (csrc/kma_hashindex.h: the slot hash and table size, the
lower bound in the postings, the prefix owner of a flattened posting, the range stack, the best /
tie rule, the similarity) against a brute-force count over all pairs, from heap arrays of exactly
the index's sizes. The case files are written here, with expectations from a plain Python set
model; the test builds and runs the program. The entry points' argument checks come back
KMA_E_INVALID before any device is touched, and the new symbols are exported."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import PKG

EXE = os.path.join(PKG, "build", "kma_hashindex_check")


def make_case(seed, n_proto, n_genome, universe, hot):
    """Key lists over a small universe: `hot` keys are held by most prototypes (long postings,
    many candidates per protein), some genome proteins are copies of prototypes (ties and 1.0),
    some share nothing, some are empty, and one is longer than several 256-key chunks."""
    rng = np.random.default_rng(seed)
    protos = []
    for p in range(n_proto):
        keys = rng.integers(hot, universe, rng.integers(0, 60)).tolist()
        if p % 4:
            keys += rng.integers(0, hot, rng.integers(1, 4)).tolist()
        protos.append(keys + keys[:3])  # repeats: the set is their distinct values
    for p in (5, n_proto // 2, n_proto - 1):  # exact copies: equal similarity, the earlier wins
        protos[p] = list(protos[2])
    genome = []
    for g in range(n_genome):
        kind = g % 6
        if kind == 0:
            keys = list(protos[rng.integers(0, n_proto)])
        elif kind == 1:
            keys = rng.integers(universe, 2 * universe, 40).tolist()  # shares nothing
        elif kind == 2:
            keys = []
        else:
            keys = rng.integers(0, universe, rng.integers(1, 120)).tolist()
        genome.append(keys)
    genome.append(rng.integers(0, universe, 1500).tolist())  # six chunks of 256 positions
    genome.append(list(protos[2]))
    return protos, genome


def expectations(protos, genome, min_sim):
    psets = [set(p) for p in protos]
    out = []
    for g in genome:
        gs = set(g)
        best, best_sim, shared, cand = -1, 0.0, 0, 0
        for p, ps in enumerate(psets):
            c = len(gs & ps)
            if not c:
                continue
            cand += 1
            sim = c / (len(ps) + len(gs) - c)
            if sim >= min_sim and (best < 0 or sim > best_sim):
                best, best_sim, shared = p, sim, c
        out.append((best, shared, cand))
    return out


def write_case(path, protos, genome, cap, min_sim, expect):
    with open(path, "wb") as f:
        f.write(struct.pack("<IIIId", len(protos), len(genome), cap, 0, min_sim))
        for keys in protos + genome:
            f.write(struct.pack("<I", len(keys)) + np.asarray(keys, np.uint64).tobytes())
        for best, shared, cand in expect:
            f.write(struct.pack("<iII", best, shared, cand))


def run_check(path):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    return subprocess.run([EXE, str(path)], capture_output=True, text=True, env=env, timeout=120)


@pytest.fixture(scope="module")
def check_program(native_lib):
    subprocess.run(["make", "-s", "-C", PKG, "build/kma_hashindex_check"], check=True)
    return EXE


@pytest.fixture(scope="module")
def case():
    protos, genome = make_case(41, 600, 60, 3000, 6)
    return protos, genome, expectations(protos, genome, 0.0125)


@pytest.mark.parametrize("cap", [2048, 64, 4, 1])
def test_block_model_against_brute_force_under_sanitizers(check_program, case, tmp_path, cap):
    """The table fits every protein at CAP 2048; at 64, 4 and 1 the proteins holding a hot key
    overflow and are scored in halved prototype ranges, with the copies of prototype 2 in
    different ranges. The split count is the set model's."""
    protos, genome, expect = case
    path = tmp_path / "case.bin"
    write_case(path, protos, genome, cap, 0.0125, expect)
    r = run_check(path)
    assert r.returncode == 0, r.stdout + r.stderr
    n_split = sum(cand > cap for _, _, cand in expect)
    assert (n_split == 0) == (cap == 2048) and max(c for _, _, c in expect) > 64
    assert f"hashindex_check ok: {len(protos)} prototypes, {len(genome)} proteins, " \
           f"{n_split} split, " in r.stdout
    assert expect[-1][0] == 2 and expect[-1][1] == len(set(protos[2]))


def test_block_model_check_fails_on_a_wrong_count(check_program, case, tmp_path):
    """The program compares: an expected shared count off by one fails it."""
    protos, genome, expect = case
    bad = list(expect)
    g = next(i for i, e in enumerate(bad) if e[0] >= 0)
    bad[g] = (bad[g][0], bad[g][1] + 1, bad[g][2])
    path = tmp_path / "bad.bin"
    write_case(path, protos, genome, 64, 0.0125, bad)
    r = run_check(path)
    assert r.returncode == 1 and "wrong count" in r.stderr


def test_exports_present(native_lib):
    import kmeranno
    for name in ("kma_proto_index_create", "kma_proto_index_info", "kma_proto_index_destroy",
                 "kma_hash_annotate_indexed"):
        assert name in kmeranno.EXPORTS and hasattr(native_lib, name)
    assert native_lib.kma_abi_version() == 7
    assert kmeranno.OPT_HASH_CAP == 12 and kmeranno.get_option(kmeranno.OPT_HASH_CAP) == 0
    with pytest.raises(kmeranno.KmerAnnoError):
        kmeranno.get_option(11)  # no option has this number (tests/test_abi.py sets it in vain)
    for bad in (-1, 2049):
        with pytest.raises(kmeranno.KmerAnnoError):
            kmeranno.set_option(kmeranno.OPT_HASH_CAP, bad)
    with kmeranno.options(hash_cap=4):
        assert kmeranno.get_option(kmeranno.OPT_HASH_CAP) == 4
    assert kmeranno.get_option(kmeranno.OPT_HASH_CAP) == 0


def _err(native_lib):
    return native_lib.kma_last_error().decode()


def test_invalid_arguments_come_back_without_a_device(native_lib):
    """Null index or outputs, decreasing offsets, k and min_sim out of range are KMA_E_INVALID
    with a message, from checks that run before the device is entered (device 12345 does not
    exist: a call that got as far as the device would be KMA_E_DEVICE)."""
    import ctypes as C
    import kmeranno as k
    L, dev = native_lib, 12345
    res = np.frombuffer(b"MKVLAAGIVALLMKVLAAGIV" + b"\0" * 32, np.uint8).copy()
    off = np.array([0, 12, 21], np.uint64)
    down = np.array([0, 13, 12], np.uint64)
    best, sim = np.zeros(2, np.int32), np.zeros(2, np.float64)
    cnt, stats = np.zeros(2, np.uint32), np.zeros(3, np.uint64)

    def p(a):
        return a.ctypes.data

    h = C.c_void_p()
    create = L.kma_proto_index_create
    for rc in (create(p(res), p(off), 2, 8, dev, None), create(None, p(off), 2, 8, dev, C.byref(h)),
               create(p(res), None, 2, 8, dev, C.byref(h)),
               create(p(res), p(down), 2, 8, dev, C.byref(h)),
               create(p(res), p(off), 2, 1, dev, C.byref(h)),
               create(p(res), p(off), 2, 13, dev, C.byref(h))):
        assert rc == k.E_INVALID and not h.value
    assert create(p(res), p(down), 2, 8, dev, C.byref(h)) == k.E_INVALID
    assert "prototype offsets decrease at 1" in _err(L)
    assert create(p(res), p(off), 2, 13, dev, C.byref(h)) == k.E_INVALID and "2..12" in _err(L)
    # a well-formed request reaches the device that is not there
    assert create(p(res), p(off), 2, 8, dev, C.byref(h)) == k.E_DEVICE and not h.value
    # an index of no prototypes touches no device: every call on it is decided on the host
    assert create(None, p(off), 0, 8, dev, C.byref(h)) == k.OK and h.value
    info = k.ProtoIndexInfo()
    assert L.kma_proto_index_info(h, C.byref(info)) == k.OK
    assert (info.n_proto, info.k, info.n_keys, info.n_postings, info.bytes) == (0, 8, 0, 0, 0)
    assert L.kma_proto_index_info(None, C.byref(info)) == k.E_INVALID
    assert L.kma_proto_index_info(h, None) == k.E_INVALID
    anno = L.kma_hash_annotate_indexed
    for rc in (anno(None, p(res), p(off), 2, 0.1, p(best), p(sim), p(cnt), p(stats)),
               anno(h, p(res), p(off), 2, 0.1, None, p(sim), p(cnt), p(stats)),
               anno(h, p(res), p(off), 2, 0.1, p(best), None, p(cnt), p(stats)),
               anno(h, None, p(off), 2, 0.1, p(best), p(sim), p(cnt), p(stats)),
               anno(h, p(res), None, 2, 0.1, p(best), p(sim), p(cnt), p(stats)),
               anno(h, p(res), p(down), 2, 0.1, p(best), p(sim), p(cnt), p(stats)),
               anno(h, p(res), p(off), 2, 1.0, p(best), p(sim), p(cnt), p(stats)),
               anno(h, p(res), p(off), 2, -0.5, p(best), p(sim), p(cnt), p(stats)),
               anno(h, p(res), p(off), 2, float("nan"), p(best), p(sim), p(cnt), p(stats))):
        assert rc == k.E_INVALID
    assert anno(None, p(res), p(off), 2, 0.1, p(best), p(sim), p(cnt), None) == k.E_INVALID
    assert "null index" in _err(L)
    assert anno(h, p(res), p(down), 2, 0.1, p(best), p(sim), p(cnt), None) == k.E_INVALID
    assert "genome protein offsets decrease at 1" in _err(L)
    # no prototypes: every protein keeps the default proposal, out_stats optional
    best[:], sim[:], stats[:] = 7, 7.0, 7
    assert anno(h, p(res), p(off), 2, 0.1, p(best), p(sim), None, p(stats)) == k.OK
    assert best.tolist() == [-1, -1] and sim.tolist() == [0.0, 0.0] and stats.tolist() == [0, 0, 0]
    assert anno(h, p(res), p(off), 2, 0.1, p(best), p(sim), None, None) == k.OK
    assert L.kma_proto_index_destroy(h) == k.OK
    assert L.kma_proto_index_destroy(None) == k.OK


def test_python_wrappers_refuse_before_the_device(native_lib):
    import kmeranno as k
    res, off = k.pack_strings(["MKVLAAGIVALL", "LAAGMKVLAAGIV"])
    with pytest.raises(k.KmerAnnoError) as e:
        k.ProtoIndex(res, off, k=1, device=12345)
    assert e.value.code == k.E_INVALID
    with pytest.raises(k.KmerAnnoError) as e:
        k.ProtoIndex(res, off[::-1].copy(), device=12345)
    assert e.value.code == k.E_INVALID
    with k.ProtoIndex.from_strings([], device=12345) as idx:
        assert idx.info().n_proto == 0 and idx.info().k == 8
        best, sim, cnt, st = k.hash_annotate_indexed(idx, res, off, stats=True)
        assert best.tolist() == [-1, -1] and sim.tolist() == [0.0, 0.0] and len(cnt) == 0
        with pytest.raises(k.KmerAnnoError) as e:
            k.hash_annotate_indexed(idx, res, off, min_sim=1.0)
        assert e.value.code == k.E_INVALID
    with pytest.raises(k.KmerAnnoError):
        idx.info()  # closed


def test_command_refuses_bad_arguments(tmp_path, native_lib):
    """minLen < K, a bad minSim and a missing input directory are refused before anything runs."""
    from kmeranno import hashanno
    anno = tmp_path / "anno.tbl"
    anno.write_text("protein\tannotation\n" + "M" * 60 + "\trole\n")
    (tmp_path / "in").mkdir()
    for extra in (["-K", "8", "--minLen", "7"], ["--minSim", "1.0"], ["-K", "1"]):
        with pytest.raises(SystemExit):
            hashanno.main([str(anno), str(tmp_path / "in")] + extra)
    with pytest.raises(SystemExit):
        hashanno.main([str(anno), str(tmp_path / "nowhere")])
    rows = hashanno.read_annotation_file(str(anno))
    assert rows == [("M" * 60, "role")]
