"""The duplicate check's grouping at scale and on chosen digests (tests/seqcheck_cases.py has the
cases and their references; tests/test_seqcheck_workload.py shows on the CPU that they aim
right). Everything is compared for exact equality: rep, size, mixed and the three counts.

Probe tests: kmers.anno_amd/build/kma_seqcheck_probe (host/seqcheck_probe.hip, the library's
own kma_md5.o under a main) runs kma::launch_seq_check on the crafted records, all in one child
process, against the dict grouping. They pin what real MD5 digests cannot: digests equal in one
64-bit half, in three words, in all but one bit are different groups, and a run's members stay
in input order. KMA_SEQCHECK_PROBE names another build of the program (a mutation run of the
suite; with KMERANNO_LIB for the library).

Entry tests: kmeranno.check_sequences on sequences made from group ids, against np.unique over
the ids: 2^20 (rocPRIM's last merge-sort size), 2^20 + 1 (the first onesweep size) and
2,500,000 sequences with 10% empty ones, all above the MD5 kernel's grid cap; sequence counts at
the wave, block and sort-path edges; views that start inside a batch; lower-case copies under
both flags; and the function ids 0 and 0xFFFFFFFF inside groups."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import seqcheck_cases as sc
from conftest import PKG

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kma(native_lib):
    import kmeranno
    assert kmeranno.device_count() >= 1
    return kmeranno


def probe_program():
    exe = os.environ.get("KMA_SEQCHECK_PROBE")
    if not exe:
        subprocess.run(["make", "-s", "-C", PKG, "build/kma_seqcheck_probe"], check=True)
        exe = os.path.join(PKG, "build", "kma_seqcheck_probe")
    return exe


@pytest.fixture(scope="module")
def probe_results(native_lib, tmp_path_factory):
    """{record name: (record, (rep, size, mixed, stats))}: one run of the probe program over all
    crafted records."""
    exe = probe_program()
    tmp = tmp_path_factory.mktemp("seqcheck_probe")
    records = sc.probe_records()
    sc.write_records(tmp / "records.bin", records)
    r = subprocess.run([exe, str(tmp / "records.bin"), str(tmp / "out.bin")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"seqcheck_probe ok: {len(records)} records" in r.stdout
    got = sc.read_results(tmp / "out.bin", records)
    return {rec.name: (rec, g) for rec, g in zip(records, got)}


def assert_equal(got, want, what):
    for name, g, w in zip(("rep", "size", "mixed"), got, want):
        wrong = np.flatnonzero(np.asarray(g) != np.asarray(w))
        assert len(wrong) == 0, (f"{what}: {name} wrong at {len(wrong)} of {len(w)}, first "
                                 f"{wrong[:5].tolist()}: {np.asarray(g)[wrong[:5]].tolist()} for "
                                 f"{np.asarray(w)[wrong[:5]].tolist()}")
    assert [int(x) for x in got[3]] == list(want[3]), what


@pytest.mark.parametrize("record", ["lattice", "neighbours", "swaps", "same_low", "same_high",
                                    "stability"])
def test_probe_groups_crafted_digests(probe_results, record):
    rec, got = probe_results[record]
    assert_equal(got, (rec.rep, rec.size, rec.mixed, rec.stats), record)


def test_probe_refuses_a_malformed_file(native_lib, tmp_path):
    """A truncated record is status 2 before the device is touched; nothing is written."""
    exe = probe_program()
    sc.write_records(tmp_path / "records.bin", [sc.swaps()])
    whole = (tmp_path / "records.bin").read_bytes()
    (tmp_path / "short.bin").write_bytes(whole[:-3])
    r = subprocess.run([exe, str(tmp_path / "short.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "truncated body" in r.stderr
    assert not (tmp_path / "out.bin").exists()


@pytest.mark.parametrize("n,empties", [(sc.SCALE_SIZES[0], False), (sc.SCALE_SIZES[1], False),
                                       (sc.SCALE_SIZES[2], True)])
def test_entry_at_scale(kma, n, empties):
    c = sc.scale_case(n, empties)
    digests = n == sc.MERGE_SORT_LIMIT + 1
    out = kma.check_sequences(c.residues, c.offsets, c.fun, 0, digests=digests)
    assert_equal(out, (c.rep, c.size, c.mixed, c.stats), f"n = {n}")
    if digests:     # the count-capped grid: every wave owns hundreds of sequences
        body, off = c.residues.tobytes(), c.offsets.tolist()
        want = b"".join(hashlib.md5(body[off[i]:off[i + 1]]).digest() for i in range(n))
        got = out[4].reshape(-1).view("<u8").reshape(n, 2)
        wrong = np.flatnonzero((got != np.frombuffer(want, "<u8").reshape(n, 2)).any(axis=1))
        assert len(wrong) == 0, f"{len(wrong)} digests wrong, first at {wrong[:5].tolist()}"
    # without function ids: the same groups, nothing mixed
    if n == sc.SCALE_SIZES[0]:
        rep, size, mixed, stats = kma.check_sequences(c.residues, c.offsets, None, 0)
        assert_equal((rep, size, mixed, stats), (c.rep, c.size, np.zeros(n, np.uint8),
                                                 c.stats[:2] + [0]), f"n = {n}, no ids")


def test_entry_upper_flag_at_scale(kma):
    u = sc.upper_case()
    for flags in (sc.UPPER, 0):
        out = kma.check_sequences(u.residues, u.offsets, u.fun, flags)
        assert_equal(out, u.expected[flags], f"flags = {flags}")


def test_entry_count_edges(kma):
    for n in sc.COUNT_EDGES:
        c = sc.edge_case(n)
        out = kma.check_sequences(c.residues, c.offsets, c.fun, 0)
        assert_equal(out, (c.rep, c.size, c.mixed, c.stats), f"n = {n}")


@pytest.mark.parametrize("k", sc.VIEW_STARTS)
def test_entry_view_from_inside_a_batch(kma, k):
    (res, off, fun), want = sc.view_of(sc.view_case(), k)
    assert off[0] != 0
    assert_equal(kma.check_sequences(res, off, fun, 0), want, f"offsets[{k}:]")


def test_entry_function_id_patterns(kma):
    c, want = sc.fun_pattern_case()
    out = kma.check_sequences(c.residues, c.offsets, c.fun, 0)
    assert_equal(out, (c.rep, c.size, c.mixed, c.stats), "patterns")
    assert (out[2] == want).all() and out[3].tolist() == [8, 8, 5]
