"""Call sequences on long-lived tables and workspaces (tests/session_cases.py).

Every other GPU test creates a table, makes one kind of call, compares and destroys it. A host
keeps its table for the life of the process and calls it for every genome, from several threads,
with proteins and contigs in turn. What survives a call is then reused by the next one: the
pooled host contexts (grow-only device and pinned buffers that the protein path, the 6-frame path
and the strict peg join lay out differently, their event rings, their workspace), a workspace's
hash-set memory, staged hits, group sums and emit counter, its options and timing ring, the strict
join's per-slot counters, the staging pool and the replica list.

Each step's expected value is the oracle's answer on that step's input alone (oracle.c_oracle:
apply_mt, annotate_contigs, peg_connect and the operators' twins), every output array compared
whole by ==. A step that repeats an earlier step's input must also equal that earlier output.
tests/test_session_workload.py shows on the oracle alone that no step is degenerate.
"""
import ctypes as C
import threading

import numpy as np
import pytest

import session_cases as sc
from test_gpu_orf import make_props
from test_gpu_orf import small as orf_small  # noqa: F401 (fixture, under another name)
from test_gpu_set_ops import (PROP_FIELDS, check_build, check_distances, check_hash,
                              check_propose, hash_shared_case, java_best, pack, shared_input)
from test_gpu_translate import expect as translate_expect
from test_gpu_translate import small as translate_small  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu
K, N_FID = sc.K, sc.N_FID
GUARD = 16                      # untouched records / words after every device output
PROTEIN_OUT = ("fid", "count", "status", "tally")


@pytest.fixture(scope="module")
def kma(native_lib):
    import kmeranno
    assert kmeranno.device_count() >= 1
    return kmeranno


def make_table(kma, devices=None):
    keys, fids = sc.table_rows()
    if devices:
        return kma.SignatureTable.from_rows_replicated(sc.table_kmers(), fids, devices, K)
    return kma.SignatureTable.from_packed(keys, fids, K)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((a == b).all())


def same_records(a, b, fields=sc.HIT_FIELDS):
    """Structured arrays equal in every named field (the pad bytes aside)."""
    return len(a) == len(b) and all(same(a[f], b[f]) for f in fields)


def assert_hits(hits, e, what=""):
    assert len(hits) == len(e[0]), what
    for f, b in zip(sc.HIT_FIELDS, e):
        assert (hits[f] == b).all(), (what, f)


def host_proteins(kma, t, s):
    res, off = sc.protein_batch(s.inp)
    with kma.options(**s.opts):
        return kma.annotate_proteins(t, res, off, s.min_hits, s.flags, n_fid=N_FID)


def host_contigs(kma, t, s):
    dna, off = sc.genome(s.inp)
    with kma.options(**s.opts):
        return kma.annotate_contigs(t, dna, off, s.code, n_fid=N_FID)


def check_protein_out(got, want, what):
    for name, a, b in zip(PROTEIN_OUT, got, want):
        assert same(a, b), (what, name)


def check_contig_out(got, want, what):
    hits, tally = got
    assert_hits(hits, want[0], what)  # len(hits) is the published total
    assert same(tally, want[1]), (what, "tally")


# ---- 1. host session on one table ---------------------------------------------------------------
def contigs_abi_step(kma, t, s, want):
    """kma_annotate_contigs itself (the Python wrapper hides the capacity retry): a hit buffer
    prefilled with a pattern and a tally prefilled with counts."""
    lib = kma.load()
    dna, off = sc.genome(s.inp)
    e, e_tally = want
    nc, needed = len(off) - 1, len(e[0])
    hits = np.frombuffer(b"\xa5" * ((needed + GUARD) * kma.HIT_DTYPE.itemsize),
                         kma.HIT_DTYPE).copy()
    pattern = hits.copy()
    pre = (np.arange(nc * N_FID, dtype=np.uint32) % 5 + 1).reshape(nc, N_FID)
    tally = pre.copy()
    nh = C.c_uint64(12345)
    cap = needed if s.cap is None else needed + s.cap
    rc = lib.kma_annotate_contigs(t._h, dna, off, nc, 11, None if s.cap is None else
                                  hits.ctypes.data, cap, C.byref(nh), tally.ctypes.data, N_FID)
    assert nh.value == needed, s.name
    if s.cap == 0:
        assert rc == kma.OK, s.name
        assert_hits(hits[:needed], e, s.name)
        assert hits[needed:].tobytes() == pattern[needed:].tobytes(), s.name
        assert same(tally, pre + e_tally), s.name  # accumulated into the caller's counts
    else:  # "nothing is written on KMA_E_CAPACITY" (include/kmeranno.h; *n_hits = needed aside)
        assert rc == kma.E_CAPACITY, s.name
        assert hits.tobytes() == pattern.tobytes(), s.name
        assert same(tally, pre), s.name


@pytest.mark.parametrize("variant", ["two-choice", "chained", "two-replicas"])
def test_host_session_on_one_table(kma, oracle_c, variant):
    """sc.host_steps() in order on one SignatureTable, created once: 13 degenerate proteins, a
    60 kb genome, 1,500 proteins in 7 pipeline pieces, contig calls of 40 bases, of no contig
    and of empty contigs, a 300 kb genome (two emit groups) and the 60 kb one again, the
    capacity protocol at the C ABI, three refused protein calls each followed by a good one, three
    long proteins (LDS pool, workspace hash set), the four flag settings, KMA_OPT_PACKED_INPUT
    1, 0, 2, 1 with a genome in between, and the 6-frame call under every genetic code.

    Step 11 runs all 18 genetic codes the header lists (only 11 and 4 had gone through the probe
    kernel before), codes 1 and 11 with identical hits, an unknown code refused and the next call
    right. The oracle's code tables are the same text as the library's, so this pins the kernel's
    codon indexing, its complement x ^ 2 and the per-call table argument for every codon value
    under every code, not the NCBI strings themselves.

    Under two-choice and chained placement (KMA_OPT_PLACEMENT), and on a table with two replicas
    on device 0, whose host calls shard every batch over two contexts."""
    kma.set_option(kma.OPT_PLACEMENT, 0 if variant == "chained" else -1)
    done = {}
    with make_table(kma, [0, 0] if variant == "two-replicas" else None) as t:
        assert t.info.two_choice == (0 if variant == "chained" else 1)
        assert len(t.replicas) == (2 if variant == "two-replicas" else 1)
        for s in sc.host_steps():
            if s.kind == "proteins":
                got = host_proteins(kma, t, s)
                check_protein_out(got, sc.expect_proteins(oracle_c, s.inp, s.min_hits, s.flags),
                                  s.name)
                if s.same_as:
                    check_protein_out(got, done[s.same_as], (s.name, s.same_as))
            elif s.kind == "contigs":
                got = host_contigs(kma, t, s)
                check_contig_out(got, sc.expect_contigs(oracle_c, s.inp, s.code), s.name)
                if s.same_as:
                    assert same_records(got[0], done[s.same_as][0]), (s.name, s.same_as)
                    assert same(got[1], done[s.same_as][1]), (s.name, s.same_as)
            elif s.kind == "contigs_abi":
                contigs_abi_step(kma, t, s, sc.expect_contigs(oracle_c, s.inp))
                continue
            elif s.kind == "proteins_fail":
                res, off = sc.protein_batch(s.inp)
                if s.bad_offsets:
                    off = off.copy()
                    off[8] = off[7] - np.uint64(7)
                with pytest.raises(kma.KmerAnnoError) as err:
                    kma.annotate_proteins(t, res, off, s.min_hits, s.flags, n_fid=N_FID)
                assert err.value.code == kma.E_INVALID, s.name
                continue
            elif s.kind == "contigs_fail":
                with pytest.raises(kma.KmerAnnoError) as err:
                    host_contigs(kma, t, s)
                assert err.value.code == kma.E_INVALID, s.name
                continue
            else:
                raise AssertionError(s.kind)
            done[s.name] = got
    assert len(done) == sum(s.kind in ("proteins", "contigs") for s in sc.host_steps())


# ---- 2. peg-table session -----------------------------------------------------------------------
def test_peg_table_session(kma, oracle_c):
    """One peg table; strict A, strict A, non-strict A, strict B (smaller), strict A, non-strict
    B: the strict join zeroes and refills its per-slot location counters in the context's d_aux
    on every call, and a non-strict call in between leaves them stale. Genome A carries copied
    segments, so strict drops connections. Then the capacity protocol at the C ABI."""
    pc = sc.peg_case()
    t, _ = kma.SignatureTable.from_pegs(pc.residues, pc.offsets, K)
    strict_a = []
    with t:
        for i, (g, strict) in enumerate(sc.PEG_STEPS):
            hits = kma.connect_pegs(t, *pc.genomes[g], 11, strict)
            assert_hits(hits, sc.expect_pegs(oracle_c, g, strict), (i, g, strict))
            if g == "A" and strict:
                strict_a.append(hits)
        assert len(strict_a) == 3
        for h in strict_a[1:]:
            assert same_records(h, strict_a[0])
        lib = kma.load()
        dna, off = pc.genomes["A"]
        e = sc.expect_pegs(oracle_c, "A", True)
        needed = len(e[0])
        for cap in (needed - 1, needed):
            hits = np.frombuffer(b"\xa5" * ((needed + GUARD) * 16), kma.HIT_DTYPE).copy()
            nh = C.c_uint64(7)
            rc = lib.kma_connect_pegs(t._h, dna, off, len(off) - 1, 11, 1, hits.ctypes.data, cap,
                                      C.byref(nh))
            assert nh.value == needed
            if cap < needed:
                assert rc == kma.E_CAPACITY and hits.tobytes() == b"\xa5" * len(hits.tobytes())
            else:
                assert rc == kma.OK
                assert_hits(hits[:needed], e, "cap = needed")
                assert hits[needed:].tobytes() == b"\xa5" * (GUARD * 16)


# ---- 3. device session on one workspace and one stream ------------------------------------------
TALLY_GUARD = 1234567


def _tally_pre(n):
    return (np.arange(n, dtype=np.int64) * 7 % 11 + 1).astype(np.int32)


def run_device_session(kma, oracle_c, t, sync_each):
    """sc.device_steps() on one Workspace and one torch stream. Every input is on the device and
    every output buffer prefilled (sentinels, GUARD extra records or words, tallies holding
    counts) before the first call; with sync_each False nothing waits for the device between
    the calls but the reserve calls themselves, until one synchronisation at the end. Returns
    {step: {name: numpy array}} and the staged expectations."""
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    sp = stream.cuda_stream
    rec = kma.HIT_DTYPE.itemsize
    steps = sc.device_steps()
    staged = {}
    for s in steps:
        if s.kind == "proteins":
            res, off = sc.protein_batch(s.inp)
            sub = np.ascontiguousarray(off[s.lo:s.hi + 1])
            r0, r1, n = int(sub[0]), int(sub[-1]), s.hi - s.lo
            src = res if s.entry == "ascii" else kma.pack_residues(t, res[r0:r1])
            d = dict(inp=torch.from_numpy(src).to(dev),
                     off=torch.from_numpy(sub.view(np.int64).copy()).to(dev),
                     fid=torch.full((n + GUARD,), -7, dtype=torch.int32, device=dev),
                     count=torch.full((n + GUARD,), -7, dtype=torch.int32, device=dev),
                     status=torch.full((n + GUARD,), 9, dtype=torch.uint8, device=dev),
                     tally=torch.from_numpy(np.concatenate(
                         [_tally_pre(N_FID), np.full(GUARD, TALLY_GUARD, np.int32)])).to(dev),
                     n=n, n_res=r1 - r0)
            assert d["inp"].data_ptr() % 8 == 0
        elif s.kind in ("contigs", "over"):
            dna, off = sc.genome(s.inp)
            lead = getattr(s, "lead", 0)
            nc = len(off) - 1
            total = len(sc.expect_contigs(oracle_c, s.inp)[0][0])
            cap = total if getattr(s, "cap", None) is None else s.cap
            buf = np.concatenate([np.full(lead, ord("g"), np.uint8), dna])
            d = dict(inp=torch.from_numpy(buf).to(dev),
                     off=torch.from_numpy((off + np.uint64(lead)).view(np.int64).copy()).to(dev),
                     hits=torch.full(((max(cap, total) + GUARD) * rec,), 0xEE, dtype=torch.uint8,
                                     device=dev),
                     n_hits=torch.full((1 + GUARD,), -3, dtype=torch.int64, device=dev),
                     tally=torch.from_numpy(np.concatenate(
                         [_tally_pre(nc * N_FID), np.full(GUARD, TALLY_GUARD, np.int32)])).to(dev),
                     nc=nc, cap=cap, total=total)
        else:
            d = {}
        staged[s.name] = d
    n200 = int(sc.protein_batch("p200")[1][-1])
    ws = kma.Workspace(0, n200, 200)
    ws.reserve_contigs(sc.n_bases("g60"))
    torch.cuda.synchronize()
    try:
        for s in steps:
            d = staged[s.name]
            if s.kind == "proteins":
                for o, v in (s.ws_opts or {}).items():
                    ws.set_option({"block_proteins": kma.OPT_BLOCK_PROTEINS,
                                   "defer": kma.OPT_DEFER}[o], kma.OPT_DEFAULT if v is None else v)
                call = (kma.annotate_proteins_device if s.entry == "ascii"
                        else kma.annotate_packed_device)
                call(t, ws, d["inp"].data_ptr(), d["off"].data_ptr(), d["n"], d["n_res"],
                     sc.MIN_HITS, 0, d["fid"].data_ptr(), d["count"].data_ptr(),
                     d["status"].data_ptr(), d["tally"].data_ptr(), N_FID, sp)
            elif s.kind == "contigs":
                kma.annotate_contigs_device(t, ws, d["inp"].data_ptr(), d["off"].data_ptr(),
                                            d["nc"], sc.n_bases(s.inp), 11, d["hits"].data_ptr(),
                                            d["cap"], d["n_hits"].data_ptr(),
                                            d["tally"].data_ptr(), N_FID, sp)
            elif s.kind == "over":  # refused before any kernel runs
                with pytest.raises(kma.KmerAnnoError) as err:
                    kma.annotate_contigs_device(t, ws, d["inp"].data_ptr(), d["off"].data_ptr(),
                                                d["nc"], 10**7, 11, d["hits"].data_ptr(),
                                                d["cap"], d["n_hits"].data_ptr(),
                                                d["tally"].data_ptr(), N_FID, sp)
                assert err.value.code == kma.E_CAPACITY
            elif s.kind == "reserve":
                ws.reserve(int(sc.protein_batch(s.inp)[1][-1]))
            elif s.kind == "reserve_contigs":
                ws.reserve_contigs(sc.n_bases(s.inp))
            if sync_each:
                stream.synchronize()
        stream.synchronize()
        torch.cuda.synchronize()
    finally:
        ws.close()
    out = {}
    for s in steps:
        out[s.name] = {k: v.cpu().numpy() for k, v in staged[s.name].items()
                       if k not in ("inp", "off") and hasattr(v, "cpu")}
    return out, staged


def check_device_session(kma, oracle_c, out, staged):
    for s in sc.device_steps():
        o, d = out[s.name], staged[s.name]
        if s.kind == "proteins":
            n = d["n"]
            fid, cnt, st, tally = sc.expect_proteins(oracle_c, s.inp, lo=s.lo, hi=s.hi)
            assert same(o["fid"][:n], fid) and same(o["count"][:n], cnt), s.name
            assert same(o["status"][:n], st), s.name
            assert (o["fid"][n:] == -7).all() and (o["count"][n:] == -7).all(), s.name
            assert (o["status"][n:] == 9).all(), s.name
            assert same(o["tally"][:N_FID], _tally_pre(N_FID) + tally.astype(np.int32)), s.name
            assert (o["tally"][N_FID:] == TALLY_GUARD).all(), s.name
        elif s.kind == "contigs":
            e, e_tally = sc.expect_contigs(oracle_c, s.inp)
            total, cap, nt = d["total"], d["cap"], d["nc"] * N_FID
            assert o["n_hits"][0] == total and (o["n_hits"][1:] == -3).all(), s.name
            m = min(cap, total)
            hits = o["hits"].view(kma.HIT_DTYPE)
            assert_hits(hits[:m], [x[:m] for x in e], s.name)
            assert (o["hits"][m * kma.HIT_DTYPE.itemsize:] == 0xEE).all(), s.name  # past cap
            assert same(o["tally"][:nt], _tally_pre(nt) + e_tally.reshape(-1).astype(np.int32)), \
                s.name
            assert (o["tally"][nt:] == TALLY_GUARD).all(), s.name
        elif s.kind == "over":  # the refused call wrote nothing
            assert (o["hits"] == 0xEE).all() and (o["n_hits"] == -3).all(), s.name
            assert same(o["tally"][:-GUARD], _tally_pre(d["nc"] * N_FID)), s.name


@pytest.mark.parametrize("packed_input", [1, 2])
def test_device_session_without_host_sync(kma, oracle_c, packed_input):
    """One workspace, one stream: ASCII proteins, contigs, a packed stream, contigs with cap 100
    (the total is published, records past cap stay untouched) and with full capacity, workspace
    options set and reset, the workspace reserved larger in mid-session for both paths, a call
    above the reservation refused and the next one right. d_offsets[0] is nonzero in four calls
    and every tally is accumulated into counts already there. Issued back to back with no host
    synchronisation, then the whole session again with one after every call: identical arrays.
    Under KMA_OPT_PACKED_INPUT 1 (the staged ASCII probe) and 2 (the pack kernel into the
    workspace's stream, which the larger reservation reallocates)."""
    kma.set_option(kma.OPT_PACKED_INPUT, packed_input)
    with make_table(kma) as t:
        free, _ = run_device_session(kma, oracle_c, t, sync_each=False)
        out, staged = run_device_session(kma, oracle_c, t, sync_each=True)
        check_device_session(kma, oracle_c, free, staged)
        check_device_session(kma, oracle_c, out, staged)
        for name in out:
            assert set(out[name]) == set(free[name])
            for k in out[name]:
                assert same(out[name][k], free[name][k]), (name, k)


def _device_inputs(kma, oracle_c, torch):
    """p200 and g60 on the device with zeroed outputs, for the timing and graph tests."""
    dev = torch.device("cuda", 0)
    res, off = sc.protein_batch("p200")
    dna, goff = sc.genome("g60")
    total = len(sc.expect_contigs(oracle_c, "g60")[0][0])
    return dict(
        res=torch.from_numpy(res).to(dev), off=torch.from_numpy(off.view(np.int64).copy()).to(dev),
        n=len(off) - 1, n_res=int(off[-1]),
        fid=torch.zeros(len(off) - 1, dtype=torch.int32, device=dev),
        count=torch.zeros(len(off) - 1, dtype=torch.int32, device=dev),
        status=torch.zeros(len(off) - 1, dtype=torch.uint8, device=dev),
        ptally=torch.zeros(N_FID, dtype=torch.int32, device=dev),
        dna=torch.from_numpy(dna).to(dev),
        goff=torch.from_numpy(goff.view(np.int64).copy()).to(dev),
        nc=len(goff) - 1, n_bases=int(goff[-1]), cap=total + 3,
        hits=torch.zeros((total + 3) * kma.HIT_DTYPE.itemsize, dtype=torch.uint8, device=dev),
        n_hits=torch.zeros(1, dtype=torch.int64, device=dev),
        ctally=torch.zeros((len(goff) - 1) * N_FID, dtype=torch.int32, device=dev))


def _proteins(kma, t, ws, d, sp):
    kma.annotate_proteins_device(t, ws, d["res"].data_ptr(), d["off"].data_ptr(), d["n"],
                                 d["n_res"], sc.MIN_HITS, 0, d["fid"].data_ptr(),
                                 d["count"].data_ptr(), d["status"].data_ptr(),
                                 d["ptally"].data_ptr(), N_FID, sp)


def _contigs(kma, t, ws, d, sp):
    kma.annotate_contigs_device(t, ws, d["dna"].data_ptr(), d["goff"].data_ptr(), d["nc"],
                                d["n_bases"], 11, d["hits"].data_ptr(), d["cap"],
                                d["n_hits"].data_ptr(), d["ctally"].data_ptr(), N_FID, sp)


def test_timing_across_entry_points(kma, oracle_c):
    """Timing on, then two protein calls, one contig call, one protein call. phases_read reports
    "the calls laid out like the last one (same entry point)": the three protein calls, one phase
    named annotate_kernel (the default KMA_OPT_PACKED_INPUT runs no pack kernel); the read clears
    the ring, so both reads then return zero calls. No time is asserted."""
    torch = pytest.importorskip("torch")
    d = _device_inputs(kma, oracle_c, torch)
    sp = torch.cuda.current_stream().cuda_stream
    with make_table(kma) as t:
        ws = kma.Workspace(0, d["n_res"], d["n"])
        ws.reserve_contigs(d["n_bases"])
        torch.cuda.synchronize()
        ws.timing(True)
        _proteins(kma, t, ws, d, sp)
        _proteins(kma, t, ws, d, sp)
        _contigs(kma, t, ws, d, sp)
        _proteins(kma, t, ws, d, sp)
        calls, phases = ws.phases_read()
        assert calls == 3 and list(phases) == ["annotate_kernel"]
        assert ws.phases_read() == (0, {})
        assert ws.timing_read()[0] == 0
        # and laid out like a contig call when that is the last one
        _proteins(kma, t, ws, d, sp)
        _contigs(kma, t, ws, d, sp)
        calls, phases = ws.phases_read()
        assert calls == 1 and list(phases) == ["contigs_probe_kernel", "scan_emit"]
        assert ws.timing_read()[0] == 0
        torch.cuda.synchronize()
        ws.close()
    fid, cnt, st, tally = sc.expect_proteins(oracle_c, "p200")
    assert same(d["fid"].cpu().numpy(), fid) and same(d["status"].cpu().numpy(), st)
    assert same(d["ptally"].cpu().numpy(), 4 * tally.astype(np.int32))


def test_graph_of_a_protein_and_a_contig_call(kma, oracle_c):
    """One linear graph (torch.cuda.graph) holding kma_annotate_proteins_device and
    kma_annotate_contigs_device on the same workspace and stream (the header calls both
    graph-capturable; only the contig call had been captured), replayed three times with the
    outputs zeroed in between: every replay equals the oracle and the tallies grow by one
    call's worth per replay."""
    torch = pytest.importorskip("torch")
    d = _device_inputs(kma, oracle_c, torch)
    fid, cnt, st, ptally = sc.expect_proteins(oracle_c, "p200")
    e, ctally = sc.expect_contigs(oracle_c, "g60")
    with make_table(kma) as t:
        ws = kma.Workspace(0, d["n_res"], d["n"])
        ws.reserve_contigs(d["n_bases"])
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            sp = torch.cuda.current_stream().cuda_stream
            _proteins(kma, t, ws, d, sp)
            _contigs(kma, t, ws, d, sp)
        torch.cuda.synchronize()
        assert int(d["n_hits"].item()) == 0 and not d["ptally"].any()  # captured, not run
        for rep in range(1, 4):
            for k in ("fid", "count", "status", "hits", "n_hits"):
                d[k].zero_()
            g.replay()
            torch.cuda.synchronize()
            assert same(d["fid"].cpu().numpy(), fid) and same(d["count"].cpu().numpy(), cnt), rep
            assert same(d["status"].cpu().numpy(), st), rep
            assert same(d["ptally"].cpu().numpy(), rep * ptally.astype(np.int32)), rep
            assert int(d["n_hits"].item()) == len(e[0]), rep
            assert_hits(d["hits"].cpu().numpy().view(kma.HIT_DTYPE)[:len(e[0])], e, rep)
            assert not d["hits"][len(e[0]) * kma.HIT_DTYPE.itemsize:].any(), rep
            assert same(d["ctally"].cpu().numpy(),
                        rep * ctally.reshape(-1).astype(np.int32)), rep
        del g
        ws.close()


# ---- 4. threads ---------------------------------------------------------------------------------
LOOPS = 3


def run_threads(jobs, meanwhile=None):
    """jobs: {name: callable}; each runs LOOPS times on a thread of its own and its results are
    returned per loop. meanwhile: called on this thread as soon as the first call of any job has
    returned, while the jobs go on."""
    results, errors = {name: [] for name in jobs}, []
    first = threading.Event()

    def run(name, fn):
        try:
            for _ in range(LOOPS):
                results[name].append(fn())
                first.set()
        except Exception as e:  # noqa: BLE001 (reported below)
            errors.append((name, e))
            first.set()
    threads = [threading.Thread(target=run, args=kv) for kv in jobs.items()]
    for th in threads:
        th.start()
    if meanwhile:
        assert first.wait(timeout=120)
        meanwhile()
    for th in threads:
        th.join(timeout=120)
    assert not errors, errors
    assert not any(th.is_alive() for th in threads)
    assert all(len(r) == LOOPS for r in results.values())
    return results


def test_threads_mixed_callers_on_one_table(kma, oracle_c):
    """Four threads on one signature table, each another kind of host call (13 proteins; 1,500
    proteins with tally; the 60 kb genome with tally; the 300 kb genome), three times each, while
    this thread adds a replica (kma_table_replicate is documented as safe while calls run): every
    result equals the single-threaded one, which equals the oracle."""
    steps = {s.name: s for s in sc.host_steps()}
    pick = {"p13": steps["1"], "p1500": steps["3"], "g60": steps["2"], "g300": steps["5-300k"]}
    with make_table(kma) as t:
        single = {}
        for name, s in pick.items():
            if s.kind == "proteins":
                single[name] = host_proteins(kma, t, s)
                check_protein_out(single[name], sc.expect_proteins(oracle_c, s.inp), name)
            else:
                single[name] = host_contigs(kma, t, s)
                check_contig_out(single[name], sc.expect_contigs(oracle_c, s.inp), name)
        kma.set_option(kma.OPT_HOST_PIECE_MIN, sc.PIECE_MIN)  # (options are process-wide)
        res = {n: sc.protein_batch(s.inp) for n, s in pick.items() if s.kind == "proteins"}
        dna = {n: sc.genome(s.inp) for n, s in pick.items() if s.kind == "contigs"}
        jobs = {}
        for name in pick:
            if name in res:
                jobs[name] = lambda n=name: kma.annotate_proteins(t, *res[n], sc.MIN_HITS, 0,
                                                                  n_fid=N_FID)
            else:
                jobs[name] = lambda n=name: kma.annotate_contigs(t, *dna[n], 11, n_fid=N_FID)
        got = run_threads(jobs, meanwhile=lambda: t.replicate([0]))
        assert t.replicas == [0, 0]
        def unchanged(r, name):
            if name in res:
                check_protein_out(r, single[name], name)
            else:
                assert same_records(r[0], single[name][0]) and same(r[1], single[name][1]), name
        for name, loops in got.items():
            for r in loops:
                unchanged(r, name)
        # and once more, now sharded over both replicas
        for name, s in pick.items():
            unchanged(host_proteins(kma, t, s) if s.kind == "proteins" else host_contigs(kma, t, s),
                      name)


def test_threads_on_one_peg_table(kma, oracle_c):
    """Two threads run the strict join and two the non-strict one, on genomes A and B, on one peg
    table: each takes a context of its own, with its own per-slot counters."""
    pc = sc.peg_case()
    t, _ = kma.SignatureTable.from_pegs(pc.residues, pc.offsets, K)
    with t:
        cases = {(g, strict): None for g in "AB" for strict in (True, False)}
        for g, strict in cases:
            cases[g, strict] = kma.connect_pegs(t, *pc.genomes[g], 11, strict)
            assert_hits(cases[g, strict], sc.expect_pegs(oracle_c, g, strict), (g, strict))
        got = run_threads({c: (lambda c=c: kma.connect_pegs(t, *pc.genomes[c[0]], 11, c[1]))
                           for c in cases})
        for c, loops in got.items():
            for hits in loops:
                assert same_records(hits, cases[c]), c


def test_threads_table_less_operators(kma, oracle_c, orf_small, translate_small):
    """kma_hash_annotate, kma_protein_distances with kma_protein_best_match, kma_build_signatures,
    kma_propose_pegs, kma_translate_locations and kma_extend_proposals (two callers on one shared
    OrfIndex: "concurrent calls on one index are allowed"), all at once: they share the device,
    the staging pool and nothing else. Six threads, and this thread as the second caller on the
    index. Inputs: the small proteins of test_gpu_set_ops.shared_input(8), the small genomes of
    the ORF and translate tests, the peg session's connections. Each expected value was computed
    single-threaded first and compared with the oracle there."""
    si = shared_input(8)
    prots = [si.prots[i] for i in si.small]
    res, off = pack(prots)
    n = len(prots)
    # hash annotator
    genome, protos = hash_shared_case(8)
    small_g, small_p = [genome[i] for i in si.small], [p for p in protos if len(p) < 1000]
    g, go = pack(small_g)
    p, po = pack(small_p)
    want_hash = check_hash(kma, oracle_c, (g, go), (p, po), 8, 0.0125)
    # distances and best match: every protein against its four successors
    pa = np.repeat(np.arange(n, dtype=np.uint32), 4)
    pb = ((pa + np.tile(np.arange(1, 5, dtype=np.uint32), n)) % n).astype(np.uint32)
    want_dist = check_distances(kma, oracle_c, res, off, pa, pb, 8, 0)
    query = np.arange(n, dtype=np.uint32)
    cand_off = (np.arange(n + 1) * 4).astype(np.uint64)
    want_best = kma.protein_best_match(res, off, query, cand_off, pb, 0.9, 8)
    ebest, ebd = java_best(oracle_c.protein_distances(res, off, pa, pb, 8, 0)[3], pb, cand_off, 0.9)
    assert same(want_best[0], ebest) and same(want_best[1], ebd)
    # signature build
    roles = [si.roles[i] for i in si.small]
    want_build = check_build(kma, oracle_c, res, off, roles, 8)
    # proposals from the peg session's connections
    pc = sc.peg_case()
    peg_len = np.diff(pc.offsets).astype(np.uint32)
    t, _ = kma.SignatureTable.from_pegs(pc.residues, pc.offsets, K)
    with t:
        conn = kma.connect_pegs(t, *pc.genomes["B"], 11, False)
    want_prop = check_propose(kma, oracle_c, conn, peg_len, 8)
    assert len(want_prop[0]) >= 10
    # translation
    tcontigs, trows = translate_small
    trows = trows[::37]
    tdna, toff = kma.pack_strings(tcontigs)
    locs = kma.make_locations(trows)
    want_tr = kma.translate_locations(tdna, toff, locs, 11, False)
    raw = translate_expect(tcontigs, trows, 11)[0]
    text = want_tr[0].tobytes()
    assert [text[int(a):int(b)].decode("latin-1")
            for a, b in zip(want_tr[1][:-1], want_tr[1][1:])] == raw
    # ORF extension on one shared index
    ocontigs, orows, oexp = orf_small
    props = make_props(kma, orows)
    odna, ooff = kma.pack_strings(ocontigs)
    with kma.OrfIndex(odna, ooff) as idx:
        want_orf = kma.extend_proposals(idx, props, 0.0, 0)
        assert list(zip(want_orf[2].tolist(), want_orf[0].tolist(), want_orf[1].tolist())) == \
            oexp[11]
        half = len(props) // 2
        mine = []
        jobs = {
            "hash": lambda: kma.hash_annotate(g, go, p, po, 8, 0.0125),
            "distances": lambda: (kma.protein_distances(res, off, pa, pb, 8, 0) +
                                  kma.protein_best_match(res, off, query, cand_off, pb, 0.9, 8)),
            "build": lambda: kma.build_signatures(res, off, roles, 8),
            "propose": lambda: kma.propose_pegs(conn, peg_len, 8),
            "translate": lambda: kma.translate_locations(tdna, toff, locs, 11, False),
            "extend": lambda: kma.extend_proposals(idx, props[:half], 0.0, 0),
        }
        got = run_threads(jobs, meanwhile=lambda: mine.extend(
            kma.extend_proposals(idx, props[half:], 0.0, 0) for _ in range(LOOPS)))
    want = {"hash": want_hash, "distances": want_dist + want_best, "build": want_build,
            "translate": want_tr}
    for r in got["propose"]:
        assert same_records(r[0], want_prop[0], PROP_FIELDS) and same(r[1], want_prop[1])
    for name, w in want.items():
        for r in got[name]:
            assert len(r) == len(w)
            for a, b in zip(r, w):
                assert same(np.asarray(a), np.asarray(b)), name
    for r in got["extend"]:
        assert all(same(r[i], want_orf[i][:half]) for i in range(3)) and r[3][0] == half
    assert len(mine) == LOOPS
    for r in mine:
        assert all(same(r[i], want_orf[i][half:]) for i in range(3))
        assert r[3][0] == len(props) - half
