"""The sessions of tests/session_cases.py meet the conditions tests/test_gpu_sessions.py relies on,
shown on the oracle alone (no GPU): no step is degenerate. Each test prints the counts its
conditions are about (pytest -s shows them).

The 13-protein batch p13 keeps the lengths of test_degenerate_proteins, nine of them below K, so
the 30%-called condition cannot hold for it (four proteins reach K); it is asserted for the
1,500-protein batch, and p13 instead shows all four statuses on its four proteins of K or more
residues."""
import numpy as np
import pytest

import session_cases as sc

NONE, CALLED, AMBIGUOUS, BELOW_MIN = 0, 1, 2, 3


def _steps(kind):
    return [s for s in sc.host_steps() if s.kind == kind]


def test_step_list_shape():
    steps = sc.host_steps()
    names = [s.name for s in steps]
    assert len(set(names)) == len(names)
    for i, s in enumerate(steps):
        if s.same_as is not None:  # refers to an earlier step of the same kind
            j = names.index(s.same_as)
            assert j < i and steps[j].kind == s.kind
            if s.name != "11-code11":
                assert steps[j].inp == s.inp
    assert [s.code for s in steps if s.name.startswith("11-code") and s.kind == "contigs"] == \
        list(sc.ALL_CODES)
    assert len(_steps("proteins_fail")) == 3 and len(_steps("contigs_fail")) == 1
    assert len(_steps("contigs_abi")) == 3


def test_table_rows():
    keys, fids = sc.table_rows()
    print(f"table rows {len(keys)}, distinct {len(np.unique(keys))}")
    assert 40_000 <= len(keys) <= 400_000 and fids.max() < sc.N_FID and keys.min() > 0


def test_protein_steps(oracle_c):
    lens13 = np.diff(sc.protein_batch("p13")[1]).astype(int)
    assert lens13.tolist() == sc.DEGENERATE_LENGTHS
    fid, cnt, st, tally = sc.expect_proteins(oracle_c, "p13")
    print("p13 status", st.tolist())
    assert (st[lens13 < sc.K] == NONE).all()
    assert set(st.tolist()) == {NONE, CALLED, AMBIGUOUS, BELOW_MIN} and tally.sum() >= 1
    for name in ("p1500", "p200", "pbig"):
        fid, cnt, st, tally = sc.expect_proteins(oracle_c, name)
        by = np.bincount(st, minlength=4)
        print(f"{name}: {len(st)} proteins, none {by[0]} called {by[1]} ambiguous {by[2]} "
              f"below-min {by[3]}")
        assert by[CALLED] >= 0.3 * len(st) and by.min() >= 1
    assert len(sc.expect_proteins(oracle_c, "p1500")[2]) == 1500
    n_res = int(sc.protein_batch("p1500")[1][-1])
    print(f"p1500: {n_res} residues, {n_res // sc.PIECE_MIN} pieces of >= {sc.PIECE_MIN}")
    assert n_res // sc.PIECE_MIN >= 4


def test_step8_long_proteins(oracle_c):
    res, off = sc.protein_batch("plong")
    lens = np.diff(off).astype(int)
    fid, cnt, st, _ = sc.expect_proteins(oracle_c, "plong")
    at = sc.PLONG_AT
    print("plong lengths", lens.tolist(), "counts", cnt.tolist(), "status", st.tolist())
    # one of >= 2,800 windows beside short ones (the first six proteins share a block of 6)
    assert at["lds"] < 6 and lens[at["lds"]] - sc.K + 1 >= 2800
    assert (np.delete(lens[:6], at["lds"]) <= 100).all()
    assert st[at["lds"]] == CALLED and cnt[at["lds"]] >= 2800
    # one of about 12,000 residues whose hit list passes 4,096 entries
    assert 11_000 <= lens[at["gset"]] <= 13_000
    assert st[at["gset"]] == CALLED and cnt[at["gset"]] > 4096 and fid[at["gset"]] == sc.LONG_FID
    # one of about 3,000 residues
    assert 2900 <= lens[at["third"]] <= 3100 and st[at["third"]] == CALLED
    assert 500 < cnt[at["third"]] < lens[at["third"]] - sc.K


def test_step9_flags_change_the_counts(oracle_c):
    counts = [sc.expect_proteins(oracle_c, "p1500", flags=f)[1] for f in (0, 1, 2, 3)]
    for i in range(4):
        for j in range(i + 1, 4):
            d = int((counts[i] != counts[j]).sum())
            print(f"flags {i} vs {j}: {d} counts differ")
            assert d >= 10


def test_contig_steps(oracle_c):
    for name in ("g60", "g300", "g20"):
        (ct, lf, sd, fr, fid), tally = sc.expect_contigs(oracle_c, name)
        nc = len(sc.genome(name)[1]) - 1
        print(f"{name}: {sc.n_bases(name)} bases, {len(ct)} hits, '+' {(sd == ord('+')).sum()}, "
              f"frames {np.bincount(fr, minlength=4)[1:].tolist()}")
        assert set(sd.tolist()) == {ord("+"), ord("-")} and set(fr.tolist()) == {1, 2, 3}
        assert len(np.unique(ct)) == nc and tally.sum() == len(ct)
    for name in ("g40", "none", "empty"):
        n = len(sc.expect_contigs(oracle_c, name)[0][0])
        print(f"{name}: {n} hits")
        assert n < 10
    assert sc.n_bases("g40") == 40 < sc.CONTIG_TILE
    # step 6's total; the cap of the device session's step 4 lies below it
    assert len(sc.expect_contigs(oracle_c, "g60")[0][0]) >= 200
    # one emit group covers 256 probe blocks of 1,024 positions: g60 has one, g300 two
    span = sc.CONTIG_TILE * sc.EMIT_GROUP
    assert sc.n_bases("g60") < span < sc.n_bases("g300") <= 2 * span


def test_step11_every_genetic_code(oracle_c):
    dna = sc.genome("g20")[0]
    assert {ord(c) for c in "nNuUacgtACGT"} <= set(dna.tolist())
    ref = sc.expect_contigs(oracle_c, "g20", 11)[0]
    for code in sc.ALL_CODES:
        e = sc.expect_contigs(oracle_c, "g20", code)[0]
        same = len(e[0]) == len(ref[0]) and all((a == b).all() for a, b in zip(e, ref))
        print(f"code {code}: {len(e[0])} hits, equal to code 11's: {same}")
        assert len(e[0]) >= 200
        assert same == (code in (1, 11))


def test_peg_session(oracle_c):
    pc = sc.peg_case()
    assert 290 <= pc.n_peg <= 310
    loose, strict = sc.expect_pegs(oracle_c, "A", False), sc.expect_pegs(oracle_c, "A", True)
    print(f"A: {len(loose[0])} connections, strict keeps {len(strict[0])}")
    assert len(loose[0]) - len(strict[0]) >= 50 and len(strict[0]) >= 500
    b = sc.expect_pegs(oracle_c, "B", True)
    nb = int(pc.genomes["B"][1][-1])
    print(f"B: {nb} bases, strict keeps {len(b[0])}")
    assert nb < int(pc.genomes["A"][1][-1]) and len(b[0]) >= 500
    assert [g for g, s in sc.PEG_STEPS if s] == ["A", "A", "B", "A"]


def test_device_session_shape(oracle_c):
    steps = sc.device_steps()
    assert sum(1 for s in steps if getattr(s, "lo", 0) or getattr(s, "lead", 0)) >= 2
    total = len(sc.expect_contigs(oracle_c, "g60")[0][0])
    assert [s.cap for s in steps if s.name == "4"] == [100] and total > 100
    n200 = int(sc.protein_batch("p200")[1][-1])
    nbig = int(sc.protein_batch("pbig")[1][-1])
    print(f"device session: p200 {n200} residues, pbig {nbig}")
    assert nbig > 2 * n200 and len(sc.protein_batch("pbig")[1]) == 3001
    fid, cnt, st, _ = sc.expect_proteins(oracle_c, "pbig")
    f1, c1, s1, _ = sc.expect_proteins(oracle_c, "p1500")
    assert (fid == np.tile(f1, 2)).all() and (cnt == np.tile(c1, 2)).all()
