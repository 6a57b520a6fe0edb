"""The build command (python -m kmeranno.build: BuildKmerProcessor.java:137-223 above the streamed
signature build) on the reference's own genome fixture small.gto, written twice into a genome
directory: as it is, and under another id with its features shuffled. The role file and the
good-role file are synthesized from the fixture's functions. The command's rows are compared, as a
set, with oracle_py.build_signatures over this test's own calls of resolve_roles, and the file it
writes is loaded and applied."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu
K = 8


def _pegs(genome):
    from kmeranno.seqcheck import genome_pegs
    return [(prot, func) for _, prot, func in genome_pegs(genome)]


@pytest.fixture(scope="module")
def inputs(native_lib, small_gto, tmp_path_factory):
    from kmeranno.seqcheck import roles_of
    d = tmp_path_factory.mktemp("build_cmd")
    gdir = d / "genomes"
    gdir.mkdir()
    rng = np.random.default_rng(11)
    second = dict(small_gto, id="1280.99999")
    second["features"] = [small_gto["features"][i]
                          for i in rng.permutation(len(small_gto["features"]))]
    with open(gdir / "a_small.gto", "w") as f:
        json.dump(small_gto, f)
    with gzip.open(gdir / "b_shuffled.gto.gz", "wt") as f:
        json.dump(second, f)
    (gdir / "notes.txt").write_text("not a genome\n")
    # roles: every role of a peg's function but the commonest, 60 of them good, 40 more known
    # (both roles of two two-role functions good: those pegs are skipped; of a third, one good
    # and one only known: that peg is counted)
    funcs = sorted({func for _, func in _pegs(small_gto)})
    multi = [roles_of(f) for f in funcs if len(roles_of(f)) == 2
             and "hypothetical protein" not in roles_of(f)]
    assert len(multi) >= 3
    good_first = multi[0] + multi[1] + multi[2][:1]
    names = sorted({r for f in funcs for r in roles_of(f)} - {"hypothetical protein"}
                   - set(good_first) - set(multi[2]))
    rest = [names[i] for i in rng.permutation(len(names))[:94]]
    picked = good_first + rest[:55] + multi[2][1:] + rest[55:]
    assert len(picked) == 100 and len(set(picked)) == 100
    ids = [f"Role{i:03d}" for i in range(100)]

    def disguise(i, name):  # the role file's spelling differs in case and white space
        return name.upper() if i % 3 == 0 else name.replace(" ", "  ") if i % 3 == 1 else name
    (d / "roles.in.subsystems").write_text(
        "".join(f"{rid}\tchk{i}\t{disguise(i, nm)}\n" for i, (rid, nm) in enumerate(zip(ids, picked))))
    (d / "roles.to.use").write_text("".join(f"{rid}\n" for rid in ids[:60]) + "RoleNoKmers\n")
    (d / "genomes.tbl").write_text("genome_id\tname\n1280.99999\tthe shuffled copy\n")
    return d, gdir, [small_gto, second]


def run_build(d, gdir, *extra):
    env = dict(os.environ, PYTHONPATH=os.path.join(PKG, "python"))
    r = subprocess.run([sys.executable, "-m", "kmeranno.build", str(d / "roles.in.subsystems"),
                        str(d / "roles.to.use"), str(gdir), *extra],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def expected_rows(d, genomes):
    from kmeranno import build
    from oracle import oracle_py
    role_map, _ = build.load_role_map(str(d / "roles.in.subsystems"))
    good_ids = build.read_set(str(d / "roles.to.use"))
    good = {r: i for i, r in enumerate(good_ids)}
    prots, roles = [], []
    for g in genomes:
        for prot, func in _pegs(g):
            prots.append(prot)
            roles.append(build.resolve_roles(func, role_map, good))
    keep = oracle_py.build_signatures(prots, roles, K)
    return {f"{km}\t{good_ids[r]}" for km, r in keep.items()}, prots, roles


def test_build_command(inputs, oracle_c, tmp_path):
    d, gdir, genomes = inputs
    small = run_build(d, gdir, "--batch-residues", "20000")
    default = run_build(d, gdir)
    assert small.stdout == default.stdout
    lines = default.stdout.splitlines()
    want, prots, roles = expected_rows(d, genomes)
    n_role = sum(r >= 0 for r in roles)
    assert n_role > 100 and sum(r == -2 for r in roles) > 0 and len(want) > 10_000
    assert len(set(lines)) == len(lines) and set(lines) == want
    assert [ln.split("\t")[0] for ln in lines] == sorted(ln.split("\t")[0] for ln in lines)
    # the log: per genome (file-name order), the total and the good role without kmers
    log = default.stderr.splitlines()
    per = [sum(r >= 0 for r in roles[:len(roles) // 2]), sum(r == -1 for r in roles[:len(roles) // 2])]
    assert log[0] == f"a_small.gto: {per[0]} interesting pegs found, {per[1]} buffered."
    assert log[1] == f"b_shuffled.gto.gz: {per[0]} interesting pegs found, {per[1]} buffered."
    assert log[2] == f"{len(want)} discriminating kmers remaining."
    assert "No kmers found for RoleNoKmers: ." in log[3:]
    # -g: the one genome named
    one = run_build(d, gdir, "-g", str(d / "genomes.tbl"), "-K", "8")
    want_one, _, _ = expected_rows(d, genomes[1:])
    assert set(one.stdout.splitlines()) == want_one
    # (the copy holds the same proteins, so the rows alone do not tell: the log names the genomes)
    assert one.stderr.splitlines()[0].startswith("b_shuffled.gto.gz: ")
    assert "a_small" not in one.stderr
    # round trip: the file is a kmerdb.tbl
    import kmeranno as kma
    path = tmp_path / "kmerdb.tbl"
    path.write_text(default.stdout)
    res, off = oracle_c.pack_strings(prots)
    table, role_ids, last_k = kma.SignatureTable.from_tsv(str(path), K)
    with table as t:
        fid, cnt, st, _ = kma.annotate_proteins(t, res, off, 5)
    assert last_k == K
    fid_of = {r: i for i, r in enumerate(role_ids)}
    rows = [ln.split("\t") for ln in lines]
    ot = oracle_c.Table([km for km, _ in rows], np.array([fid_of[r] for _, r in rows], np.int32))
    efid, ecnt, est = oracle_c.apply(ot, res, off, K, 5, 0)
    assert (st == est).all() and (fid == efid).all() and (cnt == ecnt).all()
    called = (st == kma.STATUS_CALLED) & (np.asarray(roles) >= 0)
    assert called.sum() > 100
    good_ids = [ln for ln in (d / "roles.to.use").read_text().splitlines() if ln]
    assert all(role_ids[f] == good_ids[r] for f, r in zip(fid[called], np.asarray(roles)[called]))
