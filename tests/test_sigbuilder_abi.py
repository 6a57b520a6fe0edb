"""The streamed signature build's entry points and the build command's host side (no GPU).

kma_sig_builder_*: every KMA_E_INVALID refusal comes back before a device is touched (a request
that got as far as the device would be KMA_E_DEVICE on the device number used here, which does
not exist). kmeranno.build: resolve_roles restates BuildKmerProcessor.java:158-165 on
hand-written functions; the readers of the role file, the good-role file and the -g file."""
import ctypes as C

import numpy as np
import pytest

NO_DEVICE = 12345


def test_exports(native_lib):
    import kmeranno as k
    for name in ("kma_sig_builder_create", "kma_sig_builder_add", "kma_sig_builder_info_get",
                 "kma_sig_builder_finish", "kma_sig_builder_destroy"):
        assert name in k.EXPORTS and hasattr(native_lib, name)
    assert native_lib.kma_abi_version() == 7
    assert C.sizeof(k.SigBuilderInfo) == 64


def test_invalid_arguments_come_back_without_a_device(native_lib):
    import kmeranno as k
    L = native_lib
    h = C.c_void_p()
    refused = [((8, 0, NO_DEVICE, None), "null argument"),
               ((0, 0, NO_DEVICE, C.byref(h)), "kmer size 0"),
               ((13, 0, NO_DEVICE, C.byref(h)), "kmer size 13"),
               ((-1, 0, NO_DEVICE, C.byref(h)), "kmer size -1"),
               ((8, 2, NO_DEVICE, C.byref(h)), "bad flags"),
               ((8, 0x80000000, NO_DEVICE, C.byref(h)), "bad flags")]
    for args, msg in refused:
        assert L.kma_sig_builder_create(*args) == k.E_INVALID, args
        assert msg in L.kma_last_error().decode(), args
        assert not h.value
    for flags in (0, k.F_END_EXCLUSIVE):
        for kk in (1, 8, 12):
            assert L.kma_sig_builder_create(kk, flags, NO_DEVICE, C.byref(h)) == k.E_DEVICE
            assert not h.value
    res, off, roles = np.zeros(16, np.uint8), np.array([0, 9], np.uint64), np.zeros(1, np.int32)
    assert L.kma_sig_builder_add(None, res.ctypes.data, off.ctypes.data, roles.ctypes.data,
                                 1) == k.E_INVALID
    assert L.kma_sig_builder_add(None, None, None, None, 0) == k.E_INVALID
    info = k.SigBuilderInfo()
    assert L.kma_sig_builder_info_get(None, C.byref(info)) == k.E_INVALID
    n = C.c_uint64(77)
    assert L.kma_sig_builder_finish(None, None, None, 0, C.byref(n)) == k.E_INVALID
    assert L.kma_sig_builder_destroy(None) == k.OK
    with pytest.raises(k.KmerAnnoError) as e:
        k.SigBuilder(k=13, device=NO_DEVICE)
    assert e.value.code == k.E_INVALID
    with pytest.raises(k.KmerAnnoError) as e:
        k.SigBuilder(k=8, flags=4, device=NO_DEVICE)
    assert e.value.code == k.E_INVALID
    with pytest.raises(k.KmerAnnoError) as e:
        k.SigBuilder(device=NO_DEVICE)
    assert e.value.code == k.E_DEVICE


ROLE_FILE = ("AlaRace\tx1\tAlanine racemase (EC 5.1.1.1)\n"
             "ThrSynt\tx2\tThreonine synthase (EC 4.2.3.1)\n"
             "DnaPoly\tx3\tDNA polymerase I (EC 2.7.7.7)\n"
             "HypoProt\tx4\tKnown but not good\n")


@pytest.fixture()
def role_files(tmp_path):
    from kmeranno import build
    rf, gf = tmp_path / "roles.in.subsystems", tmp_path / "roles.to.use"
    rf.write_text(ROLE_FILE)
    gf.write_text("ThrSynt\nAlaRace\n\nDnaPoly  \nThrSynt\n")
    role_map, names = build.load_role_map(str(rf))
    good_ids = build.read_set(str(gf))
    return role_map, names, good_ids, {r: i for i, r in enumerate(good_ids)}


def test_role_file_readers(role_files, tmp_path):
    from kmeranno import build
    role_map, names, good_ids, good = role_files
    assert good_ids == ["ThrSynt", "AlaRace", "DnaPoly"]  # file order, each once, no empty line
    assert role_map["alanine racemase (ec 5.1.1.1)"] == "AlaRace"
    assert names["HypoProt"] == "Known but not good" and len(role_map) == 4
    gfile = tmp_path / "genomes.tbl"
    gfile.write_text("genome_id\tname\n83333.1\tEscherichia coli\n\n511145.12\tother\n")
    assert build.read_genome_ids(str(gfile)) == {"83333.1", "511145.12"}  # the header is skipped
    gfile.write_text("83333.1\tname\n")
    assert build.read_genome_ids(str(gfile)) == set()
    assert build.kmer_of((1 << 35) | (3 << 30) | 27, 8) == "AC@@@@@*".replace("@", "?")


def test_resolve_roles(role_files):
    from kmeranno.build import resolve_roles
    role_map, _, _, good = role_files
    A, T, D = good["AlaRace"], good["ThrSynt"], good["DnaPoly"]
    assert (T, A, D) == (0, 1, 2)
    rr = lambda f: resolve_roles(f, role_map, good)  # noqa: E731
    assert rr("Alanine racemase (EC 5.1.1.1)") == A
    # two good roles: skipped
    assert rr("Alanine racemase (EC 5.1.1.1) / Threonine synthase (EC 4.2.3.1)") == -2
    assert rr("Alanine racemase (EC 5.1.1.1) @ DNA polymerase I (EC 2.7.7.7)") == -2
    assert rr("Alanine racemase (EC 5.1.1.1); Threonine synthase (EC 4.2.3.1)") == -2
    # one good role plus one known role that is not good: counted
    assert rr("Threonine synthase (EC 4.2.3.1) / Known but not good") == T
    assert rr("Known but not good @ DNA polymerase I (EC 2.7.7.7)") == D
    # one good role plus a role the map does not know: counted
    assert rr("DNA polymerase I (EC 2.7.7.7) / Hypothetical protein") == D
    # a known role that is not good, alone: buffered; an unknown function and none: buffered
    assert rr("Known but not good") == -1
    assert rr("hypothetical protein") == -1
    assert rr("") == -1 and rr(None) == -1
    # a comment after " #" is dropped
    assert rr("Alanine racemase (EC 5.1.1.1) # Threonine synthase (EC 4.2.3.1)") == A
    assert rr("hypothetical protein # Alanine racemase (EC 5.1.1.1)") == -1
    # case and white space are folded
    assert rr("alanine   RACEMASE (ec 5.1.1.1)") == A
    assert rr("  Threonine\tsynthase  (EC 4.2.3.1)  ") == T
