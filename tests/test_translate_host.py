"""§8(f)2, makeFeature's protein on the host: kmeranno.projector.peg_translate, the restatement
of Genome.getDna + DnaTranslator.pegTranslate(dna, 1, len - 3) (both external,
KmerProcessor.java:304-305), against the oracle composition — oracle_py.reverse_complement and
oracle_py.translate on the location's substring, with the trim and the 'M' rule composed here —
and pinned on the stored translations of the reference's own fixture (CPU only)."""
import numpy as np

from oracle import oracle_py

STARTS = ("ATG", "GTG", "TTG")
CODES = (1, 4, 11, 25)  # the genetic codes oracle_py and the product both know


def oracle_translate(contig: str, strand: str, left: int, right: int, gcode: int, peg: bool,
                     translate=oracle_py.translate) -> str:
    """The expected protein of a location: its substring (reverse complemented on '-') through
    the oracle's translate; peg mode drops the last whole codon and turns a first ATG / GTG / TTG
    into M."""
    sub = contig[left - 1:right]
    if strand == "-":
        sub = oracle_py.reverse_complement(sub)
    prot = translate(sub, 1, gcode)
    if not peg:
        return prot
    prot = prot[:max(len(sub) // 3 - 1, 0)]
    if prot and sub[:3].upper().replace("U", "T") in STARTS:
        prot = "M" + prot[1:]
    return prot


def single_region_pegs(gto):
    return [f for f in gto["features"]
            if f.get("protein_translation") and len(f["location"]) == 1]


def peg_location(projector, gto, feat):
    """A GTO location [contig id, begin, strand, length] as a projector.Location."""
    ids = [c["id"] for c in gto["contigs"]]
    cid, begin, strand, length = feat["location"][0]
    begin, length = int(begin), int(length)
    left, right = (begin, begin + length - 1) if strand == "+" else (begin - length + 1, begin)
    return projector.Location(ids.index(cid), strand, left, right, cid)


def test_peg_translate_matches_the_oracle_composition():
    """Random contigs with N, lower case, U / u and a byte >= 128, every span of 0..8 bases and
    a few longer ones, both strands, both modes, every code both sides know."""
    from kmeranno import projector
    rng = np.random.default_rng(31)
    pool = np.frombuffer(b"ACGT" * 6 + b"acgt" * 2 + b"NnUu\xff-", np.uint8)
    n_checked = 0
    for n in (0, 1, 2, 3, 7, 40, 211):
        contig = pool[rng.integers(0, len(pool), n)].tobytes().decode("latin-1")
        spans = [(lft, lft + ln - 1) for ln in range(0, 9) for lft in range(1, n - ln + 2)]
        spans += [(lft, lft + ln - 1) for ln in (24, 25, 38) for lft in range(1, n - ln + 2, 5)]
        for gcode in CODES:
            for left, right in spans:
                for strand in "+-":
                    for peg in (False, True):
                        got = projector.peg_translate(
                            contig, projector.Location(0, strand, left, right), gcode, peg)
                        want = oracle_translate(contig, strand, left, right, gcode, peg)
                        assert got == want, (n, gcode, left, right, strand, peg, got, want)
                        n_checked += 1
    assert n_checked > 30_000
    # the inputs exercise what they claim: X codons, both M outcomes, a code difference
    c = "ttgGCuTGANTG\xffTGTAA"
    loc = projector.Location(0, "+", 1, len(c))
    assert projector.peg_translate(c, loc, 11, True) == "MA*XX"
    assert projector.peg_translate(c, loc, 11, False) == "LA*XX*"
    assert projector.peg_translate(c, loc, 4, False) == "LAWXX*"
    assert projector.peg_translate(c, loc, 25, False) == "LAGXX*"
    rc = oracle_py.reverse_complement(c)
    assert projector.peg_translate(rc, projector.Location(0, "-", 1, len(c)), 11, True) == "MA*XX"


def test_peg_translate_defaults_to_peg_mode_and_refuses_unknown_codes():
    import pytest
    from kmeranno import projector
    loc = projector.Location(0, "+", 1, 9)
    assert projector.peg_translate("GTGGCTTAA", loc) == "MA"
    assert projector.peg_translate("CTGGCTTAA", loc) == "LA"
    assert projector.peg_translate("GCTGTGTAA", loc) == "AV"  # an internal GTG stays V
    for bad in (0, 7, 8, 15, 26):
        with pytest.raises(ValueError):
            projector.peg_translate("GTGGCTTAA", loc, bad)


def test_small_gto_pins_the_peg_rule(small_gto):
    """The reference's fixture stores the translation its pipeline gave every peg: peg mode
    reproduces 711 of the 712 single-region pegs; the one other, fig|97478.30.peg.413, runs off
    forward base 1 without a stop codon and stores the untrimmed translation with the M rule."""
    from kmeranno import projector
    contigs = [c["dna"] for c in small_gto["contigs"]]
    gcode = small_gto["genetic_code"]
    pegs = single_region_pegs(small_gto)
    assert len(pegs) == 712
    other, first = [], {}
    for f in pegs:
        loc = peg_location(projector, small_gto, f)
        got = projector.peg_translate(contigs[loc.contig], loc, gcode, True)
        assert got == oracle_translate(contigs[loc.contig], loc.strand, loc.left, loc.right,
                                       gcode, True)
        if got != f["protein_translation"]:
            other.append(f["id"])
        codon = projector.peg_translate(contigs[loc.contig], loc, gcode, False)[:1]
        first[codon] = first.get(codon, 0) + 1
    assert other == ["fig|97478.30.peg.413"]
    assert first == {"M": 586, "L": 80, "V": 46}  # ATG, TTG, GTG first codons, untouched in raw mode
    f = next(f for f in pegs if f["id"] == other[0])
    loc = peg_location(projector, small_gto, f)
    assert (loc.contig_id, loc.strand, loc.left, loc.right) == ("97478.30.con.0003", "-", 1, 2565)
    raw = projector.peg_translate(contigs[loc.contig], loc, gcode, False)
    assert len(raw) == 855 and "*" not in raw
    assert "M" + raw[1:] == f["protein_translation"]


def test_header_symbol_is_exported():
    import kmeranno
    from test_abi import header_functions
    assert "kma_translate_locations" in header_functions()
    assert "kma_translate_locations" in kmeranno.EXPORTS
    assert kmeranno.TR_PEG == 1 and kmeranno.LOCATION_DTYPE.itemsize == 16
    assert [kmeranno.LOCATION_DTYPE.fields[n][1] for n in ("contig", "left", "right", "strand")] \
        == [0, 4, 8, 12]
