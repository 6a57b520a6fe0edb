"""projector.annotate_proposals(extended=...) without a GPU: the (left, right, status) arrays that
kmeranno.extend_proposals would return are computed here with oracle/proposal_list.py:extend, on
the inputs of tests/test_projector.py::test_proposal_list_is_the_java_treeset (built to hit the
comparator's quirks and to merge). The host branch that takes the ORF and the rejected / weak /
small decision from the arrays must reproduce the extended=None result: features, order and
counters."""
import numpy as np
import pytest

from kmeranno import projector
from oracle.proposal_list import Loc, extend

KEPT, REJECTED, WEAK, SMALL = 0, 1, 2, 3
DTYPE = [("peg", "<u4"), ("contig", "<u4"), ("left", "<i4"), ("right", "<i4"),
         ("evidence", "<u4"), ("strand", "u1"), ("frame", "u1"), ("pad", "<u2")]


def _inputs():
    rng = np.random.default_rng(12)
    orf = "ATG" + "".join(rng.choice(["GCT", "AAA", "CTG", "GAT"], 60)) + "TAA"
    contig = ("CCC" + orf + "CC" + "TTA" + "GGG" * 10 + orf[::-1].translate(
        str.maketrans("ACGT", "TGCA")) + "GG") * 3
    props = []
    L = len(orf)
    for rep in range(3):
        base = rep * (len(contig) // 3)
        for shift in (0, 30, 60, 9, 90):  # one stop end, several starts inside the ORF
            props.append((0, "+", base + 4 + shift, base + 4 + shift + 23, 50 + (shift * 7) % 11))
        mleft = base + 4 + L + 2 + 3 + 30
        for shift in (0, 30, 60):
            props.append((0, "-", mleft + L - 24 - shift, mleft + L - 1 - shift, 45 + shift % 13))
    arr = np.zeros(len(props), DTYPE)
    for i, (c, s, lft, rgt, ev) in enumerate(props):
        arr[i] = (i % 4, c, lft, rgt, ev, ord(s), 0, 0)
    return arr, [f"F{i}" for i in range(4)], [contig], ["c1"]


def _extended(arr, contigs, min_strength, min_evidence, gcode=11):
    """What kma_extend_proposals returns, from the oracle's extend (the DNA strength is
    min_strength / 3, as annotate_proposals passes it)."""
    n = len(arr)
    left, right = np.zeros(n, np.int32), np.zeros(n, np.int32)
    status = np.zeros(n, np.uint8)
    for i, p in enumerate(arr):
        real = extend(contigs[int(p["contig"])],
                      Loc("", chr(p["strand"]), int(p["left"]), int(p["right"])), gcode)
        if real is None:
            status[i] = REJECTED
            continue
        left[i], right[i] = real.left, real.right
        if int(p["evidence"]) / real.length() < min_strength / 3:
            status[i] = WEAK
        elif int(p["evidence"]) < min_evidence:
            status[i] = SMALL
    return left, right, status


def _summary(feats, plist):
    return ([(f[0], f[1], f[2].contig, f[2].strand, f[2].left, f[2].right, f[3], f[4])
             for f in feats],
            (plist.made, plist.rejected, plist.weak, plist.small, plist.merged))


@pytest.mark.parametrize("min_strength,min_evidence", [(0.5, 10), (0.5, 52), (0.8, 10)])
def test_extended_arrays_reproduce_the_host_path(min_strength, min_evidence):
    arr, funcs, contigs, ids = _inputs()
    plain = projector.annotate_proposals(arr, funcs, contigs, "g", ids, min_strength,
                                         min_evidence)
    ext = _extended(arr, contigs, min_strength, min_evidence)
    fed = projector.annotate_proposals(arr, funcs, contigs, "g", ids, min_strength,
                                       min_evidence, extended=ext)
    assert _summary(*fed) == _summary(*plain)
    made, rejected, weak, small, merged = _summary(*plain)[1]
    assert made == len(arr) and len(plain[0]) > 0
    if (min_strength, min_evidence) == (0.5, 10):
        assert merged > 0 and len(plain[0]) > 2
    if min_evidence == 52:
        assert small > 0
    if min_strength == 0.8:
        assert weak > 0


def test_extended_decides_without_the_dna():
    """With extended= the ORF comes from the arrays alone: rejected rows stay rejected and kept
    rows keep their edges even when the contigs passed hold no DNA to walk."""
    arr, funcs, contigs, ids = _inputs()
    ext = _extended(arr, contigs, 0.5, 10)
    ext[2][0] = REJECTED
    feats, plist = projector.annotate_proposals(arr, funcs, [""], "g", ids, extended=ext)
    want, wlist = projector.annotate_proposals(arr[1:], funcs, contigs, "g", ids)
    assert _summary(feats, plist)[0] == _summary(want, wlist)[0]
    assert plist.made == len(arr) and plist.rejected == wlist.rejected + 1


def test_extended_arrays_must_match_the_proposals():
    arr, funcs, contigs, ids = _inputs()
    ext = _extended(arr, contigs, 0.5, 10)
    with pytest.raises(ValueError):
        projector.annotate_proposals(arr, funcs, contigs, "g", ids,
                                     extended=tuple(x[:-1] for x in ext))
