"""CPU tests of tests/convert_judge.py: the two restatements of `convert` against each other on the cases of tests/bam_cases.py, and
against hand-derived vectors (tests/golden/convert_vectors.json).

Where no run holds two N the reference's loop as written (`literal`) and the stated semantics (`stated`) give the same bytes.
Where one does, `literal` writes the run in front of it once more for every record of the dropped run without raising nrec, so a
chunk's nrec no longer counts the records its nbytes hold and the file cannot be read back: that is why the project departs from
the loop there, checked here and not merely claimed."""
import struct

import pytest

import bam_cases as B
import convert_judge as J
from util import load_golden, pkg

V = load_golden("convert_vectors.json")


@pytest.fixture(scope="module")
def cases():
    return B.all_cases(pkg.convert_limits()) + B.chunk_cases()


def test_literal_and_stated_agree_without_a_two_n_run(cases):
    n = 0
    for c in cases:
        if c.get("two_n"):
            continue
        for fb in c["filters"]:
            lit = J.literal(c["records"], fb)
            st = J.stated(c["records"], fb)
            assert b"".join(lit) == st["bytes"] and len(lit) == st["stats"]["n_chunks"], (c["name"], fb)
            bw, uw = J.widths(c["records"])
            assert [J.records_held(ch, bw, uw) for ch in lit] == st["nrec"] == [struct.unpack_from("<I", ch, 4)[0] for ch in lit], c["name"]
            n += 1
    assert n >= 40


def test_literal_breaks_the_chunk_on_every_case_with_a_two_n_run(cases):
    two = [c for c in cases if c.get("two_n")]
    assert len(two) >= 3
    for c in two:
        for fb in c["filters"]:
            lit = J.literal(c["records"], fb)
            bw, uw = J.widths(c["records"])
            assert any(J.records_held(ch, bw, uw) != struct.unpack_from("<I", ch, 4)[0] for ch in lit), c["name"]
            st = J.stated(c["records"], fb)   # ... and the stated semantics do not
            p = 0
            for k, n in enumerate(st["nrec"]):
                nbytes, nrec = struct.unpack_from("<II", st["bytes"], p)
                assert nrec == n == J.records_held(st["bytes"][p:p + nbytes], bw, uw) and p == st["chunk_off"][k]
                p += nbytes
            assert p == len(st["bytes"])


def test_the_coding_vectors():
    for v in V["coding"]:
        assert J.code(v["seq"], 0) == v["value"] == pkg.rad.seq_to_int(v["seq"]), v
    for n, w in V["widths"]:
        assert J.width_for(n) == w == pkg.rad.width_for_len(n)
    for v in V["cut"]:   # a later run's string is coded whole and cut to the first record's width
        recs = [B.rec("a", cr=v["first"], ur="A"), B.rec("b", cr=v["later"], ur="A")]
        for out in (J.stated(recs, False)["bytes"], b"".join(J.literal(recs, False))):
            w = J.width_for(len(v["first"]))
            second = 8 + (4 + w + 1 + 4)
            assert out[second + 4:second + 4 + w].hex() == v["stored_hex"], v


def test_the_orientation_vectors():
    for v in V["orientation"]:
        out = J.stated([B.rec("a", ref=v["ref"], flag=v["flag"])], False)["bytes"]
        assert struct.unpack_from("<I", out, len(out) - 4)[0] == v["word"], v


def test_the_chunk_cut_vectors():
    for n, want in V["chunks"]:
        recs = [B.rec("r%d" % i, cr="ACGT", ur="AC") for i in range(n)]
        assert J.stated(recs, False)["nrec"] == want and [struct.unpack_from("<I", ch, 4)[0] for ch in J.literal(recs, False)] == want, n


def test_every_error_case_is_refused_at_its_record():
    for c, fb, _, index in B.error_cases():
        if c["name"] in B.MALFORMED:
            continue
        for f in (J.stated,) if c["name"] == "ref_too_large" else (J.stated, J.literal):   # (the loop as written never looks a reference id up)
            with pytest.raises(J.Refusal) as e:
                f(c["records"], fb) if f is J.literal else f(c["records"], fb, n_ref=len(c["ref_names"]))
            assert e.value.index == index, (c["name"], f.__name__)
