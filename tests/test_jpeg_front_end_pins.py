"""The host front end of the device JPEG decoder (hawq_amd/jpeg.py) against what it was recorded to do (tests/jpeg_pins.py,
tests/golden/make_jpeg_front_end_pins.py): the outcome of ``parse_jpeg`` - which reason, or every field of the record - on some twenty
thousand mutated fixture files, parsed with and without ``progressive=True``, and the bytes of the planners' blobs.  No GPU."""
import functools
import json
import os

from tests import helpers as H
from tests import jpeg_pins


def _golden(name):
    with open(os.path.join(H.GOLDEN, name)) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def _parser():
    return jpeg_pins.parser_pins()


def test_the_corpus_is_as_large_and_as_varied_as_it_has_to_be():
    got = _parser()
    print({k: got[k] for k in ("inputs", "reasons", "accepted")})
    assert got["inputs"] >= 15000 and got["reasons"] >= 25 and 5 * got["accepted"] >= got["inputs"]
    names = set(got["fixtures"]) | set(got["structural"])
    assert {"prog/tables_13x17_422", "prog/deep_33x31_420"} <= set(got["fixtures"])
    for kind, refused in (("base", ("progressive", "cmyk", "png", "cut_header")),
                          ("prog", ("cut_last_scan", "adobe", "two_components", "ac_before_dc", "ah_not_previous_al", "65_scans"))):
        assert {"%s/refused_%s" % (kind, r) for r in refused} <= names
    byte_level = " ".join(got["fixtures"])
    assert all(word in byte_level for word in ("444", "422", "420", "gray", "rst"))


def test_parser_outcomes_under_mutation_are_the_recorded_ones():
    got, want = _parser(), _golden("jpeg_front_end_parser.json")
    for name, pins in want["fixtures"].items():   # unit by unit, so a difference names the segment
        assert got["fixtures"][name]["outcomes"] == pins["outcomes"], name
        for label, digest in pins["units"].items():
            assert got["fixtures"][name]["units"].get(label) == digest, (name, label)
    assert got["structural_outcomes"] == want["structural_outcomes"]
    for name, digest in want["structural"].items():
        assert got["structural"].get(name) == digest, name
    assert got == want   # nothing more and nothing less than recorded


def test_planner_blobs_are_the_recorded_bytes():
    got, want = jpeg_pins.planner_pins(), _golden("jpeg_front_end_planner.json")
    for label, pins in want.items():
        assert got.get(label) == pins, label
    assert set(got) == set(want)
