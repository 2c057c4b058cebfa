"""hawq_conv2d's dispatcher, checked without a device: for every argument struct of tests/conv_choice_cases.py the host-only
query hawq_conv2d_choice (argument check + choice of kernel, no launch) must answer exactly what the fixture holds - family,
resolved tile, function-table slot, grid, block, dynamic LDS and the computed kernel arguments, or the return code and the
refusal text.  The fixture (tests/golden/conv_choices.json, written by tests/golden/make_conv_choices.py) was recorded from
the commit before the dispatcher was split into check / choose / launch, so a launch that silently moves to another - still
bit-exact - kernel fails here, which no GPU test can see."""
import ctypes as C
import importlib.util
import json
import os

import pytest

from hawq_amd import _lib
from tests import conv_choice_cases as cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "conv_choices.json")
_spec = importlib.util.spec_from_file_location("make_conv_choices", os.path.join(GOLDEN, "make_conv_choices.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)   # record(), check_coverage(): the generator's own, so the test compares what it wrote


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_struct_is_mirrored_field_for_field(golden):
    assert golden["fields"] == [n for n, _ in _lib.ConvChoice._fields_]
    assert C.sizeof(_lib.ConvChoice) == 4 * 26


def test_the_fixture_covers_every_tile_slot_and_refusal(golden):
    gen.check_coverage(golden)


def test_every_choice_equals_the_recorded_one(lib, golden):
    all_cases = cases.build_cases()
    assert gen.names_digest([n for n, _ in all_cases]) == golden["cases"], "the case list changed: regenerate the fixture from the recorded commit"
    assert len(all_cases) == len(gen.expand(golden))
    wrong = [(name, want, got) for (name, a), want in zip(all_cases, gen.expand(golden)) if (got := gen.record(lib, a)) != want]
    assert not wrong, f"{len(wrong)} of {len(all_cases)} cases differ; first: {wrong[0]}"


def test_null_arguments_are_refused_with_the_recorded_text(lib, golden):
    assert [lib.hawq_conv2d_choice(None, C.byref(_lib.ConvChoice())), lib.hawq_last_error().decode()] == golden["null_args"]
    assert lib.hawq_conv2d_choice(C.byref(cases.build_cases()[0][1]), None) != 0


def test_splitk_queries_equal_the_recorded_ones(lib, golden):
    sk = cases.splitk_cases()
    assert gen.names_digest([n for n, _, _ in sk]) == golden["splitk_cases"]
    wrong = [(name, want, got) for (name, a, s), want in zip(sk, golden["splitk"]) if (got := gen.record_splitk(lib, a, s)) != want]
    assert not wrong, f"{len(wrong)} of {len(sk)} split-K cases differ; first: {wrong[0]}"
    assert any(r[0] == 1 for r in golden["splitk"]) and any(r[0] == 0 and "do not divide" in r[2] for r in golden["splitk"])
