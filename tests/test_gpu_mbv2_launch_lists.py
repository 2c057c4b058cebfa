"""The launch lists of the MobileNetV2 engine (hawq_amd/engine_mbv2.py) against tests/golden/mbv2_launch_lists.json, recorded before the
engine got its launch records (tests/golden/make_mbv2_launch_lists.py): per configuration the fp32 and the uint8 chain launch by launch -
entry point, every field of every argument block, every plain argument, the wiring of the buffers - and the plan's counters, bytes
and taps.  Each configuration is built once, at the smallest shape that still takes its path."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_mbv2_launch_lists", os.path.join(GOLDEN, "make_mbv2_launch_lists.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

_built = {}


def built(name):
    """what the generator records for configuration `name` now (built once per session), as JSON gives it back"""
    if name not in _built:
        got = gen.record(name)
        _built[name] = got, json.loads(json.dumps(got))
    return _built[name]


@pytest.fixture(scope="module")
def recorded():
    with open(gen.OUT) as f:
        text = f.read()
    return text, json.loads(text)


def _names(lists, chain=0, key="ops"):
    return [op[0] for op in lists["chains"][chain][key]]


def test_the_fixture_holds_the_ten_configurations(recorded):
    _, lists = recorded
    assert list(lists) == list(gen.CONFIGS) and len(lists) == 10
    assert [len(lists[k]["chains"]) for k in lists] == [1] * 9 + [2]
    assert all((c["ops_u8"] is None) == (k == "tapped") for k in lists for c in lists[k]["chains"])


@pytest.mark.parametrize("name", list(gen.CONFIGS))
def test_launch_lists_equal_the_recorded_ones(recorded, name):
    text, lists = recorded
    got, as_json = built(name)
    want = lists[name]
    for c, (g, w) in enumerate(zip(as_json["chains"], want["chains"])):   # (the first difference, readably, before the whole comparison)
        for key in ("ops", "ops_u8"):
            if w[key] is not None:
                assert [op[0] for op in g[key]] == [op[0] for op in w[key]], (c, key)
                for i, (og, ow) in enumerate(zip(g[key], w[key])):
                    assert og == ow, (c, key, i, og[0])
        assert {k: v for k, v in g.items() if not k.startswith("ops")} == {k: v for k, v in w.items() if not k.startswith("ops")}, c
    assert as_json == want
    # and the generator reproduces the file's line for this configuration byte for byte
    assert gen.dumps({name: got}).split("\n")[1] in [line.rstrip(",") for line in text.split("\n")]


def test_default_runs_sixteen_one_launch_units_and_a_one_launch_stem():
    _, d = built("default")
    (chain,) = d["chains"]
    assert chain["n_fused_units"] == 16 and _names(d).count("hawq_linear_bottleneck") == 16
    assert chain["stem"] and _names(d)[0] == "hawq_stem3x3s2" and _names(d, key="ops_u8")[0] == "hawq_stem3x3s2"
    assert d["n_launches"] == len(chain["ops"]) == len(chain["ops_u8"])


def test_unfused_runs_three_launches_per_unit_and_the_im2col_init_block():
    _, d = built("unfused")
    (chain,) = d["chains"]
    assert chain["n_fused_units"] == 0 and "hawq_linear_bottleneck" not in _names(d) and not chain["stem"]
    assert len(chain["ops"]) == len(built("default")[1]["chains"][0]["ops"]) + 2 * 16 + 1
    assert _names(d)[:2] == ["hawq_quantize_im2col3x3s2", "hawq_conv2d"] and _names(d, key="ops_u8")[0] == "hawq_quantize_im2col3x3s2_u8"
    assert _names(d, key="ops_u8")[1:] == _names(d)[1:]   # the uint8 chain differs in the input launch alone
