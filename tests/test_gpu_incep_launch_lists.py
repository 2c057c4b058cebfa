"""The launch lists of the InceptionV3 engine (hawq_amd/engine_inception.py) against tests/golden/incep_launch_lists.json, recorded
before the engine got its launch records (tests/golden/make_incep_launch_lists.py), and the data dependencies of the issued chains:
every launch comes after whatever writes its input.  One calibrated model, batch 1, 299 x 299."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_incep_launch_lists", os.path.join(GOLDEN, "make_incep_launch_lists.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def model():
    return gen.calibrated_model()


@pytest.fixture(scope="module")
def recorded():
    with open(gen.OUT) as f:
        text = f.read()
    return text, json.loads(text)


def test_the_fixture_holds_the_six_configurations(recorded):
    _, lists = recorded
    assert list(lists) == list(gen.CONFIGS) and len(lists) == 6
    assert [len(lists[k]["op_names"]) for k in lists] == [147, 145, 100, 98, 147, 147 - sum(
        len(c) - 1 for c, _ in lists["grouped+forced_groups_tile_4"]["group_launches"])]
    assert [len(lists[k]["op_names_u8"]) for k in lists][:4] == [145, 145, 98, 98]


@pytest.mark.parametrize("name", list(gen.CONFIGS))
def test_launch_lists_equal_the_recorded_ones(model, recorded, name):
    text, lists = recorded
    got = gen.record(model, name)
    assert json.loads(json.dumps(got)) == lists[name]
    # and the generator reproduces the file's line for this configuration byte for byte
    assert gen.dumps({name: got}).split("\n")[1] in [line.rstrip(",") for line in text.split("\n")]


# ---------------------------------------------------------------------- dependencies in the issued order
def _blocks(op):
    """the conv / pool argument blocks of one issued launch (the members of a grouped launch from its group block)"""
    from hawq_amd import _lib
    out = []
    for arg in op.args[1:]:
        block = getattr(arg, "_obj", None)
        if isinstance(block, _lib.IncepGroupArgs):
            out += [block.conv[k] for k in range(block.n)]
        elif isinstance(block, (_lib.IncepConvArgs, _lib.IncepPoolArgs)):
            out.append(block)
    return out


def _who(block):
    """what identifies a launch across chains: the slice it writes (a one-launch stem writes conv1's)"""
    return (type(block).__name__, block.out, block.c_off)


def _uses(chain):
    """per buffer (base pointer) the launches that write it and that read it, as {who: position in `chain`}; `chain` lists the blocks
    of each launch.  A block with `in` NULL (a one-launch stem's conv1) reads no buffer of the plan."""
    writers, readers = {}, {}
    for pos, blocks in enumerate(chain):
        for b in blocks:
            writers.setdefault(b.out, {})[_who(b)] = pos
            if b.in_ is not None:
                readers.setdefault(b.in_, {})[_who(b)] = pos
    return writers, readers


@pytest.mark.parametrize("grouped", [False, True], ids=["default", "grouped"])
def test_every_launch_follows_what_writes_its_input(model, grouped):
    from hawq_amd.engine_inception import InceptionEngine
    from hawq_amd.skeleton import synthetic_images
    eng = InceptionEngine(model, grouped=grouped)
    with torch.no_grad():
        eng(synthetic_images(1, seed=1, size=299).cuda())
        eng.forward_uint8(torch.zeros(1, 299, 299, 3, dtype=torch.uint8, device="cuda"))
    assert (eng.n_launches, eng.n_launches_u8) == ((100, 98) if grouped else (147, 145))
    # the default chain: the records in their own order, one block each
    default = [[r.args[0]] for r in eng._launches if r.kind in ("conv", "pool")]
    assert len(default) == 95 + 49
    w0, r0 = _uses(default)
    conv1 = eng._convs[0].args[0]
    for u8, ops in ((False, eng._ops), (True, eng._ops_u8)):
        chain = [b for b in map(_blocks, ops) if b]
        assert sum(map(len, chain)) == 95 + 49 and len(chain) == len(ops) - (1 if u8 else 3)
        w, r = _uses(chain)
        for buf, readers in r.items():   # every launch that writes a buffer precedes every launch that reads it
            for who_w, pw in w.get(buf, {}).items():
                for who_r, pr in readers.items():
                    assert pw < pr, (who_w, who_r)
        assert len(r) > 50 and sum(buf in w for buf in r) >= len(r) - 1   # all but conv1's input are written by a block's launch
        # the same writers and readers per buffer as in the default chain (the uint8 stem does not read conv1's input buffer)
        want_r = {buf: set(d) for buf, d in r0.items()}
        if u8:
            want_r[conv1.in_].discard(_who(conv1))
            want_r = {buf: s for buf, s in want_r.items() if s}
        assert {buf: set(d) for buf, d in w.items()} == {buf: set(d) for buf, d in w0.items()}
        assert {buf: set(d) for buf, d in r.items()} == want_r
