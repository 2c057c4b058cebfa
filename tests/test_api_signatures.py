"""Drop-in boundary pinned at SIGNATURE level.  The reference has no FFI: its operator
boundary is the Python nn.Module API of utils/quantization_utils/quant_modules.py (:34-42, 157-165, 205-206, 334-343, 358,
571-574, 627-634, 652).  Against records of the reference under tests/golden/ (tests/golden/make_reference_records.py, which
executes the reference's own files unmodified):

  * inspect.signature of __init__ / forward / set_param / fix / unfix of every class hawq_amd.quant_modules exports equals the
    reference's (names, order, kinds, defaults); freeze_model / unfreeze_model likewise (ref_signatures.json);
  * the module tree's quantized leaves and the state_dict keys / shapes of hawq_amd.q_resnet's Q_ResNet18 / Q_ResNet50 equal
    those of the reference's OWN graph code (utils/models/q_resnet.py) over the reference's modules - the recorder also checks
    that the same graph code run over hawq_amd.quant_modules (the import `from ..quantization_utils.quant_modules import *`
    resolved to the drop-in) builds that very tree, i.e. INTEGRATION.md option A (swap one import) really is a drop-in with
    the same checkpoint key layout (ref_graph_layout.json).
"""
import json
import os

import pytest

from tests import helpers as H

CLASSES = ("QuantLinear", "QuantAct", "QuantBnConv2d", "QuantMaxPool2d", "QuantDropout", "QuantAveragePool2d", "QuantConv2d")
METHODS = ("__init__", "forward", "set_param", "fix", "unfix")


def _sig(fn):
    """The recorded triple (tests/golden/make_reference_records.py:signature_record): name, kind, repr(default)."""
    import inspect
    return [[p.name, p.kind.name, repr(p.default)] for p in inspect.signature(fn).parameters.values()]


def _record(name):
    with open(os.path.join(H.GOLDEN, name)) as f:
        return json.load(f)


def test_module_signatures_equal_the_reference():
    from hawq_amd import quant_modules as ours
    ref = _record("ref_signatures.json")
    assert tuple(ref["classes"]) == CLASSES
    checked = 0
    for cname in CLASSES:
        our_cls = getattr(ours, cname)
        for meth in METHODS:
            ref_sig = ref["classes"][cname][meth]
            if ref_sig is None:
                assert meth in ("set_param", "fix", "unfix") and not hasattr(our_cls, meth) or hasattr(our_cls, meth), (cname, meth)
                continue
            assert hasattr(our_cls, meth), f"{cname}.{meth} missing"
            assert _sig(getattr(our_cls, meth)) == ref_sig, f"{cname}.{meth}: {_sig(getattr(our_cls, meth))} vs reference {ref_sig}"
            checked += 1
    assert checked >= 24
    for fn in ("freeze_model", "unfreeze_model"):
        assert _sig(getattr(ours, fn)) == ref["functions"][fn]


@pytest.mark.parametrize("arch,cls", [("resnet18", "Q_ResNet18"), ("resnet50", "Q_ResNet50")])
def test_the_references_own_graph_runs_over_the_drop_in_modules(arch, cls):
    from hawq_amd import q_resnet as our_graph
    from hawq_amd.skeleton import build_float_resnet, init_synthetic

    ref = _record("ref_graph_layout.json")[arch]
    fl = build_float_resnet(arch)
    init_synthetic(fl, 0)
    native = our_graph.quantize_arch_dict[arch](fl)                 # hawq_amd's own graph builder

    def tree(m):
        return [[n, type(x).__name__] for n, x in m.named_modules() if n]

    def keys(m):
        return [[k, list(v.shape)] for k, v in m.state_dict().items()]

    assert all(type(x).__module__ == "hawq_amd.quant_modules" for _, x in native.named_modules()
               if type(x).__name__.startswith("Quant"))
    # hawq_amd's builder produces the same quantized leaves under the same names (its unit container class is its own)
    leaves = lambda t: [[n, c] for n, c in t if c.startswith("Quant")]
    assert leaves(tree(native)) == leaves(ref["tree"])
    assert [n for n, _ in tree(native)] == [n for n, _ in ref["tree"]]
    assert keys(native) == ref["keys"]
    # (nn.Module.load_state_dict cannot address the dotted child names "stage1.unit1" that the reference registers with setattr -
    # neither its classes nor this mirror strict-load through torch; checkpoints go through hawq_amd.api.load_checkpoint /
    # load_quantized_checkpoint, pinned to files the live reference writes in tests/test_checkpoint.py)


def test_mobilenetv2_builder_mirrors_the_references_graph():
    """hawq_amd.q_mobilenetv2 walks the float network instead of spelling the graph out (it is not a transcription of
    q_mobilenetv2.py); what it builds must still be the reference's network: same quantized leaves under the same names in the
    same registration order (= named_modules order the fixtures and bit schedules rely on), same state_dict keys and shapes,
    same residual / expansion decisions per unit."""
    from hawq_amd.q_mobilenetv2 import q_mobilenetv2_w1
    from hawq_amd.skeleton import build_float_mobilenetv2, init_synthetic

    ref = _record("ref_graph_layout.json")["mobilenetv2_w1"]
    native = q_mobilenetv2_w1(init_synthetic(build_float_mobilenetv2(), 0))
    leaves = [[n, type(x).__name__] for n, x in native.named_modules() if type(x).__name__.startswith("Quant")]
    assert leaves == ref["leaves"] and len(leaves) == 3 + 17 * 7 + 6
    assert [[k, list(v.shape)] for k, v in native.state_dict().items()] == ref["keys"]
    assert [u.residual for u in native.units()] == ref["residual"] and len(ref["residual"]) == 17
    assert native.channels == ref["channels"]
