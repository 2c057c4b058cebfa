"""Writes tests/golden/incep_launch_lists.json: the launch lists of the InceptionV3 engine (hawq_amd/engine_inception.py) at batch 1,
299 x 299, per configuration - what tests/test_gpu_incep_launch_lists.py compares a rebuilt engine with.  Needs the MI355X (the
engine asks the library which tiles, groups and pool launches it takes).  Run from the repository root:

    python tests/golden/make_incep_launch_lists.py [OUT]

Per configuration, one line of the file: ``op_names``, the uint8 chain's names, the op index of every conv launch and of every pool
launch, ``conv_launches``, ``pool_launches``, the integer shape fields of every pool block (no table values: they depend on the
calibration) and ``group_launches``.  The file was first recorded on the commit before the engine got its launch records, by this
script with ``op_indices`` reading ``_convs`` / ``_pools`` instead; this version reproduces it byte for byte.
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "tests", "golden", "incep_launch_lists.json")
POOL_FIELDS = ("N", "H", "W", "C", "in_bits", "in_pitch", "in_off", "out_bits", "ldo", "c_off", "pre", "post")
CONFIGS = {   # name -> (engine options, forced plan: None, ("tiles", id) or ("groups", id))
    "default": ({}, None),
    "fast_pools+fused_stem": ({"fast_pools": True, "fused_stem": True}, None),
    "grouped": ({"grouped": True}, None),
    "grouped+fast_pools+fused_stem": ({"grouped": True, "fast_pools": True, "fused_stem": True}, None),
    "forced_tile_3": ({}, ("tiles", 3)),
    "grouped+forced_groups_tile_4": ({"grouped": True}, ("groups", 4)),
}


def calibrated_model():
    from hawq_amd.api import build_quantized_resnet, calibrate
    from hawq_amd.skeleton import synthetic_images
    model = build_quantized_resnet("inceptionv3", "uniform8", seed=0).cuda()
    calibrate(model, synthetic_images(2, seed=0, size=299).cuda())
    return model


def op_indices(eng):
    """(op index of every conv launch, op index and argument block of every pool launch), in the default plan's order"""
    at = [(eng._at[r], r) for r in eng._launches]
    return [idx for idx, r in at if r.kind == "conv"], [(idx, r.args[0]) for idx, r in at if r.kind == "pool"]


def forced_plan(probe, force):
    """tile `id` on every conv launch that takes it / every level of two or more convs that takes tile `id` as a group"""
    from hawq_amd import _lib
    from hawq_amd.engine_inception import make_plan
    kind, tile = force
    keys, T = probe.conv_launches, _lib.load().hawq_incep_conv_num_tiles()
    if kind == "tiles":
        return make_plan(probe._batch, keys, T, [tile if probe._tile_ok(i, tile) else 0 for i in range(len(keys))], [{} for _ in keys])
    groups = [{"convs": lv, "tile": tile} for lv in probe.conv_level_list if len(lv) >= 2 and probe._group_ok(lv, tile)]
    return make_plan(probe._batch, keys, T, [0] * len(keys), [{} for _ in keys], groups)


def describe(eng):
    """the launch lists of an engine that has run ``eng(x)`` and ``eng.forward_uint8(u8)``"""
    convs, pools = op_indices(eng)
    return {"op_names": eng.op_names, "op_names_u8": [op.args[0] for op in eng._ops_u8], "conv_ops": convs,
            "pool_ops": [idx for idx, _ in pools], "conv_launches": [list(k) for k in eng.conv_launches],
            "pool_launches": [list(p) for p in eng.pool_launches],
            "pool_shapes": [[int(getattr(a, f)) for f in POOL_FIELDS] for _, a in pools],
            "group_launches": [[list(c), int(t)] for c, t in eng.group_launches]}


def record(model, name):
    from hawq_amd.engine_inception import InceptionEngine
    from hawq_amd.skeleton import synthetic_images
    opts, force = CONFIGS[name]
    x = synthetic_images(1, seed=1, size=299).cuda()
    u8 = torch.zeros(1, 299, 299, 3, dtype=torch.uint8, device="cuda")
    with torch.no_grad():
        if force is not None:
            probe = InceptionEngine(model, use_graph=False, **opts)
            probe(x)
            opts = dict(opts, plan=json.loads(json.dumps(forced_plan(probe, force))))
        eng = InceptionEngine(model, **opts)
        eng(x)
        eng.forward_uint8(u8)
    return describe(eng)


def dumps(lists):
    return "{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'), sort_keys=True)}" for k, v in lists.items()) + "\n}\n"


if __name__ == "__main__":
    model = calibrated_model()
    with open(sys.argv[1] if len(sys.argv) > 1 else OUT, "w") as f:
        f.write(dumps({name: record(model, name) for name in CONFIGS}))
