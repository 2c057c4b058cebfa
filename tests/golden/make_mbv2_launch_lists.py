"""Writes tests/golden/mbv2_launch_lists.json: the launch lists of the MobileNetV2 engine (hawq_amd/engine_mbv2.py) per configuration -
what tests/test_gpu_mbv2_launch_lists.py compares a rebuilt engine with.  Needs the MI355X (the engine asks the library which units,
stem and classifier launches it takes).  Run from the repository root:

    python tests/golden/make_mbv2_launch_lists.py [OUT]

``mobilenetv2_w1``, seed 0, calibrated on ``synthetic_images(2, seed=0)``; HAWQ_MBV2_TILES=0 (the library's heuristic tiles: no tuning,
no timing); the switches of a configuration are set for its engine alone and the environment is restored afterwards.

Per configuration, one line of the file.  ``chains``: per launch chain (two under ``two_chains``) the fp32 launches ``ops`` and the
``forward_uint8`` launches ``ops_u8`` (null for the tapped plan, which has no graph and runs fp32 images alone), each launch as
[entry point, arguments before the stream]; ``n_fused_units``, ``n_fast_closing``, ``stem`` (``_stem_args is not None``) and ``taps``
(name -> [shape, true channels, dtype]).  Of the whole engine: ``n_launches``, ``fast_requant_launches``, ``total_plan_bytes``.
An argument is an integer, a float, or - a ctypes block - the list of its fields in the order of ``hawq_amd._lib`` (a nested block
a nested list).  Every pointer (argument or field) is replaced by the index of its address's first appearance in that chain, NULL by
null: the wiring of activations, weights, tables, ``x_in`` and ``logits`` without the addresses.  The calibration is the same in
every process (two runs on the commit below gave identical files), so the requant scalars and ``fast_tables`` words are recorded
too: no field is left out.  The file was first recorded on the commit before the engine got its launch records, by this script with
``chain_ops`` putting ``_u8_op`` at ``_u8_index`` of ``_ops``; this version reproduces it byte for byte.
"""
import ctypes as C
import json
import os
import sys
from functools import lru_cache

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "tests", "golden", "mbv2_launch_lists.json")
SWITCHES = ("HAWQ_MBV2_UNFUSED", "HAWQ_MBV2_EXACT", "HAWQ_MBV2_PAD64", "HAWQ_MBV2_UNIT_TILE", "HAWQ_MBV2_NO_WIDE_UNITS", "HAWQ_NO_FC2",
            "HAWQ_MBV2_CHAINS", "HAWQ_MBV2_TILES")
ODD = (72, 104)   # the tiles hang over every edge: maps 36 x 52 ... 3 x 4
CONFIGS = {   # name -> (scheme, batch, (H, W), environment, engine options)
    "default": ("uniform8", 3, (224, 224), {}, {"chains": 1}),
    "odd": ("bops_0.5", 3, ODD, {}, {"chains": 1}),
    "unfused": ("uniform8", 3, ODD, {"HAWQ_MBV2_UNFUSED": "1"}, {"chains": 1}),
    "exact": ("uniform8", 3, ODD, {"HAWQ_MBV2_EXACT": "1"}, {"chains": 1}),
    "pad64": ("uniform8", 3, ODD, {"HAWQ_MBV2_PAD64": "1"}, {"chains": 1}),
    "unit_tile_1": ("uniform8", 3, ODD, {"HAWQ_MBV2_UNIT_TILE": "1"}, {"chains": 1}),
    "no_wide": ("uniform8", 3, ODD, {"HAWQ_MBV2_NO_WIDE_UNITS": "1"}, {"chains": 1}),
    "no_fc2": ("uniform8", 3, ODD, {"HAWQ_NO_FC2": "1"}, {"chains": 1}),
    "tapped": ("uniform8", 2, ODD, {}, {"chains": 1, "keep_accumulators": True}),
    "two_chains": ("uniform8", 5, ODD, {}, {"chains": 2}),   # sub-batches 3 and 2
}


@lru_cache(maxsize=None)
def calibrated_model(scheme):
    from hawq_amd.api import build_quantized_model, calibrate
    from hawq_amd.skeleton import synthetic_images
    model = build_quantized_model("mobilenetv2_w1", scheme, seed=0).cuda()
    calibrate(model, synthetic_images(2, seed=0).cuda())
    return model


def chain_ops(sub):
    """(the fp32 launches, the uint8 launches or None) of one chain"""
    return sub._ops, sub._ops_u8


def _block(b, addr):
    out = []
    for field, ftype in b._fields_:
        v = getattr(b, field)
        out.append(addr(v) if ftype is C.c_void_p else _block(v, addr) if isinstance(v, C.Structure) else int(v))
    return out


def describe_ops(ops):
    from hawq_amd import _lib
    seen = {}

    def addr(p):
        return None if not p else seen.setdefault(int(p), len(seen))

    out = []
    for op in ops:
        name, args = op.args[0], op.args[1:-1]   # (the last argument is the stream)
        types = _lib.SIGNATURES[name][:len(args)]
        out.append([name, [_block(a._obj, addr) if hasattr(a, "_obj") else addr(a) if t is C.c_void_p else
                           float(a) if t is C.c_float else int(a) for t, a in zip(types, args)]])
    return out


def describe(eng, with_u8):
    """the launch lists of an engine that has run ``eng(x)`` and, `with_u8`, ``eng.forward_uint8(u8)``"""
    chains = []
    for sub in (eng.subs or [eng]):
        ops, ops_u8 = chain_ops(sub)
        chains.append({"ops": describe_ops(ops), "ops_u8": describe_ops(ops_u8) if with_u8 else None,
                       "n_fused_units": sub.n_fused_units, "n_fast_closing": sub.n_fast_closing, "stem": sub._stem_args is not None,
                       "taps": {k: [list(shp), c, str(t.dtype)] for k, (t, shp, c) in sub.taps.items()}})
    return {"chains": chains, "n_launches": eng.n_launches, "fast_requant_launches": eng.fast_requant_launches,
            "total_plan_bytes": eng.total_plan_bytes}


def record(name):
    from hawq_amd.engine_mbv2 import MobileNetV2Engine
    from hawq_amd.skeleton import synthetic_images
    scheme, n, (h, w), env, opts = CONFIGS[name]
    model = calibrated_model(scheme)
    x = synthetic_images(n, seed=1)[:, :, :h, :w].contiguous().cuda()
    u8 = torch.zeros(n, h, w, 3, dtype=torch.uint8, device="cuda")
    with_u8 = not opts.get("keep_accumulators")
    saved = {k: os.environ.pop(k) for k in SWITCHES if k in os.environ}
    os.environ.update({"HAWQ_MBV2_TILES": "0"}, **env)
    try:
        with torch.no_grad():
            eng = MobileNetV2Engine(model, **opts)
            eng(x)
            if with_u8:
                eng.forward_uint8(u8)
        return describe(eng, with_u8)
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(saved)


def dumps(lists):
    return "{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'), sort_keys=True)}" for k, v in lists.items()) + "\n}\n"


if __name__ == "__main__":
    with open(sys.argv[1] if len(sys.argv) > 1 else OUT, "w") as f:
        f.write(dumps({name: record(name) for name in CONFIGS}))
