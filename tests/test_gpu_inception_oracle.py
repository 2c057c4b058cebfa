"""InceptionV3 on the GPU against an INDEPENDENT computation: oracle/oracle_inception.py, the CPU restatement of the reference's
frozen integer forward that tests/test_oracle_inception_vs_golden.py pins to the live reference at two operating points.  Unlike
the GPU-against-GPU equalities of the other InceptionV3 files, nothing here shares a kernel, a table builder or a clamp rule
with what it checks: full tensors of every unit output (``eng.unit_output``) and the logits, bit for bit, no tolerance.

Off the fixtures' operating point: weights of seed 1, ranges calibrated by the ORACLE on two images of seed 3 (and, in a test of
its own, by the device - the two must agree exactly), evaluated on images of other seeds at batches 1, 5 and 17 (17 leaves a
ragged last pixel tile on every map), for uniform8 and uniform4, through the default plan, every conv tile id forced wherever
``tile_ok`` accepts it, the tuned plan - each as a captured graph and launch by launch - and ``forward_modules``, whose
QuantBnConv2d / QuantAct hooks are held to the oracle's per-conv accumulators and per-QuantAct integers (a failure names the launch).
The uint8 entry against the oracle's float32 ToTensor + Normalize; the batch-128 configuration of tools/inception_bench.py --tune
against tests/golden/b128_inceptionv3_*.npz (written by the oracle, tests/golden/make_b128_inception.py).

Oracle cost: about 1.2 s per image on 8 threads, less on 16.  Live oracle images per scheme in this file: 2 (calibration) + 1 + 5 + 17 (unseen
inputs) + 1 (narrowed concat ranges) + 2 (uint8) + 4 (one slice of the batch-128 fixture) = 32, cached per (scheme, seed, batch) within the module - the order
of the 16-image ResNet50 slice tests/test_gpu_b128.py recomputes per configuration (32 x 5.7 against 16 x 4.1 GMAC).
This file never reads the reference tree.
"""
import json

import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu

SCHEMES = ["uniform8", "uniform4"]
W_SEED, CAL = 1, (2, 3)            # weight seed; calibration (batch, image seed)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
_CACHE = {}


def _images(b, seed):
    from hawq_amd.skeleton import synthetic_images
    return synthetic_images(b, seed=seed, size=299)


def _state(scheme, narrow=False):
    """the oracle's state for (scheme, W_SEED), calibrated BY THE ORACLE on CAL (cached).  ``narrow``: a copy whose concat ranges
    (every q_rescaling_activ, the units' and Inception-C's inner ones) are a quarter of the calibrated ones - ranges that are not
    nested, as the running averages of a trained checkpoint need not be (quant_modules.py:252-258): a branch's 16-bit values then
    reach past the unit's range and the concat requant's clamp decides (quant_utils.py:410-413)."""
    key = ("state", scheme, narrow)
    if key not in _CACHE:
        import copy
        from hawq_amd.api import build_quantized_resnet
        from oracle import oracle_inception as OI
        if narrow:
            st = copy.deepcopy(_state(scheme))
            for a in OI.acts_of(st):
                if a["name"].endswith("q_rescaling_activ"):
                    a["x_min"], a["x_max"] = a["x_min"] * np.float32(0.25), a["x_max"] * np.float32(0.25)
        else:
            st = OI.extract_float_state(build_quantized_resnet("inceptionv3", scheme, seed=W_SEED))
            OI.forward_int(st, _images(*CAL).numpy(), calibrate=True)
        _CACHE[key] = st
    return _CACHE[key]


def _oracle(scheme, seed, batch, u8=False, narrow=False):
    """dict(logits, units {name: int64 NCHW}, tr) of the oracle on images (batch, seed), cached per (scheme, seed, batch); the
    whole trace (accumulators as int32, QuantAct integers as int32) is kept for batches of at most 5 images"""
    key = (scheme, seed, batch, u8, narrow)
    if key not in _CACHE:
        from oracle import oracle_inception as OI
        st = _state(scheme, narrow)
        x = _u8_images(batch, seed).numpy() if u8 else _images(batch, seed).numpy()
        ys, units, tr_keep = [], {n: [] for n in OI.unit_names(st)}, None
        for b0 in range(0, batch, 6):   # a frozen forward treats every image on its own: slices bound the trace's memory
            y, tr = (OI.forward_uint8(st, x[b0:b0 + 6], MEAN, STD) if u8 else OI.forward_int(st, x[b0:b0 + 6]))
            ys.append(y)
            for n in units:
                units[n].append(OI.unit_output(tr, n))
            if batch <= 5:
                tr_keep = {k: v.astype(np.int32) for k, v in tr.items() if k.endswith((".acc", ".q"))}
            del tr
        _CACHE[key] = dict(logits=np.concatenate(ys), units={n: np.concatenate(v) for n, v in units.items()}, tr=tr_keep)
    return _CACHE[key]


def _u8_images(b, seed):
    return torch.randint(0, 256, (b, 299, 299, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _model(scheme, narrow=False):
    """hawq_amd's model for (scheme, W_SEED) on the GPU, frozen on the ranges of the ORACLE's state"""
    from hawq_amd.api import build_quantized_resnet
    from hawq_amd.quant_modules import QuantAct, freeze_model
    from oracle import oracle_inception as OI
    ranges = OI.acts_of(_state(scheme, narrow))
    model = build_quantized_resnet("inceptionv3", scheme, seed=W_SEED).cuda()
    acts = [(n, m) for n, m in model.named_modules() if isinstance(m, QuantAct)]
    assert [n for n, _ in acts] == [a["name"] for a in ranges]
    for (n, m), a in zip(acts, ranges):
        m.x_min.fill_(float(a["x_min"][0])), m.x_max.fill_(float(a["x_max"][0]))
        m.compute_scale()
    freeze_model(model)
    model.eval()
    return model


def _num_tiles():
    from hawq_amd import _lib
    return _lib.load().hawq_incep_conv_num_tiles()


def _forced_plan(eng, tile):
    """`tile` on every conv launch of eng's current batch shape that accepts it, tile 0 elsewhere; some launch must accept it"""
    from hawq_amd.engine_inception import make_plan
    keys = eng.conv_launches
    tiles = [tile if eng._tile_ok(i, tile) else 0 for i in range(len(keys))]
    assert tiles.count(tile) > 0, f"tile {tile} is accepted by no conv launch of the network"
    return json.loads(json.dumps(make_plan(eng._batch, keys, _num_tiles(), tiles, [{} for _ in keys])))


def _assert_engine_equals(eng, y, ref, what):
    for n, want in ref["units"].items():   # first, so that a failure names the earliest unit that differs
        got = eng.unit_output(n)
        assert got.shape == want.shape, (what, n)
        assert np.array_equal(got, want), f"{what}: {n}: {int((got != want).sum())} of {want.size} values differ from the oracle"
    y = y.cpu().numpy()
    assert np.array_equal(y, ref["logits"]), f"{what}: logits of {int((y != ref['logits']).any(1).sum())} images differ"


def _engines(model, x, graphs=(True, False)):
    """(description, engine) of every plan under test, each already built for x's batch shape: default, every forced tile, tuned"""
    from hawq_amd.engine_inception import InceptionEngine
    for use_graph in graphs:
        mode = "graph" if use_graph else "eager"
        base = InceptionEngine(model, use_graph=use_graph)
        yield f"default plan, {mode}", base
        assert base._batch == (x.shape[0], x.shape[2], x.shape[3])   # the caller ran it: its launch list is what tile_ok judges
        for tile in range(1, _num_tiles() + 1):
            plan = _forced_plan(base, tile)
            eng = InceptionEngine(model, use_graph=use_graph, plan=plan)
            yield f"tile {tile} forced on {plan['tiles'].count(tile)} launches, {mode}", eng
            assert eng.conv_tiles == plan["tiles"] and eng.n_timing_launches == 0
        eng = InceptionEngine(model, use_graph=use_graph, tune=True)
        yield f"tuned plan, {mode}", eng
        assert eng.n_timing_launches > 0 and len(eng.conv_tiles) == 95


@pytest.mark.parametrize("batch", [1, 5, 17])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_plans_match_the_oracle_on_unseen_inputs(scheme, batch):
    """logits and the full tensor of every unit output, for the default plan, every forced tile, the tuned plan - graph (run, then
    replayed) and eager"""
    seed = 20 + batch
    ref = _oracle(scheme, seed, batch)
    assert np.abs(ref["logits"]).max() > 0 and all(np.abs(v).max() > 0 for v in ref["units"].values())
    model = _model(scheme)
    x = _images(batch, seed).cuda()
    seen = []
    with torch.no_grad():
        for what, eng in _engines(model, x):
            y = eng(x)
            _assert_engine_equals(eng, y, ref, f"{scheme} b{batch} {what}")
            if eng.use_graph:
                assert eng._graph is not None
                _assert_engine_equals(eng, eng(x), ref, f"{scheme} b{batch} {what}, replay")
            seen.append(what)
    assert len(seen) == 2 * (2 + _num_tiles())


@pytest.mark.parametrize("scheme", SCHEMES)
def test_plans_match_the_oracle_where_the_concat_clamp_decides(scheme):
    """Ranges that are not nested (``_state(narrow=True)``): branch values beyond the unit's range, so the clamp of the concat
    requant - REQUANT2's second clamp, the max-pool branch's and the inner concat's post clamp - is what the result hangs on.
    One image; every plan, and the module path."""
    ref = _oracle(scheme, 31, 1, narrow=True)
    sat = {n: int((np.abs(v) >= 32767).sum()) for n, v in ref["units"].items()}
    assert all(c > 0 for c in sat.values()), sat   # every unit output does saturate
    model = _model(scheme, narrow=True)
    x = _images(1, 31).cuda()
    with torch.no_grad():
        for what, eng in _engines(model, x, graphs=(True,)):
            _assert_engine_equals(eng, eng(x), ref, f"{scheme} narrow ranges, {what}")
        units = {}
        hooks = [m.register_forward_hook(lambda mod, i, o, name=name: units.__setitem__(
            name, torch.round(o[0].double() / o[1].double().reshape(-1)[0]).long().cpu().numpy())) for name, m in model.units()]
        y = model.forward_modules(x).cpu().numpy()
        for h in hooks:
            h.remove()
    for n, want in ref["units"].items():
        assert np.array_equal(units[n], want), n
    assert np.array_equal(y, ref["logits"])


@pytest.mark.parametrize("batch", [1, 5, 17])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_module_path_matches_the_oracle_launch_by_launch(scheme, batch):
    """forward_modules: logits and every unit output; at batches 1 and 5 also, through forward hooks, the int32 accumulators of
    every QuantBnConv2d and the integers behind every QuantAct, against the oracle's trace by module name"""
    from hawq_amd.quant_modules import QuantAct, QuantBnConv2d
    seed = 20 + batch
    ref = _oracle(scheme, seed, batch)
    model = _model(scheme)
    tr, bad, n_checked, hooks, units = ref["tr"], [], [0, 0], [], {}

    def conv_hook(mod, inp, out, name):
        acc, (n, ho, wo, cp) = mod.last_accumulators
        got = acc.view(n, ho, wo, cp)[..., :mod.out_channels].permute(0, 3, 1, 2).cpu().numpy()
        n_checked[0] += 1
        if not np.array_equal(got, tr[name + ".acc"]):
            bad.append(name + ".acc")

    def act_hook(mod, inp, out, name):
        got = torch.round(out[0].double() / out[1].double().reshape(-1)[0]).to(torch.int32).cpu().numpy()
        n_checked[1] += 1
        if not np.array_equal(got, tr[name + ".q"]):
            bad.append(name + ".q")

    if tr is not None:
        for name, m in model.named_modules():
            if isinstance(m, QuantBnConv2d):
                hooks.append(m.register_forward_hook(lambda mod, i, o, name=name: conv_hook(mod, i, o, name)))
            elif isinstance(m, QuantAct):
                hooks.append(m.register_forward_hook(lambda mod, i, o, name=name: act_hook(mod, i, o, name)))
    for name, m in model.units():
        hooks.append(m.register_forward_hook(lambda mod, i, o, name=name: units.__setitem__(
            name, torch.round(o[0].double() / o[1].double().reshape(-1)[0]).long().cpu().numpy())))
    with torch.no_grad():
        y = model.forward_modules(_images(batch, seed).cuda()).cpu().numpy()
    for h in hooks:
        h.remove()
    assert not bad, f"{scheme} b{batch}: first launches off the oracle (in execution order): {bad[:6]} ({len(bad)} in all)"
    if tr is not None:
        assert n_checked == [94, 162]
    else:
        assert batch > 5
    assert list(units) == list(ref["units"])
    for n, want in ref["units"].items():
        assert np.array_equal(units[n], want), n
    assert np.array_equal(y, ref["logits"])


@pytest.mark.parametrize("scheme", SCHEMES)
def test_forward_uint8_matches_the_oracles_uint8_entry(scheme):
    """random uint8 NHWC images: the stem kernel's table look-up against float32 ToTensor + Normalize + the input QuantAct written
    out on the host, then the whole network: logits and every unit output, default and tuned plan, run and replay"""
    from hawq_amd.engine_inception import InceptionEngine
    ref = _oracle(scheme, 4, 2, u8=True)
    model = _model(scheme)
    u8 = _u8_images(2, 4).cuda()
    with torch.no_grad():
        for what, eng in (("default", InceptionEngine(model)), ("tuned", InceptionEngine(model, tune=True)),
                          ("eager", InceptionEngine(model, use_graph=False))):
            _assert_engine_equals(eng, eng.forward_uint8(u8, MEAN, STD), ref, f"{scheme} uint8 {what}")
            _assert_engine_equals(eng, eng.forward_uint8(u8, MEAN, STD), ref, f"{scheme} uint8 {what}, again")
            assert eng.n_launches_u8 == 145


@pytest.mark.parametrize("scheme", SCHEMES)
def test_device_calibration_gives_the_oracles_ranges(scheme):
    """calibrate(model, x) - the un-frozen module path, min / max kernels included - freezes exactly the ranges of the oracle's
    calibrate=True forward, for weights and images other than the fixtures'"""
    from hawq_amd.api import build_quantized_resnet, calibrate
    from hawq_amd.quant_modules import QuantAct
    st = _state(scheme)
    model = build_quantized_resnet("inceptionv3", scheme, seed=W_SEED).cuda()
    calibrate(model, _images(*CAL).cuda())
    acts = [(n, m) for n, m in model.named_modules() if isinstance(m, QuantAct)]
    assert [n for n, _ in acts] == [n for n, _, _ in st["ranges"]] and len(acts) == 162
    off = [(n, float(m.x_min), float(lo[0]), float(m.x_max), float(hi[0])) for (n, m), (_, lo, hi) in zip(acts, st["ranges"])
           if np.float32(float(m.x_min)) != lo[0] or np.float32(float(m.x_max)) != hi[0]]
    assert not off, f"{len(off)} of {len(acts)} ranges differ; first (name, device min, oracle min, device max, oracle max): {off[0]}"


@pytest.mark.parametrize("scheme", SCHEMES)
def test_benchmarked_configuration_matches_the_oracle_fixture_at_batch_128(scheme):
    """The engines tools/inception_bench.py --tune builds (weights seed 0, ranges calibrated on the device on 2 images of seed 0,
    128 images of seed 1; the fixed plan and the tuned plan) and every forced tile at that batch: all 128 x 1000 logits and the
    SHA-256 of every unit output per slice equal tests/golden/b128_inceptionv3_<scheme>.npz; the last slice is recomputed by the
    oracle here, from the ranges the device froze."""
    import gc
    from hawq_amd.api import build_quantized_resnet, calibrate
    from hawq_amd.engine_inception import InceptionEngine
    from hawq_amd.quant_modules import QuantAct
    from oracle import oracle_inception as OI
    fx = H.load(f"b128_inceptionv3_{scheme}.npz")
    model = build_quantized_resnet("inceptionv3", scheme, seed=0).cuda()
    calibrate(model, _images(int(fx["calib"]), int(fx["calib_seed"])).cuda())
    acts = [(n, m) for n, m in model.named_modules() if isinstance(m, QuantAct)]
    assert [n for n, _ in acts] == [str(n) for n in fx["act_names"]]
    assert np.array_equal(np.array([float(m.x_min) for _, m in acts], np.float32), fx["act_x_min"])
    assert np.array_equal(np.array([float(m.x_max) for _, m in acts], np.float32), fx["act_x_max"])
    x = _images(128, int(fx["seed"]))
    assert H.sha(x.numpy()) == str(fx["input_sha"])
    xd, s = x.cuda(), int(fx["slice"])
    names = [str(n) for n in fx["unit_names"]]
    assert names == [n for n, _ in model.units()] and fx["unit_sha"].shape == (128 // s, len(names))

    def check(eng, what):
        with torch.no_grad():
            y = eng(xd)
            y2 = eng(xd)   # the replay of the captured graph, as the timed loop runs it
        assert eng.use_graph and eng._graph is not None and eng._batch == (128, 299, 299)
        for ui, n in enumerate(names):
            u = eng.unit_output(n)
            assert u.shape[0] == 128 and np.abs(u).max() < 32768
            for k in range(128 // s):
                assert H.sha(u[k * s:(k + 1) * s].astype(np.int16)) == str(fx["unit_sha"][k][ui]), (what, n, f"slice {k}")
        y = y.cpu().numpy()
        assert np.array_equal(y, fx["logits"]), f"{what}: {int((y != fx['logits']).any(1).sum())} of 128 images differ"
        assert np.array_equal(y.argmax(1), fx["top1"]) and np.array_equal(y2.cpu().numpy(), y)

    fixed = InceptionEngine(model)
    check(fixed, "fixed plan")
    plans = [(t, _forced_plan(fixed, t)) for t in range(1, _num_tiles() + 1)]
    del fixed
    tuned = InceptionEngine(model, tune=True)
    check(tuned, "tuned plan")
    assert tuned.n_timing_launches > 0 and len(tuned.conv_tiles) == 95
    print(f"{scheme}: tuned tiles at batch 128: {''.join(str(t) for t in tuned.conv_tiles)}")
    del tuned
    for t, plan in plans:
        gc.collect(), torch.cuda.empty_cache()
        eng = InceptionEngine(model, plan=plan)
        check(eng, f"tile {t} forced on {plan['tiles'].count(t)} launches")
        assert eng.conv_tiles == plan["tiles"]
        del eng
    # one slice recomputed by the oracle on this machine, from the ranges the DEVICE calibration froze
    st = OI.extract_float_state(model)
    ref, tr = OI.forward_int(st, x[128 - s:].numpy())
    assert np.array_equal(ref, fx["logits"][128 - s:])
    assert [H.sha(OI.unit_output(tr, n).astype(np.int16)) for n in names] == [str(v) for v in fx["unit_sha"][-1]]
