"""Pins oracle/oracle_inception.py (the CPU restatement of the frozen Q_InceptionV3 forward) to the LIVE reference's records
(tests/golden/make_inception_golden.py, written from the unmodified reference).  CPU only.

  net_inceptionv3_<scheme>_b2.npz         the operating point the GPU suite already uses: frozen state, unit digests, logits
  net_inceptionv3_<scheme>_b2_trace.npz   the same run: a digest of every QuantAct output and every conv accumulator, by name
  net_inceptionv3_<scheme>_b3_live2.npz   a second operating point (weights seed 1, calibrated on 2 images of seed 3, three other
                                          images of seed 11 evaluated): what justifies using the oracle off the first one
  b128_inceptionv3_<scheme>.npz           written by the oracle itself (tests/golden/make_b128_inception.py); one slice recomputed
"""
import hashlib

import numpy as np
import pytest

from tests import helpers as H

f32 = np.float32
SCHEMES = ["uniform8", "uniform4"]


def _sha8(w):
    return hashlib.sha256(np.ascontiguousarray(np.asarray(w).astype(np.int8)).tobytes()).hexdigest()


def _state(scheme, seed=0):
    from hawq_amd.api import build_quantized_resnet
    from oracle import oracle_inception as OI
    return OI.extract_float_state(build_quantized_resnet("inceptionv3", scheme, seed=seed))


def _load_frozen_state(st, fx):
    """a live record's ranges into `st`; returns the oracle ``ckpt`` of its integer buffers (scales, biases, weight patches, fc)"""
    from oracle import oracle_inception as OI
    acts, convs = OI.acts_of(st), OI.convs_of(st)
    assert [a["name"] for a in acts] == [str(n) for n in fx["act_names"]]
    assert [c["name"] for c in convs] == [str(n) for n in fx["conv_names"]]
    for i, a in enumerate(acts):
        a["x_min"], a["x_max"] = np.array([fx["act_x_min"][i]], f32), np.array([fx["act_x_max"][i]], f32)
    ck, off = {}, 0
    for li, c in enumerate(convs):
        co = c["w"].shape[0]
        ck[c["name"]] = dict(scale=fx["conv_scale"][off:off + co], bias=fx["conv_bias"][off:off + co],
                             wpatch=[(int(i), int(v)) for l, i, v in fx["conv_wpatch"] if l == li])
        off += co
    assert off == fx["conv_scale"].size
    ck[OI.FC] = dict(scale=fx["fc_scale"], bias=fx["fc_bias"])
    return ck


def _check_against_record(st, fx, x, tracefx=None):
    from oracle import oracle, oracle_inception as OI
    assert H.sha(x) == str(fx["input_sha"])
    ck = _load_frozen_state(st, fx)
    logits, tr = OI.forward_int(st, x, ckpt=ck)
    for i, a in enumerate(OI.acts_of(st)):   # the scale rule (quant_modules.py:262-270) on the recorded ranges
        assert oracle.act_scale(a["x_min"], a["x_max"], a["bits"], a["mode"])[0] == fx["act_scale"][i], a["name"]
    for li, c in enumerate(OI.convs_of(st)):   # own weight preparation + the recorded patches = the reference's integers
        assert _sha8(tr[c["name"] + ".weight_integer"]) == str(fx["conv_wsha"][li]), c["name"]
    assert _sha8(tr[OI.FC + ".weight_integer"]) == str(fx["fc_wsha"])
    assert [str(n) for n in fx["unit_names"]] == OI.unit_names(st)
    for i, n in enumerate(OI.unit_names(st)):
        assert np.array_equal(H.digest(OI.unit_output(tr, n)), fx["unit_digest"][i]), n
    assert np.array_equal(logits, fx["logits"]) and np.array_equal(logits.argmax(1), fx["top1"])
    if tracefx is not None:
        assert str(tracefx["input_sha"]) == str(fx["input_sha"]) and np.array_equal(tracefx["logits"], fx["logits"])
        assert [str(n) for n in tracefx["act_names"]] == [a["name"] for a in OI.acts_of(st)]
        assert [str(n) for n in tracefx["conv_names"]] == [c["name"] for c in OI.convs_of(st)]
        for i, n in enumerate(str(v) for v in tracefx["act_names"]):
            assert np.array_equal(H.digest(tr[n + ".q"]), tracefx["act_outdigest"][i]), n
            assert int(np.abs(tr[n + ".q"]).max()) == int(tracefx["act_outmax"][i]), n
        for i, n in enumerate(str(v) for v in tracefx["conv_names"]):
            assert np.array_equal(H.digest(tr[n + ".acc"]), tracefx["conv_accdigest"][i]), n
        assert np.array_equal(tr[OI.FC + ".acc"], tracefx["fc_acc"])
    return logits, tr


@pytest.mark.parametrize("scheme", SCHEMES)
def test_inception_oracle_matches_the_live_reference_fixture_and_its_trace(scheme):
    """On the recorded frozen state (ranges, conv_scale, conv_bias, patched weights checked by conv_wsha, fc records) the oracle
    gives every unit_digest and all logits bit for bit, and every QuantAct output and conv accumulator of the trace record."""
    from hawq_amd.skeleton import synthetic_images
    fx, tfx = H.load(f"net_inceptionv3_{scheme}_b2.npz"), H.load(f"net_inceptionv3_{scheme}_b2_trace.npz")
    assert len(tfx["act_names"]) == 162 and len(tfx["conv_names"]) == 94
    _check_against_record(_state(scheme), fx, synthetic_images(2, seed=0, size=299).numpy(), tfx)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_inception_oracle_matches_the_second_live_record(scheme):
    """Another weight seed, ranges calibrated on images other than the three evaluated, batch 3: logits, unit digests, the trace."""
    from hawq_amd.skeleton import synthetic_images
    fx = H.load(f"net_inceptionv3_{scheme}_b3_live2.npz")
    b, seed = (int(v) for v in fx["images"])
    assert (b, seed) == (3, 11) and int(fx["model_seed"]) == 1 and [int(v) for v in fx["calib"]] == [2, 3]
    fx0 = H.load(f"net_inceptionv3_{scheme}_b2.npz")
    assert str(fx["input_sha"]) != str(fx0["input_sha"]) and not np.array_equal(fx["act_x_max"], fx0["act_x_max"])
    _check_against_record(_state(scheme, seed=1), fx, synthetic_images(b, seed=seed, size=299).numpy(), fx)


@pytest.mark.parametrize("scheme,record", [(s, r) for s in SCHEMES for r in ("b2", "b3_live2")])
def test_inception_ieee_prep_differs_from_reference_only_by_sqrt_quirk_and_calibration_agrees(scheme, record):
    """The oracle's own preparation from the float parameters, and its own calibration (calibrate=True on the record's calibration
    images): weight integers equal the reference's except at the entries listed in conv_wpatch; calibrated ranges equal the
    record's whenever the scales do - and then so do the logits.  Scales: torch-CPU's sqrt may return the neighbouring binary32
    (a relative 2^-23 at most); the three binary32 operations behind it (gamma / std, w * factor, max|w| / n) carry that through
    and each re-rounds both chains (up to 2^-24 apiece, 2^-23 between them), so the scales agree within 4 * 2^-23."""
    from hawq_amd.skeleton import synthetic_images
    from oracle import oracle_inception as OI
    fx = H.load(f"net_inceptionv3_{scheme}_{record}.npz")
    live2 = record != "b2"
    st = _state(scheme, seed=int(fx["model_seed"]) if live2 else 0)
    cb, cs = (int(v) for v in fx["calib"]) if live2 else (2, 0)
    eb, es = (int(v) for v in fx["images"]) if live2 else (2, 0)
    _, tr = OI.forward_int(st, synthetic_images(cb, seed=cs, size=299).numpy(), calibrate=True)
    patched = {int(l) for l, _, _ in fx["conv_wpatch"]}
    off, ndiff = 0, 0
    for li, c in enumerate(OI.convs_of(st)):
        s = tr[c["name"] + ".convbn_scaling_factor"]
        ref = fx["conv_scale"][off:off + s.size]
        off += s.size
        assert np.all(np.abs(s.astype(np.float64) - ref) <= 4 * 2.0 ** -23 * np.abs(ref)), c["name"]
        ndiff += int((s != ref).sum())
        if li not in patched:   # elsewhere the IEEE weights ARE the reference's
            assert _sha8(tr[c["name"] + ".weight_integer"]) == str(fx["conv_wsha"][li]), c["name"]
        else:
            w = tr[c["name"] + ".weight_integer"].copy()
            for l, i, v in fx["conv_wpatch"]:
                if l == li:
                    assert w.reshape(-1)[i] != v
                    w.reshape(-1)[i] = v
            assert _sha8(w) == str(fx["conv_wsha"][li]), c["name"]
    assert _sha8(tr[OI.FC + ".weight_integer"]) == str(fx["fc_wsha"])
    assert len(fx["conv_wpatch"]) <= 4 and ndiff < 0.02 * off
    # calibration: on the reference's own weight integers, scales and biases (ckpt) the oracle's un-frozen forward must freeze
    # the record's ranges exactly - every QuantAct sees the reference's fp32 tensor - and then give its logits
    st = _state(scheme, seed=int(fx["model_seed"]) if live2 else 0)
    x_min, x_max = fx["act_x_min"], fx["act_x_max"]
    ck = _load_frozen_state(st, fx)
    for a in OI.acts_of(st):
        a["x_min"], a["x_max"] = np.zeros(1, f32), np.zeros(1, f32)
    OI.forward_int(st, synthetic_images(cb, seed=cs, size=299).numpy(), calibrate=True, ckpt=ck)
    assert [n for n, _, _ in st["ranges"]] == [str(n) for n in fx["act_names"]]
    for i, (n, lo, hi) in enumerate(st["ranges"]):
        assert lo[0] == x_min[i] and hi[0] == x_max[i], n
    y, _ = OI.forward_int(st, synthetic_images(eb, seed=es, size=299).numpy(), ckpt=ck)
    assert np.array_equal(y, fx["logits"])
    print(f"{scheme} {record}: {ndiff} of {off} IEEE scales differ from the reference's, {len(fx['conv_wpatch'])} patched weights")


def test_inception_uint8_entry_is_the_float_pipeline_written_out():
    """normalize_uint8 against torch's own ToTensor + Normalize arithmetic for every (channel, byte) pair, and the uint8 entry against
    the fp32 entry on that tensor."""
    import torch
    from oracle import oracle_inception as OI
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    u = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1).repeat(3, 3)
    t = torch.from_numpy(u).permute(0, 3, 1, 2).to(torch.float32).div(255)
    t = t.sub(torch.tensor(mean).view(1, 3, 1, 1)).div(torch.tensor(std).view(1, 3, 1, 1))
    assert np.array_equal(OI.normalize_uint8(u, mean, std), t.numpy())


@pytest.mark.parametrize("scheme", SCHEMES)
def test_b128_inception_fixture_is_what_the_oracle_computes(scheme):
    """tests/golden/b128_inceptionv3_*.npz (the workload tools/inception_bench.py times, at batch 128) were written by
    tests/golden/make_b128_inception.py from this oracle: recalibrate, recompute one slice and its per-unit hashes."""
    from hawq_amd.skeleton import synthetic_images
    from oracle import oracle_inception as OI
    fx = H.load(f"b128_inceptionv3_{scheme}.npz")
    st = _state(scheme)
    OI.forward_int(st, synthetic_images(int(fx["calib"]), seed=int(fx["calib_seed"]), size=299).numpy(), calibrate=True)
    assert [n for n, _, _ in st["ranges"]] == [str(n) for n in fx["act_names"]]
    assert np.array_equal(np.array([lo[0] for _, lo, _ in st["ranges"]], f32), fx["act_x_min"])
    assert np.array_equal(np.array([hi[0] for _, _, hi in st["ranges"]], f32), fx["act_x_max"])
    x = synthetic_images(128, seed=int(fx["seed"]), size=299).numpy()
    assert H.sha(x) == str(fx["input_sha"])
    s, k = int(fx["slice"]), 5
    assert fx["logits"].shape == (128, 1000) and fx["unit_sha"].shape == (128 // s, 11)
    y, tr = OI.forward_int(st, x[k * s:(k + 1) * s])
    assert np.array_equal(y, fx["logits"][k * s:(k + 1) * s])
    assert np.array_equal(fx["logits"].argmax(1), fx["top1"])
    for n, want in zip(fx["unit_names"], fx["unit_sha"][k]):
        assert H.sha(OI.unit_output(tr, str(n)).astype(np.int16)) == str(want), n


def test_inception_oracle_imports_nothing_numeric_from_the_product():
    """structure only: hawq_amd.skeleton (and bit_schedules) - never quant_utils, quant_modules, engine_inception or _lib"""
    import ast
    import os
    src = open(os.path.join(os.path.dirname(H.GOLDEN), "..", "oracle", "oracle_inception.py")).read()
    mods = set()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.ImportFrom) and node.module:
            mods.add(node.module)
            mods.update(f"{node.module}.{a.name}" for a in node.names)
        elif isinstance(node, ast.Import):
            mods.update(a.name for a in node.names)
    product = {m for m in mods if m.startswith("hawq_amd")}
    assert product and all(m.startswith(("hawq_amd.skeleton", "hawq_amd.bit_schedules")) for m in product), product
