"""Generate the InceptionV3 fixtures from the LIVE reference (build container only).

    python tests/golden/make_inception_golden.py --base   # writes tests/golden/net_inceptionv3_{uniform8,uniform4}_b2.npz
                                                          #    and tests/golden/inceptionv3_names.json
    python tests/golden/make_inception_golden.py          # writes net_inceptionv3_{scheme}_b2_trace.npz (the SAME run as
                                                          #    the _b2 files, which it reads and leaves alone) and
                                                          #    net_inceptionv3_{scheme}_b3_live2.npz (a second operating point)

Runs /root/reference's utils/models/q_inceptionv3.py unmodified (through oracle/ref_live.py's loader) on the seeded float
skeleton (hawq_amd.skeleton.build_float_inceptionv3) and synthetic 299 x 299 images, calibrates on the evaluated batch and
records:
  act_names / act_x_min / act_x_max / act_scale   every QuantAct's frozen range and scale
  conv_names / conv_scale / conv_bias             every QuantBnConv2d's weight scales and integer biases
  conv_wsha / conv_wpatch                         SHA-256 of each weight_integer (int8) and the entries where torch-CPU's
                                                  non-IEEE sqrt moved a weight against hawq_amd's IEEE preparation
  fc_scale / fc_bias / fc_wsha                    the classifier's
  unit_names / unit_digest                        digest of every unit's integer output (after its q_rescaling_activ)
  logits / top1, input_sha / weights_sha
The trace files add, for that same run (their logits must equal the recorded ones), by module name:
  act_names / act_outdigest / act_outmax          digest and largest magnitude of every QuantAct's integer output
  conv_names / conv_accdigest                     digest of rint(raw F.conv2d output) = accumulator + bias of every QuantBnConv2d
  fc_acc                                          rint(raw F.linear output)
The live2 files are a second record off that operating point: weights of seed 1, ranges calibrated on two images of seed 3,
three OTHER images (seed 11) evaluated; they hold the whole frozen state, unit digests, logits and the trace arrays.
The reference tree does not exist on the GPU machines, so its results travel as these files.
"""
from __future__ import annotations

import hashlib
import importlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import ref_live  # noqa: E402
from hawq_amd.bit_schedules import get_bit_config  # noqa: E402
from hawq_amd.quant_utils import fold_bn, quantize_weight_per_channel  # noqa: E402
from hawq_amd.skeleton import build_float_inceptionv3, init_synthetic, synthetic_images  # noqa: E402

BATCH = 2


def digest(a) -> np.ndarray:
    """Order-sensitive 3-word digest of an integer tensor in its given (NCHW) order (as make_golden.py)."""
    a = np.ascontiguousarray(a).astype(np.int64).reshape(-1)
    w = (np.arange(a.size, dtype=np.int64) % 8191) + 1
    with np.errstate(over="ignore"):
        return np.array([a.sum(), np.abs(a).sum(), (a * w).sum()], np.int64)


def sha(t) -> str:
    return hashlib.sha256(np.ascontiguousarray(t).tobytes()).hexdigest()


def reference_model(scheme, seed=0):
    ref_live.load_reference()
    qi = importlib.import_module("utils.models.q_inceptionv3")
    q = qi.q_inceptionv3(model=init_synthetic(build_float_inceptionv3(), seed))
    ref_live.apply_bit_config(q, get_bit_config("inceptionv3", scheme))
    q.eval()
    return q


LIVE2 = dict(model_seed=1, calib=(2, 3), images=(3, 11))   # (batch, image seed)


def net_fixture(scheme, model_seed=0, calib=(BATCH, 0), images=(BATCH, 0), trace=None):
    """one live run: calibrate on `calib`, freeze, evaluate `images`; `trace` (a dict) receives the per-QuantAct and per-conv
    digests of the evaluated forward"""
    q = reference_model(scheme, model_seed)
    x_cal = synthetic_images(calib[0], seed=calib[1], size=299)
    x = synthetic_images(images[0], seed=images[1], size=299)
    out = {"input_sha": np.array(sha(x.numpy())), "torch_version": np.array(torch.__version__)}
    h = hashlib.sha256()
    for p in q.state_dict().values():
        h.update(np.ascontiguousarray(p.numpy()).tobytes())
    out["weights_sha"] = np.array(h.hexdigest())
    ref_live.calibrate_and_freeze(q, x_cal)
    units = [(n, m) for n, m in q.named_modules() if n.count(".") == 2 and n.startswith("features.stage")]
    got, act_out = {}, {}
    hooks = [m.register_forward_hook(lambda mod, i, o, n=n: got.__setitem__(n, o)) for n, m in units]
    if trace is not None:
        hooks += [m.register_forward_hook(lambda mod, i, o, n=n: act_out.__setitem__(
            n, np.rint((o[0] / o[1].reshape(-1)[0]).numpy().astype(np.float64)).astype(np.int64)))
            for n, m in q.named_modules() if type(m).__name__ == "QuantAct"]
        y, conv_taps, lin_taps = ref_live.forward_with_taps(q, x)
    else:
        with torch.no_grad():
            y = q(x)
    for hk in hooks:
        hk.remove()
    if trace is not None:
        conv_names = [n for n, m in q.named_modules() if type(m).__name__ == "QuantBnConv2d"]
        assert len(conv_taps) == len(conv_names) and len(lin_taps) == 1   # call order == registration order in this graph
        trace.update(act_names=np.array(list(act_out)), act_outdigest=np.stack([digest(v) for v in act_out.values()]),
                     act_outmax=np.array([int(np.abs(v).max()) for v in act_out.values()], np.int64),
                     conv_names=np.array(conv_names),
                     conv_accdigest=np.stack([digest(np.rint(t.numpy().astype(np.float64)).astype(np.int64)) for t in conv_taps]),
                     fc_acc=np.rint(lin_taps[0].numpy().astype(np.float64)).astype(np.int64),
                     logits=y.numpy(), input_sha=out["input_sha"])
        assert [str(n) for n in trace["act_names"]] == [n for n, m in q.named_modules() if type(m).__name__ == "QuantAct"]
    out["logits"] = y.numpy()
    out["top1"] = y.argmax(1).numpy()
    out["unit_names"] = np.array([n for n, _ in units])
    out["unit_digest"] = np.stack([digest(np.rint((got[n][0] / got[n][1]).numpy().astype(np.float64))) for n, _ in units])

    acts = [(n, m) for n, m in q.named_modules() if type(m).__name__ == "QuantAct"]
    out["act_names"] = np.array([n for n, _ in acts])
    out["act_x_min"] = np.array([m.x_min.item() for _, m in acts], np.float32)
    out["act_x_max"] = np.array([m.x_max.item() for _, m in acts], np.float32)
    out["act_scale"] = np.array([m.act_scaling_factor.item() for _, m in acts], np.float32)
    convs = [(n, m) for n, m in q.named_modules() if type(m).__name__ == "QuantBnConv2d"]
    out["conv_names"] = np.array([n for n, _ in convs])
    scales, biases, wsha, patches = [], [], [], []
    for li, (n, m) in enumerate(convs):
        scales.append(m.convbn_scaling_factor.numpy())
        biases.append(m.bias_integer.numpy().astype(np.int64))
        wi = m.weight_integer.numpy()
        wsha.append(sha(wi.astype(np.int8)))
        c, b = m.conv, m.bn
        w_f, _ = fold_bn(c.weight, b.weight, b.bias, b.running_mean, b.running_var, b.eps, c.bias)
        w_ieee = quantize_weight_per_channel(w_f, m.weight_bit, m.per_channel, m.weight_percentile)[0].numpy()
        for idx in np.argwhere(wi.reshape(-1) != w_ieee.reshape(-1)).reshape(-1):
            patches.append((li, int(idx), int(wi.reshape(-1)[idx])))
    out["conv_scale"] = np.concatenate(scales).astype(np.float32)
    out["conv_bias"] = np.concatenate(biases)
    out["conv_wsha"] = np.array(wsha)
    out["conv_wpatch"] = np.array(patches, np.int64).reshape(-1, 3)
    fc = q.output.q_fc
    out["fc_scale"] = fc.fc_scaling_factor.numpy()
    out["fc_bias"] = fc.bias_integer.numpy().astype(np.int64)
    out["fc_wsha"] = np.array(sha(fc.weight_integer.numpy().astype(np.int8)))
    return out, q


def extra():
    """the trace of the recorded batch-2 runs and the second live record; the batch-2 files are read, never written"""
    for scheme in ("uniform8", "uniform4"):
        tr = {}
        out, _ = net_fixture(scheme, trace=tr)
        with np.load(os.path.join(HERE, f"net_inceptionv3_{scheme}_b2.npz")) as old:
            assert np.array_equal(old["logits"], out["logits"]) and np.array_equal(old["unit_digest"], out["unit_digest"])
            assert np.array_equal(old["act_x_min"], out["act_x_min"]) and str(old["input_sha"]) == str(out["input_sha"])
        path = os.path.join(HERE, f"net_inceptionv3_{scheme}_b2_trace.npz")
        np.savez_compressed(path, **tr)
        print(path, os.path.getsize(path), "bytes", flush=True)
        tr = {}
        out, _ = net_fixture(scheme, trace=tr, **LIVE2)
        out.update({k: v for k, v in tr.items() if k not in out})
        out.update(model_seed=np.array(LIVE2["model_seed"]), calib=np.array(LIVE2["calib"]), images=np.array(LIVE2["images"]))
        path = os.path.join(HERE, f"net_inceptionv3_{scheme}_b3_live2.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes; top1", out["top1"].tolist(), "patches", len(out["conv_wpatch"]), flush=True)


def main():
    names = None
    for scheme in ("uniform8", "uniform4"):
        out, q = net_fixture(scheme)
        path = os.path.join(HERE, f"net_inceptionv3_{scheme}_b2.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes; top1", out["top1"].tolist(), "patches", len(out["conv_wpatch"]))
        if names is None:
            ref_live.load_reference()
            ref_bit_config = importlib.import_module("bit_config").bit_config_dict
            names = {"state_dict_keys": list(q.state_dict().keys()),
                     "named_modules": [n for n, _ in q.named_modules()],
                     "schedule_names": list(ref_bit_config["bit_config_inceptionv3_uniform8"].keys())}
    with open(os.path.join(HERE, "inceptionv3_names.json"), "w") as f:
        json.dump(names, f, indent=0)


if __name__ == "__main__":
    sys.path.insert(0, ref_live.REF_ROOT)
    main() if "--base" in sys.argv else extra()
