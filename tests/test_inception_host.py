"""InceptionV3 host-side pieces (no GPU): schedules, skeleton, quantized graph names, the integer average-pool rule."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = os.path.join(ROOT, "tests", "golden", "inceptionv3_names.json")
REF_BIT_CONFIG = "/root/reference/bit_config.py"


def _recorded():
    with open(NAMES) as f:
        return json.load(f)


@pytest.mark.parametrize("scheme", ["uniform8", "uniform4"])
def test_schedule_names_equal_the_reference(scheme):
    from hawq_amd.bit_schedules import get_bit_config, inceptionv3_module_names
    cfg = get_bit_config("inceptionv3", scheme)
    assert list(cfg) == inceptionv3_module_names() == _recorded()["schedule_names"]
    assert len(cfg) == 257
    if os.path.isfile(REF_BIT_CONFIG):   # the reference's own dict, when its tree is around
        spec = importlib.util.spec_from_file_location("ref_bit_config", REF_BIT_CONFIG)
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        ref = m.bit_config_dict[f"bit_config_inceptionv3_{scheme}"]
        assert list(ref) == list(cfg)
        assert {k: (v[0] if isinstance(v, tuple) else v) for k, v in ref.items()} == cfg


def test_schedule_widths_follow_the_dataflow():
    """Unit outputs and branch ends are 16 bit, every conv input at most 8 bit, pool-branch inputs 16 bit."""
    from hawq_amd.bit_schedules import get_bit_config
    for scheme, conv_in in (("uniform8", 8), ("uniform4", 4)):
        cfg = get_bit_config("inceptionv3", scheme)
        for name, bits in cfg.items():
            if name.endswith("q_rescaling_activ"):
                assert bits == 16, name
            elif name.endswith("q_input_act"):
                assert bits in (16, conv_in), name
        assert cfg["features.q_init_block.q_conv5.q_activ"] == 16


def test_skeleton_covers_every_schedule_entry_and_state_dict_matches_the_reference():
    from hawq_amd.api import build_quantized_resnet
    from hawq_amd.q_inceptionv3 import Q_InceptionV3
    from hawq_amd.quant_modules import QuantAct
    rec = _recorded()
    for scheme in ("uniform8", "uniform4"):
        q = build_quantized_resnet("inceptionv3", scheme, seed=None)
        assert isinstance(q, Q_InceptionV3)
        mods = dict(q.named_modules())
        assert list(mods) == rec["named_modules"]
        assert list(q.state_dict()) == rec["state_dict_keys"]
        for name in rec["schedule_names"]:
            assert name in mods, name
        acts4 = [n for n, m in mods.items() if isinstance(m, QuantAct) and m.activation_bit == 4]
        assert all(mods[n].quant_mode == "asymmetric" for n in acts4)
        assert bool(acts4) == (scheme == "uniform4")


def test_skeleton_shapes_and_multiply_accumulates():
    """Float skeleton: 299 x 299 -> 8 x 8 x 2048 (torch on the CPU), and the MAC count of the roofline (about 5.7 G per image)."""
    from hawq_amd.skeleton import build_float_inceptionv3
    net = build_float_inceptionv3()
    macs = [0]

    def hook(mod, inp, out):
        macs[0] += out.numel() * mod.weight[0].numel()

    hooks = [m.register_forward_hook(hook) for m in net.modules() if isinstance(m, torch.nn.Conv2d)]
    f = net.features
    with torch.no_grad():
        x = torch.zeros(1, 3, 299, 299)
        ib = f.init_block
        for m in (ib.conv1, ib.conv2, ib.conv3, ib.pool1, ib.conv4, ib.conv5, ib.pool2):
            x = m.conv(x) if hasattr(m, "conv") else m(x)
        assert x.shape == (1, 192, 35, 35)
        for s in (1, 2, 3):
            stage = getattr(f, f"stage{s}")
            u = 1
            while hasattr(stage, f"unit{u}"):
                outs = []
                for b in getattr(stage, f"unit{u}").branches.children():
                    y = x
                    if hasattr(b, "pool"):
                        y = b.pool(y)
                    if hasattr(b, "conv"):
                        y = b.conv.conv(y)
                    if hasattr(b, "conv_list"):
                        for c in b.conv_list.children():
                            y = c.conv(y)
                    if hasattr(b, "conv1x3"):
                        y = torch.cat((b.conv1x3.conv(y), b.conv3x1.conv(y)), 1)
                    outs.append(y)
                x = torch.cat(outs, 1)
                u += 1
    for h in hooks:
        h.remove()
    assert x.shape == (1, 2048, 8, 8)
    macs[0] += 2048 * 1000
    assert 5.6e9 < macs[0] < 5.8e9, macs[0]


@pytest.mark.parametrize("divisor", [9, 64])
def test_integer_average_rule_equals_trunc_over_all_16bit_sums(divisor):
    """QuantAveragePool2d (quant_modules.py:596-602): trunc(AvgPool(x_int) + 0.01) in float32, against the integer rule of the
    kernels, (100 s + d) / (100 d) with C division (truncation toward zero), for EVERY sum s of d signed 16-bit values."""
    lim = divisor * 32768
    s = np.arange(-lim, lim + 1, dtype=np.int64)
    num = 100 * s + divisor
    rule = np.where(num >= 0, num // (100 * divisor), -((-num) // (100 * divisor)))
    f = torch.from_numpy(s.astype(np.float32))
    assert np.array_equal(torch.trunc(f / divisor + 0.01).numpy().astype(np.int64), rule)
    # and through nn.AvgPool2d itself: one window per sum, the sum spread over the window's taps
    k = 3 if divisor == 9 else 8
    sel = s[::7] if divisor == 9 else s[::97]
    base = np.trunc(sel / divisor).astype(np.int64)   # every tap gets base, the first tap the rest: taps stay within 16 bits
    taps = np.repeat(base[:, None], divisor, 1)
    taps[:, 0] += sel - base * divisor
    assert np.abs(taps).max() <= 32768 + divisor
    x = torch.from_numpy(taps.astype(np.float32).reshape(1, -1, k, k))
    pool = torch.nn.AvgPool2d(k, 1, padding=1 if k == 3 else 0)
    y = pool(x)[0, :, 1, 1] if k == 3 else pool(x)[0, :, 0, 0]
    num = 100 * sel + divisor
    rule = np.where(num >= 0, num // (100 * divisor), -((-num) // (100 * divisor)))
    assert np.array_equal(torch.trunc(y + 0.01).numpy().astype(np.int64), rule)


def test_validate_uint8_is_refused_for_inceptionv3():
    from hawq_amd.api import build_quantized_resnet, validate
    q = build_quantized_resnet("inceptionv3", "uniform8", seed=None)
    with pytest.raises(NotImplementedError):
        validate(q, [(torch.zeros(1, 299, 299, 3, dtype=torch.uint8), torch.zeros(1, dtype=torch.long))], uint8=True,
                 device="cpu")


def test_cpu_input_raises():
    from hawq_amd.api import build_quantized_resnet
    q = build_quantized_resnet("inceptionv3", "uniform8", seed=None)
    with pytest.raises(RuntimeError):
        q(torch.zeros(1, 3, 299, 299))
