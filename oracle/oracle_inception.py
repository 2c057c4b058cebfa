"""TEST INFRASTRUCTURE ONLY - CPU restatement of the reference's frozen Q_InceptionV3 forward
(utils/models/q_inceptionv3.py:51-57 Q_InceptConv, 102-120 Q_Concurrent, 135-138 / 170-176 / 203-206 / 253-257 / 316-324 the
branches, 373-376 a unit, 575-649 the stem, 740-744 the network; quant_modules.py:205-305 QuantAct, 389-494 QuantBnConv2d,
522-529 QuantMaxPool2d, 585-602 QuantAveragePool2d, 79-130 QuantLinear; quant_utils.py:344-413 fixedpoint_fn case 0).
Never imported by hawq_amd/ or bench.py: tests and the fixture generators under tests/golden/ only.

Built on the primitives of oracle/oracle.py (exact integer convs in C, dyadic round-half-even, batch_frexp) in the reference's
own NCHW / OIHW layouts.  From hawq_amd it takes structure only (skeleton.inception_units / inception_unit_branches): no
quant_utils, quant_modules, engine_inception or _lib - no table builder, clamp range, scale rule or kernel is shared with the
HIP path this file checks.

What is restated:
  * Q_InceptConv: conv + BN fold on integers -> ReLU -> QuantAct case 0 (per-channel dyadic requant, clamp);
  * a branch's q_input_act / q_pool_act / q_concat_activ: case 0 with the weight scale buffer of ones (quant_modules.py:289-293);
  * the LIST path of QuantAct (quant_modules.py:275-286) - a unit's q_rescaling_activ and Inception-C's inner one: each channel
    slice goes from its branch's scale to the QuantAct's own, weight scale S_b / S_b = 1;
  * QuantMaxPool2d(3, 2, 0) on the (monotone) fp32 image of the integers = the max of the integers;
  * QuantAveragePool2d(3, 1, 1) and (8, 1) as the reference evaluates them, in binary32: AvgPool2d of the integers with the
    padding counted, + 0.01, trunc (oracle.avgpool_f32_trunc) - NOT the kernels' (100 s + d) / (100 d) integer rule;
  * QuantLinear: fp32 logits = fl(acc + bias) * fl(S_w * S_a);
  * the input QuantAct on fp32 data, and on uint8 images after the data pipeline's float32 ToTensor + Normalize
    (quant_train.py:432-440), written out below without a look-up table.

PINNED: tests/test_oracle_inception_vs_golden.py runs this file on the live reference's fixtures
(tests/golden/net_inceptionv3_*.npz, written by tests/golden/make_inception_golden.py from the UNMODIFIED reference).
"""
from __future__ import annotations

import numpy as np

from hawq_amd.skeleton import inception_unit_branches, inception_units

from . import oracle as O

f32 = np.float32
FC = "output.q_fc"
STEM = "features.q_init_block"
_STEM_SEQ = ("q_conv1", "q_conv2", "q_conv3", "q_pool1", "q_conv4", "q_conv5", "q_pool2")


# ----------------------------------------------------------------------------------------------------------------- state
def extract_float_state(q, ckpt=None):
    """float conv / BN / fc parameters, bit widths, quant modes and frozen x_min / x_max of a Q_InceptionV3 (the reference's or
    hawq_amd's: same attribute names); no integers are taken from the model.  ``ckpt`` - {module name: dict(scale, bias, wpatch)}
    for QuantBnConv2d names and ``output.q_fc`` - is kept in the state and substituted by forward_int for this file's own IEEE
    preparation: how a reference run's integer buffers (a fixture's scales, biases and patched weights) get in."""
    np_ = O._to_np

    def a(m, name):
        return dict(name=name, bits=int(m.activation_bit), mode=str(m.quant_mode), x_min=np_(m.x_min).astype(f32).reshape(-1)[:1],
                    x_max=np_(m.x_max).astype(f32).reshape(-1)[:1])

    def ic(m, name):
        c, b = m.q_convbn.conv, m.q_convbn.bn
        assert c.groups == 1 and tuple(c.dilation) == (1, 1) and c.stride[0] == c.stride[1] and c.bias is None
        return dict(name=name + ".q_convbn", bits=int(m.q_convbn.weight_bit), w=np_(c.weight), gamma=np_(b.weight), beta=np_(b.bias),
                    mean=np_(b.running_mean), var=np_(b.running_var), eps=float(b.eps), stride=int(c.stride[0]),
                    pad=(int(c.padding[0]), int(c.padding[1])), act=a(m.q_activ, name + ".q_activ"))

    ib = q.features.q_init_block
    st = dict(input=a(ib.q_input_activ, STEM + ".q_input_activ"),
              stem={n: ic(getattr(ib, n), f"{STEM}.{n}") for n in _STEM_SEQ if n.startswith("q_conv")}, units=[], ckpt=ckpt)
    for si, ui, kind, _cin, cout, mid in inception_units():
        un = f"features.stage{si}.unit{ui}"
        unit = getattr(getattr(q.features, f"stage{si}"), f"unit{ui}")
        brs = []
        for bi, spec in enumerate(inception_unit_branches(kind, cout, mid)):
            bn = f"{un}.branches.branch{bi + 1}"
            br = getattr(unit.branches, f"branch{bi + 1}")
            d = dict(kind=spec[0], name=bn, q_input_act=a(br.q_input_act, bn + ".q_input_act"), convs=[])
            if spec[0] in ("conv1x1", "avgpool"):
                d["convs"].append(ic(br.q_conv, bn + ".q_conv"))
            if spec[0] == "avgpool":
                d["q_pool_act"] = a(br.q_pool_act, bn + ".q_pool_act")
            if spec[0] in ("seq", "seq3x3"):
                d["convs"] = [ic(getattr(br.q_conv_list, f"q_conv{i + 1}"), f"{bn}.q_conv_list.q_conv{i + 1}") for i in range(len(spec[1]))]
            if spec[0] == "seq3x3":
                d["q_conv1x3"], d["q_conv3x1"] = ic(br.q_conv1x3, bn + ".q_conv1x3"), ic(br.q_conv3x1, bn + ".q_conv3x1")
                d["q_rescaling_activ"] = a(br.q_rescaling_activ, bn + ".q_rescaling_activ")
            brs.append(d)
        st["units"].append(dict(name=un, branches=brs, q_rescaling_activ=a(unit.q_rescaling_activ, un + ".q_rescaling_activ")))
    st["q_concat_activ"] = a(q.features.q_concat_activ, "features.q_concat_activ")
    fc = q.output.q_fc
    st["fc"] = dict(bits=int(fc.weight_bit), w=np_(fc.weight), b=np_(fc.bias))
    return st


def acts_of(st):
    """every QuantAct record of the state, in the reference's registration (named_modules) order"""
    out = [st["input"]] + [st["stem"][n]["act"] for n in _STEM_SEQ if n in st["stem"]]
    for u in st["units"]:
        for b in u["branches"]:
            out.append(b["q_input_act"])
            if "q_pool_act" in b:
                out.append(b["q_pool_act"])
            out += [c["act"] for c in b["convs"]]
            if b["kind"] == "seq3x3":
                out += [b["q_conv1x3"]["act"], b["q_conv3x1"]["act"], b["q_rescaling_activ"]]
        out.append(u["q_rescaling_activ"])
    return out + [st["q_concat_activ"]]


def convs_of(st):
    """every conv record, in registration order"""
    out = [st["stem"][n] for n in _STEM_SEQ if n in st["stem"]]
    for u in st["units"]:
        for b in u["branches"]:
            out += b["convs"]
            if b["kind"] == "seq3x3":
                out += [b["q_conv1x3"], b["q_conv3x1"]]
    return out


def normalize_uint8(x_u8, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
    """uint8 NHWC [N,H,W,3] -> fp32 NCHW, the data pipeline's own binary32 steps (quant_train.py:432-440): torchvision ToTensor
    ``u.float().div(255)``, Normalize ``sub(mean).div(std)`` with mean / std as binary32."""
    u = np.ascontiguousarray(x_u8)
    assert u.dtype == np.uint8 and u.ndim == 4 and u.shape[3] == 3
    t = (u.astype(f32) / f32(255)).astype(f32)
    t = ((t - np.asarray(mean, f32).reshape(1, 1, 1, 3)).astype(f32) / np.asarray(std, f32).reshape(1, 1, 1, 3)).astype(f32)
    return np.ascontiguousarray(t.transpose(0, 3, 1, 2))


def forward_uint8(st, x_u8, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), ckpt=None):
    """the uint8 entry: host float32 ToTensor + Normalize, then the frozen forward (whose first step is the input QuantAct)"""
    return forward_int(st, normalize_uint8(x_u8, mean, std), ckpt=ckpt)


# --------------------------------------------------------------------------------------------------------------- forward
def forward_int(st, x, calibrate: bool = False, ckpt=None):
    """integer forward of a frozen Q_InceptionV3: (logits fp32 [N, 1000], Trace keyed by the reference's module names):
    ``<QuantBnConv2d>.acc`` int64 accumulator + bias (NCHW), ``<QuantAct>.q`` every QuantAct's integer output (a unit's output
    after its q_rescaling_activ is ``<unit>.q_rescaling_activ.q``), ``output.q_fc.acc``, ``logits``.  With ``calibrate`` every
    QuantAct range is (re)initialised from this batch exactly as ONE un-frozen reference forward does (quant_modules.py:233-250)
    and written back into ``st``; ``st['ranges']`` then lists (name, x_min, x_max)."""
    tr = O.Trace()
    ckpt = ckpt if ckpt is not None else st.get("ckpt")
    one = np.ones(1, f32)
    relu = lambda v: np.maximum(v, 0)
    f_of = lambda r, s: (r.astype(f32) * f32(s[0])).astype(f32)      # the fp32 tensor integers r at scale s stand for

    def sc(a, xf):
        """scale of QuantAct `a`; `xf()` is the fp32 tensor it is given (evaluated when calibrating only)"""
        if calibrate:
            t = xf()
            a["x_min"], a["x_max"] = np.asarray([t.min()], f32), np.asarray([t.max()], f32)
        return O.act_scale(a["x_min"], a["x_max"], a["bits"], a["mode"])

    def requant(a, r, s_prev):
        """QuantAct case 0 on integers r at scale s_prev with the weight scale buffer of ones"""
        s = sc(a, lambda: f_of(r, s_prev))
        m, e = O.requant_table(s_prev, one, s)
        qv = O.dyadic(r, m, e, O.act_range(a["bits"], a["mode"]))
        tr[a["name"] + ".q"] = qv
        return qv, s

    def concat_requant(a, parts):
        """the list path (quant_modules.py:275-286): parts = [(integers, scale)] -> the concat at a's own scale"""
        s = sc(a, lambda: np.concatenate([f_of(r, sb) for r, sb in parts], 1))
        rng, outs = O.act_range(a["bits"], a["mode"]), []
        for r, sb in parts:
            m, e = O.requant_table(sb, (sb / sb).astype(f32), s)
            outs.append(O.dyadic(r, m, e, rng))
        qv = np.concatenate(outs, 1)
        tr[a["name"] + ".q"] = qv
        return qv, s

    def conv(ic, q_in, s_a):
        """Q_InceptConv (q_inceptionv3.py:51-57): QuantBnConv2d on integers -> ReLU -> QuantAct case 0"""
        n = ic["name"]
        w_f, b_f = O.fold_bn(ic["w"], ic["gamma"], ic["beta"], ic["mean"], ic["var"], ic["eps"])
        w_int, s_w = O.quantize_weight(w_f, ic["bits"])
        b_int, bs = O.quantize_bias(b_f, s_w, s_a)
        if ckpt is not None and n in ckpt:
            ov = ckpt[n]
            s_w = np.asarray(ov["scale"], f32)
            bs = (s_w * f32(np.asarray(s_a, f32).reshape(-1)[0])).astype(f32)
            b_int = np.asarray(ov["bias"], np.int64)
            w_int = w_int.copy()
            for idx, val in ov.get("wpatch", ()):
                w_int.reshape(-1)[idx] = val
        acc = O.conv2d_rect(q_in, w_int, b_int, ic["stride"], ic["pad"][0], ic["pad"][1])
        tr[n + ".weight_integer"], tr[n + ".bias_integer"], tr[n + ".convbn_scaling_factor"], tr[n + ".acc"] = w_int, b_int, s_w, acc
        a = ic["act"]
        z = relu(acc)
        s_o = sc(a, lambda: (z.astype(f32) * bs.reshape(1, -1, 1, 1)).astype(f32))   # quant_modules.py:491-494, then nn.ReLU
        m, e = O.requant_table(s_a, s_w, s_o)
        qv = O.dyadic(z, m, e, O.act_range(a["bits"], a["mode"]))
        tr[a["name"] + ".q"] = qv
        return qv, s_o

    # stem (q_inceptionv3.py:575-649): the input QuantAct on fp32 data (quant_modules.py:271-274)
    x = np.ascontiguousarray(x, f32)
    a = st["input"]
    s = sc(a, lambda: x)
    r = O.quantize_f32(x, s[0], a["bits"], a["mode"])
    tr[a["name"] + ".q"] = r
    for n in _STEM_SEQ:
        if n.startswith("q_pool"):
            r = O.maxpool(r, 3, 2, 0)
        else:
            r, s = conv(st["stem"][n], r, s)

    for u in st["units"]:
        parts = []
        for b in u["branches"]:
            qb, sb = requant(b["q_input_act"], r, s)
            if b["kind"] == "maxpool":
                qb = O.maxpool(qb, 3, 2, 0)
            else:
                if b["kind"] == "avgpool":
                    qb = O.avgpool_f32_trunc(qb, 3, 1)
                    tr[b["name"] + ".q_pool.q"] = qb
                    qb, sb = requant(b["q_pool_act"], qb, sb)
                for ic in b["convs"]:
                    qb, sb = conv(ic, qb, sb)
                if b["kind"] == "seq3x3":
                    qb, sb = concat_requant(b["q_rescaling_activ"], [conv(b["q_conv1x3"], qb, sb), conv(b["q_conv3x1"], qb, sb)])
            parts.append((qb, sb))
        r, s = concat_requant(u["q_rescaling_activ"], parts)

    pooled = O.avgpool_f32_trunc(r, 8, 0)
    tr["features.q_final_pool.q"] = pooled
    qf, s_c = requant(st["q_concat_activ"], pooled, s)
    qf = qf.reshape(qf.shape[0], -1)
    fc = st["fc"]
    w_int, s_fc = O.quantize_weight(fc["w"], fc["bits"])
    b_int, bs = O.quantize_bias(fc["b"], s_fc, s_c)
    if ckpt is not None and FC in ckpt:
        s_fc = np.asarray(ckpt[FC]["scale"], f32)
        bs = (s_fc * f32(s_c[0])).astype(f32)
        b_int = np.asarray(ckpt[FC]["bias"], np.int64)
    acc = O.linear(qf, w_int, b_int)
    tr[FC + ".weight_integer"], tr[FC + ".bias_integer"], tr[FC + ".fc_scaling_factor"], tr[FC + ".acc"] = w_int, b_int, s_fc, acc
    logits = (acc.astype(f32) * bs.reshape(1, -1)).astype(f32)   # quant_modules.py:127-130
    tr["logits"] = logits
    if calibrate:
        st["ranges"] = [(a["name"], a["x_min"].copy(), a["x_max"].copy()) for a in acts_of(st)]
    return logits, tr


def unit_names(st):
    return [u["name"] for u in st["units"]]


def unit_output(tr, name):
    """a unit's integer output after its q_rescaling_activ (int64 NCHW)"""
    return tr[name + ".q_rescaling_activ.q"]
