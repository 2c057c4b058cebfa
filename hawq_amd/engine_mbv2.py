"""Fused integer executor for a frozen Q_MobileNetV2 on one MI355X.

The module path of ``hawq_amd.q_mobilenetv2`` moves fp32 NCHW ``integer x scale`` tensors between kernels like the reference
does.  This plan keeps integers: int8 NHWC activations between the convs of a unit, int32 NHWC for the 16-bit values that
flow between units and are read again (MobileNetV2's units end WITHOUT an activation, so those values are signed - the uint16
residual format of the ResNet plan does not apply), three launches per unit, one hipGraph per batch shape:

    input QuantAct -> init_block 3x3/2 (+ReLU6 + quant_act_int32 + unit 1's block-input QuantAct)
    per unit:  conv1 1x1 (+ReLU6 + quant_act1) -> conv2 depthwise 3x3 (+ReLU6 + quant_act2)
               -> conv3 1x1 (+ quant_act_int32 with / without the identity branch + next block-input QuantAct)
    final_block 1x1 (+ReLU6 + quant_act_int32_final) -> avg-pool (+quant_act_output) -> classifier (+dequant)

Integer semantics (reference: q_mobilenetv2.py:60-93, 176-209; quant_utils.py:363-456), each rounding point kept:
  * every QuantAct without identity is fixedpoint_fn case 0: ``clamp(RNE(acc * m / 2^e))`` - including the 16-bit
    ``quant_act_int32`` of units that change shape, which therefore CLAMPS to [-32768, 32767] (hawq_conv_args.res_clamp16);
    with an identity it is case 1: both branches requantised separately, summed, NOT clamped, and - unlike the ResNets - no
    ReLU follows (hawq_conv_args.res_no_relu);
  * ReLU6 sits between a conv and its QuantAct on the fp32 value.  In integers it is ReLU plus the QuantAct's own upper
    clamp: the QuantAct's calibrated range cannot exceed 6, so ``RNE(round(6 / S_a / S_w[c]) * m / 2^e) >= q_hi`` and the clamp
    at ``q_hi`` decides first.  ``_relu6_is_relu`` checks exactly that inequality per channel on the host and refuses the
    plan otherwise;
  * weights and tables are padded to multiples of 64 channels with zero weights, zero bias and ``m = 0`` tables; tensors are stored at
    the next multiple of 16 channels, their padding channels carry exact zeros;
  * the classifier is a QuantConv2d whose reference forward runs an fp32 conv on the UN-rounded ``x / S_a``
    (quant_modules.py:727-736): its logits carry float noise of the order of an ulp.  This plan returns
    ``float(acc) * fl(S_w[c] * S_a)``: identical int32 accumulators, logits within 2 ulp (tests/test_gpu_network.py).

Round 4 (97 k -> 209 k img/s at batch 128):
  * a unit whose three layers' requant tables the host proves for the fast contract and whose block input / output are at most 96
    channels wide (or, on the 7 x 7 maps, 160) is ONE launch (``hawq_linear_bottleneck``: the hidden tensors stay in LDS) - 16 of the
    17 units of the width-1 network; the init block is one launch too (``hawq_stem3x3s2``, fp32 or uint8 images);
  * the remaining units run three launches on tensors stored at their own width (``hawq_conv_args.in_pitch / out_pitch``, ABI 4),
    their closing convs with the fast contract's arithmetic on the direct epilogue where every table of the launch is proved
    (otherwise the exact general epilogue: any e, ties handled; ``n_valid`` skips the padding channels); the expansion convs run the
    fast REQUANT epilogue, the depthwise layers ``hawq_depthwise3x3_requant``;
  * tapped plans (``keep_accumulators``) always run the round-3 launch list - the taps ARE the intermediate tensors.
Every ``hawq_conv2d`` launch is tile-tuned by timing, and the batch runs as one or two concurrent sub-batch chains inside the one
hipGraph, whichever replays faster (graph, chains, entry points and event timing: hawq_amd/runner.py).
Switches (results never change): HAWQ_MBV2_UNFUSED=1 three launches per unit and the im2col init
block; HAWQ_MBV2_UNIT_TILE=1..4 organisation of the unit launch (``hawq_bottleneck_args.tile``); HAWQ_MBV2_EXACT=1 exact closing
epilogues; HAWQ_MBV2_PAD64=1 round 3's 64-padded tensors; HAWQ_MBV2_CHAINS, HAWQ_MBV2_TILES.
"""
from __future__ import annotations

import ctypes as C
import os
from functools import partial

import numpy as np
import torch

from . import _lib, packing
from .quant_modules import QuantBnConv2d
from .quant_utils import input_quant_lut, quantize_weight_per_channel, requant_table, tables_are_fast, tables_fit_fast
from .runner import EventTimer, GraphRunner, _i32, _rng, two_round_min


def _pad64(c: int) -> int:
    return (c + 63) // 64 * 64


def _pitch(c: int) -> int:
    """Channels per STORED pixel row of a c-channel tensor (round 4): the next multiple of 16, not of 64 - MobileNetV2's 16 / 24 / 32 /
    96 / 144 / 160-channel tensors are stored (almost) at their own width.  The GEMMs still see K and N padded to the 64-channel tile:
    a conv reads its K = pad64(c) bytes per pixel through `hawq_conv_args.in_pitch` (the bytes beyond the row meet zero weights) and
    writes only the first `out_pitch` channels of its 64-channel tiles (include/hawq_mi355.h, ABI 4).  HAWQ_MBV2_PAD64=1 restores the
    64-padded tensors of round 3 (A/B switch for measurements)."""
    return _pad64(c) if os.environ.get("HAWQ_MBV2_PAD64") else (c + 15) // 16 * 16


def _padded(v, n, fill=0):
    out = np.full(n, fill, np.int64)
    out[:len(v)] = v
    return out


class PlanNotApplicable(NotImplementedError):
    """The network is a configuration the fused integer plan does not take (Q_MobileNetV2.forward falls back to the module-by-module
    path on exactly this exception; anything else - a launch error, a missing library - propagates)."""


def _requant_bound(vmax, m, ek):
    """Upper bound on |RNE(v * m / 2^e)| for |v| <= vmax (per-channel arrays or scalars; unlifted or lifted tables alike)."""
    m = np.asarray(m, np.int64).reshape(-1)
    ek = np.asarray(ek, np.int64).reshape(-1)
    vmax = np.broadcast_to(np.asarray(vmax, dtype=object), m.shape)
    return max(((int(v) << int(k)) * int(mm) >> int(e)) + 1 for v, mm, e, k in zip(vmax, m, ek & 0xff, ek >> 8))


def _fast_scalar(s_in, s_out, vmax):
    """Scalar requant table lifted to the fast contract for inputs |v| <= vmax: (m, ek, tie) or None when it does not fit."""
    if vmax is None:   # no bound on the producer's output is known: the exact 64-bit arithmetic runs
        return None
    try:
        m, ek = requant_table(s_in, torch.ones(1), s_out, vbits=int(vmax).bit_length())
    except ValueError:
        return None
    vb = int(vmax).bit_length()
    if not tables_fit_fast(m, ek, vb):
        return None
    return int(m[0]), int(ek[0]), not tables_are_fast(m, ek, vb)


class _Layer:
    """Device-resident integer parameters of one QuantBnConv2d, channel-padded."""

    def __init__(self, mod: QuantBnConv2d, s_a, dev, from_buffers, im2col=False):
        if not from_buffers:
            mod.prepare(s_a)
        w = np.rint(mod.weight_integer.detach().cpu().numpy().astype(np.float64)).astype(np.int64)
        self.stride, self.pad, self.groups = int(mod.conv.stride[0]), int(mod.conv.padding[0]), int(mod.conv.groups)
        self.im2col = bool(im2col and w.shape[1:] == (3, 3, 3) and (self.stride, self.pad, self.groups) == (2, 1, 1))
        if self.im2col:   # the input quantiser writes (kh, kw, c) patches (hawq_quantize_im2col3x3s2): a 1x1 conv on K = 27 -> 64
            w = np.ascontiguousarray(w.transpose(0, 2, 3, 1)).reshape(w.shape[0], 27, 1, 1)
            self.stride, self.pad = 1, 0
        self.cout, cg, self.kh, self.kw = w.shape
        self.cin = cg * self.groups
        self.cin_p, self.cout_p = _pad64(self.cin), _pad64(self.cout)
        # stored width of the input / output tensor (the im2col rows of the init conv are 64 bytes by construction)
        self.cin_s, self.cout_s = (self.cin_p if im2col else _pitch(self.cin)), _pitch(self.cout)   # (im2col: the init layer, either input form)
        self.s_w = mod.convbn_scaling_factor.detach().float().cpu().reshape(-1)
        b = np.clip(np.rint(mod.bias_integer.detach().cpu().numpy().astype(np.float64)), -2 ** 31, 2 ** 31 - 1).astype(np.int64)
        self.bias = _i32(_padded(b, self.cout_p), dev)
        self.b_host = b
        # exact per-channel bound on |accumulator| -> bit length (8-bit activations), for the requant pre-shift check
        bound = np.abs(w).reshape(self.cout, -1).sum(1) * 128 + np.abs(b)
        self.vbits = np.array([int(v).bit_length() for v in bound], np.int64)
        if (self.vbits > 31).any():
            raise ValueError("int32 accumulator overflow is possible for this layer")
        self.w_host = w
        self.weight_bytes = int(w.size) + 12 * self.cout   # int8 weights + bias / multiplier / exponent
        if self.groups == 1:
            self.w = torch.from_numpy(packing.pack_conv_weight(w, 8, self.cin_p, self.cout_p)).to(dev)
        elif self.groups == self.cin == self.cout and (self.kh, self.kw, self.pad) == (3, 3, 1):
            w9c = np.zeros((9, self.cout_s), np.int8)   # tap-major [3][3][C] with C = the stored width of the tensors it runs on
            w9c[:, :self.cout] = w.reshape(self.cout, 9).T
            self.w = torch.from_numpy(w9c).to(dev)
            w9p = np.zeros((9, self.cout_p), np.int8)   # the one-launch unit reads whole 32-channel slices (hawq_linear_bottleneck)
            w9p[:, :self.cout] = w9c[:, :self.cout]
            self.w9p = torch.from_numpy(w9p).to(dev)
        else:
            raise PlanNotApplicable("grouped convolutions other than depthwise 3x3 are outside MobileNetV2")

    def fast_closing(self, s_a, s_out, dev):
        """Fused constants (packing.pack_ctab, bias folded) of this conv's unit-closing requant when the lifted table fits the fast
        contract: dict(ctab, tie) or None.  Lets the direct RESIDUAL epilogue run 3-instruction requants (hawq_conv2d, ConvP.gfast)."""
        try:
            mm, ee = requant_table(s_a, self.s_w, s_out, vbits=self.vbits)
        except ValueError:
            return None
        if not tables_fit_fast(mm, ee, self.vbits):
            return None
        cp = self.cout_p
        return dict(ctab=_i32(packing.pack_ctab(_padded(self.b_host, cp), _padded(mm, cp), _padded(ee, cp, 33)), dev),
                    tie=not tables_are_fast(mm, ee, self.vbits))

    def table(self, s_a, s_out, dev):
        """(m, e) of QuantAct(conv output): ratio S_a * S_w[c] / S_out, padded channels m = 0"""
        m, e = requant_table(s_a, self.s_w, s_out, lift=False)
        return _i32(_padded(m, self.cout_p), dev), _i32(_padded(e, self.cout_p, 33), dev), m, e


def _relu6_is_relu(s_a, s_w, m, e, q_hi) -> bool:
    """ReLU6 == ReLU + the following QuantAct's clamp, iff the requantised image of fp32 6.0 reaches q_hi in every channel.
    The reference turns a ReLU6-saturated value into z = round(6 / S_a / S_w[c]) (fixedpoint_fn, quant_utils.py:390-392) and
    requantises THAT; this plan requantises the larger accumulator: both land on q_hi iff RNE(z * m / 2^e) >= q_hi (exact
    integers below; every smaller accumulator is below 6.0 in fp32 and takes the same path in both)."""
    s_a32, s_w32 = np.float32(s_a), np.asarray(s_w, np.float32)
    a6 = np.rint((np.float32(6.0) / s_a32 / s_w32).astype(np.float64))
    for a, mv, ev in zip(a6, np.asarray(m, np.int64), np.asarray(e, np.int64) & 0xff):
        a, mv, ev = int(a), int(mv), int(ev)
        t = a * mv + (1 << (ev - 1))
        q = t >> ev
        if t % (1 << ev) == 0 and (q & 1):   # exact tie: round half to even
            q -= 1
        if q < q_hi:
            return False
    return True


class MobileNetV2Engine(GraphRunner):
    """Callable: fp32 NCHW images on the GPU -> fp32 logits of the frozen Q_MobileNetV2 (see the module docstring)."""

    def __init__(self, model, from_buffers=None, use_graph: bool = True, keep_accumulators: bool = False, chains: int = 0):
        """``from_buffers``: run on the modules' integer buffers / stored scales (a network restored by ``load_quantized_checkpoint``)
        instead of re-deriving them from float weights and ranges; None (the default) = whatever the modules themselves are marked as
        (``use_integer_buffers``, set by the loader), and a network whose modules disagree is refused - so that an engine built directly
        on a model restored by ``load_quantized_checkpoint`` cannot silently re-derive scales from placeholder ranges.  An explicit
        False keeps the activation scales re-derived from the modules' ranges (tests load reference ranges that way).
        ``chains``: 1 = one launch chain; 2 = the batch split into two sub-batches whose chains run on two streams inside the
        one hipGraph (tails, prologues and dispatch gaps of one overlap the other's kernels, as in the ResNet engine); 0 = decided
        by timing both at the first call of a batch shape (HAWQ_MBV2_CHAINS overrides)."""
        if not model.is_frozen():
            raise RuntimeError("MobileNetV2Engine needs a frozen model (freeze_model) - ranges must be fixed")
        _lib.load()
        marks = {bool(getattr(m, "use_integer_buffers", False)) for m in model.modules() if hasattr(m, "weight_integer")}
        if from_buffers is None:
            if len(marks) > 1:
                raise RuntimeError("MobileNetV2Engine: some modules run on loaded integer buffers and others do not - reload the checkpoint "
                                   "(load_quantized_checkpoint) or the float weights (load_state_dict) as a whole")
            from_buffers = bool(marks and marks.pop())
        self.model, self.from_buffers, self.use_graph, self.keep_acc = model, from_buffers, use_graph and not keep_accumulators, keep_accumulators
        self.dev = next(model.parameters()).device
        if self.dev.type != 'cuda':
            raise RuntimeError("MobileNetV2Engine: move the model to the MI355X first (no CPU path)")
        self.stream = torch.cuda.Stream(device=self.dev)
        self.flags = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self._batch = self._graph = None
        self.taps, self.subs = {}, []
        self.chains_req = 1 if keep_accumulators else max(0, int(os.environ.get("HAWQ_MBV2_CHAINS", chains)))
        self.chains = max(1, self.chains_req)
        self._prepare()

    def _spawn(self):
        """a chain of this plan: shares the prepared parameters, owns its stream and activation buffers"""
        sub = object.__new__(MobileNetV2Engine)
        sub.model, sub.from_buffers, sub.keep_acc, sub.dev, sub.flags, sub.P = self.model, self.from_buffers, self.keep_acc, self.dev, self.flags, self.P
        sub.use_graph, sub.stream = False, torch.cuda.Stream(device=self.dev)
        sub._batch = sub._graph = None
        sub.taps, sub.subs, sub.chains, sub.chains_req = {}, [], 1, 1
        return sub

    # ------------------------------------------------------------------ host-side preparation
    def _scale(self, act):
        s = act.act_scaling_factor if self.from_buffers else act.compute_scale()
        return s.detach().float().cpu().reshape(-1)[:1]

    def _prepare(self):
        m, dev, one = self.model, self.dev, torch.ones(1)
        P = self.P = {}
        qi = m.quant_input
        if qi.activation_bit != 8 or qi.quant_mode != 'symmetric':
            raise PlanNotApplicable("quant_input must be 8-bit symmetric (every shipped schedule)")
        s_in = self._scale(qi)
        P['s_in'], P['inv_s_in'] = float(s_in.item()), float((1. / s_in).item())

        def act16(act):
            if act.activation_bit != 16 or act.quant_mode != 'symmetric':
                raise PlanNotApplicable("the unit-closing QuantAct must be 16-bit symmetric (every shipped schedule)")
            return self._scale(act)

        def activated(layer, s_a, act):
            """conv -> ReLU6 -> QuantAct(case 0): table + clamp; refuses if ReLU6 is not ReLU + clamp here"""
            s_o = self._scale(act)
            md, ed, mh, eh = layer.table(s_a, s_o, dev)
            lo, hi = _rng(act)
            if not _relu6_is_relu(float(s_a.item()), layer.s_w.numpy(), mh, eh, hi):
                raise PlanNotApplicable("a QuantAct range above 6.0 behind ReLU6: the integer plan folds ReLU6 into the clamp")
            ent = dict(m=md, e=ed, lo=max(lo, 0), hi=hi, s=s_o)
            if layer.groups == 1:
                # the conv kernels' short requant (one v_mad_i64_i32 against a fused per-channel constant) where the lifted table
                # fits its contract; bit 2 keeps exact round-half-even where a tie cannot be excluded on the host
                mm, ee = requant_table(s_a, layer.s_w, s_o, vbits=layer.vbits)
                if tables_fit_fast(mm, ee, layer.vbits):
                    cp = layer.cout_p
                    ent['ctab'] = _i32(packing.pack_ctab(_padded(layer.b_host, cp), _padded(mm, cp), _padded(ee, cp, 33)), dev)
                    ent['m'], ent['e'] = _i32(_padded(mm, cp), dev), _i32(_padded(ee, cp, 33), dev)
                    ent['fast'] = (1 if tables_are_fast(mm, ee, layer.vbits) else 5) | (8 if not (np.asarray(ee) >> 8).any() else 0)   # bit 3: no pre-shifts
            else:
                # depthwise: the same contract for the one-launch unit (hawq_linear_bottleneck); hawq_depthwise3x3_requant keeps (m, e)
                try:
                    mm, ee = requant_table(s_a, layer.s_w, s_o, vbits=layer.vbits)
                    fits = tables_fit_fast(mm, ee, layer.vbits)
                except ValueError:
                    fits = False
                if fits:
                    cp = layer.cout_p
                    ent['dw_ctab'] = _i32(packing.pack_ctab(_padded(layer.b_host, cp), _padded(mm, cp), _padded(ee, cp, 33)), dev)
                    ent['dw_fast'] = (1 if tables_are_fast(mm, ee, layer.vbits) else 5) | (8 if not (np.asarray(ee) >> 8).any() else 0)
            return ent

        # init block: conv -> ReLU6 -> quant_act_int32 (16 bit)
        init = _Layer(m.init_block, s_in, dev, self.from_buffers, im2col=True)
        s16 = act16(m.quant_act_int32)
        md, ed, mh, eh = init.table(s_in, s16, dev)
        if not _relu6_is_relu(float(s_in.item()), init.s_w.numpy(), mh, eh, 32767):
            raise PlanNotApplicable("quant_act_int32 range above 6.0 behind ReLU6")
        P['init'] = dict(layer=init, m=md, e=ed, fast=init.fast_closing(s_in, s16, dev))
        units = []
        s_prev = s16
        ob_prev = 32768   # bound on |16-bit output| of the producer in front of the current unit (init: ReLU + clamp)
        for u in m.units():
            d = dict(residual=bool(u.residual))
            qa = u.quant_act
            s_a = self._scale(qa)
            mq, eq = requant_table(s_prev, one, s_a, lift=False)
            d['mq'], d['eq'], d['q_rng'] = int(mq[0]), int(eq[0]), _rng(qa)
            d['q_fast'] = _fast_scalar(s_prev, s_a, ob_prev)   # the same table lifted for the producer's fast arithmetic
            s_x = s_a
            d['layers'] = []
            for conv, act in u.activated:
                L = _Layer(getattr(u, conv), s_x, dev, self.from_buffers)
                ent = activated(L, s_x, getattr(u, act))
                ent['layer'] = L
                d['layers'].append(ent)
                s_x = ent['s']
            proj = _Layer(u.conv3, s_x, dev, self.from_buffers)
            s_o = act16(u.quant_act_int32)
            md, ed, _, _ = proj.table(s_x, s_o, dev)
            d['proj'] = dict(layer=proj, m=md, e=ed, fast=proj.fast_closing(s_x, s_o, dev))
            _, _, mh3, eh3 = proj.table(s_x, s_o, dev)
            ob = _requant_bound([(1 << int(v)) for v in proj.vbits], mh3, eh3)
            if d['residual']:
                m1, e1 = requant_table(s_prev, one, s_o, lift=False)
                d['m_id'], d['e_id'] = int(m1[0]), int(e1[0])
                d['id_fast'] = _fast_scalar(s_prev, s_o, ob_prev)
                # case 1: the un-clamped sum of the two branches.  A bound that leaves 31 bits is no bound the fast tables may be lifted
                # for: the consumers' q_fast / id_fast stay None (they run the exact arithmetic) instead of trusting a capped figure
                ob = None if ob_prev is None else ob + _requant_bound(ob_prev, m1, e1)
                if ob is not None and ob > (1 << 30):
                    ob = None
            else:
                ob = min(ob, 32768)                          # case 0 clamps to the 16-bit range
            units.append(d)
            s_prev, ob_prev = s_o, ob
        P['units'] = units
        qb = m.quant_act_before_final_block
        s_b = self._scale(qb)
        mq, eq = requant_table(s_prev, one, s_b, lift=False)
        P['before_final'] = dict(mq=int(mq[0]), eq=int(eq[0]), rng=_rng(qb), q_fast=_fast_scalar(s_prev, s_b, ob_prev))
        fin = _Layer(m.features.final_block, s_b, dev, self.from_buffers)
        s_f = act16(m.quant_act_int32_final)
        md, ed, mh, eh = fin.table(s_b, s_f, dev)
        if not _relu6_is_relu(float(s_b.item()), fin.s_w.numpy(), mh, eh, 32767):
            raise PlanNotApplicable("quant_act_int32_final range above 6.0 behind ReLU6")
        P['final'] = dict(layer=fin, m=md, e=ed, fast=fin.fast_closing(s_b, s_f, dev))
        ao = m.quant_act_output
        s8 = self._scale(ao)
        mq, eq = requant_table(s_f, one, s8, lift=False)
        P['out'] = dict(mq=int(mq[0]), eq=int(eq[0]), rng=_rng(ao))
        if _rng(ao)[0] < -128 or _rng(ao)[1] > 127:
            raise PlanNotApplicable("quant_act_output must fit int8")
        oc = m.output
        if oc.bias is not None or tuple(oc.kernel_size) != (1, 1) or oc.groups != 1:
            raise PlanNotApplicable("the classifier must be a bias-free 1x1 QuantConv2d")
        if self.from_buffers or getattr(oc, "use_integer_buffers", False):
            w_int, s_w = oc.weight_integer.detach().float().cpu(), oc.conv_scaling_factor.detach().float().cpu().reshape(-1)
        else:
            w_int, s_w = quantize_weight_per_channel(oc.weight, oc.weight_bit, oc.per_channel, oc.weight_percentile)
            oc.weight_integer, oc.conv_scaling_factor = w_int.to(dev), s_w.to(dev)
            s_w = s_w.float().cpu().reshape(-1)
        w = np.rint(w_int.numpy().astype(np.float64)).astype(np.int64)
        nout, k = w.shape[0], w.shape[1]
        nout_p = _pad64(nout)
        fscale = np.zeros(nout_p, np.float32)
        fscale[:nout] = (s_w.view(1, -1) * s8.view(1, -1)).numpy().reshape(-1)   # fl(S_w[c] * S_a), quant_modules.py:735
        P['fc'] = dict(w=torch.from_numpy(packing.pack_conv_weight(w.reshape(nout, k, 1, 1), 8, _pad64(k), nout_p)).to(dev),
                       bias=_i32(np.zeros(nout_p), dev), fscale=torch.from_numpy(fscale).to(dev), nout=nout, nout_p=nout_p, k=_pad64(k))

    # ------------------------------------------------------------------ launch list
    def _conv_args(self, L, x, N, H, W):
        a = _lib.ConvArgs()
        a.in_, a.wgt, a.bias = x.data_ptr(), L.w.data_ptr(), L.bias.data_ptr()
        a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.stride, a.pad = N, H, W, L.cin_p, L.cout_p, L.kh, L.kw, L.stride, L.pad
        a.in_bits = a.w_bits = 8
        a.flags = self.flags.data_ptr()
        a.in_pitch = L.cin_s if L.cin_s != L.cin_p else 0       # 0 = dense rows
        a.out_pitch = L.cout_s if L.cout_s != L.cout_p else 0   # (RAW taps reset it: the accumulators are dense [M][Cout])
        return a

    def _one_launch(self, u, nq_fast, h, w) -> bool:
        """Does this unit run as one hawq_linear_bottleneck launch?  Needs: conv1 1x1 + depthwise 3x3 + conv3 1x1 with every requant
        table proved for the fast contract, block input and output at most 96 channels wide (the launch keeps the projection's
        accumulators of an 8 x 16 pixel tile in registers) - or, on output maps of at most 8 x 8 pixels, the 160 / 320-channel units of
        the width-1 network (8 x 8 tiles, the projection spread over the waves by output blocks; (h, w) = the unit's input map).  HAWQ_MBV2_UNFUSED=1: three launches per unit everywhere (A/B switch);
        tapped plans (keep_accumulators) always run the three launches - the taps ARE the intermediate tensors."""
        if self.keep_acc or os.environ.get("HAWQ_MBV2_UNFUSED") or os.environ.get("HAWQ_MBV2_EXACT") or os.environ.get("HAWQ_MBV2_PAD64"):
            return False
        if len(u['layers']) != 2:
            return False
        e1, e2 = u['layers']
        L1, L2, L3 = e1['layer'], e2['layer'], u['proj']['layer']
        if L1.groups != 1 or (L1.kh, L1.kw, L1.stride) != (1, 1, 1) or L2.groups == 1 or (L3.kh, L3.kw, L3.stride) != (1, 1, 1):
            return False
        if not e1.get('fast') or 'dw_ctab' not in e2 or u['proj']['fast'] is None or nq_fast is None:
            return False
        if u['residual'] and u.get('id_fast') is None:
            return False
        if e1['hi'] > 127 or e2['hi'] > 127:
            return False
        narrow = (16, 32, 64) if os.environ.get("HAWQ_MBV2_UNIT_TILE") == "1" else (16, 32, 64, 96)
        if L1.cin_s in narrow and L3.cout_s in narrow:
            return True
        # wider units: the launch's 8 x 8 tile family - output maps of at most 8 x 8 pixels (the 7 x 7 maps of the 224 x 224 network)
        ho, wo = (h - 1) // L2.stride + 1, (w - 1) // L2.stride + 1
        return (os.environ.get("HAWQ_MBV2_UNIT_TILE") != "1" and not os.environ.get("HAWQ_MBV2_NO_WIDE_UNITS") and ho <= 8 and wo <= 8 and L2.cout > 96
                and (L1.cin_s, L3.cout_s, L2.stride) in ((160, 160, 1), (96, 160, 2)))   # (the launch also takes 160 -> 320: 34 us against 29 us as three launches)

    def _tap(self, ops, keep, name, a, N, ho, wo, cout, cout_p):
        """extra RAW launch exposing the conv's int32 accumulators (tests only)"""
        acc = self._alloc(N * ho * wo * cout_p, torch.int32)
        r = _lib.ConvArgs()
        C.memmove(C.byref(r), C.byref(a), C.sizeof(r))
        r.epilogue, r.out_acc, r.res_in, r.res_out, r.out_q = _lib.EPI_RAW, acc.data_ptr(), None, None, None
        r.fast_tables, r.ctab, r.out_pitch = 0, None, 0
        keep += [acc, r]
        self.taps[name] = (acc, (N, ho, wo, cout_p), cout)
        ops.append(partial(_lib.call, "hawq_conv2d", C.byref(r), self.stream.cuda_stream))

    def _time_graph(self, reps: int = 12) -> float:
        return super()._time_graph(reps)

    def _on_graph_dropped(self):
        self.x_u8 = None

    def _build(self, N, H, W, x_view=None, logits_view=None):
        if x_view is None and self.chains_req == 0 and self.use_graph and N >= 16:
            timing = {}
            for c in (1, 2):   # keep whichever chain count replays faster
                self.chains = c
                self._build_chains(N, H, W)
                timing[c] = self._time_graph()
                self._drop_graph()
            self.chains, self.chain_timing_ms = min(timing, key=timing.get), timing
        self._build_chains(N, H, W, x_view, logits_view)

    def _build_chains(self, N, H, W, x_view=None, logits_view=None):
        self._drop_graph()
        if self.chains > 1 and N >= 2 * self.chains and x_view is None:
            nout = self.P['fc']['nout']
            self.x_in = torch.empty(N, 3, H, W, dtype=torch.float32, device=self.dev)
            self.logits = torch.empty(N, nout, dtype=torch.float32, device=self.dev)
            self.subs, b0 = [], 0
            for i in range(self.chains):
                b1 = b0 + N // self.chains + (1 if i < N % self.chains else 0)
                sub = self._spawn()
                sub._build_chains(b1 - b0, H, W, self.x_in[b0:b1], self.logits[b0:b1])
                self.subs.append(sub)
                b0 = b1
            self._ops, self._keep, self._batch, self.taps = [], [], (N, H, W), {}
            return
        self.subs = []
        self._build_one(N, H, W, x_view, logits_view)

    def _alloc(self, n, dtype):
        # 64 elements of slack: a conv that reads a narrow tensor through in_pitch fetches up to 48 bytes past the last pixel row
        return torch.empty(n + 64, dtype=dtype, device=self.dev)[:n]

    def _build_one(self, N, H, W, x_view=None, logits_view=None):
        P, dev, sp = self.P, self.dev, self.stream.cuda_stream
        ops, keep, self.taps, self._graph = [], [], {}, None
        self._convs, self._tuned = [], False   # hawq_conv2d argument structs of the plan (tile autotuning)
        self.n_fast = 0
        self.n_fused_units = 0    # units that run as ONE launch (hawq_linear_bottleneck)
        self.n_fast_closing = 0   # unit-closing launches whose tables are all proved: the direct epilogue with 3-instruction requants
        self.plan_bytes = N * 3 * H * W * 4   # bytes the plan has to move at the networks' true widths (no padding channels)
        alloc = self._alloc
        self.x_in = x_view if x_view is not None else alloc(N * 3 * H * W, torch.float32).view(N, 3, H, W)
        init = P['init']['layer']
        # the init block as ONE launch (hawq_stem3x3s2): input QuantAct + 3x3 / stride 2 conv + closing QuantActs, no patch rows in memory
        one_stem = bool(init.im2col and P['init']['fast'] is not None and P['units'][0]['q_fast'] is not None and not self.keep_acc
                        and init.cout_s in (16, 32) and not any(os.environ.get(k) for k in ("HAWQ_MBV2_UNFUSED", "HAWQ_MBV2_EXACT", "HAWQ_MBV2_PAD64")))
        self._stem_args = None
        if one_stem:
            H0, W0 = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
            xq = None
            self._u8_index, self._xq, self._u8_op = len(ops), None, None   # forward_uint8 swaps this launch for its uint8 form
        elif init.im2col:
            # input QuantAct (quant_modules.py:271-274) straight into the init conv's 27-value patches, one 64-byte row per output pixel
            H0, W0 = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
            xq = alloc(N * H0 * W0 * 64, torch.int8)
            self._u8_index, self._xq, self._u8_op = len(ops), xq, None   # forward_uint8 swaps this launch for the table look-up form
            ops.append(partial(_lib.call, "hawq_quantize_im2col3x3s2", self.x_in.data_ptr(), xq.data_ptr(), N, 3, H, W, P['inv_s_in'], -128, 127, sp))
            keep.append(xq)
        else:
            # input QuantAct then int8 NHWC, channels padded to 64
            self._u8_index = None
            H0, W0 = H, W
            xq_f = alloc(N * 3 * H * W, torch.float32)
            xq = alloc(N * H * W * init.cin_p, torch.int8).zero_()
            ops.append(partial(_lib.call, "hawq_fakequant_f32", self.x_in.data_ptr(), xq_f.data_ptr(), N * 3 * H * W, P['inv_s_in'], P['s_in'], -128, 127, sp))
            ops.append(partial(_lib.call, "hawq_f32_nchw_to_q_nhwc", xq_f.data_ptr(), xq.data_ptr(), N, 3, H, W, init.cin_p, 8, P['s_in'], sp))
            keep += [xq_f, xq]

        def closing(L, m, e, x, n, h, w, res_in, m_id, e_id, relu, clamp16, nxt_q, name, need16=True, fast=None, id_fast=None, q_fast=None,
                    unit=None, stem=None, carrier16=False):
            """conv + unit-closing 16-bit QuantAct (+ the next block-input QuantAct) -> (int32 tensor, int8 q, ho, wo);
            the 32-bit carrier is only written where something reads it (the next unit's identity, the pool, a tap).
            ``unit`` = dict(x, h, w, conv1 entry, conv2 entry): the whole unit as ONE launch (hawq_linear_bottleneck) - x is then the
            unit's block input and (h, w) the depthwise conv's output grid; ``stem`` = (H, W) of the images: the init block as ONE
            launch on them (hawq_stem3x3s2), L being its im2col form"""
            ho, wo = (h + 2 * L.pad - L.kh) // L.stride + 1, (w + 2 * L.pad - L.kw) // L.stride + 1
            a = self._conv_args(L, (x if unit is None else unit['x']) if stem is None else self.x_in, n, h, w)
            a.epilogue, a.m, a.e = _lib.EPI_RESIDUAL, m.data_ptr(), e.data_ptr()
            out16 = None
            u16 = bool(carrier16 and relu and clamp16 and not self.keep_acc)   # post-ReLU, clamped: 0 .. 32767 fits the uint16 carrier
            if need16 or self.keep_acc:
                out16 = alloc(n * ho * wo * L.cout_s, torch.int16 if u16 else torch.int32)
                a.res_out, a.res_out_bits = out16.data_ptr(), (16 if u16 else 32)
            in_bytes = h * w * L.cin if unit is None else unit['h'] * unit['w'] * unit['e1']['layer'].cin   # (the hidden tensors stay on chip)
            if stem is not None:
                in_bytes = 0   # (the images are already counted; no patch rows)
            self.plan_bytes += n * (in_bytes + ho * wo * L.cout * (((2 if u16 else 4) if need16 else 0) + (1 if nxt_q is not None else 0) + (4 if res_in is not None else 0))) + L.weight_bytes
            use_fast = (fast is not None and (res_in is None or id_fast is not None) and (nxt_q is None or q_fast is not None)
                        and not os.environ.get("HAWQ_MBV2_EXACT"))
            if res_in is not None:
                a.res_in, a.res_in_bits, a.m_id_scalar, a.e_id_scalar = res_in.data_ptr(), 32, m_id, e_id
                if use_fast:
                    a.m_id_scalar, a.e_id_scalar = id_fast[0], id_fast[1]
            a.res_no_relu, a.res_clamp16 = int(not relu), int(clamp16)
            a.n_valid = L.cout   # the exact epilogue skips the padding channels
            # every table of this launch lifted and bounded by the host -> the direct epilogue's 3-instruction requants (hawq_conv2d,
            # ConvP.gfast); otherwise its exact dyadic_rne form.  HAWQ_MBV2_EXACT=1: A/B switch for measurements
            if use_fast:
                tie = fast['tie'] or (res_in is not None and id_fast[2]) or (nxt_q is not None and q_fast[2])
                a.fast_tables, a.ctab = (5 if tie else 1), fast['ctab'].data_ptr()
                self.n_fast_closing = getattr(self, "n_fast_closing", 0) + 1
            q = None
            if nxt_q is not None:
                q = alloc(n * ho * wo * L.cout_s, torch.int8)
                a.out_q, a.out_bits, a.mq, a.eq, (a.q_lo, a.q_hi) = q.data_ptr(), 8, nxt_q[0], nxt_q[1], nxt_q[2]
                if use_fast:
                    a.mq, a.eq = q_fast[0], q_fast[1]
            if self.keep_acc:
                self._tap(ops, keep, name, a, n, ho, wo, L.cout, L.cout_p)
            keep.extend([a, out16, q])
            if unit is not None:
                if not use_fast:
                    raise RuntimeError("one-launch unit without proved tables (plan logic error)")
                e1, e2 = unit['e1'], unit['e2']
                L1, L2 = e1['layer'], e2['layer']
                b = _lib.BottleneckArgs()
                x1 = self._conv_args(L1, unit['x'], n, unit['h'], unit['w'])
                x1.epilogue, x1.relu, x1.q_lo, x1.q_hi, x1.out_bits = _lib.EPI_REQUANT, 1, e1['lo'], e1['hi'], 8
                x1.fast_tables, x1.ctab, x1.out_pitch = e1['fast'], e1['ctab'].data_ptr(), 0
                C.memmove(C.byref(b.expand), C.byref(x1), C.sizeof(x1))
                C.memmove(C.byref(b.project), C.byref(a), C.sizeof(a))
                b.dw_wgt9c, b.dw_ctab = L2.w9p.data_ptr(), e2['dw_ctab'].data_ptr()
                b.dw_stride, b.dw_q_lo, b.dw_q_hi, b.dw_fast_tables, b.c_mid = L2.stride, e2['lo'], e2['hi'], e2['dw_fast'], L2.cout
                b.tile = int(os.environ.get("HAWQ_MBV2_UNIT_TILE", 0))   # 1: the [pixel][channel] organisation of the launch (A/B switch)
                if not _lib.load().hawq_linear_bottleneck_ok(C.byref(b)):
                    raise RuntimeError("hawq_linear_bottleneck refuses a unit the plan selected for it")
                keep.append(b)
                self.plan_bytes += L1.weight_bytes + L2.weight_bytes
                self.n_fused_units += 1
                ops.append(partial(_lib.call, "hawq_linear_bottleneck", C.byref(b), sp))
            elif stem is not None:
                if not use_fast or not _lib.load().hawq_stem3x3s2_ok(self.x_in.data_ptr(), None, None, stem[0], stem[1], C.byref(a)):
                    raise RuntimeError("hawq_stem3x3s2 refuses the init block the plan selected for it")
                self._stem_args = a
                ops.append(partial(_lib.call, "hawq_stem3x3s2", self.x_in.data_ptr(), None, None, stem[0], stem[1], P['inv_s_in'], -128, 127, C.byref(a), sp))
            else:
                self._convs.append((name, a))
                ops.append(partial(_lib.call, "hawq_conv2d", C.byref(a), sp))
            if out16 is not None:
                self.taps[name + ":out16"] = (out16, (n, ho, wo, L.cout_s), L.cout)
            if q is not None:
                self.taps[name + ":next_q"] = (q, (n, ho, wo, L.cout_s), L.cout)
            return out16, q, ho, wo

        units = P['units']
        u0 = units[0]
        x16, q, h, w = closing(init, P['init']['m'], P['init']['e'], xq, N, H0, W0, None, 0, 33, True, True,
                               (u0['mq'], u0['eq'], u0['q_rng']), "init_block", need16=u0['residual'], fast=P['init']['fast'], q_fast=u0['q_fast'],
                               stem=(H, W) if one_stem else None)
        for ui, u in enumerate(units):
            name = f"unit{ui + 1}"
            x = q
            nxt = units[ui + 1] if ui + 1 < len(units) else None
            nq = (nxt['mq'], nxt['eq'], nxt['q_rng']) if nxt is not None else (P['before_final']['mq'], P['before_final']['eq'], P['before_final']['rng'])
            nq_fast = nxt['q_fast'] if nxt is not None else P['before_final']['q_fast']
            pr = u['proj']
            if self._one_launch(u, nq_fast, h, w):
                e1, e2 = u['layers']
                s2 = e2['layer'].stride
                ho, wo = (h - 1) // s2 + 1, (w - 1) // s2 + 1
                x16, q, h, w = closing(pr['layer'], pr['m'], pr['e'], None, N, ho, wo, x16 if u['residual'] else None, u.get('m_id', 0), u.get('e_id', 33),
                                       False, not u['residual'], nq, name + ".conv3", need16=bool(nxt is not None and nxt['residual']),
                                       fast=pr['fast'], id_fast=u.get('id_fast'), q_fast=nq_fast, unit=dict(x=x, h=h, w=w, e1=e1, e2=e2))
                continue
            for li, ent in enumerate(u['layers']):
                L = ent['layer']
                ho, wo = (h + 2 * L.pad - L.kh) // L.stride + 1, (w + 2 * L.pad - L.kw) // L.stride + 1
                out = alloc(N * ho * wo * L.cout_s, torch.int8)
                lname = f"{name}.{'conv1' if L.groups == 1 else 'conv2'}"
                if L.groups == 1:
                    a = self._conv_args(L, x, N, h, w)
                    a.epilogue, a.relu, a.m, a.e = _lib.EPI_REQUANT, 1, ent['m'].data_ptr(), ent['e'].data_ptr()
                    a.out_q, a.out_bits, a.q_lo, a.q_hi = out.data_ptr(), 8, ent['lo'], ent['hi']
                    if ent.get('fast'):
                        a.fast_tables, a.ctab = ent['fast'], ent['ctab'].data_ptr()
                        self.n_fast += 1
                    else:
                        a.n_valid = L.cout
                    if self.keep_acc:
                        self._tap(ops, keep, lname, a, N, ho, wo, L.cout, L.cout_p)
                    keep.append(a)
                    self._convs.append((lname, a))
                    ops.append(partial(_lib.call, "hawq_conv2d", C.byref(a), sp))
                else:
                    acc = alloc(N * ho * wo * L.cout_s, torch.int32) if self.keep_acc else None
                    if acc is not None:
                        self.taps[lname] = (acc, (N, ho, wo, L.cout_s), L.cout)
                    if acc is None and 'dw_ctab' in ent and ent['hi'] <= 127 and not os.environ.get("HAWQ_MBV2_EXACT"):
                        # the host-proved short requant (the accumulator tap needs the exact launch's second output)
                        ops.append(partial(_lib.call, "hawq_depthwise3x3_requant_fast", x.data_ptr(), L.w.data_ptr(), ent['dw_ctab'].data_ptr(), ent['dw_fast'] & 7,
                                           N, h, w, L.cout_s, L.cout, L.stride, ent['lo'], ent['hi'], out.data_ptr(), sp))
                    else:
                        ops.append(partial(_lib.call, "hawq_depthwise3x3_requant", x.data_ptr(), L.w.data_ptr(), L.bias.data_ptr(), ent['m'].data_ptr(),
                                           ent['e'].data_ptr(), N, h, w, L.cout_s, L.cout, L.stride, 1, ent['lo'], ent['hi'], out.data_ptr(),
                                           None if acc is None else acc.data_ptr(), sp))
                    keep.append(acc)
                self.plan_bytes += N * (h * w * L.cin + ho * wo * L.cout) + L.weight_bytes
                self.taps[lname + ":q"] = (out, (N, ho, wo, L.cout_s), L.cout)
                keep.append(out)
                x, h, w = out, ho, wo
            x16, q, h, w = closing(pr['layer'], pr['m'], pr['e'], x, N, h, w, x16 if u['residual'] else None, u.get('m_id', 0), u.get('e_id', 33),
                                   False, not u['residual'], nq, name + ".conv3", need16=bool(nxt is not None and nxt['residual']),
                                   fast=pr['fast'], id_fast=u.get('id_fast'), q_fast=nq_fast)
        fin = P['final']
        # (the final block's values are post-ReLU and clamped: a uint16 carrier halves what the pool reads)
        x16, _, h, w = closing(fin['layer'], fin['m'], fin['e'], q, N, h, w, None, 0, 33, True, True, None, "final_block", fast=fin['fast'], carrier16=True)
        cl = fin['layer'].cout_s
        if cl != fin['layer'].cout_p:
            raise PlanNotApplicable("the final block's width must be a multiple of 64 (the pool and the classifier read dense rows)")
        qf = alloc(N * cl, torch.int8)
        pooled = alloc(N * cl, torch.int32) if self.keep_acc else None
        o = P['out']
        ops.append(partial(_lib.call, "hawq_avgpool_requant", x16.data_ptr(), 16 if x16.dtype == torch.int16 else 32, N, h * w, cl, qf.data_ptr(), None if pooled is None else pooled.data_ptr(),
                           o['mq'], o['eq'], o['rng'][0], o['rng'][1], sp))
        fc = P['fc']
        if fc['k'] != cl:
            raise RuntimeError("classifier width does not match the final block")
        self.logits = logits_view if logits_view is not None else alloc(N * fc['nout'], torch.float32).view(N, fc['nout'])
        a = _lib.ConvArgs()
        a.in_, a.wgt, a.bias = qf.data_ptr(), fc['w'].data_ptr(), fc['bias'].data_ptr()
        a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.stride, a.pad = N, 1, 1, fc['k'], fc['nout_p'], 1, 1, 1, 0
        a.in_bits = a.w_bits = 8
        a.epilogue = _lib.EPI_DEQUANT
        a.out_f32, a.fscale, a.ldo, a.n_valid = self.logits.data_ptr(), fc['fscale'].data_ptr(), fc['nout'], fc['nout']
        if self.keep_acc:
            self._tap(ops, keep, "output", a, N, 1, 1, fc['nout'], fc['nout_p'])
        if _lib.load().hawq_fc_dequant_ok(N, fc['k'], fc['nout_p']) and not os.environ.get("HAWQ_NO_FC2"):
            # round 5: the classifier's own kernel (fc_dequant.hip), the same bytes as the DEQUANT epilogue; nothing to tune
            ops.append(partial(_lib.call, "hawq_fc_dequant", qf.data_ptr(), fc['w'].data_ptr(), fc['bias'].data_ptr(), fc['fscale'].data_ptr(),
                               self.logits.data_ptr(), N, fc['k'], fc['nout_p'], fc['nout'], fc['nout'], sp))
        else:
            self._convs.append(("output", a))
            ops.append(partial(_lib.call, "hawq_conv2d", C.byref(a), sp))
        keep += [qf, pooled, a]
        self._ops, self._keep, self._batch = ops, keep, (N, H, W)

    def _autotune(self, reps: int = 3):
        """Time every hawq_conv2d launch of the plan with each tile configuration the library accepts for it (HIP events on the
        engine stream, the real buffers - every tile gives the same integers) and keep the fastest; two rounds, per-tile minimum.
        HAWQ_MBV2_TILES replays a dotted list (as `tile_choice` prints it), HAWQ_MBV2_TILES=0 keeps the library's heuristic."""
        self._tuned = True
        fixed = os.environ.get("HAWQ_MBV2_TILES")
        if fixed is not None:
            ids = [int(v) for v in fixed.split(".")]
            for (_, a), t in zip(self._convs, ids if len(ids) == len(self._convs) else [0] * len(self._convs)):
                a.tile = t
            return
        lib, sp = _lib.load(), self.stream.cuda_stream
        n_tiles = lib.hawq_conv2d_num_tiles() - lib.hawq_conv2d_num_band_tiles()   # the 3x3 band tiles are not for 1x1 layers
        with EventTimer(sp) as timer:
            for _, a in self._convs:
                def tile(t):
                    a.tile = t
                    return partial(_lib.call, "hawq_conv2d", C.byref(a), sp)   # (raises when this tile does not take the launch)
                times = two_round_min(timer, range(1, n_tiles + 1), tile, reps)
                a.tile = min(times, key=times.get) if times else 0

    @property
    def tile_choice(self):
        return self.subs[0].tile_choice if self.subs else ".".join(str(a.tile) for _, a in self._convs)

    @property
    def total_plan_bytes(self):
        return sum(sub.plan_bytes for sub in self.subs) if self.subs else self.plan_bytes

    @property
    def fast_requant_launches(self):
        return self.subs[0].n_fast if self.subs else self.n_fast

    # ------------------------------------------------------------------ execution
    def _launch_chain(self, u8):
        if not self._tuned and not self.keep_acc:
            for op in self._ops:   # every buffer holds valid data before launches are timed on it
                op()
            self._autotune()
        for i, op in enumerate(self._ops):
            if u8 and i == self._u8_index:
                self._u8_op()
            else:
                op()

    # ------------------------------------------------------------------ uint8 image input (quant_train.py:428-440)
    def _ensure_u8(self, N, H, W, x_view=None, lut=None):
        if getattr(self, "x_u8", None) is not None:
            return
        self.lut_dev = lut if lut is not None else torch.zeros(3 * 256, dtype=torch.int8, device=self.dev)
        self._lut_key = None   # a fresh table buffer: the next forward_uint8 uploads its look-up table
        self.x_u8 = x_view if x_view is not None else torch.empty(N, H, W, 3, dtype=torch.uint8, device=self.dev)
        if self.subs:
            b0 = 0
            for sub in self.subs:
                n = sub._batch[0]
                sub._ensure_u8(n, H, W, self.x_u8[b0:b0 + n], self.lut_dev)
                b0 += n
            return
        if self._u8_index is None:
            raise NotImplementedError("uint8 input needs the im2col input quantiser (3x3 / stride 2 init conv on 3 channels)")
        if self._stem_args is not None:
            self._u8_op = partial(_lib.call, "hawq_stem3x3s2", None, self.x_u8.data_ptr(), self.lut_dev.data_ptr(), H, W, 0.0, 0, 0,
                                  C.byref(self._stem_args), self.stream.cuda_stream)
            return
        self._u8_op = partial(_lib.call, "hawq_quantize_im2col3x3s2_u8", self.x_u8.data_ptr(), self.lut_dev.data_ptr(), self._xq.data_ptr(),
                              N, 3, H, W, self.stream.cuda_stream)

    def forward_uint8(self, x_u8, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
        """uint8 NHWC images [N,H,W,3] (decoder output, after resize / crop) -> fp32 logits; bit for bit what ``self(normalised
        fp32 NCHW tensor)`` returns for the tensor the reference's data pipeline would have built (ToTensor + Normalize + the input
        QuantAct are one table look-up, ``hawq_amd.quant_utils.input_quant_lut``)."""
        if not x_u8.is_cuda or x_u8.dtype != torch.uint8 or x_u8.dim() != 4 or x_u8.shape[3] != 3:
            raise ValueError("expected a uint8 NHWC [N,H,W,3] tensor on the MI355X")
        return self._forward_uint8(x_u8, mean, std)

    def _upload_lut(self, mean, std):   # (this engine's kernels read the table flat)
        self.lut_dev.copy_(input_quant_lut(self.P['inv_s_in'], mean, std).reshape(-1).to(self.dev), non_blocking=False)

    @property
    def n_launches(self):
        return sum(len(sub._ops) for sub in self.subs) if self.subs else len(self._ops)

    def tap(self, name):
        """int32 / int8 NHWC tensor of a tapped stage as an NCHW int64 numpy array without the padding channels."""
        t, shp, c = self.taps[name]
        a = t.cpu().numpy().reshape(shp).astype(np.int64)[..., :c]
        return a.transpose(0, 3, 1, 2)
