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
Switches (results never change; set by any non-empty string, "0" included; ``Switches.from_env`` reads them ONCE, in the constructor,
and sub-chains share the record): HAWQ_MBV2_UNFUSED=1 three launches per unit and the im2col init block; HAWQ_MBV2_UNIT_TILE=1..4
organisation of the unit launch (``hawq_bottleneck_args.tile``; 1 also keeps units wider than 64 channels on three launches);
HAWQ_MBV2_NO_WIDE_UNITS=1 three launches for the 160-wide units of the 7 x 7 maps; HAWQ_MBV2_EXACT=1 exact closing epilogues and
depthwise requants, HAWQ_MBV2_PAD64=1 round 3's 64-padded tensors (both with UNFUSED's launch list); HAWQ_NO_FC2=1 the classifier on
``hawq_conv2d``.  HAWQ_MBV2_CHAINS is read by the constructor too, HAWQ_MBV2_TILES when a batch shape's launches are first tuned.

Records, choice, writer.  The form of a launch is decided by pure functions of the switches and plain numbers: ``unit_launches`` (a
unit as one launch or three), ``stem_form`` (the init block), ``closing_is_fast`` (a closing conv's epilogue).  ``_build_one`` is the
sequence of emitter calls for init block, units and head; each appends one ``Launch`` record per launch, in issue order, and the three
kinds of closing launch (``hawq_conv2d``, unit, stem) fill their closing conv's ``hawq_conv_args`` block in one function, ``_closing``.  Plan
bytes, counters, the tuner's list, ``taps`` and ``_stem_args`` are read off the records; one writer (``_write``) turns them into the callables
of a chain: ``_ops`` and, for ``forward_uint8``, ``_ops_u8``, which differs in the input launch alone.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import namedtuple
from functools import partial

import numpy as np
import torch

from . import _lib, packing
from .quant_modules import QuantBnConv2d
from .quant_utils import input_quant_lut, quantize_weight_per_channel, requant_table, tables_are_fast, tables_fit_fast
from .runner import EventTimer, GraphRunner, _i32, _rng, two_round_min


def _pad64(c: int) -> int:
    return (c + 63) // 64 * 64


class Switches(namedtuple("Switches", "unfused exact pad64 unit_tile no_wide_units no_fc2", defaults=(False, False, False, 0, False, False))):
    """The measurement switches of this engine (module docstring), as its constructor found them."""
    round3 = property(lambda self: self.unfused or self.exact or self.pad64)   # every unit on three launches, the init block on im2col rows

    @classmethod
    def from_env(cls, environ) -> "Switches":
        """From the mapping `environ`; a switch is set by any non-empty string (``os.environ.get`` truthiness: "0" sets it)."""
        on = [bool(environ.get(var)) for var in ("HAWQ_MBV2_UNFUSED", "HAWQ_MBV2_EXACT", "HAWQ_MBV2_PAD64", "HAWQ_MBV2_NO_WIDE_UNITS", "HAWQ_NO_FC2")]
        return cls(*on[:3], int(environ.get("HAWQ_MBV2_UNIT_TILE", 0)), *on[3:])


def _pitch(c: int, pad64: bool = False) -> int:
    """Channels per STORED pixel row of a c-channel tensor (round 4): the next multiple of 16, not of 64 - MobileNetV2's 16 / 24 / 32 /
    96 / 144 / 160-channel tensors are stored (almost) at their own width.  The GEMMs still see K and N padded to the 64-channel tile:
    a conv reads its K = pad64(c) bytes per pixel through `hawq_conv_args.in_pitch` (the bytes beyond the row meet zero weights) and
    writes only the first `out_pitch` channels of its 64-channel tiles (include/hawq_mi355.h, ABI 4).  `pad64` (HAWQ_MBV2_PAD64=1)
    restores the 64-padded tensors of round 3 (A/B switch for measurements)."""
    return _pad64(c) if pad64 else (c + 15) // 16 * 16


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


def _lifted(s_in, s_w, s_out, vbits, bias, dev):
    """The table of QuantAct(conv output) lifted to the conv kernels' fast contract (one v_mad_i64_i32 against a fused per-channel constant):
    None when it does not fit, else (ctab: the fused constants on the device, `bias` folded; m, e: the lifted tables padded to 64 channels,
    on the host; the launch's ``fast_tables`` word: bit 0 the contract, bit 2 exact round-half-even where the host cannot exclude a tie, bit 3 no pre-shifts)."""
    try:
        m, e = requant_table(s_in, s_w, s_out, vbits=vbits)
    except ValueError:
        return None
    if not tables_fit_fast(m, e, vbits):
        return None
    flags = (1 if tables_are_fast(m, e, vbits) else 5) | (8 if not (np.asarray(e) >> 8).any() else 0)
    cp = _pad64(len(bias))
    m, e = _padded(m, cp), _padded(e, cp, 33)
    return _i32(packing.pack_ctab(_padded(bias, cp), m, e), dev), m, e, flags


# What ``unit_launches`` reads of a unit: stored width of the block input, true width of the hidden tensors, stored width of the block output;
# strides and kernels of conv1, conv2, conv3; depthwise: conv1 dense, conv2 one group per channel; residual and whether the identity scalar is
# lifted; proved: conv1's, conv2's, conv3's table and the next block-input scalar are lifted for the fast contract; tops: conv1's / conv2's clamp
UnitShape = namedtuple("UnitShape", "cin_s hidden cout_s strides kernels depthwise residual id_proved proved tops",
                       defaults=((1, 1, 1), (1, 3, 1), True, False, True, (True,) * 4, (127, 127)))


def _unit_shape(u, q_proved: bool) -> UnitShape:
    """of the prepared unit `u` (an entry of ``P['units']``) in front of a block-input QuantAct whose scalar table is lifted or not"""
    e1, e2 = u['layers']
    L = L1, L2, L3 = e1['layer'], e2['layer'], u['proj']['layer']
    return UnitShape(L1.cin_s, L2.cout, L3.cout_s, tuple(l.stride for l in L), tuple(l.kh if l.kh == l.kw else (l.kh, l.kw) for l in L),
                     L1.groups == 1 and L2.groups != 1, u['residual'], u.get('id_fast') is not None,
                     (bool(e1.get('fast')), 'dw_ctab' in e2, u['proj']['fast'] is not None, q_proved), (e1['hi'], e2['hi']))


def unit_launches(sw: Switches, tapped: bool, u: UnitShape, h: int, w: int) -> int:
    """1: the unit on the (h, w) map runs as ONE hawq_linear_bottleneck launch; 3: conv1, conv2, conv3 launch by launch.  One launch needs
    conv1 1x1 + depthwise 3x3 + conv3 1x1, every requant table proved for the fast contract, and block input and output at most 96 channels
    wide (the launch keeps the projection's accumulators of an 8 x 16 pixel tile in registers) - or, on output maps of at most 8 x 8 pixels
    (the 7 x 7 maps of the 224 x 224 network), the 160-wide units of the width-1 network (8 x 8 tiles, the projection spread over the waves
    by output blocks).  Tapped plans (keep_accumulators) always run three launches - the taps ARE the intermediate tensors."""
    pointwise = u.depthwise and u.kernels == (1, 3, 1) and u.strides[0] == u.strides[2] == 1
    if tapped or sw.round3 or not pointwise or not all(u.proved) or (u.residual and not u.id_proved) or max(u.tops) > 127:
        return 3
    narrow = (16, 32, 64) if sw.unit_tile == 1 else (16, 32, 64, 96)
    if u.cin_s in narrow and u.cout_s in narrow:
        return 1
    s2 = u.strides[1]
    wide = (sw.unit_tile != 1 and not sw.no_wide_units and (h - 1) // s2 + 1 <= 8 and (w - 1) // s2 + 1 <= 8 and u.hidden > 96
            and (u.cin_s, u.cout_s, s2) in ((160, 160, 1), (96, 160, 2)))   # (the launch also takes 160 -> 320: 34 us against 29 us as three launches)
    return 1 if wide else 3


def stem_form(sw: Switches, tapped: bool, im2col: bool, cout_s: int, proved: bool) -> str:
    """The init block: "one" launch (hawq_stem3x3s2: input QuantAct + 3x3 / stride 2 conv + closing QuantActs, no patch rows in memory;
    `proved`: its table and unit 1's block-input scalar are lifted), "im2col" (the input quantiser writes 27-value patch rows for a 1x1
    conv) or "nhwc" (int8 NHWC padded to 64 channels: an init conv that is not 3x3 / stride 2 on 3 channels)."""
    if not im2col:
        return "nhwc"
    return "one" if proved and not tapped and not sw.round3 and cout_s in (16, 32) else "im2col"


def closing_is_fast(sw: Switches, proved: bool, id_proved: bool, q_proved: bool) -> bool:
    """A closing conv runs the direct epilogue's 3-instruction requants (hawq_conv2d, ConvP.gfast) when every table of the launch is lifted
    and bounded by the host - its own, the identity branch's, the next block-input QuantAct's (True where it has none) -, else the exact ones."""
    return proved and id_proved and q_proved and not sw.exact


class Launch:
    """One launch of a chain: `stage`, the base name of its taps (``init_block``, ``unit7.conv2``, ``final_block``, ``output`` ...; a one-launch
    unit carries its closing conv's, ``unit7.conv3``); the entry point `name`; `args`, the call's arguments before the stream (a ctypes block
    stands for its address); `kind`: "conv" (a hawq_conv2d the tuner may give a tile), "unit", "stem", "depthwise" or "other"; `nbytes`, what it
    moves at the network's true widths; `taps`, the tensors it exposes (name -> (tensor, stored NHWC shape, true channels)); `fast`: "expand" (conv1 on
    the fast REQUANT epilogue), "closing" (a closing conv, all tables proved) or None; `geom`: (N, H, W, stored C, true C, stride) where `args` hold no block."""
    __slots__ = ("stage", "name", "args", "kind", "nbytes", "taps", "fast", "geom")

    def __init__(self, stage, name, args, kind="other", nbytes=0, taps=None, fast=None, geom=None):
        self.stage, self.name, self.args, self.kind, self.nbytes, self.taps, self.fast, self.geom = stage, name, tuple(args), kind, nbytes, taps or {}, fast, geom


def plan_totals(launches) -> dict:
    """what the launches move; conv launches on the fast REQUANT epilogue; units that run as ONE launch; closing launches (conv, unit, stem) with all tables proved"""
    return dict(plan_bytes=sum(r.nbytes for r in launches), n_fast=sum(r.fast == "expand" for r in launches),
                n_fused_units=sum(r.kind == "unit" for r in launches), n_fast_closing=sum(r.fast == "closing" for r in launches))


class _Layer:
    """Device-resident integer parameters of one QuantBnConv2d, channel-padded."""

    def __init__(self, mod: QuantBnConv2d, s_a, dev, from_buffers, im2col=False, pad64=False):
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
        self.cin_s, self.cout_s = (self.cin_p if im2col else _pitch(self.cin, pad64)), _pitch(self.cout, pad64)   # (im2col: the init layer, either input form)
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
    # an engine that has not built a plan - and a sub-chain: one chain, no graph of its own
    use_graph, chains, chains_req, _launches, _ops, taps = False, 1, 1, (), (), {}
    _batch = x_u8 = _ops_u8 = None

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
        self.sw = Switches.from_env(os.environ)
        self.chains_req = 1 if keep_accumulators else max(0, int(os.environ.get("HAWQ_MBV2_CHAINS", chains)))
        self.chains = max(1, self.chains_req)
        self._prepare()

    def _spawn(self):
        """a chain of this plan: shares the prepared parameters and the switches, owns its stream and activation buffers"""
        sub = object.__new__(MobileNetV2Engine)
        sub.keep_acc, sub.dev, sub.flags, sub.P, sub.sw, sub.stream = self.keep_acc, self.dev, self.flags, self.P, self.sw, torch.cuda.Stream(device=self.dev)
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

        def conv_layer(mod, s_a, im2col=False):
            return _Layer(mod, s_a, dev, self.from_buffers, im2col, self.sw.pad64)

        def closing(L, s_a, s_o, relu6=None):
            """a conv that closes a stage: its exact table and, where the lifted one fits the fast contract, `fast` = dict(ctab, tie);
            `relu6` names the QuantAct of the init / final block, behind a ReLU6: refused if that is not ReLU + clamp here"""
            md, ed, mh, eh = L.table(s_a, s_o, dev)
            if relu6 and not _relu6_is_relu(float(s_a.item()), L.s_w.numpy(), mh, eh, 32767):
                raise PlanNotApplicable(f"{relu6} range above 6.0 behind ReLU6")
            lifted = _lifted(s_a, L.s_w, s_o, L.vbits, L.b_host, dev)
            return dict(layer=L, m=md, e=ed, fast=None if lifted is None else dict(ctab=lifted[0], tie=bool(lifted[3] & 4))), mh, eh

        def activated(layer, s_a, act):
            """conv -> ReLU6 -> QuantAct(case 0): table + clamp; refuses if ReLU6 is not ReLU + clamp here"""
            s_o = self._scale(act)
            md, ed, mh, eh = layer.table(s_a, s_o, dev)
            lo, hi = _rng(act)
            if not _relu6_is_relu(float(s_a.item()), layer.s_w.numpy(), mh, eh, hi):
                raise PlanNotApplicable("a QuantAct range above 6.0 behind ReLU6: the integer plan folds ReLU6 into the clamp")
            ent = dict(layer=layer, m=md, e=ed, lo=max(lo, 0), hi=hi, s=s_o)
            lifted = _lifted(s_a, layer.s_w, s_o, layer.vbits, layer.b_host, dev)
            if lifted is not None and layer.groups == 1:   # the conv kernels' short requant instead of the exact table
                ent.update(ctab=lifted[0], m=_i32(lifted[1], dev), e=_i32(lifted[2], dev), fast=lifted[3])
            elif lifted is not None:   # depthwise: for the one-launch unit and hawq_depthwise3x3_requant_fast; the exact launch keeps (m, e)
                ent.update(dw_ctab=lifted[0], dw_fast=lifted[3])
            return ent

        # init block: conv -> ReLU6 -> quant_act_int32 (16 bit)
        s16 = act16(m.quant_act_int32)
        P['init'] = closing(conv_layer(m.init_block, s_in, im2col=True), s_in, s16, "quant_act_int32")[0]
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
                ent = activated(conv_layer(getattr(u, conv), s_x), s_x, getattr(u, act))
                d['layers'].append(ent)
                s_x = ent['s']
            proj = conv_layer(u.conv3, s_x)
            s_o = act16(u.quant_act_int32)
            d['proj'], mh3, eh3 = closing(proj, s_x, s_o)
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
        s_f = act16(m.quant_act_int32_final)
        P['final'] = closing(conv_layer(m.features.final_block, s_b), s_b, s_f, "quant_act_int32_final")[0]
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

    # ------------------------------------------------------------------ launch records
    def _alloc(self, n, dtype):
        # 64 elements of slack: a conv that reads a narrow tensor through in_pitch fetches up to 48 bytes past the last pixel row
        return torch.empty(n + 64, dtype=dtype, device=self.dev)[:n]

    def _buf(self, n, dtype):
        """a plan buffer: kept alive with the plan (the captured launches hold its address)"""
        self._keep.append(self._alloc(n, dtype))
        return self._keep[-1]

    def _emit(self, r: Launch, tap=None):
        """The next record of the chain.  A tapped plan (tests only) first exposes the int32 accumulators of the record's conv, `tap`
        = (its argument block, true output channels), through a RAW launch on a copy of the block, under the record's stage name."""
        if tap is not None and self.keep_acc:
            a, cout = tap
            ho, wo = (a.H + 2 * a.pad - a.KH) // a.stride + 1, (a.W + 2 * a.pad - a.KW) // a.stride + 1
            acc, raw = self._buf(a.N * ho * wo * a.Cout, torch.int32), _lib.ConvArgs()   # (the accumulators are dense [M][Cout])
            C.memmove(C.byref(raw), C.byref(a), C.sizeof(raw))
            raw.epilogue, raw.out_acc, raw.res_in, raw.res_out, raw.out_q = _lib.EPI_RAW, acc.data_ptr(), None, None, None
            raw.fast_tables, raw.ctab, raw.out_pitch = 0, None, 0
            self._launches.append(Launch(r.stage, "hawq_conv2d", (raw,), taps={r.stage: (acc, (a.N, ho, wo, a.Cout), cout)}))
        self._launches.append(r)

    def _conv_args(self, L, x, N, H, W):
        a = _lib.ConvArgs()
        a.in_, a.wgt, a.bias = x.data_ptr(), L.w.data_ptr(), L.bias.data_ptr()
        a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.stride, a.pad = N, H, W, L.cin_p, L.cout_p, L.kh, L.kw, L.stride, L.pad
        a.in_bits, a.w_bits, a.flags = 8, 8, self.flags.data_ptr()
        a.in_pitch = L.cin_s if L.cin_s != L.cin_p else 0       # 0 = dense rows
        a.out_pitch = L.cout_s if L.cout_s != L.cout_p else 0   # (RAW taps reset it)
        return a

    def _closing(self, stage, ent, x, n, h, w, res, nxt, relu, need16=True, carrier16=False):
        """The hawq_conv_args block of a closing conv `ent` (P['init'], a unit's 'proj', P['final']) on an (h, w) map with `x`'s address as its input:
        conv + 16-bit QuantAct - the identity branch `res` = (int32 carrier, m_id, e_id, id_fast) summed in and the sum not clamped, or None - + the
        next block-input QuantAct `nxt` = (mq, eq, (lo, hi), q_fast) or None.  The carrier is only written where something reads it (`need16`: the next unit's
        identity, the pool; or a tap), as uint16 where `carrier16` allows.  -> (block, carrier, int8 q, ho, wo, fast, bytes written + weight bytes, taps)"""
        L = ent['layer']
        ho, wo = (h + 2 * L.pad - L.kh) // L.stride + 1, (w + 2 * L.pad - L.kw) // L.stride + 1
        a, taps, out16, q, shape = self._conv_args(L, x, n, h, w), {}, None, None, (n, ho, wo, L.cout_s)
        a.epilogue, a.m, a.e = _lib.EPI_RESIDUAL, ent['m'].data_ptr(), ent['e'].data_ptr()
        a.res_no_relu, a.res_clamp16, a.n_valid = int(not relu), int(res is None), L.cout   # (the exact epilogue skips the padding channels)
        fast = closing_is_fast(self.sw, ent['fast'] is not None, res is None or res[3] is not None, nxt is None or nxt[3] is not None)
        if fast:
            tie = ent['fast']['tie'] or (res is not None and res[3][2]) or (nxt is not None and nxt[3][2])
            a.fast_tables, a.ctab = (5 if tie else 1), ent['fast']['ctab'].data_ptr()
        u16 = bool(carrier16 and relu and res is None and not self.keep_acc)   # post-ReLU, clamped: 0 .. 32767 fits the uint16 carrier
        if need16 or self.keep_acc:
            out16 = self._buf(n * ho * wo * L.cout_s, torch.int16 if u16 else torch.int32)
            a.res_out, a.res_out_bits, taps[stage + ":out16"] = out16.data_ptr(), (16 if u16 else 32), (out16, shape, L.cout)
        if res is not None:
            a.res_in, a.res_in_bits, (a.m_id_scalar, a.e_id_scalar) = res[0].data_ptr(), 32, (res[3][:2] if fast else res[1:3])
        if nxt is not None:
            q = self._buf(n * ho * wo * L.cout_s, torch.int8)
            a.out_q, a.out_bits, (a.q_lo, a.q_hi), (a.mq, a.eq) = q.data_ptr(), 8, nxt[2], (nxt[3][:2] if fast else nxt[:2])
            taps[stage + ":next_q"] = (q, shape, L.cout)
        per_pixel = ((2 if u16 else 4) if need16 else 0) + (1 if nxt is not None else 0) + (4 if res is not None else 0)
        return a, out16, q, ho, wo, fast, n * ho * wo * L.cout * per_pixel + L.weight_bytes, taps

    def _emit_closing_conv(self, stage, ent, x, n, h, w, res, nxt, relu, need16=True, carrier16=False):
        """a closing conv on its own: hawq_conv2d on the int8 tensor `x` -> (carrier, q, ho, wo)"""
        a, out16, q, ho, wo, fast, nbytes, taps = self._closing(stage, ent, x, n, h, w, res, nxt, relu, need16, carrier16)
        self._emit(Launch(stage, "hawq_conv2d", (a,), "conv", nbytes + n * h * w * ent['layer'].cin, taps, "closing" if fast else None), tap=(a, ent['layer'].cout))
        return out16, q, ho, wo

    def _emit_unit(self, stage, u, x, n, h, w, res, nxt, need16):
        """a whole unit on its block input `x` (an (h, w) map) as ONE hawq_linear_bottleneck launch: the hidden tensors stay on chip"""
        (e1, e2), b = u['layers'], _lib.BottleneckArgs()
        L1, L2 = e1['layer'], e2['layer']
        a, out16, q, ho, wo, fast, nbytes, taps = self._closing(stage, u['proj'], x, n, (h - 1) // L2.stride + 1, (w - 1) // L2.stride + 1,
                                                               res, nxt, False, need16)
        if not fast:
            raise RuntimeError("one-launch unit without proved tables (plan logic error)")
        x1 = self._conv_args(L1, x, n, h, w)
        x1.epilogue, x1.relu, x1.q_lo, x1.q_hi, x1.out_bits = _lib.EPI_REQUANT, 1, e1['lo'], e1['hi'], 8
        x1.fast_tables, x1.ctab, x1.out_pitch = e1['fast'], e1['ctab'].data_ptr(), 0
        C.memmove(C.byref(b.expand), C.byref(x1), C.sizeof(x1))
        C.memmove(C.byref(b.project), C.byref(a), C.sizeof(a))
        b.dw_wgt9c, b.dw_ctab, b.tile = L2.w9p.data_ptr(), e2['dw_ctab'].data_ptr(), self.sw.unit_tile   # (tile 1: the [pixel][channel] organisation, A/B switch)
        b.dw_stride, b.dw_q_lo, b.dw_q_hi, b.dw_fast_tables, b.c_mid = L2.stride, e2['lo'], e2['hi'], e2['dw_fast'], L2.cout
        if not _lib.load().hawq_linear_bottleneck_ok(C.byref(b)):
            raise RuntimeError("hawq_linear_bottleneck refuses a unit the plan selected for it")
        self._emit(Launch(stage, "hawq_linear_bottleneck", (b,), "unit", nbytes + n * h * w * L1.cin + L1.weight_bytes + L2.weight_bytes, taps, "closing"))
        return out16, q, ho, wo

    def _emit_hidden(self, stage, ent, x, n, h, w):
        """an activated conv of a unit on its own: conv1 (hawq_conv2d, REQUANT) or the depthwise conv2 -> (int8 tensor, ho, wo)"""
        L = ent['layer']
        ho, wo = (h + 2 * L.pad - L.kh) // L.stride + 1, (w + 2 * L.pad - L.kw) // L.stride + 1
        out, nbytes, shape = self._buf(n * ho * wo * L.cout_s, torch.int8), n * (h * w * L.cin + ho * wo * L.cout) + L.weight_bytes, (n, ho, wo, L.cout_s)
        taps, geom = {stage + ":q": (out, shape, L.cout)}, (n, h, w, L.cout_s, L.cout, L.stride)
        if L.groups == 1:
            a = self._conv_args(L, x, n, h, w)
            a.epilogue, a.relu, a.m, a.e = _lib.EPI_REQUANT, 1, ent['m'].data_ptr(), ent['e'].data_ptr()
            a.out_q, a.out_bits, a.q_lo, a.q_hi = out.data_ptr(), 8, ent['lo'], ent['hi']
            if ent.get('fast'):
                a.fast_tables, a.ctab = ent['fast'], ent['ctab'].data_ptr()
            else:
                a.n_valid = L.cout
            self._emit(Launch(stage, "hawq_conv2d", (a,), "conv", nbytes, taps, "expand" if ent.get('fast') else None), tap=(a, L.cout))
        elif not self.keep_acc and 'dw_ctab' in ent and ent['hi'] <= 127 and not self.sw.exact:   # the host-proved short requant
            self._emit(Launch(stage, "hawq_depthwise3x3_requant_fast", (x.data_ptr(), L.w.data_ptr(), ent['dw_ctab'].data_ptr(), ent['dw_fast'] & 7, *geom,
                                                                        ent['lo'], ent['hi'], out.data_ptr()), "depthwise", nbytes, taps, geom=geom))
        else:   # (a tapped plan's accumulators are this launch's second output)
            acc = self._buf(n * ho * wo * L.cout_s, torch.int32) if self.keep_acc else None
            taps.update({stage: (acc, shape, L.cout)} if self.keep_acc else {})
            self._emit(Launch(stage, "hawq_depthwise3x3_requant", (x.data_ptr(), L.w.data_ptr(), L.bias.data_ptr(), ent['m'].data_ptr(), ent['e'].data_ptr(), *geom,
                                                                   1, ent['lo'], ent['hi'], out.data_ptr(), acc.data_ptr() if self.keep_acc else None), "depthwise", nbytes, taps, geom=geom))
        return out, ho, wo

    def _emit_init(self, N, H, W, nxt, need16):
        """the input QuantAct and the init block, in the form ``stem_form`` chooses -> (carrier, q, ho, wo)"""
        P, ent = self.P, self.P['init']
        init, x_in, images = ent['layer'], self.x_in.data_ptr(), N * 3 * H * W * 4
        form = stem_form(self.sw, self.keep_acc, init.im2col, init.cout_s, ent['fast'] is not None and nxt[3] is not None)
        H0, W0 = ((H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1) if init.im2col else (H, W)
        if form == "one":   # (no patch rows in memory: the launch reads the images)
            a, out16, q, ho, wo, fast, nbytes, taps = self._closing("init_block", ent, self.x_in, N, H0, W0, None, nxt, True, need16)
            if not fast or not _lib.load().hawq_stem3x3s2_ok(x_in, None, None, H, W, C.byref(a)):
                raise RuntimeError("hawq_stem3x3s2 refuses the init block the plan selected for it")
            self._emit(Launch("init_block", "hawq_stem3x3s2", (x_in, None, None, H, W, P['inv_s_in'], -128, 127, a), "stem", images + nbytes, taps, "closing"))
            return out16, q, ho, wo
        if form == "im2col":   # input QuantAct (quant_modules.py:271-274) straight into the init conv's 27-value patches, one 64-byte row per output pixel
            xq = self._buf(N * H0 * W0 * 64, torch.int8)
            self._emit(Launch("quant_input", "hawq_quantize_im2col3x3s2", (x_in, xq.data_ptr(), N, 3, H, W, P['inv_s_in'], -128, 127), nbytes=images))
        else:   # input QuantAct then int8 NHWC, channels padded to 64
            xq_f, xq = self._buf(N * 3 * H * W, torch.float32), self._buf(N * H * W * init.cin_p, torch.int8).zero_()
            self._emit(Launch("quant_input", "hawq_fakequant_f32", (x_in, xq_f.data_ptr(), N * 3 * H * W, P['inv_s_in'], P['s_in'], -128, 127), nbytes=images))
            self._emit(Launch("quant_input", "hawq_f32_nchw_to_q_nhwc", (xq_f.data_ptr(), xq.data_ptr(), N, 3, H, W, init.cin_p, 8, P['s_in'])))
        return self._emit_closing_conv("init_block", ent, xq, N, H0, W0, None, nxt, True, need16)

    def _emit_head(self, q, N, h, w, logits_view):
        """final block, average pool (+ quant_act_output) and the classifier (+ dequant) into ``logits``"""
        fin, o, fc = self.P['final'], self.P['out'], self.P['fc']
        x16, _, h, w = self._emit_closing_conv("final_block", fin, q, N, h, w, None, None, True, carrier16=True)   # (post-ReLU, clamped: a uint16 carrier halves what the pool reads)
        cl = fin['layer'].cout_s
        if cl != fin['layer'].cout_p:
            raise PlanNotApplicable("the final block's width must be a multiple of 64 (the pool and the classifier read dense rows)")
        if fc['k'] != cl:
            raise RuntimeError("classifier width does not match the final block")
        qf, pooled = self._buf(N * cl, torch.int8), (self._buf(N * cl, torch.int32) if self.keep_acc else None)
        self._emit(Launch("pool", "hawq_avgpool_requant", (x16.data_ptr(), 16 if x16.dtype == torch.int16 else 32, N, h * w, cl, qf.data_ptr(),
                          None if pooled is None else pooled.data_ptr(), o['mq'], o['eq'], o['rng'][0], o['rng'][1]), geom=(N, h, w, cl, cl, 1)))
        self.logits = logits_view if logits_view is not None else self._buf(N * fc['nout'], torch.float32).view(N, fc['nout'])
        a = _lib.ConvArgs()
        a.in_, a.wgt, a.bias = qf.data_ptr(), fc['w'].data_ptr(), fc['bias'].data_ptr()
        a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.stride, a.pad = N, 1, 1, fc['k'], fc['nout_p'], 1, 1, 1, 0
        a.in_bits, a.w_bits, a.epilogue = 8, 8, _lib.EPI_DEQUANT
        a.out_f32, a.fscale, a.ldo, a.n_valid = self.logits.data_ptr(), fc['fscale'].data_ptr(), fc['nout'], fc['nout']
        if _lib.load().hawq_fc_dequant_ok(N, fc['k'], fc['nout_p']) and not self.sw.no_fc2:
            # round 5: the classifier's own kernel (fc_dequant.hip), the same bytes as the DEQUANT epilogue; nothing to tune
            r = Launch("output", "hawq_fc_dequant", (a.in_, a.wgt, a.bias, a.fscale, a.out_f32, N, fc['k'], fc['nout_p'], fc['nout'], fc['nout']),
                       geom=(N, 1, 1, fc['k'], fc['nout'], 1))
        else:
            r = Launch("output", "hawq_conv2d", (a,), "conv")
        self._emit(r, tap=(a, fc['nout']))

    def _build_one(self, N, H, W, x_view=None, logits_view=None):
        """the records of one chain over N images, in issue order - init block, units, head - and its callables"""
        units, b = self.P['units'], self.P['before_final']
        self._launches, self._keep, self._graph, self._tuned = [], [], None, False
        self.x_in = x_view if x_view is not None else self._buf(N * 3 * H * W, torch.float32).view(N, 3, H, W)
        block_in = [(u['mq'], u['eq'], u['q_rng'], u['q_fast']) for u in units] + [(b['mq'], b['eq'], b['rng'], b['q_fast'])]   # the block-input QuantActs
        x16, q, h, w = self._emit_init(N, H, W, block_in[0], need16=units[0]['residual'])
        for ui, u in enumerate(units):
            name, nxt = f"unit{ui + 1}", block_in[ui + 1]
            res = (x16, u['m_id'], u['e_id'], u.get('id_fast')) if u['residual'] else None
            need16 = bool(ui + 1 < len(units) and units[ui + 1]['residual'])
            if len(u['layers']) == 2 and unit_launches(self.sw, self.keep_acc, _unit_shape(u, nxt[3] is not None), h, w) == 1:
                x16, q, h, w = self._emit_unit(name + ".conv3", u, q, N, h, w, res, nxt, need16)
                continue
            for ent in u['layers']:
                q, h, w = self._emit_hidden(f"{name}.{'conv1' if ent['layer'].groups == 1 else 'conv2'}", ent, q, N, h, w)
            x16, q, h, w = self._emit_closing_conv(name + ".conv3", u['proj'], q, N, h, w, res, nxt, False, need16)
        self._emit_head(q, N, h, w, logits_view)
        self.taps, self._batch = {k: v for r in self._launches for k, v in r.taps.items()}, (N, H, W)
        self._ops, self._ops_u8 = self._write(), None

    # ------------------------------------------------------------------ chains, tuning
    def _on_graph_dropped(self):
        self.x_u8 = self._ops_u8 = None

    def _build(self, N, H, W, x_view=None, logits_view=None):
        if x_view is None and self.chains_req == 0 and self.use_graph and N >= 16:
            timing = {}
            for c in (1, 2):   # keep whichever chain count replays faster
                self.chains = c
                self._build_chains(N, H, W)
                timing[c] = self._time_graph(12)
                self._drop_graph()
            self.chains, self.chain_timing_ms = min(timing, key=timing.get), timing
        self._build_chains(N, H, W, x_view, logits_view)

    def _build_chains(self, N, H, W, x_view=None, logits_view=None):
        self._drop_graph()
        if self.chains > 1 and N >= 2 * self.chains and x_view is None:
            self.x_in = torch.empty(N, 3, H, W, dtype=torch.float32, device=self.dev)
            self.logits = torch.empty(N, self.P['fc']['nout'], dtype=torch.float32, device=self.dev)
            self.subs, b0 = [], 0
            for i in range(self.chains):
                b1 = b0 + N // self.chains + (1 if i < N % self.chains else 0)
                sub = self._spawn()
                sub._build_chains(b1 - b0, H, W, self.x_in[b0:b1], self.logits[b0:b1])
                self.subs.append(sub)
                b0 = b1
            self._launches, self._ops, self._keep, self._batch, self.taps = [], [], [], (N, H, W), {}
            return
        self.subs = []
        self._build_one(N, H, W, x_view, logits_view)

    def _autotune(self, reps: int = 3):
        """Time every hawq_conv2d launch of the plan with each tile configuration the library accepts for it (HIP events on the
        engine stream, the real buffers - every tile gives the same integers) and keep the fastest; two rounds, per-tile minimum.
        HAWQ_MBV2_TILES replays a dotted list (as `tile_choice` prints it), HAWQ_MBV2_TILES=0 keeps the library's heuristic."""
        self._tuned = True
        convs, fixed = self._convs, os.environ.get("HAWQ_MBV2_TILES")
        if fixed is not None:
            ids = [int(v) for v in fixed.split(".")]
            for (_, a), t in zip(convs, ids if len(ids) == len(convs) else [0] * len(convs)):
                a.tile = t
            return
        lib, sp = _lib.load(), self.stream.cuda_stream
        n_tiles = lib.hawq_conv2d_num_tiles() - lib.hawq_conv2d_num_band_tiles()   # the 3x3 band tiles are not for 1x1 layers
        with EventTimer(sp) as timer:
            for _, a in convs:
                def tile(t):
                    a.tile = t
                    return partial(_lib.call, "hawq_conv2d", C.byref(a), sp)   # (raises when this tile does not take the launch)
                times = two_round_min(timer, range(1, n_tiles + 1), tile, reps)
                a.tile = min(times, key=times.get) if times else 0

    # ------------------------------------------------------------------ read off the records
    # (stage, argument block) of the hawq_conv2d launches the tuner may give a tile, in issue order
    _convs = property(lambda self: [(r.stage, r.args[0]) for r in self._launches if r.kind == "conv"])
    tile_choice = property(lambda self: self.subs[0].tile_choice if self.subs else ".".join(str(a.tile) for _, a in self._convs))
    # the init block's argument block where it runs as one hawq_stem3x3s2 launch, else None
    _stem_args = property(lambda self: self._launches[0].args[-1] if self._launches and self._launches[0].kind == "stem" else None)

    def _total(self, key):
        """`key` of ``plan_totals`` for this chain or, of a split batch, for its first sub-chain (every chain takes the same decisions)"""
        return plan_totals((self.subs[0] if self.subs else self)._launches)[key]

    plan_bytes = property(lambda self: plan_totals(self._launches)["plan_bytes"])
    total_plan_bytes = property(lambda self: sum(sub.plan_bytes for sub in self.subs) if self.subs else self.plan_bytes)
    n_launches = property(lambda self: sum(len(sub._ops) for sub in self.subs) if self.subs else len(self._ops))
    fast_requant_launches = property(lambda self: self._total("n_fast"))
    n_fused_units = property(lambda self: self._total("n_fused_units"))
    n_fast_closing = property(lambda self: self._total("n_fast_closing"))

    # ------------------------------------------------------------------ the writer, execution
    def _write(self, u8=False):
        """The callables of this chain, from its records - the only place that makes one.  `u8`: the chain of ``forward_uint8``, the fp32
        chain behind the uint8 form of its input launch (the one-launch stem, or the im2col input quantiser, as a table look-up on ``x_u8``)."""
        def op(name, *args):
            return partial(_lib.call, name, *(C.byref(v) if isinstance(v, C.Structure) else v for v in args), self.stream.cuda_stream)

        if not u8:
            return [op(r.name, *r.args) for r in self._launches]
        first, (N, H, W) = self._launches[0], self._batch
        if first.kind == "stem":
            head = op("hawq_stem3x3s2", None, self.x_u8.data_ptr(), self.lut_dev.data_ptr(), H, W, 0.0, 0, 0, first.args[-1])
        elif first.name == "hawq_quantize_im2col3x3s2":
            head = op("hawq_quantize_im2col3x3s2_u8", self.x_u8.data_ptr(), self.lut_dev.data_ptr(), first.args[1], N, 3, H, W)
        else:
            raise NotImplementedError("uint8 input needs the im2col input quantiser (3x3 / stride 2 init conv on 3 channels)")
        return [head] + self._ops[1:]

    def _launch_chain(self, u8):
        if not self._tuned and not self.keep_acc:
            for op in self._ops:   # every buffer holds valid data before launches are timed on it
                op()
            self._autotune()
        for op in (self._ops_u8 if u8 else self._ops):
            op()

    # ------------------------------------------------------------------ uint8 image input (quant_train.py:428-440)
    def _ensure_u8(self, N, H, W, x_view=None, lut=None):
        if self.x_u8 is not None:
            return
        self.lut_dev = lut if lut is not None else torch.zeros(3 * 256, dtype=torch.int8, device=self.dev)
        self._lut_key = None   # a fresh table buffer: the next forward_uint8 uploads its look-up table
        self.x_u8 = x_view if x_view is not None else torch.empty(N, H, W, 3, dtype=torch.uint8, device=self.dev)
        b0 = 0
        for sub in self.subs:
            sub._ensure_u8(sub._batch[0], H, W, self.x_u8[b0:b0 + sub._batch[0]], self.lut_dev)
            b0 += sub._batch[0]
        if not self.subs:
            self._ops_u8 = self._write(u8=True)

    def forward_uint8(self, x_u8, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
        """uint8 NHWC images [N,H,W,3] (decoder output, after resize / crop) -> fp32 logits; bit for bit what ``self(normalised
        fp32 NCHW tensor)`` returns for the tensor the reference's data pipeline would have built (ToTensor + Normalize + the input
        QuantAct are one table look-up, ``hawq_amd.quant_utils.input_quant_lut``)."""
        if not x_u8.is_cuda or x_u8.dtype != torch.uint8 or x_u8.dim() != 4 or x_u8.shape[3] != 3:
            raise ValueError("expected a uint8 NHWC [N,H,W,3] tensor on the MI355X")
        return self._forward_uint8(x_u8, mean, std)

    def _upload_lut(self, mean, std):   # (this engine's kernels read the table flat)
        self.lut_dev.copy_(input_quant_lut(self.P['inv_s_in'], mean, std).reshape(-1).to(self.dev), non_blocking=False)

    def tap(self, name):
        """int32 / int8 NHWC tensor of a tapped stage as an NCHW int64 numpy array without the padding channels."""
        t, shp, c = self.taps[name]
        a = t.cpu().numpy().reshape(shp).astype(np.int64)[..., :c]
        return a.transpose(0, 3, 1, 2)
