"""Float ResNet skeletons with the attribute tree HAWQ's quantized graphs dereference.

The reference builds its float model with ``pytorchcv.model_provider.get_model``
(quant_train.py:227,233) and then walks ``features.init_block.conv.{conv,bn}``,
``features.stageN.unitM.{resize_identity, body.conv1..3.{conv,bn}, identity_conv.{conv,bn}}``
and ``output`` (utils/models/q_resnet.py:22-51, 84-112, 206-229, 270-289).
pytorchcv is not installable here, so this module provides stand-ins with exactly that
attribute tree.  ``resnet50`` puts the stride on the first 1x1 conv of a bottleneck
(pytorchcv ``conv1_stride=True``), ``resnet50b`` on the 3x3.

Only shapes/names matter: weights come from a checkpoint or from ``init_synthetic``.
"""
from __future__ import annotations

import torch
import torch.nn as nn

ARCH = {
    #            units per stage, stage widths,            bottleneck, stride on conv1
    "resnet18": ((2, 2, 2, 2), (64, 128, 256, 512), False, True),
    "resnet50": ((3, 4, 6, 3), (256, 512, 1024, 2048), True, True),
    "resnet50b": ((3, 4, 6, 3), (256, 512, 1024, 2048), True, False),
    "resnet101": ((3, 4, 23, 3), (256, 512, 1024, 2048), True, True),
}


def _conv_bn(cin, cout, k, stride, pad):
    blk = nn.Module()
    blk.conv = nn.Conv2d(cin, cout, k, stride, pad, bias=False)
    blk.bn = nn.BatchNorm2d(cout)
    return blk


def _unit(cin, cout, stride, bottleneck, conv1_stride):
    u = nn.Module()
    u.resize_identity = (cin != cout) or (stride != 1)
    u.body = nn.Module()
    if bottleneck:
        mid = cout // 4
        s1, s2 = (stride, 1) if conv1_stride else (1, stride)
        u.body.conv1 = _conv_bn(cin, mid, 1, s1, 0)
        u.body.conv2 = _conv_bn(mid, mid, 3, s2, 1)
        u.body.conv3 = _conv_bn(mid, cout, 1, 1, 0)
    else:
        u.body.conv1 = _conv_bn(cin, cout, 3, stride, 1)
        u.body.conv2 = _conv_bn(cout, cout, 3, 1, 1)
    if u.resize_identity:
        u.identity_conv = _conv_bn(cin, cout, 1, stride, 0)
    return u


def build_float_resnet(arch: str, num_classes: int = 1000) -> nn.Module:
    units, widths, bottleneck, conv1_stride = ARCH[arch]
    net = nn.Module()
    net.arch = arch
    net.features = nn.Module()
    net.features.init_block = nn.Module()
    net.features.init_block.conv = _conv_bn(3, 64, 7, 2, 3)
    cin = 64
    for si, (n, w) in enumerate(zip(units, widths)):
        stage = nn.Module()
        for ui in range(n):
            stride = 2 if (ui == 0 and si > 0) else 1
            setattr(stage, f"unit{ui + 1}", _unit(cin, w, stride, bottleneck, conv1_stride))
            cin = w
        setattr(net.features, f"stage{si + 1}", stage)
    net.output = nn.Linear(cin, num_classes)
    return net


def build_float_mobilenetv2(num_classes: int = 1000) -> nn.Module:
    """pytorchcv ``mobilenetv2_w1`` attribute tree as utils/models/q_mobilenetv2.py:120-172 dereferences it:
    ``features.init_block.{conv,bn}`` (3x3/2, 3->32), ``features.stageN.unitM.{conv1,conv2,conv3}.{conv,bn}`` (1x1 expand x6 -
    x1 in the very first unit -, 3x3 depthwise, 1x1 linear projection), ``features.final_block.{conv,bn}`` (1x1 320->1280),
    ``features.final_pool`` (AvgPool2d(7)), ``output`` (1x1 conv, no bias)."""
    layers, downsample, widths = [1, 2, 3, 4, 3, 3, 1], [0, 1, 1, 1, 0, 1, 0], [16, 24, 32, 64, 96, 160, 320]
    channels = [[]]
    for c, n, d in zip(widths, layers, downsample):   # q_get_mobilenetv2's grouping (q_mobilenetv2.py:224-233)
        if d:
            channels.append([c] * n)
        else:
            channels[-1] += [c] * n
    net = nn.Module()
    net.arch = "mobilenetv2_w1"
    net.features = nn.Module()
    net.features.init_block = _conv_bn(3, 32, 3, 2, 1)
    cin = 32
    for si, per_stage in enumerate(channels):
        stage = nn.Module()
        for ui, cout in enumerate(per_stage):
            stride = 2 if (ui == 0 and si != 0) else 1
            mid = cin * 6 if (si != 0 or ui != 0) else cin
            u = nn.Module()
            u.conv1 = _conv_bn(cin, mid, 1, 1, 0)
            u.conv2 = _conv_bn(mid, mid, 3, stride, 1)
            u.conv2.conv = nn.Conv2d(mid, mid, 3, stride, 1, groups=mid, bias=False)
            u.conv3 = _conv_bn(mid, cout, 1, 1, 0)
            setattr(stage, f"unit{ui + 1}", u)
            cin = cout
        setattr(net.features, f"stage{si + 1}", stage)
    net.features.final_block = _conv_bn(cin, 1280, 1, 1, 0)
    net.features.final_pool = nn.AvgPool2d(kernel_size=7, stride=1)
    net.output = nn.Conv2d(1280, num_classes, 1, bias=False)
    net.channels = channels
    return net


def init_synthetic(net: nn.Module, seed: int = 0) -> nn.Module:
    """Deterministic synthetic weights (no zoo checkpoints are reachable here).

    Conv/linear keep PyTorch's default init drawn under ``manual_seed(seed)``; BN
    statistics are randomised so that BN folding (quant_modules.py:441-449) is not a
    no-op: running_mean~N(0,.1), running_var~U(.5,1.5), weight~U(.5,1.5), bias~N(0,.1).
    Module construction order fixes the RNG stream, so the same seed gives the same
    tensors in every process that uses the same torch build.
    """
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                fan_in = m.weight[0].numel()
                bound = (1.0 / fan_in) ** 0.5
                m.weight.copy_((torch.rand(m.weight.shape, generator=g) * 2 - 1) * bound)
                if m.bias is not None:
                    m.bias.copy_((torch.rand(m.bias.shape, generator=g) * 2 - 1) * bound)
            elif isinstance(m, nn.BatchNorm2d):
                c = m.num_features
                m.running_mean.copy_(torch.randn(c, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(c, generator=g) + 0.5)
                m.weight.copy_(torch.rand(c, generator=g) + 0.5)
                m.bias.copy_(torch.randn(c, generator=g) * 0.1)
    return net


def synthetic_images(batch: int, seed: int = 0, size: int = 224) -> torch.Tensor:
    """Normalised-image-like synthetic input: seeded N(0,1)."""
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randn(batch, 3, size, size, generator=g)


# InceptionV3 (pytorchcv ``inceptionv3``): per unit kind, the branches in registration order.  A branch is ("conv1x1", out),
# ("seq", [(out, kernel, stride, padding), ...]), ("seq3x3", [...]) - a sequence followed by parallel 1x3 / 3x1 convs -,
# ("avgpool", out) or ("maxpool",).  Kernels / paddings are int or (h, w).
INCEPTION_STAGES = [[256, 288, 288], [768, 768, 768, 768, 768], [1280, 2048, 2048]]
INCEPTION_B_MID = [128, 160, 160, 192]


def inception_unit_branches(kind: str, out_channels: int, mid: int = 0):
    """Branches of one InceptionV3 unit (the structure utils/models/q_inceptionv3.py:327-572 dereferences)."""
    if kind == "A":
        return [("conv1x1", 64), ("seq", [(48, 1, 1, 0), (64, 5, 1, 2)]),
                ("seq", [(64, 1, 1, 0), (96, 3, 1, 1), (96, 3, 1, 1)]), ("avgpool", out_channels - 224)]
    if kind == "RA":
        return [("seq", [(384, 3, 2, 0)]), ("seq", [(64, 1, 1, 0), (96, 3, 1, 1), (96, 3, 2, 0)]), ("maxpool",)]
    if kind == "B":
        return [("conv1x1", 192),
                ("seq", [(mid, 1, 1, 0), (mid, (1, 7), 1, (0, 3)), (192, (7, 1), 1, (3, 0))]),
                ("seq", [(mid, 1, 1, 0), (mid, (7, 1), 1, (3, 0)), (mid, (1, 7), 1, (0, 3)), (mid, (7, 1), 1, (3, 0)),
                         (192, (1, 7), 1, (0, 3))]),
                ("avgpool", 192)]
    if kind == "RB":
        return [("seq", [(192, 1, 1, 0), (320, 3, 2, 0)]),
                ("seq", [(192, 1, 1, 0), (192, (1, 7), 1, (0, 3)), (192, (7, 1), 1, (3, 0)), (192, 3, 2, 0)]), ("maxpool",)]
    if kind == "C":
        return [("conv1x1", 320), ("seq3x3", [(384, 1, 1, 0)]), ("seq3x3", [(448, 1, 1, 0), (384, 3, 1, 1)]), ("avgpool", 192)]
    raise KeyError(kind)


def inception_units():
    """(stage, unit, kind, in_channels, out_channels, mid) of every InceptionV3 unit in order."""
    cin, out = 192, []
    for si, per_stage in enumerate(INCEPTION_STAGES):
        for ui, cout in enumerate(per_stage):
            kind = ("RA", "RB")[si - 1] if (ui == 0 and si > 0) else ("A", "B", "C")[si]
            mid = INCEPTION_B_MID[ui - 1] if kind == "B" else 0
            out.append((si + 1, ui + 1, kind, cin, cout, mid))
            cin = cout
    return out


def _incept_conv(cin, cout, k, stride, pad):
    blk = nn.Module()
    blk.conv = nn.Conv2d(cin, cout, k, stride, pad, bias=False)
    blk.bn = nn.BatchNorm2d(cout, eps=1e-3)
    blk.activ = nn.ReLU(inplace=True)
    return blk


def build_float_inceptionv3(num_classes: int = 1000) -> nn.Module:
    """pytorchcv ``inceptionv3`` attribute tree as utils/models/q_inceptionv3.py dereferences it:
    ``features.init_block.conv1..conv5``, ``features.stageN.unitM.branches.branchK`` with ``conv`` (1x1 and average-pool
    branches, the latter also ``pool``), ``conv_list.convI`` (sequences) and ``conv1x3`` / ``conv3x1`` (Inception-C), each conv
    a ``{conv, bn}`` block; ``features.final_pool`` (AvgPool2d(8)), ``output.fc``.  Input 299 x 299."""
    net = nn.Module()
    net.arch = "inceptionv3"
    net.features = nn.Module()
    ib = nn.Module()
    for i, (cin, cout, k, s, p) in enumerate(((3, 32, 3, 2, 0), (32, 32, 3, 1, 0), (32, 64, 3, 1, 1))):
        setattr(ib, f"conv{i + 1}", _incept_conv(cin, cout, k, s, p))
    ib.pool1 = nn.MaxPool2d(3, 2)
    ib.conv4 = _incept_conv(64, 80, 1, 1, 0)
    ib.conv5 = _incept_conv(80, 192, 3, 1, 0)
    ib.pool2 = nn.MaxPool2d(3, 2)
    net.features.init_block = ib
    for si, ui, kind, cin, cout, mid in inception_units():
        if ui == 1:
            setattr(net.features, f"stage{si}", nn.Module())
        unit = nn.Module()
        unit.branches = nn.Module()
        for bi, br in enumerate(inception_unit_branches(kind, cout, mid)):
            b = nn.Module()
            if br[0] == "conv1x1":
                b.conv = _incept_conv(cin, br[1], 1, 1, 0)
            elif br[0] in ("seq", "seq3x3"):
                b.conv_list = nn.Module()
                c = cin
                for i, (co, k, s, p) in enumerate(br[1]):
                    setattr(b.conv_list, f"conv{i + 1}", _incept_conv(c, co, k, s, p))
                    c = co
                if br[0] == "seq3x3":
                    b.conv1x3 = _incept_conv(c, c, (1, 3), 1, (0, 1))
                    b.conv3x1 = _incept_conv(c, c, (3, 1), 1, (1, 0))
            elif br[0] == "avgpool":
                b.pool = nn.AvgPool2d(3, 1, 1)
                b.conv = _incept_conv(cin, br[1], 1, 1, 0)
            else:
                b.pool = nn.MaxPool2d(3, 2)
            setattr(unit.branches, f"branch{bi + 1}", b)
        setattr(getattr(net.features, f"stage{si}"), f"unit{ui}", unit)
    net.features.final_pool = nn.AvgPool2d(8, 1)
    net.output = nn.Module()
    net.output.dropout = nn.Dropout(0.5)
    net.output.fc = nn.Linear(2048, num_classes)
    return net


class EngineOwner:
    """What the three quantised networks share in keeping their fused executor (each model's ``engine()`` builds it into
    ``self._engine``): dropping it when it has gone stale."""

    def invalidate_engine(self):
        self._engine = None

    def _on_state_dict_loaded(self):
        """load_state_dict brought new float parameters / ranges: the cached plan is stale, and so is any trust in integer
        buffers loaded earlier from a quantized checkpoint (hawq_amd.api.load_quantized_checkpoint sets it again itself)."""
        from .quant_modules import trust_integer_buffers
        self.invalidate_engine()
        trust_integer_buffers(self, False)
        if getattr(self, "engine_defaults", None):
            self.engine_defaults = dict(self.engine_defaults, from_buffers=False)

