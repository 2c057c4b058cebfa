"""Quantised InceptionV3 over the drop-in modules, built from the float network's own tree.

Mirrors utils/models/q_inceptionv3.py of the reference: the same class names, attribute names, registration order and
``(tensor, scale)`` tuple convention, so ``state_dict`` keys and the ``bit_config_inceptionv3_*`` schedules (bit_config.py)
line up with the reference's checkpoints.  The branch structure comes from ``hawq_amd.skeleton.inception_unit_branches``.

Dataflow of one unit (quant_modules.py:205-305):
* every branch opens with ``q_input_act``, which requantises the unit's 16-bit tensor to the branch's own scale;
* ``Q_InceptConv`` = conv + BN -> ReLU -> ``QuantAct`` (case 0); the last one of a branch produces 16-bit values;
* ``Q_Concurrent`` concatenates the branch outputs and returns ``(tensor, [branch scales], [branch widths])``; the unit's
  ``q_rescaling_activ`` then requantises each channel slice from its branch's scale to the unit scale (the list path of
  QuantAct).  Inception-C's 3x3 branches hold such a concat of their own (1x3 and 3x1 convs).

Execution: a frozen, eval-mode network called on a CUDA tensor runs the FUSED INTEGER PLAN of
``hawq_amd.engine_inception.InceptionEngine`` (int16 unit tensors, int8 branch tensors, one hipGraph per batch shape).
Otherwise (un-frozen = range calibration, or ``fused = False``) it steps module by module through the HIP library in the
reference's fp32-tuple convention (convs on ``hawq_incep_conv``, the 3x3 average pools on ``hawq_avgpool3x3_f32``, every
QuantAct on ``hawq_fixedpoint_f32``).  CPU tensors raise.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .quant_modules import QuantAct, QuantAveragePool2d, QuantBnConv2d, QuantDropout, QuantLinear, QuantMaxPool2d
from .skeleton import EngineOwner, inception_unit_branches, inception_units


class Q_InceptConv(nn.Module):
    """conv + BN -> ReLU -> QuantAct (q_inceptionv3.py:16-57)."""

    def __init__(self, model):
        super().__init__()
        self.q_convbn = QuantBnConv2d()
        self.q_convbn.set_param(model.conv, model.bn)
        self.q_convbn.incep_conv = True   # InceptionV3 windows / paddings: the rectangular conv kernel
        self.relu = nn.ReLU(inplace=True)
        self.q_activ = QuantAct()

    def forward(self, x):
        a_sf = x[1]
        x, w_sf = self.q_convbn(x)
        return self.q_activ(torch.relu(x), a_sf, w_sf, None, None)


class Q_Concurrent(nn.Sequential):
    """Runs every branch on the same input and concatenates along channels (q_inceptionv3.py:84-120)."""

    def __init__(self, axis=1, stack=False):
        super().__init__()
        self.axis, self.stack = axis, stack

    def forward(self, x):
        outs, scales, widths = [], [], []
        for branch in self._modules.values():
            y, s = branch(x)
            outs.append(y), scales.append(s), widths.append(y.shape[1])
        out = torch.stack(outs, dim=self.axis) if self.stack else torch.cat(outs, dim=self.axis)
        return out, scales, widths


class Q_MaxPoolBranch(nn.Module):
    """q_input_act (16 bit) -> max 3x3 / 2 (q_inceptionv3.py:123-138)."""

    def __init__(self):
        super().__init__()
        self.q_input_act = QuantAct()
        self.q_pool = QuantMaxPool2d(kernel_size=3, stride=2, padding=0)

    def forward(self, x):
        return self.q_pool(self.q_input_act(x))


class Q_AvgPoolBranch(nn.Module):
    """q_input_act (16 bit) -> average 3x3 / 1 / pad 1 -> q_pool_act -> 1x1 conv (q_inceptionv3.py:141-176)."""

    def __init__(self, model):
        super().__init__()
        self.q_input_act = QuantAct()
        self.q_pool = QuantAveragePool2d(kernel_size=3, stride=1, padding=1)
        self.q_pool_act = QuantAct()
        self.q_conv = Q_InceptConv(model.conv)

    def forward(self, x):
        return self.q_conv(self.q_pool_act(self.q_pool(self.q_input_act(x))))


class Q_Conv1x1Branch(nn.Module):
    """q_input_act -> 1x1 conv (q_inceptionv3.py:179-206)."""

    def __init__(self, model):
        super().__init__()
        self.q_input_act = QuantAct()
        self.q_conv = Q_InceptConv(model.conv)

    def forward(self, x):
        return self.q_conv(self.q_input_act(x))


class Q_ConvSeqBranch(nn.Module):
    """q_input_act -> a sequence of convs (q_inceptionv3.py:209-257)."""

    def __init__(self, model):
        super().__init__()
        self.q_input_act = QuantAct()
        self.q_conv_list = nn.Sequential()
        i = 1
        while hasattr(model.conv_list, f"conv{i}"):
            self.q_conv_list.add_module(f"q_conv{i}", Q_InceptConv(getattr(model.conv_list, f"conv{i}")))
            i += 1

    def forward(self, x):
        return self.q_conv_list(self.q_input_act(x))


class Q_ConvSeq3x3Branch(Q_ConvSeqBranch):
    """A sequence, then parallel 1x3 and 3x1 convs joined by a concat requant (q_inceptionv3.py:260-324)."""

    def __init__(self, model):
        super().__init__(model)
        self.q_conv1x3 = Q_InceptConv(model.conv1x3)
        self.q_conv3x1 = Q_InceptConv(model.conv3x1)
        self.q_rescaling_activ = QuantAct()

    def forward(self, x):
        x = super().forward(x)
        y1, s1 = self.q_conv1x3(x)
        y2, s2 = self.q_conv3x1(x)
        return self.q_rescaling_activ((torch.cat((y1, y2), dim=1), [s1, s2], [y1.shape[1], y2.shape[1]]))


_BRANCH = {"conv1x1": Q_Conv1x1Branch, "seq": Q_ConvSeqBranch, "seq3x3": Q_ConvSeq3x3Branch, "avgpool": Q_AvgPoolBranch}


class Q_InceptionUnit(nn.Module):
    """Branches + concat requant: the common form of the five unit classes below (q_inceptionv3.py:327-572), whose only
    differences are their branch tables."""
    kind = ""

    def __init__(self, model, in_channels, out_channels, mid_channels=0):
        super().__init__()
        self.branches = Q_Concurrent()
        for bi, br in enumerate(inception_unit_branches(self.kind, out_channels, mid_channels)):
            fb = getattr(model.branches, f"branch{bi + 1}")
            self.branches.add_module(f"branch{bi + 1}", Q_MaxPoolBranch() if br[0] == "maxpool" else _BRANCH[br[0]](fb))
        self.q_rescaling_activ = QuantAct()

    def forward(self, x):
        return self.q_rescaling_activ(self.branches(x))


class Q_InceptionAUnit(Q_InceptionUnit):
    kind = "A"


class Q_ReductionAUnit(Q_InceptionUnit):
    kind = "RA"


class Q_InceptionBUnit(Q_InceptionUnit):
    kind = "B"


class Q_ReductionBUnit(Q_InceptionUnit):
    kind = "RB"


class Q_InceptionCUnit(Q_InceptionUnit):
    kind = "C"


_UNIT = {c.kind: c for c in (Q_InceptionAUnit, Q_ReductionAUnit, Q_InceptionBUnit, Q_ReductionBUnit, Q_InceptionCUnit)}


class Q_InceptInitBlock(nn.Module):
    """Stem (q_inceptionv3.py:575-649): input QuantAct, conv1 3x3/2, conv2 3x3, conv3 3x3 pad 1, max pool, conv4 1x1,
    conv5 3x3, max pool."""

    def __init__(self, model):
        super().__init__()
        self.q_input_activ = QuantAct()
        self.q_conv1 = Q_InceptConv(model.conv1)
        self.q_conv2 = Q_InceptConv(model.conv2)
        self.q_conv3 = Q_InceptConv(model.conv3)
        self.q_pool1 = QuantMaxPool2d(kernel_size=3, stride=2, padding=0)
        self.q_conv4 = Q_InceptConv(model.conv4)
        self.q_conv5 = Q_InceptConv(model.conv5)
        self.q_pool2 = QuantMaxPool2d(kernel_size=3, stride=2, padding=0)

    def forward(self, x):
        x = self.q_input_activ(x)
        for m in (self.q_conv1, self.q_conv2, self.q_conv3, self.q_pool1, self.q_conv4, self.q_conv5, self.q_pool2):
            x = m(x)
        return x


class Q_InceptionV3(EngineOwner, nn.Module):
    """Quantised mirror of a pytorchcv-style float InceptionV3 (q_inceptionv3.py:652-744)."""

    def __init__(self, model, dropout_rate=0.5, in_size=(299, 299), num_classes=1000):
        super().__init__()
        self.in_size, self.num_classes = in_size, num_classes
        self.features = nn.Sequential()
        self.features.add_module("q_init_block", Q_InceptInitBlock(model.features.init_block))
        for si, ui, kind, cin, cout, mid in inception_units():
            if ui == 1:
                self.features.add_module(f"stage{si}", nn.Sequential())
            fu = getattr(getattr(model.features, f"stage{si}"), f"unit{ui}")
            getattr(self.features, f"stage{si}").add_module(f"unit{ui}", _UNIT[kind](fu, cin, cout, mid))
        self.features.add_module("q_final_pool", QuantAveragePool2d(kernel_size=8, stride=1))
        self.features.add_module("q_concat_activ", QuantAct())
        self.output = nn.Sequential()
        self.output.add_module("q_dropout", QuantDropout(p=dropout_rate))
        q_fc = QuantLinear()
        q_fc.set_param(model.output.fc)
        self.output.add_module("q_fc", q_fc)
        self.fused = True          # use the integer plan when frozen + eval + CUDA
        self._engine = None
        self.register_load_state_dict_post_hook(lambda module, incompatible_keys: module._on_state_dict_loaded())

    def units(self):
        for si, ui, *_ in inception_units():
            yield f"features.stage{si}.unit{ui}", getattr(getattr(self.features, f"stage{si}"), f"unit{ui}")

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("hawq_amd.Q_InceptionV3: the input must live on the MI355X (no CPU path exists)")
        if self.fused and not self.training and self.is_frozen():
            return self.engine()(x)
        return self.forward_modules(x)

    def forward_modules(self, x):
        """Module-by-module forward (q_inceptionv3.py:740-744)."""
        x, a_sf = self.features(x)
        return self.output((x.view(x.size(0), -1), a_sf))

    def is_frozen(self):
        acts = [m for m in self.modules() if isinstance(m, QuantAct)]
        convs = [m for m in self.modules() if isinstance(m, (QuantBnConv2d, QuantLinear))]
        return all((not m.running_stat) for m in acts) and all(m.fix_flag for m in convs)

    def engine(self, **kw):
        """Build (or return the cached) fused integer plan of this frozen network (hawq_amd/engine_inception.py)."""
        from .engine_inception import InceptionEngine
        if self._engine is None or kw:
            self._engine = InceptionEngine(self, **kw)
        return self._engine


def q_inceptionv3(model):
    """Entry point named like the reference's (q_inceptionv3.py:747-786), for the float network it is given."""
    return Q_InceptionV3(model)
