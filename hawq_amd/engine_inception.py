"""Fused integer plan of a frozen Q_InceptionV3 (hawq_amd/q_inceptionv3.py): one plan per batch shape, captured once into a
hipGraph and replayed (hawq_amd/runner.py).

Buffers are NHWC integers: int16 for the unit tensors (the 16-bit ``q_rescaling_activ`` outputs) and int8 for everything a
conv reads (every conv input of the schedules is at most 8 bits; 4-bit values travel in int8 containers).  Per unit, the
branches launch one after another on the plan's stream:
* conv branches: ``hawq_incep_requant`` (the branch's ``q_input_act``, int16 -> int8), then one ``hawq_incep_conv`` per conv
  (REQUANT: ReLU + the conv's ``q_activ``); the branch's last conv uses REQUANT2, whose second requant is the unit's concat
  rescale (branch scale -> unit scale, quant_modules.py:275-286), and writes its channel slice of the unit buffer in place;
* Inception-C's 3x3 branches: the 1x3 / 3x1 convs write their REQUANT2 results (conv scale -> the branch's inner concat scale)
  into an int16 buffer of their own, and ``hawq_incep_requant`` rescales it into the unit buffer;
* average-pool branches: ``hawq_incep_avgpool_branch`` (16-bit ``q_input_act``, 3x3 sum, trunc rule, ``q_pool_act``) -> int8,
  then the 1x1 conv as above;
* max-pool branches: ``hawq_incep_maxpool3s2`` (16-bit ``q_input_act``, max, concat rescale) into the unit buffer.
Stem: the input QuantAct (``hawq_fakequant_f32`` + ``hawq_f32_nchw_to_q_nhwc``; under ``fused_stem`` one launch with conv1),
five convs, two max pools.  Head: ``hawq_incep_global_avgpool`` (8 x 8 trunc rule + ``q_concat_activ``), the classifier as a 1x1
RAW conv and ``hawq_acc_nhwc_to_f32_nchw`` (fp32 logits = (acc + bias) * fl(S_w * S_a), quant_modules.py:125-130).
uint8 images (``forward_uint8``): the same plan and buffers with its first three launches (input QuantAct + conv1) replaced by one
``hawq_incep_stem_u8``, whose table look-up is ToTensor + Normalize + the input QuantAct (``input_quant_lut``); a graph of its own.

Every requant is the exact dyadic form of fixedpoint_fn (``requant_table(..., lift=False)``).

Mechanism.  ``_build`` emits one ``Launch`` record per launch of that default plan, in its order (``_launches``: 147 records, the
input QuantAct's two launches and conv1 among the stem's), and nothing rewrites the list afterwards.  What ``tune``, ``plan=`` or
the defaults decide is one value (``_choose``): the tile id per conv launch or None, the grouped launches or None, and the fan-out
boundaries or None.  One writer
(``_write``) turns records + choice + the engine's options into the callables of a chain (``_ops``, ``_ops_u8``): it picks the entry
point of every record, the stem that heads the chain and, with groups, the order (``grouped_order``, a pure function).

Conv tiles.  By default every conv launch (94 convs + the classifier) is ``hawq_incep_conv``.  ``InceptionEngine(model, tune=True)``
times, once the buffers of a batch shape exist and before the graph is captured, every conv launch on its own buffers with tile 0
(that kernel) and with every LDS-tiled kernel of ``hawq_incep_conv_tiled`` that ``hawq_incep_conv_tile_ok`` accepts (HIP events,
``_TUNE_WARMUP`` untimed + ``_TUNE_REPS`` timed launches, the median: ``EventTimer.median_us``), keeps the fastest id per launch and
issues ``hawq_incep_conv_tiled`` with it; launch list, order, stream and buffers are those of the default plan, and every tile
computes the same integers, so the result is bit-identical.  The uint8 plan shares the choice (its stem kernel replaces conv1).
``export_plan()`` returns the choice as a JSON-serialisable dict (``make_plan``); ``InceptionEngine(model, plan=p)`` replays it
without timing anything and raises ``plan.StalePlan`` when it does not fit (``check_plan``: another launch list, tile inventory
or batch shape, or a tile the library now refuses).

Pool kernels.  By default the 49 pool / requant launches are the four entry points named above.  ``InceptionEngine(model,
fast_pools=True)`` issues every one of them that ``hawq_incep_pool_v_ok`` accepts as ``hawq_incep_pool_v`` with the op id of its entry
point instead (``pool_launches``): the vectorised kernels of hawq_amd/csrc/incep_pool.hip on the same argument block, buffers and
stream, which write the same bytes - launch list and results are unchanged.  The choice is an engine argument, not part of a plan:
it composes with ``tune`` and ``plan``.

Fused fp32 stem.  ``InceptionEngine(model, fused_stem=True)`` replaces the fp32 plan's first three launches (``hawq_fakequant_f32``,
``hawq_f32_nchw_to_q_nhwc``, conv1) by one ``hawq_incep_stem_f32`` on ``x_in`` (hawq_amd/csrc/incep_stem_f32.hip), the fp32 twin of the
uint8 stem kernel: the same bytes in conv1's output buffer, 145 launches instead of 147, and neither the fake-quantised fp32 copy nor
the 16-channel int8 image is allocated (the input QuantAct's two records carry NULL for them and are never issued).  A model whose
input QuantAct or conv1 the kernel cannot take raises ``PlanNotApplicable`` (``_stem_refusal``, ``hawq_incep_stem_f32_ok``) - there is
no fall-back to the three launches.  ``conv_launches`` keeps conv1's key, so plans are interchangeable between engines with and
without the option; a fused-stem plan carries conv1's tile id and ignores it, as the uint8 plan does, and ``tune=True`` does not
time conv1 (its entry records tile 0 and no times).  An engine argument like ``fast_pools``, composing with every other one.

Grouped conv launches.  ``InceptionEngine(model, grouped=True)`` issues the sibling convs at one depth of a unit's branches
(``conv_levels``) as ONE ``hawq_incep_conv_group`` launch (hawq_amd/csrc/incep_group.hip): members keep their argument blocks, buffers
and output slices, only the grid is shared, and the launch writes the bytes the single launches write.  A grouped unit issues its
level-0 records first (branch-input requants, the average pool, the max-pool branch), then level 1, level 2, ...; the inner-concat
requant of an 8 x 8 unit follows the level that holds its 1x3 / 3x1 pair (``grouped_order``).  Every launch owns its output buffer,
so the order across branches is free.  A level of one conv stays a single launch: 27 grouped launches holding 74 convs and 21
single ones instead of 95, ``n_launches`` 100 instead of 147.  ``conv_launches`` keeps the default plan's order, so tile plans cross
over between engines with and without the option.  Which levels are grouped, and on which tile (one id in 1 .. T for a whole group):
* neither ``tune`` nor ``plan``: every level of two or more convs on tile 3 if ``hawq_incep_conv_group_ok`` takes it, else singles;
* ``tune=True``: after the per-conv timing every such level is timed on every tile the group accepts (the same method and buffers)
  and kept with its fastest tile only if that beats the sum of its members' best single times (``group_candidates`` has both);
* ``plan=``: the ``"groups"`` entries of the plan (``check_groups``), none if it has no such field; no timing launch.
``export_plan()`` of a grouped engine writes ``"groups"``; an engine without ``grouped`` ignores the field.  ``group_launches`` lists
(member conv indices, tile) per grouped launch in launch order.  Not the default.

Fan-out epilogues.  Every conv branch of a unit starts with a ``hawq_incep_requant`` of the previous unit's whole 16-bit concat
buffer (31 launches per forward).  ``InceptionEngine(model, fan_out=True)`` lets the convs that wrote that buffer store the int8
copies themselves: ``hawq_incep_conv_group_fan`` (hawq_amd/csrc/incep_fan.hip), the grouped launch whose epilogue requantises the
value it has just stored once more per consumer and stores it into the consumer's buffer.  The records stay the default plan's;
``fan_boundaries`` (a pure function over tags and argument blocks) finds, per unit, its entry requants, which slices of their input a
conv of the previous unit produced (REQUANT2 into that buffer) and, per producer, the fan targets - each entry requant's output,
pitch and ``post`` table at the producer's channels.  A boundary with at least one conv-produced slice is a candidate (units 1 - 10;
unit 0 reads the stem's max pool).  For a chosen boundary the writer issues its producer launches - single convs as groups of one,
grouped launches with their members' fans - through the fan entry point and drops the entry requants, or, where a pool or an
inner-concat requant produced part of the input (units 4, 9, 10), issues them on those channel ranges only (``in_off`` / ``c_off`` /
``C`` of a fresh block; adjacent ranges merged): 128 launches instead of 147, 81 instead of 100 with ``grouped``.  Which boundaries:
* neither ``tune`` nor a ``"fan_out"`` field in ``plan``: every candidate whose producer launches the library takes, each on tile 3 or
  else the first of 2, 1, 4 that ``hawq_incep_conv_group_fan_ok`` accepts (a tile plan without the field fixes the other convs only);
* ``tune=True``: per boundary two blocks of launches are timed on the real buffers - its producers as the rest of the choice issues
  them followed by its entry requants, and the fan-out producers (each on the fastest tile it accepts) followed by the residual
  requants - and the boundary is kept only if the second block is faster (``fan_candidates`` has both times);
* ``plan=`` with the field: exactly its entries (``check_fan_out``: StalePlan for a unit that is no candidate, launches other than
  the boundary's producer launches, a refused tile); an empty list means none.  No timing launch.
``export_plan()`` of a fan-out engine writes ``"fan_out": [{"unit", "tiles": {producer launch: tile}, "us"}]``; an engine without
``fan_out`` ignores the field.  ``fan_launches`` lists (unit, member conv indices, tile) per fan-out launch, ``residual_requants``
(unit, record, in_off, C) per shortened entry requant.  Pool kernels, inner-concat requants, stem and head are untouched.  Not the
default: at batch 1 - 16 the longer epilogue costs more than the launches it saves.

Nibble operands.  ``InceptionEngine(model, nibble=True)`` stores 4-bit tensors and weights hawq4 and runs the convs that read them on
``hawq_incep_conv_nib`` (hawq_amd/csrc/incep_nib.hip): the launch list keeps its length and order, the integers are the default plan's.
``nibble_storage`` (a pure function) decides per tensor a conv reads: hawq4 if its values lie in 0 .. 15 (a 4-bit QuantAct behind a
ReLU, or fed by such values through requants with m >= 0: ``_T.rng``), its producer can write nibbles - a branch-entry requant, issued
as ``hawq_incep_pool_v`` with ``out_bits`` 4, or a conv that itself runs on the nibble kernel - and every conv that reads it is a
4-bit x 4-bit conv the kernel takes; int8 otherwise (pool outputs, the stem, 8-bit layers).  A conv runs on the nibble kernel, on
hawq4 weights, exactly when the tensor it reads is hawq4; the int8 form of such a tensor or weight is not kept.  Which convs:
* neither ``tune`` nor ``plan``: every conv the policy allows, each on the first tile of ``_NIB_TILES`` the library takes;
* ``tune=True``: after the int8 tiles every such conv is timed on every nibble tile it accepts, on the buffers of a forward of the
  all-nibble plan, and counts as a nibble conv only if its fastest nibble tile beats its fastest int8 tile; the policy then runs
  again, so a tensor falls back to int8 if any of its consumers does (``nibble_us`` has the times);
* ``plan=`` with a ``"nibble"`` field: exactly its (conv, tile) pairs, StalePlan if the policy would not store those tensors or the
  library refuses a tile; a plan without the field takes the untuned choice; an engine without ``nibble`` ignores the field.
``nibble_convs`` maps conv launch -> nibble tile, ``nibble_tensors`` lists the hawq4 tensors, ``nibble_bytes`` the conv operand bytes
(weights, activations) in int8 containers and in this plan.  It composes with ``fast_pools``, ``fused_stem`` and ``forward_uint8``;
with ``grouped`` or ``fan_out``, and on a model without such a conv (uniform8), it raises ``PlanNotApplicable``.  Not the default.

Mixed-form groups.  ``InceptionEngine(model, nibble=True, nibble_groups=True)`` issues the conv levels of a nibble plan as
``hawq_incep_conv_group_nib`` launches (hawq_amd/csrc/incep_group_nib.hip): the grouped launch whose members are int8 or hawq4 one
by one, a bit mask saying which.  ``grouped`` names the int8 launch and still does not compose with ``nibble``; ``nibble_groups``
without ``nibble`` raises ``PlanNotApplicable``.  The nibble choice is made first, exactly as without the option; then every level
of two or more convs becomes one launch, a nibble conv on its hawq4 block and every other member on its own block, members with the
most K steps first (K / 64 int8, K / 128 hawq4: free, and unmeasured).  Which levels, and on which of the launch's two tiles:
* neither ``tune`` nor a ``"nibble_groups"`` field in ``plan``: every level the library takes on tile 2 (128 px x 64 ch), in
  ``grouped_order`` - the launch count of a ``grouped`` engine;
* ``tune=True``: after the nibble choice every candidate level is timed on both tiles, on the buffers of a forward of the chosen
  nibble plan, and kept on the faster one only if that beats the sum of its members' chosen single launches (best int8 tile or best
  nibble tile);
* ``plan=`` with the field: exactly its entries (``check_groups``: StalePlan for an entry that is not a level, overlaps another or is
  refused); ``export_plan()`` writes ``"nibble_groups": [{"convs", "tile", "us"}]``; an engine without the option ignores it.
``group_launches`` lists (member conv indices, tile) per launch and ``nibble_group_masks`` the mask of each (bit k: member k is
hawq4).  It composes with ``fast_pools``, ``fused_stem``, ``forward_uint8``, ``tune`` and ``plan``.  Not the default.

Fan-out epilogues on a nibble plan.  ``InceptionEngine(model, nibble=True, nibble_fan=True)`` folds the entry requants of a nibble plan
into the convs that wrote the concat buffer, as ``fan_out`` does on an int8 plan, through ``hawq_incep_conv_group_nib_fan``
(hawq_amd/csrc/incep_fan_nib.hip): the mixed-form grouped launch whose members store every fan output as int8 or as hawq4 rows, one
``fan_mask`` bit per output.  ``fan_out`` names the int8 launch and still does not compose with ``nibble``; ``nibble_fan`` without
``nibble`` raises ``PlanNotApplicable``.  The nibble choice and the group choice are made first, exactly as without the option; then
``fan_boundaries(launches, issued)`` reads the boundaries with every entry requant as the nibble plan issues it (``out_bits`` 4 into
its own hawq4 buffer, or the int8 record), so that a fan target carries that block's buffer, clamp and form (``"forms"``).  Residual
channel ranges (units 4, 9, 10) stay with the entry requants, shortened; a boundary whose hawq4 entry requant ``hawq_incep_pool_v``
does not take on such a range is no candidate.  A producer launch is a level of ``nibble_groups`` with its members' fans, or a single
conv as a group of one (its mask bit set if it is a nibble conv).  Which boundaries, and on which of the launch's two tiles:
* neither ``tune`` nor a ``"nibble_fan"`` field in ``plan``: every candidate the library takes, each producer launch on tile 2, else 1;
* ``tune=True``: per boundary the two blocks ``fan_out`` times, on the buffers of a forward of the chosen nibble plan - its producer
  launches and entry requants as that plan issues them against the fan launches and the residual requants - kept only if the second
  is faster;
* ``plan=`` with the field: exactly its entries (``check_fan_out`` with the new check); ``export_plan()`` writes ``"nibble_fan":
  [{"unit", "tiles", "us"}]``; an engine without the option ignores it.
``fan_launches`` and ``residual_requants`` report as for ``fan_out``, ``nibble_fan_masks`` lists the ``fan_mask`` of each fan launch
beside ``nibble_group_masks``.  It composes with ``nibble_groups``, ``fast_pools``, ``fused_stem``, ``forward_uint8``, ``tune`` and
``plan``.  Not the default (DESIGN.md 10.3 has what the tuner keeps).

Split-K launches.  ``InceptionEngine(model, grouped=True, splitk=...)`` lets conv launches with few workgroups (batch 1 - 16) run as
``hawq_incep_conv_group_splitk`` (hawq_amd/csrc/incep_splitk.hip): the grouped launch on 128 px x 64 ch tiles whose members' K loops
are cut into slices, one workgroup each; the bytes written are the grouped launch's.  Candidates are the conv launches the grouped
plan issues behind conv1 - a grouped level, a single conv as a group of one, the classifier; records, order and ``n_launches`` stay,
a split launch takes the place of the launch it replaces.  Which launches, with which slice counts (one per member, 1 = uncut):
* ``splitk=True``, neither ``tune`` nor ``plan``: a launch of W workgroups (on 128 x 64 tiles) with W < CUs gets S_max = the largest power
  of two <= min(16, CUs // W) and per member ``split_slices(steps, S_max)`` - at least two K steps a slice, no empty slice; a launch
  left with all ones, or refused by ``hawq_incep_conv_group_splitk_ok``, stays as it is;
* ``splitk=n`` (n >= 2): the same with S_max = n for every candidate, whatever W;
* ``tune=True``: after tiles and groups every candidate with W < CUs is timed as the plan issues it and with S_max in 2, 4, 8, 16 (the
  method and buffers of the group timing) and kept on its fastest count only if that beats the plain launch (``splitk_candidates``
  lists convs, slices, times and ``kept``);
* ``plan=``: exactly the entries of its ``"splitk"`` field, StalePlan for one that is no issued launch of this plan or that the
  library refuses; a plan without the field splits nothing; an engine without the option ignores the field.
``export_plan()`` writes ``"splitk": [{"convs", "slices", "us"}]`` only when some launch is split.  ``splitk_launches`` lists (member
conv indices, slices) per split launch.  One slab and one zeroed counter buffer serve all of them (``_split_workspace``).  Without
``grouped`` (and without the nibble form below), or with ``fan_out`` or ``nibble_fan``, it raises ``PlanNotApplicable``; it composes
with ``fast_pools``, ``fused_stem``, ``forward_uint8``, ``tune``, ``plan`` and ``use_graph``.  Not the default: untuned it is slower
than the grouped plan.
``InceptionEngine(model, nibble=True, nibble_groups=True, splitk=...)`` is the same option on a nibble plan: the split launch is
``hawq_incep_conv_group_nib_splitk`` (hawq_amd/csrc/incep_group_nib_splitk.hip) on mixed-group tile 2, whose members are int8 or
hawq4 one by one as in ``hawq_incep_conv_group_nib``; the bytes written are that launch's.  The nibble choice and the group choice
are made first, exactly as without the option.  Candidates are the launches that plan issues behind conv1 - a mixed-form level with
its mask, a single conv as a group of one (mask 1 if it is a nibble conv), the classifier - and a member's K steps count 64-byte
rows of its own form: K / 64 int8, K / 128 hawq4, so a hawq4 member has half the steps to cut.  W, S_max, ``split_slices``, the
timing (against ``hawq_incep_conv_group_nib``, ``hawq_incep_conv_nib`` or ``hawq_incep_conv_tiled``, whichever the plan issues), the
``"splitk"`` field and its StalePlan rules are as above; which kernel an entry means follows from the plan's own ``"nibble"`` and
``"nibble_groups"`` fields.  ``nibble=True`` without ``nibble_groups`` has no split form and raises ``PlanNotApplicable``.

Band kernel for the stem.  ``InceptionEngine(model, stem_band=True)`` runs the stem's 3x3 / stride 1 convs (conv2, conv3, conv5) on
``hawq_incep_conv_band`` (hawq_amd/csrc/incep_band.hip), which stages a band's input halo in LDS once instead of gathering every tap
from global memory; same argument block, same bytes.  A candidate is a conv record of the stem that ``hawq_incep_conv_band_ok``
accepts (conv1 is stride 2; under ``fused_stem`` it is not launched at all).  Records, kinds, ``conv_launches`` and the launch digest
stay: only the entry point of the chosen records changes.  Which candidates:
* neither ``tune`` nor ``plan``: all of them;
* ``tune=True``: each is timed on the band kernel next to its tiles (the same method and buffers) and kept only where the band beats
  the chosen tile - a tie goes to the tile (``stem_band_us``: conv -> microseconds);
* ``plan=``: exactly the conv indices of its ``"stem_band"`` field (``check_stem_band``: StalePlan for an entry that is no candidate,
  is named twice or that the library refuses); a plan without the field runs no band launch.
``export_plan()`` writes ``"stem_band"`` (and ``"stem_band_us"``) only when the option is on; an engine without it ignores them.
``stem_band_convs`` lists the kept conv indices.  A record that the plan runs as a split-K launch keeps that launch.  The stem is
int8 under every other option, so this one composes with all of them.  The units' 3x3 convs are not candidates (their choice
interacts with the groups).  Not the default.

Conv + max pool in one launch for the stem.  ``InceptionEngine(model, stem_pool=True)`` issues a stem conv whose dense output only
the ``hawq_incep_maxpool3s2`` record behind it reads (no ``pre`` / ``post``; ``stem_pool_pairs``: conv3 + pool1 and conv5 + pool2,
conv indices 2 and 4) as one ``hawq_incep_conv_band_pool`` (hawq_amd/csrc/incep_band_pool.hip) on a copy of the conv's block whose
``out`` / ``ldo`` / ``c_off`` are the pool's: the full-resolution tensor is never written.  The records stay; ``_write`` issues the
launch in the conv's place and nothing in the pool's, so ``n_launches`` drops by one per pair (``pool_launches`` names the fused
launch for such a pool).  The conv's buffer stays allocated (the tuner and the two-launch form use it).  Which pairs:
* neither ``tune`` nor ``plan``: every candidate ``hawq_incep_conv_band_pool_ok`` accepts;
* ``tune=True``: last of all choices, the pair as the plan issues it (conv on its chosen tile or band launch, then the pool on the
  entry point ``fast_pools`` selects) is timed as a block against the fused launch, which is kept only where it is faster - a tie
  goes to the pair (``stem_pool_us``: conv -> [pair, fused] microseconds);
* ``plan=``: exactly the conv indices of its ``"stem_pool"`` field (``check_stem_pool``: StalePlan for an entry that is no
  candidate, is named twice or that the library refuses); a plan without the field fuses nothing.
``export_plan()`` writes ``"stem_pool"`` and ``"stem_pool_us"`` only when the option is on; an engine without it ignores them.
``stem_pool_convs`` lists the kept convs; ``stem_band_convs`` leaves them out (the pooled launch wins).  A conv that the plan runs
as a split-K launch keeps that launch and its pool.  No candidate at all raises ``PlanNotApplicable``.  Not the default.

Average pool + 1x1 conv in one launch.  ``InceptionEngine(model, pool_conv=True)`` issues an average-pool branch - the
``hawq_incep_avgpool_branch`` record and the 1x1 conv record behind it, the only reader of its dense int8 output
(``pool_conv_pairs``: nine, one per Inception-A, -B and -C unit) - as one ``hawq_incep_avgpool_conv`` (hawq_amd/csrc/incep_pool_conv.hip)
on the two records' own blocks.  The records stay; ``_write`` issues the launch in the conv's place and nothing in the pool's, so
``n_launches`` drops by one per pair - not under ``grouped``, where the conv was a member of its level's launch and the fused
launch takes the pool's slot; the int8 intermediate stays allocated (the tuner and the two-launch form use it).  Which pairs:
* neither ``tune`` nor ``plan``: every candidate ``hawq_incep_avgpool_conv_ok`` accepts;
* ``tune=True``: after tiles and groups and before the fans, two blocks are timed per candidate on the buffers of a forward - the
  pool (on the entry point ``fast_pools`` selects) followed by the unit's level-1 conv launch as the choice issues it (a group, or the
  conv alone), against the fused launch followed by that level without the conv - and the pair is fused only where the second block
  is faster; a tie goes to the two launches (``pool_conv_us``: conv -> [two launches, fused] microseconds);
* ``plan=``: exactly the conv indices of its ``"pool_conv"`` field (``check_pool_conv``: StalePlan for an entry that is no candidate,
  is named twice or that the library refuses); a plan without the field fuses nothing.
``export_plan()`` writes ``"pool_conv"`` and ``"pool_conv_us"`` only when the option is on; an engine without it ignores them.
Under ``grouped`` a fused conv leaves its level before the level is issued: the rest keeps the level's tile if the library takes
the smaller group and runs as single launches otherwise (the plan's ``"groups"`` still name whole levels).  Under ``fan_out`` a
fused conv does not fan out: its slice of the unit buffer is one of the boundary's residual ranges (``fan_boundaries(...,
unfanned)``).  ``pool_conv_convs`` lists the fused convs.  With ``nibble``, ``nibble_groups``, ``nibble_fan`` or ``splitk`` it raises
``PlanNotApplicable`` (the kernel has no nibble or split form).  Not the default.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import json
from functools import partial
from itertools import groupby

import numpy as np
import torch

from . import _lib
from .plan import StalePlan
from .quant_modules import QuantAct
from .quant_utils import requant_table
from .runner import EventTimer, GraphRunner, _rng


class PlanNotApplicable(RuntimeError):
    pass


def _pad16(c):
    return (c + 15) // 16 * 16


def _scale(act: QuantAct):
    if getattr(act, "use_integer_buffers", False):
        return act.act_scaling_factor.detach().reshape(-1)[:1].float().cpu()
    return act.compute_scale().detach().reshape(-1)[:1].float().cpu()


def _scalar_table(s_in, s_out):
    m, ek = requant_table(s_in, torch.ones(1), s_out, lift=False)
    return int(m[0]), int(ek[0])


def pack_stem_u8_weights(w_int, cout_p):
    """int8 [Cout][3][3][3] conv1 weights -> the [cout_p][32] rows of ``hawq_incep_stem_u8``: k = (kh * 3 + kw) * 3 + c for
    k < 27, zeros for k = 27 .. 31 and for rows Cout .. cout_p - 1."""
    co = w_int.shape[0]
    w = np.zeros((cout_p, 32), np.int8)
    w[:co, :27] = np.asarray(w_int, np.int8).transpose(0, 2, 3, 1).reshape(co, 27)
    return w


# ---------------------------------------------------------------------- conv tile plans (pure functions: no device, no library)
_KEY_FIELDS = ("H", "W", "Cin", "Cout", "KH", "KW", "stride", "pad_h", "pad_w", "epilogue", "out_bits", "ldo", "c_off")
_TUNE_WARMUP, _TUNE_REPS = 2, 5


def launch_key(a):
    """what identifies a conv launch in a plan: geometry, epilogue, out_bits, ldo, c_off of its argument block (not the batch)"""
    return tuple(int(getattr(a, f)) for f in _KEY_FIELDS)


def launch_digest(keys):
    """sha256 over the conv launch list (``launch_key`` tuples, in launch order)"""
    return hashlib.sha256(json.dumps([list(map(int, k)) for k in keys], separators=(",", ":")).encode()).hexdigest()


def make_plan(batch, keys, num_tiles, tiles, us, groups=None, fan_out=None, nibble=None, nibble_groups=None, nibble_fan=None,
              splitk=None, stem_band=None, stem_pool=None, pool_conv=None):
    """the dict ``export_plan`` returns: batch shape (N, H, W), digest of the launch list, tile inventory, chosen id per conv launch
    and, for the record, the measured microseconds per launch and tile id (``us[i][str(tile)]``); with `groups` (a grouped engine's
    ``{"convs": [indices into the launch list], "tile": id, "us": {...}}`` entries) also the ``"groups"`` field, and with `fan_out`
    (a fan-out engine's ``{"unit": k, "tiles": {launch: id}, "us": {...}}`` entries) the ``"fan_out"`` field; `nibble_groups`
    (entries as `groups`, tile ids of ``hawq_incep_conv_group_nib``) the ``"nibble_groups"`` field; `nibble_fan` (entries as
    `fan_out`, tile ids of ``hawq_incep_conv_group_nib_fan``) the ``"nibble_fan"`` field; a non-empty `splitk` (a split-K engine's
    ``{"convs", "slices": [per member], "us"}`` entries) the ``"splitk"`` field; `stem_band` (a stem-band engine's (kept conv
    indices, conv -> microseconds on the band kernel)) the ``"stem_band"`` and ``"stem_band_us"`` fields; `stem_pool` (a stem-pool
    engine's (kept conv indices, conv -> [pair, fused] microseconds)) the ``"stem_pool"`` and ``"stem_pool_us"`` fields; `pool_conv`
    (a pool-conv engine's (fused conv indices, conv -> [two launches, fused] microseconds)) ``"pool_conv"`` and ``"pool_conv_us"``"""
    plan = {"network": "inceptionv3", "batch": [int(v) for v in batch], "launches": launch_digest(keys), "n_launches": len(keys),
            "num_tiles": int(num_tiles), "tiles": [int(t) for t in tiles],
            "us": [{str(t): round(float(v), 3) for t, v in sorted(d.items(), key=lambda kv: int(kv[0]))} for d in us]}
    if groups is not None:
        plan["groups"] = [{"convs": [int(c) for c in g["convs"]], "tile": int(g["tile"]),
                           "us": {str(k): round(float(v), 3) for k, v in g.get("us", {}).items()}} for g in groups]
    for field, fans in (("fan_out", fan_out), ("nibble_fan", nibble_fan)):
        if fans is not None:
            plan[field] = [{"unit": int(f["unit"]), "tiles": {str(k): int(t) for k, t in f["tiles"].items()},
                            "us": {str(k): round(float(v), 3) for k, v in f.get("us", {}).items()}} for f in fans]
    if nibble is not None:   # a nibble engine's (conv -> nibble tile, conv -> {tile: microseconds})
        plan["nibble"] = [[int(c), int(t)] for c, t in sorted(nibble[0].items())]
        plan["nibble_us"] = {str(c): {str(t): round(float(v), 3) for t, v in d.items()} for c, d in sorted(nibble[1].items())}
    if nibble_groups is not None:
        plan["nibble_groups"] = [{"convs": [int(c) for c in g["convs"]], "tile": int(g["tile"]),
                                  "us": {str(k): round(float(v), 3) for k, v in g.get("us", {}).items()}} for g in nibble_groups]
    if splitk:   # only when some launch is split
        plan["splitk"] = [{"convs": [int(c) for c in e["convs"]], "slices": [int(s) for s in e["slices"]],
                           "us": {str(k): round(float(v), 3) for k, v in e.get("us", {}).items()}} for e in splitk]
    if stem_band is not None:
        plan["stem_band"] = sorted(int(c) for c in stem_band[0])
        plan["stem_band_us"] = {str(c): round(float(v), 3) for c, v in sorted(stem_band[1].items())}
    if stem_pool is not None:
        plan["stem_pool"] = sorted(int(c) for c in stem_pool[0])
        plan["stem_pool_us"] = {str(c): [round(float(v), 3) for v in us] for c, us in sorted(stem_pool[1].items())}
    if pool_conv is not None:
        plan["pool_conv"] = sorted(int(c) for c in pool_conv[0])
        plan["pool_conv_us"] = {str(c): [round(float(v), 3) for v in us] for c, us in sorted(pool_conv[1].items())}
    return plan


def check_plan(plan, batch, keys, num_tiles, ok):
    """The tile ids of `plan` for the conv launches `keys` at batch shape `batch`, or StalePlan when the plan was recorded for
    another batch shape, launch list or tile inventory, or names a tile that ``ok(i, tile)`` (launch index, tile id) refuses."""
    try:
        p_batch, p_digest, p_tiles, p_num = list(plan["batch"]), plan["launches"], list(plan["tiles"]), plan["num_tiles"]
    except (KeyError, TypeError) as exc:
        raise StalePlan(f"not an InceptionV3 conv tile plan: {exc!r}") from exc
    if p_batch != [int(v) for v in batch]:
        raise StalePlan(f"plan recorded for batch shape {p_batch}, not {list(batch)}")
    if p_num != num_tiles:
        raise StalePlan(f"plan recorded with {p_num} conv tiles; this library has {num_tiles}")
    if p_digest != launch_digest(keys) or len(p_tiles) != len(keys):
        raise StalePlan("plan recorded for another conv launch list")
    for i, t in enumerate(p_tiles):
        if not isinstance(t, int) or isinstance(t, bool) or not 0 <= t <= num_tiles or not ok(i, t):
            raise StalePlan(f"conv launch {i} {tuple(keys[i])}: tile {t!r} is refused")
    return p_tiles


def check_stem_band(entries, candidates, ok):
    """The conv launches of a plan's ``"stem_band"`` field (None: no such field, no band launch), or StalePlan: not a list, an
    entry that is not one of `candidates` (the stem's conv launches, as indices into the conv launch list), one named twice, or
    one that ``ok(i)`` refuses."""
    if entries is None:
        return []
    if not isinstance(entries, (list, tuple)):
        raise StalePlan(f"not a list of stem conv launches: {entries!r}")
    for i, c in enumerate(entries):
        if not isinstance(c, int) or isinstance(c, bool) or c not in candidates:
            raise StalePlan(f"stem band launch {c!r}: not a conv launch of the stem")
        if c in entries[:i]:
            raise StalePlan(f"stem band launch {c}: named twice")
        if not ok(c):
            raise StalePlan(f"stem band launch {c}: the band kernel refuses it")
    return list(entries)


def stem_pool_pairs(records):
    """conv index -> (conv record, pool record) of every stem conv + max pool pair that one ``hawq_incep_conv_band_pool`` launch
    can stand for: a conv record of the stem that writes a dense tensor which the ``hawq_incep_maxpool3s2`` record behind it reads
    whole, in the same container and without ``pre`` / ``post`` tables, and which no other record reads."""
    def reads(q, ptr):
        return q.args[0].in_ == ptr if q.kind in ("conv", "pool") else ptr in q.args

    pairs = {}
    for r, p in zip(records, records[1:]):
        if r.kind != "conv" or r.place != "stem" or p.kind != "pool" or p.name != "hawq_incep_maxpool3s2":
            continue
        a, b = r.args[0], p.args[0]
        dense = a.c_off == 0 and a.ldo == a.Cout and b.in_off == 0 and b.in_pitch == a.ldo and b.C == a.Cout
        if dense and b.in_ == a.out and not b.pre and not b.post and b.in_bits == a.out_bits == b.out_bits and \
                not any(reads(q, a.out) for q in records if q is not p):
            pairs[r.ref] = (r, p)
    return pairs


def check_stem_pool(entries, candidates, ok):
    """The stem convs of a plan's ``"stem_pool"`` field (None: no such field, no fused launch), or StalePlan: not a list, an entry
    that is not one of `candidates` (``stem_pool_pairs``, as indices into the conv launch list), one named twice, or one that
    ``ok(i)`` refuses."""
    if entries is None:
        return []
    if not isinstance(entries, (list, tuple)):
        raise StalePlan(f"not a list of stem conv launches: {entries!r}")
    for i, c in enumerate(entries):
        if not isinstance(c, int) or isinstance(c, bool) or c not in candidates:
            raise StalePlan(f"stem pool launch {c!r}: not a stem conv that only a max pool reads")
        if c in entries[:i]:
            raise StalePlan(f"stem pool launch {c}: named twice")
        if not ok(c):
            raise StalePlan(f"stem pool launch {c}: the fused kernel refuses it")
    return list(entries)


def pool_conv_pairs(records):
    """conv index -> (pool record, conv record) of every average-pool branch that one ``hawq_incep_avgpool_conv`` launch can stand
    for: a ``hawq_incep_avgpool_branch`` record that writes a dense int8 tensor which the 1x1 conv record behind it reads whole, and
    which no other record reads."""
    def reads(q, ptr):
        return q.args[0].in_ == ptr if q.kind in ("conv", "pool") else ptr in q.args

    pairs = {}
    for p, r in zip(records, records[1:]):
        if p.kind != "pool" or p.name != "hawq_incep_avgpool_branch" or r.kind != "conv":
            continue
        a, b = p.args[0], r.args[0]
        dense = a.c_off == 0 and a.ldo == a.C == b.Cin and a.out_bits == 8 and (b.N, b.H, b.W) == (a.N, a.H, a.W)
        if dense and b.in_ == a.out and (b.KH, b.KW) == (1, 1) and not any(reads(q, a.out) for q in records if q is not r):
            pairs[r.ref] = (p, r)
    return pairs


def check_pool_conv(entries, candidates, ok):
    """The convs of a plan's ``"pool_conv"`` field (None: no such field, no fused launch), or StalePlan: not a list, an entry that
    is not one of `candidates` (``pool_conv_pairs``, as indices into the conv launch list), one named twice, or one that ``ok(i)``
    refuses."""
    if entries is None:
        return []
    if not isinstance(entries, (list, tuple)):
        raise StalePlan(f"not a list of pool-branch conv launches: {entries!r}")
    for i, c in enumerate(entries):
        if not isinstance(c, int) or isinstance(c, bool) or c not in candidates:
            raise StalePlan(f"pool conv launch {c!r}: not a 1x1 conv that alone reads an average-pool branch")
        if c in entries[:i]:
            raise StalePlan(f"pool conv launch {c}: named twice")
        if not ok(c):
            raise StalePlan(f"pool conv launch {c}: the fused kernel refuses it")
    return list(entries)


def unit_convs(unit):
    """the Q_InceptConv modules of a unit in the default plan's launch order (branch by branch), each with (branch, depth): depth d
    is the conv's place in its branch, from 1; the 1x3 / 3x1 pair of a Q_ConvSeq3x3Branch shares the depth after its last sequential
    conv; the conv of a pool branch has depth 1"""
    out = []
    for bi, br in enumerate(unit.branches.children()):
        seq = list(br.q_conv_list) if hasattr(br, "q_conv_list") else ([br.q_conv] if hasattr(br, "q_conv") else [])
        out += [(ic, bi, d + 1) for d, ic in enumerate(seq)]
        if hasattr(br, "q_conv1x3"):
            out += [(br.q_conv1x3, bi, len(seq) + 1), (br.q_conv3x1, bi, len(seq) + 1)]
    return out


def conv_levels(unit):
    """The conv levels of a unit: ``levels[d - 1]`` lists the convs at depth d of their branch as indices into ``unit_convs(unit)``
    (ascending).  The convs of one level do not depend on each other; each depends on level d - 1 of its own branch only."""
    levels = []
    for i, (_, _, d) in enumerate(unit_convs(unit)):
        while len(levels) < d:
            levels.append([])
        levels[d - 1].append(i)
    return levels


def check_groups(groups, n_convs, levels, ok):
    """The grouped launches ``[(conv indices, tile), ...]`` of a plan's ``"groups"`` field (None: no such field, no group), or
    StalePlan: an index outside 0 .. n_convs - 1 or named twice, an entry whose convs are not exactly one of `levels` (one level
    of one unit, as lists of conv indices), or a tile that ``ok(convs, tile)`` refuses."""
    out, seen, whole = [], set(), {frozenset(lv) for lv in levels}
    if groups is None:
        return out
    try:
        entries = [(list(g["convs"]), g["tile"]) for g in groups]
    except (KeyError, TypeError) as exc:
        raise StalePlan(f"not a list of conv groups: {exc!r}") from exc
    for convs, tile in entries:
        for c in convs:
            if not isinstance(c, int) or isinstance(c, bool) or not 0 <= c < n_convs:
                raise StalePlan(f"conv group {convs}: no conv launch {c!r}")
            if c in seen:
                raise StalePlan(f"conv group {convs}: conv launch {c} is named twice")
            seen.add(c)
        if frozenset(convs) not in whole:
            raise StalePlan(f"conv group {convs} is not one level of one unit")
        if not isinstance(tile, int) or isinstance(tile, bool) or not ok(convs, tile):
            raise StalePlan(f"conv group {convs}: tile {tile!r} is refused")
        out.append((convs, tile))
    return out


class Launch:
    """One launch of the default plan: its entry point `name`; `args`, the call's arguments before the stream (for a conv or a pool
    the ctypes block alone); `kind` "conv" (`ref`: its index in the conv list), "pool" (a pool / requant; `ref`: its
    ``hawq_incep_pool_v`` op id) or "other"; `place` "stem", the unit's number or "head"; and its `level` inside a unit: 0 for
    what a branch does before its first conv, d for a conv at depth d, and for an inner-concat requant the level of the 1x3 / 3x1
    pair it follows."""
    __slots__ = ("name", "args", "kind", "ref", "place", "level")

    def __init__(self, name, args, kind="other", ref=None, place="stem", level=0):
        self.name, self.args, self.kind, self.ref, self.place, self.level = name, args, kind, ref, place, level


def grouped_order(launches, groups):
    """The sequence a grouped engine issues: entries (False, i) for record i of `launches` alone and (True, g) for the grouped launch
    g of `groups` = [(member conv indices, tile)], issued once, where its first member is met.  Stem and head stay in place; a unit
    issues its level-0 records in their default order, then its levels in ascending order, each in the default order, an inner-concat
    requant directly after the level of its pair.  Reads the records' tags only."""
    group_of = {c: g for g, (convs, _) in enumerate(groups) for c in convs}
    order, issued = [], set()
    for place, block in groupby(range(len(launches)), key=lambda i: launches[i].place):
        if place not in ("stem", "head"):   # a stable sort: the default order within a level, its convs before its requant
            block = sorted(block, key=lambda i: (launches[i].level, launches[i].kind != "conv"))
        for i in block:
            g = group_of.get(launches[i].ref) if launches[i].kind == "conv" else None
            if g is None:
                order.append((False, i))
            elif g not in issued:
                issued.add(g)
                order.append((True, g))
    return order


def fan_boundaries(launches, issued=None, unfanned=()):
    """The boundary in front of every unit of `launches`, in unit order, read from the records' tags and argument blocks alone
    (`issued`, of a nibble plan: entry requant record -> the block the plan issues in its place, with ``out_bits`` 4 into a hawq4
    buffer of its own; a fan target then carries that block's buffer, clamp and form; `unfanned`: conv records, as indices, whose launch
    has no fan-out form - their slices count as produced by no conv):
    * ``"requants"``: the unit's level-0 ``hawq_incep_requant`` records (the ``q_input_act`` of its conv branches), as indices;
    * ``"slices"``: ``(c_off, C, producer)`` for every slice of the buffer they read that an earlier record writes, by channel: the
      index of the conv record that produced it (REQUANT2, 16 bits, into that buffer), or None for a pool / requant record;
    * ``"producers"``: per such conv record index its fan targets, one per entry requant and in their order:
      ``(out, ldo, (m, ek, lo, hi), c_off, Cout)`` - that record's output buffer, pitch and ``post`` table, and where the producer's
      channels go in it;
    * ``"forms"``: per entry requant the ``out_bits`` it is issued with - 8, or 4 for a block of `issued`;
    * ``"residual"``: the channel ranges ``(in_off, C)`` of the input that no conv produced, adjacent ones merged - what is left for
      the entry requants to do;
    * ``"candidate"``: at least one slice is conv-produced (and the entry requants are plain: one 16-bit source and range, ``post``
      only, int8 out - or hawq4, as `issued`)."""
    out = []
    for k in sorted({r.place for r in launches if isinstance(r.place, int)}):
        entry = [i for i, r in enumerate(launches)
                 if r.place == k and r.level == 0 and r.kind == "pool" and r.name == "hawq_incep_requant"]
        b = {"unit": k, "requants": entry, "slices": [], "producers": {}, "residual": [], "candidate": False, "forms": []}
        out.append(b)
        if not entry:
            continue
        blocks = [(issued or {}).get(launches[i], launches[i].args[0]) for i in entry]
        b["forms"] = [4 if launches[i] in (issued or {}) else 8 for i in entry]
        f = blocks[0]
        src, pitch, lo, hi = f.in_, f.in_pitch, f.in_off, f.in_off + f.C
        plain = all((a.in_, a.in_pitch, a.in_off, a.C, a.in_bits, a.out_bits, a.pre, a.post) == (src, pitch, lo, f.C, 16, bits, 0, 1)
                    for a, bits in zip(blocks, b["forms"]))
        for i, r in enumerate(launches[:entry[0]]):
            if r.kind not in ("conv", "pool"):
                continue
            a = r.args[0]
            if (a.out, a.ldo, a.out_bits) != (src, pitch, 16) or (r.kind == "conv" and a.epilogue == _lib.INCEP_RAW):
                continue
            if r.kind == "conv":
                b["slices"].append((a.c_off, a.Cout, i if a.epilogue == _lib.INCEP_REQUANT2 and i not in unfanned else None))
            else:
                b["slices"].append((a.c_off, a.C, None))
        b["slices"].sort(key=lambda t: t[0])
        at = lo   # the residual: what no conv covers of lo .. hi
        for off, c, prod in [t for t in b["slices"] if t[2] is not None and lo <= t[0] and t[0] + t[1] <= hi] + [(hi, 0, -1)]:
            if off > at:
                b["residual"].append((at, off - at))
            at = max(at, off + c)
            if prod is not None and prod >= 0:
                b["producers"][prod] = [(a.out, a.ldo, (a.m2, a.ek2, a.lo2, a.hi2), a.c_off + off - lo, c) for a in blocks]
        b["candidate"] = plain and bool(b["producers"])
        if not b["candidate"]:
            b["producers"], b["residual"] = {}, [(lo, hi - lo)]
    return out


def fan_key(convs):
    """how a plan's ``"fan_out"`` entry names a producer launch: its member conv indices, in launch order"""
    return ",".join(str(int(c)) for c in convs)


def check_fan_out(entries, candidates, ok):
    """The boundaries ``[(unit, {launch key: tile}), ...]`` of a plan's ``"fan_out"`` field, or StalePlan: an entry that is not
    ``{"unit": k, "tiles": {key: id}}``, a unit that is not in `candidates` (unit -> the ``fan_key`` of every producer launch of its
    boundary) or is named twice, keys other than exactly those launches, or a tile that ``ok(unit, key, tile)`` refuses."""
    out, seen = [], set()
    try:
        pairs = [(e["unit"], dict(e["tiles"])) for e in entries]
    except (KeyError, TypeError, ValueError) as exc:
        raise StalePlan(f"not a list of fan-out boundaries: {exc!r}") from exc
    for unit, tiles in pairs:
        if not isinstance(unit, int) or isinstance(unit, bool) or unit not in candidates:
            raise StalePlan(f"fan-out boundary {unit!r}: not a candidate unit")
        if unit in seen:
            raise StalePlan(f"fan-out boundary {unit}: named twice")
        seen.add(unit)
        if sorted(tiles) != sorted(candidates[unit]):
            raise StalePlan(f"fan-out boundary {unit}: launches {sorted(tiles)} are not its producers {sorted(candidates[unit])}")
        for key, tile in tiles.items():
            if not isinstance(tile, int) or isinstance(tile, bool) or not ok(unit, key, tile):
                raise StalePlan(f"fan-out boundary {unit}, launch {key}: tile {tile!r} is refused")
        out.append((unit, {k: tiles[k] for k in candidates[unit]}))
    return out


_FAN_TILES = (3, 2, 1, 4)   # an untuned fan-out launch: tile 3, else the first of these the library takes
_NIB_FAN_TILES = (2, 1)     # of ``hawq_incep_conv_group_nib_fan``: 128 px x 64 ch, else 128 x 128


def nibble_storage(tensors, conv_ok):
    """The storage policy of a nibble engine, a pure function.  `tensors`: every tensor a conv reads, in the order the plan makes
    them, as ``(lo, hi, producer, consumers)`` - the range of its values, what writes it (``"requant"``: an entry requant, which
    has a hawq4 form; ``("conv", i)``: conv i, which writes nibbles only on the nibble kernel; None: a pool or the image, int8
    only) and the convs that read it; ``conv_ok[i]``: conv i is a 4-bit x 4-bit conv the nibble kernel takes (and, tuned, wins).
    Returns the indices of the tensors stored hawq4: values inside 0 .. 15, a producer that can write nibbles, and every consumer
    such a conv; every other tensor is int8.  A conv runs on the nibble kernel exactly when the tensor it reads is hawq4."""
    src_of = {c: t for t, (_, _, _, cons) in enumerate(tensors) for c in cons}
    nib = set()
    for t, (lo, hi, prod, cons) in enumerate(tensors):
        writes = prod == "requant" or (isinstance(prod, tuple) and src_of.get(prod[1]) in nib)
        if lo >= 0 and hi <= 15 and writes and cons and all(conv_ok[c] for c in cons):
            nib.add(t)
    return nib


_NIB_TILES = (2, 1, 3)   # an untuned nibble launch: the first of these the library takes


def split_slices(steps, s_max):
    """The slice count of a member with `steps` K steps (64 bytes each) under the cap `s_max`: the largest S <= min(s_max, steps // 2,
    32) without an empty slice, (S - 1) * ceil(steps / S) < steps - ``hawq_incep_conv_group_splitk_ok``'s rule -, else 1."""
    for s in range(min(s_max, steps // 2, 32), 1, -1):
        if (s - 1) * -(-steps // s) < steps:
            return s
    return 1


class _T:
    """An NHWC integer tensor of the plan: buffer, spatial size, channels, row pitch, scale, container bits; the range `rng` of its
    values where that is known to be narrower than the container, whether they are provably >= 0, and what `nibble_storage` asks:
    the producer and the convs that read it."""

    def __init__(self, buf, h, w, c, pitch, scale, bits, rng=None, nonneg=False, producer=None):
        self.buf, self.h, self.w, self.c, self.pitch, self.scale, self.bits = buf, h, w, c, pitch, scale, bits
        lo, hi = rng or (-(1 << (bits - 1)), (1 << (bits - 1)) - 1)
        self.rng, self.nonneg, self.producer, self.cons = (max(lo, 0) if nonneg else lo, hi), nonneg, producer, []


class InceptionEngine(GraphRunner):
    def __init__(self, model, use_graph: bool = True, tune: bool = False, plan=None, fast_pools: bool = False,
                 fused_stem: bool = False, grouped: bool = False, fan_out: bool = False, nibble: bool = False,
                 nibble_groups: bool = False, nibble_fan: bool = False, splitk=False, stem_band: bool = False,
                 stem_pool: bool = False, pool_conv: bool = False):
        self.model, self.use_graph = model, use_graph
        if not isinstance(splitk, (bool, int)) or (not isinstance(splitk, bool) and splitk < 2):
            raise ValueError("splitk is False, True or a slice count >= 2")
        self.splitk = splitk
        if splitk and not grouped and not (nibble and nibble_groups):
            raise PlanNotApplicable("splitk cuts the launches of a grouped plan: it needs grouped=True, or nibble=True with nibble_groups=True")
        if splitk and (fan_out or nibble_fan):
            raise PlanNotApplicable("splitk does not compose with fan_out or nibble_fan: their launches have no split-K form")
        self.splitk_launches, self.splitk_candidates, self._splits = [], [], {}
        self.tune, self.plan, self.fast_pools, self.fused_stem = bool(tune), plan, bool(fast_pools), bool(fused_stem)
        self.grouped, self.fan_out, self.nibble, self.nibble_groups = bool(grouped), bool(fan_out), bool(nibble), bool(nibble_groups)
        self.nibble_fan, self.stem_band, self.stem_pool = bool(nibble_fan), bool(stem_band), bool(stem_pool)
        self.stem_band_convs, self.stem_band_us, self._bands = [], {}, frozenset()
        self.stem_pool_convs, self.stem_pool_us, self._pooled = [], {}, {}
        self.pool_conv, self.pool_conv_convs, self.pool_conv_us, self._avg_fused = bool(pool_conv), [], {}, {}
        if self.pool_conv and (nibble or nibble_groups or nibble_fan or splitk):
            raise PlanNotApplicable("pool_conv does not compose with nibble, nibble_groups, nibble_fan or splitk: "
                                    "hawq_incep_avgpool_conv has no nibble or split form")
        if self.nibble and (self.grouped or self.fan_out):
            raise PlanNotApplicable("nibble=True does not compose with grouped or fan_out: their launches have no nibble form")
        if self.nibble_groups and not self.nibble:
            raise PlanNotApplicable("nibble_groups=True groups the launches of a nibble plan: it needs nibble=True")
        if self.nibble_fan and not self.nibble:
            raise PlanNotApplicable("nibble_fan=True folds the entry requants of a nibble plan: it needs nibble=True")
        self.nibble_convs, self.nibble_tensors, self.nibble_us, self.nibble_bytes = {}, [], {}, {}
        self.group_launches, self.group_candidates, self.nibble_group_masks, self.nibble_fan_masks = [], [], [], []
        self.fan_launches, self.fan_candidates, self.residual_requants = [], [], []
        self.n_timing_launches = 0           # conv launches issued to time tiles (0 for a default or a replayed plan)
        self.conv_tiles, self.conv_us = None, None
        self.dev = next(model.parameters()).device
        self.stream = None   # created with the first plan: building the engine object needs no device
        self._batch, self._ops, self._ops_u8, self._u8_why = None, [], None, None

    def _zeros(self, *a, **k):
        """a plan buffer: kept alive with the plan (the captured launches hold its address)"""
        t = torch.zeros(*a, **k)
        self._keep.append(t)
        return t

    # ------------------------------------------------------------------ launch records
    def _emit(self, name, args, kind="other", ref=None, level=0):
        """the next record of the default plan, at the place ``_build`` is at"""
        r = Launch(name, args, kind, ref, self._place, level)
        self._launches.append(r)
        if kind == "conv":
            self._convs.append(r)   # the conv list: `ref` is the record's index in it

    def _pool(self, name, src: _T, out_buf, out_bits, ldo, c_off, c, h, w, pre=None, post=None, level=0):
        a = _lib.IncepPoolArgs()
        a.in_, a.out = src.buf.data_ptr(), out_buf.data_ptr()
        a.N, a.H, a.W, a.C = self.N, src.h, src.w, c
        a.in_bits, a.in_pitch, a.in_off = src.bits, src.pitch, 0
        a.out_bits, a.ldo, a.c_off = out_bits, ldo, c_off
        if pre is not None:
            a.pre, (a.m1, a.ek1, a.lo1, a.hi1) = 1, pre
        if post is not None:
            a.post, (a.m2, a.ek2, a.lo2, a.hi2) = 1, post
        self._keep.append(a)
        self._emit(name, (a,), "pool", _lib.INCEP_POOL_OPS[name], level)

    def _conv(self, ic, src: _T, dst=None, c_off=0, second=None, level=0):
        """Q_InceptConv `ic` on `src` (int8): REQUANT into a new buffer, or - `dst`, `second` = (s_out2, act2) - REQUANT2 into the
        channel slice `c_off` of `dst`.  Returns the output tensor (or `dst`)."""
        cb, act = ic.q_convbn, ic.q_activ
        if src.bits != 8:
            raise PlanNotApplicable("a conv input wider than 8 bits")
        if cb.conv.groups != 1 or cb.conv.dilation != (1, 1) or cb.conv.stride[0] != cb.conv.stride[1]:
            raise PlanNotApplicable("grouped, dilated or anisotropic-stride conv")
        s_a = src.scale
        bias_scale = cb.prepare(s_a.to(self.dev))
        w_int = cb.weight_integer.detach().cpu().numpy().astype(np.int8)
        Cout, Cin, KH, KW = w_int.shape
        cin_p, cout_p = src.pitch, _pad16(Cout)
        w = np.zeros((cout_p, KH, KW, cin_p), np.int8)
        w[:Cout, :, :, :Cin] = w_int.transpose(0, 2, 3, 1)
        b = np.zeros(cout_p, np.int32)
        b[:Cout] = cb.bias_integer.detach().cpu().numpy().astype(np.int64).clip(-2 ** 31, 2 ** 31 - 1)
        s_out = _scale(act)
        m, ek = requant_table(s_a, cb.convbn_scaling_factor.detach().reshape(-1).float().cpu(), s_out, lift=False)
        mp, ekp = np.zeros(cout_p, np.int32), np.full(cout_p, 33, np.int32)
        mp[:Cout], ekp[:Cout] = m, ek
        ph, pw = cb.conv.padding
        st = cb.conv.stride[0]
        Ho, Wo = (src.h + 2 * ph - KH) // st + 1, (src.w + 2 * pw - KW) // st + 1
        lo, hi = _rng(act)
        a = _lib.IncepConvArgs()
        if dst is None:
            bits = 8 if act.activation_bit <= 8 else 16
            # ReLU in front of a requant with m >= 0: the values are >= 0 whatever the clamp's lower bound says
            out = _T(self._zeros(self.N * Ho * Wo * cout_p, dtype=torch.int8 if bits == 8 else torch.int16, device=self.dev),
                     Ho, Wo, Cout, cout_p, s_out, bits, rng=(lo, hi), nonneg=True, producer=("conv", len(self._convs)))
            a.epilogue, ldo = _lib.INCEP_REQUANT, cout_p
        else:
            if Cout % 16 or (dst.h, dst.w) != (Ho, Wo):
                raise PlanNotApplicable("concat slice does not fit")
            out = dst
            s2, act2 = second
            a.epilogue, ldo = _lib.INCEP_REQUANT2, dst.pitch
            a.m2, a.ek2 = _scalar_table(s_out, s2)
            a.q2_lo, a.q2_hi = _rng(act2)
            cout_p = Cout
        t = [torch.from_numpy(w).to(self.dev), torch.from_numpy(b).to(self.dev), torch.from_numpy(mp).to(self.dev),
             torch.from_numpy(ekp).to(self.dev)]
        a.in_ = src.buf.data_ptr() if src.buf is not None else None   # None: the fused stem's conv1, which reads x_in
        a.wgt, a.bias, a.out = t[0].data_ptr(), t[1].data_ptr(), out.buf.data_ptr()
        a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW = self.N, src.h, src.w, cin_p, cout_p, KH, KW
        a.stride, a.pad_h, a.pad_w, a.relu = st, ph, pw, 1
        a.m, a.ek, a.q_lo, a.q_hi = t[2].data_ptr(), t[3].data_ptr(), lo, hi
        a.out_bits, a.ldo, a.c_off = out.bits, ldo, c_off
        self._keep += t + [a]
        if src.buf is not None:   # what a nibble engine needs of this conv: the tensors on either side and its integer weights
            if not src.cons:
                self._tensors.append(src)
            src.cons.append(len(self._convs))
            self._conv_io[len(self._convs)] = (src, out if dst is None else None, w if self.nibble else None, t[0])
        self._emit("hawq_incep_conv", (a,), "conv", len(self._convs), level)
        return out

    def _requant_input(self, act, src: _T):
        """a branch's q_input_act of width <= 8: int16 unit tensor -> int8 branch tensor"""
        if act.activation_bit > 8:
            raise PlanNotApplicable("a 16-bit conv-branch input")
        s = _scale(act)
        out = _T(self._zeros(self.N * src.h * src.w * src.pitch, dtype=torch.int8, device=self.dev), src.h, src.w, src.c,
                 src.pitch, s, 8, rng=_rng(act), nonneg=src.nonneg, producer="requant")   # m >= 0: the sign is the source's
        self._pool("hawq_incep_requant", src, out.buf, 8, src.pitch, 0, src.pitch, src.h, src.w,
                   post=(*_scalar_table(src.scale, s), *_rng(act)))
        out.record = self._launches[-1]
        return out

    def _unit(self, unit, src: _T):
        from .q_inceptionv3 import Q_AvgPoolBranch, Q_ConvSeq3x3Branch, Q_MaxPoolBranch
        uact = unit.q_rescaling_activ
        if uact.activation_bit != 16 or uact.quant_mode != "symmetric":
            raise PlanNotApplicable("unit output other than 16-bit symmetric")
        s_u = _scale(uact)
        branches = list(unit.branches.children())
        ucs = unit_convs(unit)   # the one walk over the branches: every conv of the unit with its branch and level
        mine = [[(ic, d) for ic, b, d in ucs if b == bi] for bi in range(len(branches))]
        widths, Ho, Wo = [], None, None
        for br, cs in zip(branches, mine):   # output widths and size of each branch
            if isinstance(br, Q_MaxPoolBranch):
                widths.append(src.c)
                h, w = (src.h - 3) // 2 + 1, (src.w - 3) // 2 + 1
            else:
                pair = 2 if isinstance(br, Q_ConvSeq3x3Branch) else 0   # the 1x3 / 3x1 pair keeps the size and doubles the width
                widths.append(cs[-1][0].q_convbn.conv.out_channels * (2 if pair else 1))
                h, w = src.h, src.w
                for ic, _ in cs[:len(cs) - pair]:
                    k, p, st = ic.q_convbn.conv.kernel_size, ic.q_convbn.conv.padding, ic.q_convbn.conv.stride[0]
                    h, w = (h + 2 * p[0] - k[0]) // st + 1, (w + 2 * p[1] - k[1]) // st + 1
            if Ho is not None and (Ho, Wo) != (h, w):
                raise PlanNotApplicable("branches disagree on the output size")
            Ho, Wo = h, w
        cu = sum(widths)
        if cu % 16 or any(x % 16 for x in widths):
            raise PlanNotApplicable("channel counts must be multiples of 16")
        # every slice is a conv's (ReLU) or a pool's of `src`, requantised with m >= 0
        dst = _T(self._zeros(self.N * Ho * Wo * cu, dtype=torch.int16, device=self.dev), Ho, Wo, cu, cu, s_u, 16, nonneg=src.nonneg)
        off = 0
        for br, wd, cs in zip(branches, widths, mine):
            if isinstance(br, Q_MaxPoolBranch):
                ia = br.q_input_act
                s_b = _scale(ia)
                self._pool("hawq_incep_maxpool3s2", src, dst.buf, 16, cu, off, src.c, src.h, src.w,
                           pre=(*_scalar_table(src.scale, s_b), *_rng(ia)), post=(*_scalar_table(s_b, s_u), *_rng(uact)))
            elif isinstance(br, Q_AvgPoolBranch):
                ia, pa = br.q_input_act, br.q_pool_act
                if pa.activation_bit > 8:
                    raise PlanNotApplicable("a 16-bit q_pool_act")
                s_b, s_p = _scale(ia), _scale(pa)
                t = _T(self._zeros(self.N * src.h * src.w * src.pitch, dtype=torch.int8, device=self.dev), src.h, src.w,
                       src.c, src.pitch, s_p, 8)
                self._pool("hawq_incep_avgpool_branch", src, t.buf, 8, src.pitch, 0, src.c, src.h, src.w,
                           pre=(*_scalar_table(src.scale, s_b), *_rng(ia)), post=(*_scalar_table(s_b, s_p), *_rng(pa)))
                self._conv(cs[0][0], t, dst, off, (s_u, uact), level=cs[0][1])
            else:
                x = self._requant_input(br.q_input_act, src)
                if isinstance(br, Q_ConvSeq3x3Branch):
                    for ic, d in cs[:-2]:
                        x = self._conv(ic, x, level=d)
                    ra = br.q_rescaling_activ
                    s_r = _scale(ra)
                    inner = _T(self._zeros(self.N * Ho * Wo * wd, dtype=torch.int16, device=self.dev), Ho, Wo, wd, wd, s_r, 16)
                    for (ic, d), half in zip(cs[-2:], (0, wd // 2)):
                        self._conv(ic, x, inner, half, (s_r, ra), level=d)
                    self._pool("hawq_incep_requant", inner, dst.buf, 16, cu, off, wd, Ho, Wo,
                               post=(*_scalar_table(s_r, s_u), *_rng(uact)), level=d)   # reads what the pair's level completes
                else:
                    for ic, d in cs[:-1]:
                        x = self._conv(ic, x, level=d)
                    self._conv(cs[-1][0], x, dst, off, (s_u, uact), level=cs[-1][1])
            off += wd
        return dst

    # ------------------------------------------------------------------ plan
    def _build(self, N, H, W):
        self._drop_graph()
        self._batch = None   # until the plan below is complete (a StalePlan leaves no half-built plan behind)
        if self.stream is None:
            self.stream = torch.cuda.Stream(device=self.dev)
        self.N, dev, q = N, self.dev, self.model
        self._launches, self._convs, self._place = [], [], "stem"   # the records, the conv records among them, where `_emit` is
        self._choice = (None, None, None, None)    # the default plan's: no tiles, no groups, no fan-out, no nibbles, the default order
        self._ops, self._keep, self.unit_out = [], [], {}
        self._tensors, self._conv_io = [], {}   # the tensors convs read, in the order they are made; conv -> (src, out, weights)
        self.nibble_convs, self.nibble_tensors, self.nibble_us, self.nibble_bytes = {}, [], {}, {}
        self.conv_tiles, self.conv_us = None, None
        self.group_launches, self.group_candidates, self.nibble_group_masks, self.nibble_fan_masks = [], [], [], []
        self.fan_launches, self.fan_candidates, self.residual_requants = [], [], []
        self.splitk_launches, self.splitk_candidates, self._splits = [], [], {}
        self.stem_band_convs, self.stem_band_us, self._bands = [], {}, frozenset()
        self.stem_pool_convs, self.stem_pool_us, self._pooled = [], {}, {}
        self.pool_conv_convs, self.pool_conv_us, self._avg_fused = [], {}, {}
        ib = q.features.q_init_block
        s_in = _scale(ib.q_input_activ)
        inv, lo, hi = self._input_quant()
        self.x_in = torch.zeros(N, 3, H, W, dtype=torch.float32, device=dev)
        self._stem_a, stem_why = None, self._stem_refusal(ib)
        if self.fused_stem:
            if stem_why is not None:
                raise PlanNotApplicable(f"fused_stem: {stem_why}")
            # conv1's input as the default plan lays it out (that is conv1's launch key); neither buffer of the QuantAct ever exists
            x, xq_p, x_p = _T(None, H, W, 3, 16, s_in, 8), None, None
        else:
            xq_f = torch.zeros_like(self.x_in)
            x = _T(self._zeros(N * H * W * 16, dtype=torch.int8, device=dev), H, W, 3, 16, s_in, 8)
            self._keep += [xq_f]
            xq_p, x_p = xq_f.data_ptr(), x.buf.data_ptr()
        self._emit("hawq_fakequant_f32", (self.x_in.data_ptr(), xq_p, self.x_in.numel(), inv, 1.0, lo, hi))
        self._emit("hawq_f32_nchw_to_q_nhwc", (xq_p, x_p, N, 3, H, W, 16, 8, 1.0))
        for name in ("q_conv1", "q_conv2", "q_conv3", "q_pool1", "q_conv4", "q_conv5", "q_pool2"):
            if name.startswith("q_pool"):
                h, w = (x.h - 3) // 2 + 1, (x.w - 3) // 2 + 1
                y = _T(self._zeros(N * h * w * x.pitch, dtype=x.buf.dtype, device=dev), h, w, x.c, x.pitch, x.scale, x.bits,
                       nonneg=x.nonneg)
                self._pool("hawq_incep_maxpool3s2", x, y.buf, x.bits, x.pitch, 0, x.pitch, x.h, x.w)
                x = y
            else:
                x = self._conv(getattr(ib, name), x)
                if name == "q_conv1" and stem_why is None:   # the records up to here are what a one-launch stem stands for
                    a = self._stem_a = self._stem_args(self._convs[0].args[0], ib.q_conv1.q_convbn.weight_integer)
                    if self.fused_stem and not _lib.load().hawq_incep_stem_f32_ok(self.x_in.data_ptr(), inv, lo, hi, C.byref(a)):
                        raise PlanNotApplicable("fused_stem: hawq_incep_stem_f32 refuses conv1")
        self._ops_u8, self._u8_why = None, stem_why
        if x.bits != 16 or x.pitch != x.c:
            raise PlanNotApplicable("the stem output must be 16-bit")
        for self._place, (uname, unit) in enumerate(q.units()):   # a unit's place is its number
            x = self._unit(unit, x)
            self.unit_out[uname] = x
        self._place = "head"
        ca = q.features.q_concat_activ
        if ca.activation_bit > 8:
            raise PlanNotApplicable("a 16-bit q_concat_activ")
        s_c = _scale(ca)
        feat = _T(self._zeros(N * x.c, dtype=torch.int8, device=dev), 1, 1, x.c, x.c, s_c, 8)
        self._pool("hawq_incep_global_avgpool", x, feat.buf, 8, x.c, 0, x.c, x.h, x.w,
                   post=(*_scalar_table(x.scale, s_c), *_rng(ca)))
        fc = q.output.q_fc
        bias_scale = fc.prepare(s_c.to(dev))
        K, O = fc.in_features, fc.out_features
        op = _pad16(O)
        wf = np.zeros((op, 1, 1, K), np.int8)
        wf[:O, 0, 0, :] = fc.weight_integer.detach().cpu().numpy().astype(np.int8)
        bf = np.zeros(op, np.int32)
        bf[:O] = fc.bias_integer.detach().cpu().numpy().astype(np.int64).clip(-2 ** 31, 2 ** 31 - 1)
        fs = np.zeros(op, np.float32)
        fs[:O] = bias_scale.detach().reshape(-1).cpu().numpy()
        t = [torch.from_numpy(wf).to(dev), torch.from_numpy(bf).to(dev), torch.from_numpy(fs).to(dev)]
        acc = torch.zeros(N * op, dtype=torch.int32, device=dev)
        self.logits = torch.zeros(N, O, dtype=torch.float32, device=dev)
        a = _lib.IncepConvArgs()
        a.in_, a.wgt, a.bias, a.out = feat.buf.data_ptr(), t[0].data_ptr(), t[1].data_ptr(), acc.data_ptr()
        a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.stride = N, 1, 1, K, op, 1, 1, 1
        a.epilogue, a.ldo, a.c_off = _lib.INCEP_RAW, op, 0
        self._keep += t + [a, acc]
        self._emit("hawq_incep_conv", (a,), "conv", len(self._convs))
        self._emit("hawq_acc_nhwc_to_f32_nchw", (acc.data_ptr(), self.logits.data_ptr(), N, O, 1, 1, op, t[2].data_ptr()))
        self._choice = self._choose((N, H, W))
        self._ops = self._write()
        self._batch = (N, H, W)

    # ------------------------------------------------------------------ readers
    @property
    def op_names(self):
        """library entry point of every launch of the fp32 plan, in order"""
        return [op.args[0] for op in self._ops]

    @property
    def conv_launches(self):
        """``launch_key`` of every conv launch (the classifier last), in the default plan's order"""
        return [launch_key(r.args[0]) for r in self._convs]

    @property
    def pool_launches(self):
        """(library entry point, op id of ``hawq_incep_pool_v``) of every pool / requant launch, in the default plan's order"""
        return [(self._ops[self._at[r]].args[0], r.ref) for r in self._launches if r.kind == "pool"]

    @property
    def conv_level_list(self):
        """every conv level of every unit, in unit order, as lists of indices into ``conv_launches``"""
        convs = [r for r in self._convs if r.place not in ("stem", "head")]
        return [[r.ref for r in convs if (r.place, r.level) == k] for k in sorted({(r.place, r.level) for r in convs})]

    @property
    def n_launches(self):
        return len(self._ops)

    @property
    def n_launches_u8(self):
        """launches of the uint8 plan (built by the first ``forward_uint8`` of a batch shape)"""
        return len(self._ops_u8)

    def _tile_ok(self, i, tile):
        if self.fused_stem and i == 0:   # conv1 is not launched: its tile id is carried through a plan, never used
            return True
        return bool(_lib.load().hawq_incep_conv_tile_ok(C.byref(self._convs[i].args[0]), tile))

    def _group_args(self, convs):
        """the argument block of one grouped launch: copies of the members' blocks, in the order of `convs`"""
        g = _lib.IncepGroupArgs()
        g.n = len(convs)
        for k, c in enumerate(convs):
            g.conv[k] = self._convs[c].args[0]
        return g

    def _group_ok(self, convs, tile):
        if not 1 <= len(convs) <= _lib.INCEP_GROUP_MAX or not isinstance(tile, int):
            return False
        return bool(_lib.load().hawq_incep_conv_group_ok(C.byref(self._group_args(convs)), tile))

    def _fan_sets(self, b, groups):
        """the launches that hold the producers of boundary `b` under `groups`, as tuples of member conv indices in launch order: a
        grouped launch with a producer among its members, or the producer alone"""
        sets = []
        for i in sorted(b["producers"]):
            c = self._launches[i].ref
            s = next((tuple(convs) for convs, _ in groups or [] if c in convs), (c,))
            if s not in sets:
                sets.append(s)
        return sets

    def _fan_args(self, convs, b):
        """(group block, fan array) of one fan-out launch: the members' blocks, and per member its targets in boundary `b` (none for
        a member that is no producer); None if a producer has more targets than a fan holds"""
        targets = {self._launches[i].ref: t for i, t in b["producers"].items()}
        g, fans = self._group_args(convs), (_lib.IncepFan * len(convs))()
        for k, c in enumerate(convs):
            ts = targets.get(c, [])
            if len(ts) > _lib.INCEP_FAN_MAX:
                return None
            fans[k].n = len(ts)
            for j, (out, ldo, (m, ek, lo, hi), c_off, _) in enumerate(ts):
                f = fans[k].to[j]
                f.out, f.m, f.ek, f.lo, f.hi, f.ldo, f.c_off = out, m, ek, lo, hi, ldo, c_off
        return g, fans

    def _fan_ok(self, convs, b, tile):
        if not 1 <= len(convs) <= _lib.INCEP_GROUP_MAX or not isinstance(tile, int) or isinstance(tile, bool):
            return False
        gf = self._fan_args(convs, b)
        return gf is not None and bool(_lib.load().hawq_incep_conv_group_fan_ok(C.byref(gf[0]), gf[1], tile))

    def _nfan_args(self, convs, b, nib):
        """(group block, mask, fan array, fan_mask) of one ``hawq_incep_conv_group_nib_fan`` launch: the members as ``_ngroup_args``
        lays them out, their targets in boundary `b` as ``_fan_args`` does, and a ``fan_mask`` bit for every target whose entry
        requant the plan issues hawq4 (``b["forms"]``); None if a producer has more targets than a fan holds"""
        gf = self._fan_args(convs, b)
        if gf is None:
            return None
        g, mask = self._ngroup_args(convs, nib)
        fan_mask = sum(1 << (_lib.INCEP_FAN_MAX * k + j) for k in range(len(convs)) for j in range(gf[1][k].n) if b["forms"][j] == 4)
        return g, mask, gf[1], fan_mask

    def _nfan_ok(self, convs, b, tile, nib):
        if not 1 <= len(convs) <= _lib.INCEP_GROUP_MAX or not isinstance(tile, int) or isinstance(tile, bool):
            return False
        a = self._nfan_args(convs, b, nib)
        return a is not None and bool(_lib.load().hawq_incep_conv_group_nib_fan_ok(C.byref(a[0]), a[1], a[2], a[3], tile))

    def _residual_args(self, r, off, c, block=None):
        """a fresh block for entry requant `r` (`block`: the block a nibble plan issues in its place) on the input channels
        off .. off + c - 1 only"""
        a = _lib.IncepPoolArgs.from_buffer_copy(block or r.args[0])
        a.c_off, a.in_off, a.C = a.c_off + off - a.in_off, off, c
        return a

    # ------------------------------------------------------------------ the choice
    def _choose(self, batch):
        """What a plan decides, as one value: (tile id per conv launch, or None; grouped launches [(member conv indices, tile)], or
        None on an engine without ``grouped`` - the mixed-form launches of a ``nibble_groups`` engine take this place -; fan-out boundaries [(boundary, {producer launch: tile})], or None on an engine
        without ``fan_out`` - those of a ``nibble_fan`` engine take this place -).  From ``self.plan``, else from timing (``tune``), else the defaults: no tiles, every level of two or
        more convs on tile 3 that the library takes, and every candidate boundary whose producer launches the library takes.  Leaves
        ``conv_tiles`` and what was recorded or measured (``conv_us``, ``group_candidates``, ``fan_candidates``) for the readers
        and ``export_plan``."""
        T, tiles, groups = _lib.load().hawq_incep_conv_num_tiles(), None, None
        # members with the longest K loop first, so that the heavy workgroups start first (the order is free, and unmeasured)
        klen = lambda c: -(self._convs[c].args[0].KH * self._convs[c].args[0].KW * self._convs[c].args[0].Cin)   # noqa: E731
        cands = [sorted(lv, key=klen) for lv in self.conv_level_list if len(lv) >= 2] if self.grouped else []
        if self.plan is not None:
            tiles = check_plan(self.plan, batch, self.conv_launches, T, self._tile_ok)
            self.conv_us = [dict(d) for d in self.plan.get("us", [])] or [{} for _ in tiles]
            if self.grouped:
                groups = check_groups(self.plan.get("groups"), len(self._convs), self.conv_level_list, self._group_ok)
                us = {tuple(g["convs"]): dict(g.get("us", {})) for g in self.plan.get("groups") or []}
                self.group_candidates = [{"convs": list(c), "tile": t, "us": us[tuple(c)], "kept": True} for c, t in groups]
        elif self.tune:
            self.conv_us, timed = self._time(T, cands)
            # tile 0 always competes; ties go to the lower id; a conv that was not timed records tile 0
            tiles = [min(d, key=lambda t: (d[t], t)) if d else 0 for d in self.conv_us]
            for c, us in zip(cands, timed):   # a group is kept, on its fastest tile, only if that beats its members' single launches
                if us:
                    tile = min(us, key=lambda t: (us[t], t))
                    singles = sum(self.conv_us[i][tiles[i]] for i in c)
                    self.group_candidates.append({"convs": c, "tile": tile, "kept": us[tile] < singles,
                                                  "us": {**{str(t): v for t, v in us.items()}, "singles": singles}})
            if self.grouped:
                groups = [(g["convs"], g["tile"]) for g in self.group_candidates if g["kept"]]
        elif self.grouped:
            groups = [(c, 3) for c in cands if self._group_ok(c, 3)]
        self.conv_tiles = None if tiles is None else [int(t) for t in tiles]
        if self.stem_band:   # beside the choice, like the splits: the stem convs whose entry point is the band kernel
            self.stem_band_convs = self._choose_bands()
        nib = self._choose_nibbles(T) if self.nibble else None
        if self.nibble_groups:   # the second component then holds the mixed-form launches (``grouped`` is off: the constructor)
            groups = self._choose_nibble_groups(self.conv_tiles, nib)
        avg = {}
        if self.pool_conv:   # in front of the fans: a fused conv is no fan producer, and its level is issued without it
            avg = self._choose_pool_convs(self.conv_tiles, groups)
            self.pool_conv_convs, groups = sorted(avg), self._groups_without(groups, avg)
        unfanned = frozenset(self._launches.index(r) for _, r in avg.values())
        fans = self._choose_fans(self.conv_tiles, groups, nib if self.nibble_fan else None, unfanned) \
            if self.fan_out or self.nibble_fan else None
        self._splits = self._choose_splits(self.conv_tiles, groups, nib) if self.splitk else {}   # beside the choice: launch -> slice counts
        if self.stem_pool:   # last: the pair it competes with is the one the rest of the choice issues
            fused = self._choose_pools(self.conv_tiles, groups, nib)
            self.stem_pool_convs = sorted(fused)
            self.stem_band_convs = [c for c in self.stem_band_convs if c not in fused]   # the pooled launch wins
        self._bands = frozenset(self.stem_band_convs)   # from here on: the timing forwards above ran the default entry points
        self._pooled = fused if self.stem_pool else {}
        self._avg_fused = avg
        return self.conv_tiles, groups, fans, nib

    # ------------------------------------------------------------------ the average-pool branches' pool + conv launches
    def _groups_without(self, groups, gone):
        """`groups` as they are issued once the convs `gone` run elsewhere: a level keeps its tile on the members that are left if
        there are two or more and the library takes the smaller group, and is issued as single launches otherwise"""
        if groups is None:
            return None
        rest = [([c for c in convs if c not in gone], tile, len(convs)) for convs, tile in groups]
        return [(r, tile) for r, tile, n in rest if len(r) == n or (len(r) >= 2 and self._group_ok(r, tile))]

    def _choose_pool_convs(self, tiles, groups):
        """The average-pool branches that run as one ``hawq_incep_avgpool_conv``, as conv index -> (pool record, conv record): the
        plan's ``"pool_conv"`` entries (none without the field), else the candidates whose fused block beat the two-launch block
        (``tune``; ``pool_conv_us``: conv -> [two launches, fused]), else every candidate the library takes."""
        pairs = pool_conv_pairs(self._launches)
        if not pairs:
            raise PlanNotApplicable("pool_conv: no 1x1 conv of this model alone reads an average-pool branch")
        ok = lambda c: bool(_lib.load().hawq_incep_avgpool_conv_ok(C.byref(pairs[c][0].args[0]), C.byref(pairs[c][1].args[0])))   # noqa: E731
        if self.plan is not None:
            self.pool_conv_us = {int(c): [float(v) for v in us] for c, us in (self.plan.get("pool_conv_us") or {}).items()}
            kept = check_pool_conv(self.plan.get("pool_conv"), list(pairs), ok)
        else:
            kept = [c for c in pairs if ok(c)]
            if self.tune and kept:
                self._time_pool_convs(kept, pairs, tiles, groups)
                kept = [c for c in kept if self.pool_conv_us[c][1] < self.pool_conv_us[c][0]]   # a tie goes to the two launches
        return {c: pairs[c] for c in kept}

    def _time_pool_convs(self, cands, pairs, tiles, groups):
        """``pool_conv_us[c]`` = [two launches, fused] in microseconds for every conv of `cands`, each a block timed as a whole on
        the buffers of a forward of the plan: the pool on the entry point ``fast_pools`` selects, then the level-1 launch that holds
        the conv as (tiles, groups) issue it; against the fused launch, then that level without the conv (``_groups_without``)."""
        lib, sp, keep = _lib.load(), self.stream.cuda_stream, []

        def level(c, gs):   # the launches of c's level as the groups `gs` issue them (c alone where no group holds it)
            convs, tile = next(((cv, t) for cv, t in gs or [] if c in cv), ([c], None))
            if tile is not None:
                keep.append(self._group_args(convs))
                return [partial(_lib.call, "hawq_incep_conv_group", C.byref(keep[-1]), int(tile), sp)]
            return [partial(_lib.call, "hawq_incep_conv_tiled", C.byref(self._convs[c].args[0]), int(tiles[c]), sp)]

        self._choice = (tiles, groups, None, None)
        with EventTimer(sp, _TUNE_REPS + 1) as ev:
            torch.cuda.synchronize(self.dev)
            with torch.cuda.stream(self.stream):
                for op in self._write():
                    op()
                for c in cands:
                    p, r = pairs[c]
                    a = C.byref(p.args[0])
                    fast = self.fast_pools and lib.hawq_incep_pool_v_ok(a, p.ref)
                    two = [partial(_lib.call, "hawq_incep_pool_v", a, p.ref, sp) if fast else partial(_lib.call, p.name, a, sp)]
                    two += level(c, groups)
                    one = [partial(_lib.call, "hawq_incep_avgpool_conv", a, C.byref(r.args[0]), sp)]
                    held = [g for g in groups or [] if c in g[0]]   # the rest of the level: a smaller group, or each conv alone
                    smaller = self._groups_without(held, {c})
                    for m in [x for g in held for x in g[0] if x != c][:1 if smaller else None]:
                        one += level(m, smaller)
                    run = lambda ops: [op() for op in ops]   # noqa: E731
                    self.n_timing_launches += (len(two) + len(one)) * (_TUNE_WARMUP + _TUNE_REPS)
                    self.pool_conv_us[c] = [ev.median_us(partial(run, two), _TUNE_REPS, _TUNE_WARMUP),
                                            ev.median_us(partial(run, one), _TUNE_REPS, _TUNE_WARMUP)]
        torch.cuda.synchronize(self.dev)
        self._choice = (None, None, None, None)

    # ------------------------------------------------------------------ the stem's band kernel
    def _band_ok(self, c):
        a = self._convs[c].args[0]
        return a.in_ is not None and bool(_lib.load().hawq_incep_conv_band_ok(C.byref(a)))

    def _choose_bands(self):
        """The stem convs that run on ``hawq_incep_conv_band``, as conv indices: the plan's ``"stem_band"`` entries (none without
        the field), else the candidates whose timed band launch beat their chosen tile (``tune``; ``_time`` left ``stem_band_us``),
        else every candidate."""
        stem = [r.ref for r in self._convs if r.place == "stem"]
        if self.plan is not None:
            self.stem_band_us = {int(c): float(v) for c, v in (self.plan.get("stem_band_us") or {}).items()}
            return check_stem_band(self.plan.get("stem_band"), stem, self._band_ok)
        cands = [c for c in stem if self._band_ok(c)]
        if self.tune:
            return [c for c in cands if self.stem_band_us[c] < self.conv_us[c][self.conv_tiles[c]]]
        return cands

    # ------------------------------------------------------------------ the stem's conv + max pool launches
    def _choose_pools(self, tiles, groups, nib):
        """The stem conv + max pool pairs that run as one ``hawq_incep_conv_band_pool``, as conv index -> (the launch's block, the
        pool record it leaves nothing of): the plan's ``"stem_pool"`` entries (none without the field), else the candidates whose
        timed fused launch beat the pair as the plan issues it (``tune``; ``stem_pool_us``: conv -> [pair, fused]), else every
        candidate the library takes.  A conv that the plan runs as a split-K launch is no candidate."""
        pairs, blocks = stem_pool_pairs(self._launches), {}
        if not pairs:
            raise PlanNotApplicable("stem_pool: no stem conv of this model is read by a table-free 3x3 / stride 2 max pool alone")
        for c, (r, p) in pairs.items():   # the conv's block, writing where the pool writes
            f = _lib.IncepConvArgs.from_buffer_copy(r.args[0])
            f.out, f.ldo, f.c_off = p.args[0].out, p.args[0].ldo, p.args[0].c_off
            blocks[c] = f
        ok = lambda c: blocks[c].in_ is not None and (c,) not in self._splits and \
            bool(_lib.load().hawq_incep_conv_band_pool_ok(C.byref(blocks[c])))   # noqa: E731
        if self.plan is not None:
            self.stem_pool_us = {int(c): [float(v) for v in us] for c, us in (self.plan.get("stem_pool_us") or {}).items()}
            kept = check_stem_pool(self.plan.get("stem_pool"), list(pairs), ok)
        else:
            kept = [c for c in pairs if ok(c)]
            if self.tune and kept:
                self._time_pools(kept, pairs, blocks, tiles, groups, nib)
                kept = [c for c in kept if self.stem_pool_us[c][1] < self.stem_pool_us[c][0]]   # a tie goes to the pair
        self._keep += [blocks[c] for c in kept]
        return {c: (blocks[c], pairs[c][1]) for c in kept}

    def _time_pools(self, cands, pairs, blocks, tiles, groups, nib):
        """``stem_pool_us[c]`` = [the pair, the fused launch] in microseconds for every conv of `cands`, on the buffers of a forward
        of the plan and by the method of the other timings; the pair is the conv on its chosen tile or band launch, then the pool
        on the entry point ``fast_pools`` selects, timed as a block."""
        lib, sp = _lib.load(), self.stream.cuda_stream
        self._choice = (tiles, groups, None, nib or None)
        with EventTimer(sp, _TUNE_REPS + 1) as ev:
            torch.cuda.synchronize(self.dev)
            with torch.cuda.stream(self.stream):
                for op in self._write():
                    op()
                for c in cands:
                    a, b = C.byref(pairs[c][0].args[0]), C.byref(pairs[c][1].args[0])
                    if c in self.stem_band_convs:
                        conv = partial(_lib.call, "hawq_incep_conv_band", a, sp)
                    else:
                        conv = partial(_lib.call, "hawq_incep_conv_tiled", a, int(tiles[c]), sp)
                    if self.fast_pools and lib.hawq_incep_pool_v_ok(b, pairs[c][1].ref):
                        pool = partial(_lib.call, "hawq_incep_pool_v", b, pairs[c][1].ref, sp)
                    else:
                        pool = partial(_lib.call, pairs[c][1].name, b, sp)
                    fused = partial(_lib.call, "hawq_incep_conv_band_pool", C.byref(blocks[c]), sp)
                    self.n_timing_launches += 3 * (_TUNE_WARMUP + _TUNE_REPS)
                    self.stem_pool_us[c] = [ev.median_us(lambda: (conv(), pool()), _TUNE_REPS, _TUNE_WARMUP),
                                            ev.median_us(fused, _TUNE_REPS, _TUNE_WARMUP)]
        torch.cuda.synchronize(self.dev)
        self._choice = (None, None, None, None)

    # ------------------------------------------------------------------ split-K launches
    def _split_args(self, convs, slices):
        """(entry point, group block, the call's arguments in front of the workspace) of one split launch; a single conv is a group
        of one.  ``hawq_incep_conv_group_splitk`` on tile 3 under ``grouped``; under ``nibble_groups`` its mixed-form twin
        ``hawq_incep_conv_group_nib_splitk`` on mixed-group tile 2, the members' blocks and mask bits from the nibble choice"""
        s = (C.c_int32 * _lib.INCEP_GROUP_MAX)(*slices)
        if self.nibble_groups:
            g, mask = self._ngroup_args(convs, self._split_nib)
            return "hawq_incep_conv_group_nib_splitk", g, (C.byref(g), mask, 2, s)
        g = self._group_args(convs)
        return "hawq_incep_conv_group_splitk", g, (C.byref(g), 3, s)

    def _split_ok(self, convs, slices):
        if not 1 <= len(convs) <= _lib.INCEP_GROUP_MAX or not isinstance(slices, (list, tuple)) or len(slices) != len(convs) or \
                any(not isinstance(s, int) or isinstance(s, bool) for s in slices):
            return False
        name, _, args = self._split_args(convs, slices)
        return bool(getattr(_lib.load(), name + "_ok")(*args))

    def _split_workspace(self, launches):
        """one slab and one zeroed counter buffer for the split launches `launches` = [(convs, slices)], sized for the largest of
        them: every launch leaves the counters zero, and the launches of this engine - the fp32 chain, the uint8 chain (the same
        callables behind another stem) and the tuner's - all go to ``self.stream``, one after another, so they share it"""
        slab, cnt, sb, cb = 16, 4, C.c_int64(), C.c_int64()
        for convs, slices in launches:
            name, _, args = self._split_args(convs, slices)
            _lib.call(name + "_workspace", *args, C.byref(sb), C.byref(cb))
            slab, cnt = max(slab, sb.value), max(cnt, cb.value)
        return torch.zeros(slab, dtype=torch.uint8, device=self.dev), torch.zeros(cnt // 4, dtype=torch.int32, device=self.dev)

    def _choose_splits(self, tiles, groups, nib=None):
        """Which conv launches of the grouped plan run as its split launch (``_split_args``), {member conv indices: slice counts}.
        Candidates are the launches (tiles, groups) issue behind conv1: grouped levels - of a ``nibble_groups`` plan the mixed-form
        ones -, single convs (groups of one; hawq4 where `nib` names them), the classifier.  A member's K steps are 64-byte rows:
        four 16-channel units of an int8 member, eight of a hawq4 one.
        From the plan's ``"splitk"`` field (none without it), else timed (``tune``), else ``split_slices`` with S_max from the CU
        count (``splitk=True``) or as given (``splitk=n``).  Leaves ``splitk_candidates`` and the workspace."""
        head = self._launches.index(self._convs[0]) + 1
        issued = [tuple(groups[i][0]) if is_group else (self._launches[i].ref,)
                  for is_group, i in grouped_order(self._launches, groups)[head:] if is_group or self._launches[i].kind == "conv"]
        cus = torch.cuda.get_device_properties(self.dev).multi_processor_count
        self._split_nib = nib = nib or {}

        def shape(convs):   # workgroups on 128 x 64 tiles, K steps per member
            blocks = [self._convs[c].args[0] for c in convs]
            px = [a.N * ((a.H + 2 * a.pad_h - a.KH) // a.stride + 1) * ((a.W + 2 * a.pad_w - a.KW) // a.stride + 1) for a in blocks]
            return (sum(-(-p // 128) * -(-a.Cout // 64) for p, a in zip(px, blocks)),
                    [-(-(a.KH * a.KW * (a.Cin >> 4)) // (8 if c in nib else 4)) for c, a in zip(convs, blocks)])

        def slices_for(convs, s_max):   # None: no member is cut, or the library refuses the launch
            s = [split_slices(st, s_max) for st in shape(convs)[1]]
            return s if max(s) > 1 and self._split_ok(convs, s) else None

        if self.plan is not None:
            try:
                entries = [(tuple(e["convs"]), list(e["slices"]), dict(e.get("us", {}))) for e in self.plan.get("splitk", [])]
            except (KeyError, TypeError, ValueError) as exc:
                raise StalePlan(f"not a list of split-K launches: {exc!r}") from exc
            for convs, slices, _ in entries:
                if convs not in issued or [c for c, _, _ in entries].count(convs) != 1 or not self._split_ok(convs, slices):
                    raise StalePlan(f"split-K launch {list(convs)} with slices {slices}: not an issued launch of this plan, or refused")
            self.splitk_candidates = [{"convs": list(c), "slices": s, "us": us, "kept": True} for c, s, us in entries]
        elif self.tune:
            small = [c for c in issued if shape(c)[0] < cus]
            variants = [{n: s for n in (2, 4, 8, 16) for s in [slices_for(c, n)] if s is not None} for c in small]
            times = self._time_splits(small, variants, tiles, groups, nib)
            for c, var, us in zip(small, variants, times):
                if var:
                    best = min(var, key=lambda n: (us[str(n)], n))
                    self.splitk_candidates.append({"convs": list(c), "slices": var[best], "us": us, "kept": us[str(best)] < us["plain"]})
        else:
            for c in issued:
                w = shape(c)[0]
                if self.splitk is True and w >= cus:
                    continue
                s = slices_for(c, 1 << (min(16, cus // w).bit_length() - 1) if self.splitk is True else self.splitk)
                if s is not None:
                    self.splitk_candidates.append({"convs": list(c), "slices": s, "us": {}, "kept": True})
        kept = {tuple(e["convs"]): e["slices"] for e in self.splitk_candidates if e["kept"]}
        self._split_ws = self._split_workspace(kept.items())
        self._keep += list(self._split_ws)
        return kept

    def _time_splits(self, cands, variants, tiles, groups, nib):
        """Per candidate launch of `cands`, on the buffers of a forward of the plan (tiles, groups) and by the method of the group
        timing: ``"plain"``, the microseconds of the launch as that plan issues it, and per S_max of `variants` (``"2"`` ..) those
        of the split launch with its slice counts."""
        sp, out, gtile = self.stream.cuda_stream, [], {tuple(c): t for c, t in groups}
        ws = self._split_workspace([(c, s) for c, var in zip(cands, variants) for s in var.values()])
        self._choice = (tiles, groups, None, nib or None)
        with EventTimer(sp, _TUNE_REPS + 1) as ev:
            torch.cuda.synchronize(self.dev)
            with torch.cuda.stream(self.stream):
                for op in self._write():
                    op()
                for c, var in zip(cands, variants):
                    if not var:
                        out.append({})
                        continue
                    g, mask = self._ngroup_args(c, nib) if self.nibble_groups else (self._group_args(c), 0)
                    if c in gtile and self.nibble_groups:
                        plain = partial(_lib.call, "hawq_incep_conv_group_nib", C.byref(g), mask, int(gtile[c]), sp)
                    elif c in gtile:
                        plain = partial(_lib.call, "hawq_incep_conv_group", C.byref(g), int(gtile[c]), sp)
                    elif mask:
                        plain = partial(_lib.call, "hawq_incep_conv_nib", C.byref(g.conv[0]), int(nib[c[0]]), sp)
                    elif c[0] in self.stem_band_convs:
                        plain = partial(_lib.call, "hawq_incep_conv_band", C.byref(g.conv[0]), sp)
                    else:
                        plain = partial(_lib.call, "hawq_incep_conv_tiled", C.byref(g.conv[0]), int(tiles[c[0]]), sp)
                    self.n_timing_launches += (_TUNE_WARMUP + _TUNE_REPS) * (len(var) + 1)
                    us = {"plain": ev.median_us(plain, _TUNE_REPS, _TUNE_WARMUP)}
                    for n, s in var.items():
                        name, _, args = self._split_args(c, s)
                        us[str(n)] = ev.median_us(partial(_lib.call, name, *args, ws[0].data_ptr(), ws[1].data_ptr(), sp), _TUNE_REPS, _TUNE_WARMUP)
                    out.append(us)
        torch.cuda.synchronize(self.dev)
        self._choice = (None, None, None, None)
        return out

    # ------------------------------------------------------------------ nibbles
    def _nib_ok(self, c, tile, block=None):
        return isinstance(tile, int) and not isinstance(tile, bool) and \
            bool(_lib.load().hawq_incep_conv_nib_ok(C.byref(block or self._convs[c].args[0]), tile))

    def _nib_table(self):
        """`nibble_storage`'s view of the plan: one row per tensor of ``_tensors``; an entry requant is a producer of nibbles if
        ``hawq_incep_pool_v`` takes its launch with ``out_bits`` 4"""
        def writes(t):
            if t.producer != "requant":
                return t.producer
            p = _lib.IncepPoolArgs.from_buffer_copy(t.record.args[0])
            p.out_bits, (p.lo2, p.hi2) = 4, t.rng
            return "requant" if _lib.load().hawq_incep_pool_v_ok(C.byref(p), t.record.ref) else None
        return [(*t.rng, writes(t), list(t.cons)) for t in self._tensors]

    def _nib_blocks(self, tensors):
        """The argument blocks of a plan that stores `tensors` (indices into ``_tensors``) hawq4: conv -> its block on
        ``hawq_incep_conv_nib`` for every conv that reads one of them, entry requant record -> its ``out_bits`` 4 block.  Same
        tables, same clamps - the lower bound 0 where the values are >= 0 anyway (``_T.rng``) -; hawq4 buffers and weights are made
        once per tensor and conv (``_nib_buf``, ``_nib_w``)."""
        from .packing import pack_hawq4
        convs, pools = {}, {}
        for ti in tensors:
            t = self._tensors[ti]
            if ti not in self._nib_buf:
                self._nib_buf[ti] = torch.zeros(self.N * t.h * t.w * t.pitch // 2, dtype=torch.uint8, device=self.dev)
        for ti in tensors:
            t = self._tensors[ti]
            if t.producer == "requant":
                p = _lib.IncepPoolArgs.from_buffer_copy(t.record.args[0])
                p.out, p.out_bits, (p.lo2, p.hi2) = self._nib_buf[ti].data_ptr(), 4, t.rng
                pools[t.record] = p
            for c in t.cons:
                _, out, w, _ = self._conv_io[c]
                if c not in self._nib_w:
                    self._nib_w[c] = torch.from_numpy(pack_hawq4(w).reshape(-1)).to(self.dev)
                a = _lib.IncepConvArgs.from_buffer_copy(self._convs[c].args[0])
                a.in_, a.wgt = self._nib_buf[ti].data_ptr(), self._nib_w[c].data_ptr()
                if out is not None and out.cons and self._tensors.index(out) in tensors:
                    a.out, a.out_bits, (a.q_lo, a.q_hi) = self._nib_buf[self._tensors.index(out)].data_ptr(), 4, out.rng
                convs[c] = a
        return convs, pools

    def _choose_nibbles(self, T):
        """The fourth component of the choice, {conv: nibble tile}: the convs `nibble_storage` puts on the nibble kernel, given which
        convs are 4-bit x 4-bit and taken by it - all of them (each on the first tile of ``_NIB_TILES`` it accepts), those that
        beat their best int8 tile when timed (``tune``), or those a plan's ``"nibble"`` field names.  Leaves ``nibble_convs``,
        ``nibble_tensors``, ``nibble_us``, ``nibble_bytes`` and the blocks the writer issues, and frees what the choice leaves
        unused: the int8 form of a hawq4 tensor or weight, and the hawq4 form of everything else."""
        NT = _lib.load().hawq_incep_conv_nib_num_tiles()
        self._nib_buf, self._nib_w = {}, {}
        w4 = {c: w is not None and w.size and int(w.min()) >= -8 and int(w.max()) <= 7 for c, (_, _, w, _) in self._conv_io.items()}
        tiles_of = {c: [t for t in range(1, NT + 1) if w4.get(c) and self._nib_ok(c, t)] for c in range(len(self._convs))}
        table, able = self._nib_table(), [bool(tiles_of[c]) for c in range(len(self._convs))]
        cand = nibble_storage(table, able)
        if not cand:
            raise PlanNotApplicable("nibble: no conv of this model reads 4-bit values with 4-bit weights from a tensor that can be "
                                    "stored hawq4 (a uniform8 schedule has none)")
        convs_of = lambda ts: sorted(c for ti in ts for c in self._tensors[ti].cons)   # noqa: E731
        if self.plan is not None and "nibble" in self.plan:
            try:
                tile = {int(c): t for c, t in self.plan["nibble"]}
            except (TypeError, ValueError) as exc:
                raise StalePlan(f"not a list of (conv, nibble tile): {exc!r}") from exc
            if any(c not in tiles_of or t not in tiles_of[c] for c, t in tile.items()):
                raise StalePlan("nibble: a conv or tile of the plan is refused")
            chosen = nibble_storage(table, [c in tile for c in range(len(self._convs))])
            if convs_of(chosen) != sorted(tile):
                raise StalePlan("nibble: the plan's convs are not what the storage policy makes of them")
            self.nibble_us = {int(c): dict(d) for c, d in self.plan.get("nibble_us", {}).items()}
        elif self.tune and self.plan is None:
            self.nibble_us = self._time_nibbles(cand, tiles_of)
            best = {c: min(us, key=lambda t: (us[t], t)) for c, us in self.nibble_us.items()}
            wins = [c in best and self.nibble_us[c][best[c]] < self.conv_us[c][self.conv_tiles[c]] for c in range(len(self._convs))]
            chosen = nibble_storage(table, wins)
            tile = {c: best[c] for c in convs_of(chosen)}
        else:
            chosen = cand
            tile = {c: next(t for t in _NIB_TILES if t in tiles_of[c]) for c in convs_of(chosen)}
        self._nib_conv, self._nib_pool = self._nib_blocks(chosen)
        self.nibble_convs, self.nibble_tensors = tile, sorted(chosen)
        # bytes of the conv operands, int8 containers against this plan, and the buffers each form no longer needs
        wb = sum(io[3].numel() for io in self._conv_io.values())
        ab = sum(t.buf.numel() * t.buf.element_size() for t in self._tensors)
        dead = {id(self._conv_io[c][3]) for c in tile} | {id(self._tensors[ti].buf) for ti in chosen}
        self.nibble_bytes = {"weights": (wb, wb - sum(self._conv_io[c][3].numel() // 2 for c in tile)),
                             "activations": (ab, ab - sum(self._tensors[ti].buf.numel() // 2 for ti in chosen))}
        self._keep = [x for x in self._keep if id(x) not in dead]
        self._keep += [self._nib_buf[ti] for ti in chosen] + [self._nib_w[c] for c in tile]
        self._keep += list(self._nib_conv.values()) + list(self._nib_pool.values())
        for ti in chosen:
            self._tensors[ti].buf = self._nib_buf[ti]
        del self._nib_buf, self._nib_w
        return tile

    # ------------------------------------------------------------------ mixed-form groups
    def _ngroup_args(self, convs, nib):
        """(group block, mask) of one ``hawq_incep_conv_group_nib`` launch: a member is on its ``_nib_conv`` block, with its mask bit
        set, if it is a nibble conv of `nib`, and on its own block otherwise"""
        g, mask = _lib.IncepGroupArgs(), 0
        g.n = len(convs)
        for k, c in enumerate(convs):
            g.conv[k] = self._nib_conv[c] if c in nib else self._convs[c].args[0]
            mask |= (c in nib) << k
        return g, mask

    def _ngroup_ok(self, convs, tile, nib):
        if not 1 <= len(convs) <= _lib.INCEP_GROUP_MAX or not isinstance(tile, int) or isinstance(tile, bool):
            return False
        g, mask = self._ngroup_args(convs, nib)
        return bool(_lib.load().hawq_incep_conv_group_nib_ok(C.byref(g), mask, tile))

    def _choose_nibble_groups(self, tiles, nib):
        """The mixed-form grouped launches [(member conv indices, tile of ``hawq_incep_conv_group_nib``)] of a nibble plan whose
        nibble convs `nib` are chosen: every level of two or more convs that the library takes on tile 2; with ``tune``, on the
        faster of the two tiles, and only where that beat the sum of its members' chosen single launches; with a plan that has a
        ``"nibble_groups"`` field, exactly its entries.  Leaves ``group_candidates``."""
        # members with the most K steps first (K / 64 of an int8 member, K / 128 of a hawq4 one), so that the heavy workgroups
        # start first: as with the int8 groups, the order is free, and unmeasured
        def steps(c):
            a = self._convs[c].args[0]
            return -(-(a.KH * a.KW * a.Cin) // (128 if c in nib else 64))
        cands = [sorted(lv, key=lambda c: -steps(c)) for lv in self.conv_level_list if len(lv) >= 2]
        ok = lambda convs, tile: self._ngroup_ok(convs, tile, nib)   # noqa: E731
        if self.plan is not None and self.plan.get("nibble_groups") is not None:
            entries = self.plan["nibble_groups"]
            groups = check_groups(entries, len(self._convs), self.conv_level_list, ok)
            us = {tuple(g["convs"]): dict(g.get("us", {})) for g in entries}
            self.group_candidates = [{"convs": list(c), "tile": t, "us": us[tuple(c)], "kept": True} for c, t in groups]
        elif self.tune and self.plan is None:
            NG = _lib.load().hawq_incep_conv_group_nib_num_tiles()
            gtiles = [[t for t in range(1, NG + 1) if ok(c, t)] for c in cands]
            for c, us in zip(cands, self._time_nibble_groups(cands, gtiles, tiles, nib)):
                if us:
                    tile = min(us, key=lambda t: (us[t], t))
                    singles = sum(self.nibble_us[i][nib[i]] if i in nib else self.conv_us[i][tiles[i]] for i in c)
                    self.group_candidates.append({"convs": c, "tile": tile, "kept": us[tile] < singles,
                                                  "us": {**{str(t): v for t, v in us.items()}, "singles": singles}})
        else:
            self.group_candidates = [{"convs": c, "tile": 2, "us": {}, "kept": True} for c in cands if ok(c, 2)]
        return [(g["convs"], g["tile"]) for g in self.group_candidates if g["kept"]]

    def _time_nibble_groups(self, cands, gtiles, tiles, nib):
        """Microseconds of every candidate level on every tile of `gtiles` it accepts, as ``_time`` measures the int8 groups: on the
        buffers of a forward of the chosen nibble plan, its launches single."""
        sp, out = self.stream.cuda_stream, []
        self._choice = (tiles, None, None, nib)
        with EventTimer(sp, _TUNE_REPS + 1) as ev:
            torch.cuda.synchronize(self.dev)
            with torch.cuda.stream(self.stream):
                for op in self._write():
                    op()
                for c, ts in zip(cands, gtiles):
                    g, mask = self._ngroup_args(c, nib)
                    self.n_timing_launches += (_TUNE_WARMUP + _TUNE_REPS) * len(ts)
                    out.append({t: ev.median_us(lambda: _lib.call("hawq_incep_conv_group_nib", C.byref(g), mask, t, sp),
                                                _TUNE_REPS, _TUNE_WARMUP) for t in ts})
        torch.cuda.synchronize(self.dev)
        self._choice = (None, None, None, None)
        return out

    def _time_nibbles(self, cand, tiles_of):
        """Microseconds of every candidate conv on every nibble tile it accepts, as ``_time`` measures the int8 tiles: on the
        buffers of a forward of the plan that stores every tensor of `cand` hawq4."""
        sp = self.stream.cuda_stream
        self._nib_conv, self._nib_pool = self._nib_blocks(cand)
        convs = sorted(self._nib_conv)
        self._choice = (None, None, None, {c: tiles_of[c][0] for c in convs})
        out = {}
        with EventTimer(sp, _TUNE_REPS + 1) as ev:
            torch.cuda.synchronize(self.dev)
            with torch.cuda.stream(self.stream):
                for op in self._write():
                    op()
                for c in convs:
                    a = self._nib_conv[c]
                    tiles = [t for t in tiles_of[c] if self._nib_ok(c, t, a)]
                    self.n_timing_launches += (_TUNE_WARMUP + _TUNE_REPS) * len(tiles)
                    out[c] = {t: ev.median_us(lambda: _lib.call("hawq_incep_conv_nib", C.byref(a), t, sp), _TUNE_REPS, _TUNE_WARMUP)
                              for t in tiles}
        torch.cuda.synchronize(self.dev)
        self._choice = (None, None, None, None)
        return out

    def _choose_fans(self, tiles, groups, nib=None, unfanned=()):
        """the third component: from the plan's ``"fan_out"`` field if it has one, else timed against the plain launches (``tune``),
        else every candidate boundary on the default tiles (a tile plan without the field fixes the other convs' tiles only).
        With `nib` (the nibble convs of a ``nibble_fan`` engine) the same for the ``"nibble_fan"`` field, on the launches of
        ``hawq_incep_conv_group_nib_fan`` and the entry requants as the nibble plan issues them; a boundary whose hawq4 entry
        requant ``hawq_incep_pool_v`` does not take on a residual range is no candidate."""
        if nib is None:
            field, order, bounds, ok = "fan_out", _FAN_TILES, fan_boundaries(self._launches, unfanned=unfanned), self._fan_ok
        else:
            field, order, bounds = "nibble_fan", _NIB_FAN_TILES, fan_boundaries(self._launches, self._nib_pool)
            ok = partial(self._nfan_ok, nib=nib)
            bounds = [b for b in bounds if all(
                _lib.load().hawq_incep_pool_v_ok(C.byref(self._residual_args(r, off, c, self._nib_pool[r])), r.ref)
                for r in map(self._launches.__getitem__, b["requants"]) if r in self._nib_pool for off, c in b["residual"])]
        cands = {b["unit"]: b for b in bounds if b["candidate"]}
        sets = {k: self._fan_sets(b, groups) for k, b in cands.items()}
        if self.plan is not None and field in self.plan:
            by_key = {(k, fan_key(s)): s for k in cands for s in sets[k]}
            got = check_fan_out(self.plan[field], {k: [fan_key(s) for s in sets[k]] for k in cands},
                                lambda k, key, t: ok(by_key[k, key], cands[k], t))
            us = {e["unit"]: dict(e.get("us", {})) for e in self.plan[field]}
            self.fan_candidates = [{"unit": k, "tiles": dict(t), "us": us[k], "kept": True} for k, t in got]
            return [(cands[k], {by_key[k, key]: t for key, t in tl.items()}) for k, tl in got]
        accepted = {k: {s: [t for t in order if ok(s, b, t)] for s in sets[k]} for k, b in cands.items()}
        able = [k for k in cands if all(accepted[k][s] for s in sets[k])]   # a boundary with a refused producer launch is not chosen
        if self.tune and self.plan is None:
            for k, rec in zip(able, self._time_fans([cands[k] for k in able], [accepted[k] for k in able], tiles, groups, nib)):
                self.fan_candidates.append({"unit": k, **rec})
        else:
            self.fan_candidates = [{"unit": k, "tiles": {fan_key(s): accepted[k][s][0] for s in sets[k]}, "us": {}, "kept": True}
                                   for k in able]
        return [(cands[f["unit"]], {s: f["tiles"][fan_key(s)] for s in sets[f["unit"]]}) for f in self.fan_candidates if f["kept"]]

    def _time_fans(self, bounds, accepted, tiles, groups, nib=None):
        """Per boundary of `bounds`, on the real buffers as ``_time`` left them - with `nib`, after a forward of the chosen nibble
        plan (tiles, groups, nib), whose launches and blocks then stand for the int8 ones below - (every launch here is a pure
        function of buffers it does not write): ``"plain"``, the microseconds of its producer launches as (tiles, groups) issue them followed by its entry
        requants, one block; every producer launch with its fan on every accepted tile (``"<launch>@<tile>"``); and ``"fan"``, one
        block of the fan-out launches on their fastest tiles followed by the residual requants.  Kept if fan < plain."""
        sp, lib, out = self.stream.cuda_stream, _lib.load(), []

        def pool(a, ref, name):   # only the vectorised family stores hawq4
            fast = a.out_bits == 4 or (self.fast_pools and lib.hawq_incep_pool_v_ok(C.byref(a), ref))
            return partial(_lib.call, "hawq_incep_pool_v", C.byref(a), ref, sp) if fast else partial(_lib.call, name, C.byref(a), sp)

        def producers(s, gtile):   # the launch that holds the producers `s` as the rest of the choice issues it
            if nib is None and s in gtile:
                g = self._group_args(s)
                keep.append(g)
                return partial(_lib.call, "hawq_incep_conv_group", C.byref(g), int(gtile[s]), sp)
            if s in gtile:
                g, mask = self._ngroup_args(s, nib)
                keep.append(g)
                return partial(_lib.call, "hawq_incep_conv_group_nib", C.byref(g), mask, int(gtile[s]), sp)
            if nib is not None and s[0] in nib:
                return partial(_lib.call, "hawq_incep_conv_nib", C.byref(self._nib_conv[s[0]]), int(nib[s[0]]), sp)
            return partial(_lib.call, "hawq_incep_conv_tiled", C.byref(self._convs[s[0]].args[0]), int(tiles[s[0]]), sp)

        def fan_launch(s, b, t):
            if nib is None:
                g, f = self._fan_args(s, b)
                keep.extend([g, f])
                return partial(_lib.call, "hawq_incep_conv_group_fan", C.byref(g), f, t, sp)
            g, mask, f, fan_mask = self._nfan_args(s, b, nib)
            keep.extend([g, f])
            return partial(_lib.call, "hawq_incep_conv_group_nib_fan", C.byref(g), mask, f, fan_mask, t, sp)

        def block(ops):
            def run():
                for op in ops:
                    op()
            self.n_timing_launches += (_TUNE_WARMUP + _TUNE_REPS) * len(ops)
            return ev.median_us(run, _TUNE_REPS, _TUNE_WARMUP)

        with EventTimer(sp, _TUNE_REPS + 1) as ev:
            torch.cuda.synchronize(self.dev)
            with torch.cuda.stream(self.stream):
                if nib is not None:
                    self._choice = (tiles, groups, None, nib)
                    for op in self._write():
                        op()
                    self._choice = (None, None, None, None)
                for b, acc in zip(bounds, accepted):
                    gtile = {tuple(c): t for c, t in groups or []}
                    plain, fan, us, chosen, keep = [], [], {}, {}, []
                    for s in acc:
                        plain.append(producers(s, gtile))
                        for t in acc[s]:
                            us[f"{fan_key(s)}@{t}"] = block([fan_launch(s, b, t)])
                        chosen[s] = min(acc[s], key=lambda t: (us[f"{fan_key(s)}@{t}"], t))
                        fan.append(fan_launch(s, b, chosen[s]))
                    for i in b["requants"]:
                        r = self._launches[i]
                        issued = self._nib_pool.get(r) if nib is not None else None
                        plain.append(pool(issued or r.args[0], r.ref, r.name))
                        for off, c in b["residual"]:
                            a = self._residual_args(r, off, c, issued)
                            keep.append(a)
                            fan.append(pool(a, r.ref, r.name))
                    us["plain"], us["fan"] = block(plain), block(fan)
                    out.append({"tiles": {fan_key(s): t for s, t in chosen.items()}, "us": us, "kept": us["fan"] < us["plain"]})
        torch.cuda.synchronize(self.dev)
        return out

    def _time(self, T, cands):
        """Microseconds (HIP events, ``EventTimer.median_us``) of every accepted tile id per conv launch, and of every accepted tile
        per candidate group of `cands`: each launch on its real buffers, which hold the forward of a random image (every conv launch
        is a pure function of its input buffer, so repeating it changes nothing)."""
        sp, gtiles = self.stream.cuda_stream, [[t for t in range(1, T + 1) if self._group_ok(c, t)] for c in cands]

        def us(name, block, tiles):
            self.n_timing_launches += (_TUNE_WARMUP + _TUNE_REPS) * len(tiles)
            return {t: ev.median_us(lambda: _lib.call(name, C.byref(block), t, sp), _TUNE_REPS, _TUNE_WARMUP) for t in tiles}

        with EventTimer(sp, _TUNE_REPS + 1) as ev:
            torch.cuda.synchronize(self.dev)
            with torch.cuda.stream(self.stream):
                self.x_in.normal_()
                for op in self._write():   # ``_choice`` is still the default plan's
                    op()
                # conv1 under fused_stem is not launched, not timed
                convs = [us("hawq_incep_conv_tiled", r.args[0], [t for t in range(T + 1) if t == 0 or self._tile_ok(i, t)]
                            if i or not self.fused_stem else []) for i, r in enumerate(self._convs)]
                groups = [us("hawq_incep_conv_group", self._group_args(c), tiles) for c, tiles in zip(cands, gtiles)]
                for r in self._convs if self.stem_band else []:   # the band kernel next to the tiles of the stem convs it takes
                    if r.place == "stem" and self._band_ok(r.ref):
                        self.n_timing_launches += _TUNE_WARMUP + _TUNE_REPS
                        self.stem_band_us[r.ref] = ev.median_us(partial(_lib.call, "hawq_incep_conv_band", C.byref(r.args[0]), sp),
                                                                _TUNE_REPS, _TUNE_WARMUP)
        torch.cuda.synchronize(self.dev)
        return convs, groups

    def export_plan(self):
        """The conv tile choice of the current batch shape (and, of a grouped engine, its grouped launches) as a JSON-serialisable
        dict (``make_plan``), for ``plan=``."""
        if self.conv_tiles is None:
            raise RuntimeError("export_plan: no tuned plan (build the engine with tune=True or plan=... and run a forward first)")
        groups = [g for g in self.group_candidates if g["kept"]] if self.grouped else None
        fans = [f for f in self.fan_candidates if f["kept"]] if self.fan_out else None
        ngroups = [g for g in self.group_candidates if g["kept"]] if self.nibble_groups else None
        nfans = [f for f in self.fan_candidates if f["kept"]] if self.nibble_fan else None
        return make_plan(self._batch, self.conv_launches, _lib.load().hawq_incep_conv_num_tiles(), self.conv_tiles, self.conv_us,
                         groups, fans, (self.nibble_convs, self.nibble_us) if self.nibble else None, ngroups, nfans,
                         [e for e in self.splitk_candidates if e["kept"]] if self.splitk else None,
                         (self.stem_band_convs, self.stem_band_us) if self.stem_band else None,
                         (self.stem_pool_convs, self.stem_pool_us) if self.stem_pool else None,
                         (self.pool_conv_convs, self.pool_conv_us) if self.pool_conv else None)

    # ------------------------------------------------------------------ the writer
    def _write(self, u8=False):
        """The callables of one chain, from the records, ``_choice`` and the engine's options - the only place that makes one.  Per
        record: a conv alone, tiled with its chosen id, on the band kernel (``_bands``) or as a member of a grouped launch; a pool on its named entry point or, under
        ``fast_pools`` where the library takes it, on ``hawq_incep_pool_v``.  The stem's head (the records up to conv1) as it stands,
        as one ``hawq_incep_stem_f32`` (``fused_stem``) or, for the uint8 chain, as one ``hawq_incep_stem_u8`` in front of the fp32
        chain's own callables.  The records' order, or with groups ``grouped_order``.  The fp32 chain leaves ``_at`` (record -> index
        of the launch that covers it) and ``group_launches``.  A conv launch - grouped, or single as a group of one - that ``_splits``
        names is issued as the plan's split launch (``_split_args``: ``hawq_incep_conv_group_splitk``, or under ``nibble_groups``
        ``hawq_incep_conv_group_nib_splitk`` with its mask) with its slice counts on the engine's one workspace, in the place of the
        launch it replaces (``splitk_launches``); the uint8 chain shares those callables.  A stem conv that ``_pooled`` names is
        issued as one ``hawq_incep_conv_band_pool`` on the block kept there, and nothing is issued for its max pool record; likewise a
        conv that ``_avg_fused`` names is issued as one ``hawq_incep_avgpool_conv`` on its pool record's block and its own."""
        tiles, groups, fans, nib = self._choice
        lib, sp, launches = _lib.load(), self.stream.cuda_stream, self._launches
        fan_of = {s: (b, t) for b, by_set in fans or [] for s, t in by_set.items()}           # producer launch -> its boundary, tile
        entry = {i: b for b, _ in fans or [] for i in b["requants"]}                          # entry requant record -> its boundary

        def op(name, *args):
            return partial(_lib.call, name, *args, sp)

        def single(r):
            if r.kind == "other":
                return op(r.name, *r.args)
            if nib and r.kind == "conv" and r.ref in nib:   # hawq4 operands: the nibble kernel, on its own block
                return op("hawq_incep_conv_nib", C.byref(self._nib_conv[r.ref]), int(nib[r.ref]))
            if nib and r in self._nib_pool:   # an entry requant that writes hawq4: only the vectorised family has that form
                return op("hawq_incep_pool_v", C.byref(self._nib_pool[r]), r.ref)
            a = C.byref(r.args[0])
            if r.kind == "conv" and r.ref in self._bands:   # a stem conv on the band kernel: the record's own block
                return op("hawq_incep_conv_band", a)
            if r.kind == "conv":
                return op(r.name, a) if tiles is None else op("hawq_incep_conv_tiled", a, int(tiles[r.ref]))
            fast = self.fast_pools and lib.hawq_incep_pool_v_ok(a, r.ref)
            return op("hawq_incep_pool_v", a, r.ref) if fast else op(r.name, a)

        if u8:
            return [op("hawq_incep_stem_u8", self.x_u8.data_ptr(), self.lut_dev.data_ptr(), C.byref(self._stem_a))] + self._tail
        head = launches.index(self._convs[0]) + 1
        if self.fused_stem:
            ops = [op("hawq_incep_stem_f32", self.x_in.data_ptr(), *self._input_quant(), C.byref(self._stem_a))]
        else:
            ops = [single(r) for r in launches[:head]]
        n_stem, issued, masks, fanned, fmasks, residual, split = len(ops), [], [], [], [], [], []
        at = {r: min(i, n_stem - 1) for i, r in enumerate(launches[:head])}
        order = [(False, i) for i in range(len(launches))] if groups is None else grouped_order(launches, groups)
        for is_group, i in order[head:]:   # the stem stays in place in either order
            r = None if is_group else launches[i]
            convs, tile = groups[i] if is_group else ([r.ref], None) if r.kind == "conv" else (None, None)
            if convs is not None and tuple(convs) in fan_of:   # a producer launch of a chosen boundary, alone or grouped
                b, tile = fan_of[tuple(convs)]
                at.update((self._convs[c], len(ops)) for c in convs)
                if self.nibble_fan:   # members and fan outputs of either form
                    g, mask, f, fan_mask = self._nfan_args(convs, b, nib)
                    ops.append(op("hawq_incep_conv_group_nib_fan", C.byref(g), mask, f, fan_mask, int(tile)))
                    fmasks.append(fan_mask)
                    if is_group:
                        masks.append(mask)
                else:
                    g, f = self._fan_args(convs, b)
                    ops.append(op("hawq_incep_conv_group_fan", C.byref(g), f, int(tile)))
                self._keep += [g, f]
                fanned.append((b["unit"], list(convs), int(tile)))
                if is_group:
                    issued.append((list(convs), int(tile)))
            elif convs is not None and tuple(convs) in self._splits:   # in the place of the launch it replaces, a single conv as a group of one
                name, g, args = self._split_args(convs, self._splits[tuple(convs)])
                self._keep += [g, args[-1]]
                at.update((self._convs[c], len(ops)) for c in convs)
                ops.append(op(name, *args, self._split_ws[0].data_ptr(), self._split_ws[1].data_ptr()))
                split.append((list(convs), list(self._splits[tuple(convs)])))
                if is_group:
                    issued.append((list(convs), int(tile)))
                    if self.nibble_groups:
                        masks.append(args[1])
            elif is_group and self.nibble_groups:   # members of either operand form, each on the block its single launch has
                g, mask = self._ngroup_args(convs, nib)
                self._keep.append(g)
                at.update((self._convs[c], len(ops)) for c in convs)
                ops.append(op("hawq_incep_conv_group_nib", C.byref(g), mask, int(tile)))
                issued.append((list(convs), int(tile)))
                masks.append(mask)
            elif is_group:
                g = self._group_args(convs)
                self._keep.append(g)
                at.update((self._convs[c], len(ops)) for c in convs)
                ops.append(op("hawq_incep_conv_group", C.byref(g), int(tile)))
                issued.append((list(convs), int(tile)))
            elif i in entry:   # its producers wrote the conv-produced channels: the rest, or nothing
                b = entry[i]
                at[r] = len(ops) if b["residual"] else at[launches[min(b["producers"])]]
                for off, c in b["residual"]:
                    a = self._residual_args(r, off, c, self._nib_pool.get(r) if nib else None)
                    self._keep.append(a)
                    fast = a.out_bits == 4 or (self.fast_pools and lib.hawq_incep_pool_v_ok(C.byref(a), r.ref))   # hawq4: pool_v only
                    ops.append(op("hawq_incep_pool_v", C.byref(a), r.ref) if fast else op(r.name, C.byref(a)))
                    residual.append((b["unit"], i, off, c))
            elif r.kind == "conv" and r.ref in self._pooled:   # a stem conv + max pool pair in one launch, in the conv's place
                at[r] = at[self._pooled[r.ref][1]] = len(ops)
                ops.append(op("hawq_incep_conv_band_pool", C.byref(self._pooled[r.ref][0])))
            elif r.kind == "pool" and any(r is p for _, p in self._pooled.values()):   # nothing in the pool's place
                pass
            elif r.kind == "conv" and r.ref in self._avg_fused:   # an average-pool branch in one launch, in the conv's place
                at[r] = at[self._avg_fused[r.ref][0]] = len(ops)
                ops.append(op("hawq_incep_avgpool_conv", C.byref(self._avg_fused[r.ref][0].args[0]), C.byref(r.args[0])))
            elif r.kind == "pool" and any(r is p for p, _ in self._avg_fused.values()):   # nothing in the pool's place
                pass
            else:
                at[r] = len(ops)
                ops.append(single(r))
        self._at, self._tail, self.group_launches, self.nibble_group_masks = at, ops[n_stem:], issued, masks
        self.fan_launches, self.residual_requants, self.nibble_fan_masks = fanned, residual, fmasks
        self.splitk_launches = split
        return ops

    def _launch_chain(self, u8):
        for op in (self._ops_u8 if u8 else self._ops):
            op()

    # ------------------------------------------------------------------ uint8 image input (quant_train.py:427-440)
    def _input_quant(self):
        """(fl(1/S), lo, hi) of the input QuantAct: the arguments of the fp32 plan's ``hawq_fakequant_f32`` and of the uint8 table."""
        ia = self.model.features.q_init_block.q_input_activ
        return (float((1. / _scale(ia)).item()), *_rng(ia))

    def input_lut(self, mean, std) -> torch.Tensor:
        """int8 [3][256]: lut[c][u] = the input QuantAct of Normalize_c(ToTensor(u)), in the reference pipeline's own float32
        operations on the host (``input_quant_lut``) - a look-up is bit-identical to what the fp32 plan does to that tensor."""
        from .quant_utils import input_quant_lut
        inv, lo, hi = self._input_quant()
        return input_quant_lut(inv, mean, std, lo, hi)

    @staticmethod
    def _stem_refusal(ib):
        """why a one-launch stem kernel (``hawq_incep_stem_u8``, ``hawq_incep_stem_f32``) cannot stand for the input QuantAct + conv1
        of init block `ib` (None: it can)"""
        lo, hi = _rng(ib.q_input_activ)
        if ib.q_input_activ.activation_bit != 8 or lo < -128 or hi > 127:
            return "the input QuantAct is not 8-bit with an int8 range"
        conv = ib.q_conv1.q_convbn.conv
        if conv.in_channels != 3 or conv.out_channels % 16 or conv.kernel_size != (3, 3) or conv.stride != (2, 2) or \
                conv.padding != (0, 0) or conv.groups != 1 or conv.dilation != (1, 1):
            return "conv1 is not a 3 -> 16k channel 3x3 / stride 2 / pad 0 conv"
        if ib.q_conv1.q_activ.activation_bit > 8:
            return "conv1's output is wider than 8 bits"
        return None

    def _stem_args(self, a1, w_int):
        """conv1 (block `a1`, int8 weights `w_int`) as the one-launch stem kernels take it, one block per plan: `in` NULL, 3 input
        channels, [Cout][32] weights"""
        wt = self._zeros(a1.Cout, 32, dtype=torch.int8, device=self.dev)
        wt.copy_(torch.from_numpy(pack_stem_u8_weights(w_int.detach().cpu().numpy().astype(np.int8), a1.Cout)))
        a = _lib.IncepConvArgs.from_buffer_copy(a1)   # conv1's bias, tables, clamp, output buffer and pitch
        a.in_, a.wgt, a.Cin = None, wt.data_ptr(), 3
        self._keep.append(a)
        return a

    def _ensure_u8(self, N, H, W):
        """the uint8 plan of the current batch shape: image buffer, table and the launch list"""
        if self._ops_u8 is not None:
            return
        if self._u8_why is not None:
            raise PlanNotApplicable(f"uint8 input: {self._u8_why}")
        self.x_u8 = self._zeros(N, H, W, 3, dtype=torch.uint8, device=self.dev)
        self.lut_dev = self._zeros(3, 256, dtype=torch.int8, device=self.dev)
        self._lut_key = None
        if not _lib.load().hawq_incep_stem_u8_ok(self.x_u8.data_ptr(), self.lut_dev.data_ptr(), C.byref(self._stem_a)):
            raise PlanNotApplicable("uint8 input: hawq_incep_stem_u8 refuses conv1")
        self._ops_u8 = self._write(u8=True)

    def forward_uint8(self, x_u8, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
        """uint8 NHWC images [N,H,W,3] (decoder output, after resize / crop) -> fp32 logits, equal bit for bit to ``self(x)`` with
        x = Normalize(mean, std)(ToTensor(image)) as the reference's data pipeline builds it; the fp32 tensor never exists."""
        if not x_u8.is_cuda:
            raise NotImplementedError("InceptionEngine: uint8 images must be on the MI355X (there is no CPU path)")
        if x_u8.dtype != torch.uint8 or x_u8.dim() != 4 or x_u8.shape[3] != 3:
            raise ValueError("expected a uint8 NHWC [N,H,W,3] tensor")
        return self._forward_uint8(x_u8, mean, std)

    def unit_output(self, name):
        """int64 NCHW numpy array of a unit's integer output (after its q_rescaling_activ) of the last forward."""
        t = self.unit_out[name]
        torch.cuda.synchronize(self.dev)
        a = t.buf.view(self.N, t.h, t.w, t.pitch)[..., :t.c].permute(0, 3, 1, 2)
        return a.cpu().numpy().astype(np.int64)
