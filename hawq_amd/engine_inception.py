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


def make_plan(batch, keys, num_tiles, tiles, us, groups=None, fan_out=None):
    """the dict ``export_plan`` returns: batch shape (N, H, W), digest of the launch list, tile inventory, chosen id per conv launch
    and, for the record, the measured microseconds per launch and tile id (``us[i][str(tile)]``); with `groups` (a grouped engine's
    ``{"convs": [indices into the launch list], "tile": id, "us": {...}}`` entries) also the ``"groups"`` field, and with `fan_out`
    (a fan-out engine's ``{"unit": k, "tiles": {launch: id}, "us": {...}}`` entries) the ``"fan_out"`` field"""
    plan = {"network": "inceptionv3", "batch": [int(v) for v in batch], "launches": launch_digest(keys), "n_launches": len(keys),
            "num_tiles": int(num_tiles), "tiles": [int(t) for t in tiles],
            "us": [{str(t): round(float(v), 3) for t, v in sorted(d.items(), key=lambda kv: int(kv[0]))} for d in us]}
    if groups is not None:
        plan["groups"] = [{"convs": [int(c) for c in g["convs"]], "tile": int(g["tile"]),
                           "us": {str(k): round(float(v), 3) for k, v in g.get("us", {}).items()}} for g in groups]
    if fan_out is not None:
        plan["fan_out"] = [{"unit": int(f["unit"]), "tiles": {str(k): int(t) for k, t in f["tiles"].items()},
                            "us": {str(k): round(float(v), 3) for k, v in f.get("us", {}).items()}} for f in fan_out]
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


def fan_boundaries(launches):
    """The boundary in front of every unit of `launches`, in unit order, read from the records' tags and argument blocks alone:
    * ``"requants"``: the unit's level-0 ``hawq_incep_requant`` records (the ``q_input_act`` of its conv branches), as indices;
    * ``"slices"``: ``(c_off, C, producer)`` for every slice of the buffer they read that an earlier record writes, by channel: the
      index of the conv record that produced it (REQUANT2, 16 bits, into that buffer), or None for a pool / requant record;
    * ``"producers"``: per such conv record index its fan targets, one per entry requant and in their order:
      ``(out, ldo, (m, ek, lo, hi), c_off, Cout)`` - that record's output buffer, pitch and ``post`` table, and where the producer's
      channels go in it;
    * ``"residual"``: the channel ranges ``(in_off, C)`` of the input that no conv produced, adjacent ones merged - what is left for
      the entry requants to do;
    * ``"candidate"``: at least one slice is conv-produced (and the entry requants are plain: one 16-bit source and range, ``post``
      only, int8 out)."""
    out = []
    for k in sorted({r.place for r in launches if isinstance(r.place, int)}):
        entry = [i for i, r in enumerate(launches)
                 if r.place == k and r.level == 0 and r.kind == "pool" and r.name == "hawq_incep_requant"]
        b = {"unit": k, "requants": entry, "slices": [], "producers": {}, "residual": [], "candidate": False}
        out.append(b)
        if not entry:
            continue
        blocks = [launches[i].args[0] for i in entry]
        f = blocks[0]
        src, pitch, lo, hi = f.in_, f.in_pitch, f.in_off, f.in_off + f.C
        plain = all((a.in_, a.in_pitch, a.in_off, a.C, a.in_bits, a.out_bits, a.pre, a.post) == (src, pitch, lo, f.C, 16, 8, 0, 1)
                    for a in blocks)
        for i, r in enumerate(launches[:entry[0]]):
            if r.kind not in ("conv", "pool"):
                continue
            a = r.args[0]
            if (a.out, a.ldo, a.out_bits) != (src, pitch, 16) or (r.kind == "conv" and a.epilogue == _lib.INCEP_RAW):
                continue
            if r.kind == "conv":
                b["slices"].append((a.c_off, a.Cout, i if a.epilogue == _lib.INCEP_REQUANT2 else None))
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


class _T:
    """An NHWC integer tensor of the plan: buffer, spatial size, channels, row pitch, scale."""

    def __init__(self, buf, h, w, c, pitch, scale, bits):
        self.buf, self.h, self.w, self.c, self.pitch, self.scale, self.bits = buf, h, w, c, pitch, scale, bits


class InceptionEngine(GraphRunner):
    def __init__(self, model, use_graph: bool = True, tune: bool = False, plan=None, fast_pools: bool = False,
                 fused_stem: bool = False, grouped: bool = False, fan_out: bool = False):
        self.model, self.use_graph = model, use_graph
        self.tune, self.plan, self.fast_pools, self.fused_stem = bool(tune), plan, bool(fast_pools), bool(fused_stem)
        self.grouped, self.fan_out = bool(grouped), bool(fan_out)
        self.group_launches, self.group_candidates = [], []
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
            out = _T(self._zeros(self.N * Ho * Wo * cout_p, dtype=torch.int8 if bits == 8 else torch.int16, device=self.dev),
                     Ho, Wo, Cout, cout_p, s_out, bits)
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
        self._emit("hawq_incep_conv", (a,), "conv", len(self._convs), level)
        return out

    def _requant_input(self, act, src: _T):
        """a branch's q_input_act of width <= 8: int16 unit tensor -> int8 branch tensor"""
        if act.activation_bit > 8:
            raise PlanNotApplicable("a 16-bit conv-branch input")
        s = _scale(act)
        out = _T(self._zeros(self.N * src.h * src.w * src.pitch, dtype=torch.int8, device=self.dev), src.h, src.w, src.c,
                 src.pitch, s, 8)
        self._pool("hawq_incep_requant", src, out.buf, 8, src.pitch, 0, src.pitch, src.h, src.w,
                   post=(*_scalar_table(src.scale, s), *_rng(act)))
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
        dst = _T(self._zeros(self.N * Ho * Wo * cu, dtype=torch.int16, device=self.dev), Ho, Wo, cu, cu, s_u, 16)
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
        self._choice = (None, None, None)    # the default plan's: no tiles, no groups, no fan-out, the default order
        self._ops, self._keep, self.unit_out = [], [], {}
        self.conv_tiles, self.conv_us = None, None
        self.group_launches, self.group_candidates = [], []
        self.fan_launches, self.fan_candidates, self.residual_requants = [], [], []
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
                y = _T(self._zeros(N * h * w * x.pitch, dtype=x.buf.dtype, device=dev), h, w, x.c, x.pitch, x.scale, x.bits)
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

    def _residual_args(self, r, off, c):
        """a fresh block for entry requant `r` on the input channels off .. off + c - 1 only"""
        a = _lib.IncepPoolArgs.from_buffer_copy(r.args[0])
        a.c_off, a.in_off, a.C = a.c_off + off - a.in_off, off, c
        return a

    # ------------------------------------------------------------------ the choice
    def _choose(self, batch):
        """What a plan decides, as one value: (tile id per conv launch, or None; grouped launches [(member conv indices, tile)], or
        None on an engine without ``grouped``; fan-out boundaries [(boundary, {producer launch: tile})], or None on an engine
        without ``fan_out``).  From ``self.plan``, else from timing (``tune``), else the defaults: no tiles, every level of two or
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
        return self.conv_tiles, groups, self._choose_fans(self.conv_tiles, groups) if self.fan_out else None

    def _choose_fans(self, tiles, groups):
        """the third component: from the plan's ``"fan_out"`` field if it has one, else timed against the plain launches (``tune``),
        else every candidate boundary on the default tiles (a tile plan without the field fixes the other convs' tiles only)"""
        cands = {b["unit"]: b for b in fan_boundaries(self._launches) if b["candidate"]}
        sets = {k: self._fan_sets(b, groups) for k, b in cands.items()}
        if self.plan is not None and "fan_out" in self.plan:
            by_key = {(k, fan_key(s)): s for k in cands for s in sets[k]}
            got = check_fan_out(self.plan["fan_out"], {k: [fan_key(s) for s in sets[k]] for k in cands},
                                lambda k, key, t: self._fan_ok(by_key[k, key], cands[k], t))
            us = {e["unit"]: dict(e.get("us", {})) for e in self.plan["fan_out"]}
            self.fan_candidates = [{"unit": k, "tiles": dict(t), "us": us[k], "kept": True} for k, t in got]
            return [(cands[k], {by_key[k, key]: t for key, t in tl.items()}) for k, tl in got]
        accepted = {k: {s: [t for t in _FAN_TILES if self._fan_ok(s, b, t)] for s in sets[k]} for k, b in cands.items()}
        able = [k for k in cands if all(accepted[k][s] for s in sets[k])]   # a boundary with a refused producer launch is not chosen
        if self.tune and self.plan is None:
            for k, rec in zip(able, self._time_fans([cands[k] for k in able], [accepted[k] for k in able], tiles, groups)):
                self.fan_candidates.append({"unit": k, **rec})
        else:
            self.fan_candidates = [{"unit": k, "tiles": {fan_key(s): accepted[k][s][0] for s in sets[k]}, "us": {}, "kept": True}
                                   for k in able]
        return [(cands[f["unit"]], {s: f["tiles"][fan_key(s)] for s in sets[f["unit"]]}) for f in self.fan_candidates if f["kept"]]

    def _time_fans(self, bounds, accepted, tiles, groups):
        """Per boundary of `bounds`, on the real buffers as ``_time`` left them (every launch here is a pure function of buffers it
        does not write): ``"plain"``, the microseconds of its producer launches as (tiles, groups) issue them followed by its entry
        requants, one block; every producer launch with its fan on every accepted tile (``"<launch>@<tile>"``); and ``"fan"``, one
        block of the fan-out launches on their fastest tiles followed by the residual requants.  Kept if fan < plain."""
        sp, lib, out = self.stream.cuda_stream, _lib.load(), []

        def pool(a, ref, name):
            fast = self.fast_pools and lib.hawq_incep_pool_v_ok(C.byref(a), ref)
            return partial(_lib.call, "hawq_incep_pool_v", C.byref(a), ref, sp) if fast else partial(_lib.call, name, C.byref(a), sp)

        def block(ops):
            def run():
                for op in ops:
                    op()
            self.n_timing_launches += (_TUNE_WARMUP + _TUNE_REPS) * len(ops)
            return ev.median_us(run, _TUNE_REPS, _TUNE_WARMUP)

        with EventTimer(sp, _TUNE_REPS + 1) as ev:
            torch.cuda.synchronize(self.dev)
            with torch.cuda.stream(self.stream):
                for b, acc in zip(bounds, accepted):
                    gtile = {tuple(c): t for c, t in groups or []}
                    plain, fan, us, chosen, keep = [], [], {}, {}, []
                    for s in acc:
                        if s in gtile:
                            g = self._group_args(s)
                            keep.append(g)
                            plain.append(partial(_lib.call, "hawq_incep_conv_group", C.byref(g), int(gtile[s]), sp))
                        else:
                            plain.append(partial(_lib.call, "hawq_incep_conv_tiled", C.byref(self._convs[s[0]].args[0]), int(tiles[s[0]]), sp))
                        g, f = self._fan_args(s, b)
                        keep += [g, f]
                        for t in acc[s]:
                            us[f"{fan_key(s)}@{t}"] = block([partial(_lib.call, "hawq_incep_conv_group_fan", C.byref(g), f, t, sp)])
                        chosen[s] = min(acc[s], key=lambda t: (us[f"{fan_key(s)}@{t}"], t))
                        fan.append(partial(_lib.call, "hawq_incep_conv_group_fan", C.byref(g), f, chosen[s], sp))
                    for i in b["requants"]:
                        r = self._launches[i]
                        plain.append(pool(r.args[0], r.ref, r.name))
                        for off, c in b["residual"]:
                            a = self._residual_args(r, off, c)
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
        torch.cuda.synchronize(self.dev)
        return convs, groups

    def export_plan(self):
        """The conv tile choice of the current batch shape (and, of a grouped engine, its grouped launches) as a JSON-serialisable
        dict (``make_plan``), for ``plan=``."""
        if self.conv_tiles is None:
            raise RuntimeError("export_plan: no tuned plan (build the engine with tune=True or plan=... and run a forward first)")
        groups = [g for g in self.group_candidates if g["kept"]] if self.grouped else None
        fans = [f for f in self.fan_candidates if f["kept"]] if self.fan_out else None
        return make_plan(self._batch, self.conv_launches, _lib.load().hawq_incep_conv_num_tiles(), self.conv_tiles, self.conv_us,
                         groups, fans)

    # ------------------------------------------------------------------ the writer
    def _write(self, u8=False):
        """The callables of one chain, from the records, ``_choice`` and the engine's options - the only place that makes one.  Per
        record: a conv alone, tiled with its chosen id or as a member of a grouped launch; a pool on its named entry point or, under
        ``fast_pools`` where the library takes it, on ``hawq_incep_pool_v``.  The stem's head (the records up to conv1) as it stands,
        as one ``hawq_incep_stem_f32`` (``fused_stem``) or, for the uint8 chain, as one ``hawq_incep_stem_u8`` in front of the fp32
        chain's own callables.  The records' order, or with groups ``grouped_order``.  The fp32 chain leaves ``_at`` (record -> index
        of the launch that covers it) and ``group_launches``."""
        tiles, groups, fans = self._choice
        lib, sp, launches = _lib.load(), self.stream.cuda_stream, self._launches
        fan_of = {s: (b, t) for b, by_set in fans or [] for s, t in by_set.items()}           # producer launch -> its boundary, tile
        entry = {i: b for b, _ in fans or [] for i in b["requants"]}                          # entry requant record -> its boundary

        def op(name, *args):
            return partial(_lib.call, name, *args, sp)

        def single(r):
            if r.kind == "other":
                return op(r.name, *r.args)
            a = C.byref(r.args[0])
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
        n_stem, issued, fanned, residual = len(ops), [], [], []
        at = {r: min(i, n_stem - 1) for i, r in enumerate(launches[:head])}
        order = [(False, i) for i in range(len(launches))] if groups is None else grouped_order(launches, groups)
        for is_group, i in order[head:]:   # the stem stays in place in either order
            r = None if is_group else launches[i]
            convs, tile = groups[i] if is_group else ([r.ref], None) if r.kind == "conv" else (None, None)
            if convs is not None and tuple(convs) in fan_of:   # a producer launch of a chosen boundary, alone or grouped
                b, tile = fan_of[tuple(convs)]
                g, f = self._fan_args(convs, b)
                self._keep += [g, f]
                at.update((self._convs[c], len(ops)) for c in convs)
                ops.append(op("hawq_incep_conv_group_fan", C.byref(g), f, int(tile)))
                fanned.append((b["unit"], list(convs), int(tile)))
                if is_group:
                    issued.append((list(convs), int(tile)))
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
                    a = self._residual_args(r, off, c)
                    self._keep.append(a)
                    fast = self.fast_pools and lib.hawq_incep_pool_v_ok(C.byref(a), r.ref)
                    ops.append(op("hawq_incep_pool_v", C.byref(a), r.ref) if fast else op(r.name, C.byref(a)))
                    residual.append((b["unit"], i, off, c))
            else:
                at[r] = len(ops)
                ops.append(single(r))
        self._at, self._tail, self.group_launches = at, ops[n_stem:], issued
        self.fan_launches, self.residual_requants = fanned, residual
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
