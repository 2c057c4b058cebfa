"""The launch plan of the ResNet engine (engine.py) as data: pure host code - no torch, no library, no environment.

A recorded plan is the dict ``IntegerEngine.export_plan()`` returns (profiles/plans.json, bench.py --plan, hawq_amd.dist.share_plan):
dotted strings in launch order, chain 0's at the top level and one entry per chain under ``per_chain`` when the chains differ.
``decode`` checks such a dict against a build and gives the ``ChainChoice`` of one chain, ``encode`` is its inverse, ``from_env`` puts
the measurement switches into the same form.  In memory the decisions of a chain exist only as a ``ChainChoice``:
``IntegerEngine._choice()`` reads one off the launch list, ``IntegerEngine._apply_choice()`` alone writes one into it.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

# launches that recorded plans may still list as tuned although the engine now runs them on a kernel with nothing to tune
UNTUNED_SINCE = ("quant_output",)
SWITCHES = {"HAWQ_TILES": "tiles", "HAWQ_ER_TILES": "fused_variants", "HAWQ_ER_SPLIT_TILES": "fused_split_tiles", "HAWQ_SPLITK": "splitk"}


class StalePlan(ValueError):
    """A recorded plan does not fit the launch list / kernel inventory of this build: the engine falls back to tuning."""


class ChainChoice(NamedTuple):
    """What the tuner decides for ONE chain.  ``tiles`` / ``variants`` None: not given, to be timed (``decode`` only)."""
    tiles: Optional[list]   # tile id of every conv launch
    variants: Optional[list]   # fused variant of every expand(-> reduce) pair, 0 = two launches
    split_tiles: list       # (expand tile, reduce tile) of every pair's two-launch form
    splitk: list            # K slices (0 = not split) of every conv launch, then (expand, reduce) of every pair's two-launch form


def expand_in8_of(plan) -> str:
    """Storage policy a plan's launch list was built with (a plan without the key predates policy "2": recorded under "1")."""
    return str(plan.get("expand_in8") or "1")


def from_env(environ) -> dict:
    """The measurement switches set in the mapping `environ`, as the strings of a (partial) recorded plan."""
    return {key: environ[var] for var, key in SWITCHES.items() if environ.get(var)}


def decode(plan, chain, conv_names, n_pairs, num_tiles, variant_counts, untuned=UNTUNED_SINCE) -> ChainChoice:
    """The choice `plan` records for chain `chain` of a build with the conv launches `conv_names`, `n_pairs` pairs whose fused
    kernels come in `variant_counts` variants, and a library of `num_tiles` conv tiles; StalePlan if it was recorded for another."""
    if int(plan.get("num_conv_tiles", -1)) != num_tiles:
        raise StalePlan("recorded for a library with another tile inventory")
    # chains whose tuned choices differ (uneven sub-batches, layers only one tile takes) are recorded one by one
    per = plan.get("per_chain") or []
    if per and chain >= len(per):
        raise StalePlan(f"the recorded plan lists {len(per)} chains")

    def ints(key):   # (an empty per-chain string falls back to the top level; "chains" is never read per chain)
        s = per[chain].get(key) if per and per[chain].get(key) not in (None, "") else plan.get(key)
        return None if s in (None, "") else [int(v) for v in str(s).split(".")]
    tiles, names = ints("tiles"), plan.get("conv_launches")
    if names is not None:
        # The ONLY relaxation: the recorded list minus the launches no longer tuned must be this build's list exactly - a superset
        # recorded for a larger network (resnet101's plan on resnet50) is stale.  The tiles are then replayed by NAME.
        if [n for n in names if n not in untuned] != list(conv_names):
            raise StalePlan("recorded for another launch list (other network, schedule or storage rule)")
        if tiles is not None and len(tiles) == len(names):
            by_name = dict(zip(names, tiles))
            tiles = [by_name[n] for n in conv_names]
    if tiles is not None and len(tiles) != len(conv_names):
        raise StalePlan(f"the recorded plan lists {len(tiles)} tiles, this plan has {len(conv_names)} conv launches")
    counts = plan.get("pair_variant_counts")
    if counts is not None and list(counts) != list(variant_counts):
        raise StalePlan("the fused expand(-> reduce) kernels of this build are numbered differently")
    variants = ints("fused_variants") or (None if tiles is None else [1] * n_pairs)
    split = ints("fused_split_tiles")   # tiles of a pair's two-launch form (what runs when the recorded variant is 0)
    if split is None and variants is not None and 0 in variants:
        raise StalePlan("the recorded plan runs a pair as two launches but lists no tiles for them")
    if (variants is not None and len(variants) != n_pairs) or (split is not None and len(split) != 2 * n_pairs):
        raise StalePlan(f"the recorded fused variants / two-launch tiles are not those of {n_pairs} pairs")
    n = len(conv_names) + 2 * n_pairs
    splitk = ints("splitk") or [0] * n   # absent (every plan recorded before split-K existed): no launch is split
    if len(splitk) != n:
        raise StalePlan(f"the recorded plan lists {len(splitk)} split-K entries, this plan has {n} launches")
    return ChainChoice(tiles, variants, list(zip(split[::2], split[1::2])) if split else [(0, 0)] * n_pairs, splitk)


def encode(batch, chains, expand_in8, choices, conv_names, pair_names, num_tiles, variant_counts) -> dict:
    """The recorded plan of a build whose chains made `choices` (one ChainChoice per chain).  "splitk": the K-slice count of every conv
    launch in the order of "tiles", then two per pair in the order of "fused_variants" (its two-launch form: expand, reduce), 0 =
    hawq_conv2d; only written when some launch is split - then every chain's entry names its own counts, zeros included."""
    any_split = any(any(c.splitk) for c in choices)

    def strings(c, splitk):
        out = {"tiles": ".".join(map(str, c.tiles)), "fused_variants": ".".join(map(str, c.variants)),
               "fused_split_tiles": ".".join(f"{a}.{b}" for a, b in c.split_tiles)}
        return dict(out, splitk=".".join(map(str, c.splitk))) if splitk else out
    per = [strings(c, any_split) for c in choices] if len(choices) > 1 else []
    # the top-level strings are chain 0's; "per_chain" is only written when another chain runs something else
    extra = {"per_chain": per} if any(p != per[0] for p in per[1:]) else {}
    return {"batch": int(batch), "chains": int(chains), "expand_in8": expand_in8, **extra, **strings(choices[0], any(choices[0].splitk)),
            "conv_launches": list(conv_names), "pair_launches": list(pair_names),
            # guards against replaying a plan on a build whose kernels are numbered differently
            "num_conv_tiles": int(num_tiles), "pair_variant_counts": [int(v) for v in variant_counts]}
