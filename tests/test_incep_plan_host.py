"""The grouped launch order of the InceptionV3 engine (hawq_amd/engine_inception.py: Launch, grouped_order) as a pure function of the
records' tags: on a small network written out by hand, and on the tags that unit_convs / conv_levels give for the real model.
No model weights on a device, no library, no ctypes: no GPU needed."""
from itertools import chain, combinations

import pytest

from hawq_amd.engine_inception import Launch, conv_levels, grouped_order, unit_convs


def _rec(name, kind="other", ref=None, place="stem", level=0):
    return Launch(name, None, kind, ref, place, level)


def _conv(ref, place, level=0):
    return _rec("hawq_incep_conv", "conv", ref, place, level)


def _pool(name, place, level=0, op=0):
    return _rec(name, "pool", op, place, level)


# record index: the small network in the default plan's order.  Unit 0 is an 8 x 8-type unit whose six convs sit at the LEVELS of
# tests/test_incep_group_host.py (the stem here holds no conv, so the indices are the same); unit 1 has a max-pool branch, one level of
# two convs and a single-conv level.
NET = [
    _rec("hawq_fakequant_f32"),                          # 0
    _rec("hawq_f32_nchw_to_q_nhwc"),                     # 1
    _pool("hawq_incep_maxpool3s2", "stem", op=1),        # 2
    _pool("hawq_incep_requant", 0),                      # 3   unit 0, branch 0: 1x1
    _conv(0, 0, 1),                                      # 4
    _pool("hawq_incep_requant", 0),                      # 5   branch 1: 1x1, then the 1x3 / 3x1 pair and its inner concat
    _conv(1, 0, 1),                                      # 6
    _conv(2, 0, 2),                                      # 7
    _conv(3, 0, 2),                                      # 8
    _pool("hawq_incep_requant", 0, 2),                   # 9   the inner-concat requant: the level of its pair
    _pool("hawq_incep_requant", 0),                      # 10  branch 2: 1x1, 3x3
    _conv(4, 0, 1),                                      # 11
    _conv(5, 0, 2),                                      # 12
    _pool("hawq_incep_avgpool_branch", 0, op=2),         # 13  branch 3: the average-pool entry
    _pool("hawq_incep_requant", 1),                      # 14  unit 1, branch 0: 3x3 / 2
    _conv(6, 1, 1),                                      # 15
    _pool("hawq_incep_requant", 1),                      # 16  branch 1: 1x1, 3x3 / 2
    _conv(7, 1, 1),                                      # 17
    _conv(8, 1, 2),                                      # 18
    _pool("hawq_incep_maxpool3s2", 1, op=1),             # 19  branch 2: the max pool
    _pool("hawq_incep_global_avgpool", "head", op=3),    # 20
    _conv(9, "head"),                                    # 21
]
LEVELS = [[0, 1, 4], [2, 3, 5], [6, 7], [8]]             # conv indices per (unit, level); the first two are test_incep_group_host's
CANDIDATES = [lv for lv in LEVELS if len(lv) >= 2]
REC = {r.ref: i for i, r in enumerate(NET) if r.kind == "conv"}   # conv index -> record index

S = lambda *idx: [(False, i) for i in idx]   # noqa: E731  records issued alone
G = lambda g: [(True, g)]                    # noqa: E731  a grouped launch


def test_the_small_network_is_what_it_says():
    assert [r.ref for r in NET if r.kind == "conv"] == list(range(10))
    for u, base in ((0, 0), (1, 2)):
        convs = [r for r in NET if r.kind == "conv" and r.place == u]
        for d in sorted({r.level for r in convs}):
            assert [r.ref for r in convs if r.level == d] == LEVELS[base + d - 1]
    assert [r.place for r in NET].count("stem") == 3 and [r.place for r in NET].count("head") == 2


def test_order_without_groups():
    assert grouped_order(NET, []) == S(0, 1, 2,
                                       3, 5, 10, 13, 4, 6, 11, 7, 8, 12, 9,
                                       14, 16, 19, 15, 17, 18,
                                       20, 21)


def test_order_with_one_group():
    assert grouped_order(NET, [([0, 1, 4], 3)]) == S(0, 1, 2, 3, 5, 10, 13) + G(0) + S(7, 8, 12, 9, 14, 16, 19, 15, 17, 18, 20, 21)
    assert grouped_order(NET, [([7, 6], 4)]) == S(0, 1, 2, 3, 5, 10, 13, 4, 6, 11, 7, 8, 12, 9, 14, 16, 19) + G(0) + S(18, 20, 21)


def test_order_with_both_levels_of_a_unit_grouped_members_in_any_order():
    groups = [([5, 2, 3], 4), ([4, 1, 0], 3)]   # GROUPS of test_incep_group_host, level 2 listed first
    assert grouped_order(NET, groups) == S(0, 1, 2, 3, 5, 10, 13) + G(1) + G(0) + S(9, 14, 16, 19, 15, 17, 18, 20, 21)


def _subsets(items):
    return chain.from_iterable(combinations(items, n) for n in range(len(items) + 1))


@pytest.mark.parametrize("chosen", list(_subsets(CANDIDATES)), ids=lambda c: "+".join("".join(map(str, lv)) for lv in c) or "none")
def test_every_record_is_issued_exactly_once_and_in_a_legal_order(chosen):
    groups = [(list(reversed(lv)), 3) for lv in chosen]
    order = grouped_order(NET, groups)
    assert len(order) == len(NET) - sum(len(lv) - 1 for lv in chosen)
    assert sorted(g for is_group, g in order if is_group) == list(range(len(groups)))
    # position of every record: its own entry, or its group's
    pos = {}
    for p, (is_group, i) in enumerate(order):
        for rec in ([REC[c] for c in groups[i][0]] if is_group else [i]):
            assert rec not in pos
            pos[rec] = p
    assert sorted(pos) == list(range(len(NET)))
    # stem and head keep their places, and nothing crosses a unit boundary: the places are met in the default plan's sequence
    assert [pos[i] for i in (0, 1, 2)] == [0, 1, 2] and [pos[i] for i in (20, 21)] == [len(order) - 2, len(order) - 1]
    for i, j in zip(range(len(NET)), range(1, len(NET))):
        if NET[i].place != NET[j].place:
            assert max(pos[k] for k in range(len(NET)) if NET[k].place == NET[i].place) < \
                min(pos[k] for k in range(len(NET)) if NET[k].place == NET[j].place)
    for u in (0, 1):
        recs = [i for i, r in enumerate(NET) if r.place == u]
        convs = [i for i in recs if NET[i].kind == "conv"]
        for i in recs:   # level 0 before level 1, level d before level d + 1 (a group of a level counts once)
            for j in convs:
                if NET[i].level < NET[j].level:
                    assert pos[i] < pos[j], (i, j)
        for d in {NET[i].level for i in recs}:   # the default order within level 0 and among the convs of a level
            same = [pos[i] for i in recs if NET[i].level == d and (d == 0 or i in convs)]
            assert same == sorted(same)
    # the inner-concat requant directly follows the level of its pair (all of level 2, conv 5 of the other branch included)
    assert pos[9] == max(pos[7], pos[8], pos[12]) + 1


# ---------------------------------------------------------------------- the real model: tags from unit_convs / conv_levels
@pytest.fixture(scope="module", params=["uniform8", "uniform4"])
def model(request):
    from hawq_amd.api import build_quantized_resnet
    return build_quantized_resnet("inceptionv3", request.param, seed=0)


def _tags(model):
    """The tags of the 147 records as the engine emits them: the stem (the input QuantAct's two launches, 5 convs, 2 pools), per unit
    and branch what ``InceptionEngine._unit`` emits, the head.  Returns (records, conv levels as lists of conv indices)."""
    from hawq_amd.q_inceptionv3 import Q_AvgPoolBranch, Q_ConvSeq3x3Branch, Q_MaxPoolBranch
    recs, n = [_rec("hawq_fakequant_f32"), _rec("hawq_f32_nchw_to_q_nhwc")], 0
    for name in ("c", "c", "c", "p", "c", "c", "p"):
        recs.append(_conv(n, "stem") if name == "c" else _pool("hawq_incep_maxpool3s2", "stem", op=1))
        n += name == "c"
    levels = []
    for u, (_, unit) in enumerate(model.units()):
        ucs = unit_convs(unit)
        levels += [[n + i for i in lv] for lv in conv_levels(unit)]
        for bi, br in enumerate(unit.branches.children()):
            mine = [(n + i, d) for i, (_, b, d) in enumerate(ucs) if b == bi]
            if isinstance(br, Q_MaxPoolBranch):
                recs.append(_pool("hawq_incep_maxpool3s2", u, op=1))
            else:
                recs.append(_pool("hawq_incep_avgpool_branch", u, op=2) if isinstance(br, Q_AvgPoolBranch) else _pool("hawq_incep_requant", u))
                recs += [_conv(c, u, d) for c, d in mine]
                if isinstance(br, Q_ConvSeq3x3Branch):
                    recs.append(_pool("hawq_incep_requant", u, mine[-1][1]))
        n += len(ucs)
    recs += [_pool("hawq_incep_global_avgpool", "head", op=3), _conv(n, "head"), _rec("hawq_acc_nhwc_to_f32_nchw", place="head")]
    return recs, levels


def test_the_real_models_launch_counts(model):
    recs, levels = _tags(model)
    assert len(recs) == 147 and sum(r.kind == "conv" for r in recs) == 95 and sum(r.kind == "pool" for r in recs) == 49
    cands = [lv for lv in levels if len(lv) >= 2]
    assert len(cands) == 27 and sum(map(len, cands)) == 74
    assert grouped_order(recs, []) != [(False, i) for i in range(147)] and len(grouped_order(recs, [])) == 147
    order = grouped_order(recs, [(lv, 3) for lv in cands])
    assert len(order) == 147 - 47 == 100 and [g for is_group, g in order if is_group] == list(range(27))
    assert sorted(i for is_group, i in grouped_order(recs, [])) == list(range(147))
