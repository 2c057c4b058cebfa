"""The split-K grouped InceptionV3 conv launch (hawq_amd/csrc/incep_splitk.hip, hawq_incep_conv_group_splitk) against the grouped launch
on tile 3, byte for byte over whole sentinel-filled buffers, and against exact host computations (float64 conv + the dyadic requant in
integers), on a slab pre-filled with garbage and on the workspace the first launch left.  The cases are the smallest shapes at which
cutting K can go wrong; helpers and the reference are those of the grouped launch's test."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import test_gpu_incep_group_kernels as G
from tests.test_gpu_incep_group_kernels import RAW, RQ2, SENTINEL, _group, _host, _lib, _m, _out_hw, _to_device

pytestmark = pytest.mark.gpu

# name -> (members, slice counts per run, members also checked against the host computation)
CASES = {
    "uneven": ([_m(1, 1, 0, 0, 1, 8, 8, 320, 80)], [(2,), (3,), (5,)], (0,)),                     # 5 steps: 3 + 2, 2 + 2 + 1, one each
    "straddle": ([_m(3, 3, 1, 1, 1, 9, 9, 48, 16)], [(2,), (7,)], (0,)),                          # 27 units, 7 steps: slices start mid-tap
    "rect_17": ([_m(1, 7, 0, 3, 1, 17, 17, 160, 160), _m(7, 1, 3, 0, 1, 17, 17, 160, 192)], [(4, 6)], (1,)),   # 18 steps, P = 289 N
    "stride2": ([_m(3, 3, 0, 0, 2, 9, 9, 64, 96)], [(3,)], (0,)),                                 # 9 steps
    # the grouped launch's concat_level with Cin 256 (4 steps; its Cin 64 is one step, which has no 2 or 4 slices): unsplit beside split
    "concat_level": ([_m(1, 1, 0, 0, 1, 8, 8, 256, 64, RQ2, 16, "cat", 192, 0), _m(1, 1, 0, 0, 1, 8, 8, 256, 48),
                      _m(1, 1, 0, 0, 1, 8, 8, 256, 96, RAW), _m(1, 1, 0, 0, 1, 8, 8, 256, 32, RQ2, 16, "cat", 192, 160)], [(1, 2, 4, 1)], (1, 2, 3)),
    "pair_8": ([_m(3, 3, 1, 1, 1, 8, 8, 448, 384, RQ2, 16)], [(16,)], (0,)),                      # 63 steps: q = 4, the last slice 3
    "eight": ([_m(1, 1, 0, 0, 1, 5, 5, 128, 16) for _ in range(8)], [(2,) * 8], (7,)),            # 2 steps
}
PARAMS = [pytest.param(name, s, id=f"{name}-{'_'.join(map(str, s))}") for name, (_, runs, _) in CASES.items() for s in runs]


def _workspace(L, g, s):
    sb, cb = C.c_int64(), C.c_int64()
    assert L.hawq_incep_conv_group_splitk_workspace(C.byref(g), 3, s, C.byref(sb), C.byref(cb)) == 0, L.hawq_last_error()
    return torch.full((sb.value,), 0x5b, dtype=torch.uint8, device="cuda"), torch.zeros(cb.value // 4, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("name,slices", PARAMS)
def test_split_launch_equals_the_grouped_launch_and_the_host(name, slices, N, monkeypatch):
    L, (members, _, checked), case = _lib().load(), CASES[name], f"splitk_{name}"
    # the grouped launch's helpers make operands, buffers and argument blocks per named case of its table: in it while this test runs
    monkeypatch.setitem(G.CASES, case, (members, checked))
    ops = G._operands(case, N)
    dev, st, s = _to_device(ops), torch.cuda.current_stream().cuda_stream, (C.c_int32 * 8)(*slices)
    first, second, plain = G._buffers(case, N), G._buffers(case, N), G._buffers(case, N)
    g = _group(G._args(case, N, dev, first))
    assert L.hawq_incep_conv_group_splitk_ok(C.byref(g), 3, s) == 1
    slab, counters = _workspace(L, g, s)
    assert L.hawq_incep_conv_group_splitk(C.byref(g), 3, s, slab.data_ptr(), counters.data_ptr(), st) == 0, L.hawq_last_error()
    torch.cuda.synchronize()
    assert not counters.any()
    g2 = _group(G._args(case, N, dev, second))   # the workspace as the first launch left it
    assert L.hawq_incep_conv_group_splitk(C.byref(g2), 3, s, slab.data_ptr(), counters.data_ptr(), st) == 0, L.hawq_last_error()
    assert L.hawq_incep_conv_group(C.byref(_group(G._args(case, N, dev, plain))), 3, st) == 0, L.hawq_last_error()
    torch.cuda.synchronize()
    assert not counters.any()
    for key in plain:
        assert torch.equal(first[key], plain[key]), f"buffer {key} differs from the grouped launch's"
        assert torch.equal(second[key], plain[key]), f"buffer {key} of the second launch differs"
    for i in checked:
        mb = members[i]
        Ho, Wo = _out_hw(mb["g"])
        got = first[mb["out"] or f"out{i}"].cpu().numpy().reshape(N, Ho, Wo, mb["ldo"])[..., mb["c_off"]:mb["c_off"] + mb["g"][8]]
        want = _host(mb, ops[i])
        assert np.array_equal(got, want), f"member {i} differs from the host computation"
        assert len(np.unique(want)) > 8   # not all clamped away


@pytest.mark.parametrize("name,slices,tile,why", [("uneven", (4,), 3, b"empty slice"), ("concat_level", (1, 1, 1, 1), 3, b"more than one slice"),
                                                  ("uneven", (2,), 1, b"tile 3")])
def test_a_refused_call_is_an_error_and_writes_nothing(name, slices, tile, why, monkeypatch):
    L = _lib().load()
    monkeypatch.setitem(G.CASES, f"splitk_{name}", CASES[name][::2])
    bufs = G._buffers(f"splitk_{name}", 1)
    g, s = _group(G._args(f"splitk_{name}", 1, _to_device(G._operands(f"splitk_{name}", 1)), bufs)), (C.c_int32 * 8)(*slices)
    slab, counters = torch.full((1 << 20,), 0x5b, dtype=torch.uint8, device="cuda"), torch.zeros(64, dtype=torch.int32, device="cuda")
    assert L.hawq_incep_conv_group_splitk_ok(C.byref(g), tile, s) == 0
    rc = L.hawq_incep_conv_group_splitk(C.byref(g), tile, s, slab.data_ptr(), counters.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc != 0 and why in L.hawq_last_error()
    torch.cuda.synchronize()
    assert all((t == SENTINEL).all() for t in bufs.values()) and (slab == 0x5b).all() and not counters.any()
