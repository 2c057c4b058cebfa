"""Host side of the stage handover on the stride-2 grid (hawq_conv_args.out_sub): the engine's eligibility rule read off every
shipped graph, buffer extents of odd maps, and the struct field against the header.  No GPU."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _handover_strides(arch):
    """out_sub_stride() at every unit boundary of the float skeleton, as the engine asks it: {unit name: s} for the units whose
    last launch may subsample (the NEXT unit is a resize unit that reads its block input on a stride-s grid)."""
    from hawq_amd.engine import out_sub_stride
    from hawq_amd.skeleton import build_float_resnet
    net = build_float_resnet(arch)
    units = [(f"{sn}.{un}", u) for sn, stage in net.features.named_children() if sn.startswith("stage")
             for un, u in stage.named_children()]
    geom = lambda blk: (blk.conv.kernel_size[0], blk.conv.kernel_size[1], blk.conv.stride[0], blk.conv.padding[0])
    out = {}
    for (name, u), (_, nxt) in zip(units, units[1:]):
        if not nxt.resize_identity or u.resize_identity:
            continue
        s = out_sub_stride([geom(nxt.body.conv1), geom(nxt.identity_conv)])
        if s:
            out[name] = s
    return out


def test_eligibility_rule_on_every_shipped_graph():
    from hawq_amd.skeleton import ARCH
    want = {"resnet50": {"stage1.unit3": 2, "stage2.unit4": 2, "stage3.unit6": 2},
            "resnet101": {"stage1.unit3": 2, "stage2.unit4": 2, "stage3.unit23": 2},
            "resnet50b": {},   # the stride sits on the 3x3 conv2: conv1 reads every pixel
            "resnet18": {}}    # basic blocks: the first conv of a resize unit is a 3x3
    assert set(want) == set(ARCH)
    for arch in ARCH:
        assert _handover_strides(arch) == want[arch], arch


def test_eligibility_rule_corner_cases():
    from hawq_amd.engine import out_sub_stride
    assert out_sub_stride([(1, 1, 2, 0), (1, 1, 2, 0)]) == 2
    assert out_sub_stride([(1, 1, 3, 0), (1, 1, 3, 0)]) == 3
    assert out_sub_stride([(1, 1, 1, 0), (1, 1, 1, 0)]) == 0      # stage 1's first unit: nothing to skip
    assert out_sub_stride([(1, 1, 1, 0), (1, 1, 2, 0)]) == 0      # resnet50b
    assert out_sub_stride([(3, 3, 2, 1), (1, 1, 2, 0)]) == 0      # resnet18 / resnet34
    assert out_sub_stride([(1, 1, 2, 1), (1, 1, 2, 0)]) == 0      # a padded 1x1 reads other pixels
    assert out_sub_stride([(1, 1, 2, 0), (1, 1, 4, 0)]) == 0
    assert out_sub_stride([]) == 0


@pytest.mark.parametrize("n,s,want", [(56, 2, 28), (7, 2, 4), (9, 2, 5), (6, 2, 3), (10, 2, 5), (1, 2, 1), (7, 3, 3), (8, 3, 3)])
def test_buffer_extent_is_what_a_strided_1x1_conv_reads(n, s, want):
    from hawq_amd.engine import out_sub_extent
    assert out_sub_extent(n, s) == want == len(range(0, n, s)) == (n + 2 * 0 - 1) // s + 1


def test_out_sub_is_the_last_field_of_the_struct_and_matches_the_header(tmp_path):
    from hawq_amd import _lib
    assert _lib.ConvArgs._fields_[-1] == ("out_sub", ctypes.c_int32)
    hdr = os.path.join(ROOT, "include", "hawq_mi355.h")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\n'
                   'printf("%%zu %%zu %%zu\\n", sizeof(hawq_conv_args), offsetof(hawq_conv_args, out_sub), offsetof(hawq_conv_args, wgt2_k128));\n'
                   'return 0; }\n' % hdr)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(src)])
    size, off, prev = (int(v) for v in subprocess.check_output([str(exe)]).decode().split())
    assert size == ctypes.sizeof(_lib.ConvArgs) and off == _lib.ConvArgs.out_sub.offset
    assert off == prev + 8 and off == _lib.ConvArgs.wgt2_k128.offset + 8   # appended: every older field keeps its offset
    text = open(hdr).read()
    body = text[text.index("typedef struct hawq_conv_args {"):text.index("} hawq_conv_args;")]
    assert re.findall(r"\b(\w+);", body)[-1] == "out_sub"
    assert ctypes.sizeof(_lib.ExpandReduceArgs) == 2 * size + 8
    assert _lib.ConvArgs().out_sub == 0   # a zeroed block means what it always meant
