"""The device front end of the JPEG decoder on the MI355X (hawq_jpeg_front_scan, hawq_jpeg_front_fill, ``decode_jpeg_batch(front_end=
"device")``): the scan kernel's records equal its host twin's bit for bit, the filled blob equals the planner's byte
for byte, and the option changes neither an output byte nor the fallback list.  The C ABI runs with every buffer between poisoned
guards (tests/guard.py), with both poisons.  The fixtures and the corpus files have passed the same walker on the host under the
sanitizers (tests/test_jpeg_front_host.py); the other files differ from a fixture by a comment segment in front or by stream bytes."""
import functools

import numpy as np
import pytest
import torch

from tests import guard, jpeg_model
from tests import jpeg_front_corpus as F

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[0xA5, 0x5A], ids=["poisonA5", "poison5A"])
def arena(request):
    ar = guard.GuardArena("cuda", poison=request.param)
    yield ar
    ar.check()


class Staged:
    pass


def run_scan(ar, datas):
    """hawq_jpeg_front_scan on ``datas`` with files, table and records in the arena -> (info, what run_fill needs)"""
    from hawq_amd import _lib
    from hawq_amd.jpeg import _FINFO, pack_files
    s = Staged()
    s.table, buf, s.total = pack_files(datas)
    buf = buf.copy()
    for off, n in zip(s.table["offset"].tolist(), s.table["length"].tolist()):   # the bytes between two files belong to nobody
        buf[off + n:(off + n + 15) & ~15] = ar.poison
    s.files, s.table_dev = ar.put(buf[:s.total], "files"), ar.put(s.table.view(np.uint8), "table")
    s.info_dev = ar.empty(len(datas) * _FINFO.itemsize, torch.uint8, "info")
    _lib.call("hawq_jpeg_front_scan", s.files.data_ptr(), s.total, s.table_dev.data_ptr(), s.table.ctypes.data, len(datas), s.info_dev.data_ptr(),
              torch.cuda.current_stream().cuda_stream)
    ar.check()
    return s.info_dev.cpu().numpy().view(_FINFO), s


def run_fill(ar, s, info, files, out_offsets, out_bytes):
    """hawq_jpeg_front_fill for the accepted ``files`` into a blob in the arena, then the head as the Python path uploads it -> (layout, blob)"""
    from hawq_amd import _lib
    from hawq_amd.jpeg import front_layout
    lay = front_layout(info, files, out_offsets, out_bytes)
    place, head = ar.put(lay.place.view(np.uint8), "place"), ar.put(lay.head, "head")
    blob = ar.empty(lay.nbytes, torch.uint8, "blob")
    _lib.call("hawq_jpeg_front_fill", s.files.data_ptr(), s.total, s.table_dev.data_ptr(), s.table.ctypes.data, len(s.table), s.info_dev.data_ptr(), info.ctypes.data,
              place.data_ptr(), lay.place.ctypes.data, len(files), blob.data_ptr(), lay.nbytes, torch.cuda.current_stream().cuda_stream)
    blob[:lay.head.size].copy_(head)
    ar.check()
    return lay, blob.cpu().numpy()


def planner_blob(datas, out_offsets=None, out_bytes=None):
    from hawq_amd.jpeg import parse_jpeg, plan_jpeg_batch
    plan = plan_jpeg_batch([parse_jpeg(d) for d in datas], out_offsets, out_bytes)
    return plan, plan.blob[:plan.nbytes]


def test_scan_records_equal_the_host_twins_on_fixtures_refused_files_and_corpus(arena):
    from hawq_amd.jpeg import front_scan_host
    corpus = F.corpus()
    datas = [d for _, d in F.fixture_files()] + corpus[::max(1, len(corpus) // 200)]
    assert len(datas) > 300
    info, _ = run_scan(arena, datas)
    want = front_scan_host(datas)
    wrong = [i for i in range(len(datas)) if info[i].tobytes() != want[i].tobytes()]
    assert not wrong, [(i, info[i], want[i]) for i in wrong[:3]]
    assert (want["defer"] == 0).sum() > 100 and (want["defer"] != 0).sum() > 100


def test_filled_blob_equals_the_planners_byte_for_byte_and_the_checker_passes_it(arena):
    from hawq_amd import _lib
    good, _, _ = jpeg_model.cases()
    datas = [good[n][0] for n in good] + [jpeg_model.sample()]
    info, s = run_scan(arena, datas)
    assert (info["defer"] == 0).all()
    plan, want = planner_blob(datas)
    lay, blob = run_fill(arena, s, info, range(len(datas)), plan.out_offsets, plan.out_bytes)
    assert lay.nbytes == plan.nbytes and np.array_equal(blob, want)   # padding included: zero
    host = np.ascontiguousarray(blob)
    assert _lib.load().hawq_jpeg_batch_ok(host.ctypes.data, lay.nbytes, lay.coef_blocks, lay.plane_bytes, lay.out_bytes), _lib.load().hawq_last_error()


@functools.lru_cache(maxsize=None)
def phase_files():
    """A fixture with 15 restart intervals (RSTn wraps modulo 8) behind a comment segment of every length that moves its markers through
    all phases of the kernel's 16-byte chunk per lane and its 1024-byte stride per pass, and the committed sample (27 KB, many passes)"""
    from hawq_amd.jpeg import parse_jpeg
    good, _, cond = jpeg_model.cases()
    assert cond["max_intervals"] == 15
    data = next(good[n][0] for n in good if len(parse_jpeg(good[n][0]).intervals) == 15)
    return [data[:2] + b"\xff\xfe" + bytes([(k + 2) >> 8, (k + 2) & 255]) + b"c" * k + data[2:] for k in range(1024 + 16)] + [jpeg_model.sample()]


def test_markers_in_every_phase_of_chunk_and_pass_give_the_hosts_records_and_blob(arena):
    from hawq_amd import _lib
    from hawq_amd.jpeg import front_scan_host
    datas = phase_files()
    info, s = run_scan(arena, datas)
    want = front_scan_host(datas)
    assert (want["defer"] == 0).all() and (want["n_intervals"][:-1] == 15).all()
    first = want["scan_first"][:-1]
    assert len(set((first % 1024).tolist())) == 1024   # a marker in every phase of a pass, so one straddles two lanes and one two passes
    assert info.tobytes() == want.tobytes()
    plan, blob_want = planner_blob(datas)
    lay, blob = run_fill(arena, s, info, range(len(datas)), plan.out_offsets, plan.out_bytes)
    assert np.array_equal(blob, blob_want)
    host = np.ascontiguousarray(blob)
    assert _lib.load().hawq_jpeg_batch_ok(host.ctypes.data, lay.nbytes, lay.coef_blocks, lay.plane_bytes, lay.out_bytes), _lib.load().hawq_last_error()


def mixed_sources():
    from tests import jpeg_prog_model
    from tests.test_gpu_jpeg import damaged_files
    good, bad, _ = jpeg_model.cases()
    prog, prog_bad, _ = jpeg_prog_model.cases()
    a, truncated, damaged, b = damaged_files()
    long_header = good["noise_16x16_444"][0][:2] + b"\xff\xfe\x00\x03x" * 70 + good["noise_16x16_444"][0][2:]   # deferred by the kernel, taken by parse_jpeg
    return [good["noise_31x33_420"][0], bad["progressive"][0], a, truncated, bad["png"][0], jpeg_model.sample(), bad["cmyk"][0], damaged, long_header,
            prog["noise_16x16_420"][0], good["noise_40x24_rst2"][0], prog_bad["two_components"][0], b, good["smooth_40x23_gray"][0]]


@pytest.mark.parametrize("more", [{}, {"entropy": "sync", "min_sync_bytes": 64, "sub_bytes": 16}, {"progressive": True}], ids=["serial", "sync", "progressive"])
def test_mixed_batch_gives_the_tensors_and_fallbacks_of_the_host_front_end(more):
    from hawq_amd.jpeg import decode_jpeg_batch
    srcs = mixed_sources()
    want, want_fallbacks = decode_jpeg_batch(srcs, **more)
    got, fallbacks = decode_jpeg_batch(srcs, front_end="device", **more)
    assert fallbacks == want_fallbacks and len(fallbacks) >= 5
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    base = got[0].untyped_storage().data_ptr()
    assert all(im.is_cuda and im.untyped_storage().data_ptr() == base and im.data_ptr() % 16 == 0 for im in got)
    # a second batch reuses the staging buffers
    again, fallbacks = decode_jpeg_batch(srcs[::-1], front_end="device", **more)
    assert all(torch.equal(x, y) for x, y in zip(again, want[::-1])) and [i for i, _ in fallbacks] == sorted(len(srcs) - 1 - i for i, _ in want_fallbacks)


def test_folder_loader_with_the_device_front_end_equals_device_decode_alone(tmp_path):
    from hawq_amd.image import folder_loader
    good, bad, _ = jpeg_model.cases()
    picks = ["noise_1x1_444", "smooth_8x8_gray", "noise_13x17_422", "noise_16x16_420rst", "smooth_31x33_opt95", "noise_40x23_q30", "flat_24x24",
             "checker_32x32_q30", "noise_40x24_q100", "noise_40x24_rst7_gray", "noise_65x9_420"]
    for k, n in enumerate(picks):
        d = tmp_path / ("class%d" % (k % 3))
        d.mkdir(exist_ok=True)
        (d / (n + ".jpg")).write_bytes(good[n][0])
    (tmp_path / "class0" / "sample.jpeg").write_bytes(jpeg_model.sample())
    (tmp_path / "class1" / "progressive.jpg").write_bytes(bad["progressive"][0])
    (tmp_path / "class2" / "picture.png").write_bytes(bad["png"][0])
    ref = list(folder_loader(str(tmp_path), batch_size=5, resize=40, crop=32, device_decode=True))
    got = list(folder_loader(str(tmp_path), batch_size=5, resize=40, crop=32, device_decode=True, front_end="device"))
    assert len(got) == len(ref) == 3
    for (gb, gt), (rb, rt) in zip(got, ref):
        assert gb.is_cuda and gb.dtype == torch.uint8 and torch.equal(gt, rt) and torch.equal(gb, rb)
