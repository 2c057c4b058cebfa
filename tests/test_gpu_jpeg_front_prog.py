"""The device front end for progressive JPEGs on the MI355X (hawq_jpeg_front_scan_prog, hawq_jpeg_front_fill_prog,
``decode_jpeg_batch(front_end="device", progressive="device")``): the scan kernel's records equal its host twin's bit
for bit, the filled blob equals the planner's byte for byte, and the option changes neither an output byte nor the fallback list.  The
C ABI runs with every buffer between poisoned guards (tests/guard.py), with both poisons.  The fixtures and the corpus files have passed
the same walker on the host under the sanitizers (tests/test_jpeg_front_prog_host.py); the other files differ from a fixture by comment
segments or by stream bytes."""
import numpy as np
import pytest
import torch

from tests import guard, jpeg_model, jpeg_prog_model
from tests import jpeg_front_corpus as F
from tests import jpeg_front_prog_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[0xA5, 0x5A], ids=["poisonA5", "poison5A"])
def arena(request):
    ar = guard.GuardArena("cuda", poison=request.param)
    yield ar
    ar.check()


class Staged:
    pass


def run_scan(ar, datas):
    """hawq_jpeg_front_scan_prog on ``datas`` with files, table and records in the arena -> (info, scans, what run_fill needs)"""
    from hawq_amd import _lib
    from hawq_amd.jpeg import _FINFO, _FSCAN, pack_files
    s = Staged()
    s.table, buf, s.total = pack_files(datas)
    buf = buf.copy()
    for off, n in zip(s.table["offset"].tolist(), s.table["length"].tolist()):   # the bytes between two files belong to nobody
        buf[off + n:(off + n + 15) & ~15] = ar.poison
    s.files, s.table_dev = ar.put(buf[:s.total], "files"), ar.put(s.table.view(np.uint8), "table")
    s.info_dev = ar.empty(len(datas) * _FINFO.itemsize, torch.uint8, "info")
    s.scans_dev = ar.empty(len(datas) * 64 * _FSCAN.itemsize, torch.uint8, "scans")
    _lib.call("hawq_jpeg_front_scan_prog", s.files.data_ptr(), s.total, s.table_dev.data_ptr(), s.table.ctypes.data, len(datas), s.info_dev.data_ptr(),
              s.scans_dev.data_ptr(), torch.cuda.current_stream().cuda_stream)
    ar.check()
    return s.info_dev.cpu().numpy().view(_FINFO), s.scans_dev.cpu().numpy().view(_FSCAN).reshape(len(datas), 64), s


def run_fill(ar, s, info, scans, files, out_offsets, out_bytes):
    """hawq_jpeg_front_fill_prog for the accepted progressive ``files`` into a blob in the arena, then the head as the Python path
    uploads it -> (layout, blob)"""
    from hawq_amd import _lib
    from hawq_amd.jpeg import front_prog_layout
    lay = front_prog_layout(info, scans, files, out_offsets, out_bytes)
    place, head = ar.put(lay.place.view(np.uint8), "place"), ar.put(lay.head, "head")
    blob = ar.empty(lay.nbytes, torch.uint8, "blob")
    _lib.call("hawq_jpeg_front_fill_prog", s.files.data_ptr(), s.total, s.table_dev.data_ptr(), s.table.ctypes.data, len(s.table), s.info_dev.data_ptr(),
              info.ctypes.data, s.scans_dev.data_ptr(), scans.ctypes.data, place.data_ptr(), lay.place.ctypes.data, len(lay.place), blob.data_ptr(), lay.nbytes,
              torch.cuda.current_stream().cuda_stream)
    blob[:lay.head.size].copy_(head)
    ar.check()
    return lay, blob.cpu().numpy()


def planner_blob(datas):
    from hawq_amd.jpeg import parse_jpeg, plan_jpeg_prog_batch
    plan = plan_jpeg_prog_batch([parse_jpeg(d, progressive=True) for d in datas])
    return plan, plan.blob[:plan.nbytes]


def checker_passes(lay, blob):
    from hawq_amd import _lib
    host = np.ascontiguousarray(blob)
    return bool(_lib.load().hawq_jpeg_prog_ok(host.ctypes.data, lay.nbytes, lay.coef_blocks, lay.plane_bytes, lay.out_bytes)), _lib.load().hawq_last_error()


def test_scan_records_equal_the_host_twins_on_fixtures_refused_files_and_corpus(arena):
    from hawq_amd.jpeg import front_scan_prog_host
    corpus = F.corpus()
    datas = [d for _, d in F.fixture_files()] + corpus[::max(1, len(corpus) // 200)]
    assert len(datas) > 300
    info, scans, _ = run_scan(arena, datas)
    want, want_scans = front_scan_prog_host(datas)
    wrong = [i for i in range(len(datas)) if info[i].tobytes() != want[i].tobytes() or scans[i].tobytes() != want_scans[i].tobytes()]
    assert not wrong, [(i, info[i], want[i]) for i in wrong[:3]]
    accepted = want["defer"] == 0
    assert (accepted & (want["reserved"][:, 0] == 0)).sum() > 100 and (accepted & (want["reserved"][:, 0] == 1)).sum() > 50 and (~accepted).sum() > 50


def test_filled_blob_equals_the_planners_byte_for_byte_and_the_checker_passes_it(arena):
    _, datas = M.prog_fixtures()
    info, scans, s = run_scan(arena, datas)
    assert (info["defer"] == 0).all() and (info["reserved"][:, 0] == 1).all()
    plan, want = planner_blob(datas)
    lay, blob = run_fill(arena, s, info, scans, range(len(datas)), plan.out_offsets, plan.out_bytes)
    assert lay.nbytes == plan.nbytes and np.array_equal(blob, want)   # padding included: zero
    assert checker_passes(lay, blob)[0], checker_passes(lay, blob)[1]


def test_markers_in_every_phase_of_chunk_and_pass_give_the_hosts_records_and_blob(arena):
    """Every comment length 0..1039 in front of the frame header and between the second and third scan of a progressive file with
    restart markers: every scan's markers pass through every phase of the 16-byte lane and the 1 KiB pass"""
    from hawq_amd.jpeg import front_scan_prog_host
    datas = M.phase_files()
    assert len(datas) == 2080
    info, scans, s = run_scan(arena, datas)
    want, want_scans = front_scan_prog_host(datas)
    n_scans = int(want["reserved"][0, 1])
    assert (want["defer"] == 0).all() and (want["reserved"][:, 0] == 1).all() and (want["reserved"][:, 1] == n_scans).all()
    assert (want_scans["n_intervals"][:, :n_scans] > 1).all()
    for k in range(n_scans):   # a marker of every scan in every phase of a pass, so one straddles two lanes and one two passes
        assert len(set((want_scans["scan_first"][:1040, k] % 1024).tolist())) == 1024
    assert len(set((want_scans["scan_first"][1040:, 2] % 1024).tolist())) == 1024 and len(set(want_scans["scan_first"][1040:, 1].tolist())) == 1
    assert info.tobytes() == want.tobytes() and scans.tobytes() == want_scans.tobytes()
    plan, blob_want = planner_blob(datas)
    lay, blob = run_fill(arena, s, info, scans, range(len(datas)), plan.out_offsets, plan.out_bytes)
    assert np.array_equal(blob, blob_want)
    assert checker_passes(lay, blob)[0], checker_passes(lay, blob)[1]


def mixed_sources(k):
    """Batches of baseline and progressive files, refused and damaged ones, files the walker defers by design, and the 27 KB sample"""
    from tests.test_gpu_jpeg import damaged_files
    good, bad, _ = jpeg_model.cases()
    prog, prog_bad, _ = jpeg_prog_model.cases()
    a, truncated, damaged, b = damaged_files()
    comments = b"\xff\xfe\x00\x03x" * 70
    long_header = good["noise_16x16_444"][0][:2] + comments + good["noise_16x16_444"][0][2:]        # deferred by the kernel, taken by parse_jpeg
    long_prog = prog["noise_7x9_gray"][0][:2] + comments + prog["noise_7x9_gray"][0][2:]            # the same of a progressive file
    cut = prog["noise_40x24_420_rst"][0]
    damaged_prog = cut[:len(cut) - 40] + bytes(20) + cut[len(cut) - 20:]                            # stream bytes of the last scan zeroed
    if k == 0:
        return [good["noise_31x33_420"][0], bad["progressive"][0], a, truncated, bad["png"][0], jpeg_model.sample(), bad["cmyk"][0], damaged, long_header,
                prog["noise_16x16_420"][0], good["noise_40x24_rst2"][0], prog_bad["two_components"][0], b, good["smooth_40x23_gray"][0], long_prog,
                prog["tables_13x17_422"][0], damaged_prog, prog["deep_33x31_420"][0]]
    if k == 1:   # progressive files alone: no baseline launch makes the synchronisation
        return [prog[n][0] for n in list(prog)[::3]] + [long_prog]
    return [jpeg_model.sample(), good["noise_13x17_422"][0], prog["noise_40x24_gray_rst"][0]] + [prog[n][0] for n in list(prog)[1::4]]   # a quarter progressive and more


@pytest.mark.parametrize("more", [{}, {"entropy": "sync", "min_sync_bytes": 64, "sub_bytes": 16}, {"draft": (8, 8)}], ids=["serial", "sync", "draft"])
@pytest.mark.parametrize("batch", [0, 1, 2])
def test_mixed_batch_gives_the_tensors_and_fallbacks_of_the_host_front_end(batch, more):
    from hawq_amd.jpeg import decode_jpeg_batch
    srcs = mixed_sources(batch)
    want, want_fallbacks = decode_jpeg_batch(srcs, progressive=True, **more)
    got, fallbacks = decode_jpeg_batch(srcs, front_end="device", progressive="device", **more)
    assert fallbacks == want_fallbacks and (batch != 0 or len(fallbacks) >= 5)
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    base = got[0].untyped_storage().data_ptr()
    assert all(im.is_cuda and im.untyped_storage().data_ptr() == base and im.data_ptr() % 16 == 0 for im in got)
    # a second batch reuses the staging buffers
    again, fallbacks = decode_jpeg_batch(srcs[::-1], front_end="device", progressive="device", **more)
    assert all(torch.equal(x, y) for x, y in zip(again, want[::-1])) and [i for i, _ in fallbacks] == sorted(len(srcs) - 1 - i for i, _ in want_fallbacks)


def test_every_progressive_fixture_decodes_to_pillows_bytes_on_the_new_route():
    from hawq_amd.image import decode_image
    from hawq_amd.jpeg import decode_jpeg_batch
    _, datas = M.prog_fixtures()
    got, fallbacks = decode_jpeg_batch(datas, front_end="device", progressive="device")
    assert fallbacks == []
    assert all(torch.equal(x.cpu(), decode_image(d)) for x, d in zip(got, datas))


def test_folder_loader_with_the_option_equals_device_decode_with_progressive(tmp_path):
    from hawq_amd.image import folder_loader
    good, bad, _ = jpeg_model.cases()
    prog, _, _ = jpeg_prog_model.cases()
    picks = [("noise_1x1_444", good), ("noise_16x16_420", prog), ("noise_13x17_422", good), ("tables_13x17_422", prog), ("smooth_31x33_opt95", good),
             ("deep_33x31_420", prog), ("noise_40x24_gray_rst", prog), ("noise_40x24_rst7_gray", good), ("noise_65x9_420", good)]
    for k, (n, cases) in enumerate(picks):
        d = tmp_path / ("class%d" % (k % 3))
        d.mkdir(exist_ok=True)
        (d / ("%s_%d.jpg" % (n, k))).write_bytes(cases[n][0])
    (tmp_path / "class0" / "sample.jpeg").write_bytes(jpeg_model.sample())
    (tmp_path / "class1" / "progressive.jpg").write_bytes(bad["progressive"][0])
    (tmp_path / "class2" / "picture.png").write_bytes(bad["png"][0])
    ref = list(folder_loader(str(tmp_path), batch_size=5, resize=40, crop=32, device_decode=True, progressive=True))
    got = list(folder_loader(str(tmp_path), batch_size=5, resize=40, crop=32, device_decode=True, front_end="device", progressive="device"))
    assert len(got) == len(ref) == 3
    for (gb, gt), (rb, rt) in zip(got, ref):
        assert gb.is_cuda and gb.dtype == torch.uint8 and torch.equal(gt, rt) and torch.equal(gb, rb)
