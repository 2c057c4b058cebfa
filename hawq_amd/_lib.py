"""ctypes binding of libhawq_mi355.so (C ABI: include/hawq_mi355.h).

There is NO fallback: if the shared library is missing or an entry point is absent, importing
the product path raises.  Build it with ``python -c "import __graft_entry__ as g; g.build()"``
or ``make -C hawq_amd/csrc``.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# HAWQ_LIB: another build of the same ABI (A/B measurements of kernel variants); default = the in-tree build
LIB_PATH = os.environ.get("HAWQ_LIB") or os.path.join(_HERE, "lib", "libhawq_mi355.so")

EPI_RAW, EPI_REQUANT, EPI_RESIDUAL, EPI_DEQUANT = 0, 1, 2, 3

i32, i64, f32, vp = C.c_int32, C.c_int64, C.c_float, C.c_void_p


class ConvArgs(C.Structure):
    """struct hawq_conv_args (include/hawq_mi355.h)."""
    _fields_ = [
        ("in_", vp), ("wgt", vp), ("bias", vp),
        ("N", i32), ("H", i32), ("W", i32), ("Cin", i32), ("Cout", i32), ("KH", i32), ("KW", i32),
        ("stride", i32), ("pad", i32), ("in_bits", i32), ("w_bits", i32),
        ("in2", vp), ("wgt2", vp), ("bias2", vp),
        ("H2", i32), ("W2", i32), ("Cin2", i32), ("stride2", i32), ("in2_bits", i32), ("w2_bits", i32),
        ("epilogue", i32), ("relu", i32),
        ("m", vp), ("e", vp), ("m_id", vp), ("e_id", vp),
        ("m_id_scalar", i32), ("e_id_scalar", i32),
        ("res_in", vp), ("res_in_bits", i32),
        ("res_out", vp), ("res_out_bits", i32),
        ("out_q", vp), ("out_bits", i32), ("q_lo", i32), ("q_hi", i32), ("mq", i32), ("eq", i32),
        ("out_acc", vp), ("out_f32", vp), ("fscale", vp), ("ldo", i32), ("n_valid", i32),
        ("flags", vp), ("tile", i32), ("ctab", vp), ("ctab_id", vp), ("fast_tables", i32),
        ("in_planar", i32), ("out_planar", i32),
        ("res_no_relu", i32), ("res_clamp16", i32),
        ("in_pitch", i32), ("out_pitch", i32),
        ("wgt_band", vp), ("wgt_k128", vp), ("wgt2_k128", vp),
        ("out_sub", i32),
    ]


def res_sub(a) -> int:
    """"res_sub" of a ConvArgs block (hawq_res_sub in csrc/common.h): s >= 2 when a single-branch RESIDUAL launch reads its stored residual
    on the larger H2 x W2 map at stride2 = s, else 0."""
    return int(a.stride2) if (a.epilogue == EPI_RESIDUAL and not a.in2 and a.res_in and a.stride2 >= 2) else 0


class ConvChoice(C.Structure):
    """struct hawq_conv_choice (include/hawq_mi355.h): what hawq_conv2d would launch, from the host-only hawq_conv2d_choice."""
    _fields_ = [("family", i32), ("tile", i32), ("index", i32), ("fn_table", i32), ("fn", i32 * 3),
                ("grid", i32), ("block", i32), ("lds_bytes", i32)] + [(n, i32) for n in (
        "stride", "res_sub", "Ho", "Wo", "M", "q_lo", "mq", "eq", "m_id_s", "e_id_s", "k0", "ck0", "gfast",
        "in_pitch", "out_pitch", "ring_bytes")]


class ExpandReduceArgs(C.Structure):
    """struct hawq_expand_reduce_args (include/hawq_mi355.h)."""
    _fields_ = [("expand", ConvArgs), ("reduce", ConvArgs), ("tile", i32)]


class BottleneckArgs(C.Structure):
    """struct hawq_bottleneck_args (include/hawq_mi355.h): one launch per MobileNetV2 linear-bottleneck unit."""
    _fields_ = [("expand", ConvArgs), ("project", ConvArgs), ("dw_wgt9c", vp), ("dw_ctab", vp),
                ("dw_stride", i32), ("dw_q_lo", i32), ("dw_q_hi", i32), ("dw_fast_tables", i32), ("c_mid", i32), ("tile", i32)]


class IncepConvArgs(C.Structure):
    """struct hawq_incep_conv_args (include/hawq_mi355.h): the InceptionV3 rectangular conv."""
    _fields_ = [
        ("in_", vp), ("wgt", vp), ("bias", vp),
        ("N", i32), ("H", i32), ("W", i32), ("Cin", i32), ("Cout", i32), ("KH", i32), ("KW", i32),
        ("stride", i32), ("pad_h", i32), ("pad_w", i32),
        ("epilogue", i32), ("relu", i32),
        ("m", vp), ("ek", vp),
        ("q_lo", i32), ("q_hi", i32), ("m2", i32), ("ek2", i32), ("q2_lo", i32), ("q2_hi", i32),
        ("out", vp),
        ("out_bits", i32), ("ldo", i32), ("c_off", i32), ("reserved", i32),
    ]


INCEP_RAW, INCEP_REQUANT, INCEP_REQUANT2 = 0, 1, 2
INCEP_GROUP_MAX = 8


class IncepGroupArgs(C.Structure):
    """struct hawq_incep_group_args (include/hawq_mi355.h): the members of one grouped conv launch."""
    _fields_ = [("n", i32), ("reserved", i32), ("conv", IncepConvArgs * INCEP_GROUP_MAX)]


INCEP_FAN_MAX = 4


class IncepFanOut(C.Structure):
    """struct hawq_incep_fan_out (include/hawq_mi355.h): one int8 copy of a member's output at a consumer's scale."""
    _fields_ = [("out", vp)] + [(n, i32) for n in ("m", "ek", "lo", "hi", "ldo", "c_off")]


class IncepFan(C.Structure):
    """struct hawq_incep_fan (include/hawq_mi355.h): the fan outputs of one member of hawq_incep_conv_group_fan."""
    _fields_ = [("n", i32), ("reserved", i32), ("to", IncepFanOut * INCEP_FAN_MAX)]


# op ids of hawq_incep_pool_v, by the entry point each one stands for
INCEP_POOL_OPS = {"hawq_incep_requant": 0, "hawq_incep_maxpool3s2": 1, "hawq_incep_avgpool_branch": 2, "hawq_incep_global_avgpool": 3}


class IncepPoolArgs(C.Structure):
    """struct hawq_incep_pool_args (include/hawq_mi355.h): the InceptionV3 plan's pool / requant launches."""
    _fields_ = [("in_", vp), ("out", vp)] + [(n, i32) for n in (
        "N", "H", "W", "C", "in_bits", "in_pitch", "in_off", "out_bits", "ldo", "c_off",
        "pre", "m1", "ek1", "lo1", "hi1", "post", "m2", "ek2", "lo2", "hi2")]


class ImageDesc(C.Structure):
    """struct hawq_image_desc (include/hawq_mi355.h): one image of a hawq_image_batch launch."""
    _fields_ = [("base", C.c_uint64)] + [(n, i32) for n in (
        "h", "w", "oh", "ow", "top", "left", "skip_h", "skip_v", "hb_off", "hc_off", "vb_off", "vc_off", "kh", "kv")]


class ImageTile(C.Structure):
    """struct hawq_image_tile (include/hawq_mi355.h): the crop rows one workgroup of hawq_image_batch computes."""
    _fields_ = [("image", i32), ("row0", i32), ("rows", i32)]


class JpegBatchHdr(C.Structure):
    """struct hawq_jpeg_batch_hdr (include/hawq_mi355.h): offset 0 of the blob of a hawq_jpeg_decode_batch call."""
    _fields_ = [(n, i32) for n in ("n_images", "n_waves", "desc_off", "wave_off")]


class JpegHuff(C.Structure):
    """struct hawq_jpeg_huff (include/hawq_mi355.h): one canonical Huffman table."""
    _fields_ = [("mincode", i32 * 17), ("maxcode", i32 * 17), ("valptr", i32 * 17), ("huffval", C.c_uint8 * 256), ("reserved", i32)]


class JpegSyncJob(C.Structure):
    """struct hawq_jpeg_sync_job (include/hawq_mi355.h): one long interval of a hawq_jpeg_decode_batch_sync call."""
    _fields_ = [("wave", i32), ("n_sub", i32), ("scratch_off", i64)]


class JpegSyncSub(C.Structure):
    """struct hawq_jpeg_sync_sub (include/hawq_mi355.h): the scratch record of one sub-sequence."""
    _fields_ = [(n, i32) for n in ("start_pos", "start_uk", "end_pos", "end_uk", "blocks")] + [("dc", i32 * 3)]


class JpegDesc(C.Structure):
    """struct hawq_jpeg_desc (include/hawq_mi355.h): one image of a hawq_jpeg_decode_batch call."""
    _fields_ = ([(n, i32) for n in ("width", "height", "ncomp", "hs", "vs", "mcus_x", "mcus_y", "restart", "n_intervals")]
                + [(n, i32 * 3) for n in ("qt_off", "dc_off", "ac_off")]
                + [(n, i32) for n in ("stream_off", "stream_len", "interval_off", "scale")]
                + [(n, i64) for n in ("coef_block0", "plane_off", "out_off")])


class JpegProgHdr(C.Structure):
    """struct hawq_jpeg_prog_hdr (include/hawq_mi355.h): byte 16 of the blob of a hawq_jpeg_decode_batch_prog call."""
    _fields_ = [(n, i32) for n in ("n_scans", "n_levels", "scan_off", "level_off")]


class JpegScan(C.Structure):
    """struct hawq_jpeg_scan (include/hawq_mi355.h): one scan of one progressive image."""
    _fields_ = ([(n, i32) for n in ("image", "ncomp", "comp0", "ss", "se", "ah", "al", "level")] + [("dc_off", i32 * 3)]
                + [(n, i32) for n in ("ac_off", "restart", "n_intervals", "interval_off", "stream_off", "stream_len")] + [("reserved", i32 * 3)])


class JpegResumeSeg(C.Structure):
    """struct hawq_jpeg_resume_seg (include/hawq_mi355.h): one segment of a restart interval of a resume call."""
    _fields_ = [(n, i32) for n in ("wave", "unit0", "n_units", "byte", "bit", "eobrun")] + [("pred", i32 * 3), ("reserved", i32)]


class JpegFrontFile(C.Structure):
    """struct hawq_jpeg_front_file (include/hawq_mi355.h): where one raw file lies in the files buffer of hawq_jpeg_front_scan."""
    _fields_ = [("offset", i64), ("length", i64)]


class JpegFrontInfo(C.Structure):
    """struct hawq_jpeg_front_info (include/hawq_mi355.h): what hawq_jpeg_front_scan found in one file."""
    _fields_ = ([(n, i32) for n in ("defer", "width", "height", "ncomp", "hs", "vs", "restart", "n_intervals")] + [(n, i32 * 3) for n in ("tq", "td", "ta")]
                + [("qt_at", i32 * 4), ("huff_at", i32 * 4), ("scan_first", i32), ("scan_end", i32), ("reserved", i32 * 5)])


class JpegFrontPlace(C.Structure):
    """struct hawq_jpeg_front_place (include/hawq_mi355.h): where hawq_jpeg_front_fill writes one file's share of the blob."""
    _fields_ = [("file", i32)] + [(n, i32 * 3) for n in ("qt_off", "dc_off", "ac_off")] + [("interval_off", i32), ("stream_off", i32), ("reserved", i32 * 4)]


class JpegFrontScanRec(C.Structure):
    """struct hawq_jpeg_front_scan_rec (include/hawq_mi355.h): what hawq_jpeg_front_scan_prog found in one scan of a progressive file."""
    _fields_ = ([(n, i32) for n in ("ncomp", "comp0", "ss", "se", "ah", "al", "level")] + [("dc_at", i32 * 3)]
                + [(n, i32) for n in ("ac_at", "restart", "n_intervals", "scan_first", "scan_end", "reserved")])


class JpegFrontScanPlace(C.Structure):
    """struct hawq_jpeg_front_scan_place (include/hawq_mi355.h): where hawq_jpeg_front_fill_prog writes one scan's share of the blob."""
    _fields_ = ([("file", i32), ("scan", i32), ("qt_off", i32 * 3), ("dc_off", i32 * 3)]
                + [(n, i32) for n in ("ac_off", "interval_off", "stream_off")] + [("reserved", i32 * 5)])


# name -> (argtypes); every function returns int except hawq_last_error
SIGNATURES = {
    "hawq_abi_version": [],
    "hawq_device_ok": [],
    "hawq_conv2d": [C.POINTER(ConvArgs), vp],
    "hawq_conv2d_choice": [C.POINTER(ConvArgs), C.POINTER(ConvChoice)],
    "hawq_conv2d_num_tiles": [],
    "hawq_conv2d_num_band_tiles": [],
    "hawq_conv2d_band_tile": [C.POINTER(ConvArgs)],
    "hawq_conv2d_num_band2_tiles": [],
    "hawq_conv2d_band2_tile": [C.POINTER(ConvArgs)],
    "hawq_conv2d_band2_sub_extent": [C.POINTER(ConvArgs), i32, i32, C.POINTER(i32)],
    "hawq_pack_w3x3_band": [vp, vp, i32, i32],
    "hawq_conv2d_num_gemm2_tiles": [],
    "hawq_conv2d_gemm2_first": [],
    "hawq_pack_w1x1_k128": [vp, vp, i32, i32],
    "hawq_conv2d_splitk_ok": [C.POINTER(ConvArgs), i32],
    "hawq_conv2d_splitk_workspace": [C.POINTER(ConvArgs), i32, C.POINTER(i64), C.POINTER(i64)],
    "hawq_conv2d_splitk": [C.POINTER(ConvArgs), i32, vp, vp, vp],
    "hawq_fc_dequant_ok": [i32, i32, i32],
    "hawq_fc_dequant": [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp],
    "hawq_conv_expand_reduce": [C.POINTER(ExpandReduceArgs), vp],
    "hawq_conv_expand_reduce_variants": [C.POINTER(ExpandReduceArgs)],
    "hawq_conv_expand_reduce_variant_shape": [C.POINTER(ExpandReduceArgs), i32, C.POINTER(i32), C.POINTER(i32)],
    "hawq_linear_bottleneck": [C.POINTER(BottleneckArgs), vp],
    "hawq_linear_bottleneck_ok": [C.POINTER(BottleneckArgs)],
    "hawq_stem3x3s2": [vp, vp, vp, i32, i32, f32, i32, i32, C.POINTER(ConvArgs), vp],
    "hawq_stem3x3s2_ok": [vp, vp, vp, i32, i32, C.POINTER(ConvArgs)],
    "hawq_quantize_input": [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, f32, i32, i32, vp],
    "hawq_stem_conv7": [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp],
    "hawq_stem_fused": [vp, i32, i32, i32, i32, f32, i32, i32, vp, vp, vp, vp, i32, i32, vp, vp, i32, i32, i32, i32, i32,
                        i32, vp],
    "hawq_stem_fused_u8": [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, i32, i32, vp, vp, i32, i32, i32, i32, i32, i32, vp],
    "hawq_maxpool3s2_requant": [vp, i32, i32, i32, i32, vp, vp, i32, i32, i32, i32, i32, vp],
    "hawq_requant_residual": [vp, i32, i64, vp, i32, i32, i32, i32, i32, vp],
    "hawq_avgpool_requant": [vp, i32, i32, i32, i32, vp, vp, i32, i32, i32, i32, vp],
    "hawq_f32_nchw_to_q_nhwc": [vp, vp, i32, i32, i32, i32, i32, i32, f32, vp],
    "hawq_acc_nhwc_to_f32_nchw": [vp, vp, i32, i32, i32, i32, i32, vp, vp],
    "hawq_fixedpoint_f32": [vp, vp, i32, i32, i32, f32, vp, vp, vp, i32, vp, f32, vp, vp, vp, i32, f32, i32, i32,
                            i32, vp],
    "hawq_fakequant_f32": [vp, vp, i64, f32, f32, i32, i32, vp],
    "hawq_avgpool_f32": [vp, vp, i32, i32, f32, vp],
    "hawq_conv2d_grouped": [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp],
    "hawq_depthwise3x3": [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp],
    "hawq_depthwise3x3_requant": [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp],
    "hawq_depthwise3x3_requant_fast": [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp],
    "hawq_quantize_im2col3x3s2": [vp, vp, i32, i32, i32, i32, f32, i32, i32, vp],
    "hawq_quantize_im2col3x3s2_u8": [vp, vp, vp, i32, i32, i32, i32, vp],
    "hawq_resample_u8": [vp, i32, i32, vp, vp, i32, i32, i32, i32, i32, vp, vp],
    "hawq_image_batch": [vp, i32, vp, i32, vp, vp, i32, i32, vp],
    "hawq_image_batch_ok": [vp, i32, vp, i32, vp, i64, i32, i32],
    "hawq_image_batch_lds_budget": [],
    "hawq_jpeg_batch_ok": [vp, i64, i64, i64, i64],
    "hawq_jpeg_decode_batch": [vp, vp, i64, vp, i64, vp, i64, vp, i64, vp, vp, vp],
    "hawq_jpeg_sync_ok": [vp, i64, i32, i32, i64, i32, i64],
    "hawq_jpeg_decode_batch_sync": [vp, vp, i64, vp, i64, vp, i64, vp, i64, vp, i32, i32, i64, i32, vp, i64, vp, vp],
    "hawq_jpeg_prog_ok": [vp, i64, i64, i64, i64],
    "hawq_jpeg_decode_batch_prog": [vp, vp, i64, vp, i64, vp, i64, vp, i64, vp, vp, vp],
    "hawq_jpeg_resume_record": [vp, i64, i32, i32, vp, i64, C.POINTER(i64)],
    "hawq_jpeg_resume_ok": [vp, i64, i32, i64, i64],
    "hawq_jpeg_decode_batch_resume": [vp, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, i64, vp, vp],
    "hawq_jpeg_decode_batch_prog_resume": [vp, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, i64, vp, vp],
    "hawq_jpeg_front_scan": [vp, i64, vp, vp, i32, vp, vp],
    "hawq_jpeg_front_scan_host": [vp, i64, vp, i32, vp],
    "hawq_jpeg_front_fill_ok": [vp, vp, i32, vp, i32, i64, i64],
    "hawq_jpeg_front_fill": [vp, i64, vp, vp, i32, vp, vp, vp, vp, i32, vp, i64, vp],
    "hawq_jpeg_front_scan_prog": [vp, i64, vp, vp, i32, vp, vp, vp],
    "hawq_jpeg_front_scan_prog_host": [vp, i64, vp, i32, vp, vp],
    "hawq_jpeg_front_fill_prog_ok": [vp, vp, vp, i32, vp, i32, i64, i64],
    "hawq_jpeg_front_fill_prog": [vp, i64, vp, vp, i32, vp, vp, vp, vp, vp, vp, i32, vp, i64, vp],
    "hawq_minmax_f32": [vp, i64, vp, vp, vp],
    "hawq_kthvalue_f32": [vp, i64, i64, i32, vp, vp, vp],
    "hawq_incep_conv": [C.POINTER(IncepConvArgs), vp],
    "hawq_incep_conv_num_tiles": [],
    "hawq_incep_conv_tile_ok": [C.POINTER(IncepConvArgs), i32],
    "hawq_incep_conv_tiled": [C.POINTER(IncepConvArgs), i32, vp],
    "hawq_incep_conv_group_ok": [C.POINTER(IncepGroupArgs), i32],
    "hawq_incep_conv_group": [C.POINTER(IncepGroupArgs), i32, vp],
    "hawq_incep_conv_group_fan_ok": [C.POINTER(IncepGroupArgs), C.POINTER(IncepFan), i32],
    "hawq_incep_conv_group_fan": [C.POINTER(IncepGroupArgs), C.POINTER(IncepFan), i32, vp],
    "hawq_incep_stem_u8": [vp, vp, C.POINTER(IncepConvArgs), vp],
    "hawq_incep_stem_u8_ok": [vp, vp, C.POINTER(IncepConvArgs)],
    "hawq_incep_stem_f32": [vp, f32, i32, i32, C.POINTER(IncepConvArgs), vp],
    "hawq_incep_stem_f32_ok": [vp, f32, i32, i32, C.POINTER(IncepConvArgs)],
    "hawq_avgpool3x3_f32": [vp, vp, i32, i32, i32, f32, vp],
    "hawq_incep_requant": [C.POINTER(IncepPoolArgs), vp],
    "hawq_incep_maxpool3s2": [C.POINTER(IncepPoolArgs), vp],
    "hawq_incep_avgpool_branch": [C.POINTER(IncepPoolArgs), vp],
    "hawq_incep_global_avgpool": [C.POINTER(IncepPoolArgs), vp],
    "hawq_incep_pool_v_ok": [C.POINTER(IncepPoolArgs), i32],
    "hawq_incep_pool_v": [C.POINTER(IncepPoolArgs), i32, vp],
    "hawq_incep_pool_v_avg3_tile": [C.POINTER(IncepPoolArgs), C.POINTER(i32), C.POINTER(i32)],
    "hawq_graph_begin": [vp],
    "hawq_graph_end": [vp, C.POINTER(vp)],
    "hawq_graph_launch": [vp, vp],
    "hawq_graph_destroy": [vp],
    "hawq_event_create": [C.POINTER(vp)],
    "hawq_event_record": [vp, vp],
    "hawq_event_elapsed_ms": [vp, vp, C.POINTER(f32)],
    "hawq_event_destroy": [vp],
}

_lib = None


class HawqLibraryError(RuntimeError):
    pass


def library_path() -> str:
    """Path of the shared library this process loads (the in-tree build unless HAWQ_LIB names another one)."""
    return LIB_PATH


def load():
    """Load the HIP library or raise - never degrade to a CPU path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise HawqLibraryError(
            f"{LIB_PATH} not found: hawq_amd has no CPU fallback. Build the gfx950 library first "
            "(`python -c 'import __graft_entry__ as g; g.build()'` or `make -C hawq_amd/csrc`).")
    lib = C.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as exc:
            raise HawqLibraryError(f"{LIB_PATH} does not export {name}") from exc
        fn.argtypes = argtypes
        fn.restype = C.c_int
    lib.hawq_last_error.restype = C.c_char_p
    lib.hawq_last_error.argtypes = []
    if lib.hawq_abi_version() != 5:
        raise HawqLibraryError("libhawq_mi355.so ABI version mismatch")
    _lib = lib
    return lib


def check(rc: int):
    if rc != 0:
        raise RuntimeError("libhawq_mi355: " + load().hawq_last_error().decode())


def call(name: str, *args):
    check(getattr(load(), name)(*args))
