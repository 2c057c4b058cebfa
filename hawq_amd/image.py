"""Image pipeline in front of the uint8 input path (quant_train.py:427-440): ``transforms.Resize(resize)`` and
``transforms.CenterCrop(crop)`` on the decoded image, on the MI355X, with (resize, crop) = ``eval_geometry(arch)``: (342, 299) for
InceptionV3, (256, 224) for every other network; ``ToTensor`` + ``Normalize`` + the input QuantAct are the look-up table of
``forward_uint8`` (``IntegerEngine`` and ``InceptionEngine``).

torchvision's Resize on a PIL image is ``Image.resize(..., BILINEAR)``: Pillow's antialiased separable resampling
(libImaging/Resample.c).  The coefficient construction below restates its ``precompute_coeffs`` (binary64, support scaled by
the down-sampling factor, taps normalised to sum 1) and ``normalize_coeffs_8bpc`` (22 fractional bits, round half away);
the two passes run in ``hawq_resample_u8``.  Pinned to REAL Pillow output: ``tests/golden/pillow_resize.npz``
(``make_pillow.py``, Pillow 12.2) holds what ``Image.resize(..., BILINEAR)`` + the crop produce for nine geometries and a JPEG;
``oracle/pil_resample.py`` and this device stage both reproduce it bit for bit.

``resize_center_crop`` / ``preprocess_batch`` work image by image; ``preprocess_batch_fused`` does a whole ragged batch with one
``hawq_image_batch`` launch from the tables of ``plan_batch``: same coefficients, same bytes.

JPEG decoding is on the host by default, as in the reference (``datasets.ImageFolder``'s ``pil_loader`` inside DataLoader workers,
quant_train.py:428-445): ``decode_image`` / ``folder_loader`` below use Pillow when it is installed and say so when it is not;
everything after the decoded uint8 HWC pixels runs on the MI355X.  ``folder_loader(device_decode=True)`` decodes baseline JPEGs on the
MI355X as well (``hawq_amd/jpeg.py``, DESIGN.md 12: the same bytes; other files still go through ``decode_image``).
"""
from __future__ import annotations

import ctypes as C
import functools
import math

import numpy as np
import torch

from . import _lib

PRECISION_BITS = 32 - 8 - 2


def bilinear_coeffs(in_size: int, out_size: int):
    """Resample.c: precompute_coeffs (bilinear filter, support 1.0) + normalize_coeffs_8bpc.
    Returns (bounds int32 [out, 2] = (first input index, taps), coef int32 [out, ksize], ksize)."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.float64)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        x = np.arange(xmax, dtype=np.float64)
        w = np.abs((x + xmin - center + 0.5) * ss)
        w = np.where(w < 1.0, 1.0 - w, 0.0)
        ww = w.sum()
        if ww != 0.0:
            w = w / ww
        kk[xx, :xmax] = w
        bounds[xx] = (xmin, xmax)
    coef = np.where(kk < 0, (-0.5 + kk * (1 << PRECISION_BITS)).astype(np.int64), (0.5 + kk * (1 << PRECISION_BITS)).astype(np.int64))
    return bounds, coef.astype(np.int32), ksize


def eval_geometry(arch: str):
    """(resize, crop) of the reference's validation pipeline for `arch` (quant_train.py:427-429, ``test_resolution``):
    Resize(342) + CenterCrop(299) for InceptionV3, Resize(256) + CenterCrop(224) otherwise."""
    return (342, 299) if arch == "inceptionv3" else (256, 224)


def resize_crop_geometry(h: int, w: int, resize: int = 256, crop: int = 224):
    """torchvision Resize(int) (smaller edge -> resize, other edge int(resize * long / short)) + CenterCrop(crop):
    (resized h, resized w, crop top, crop left)."""
    if w <= h:
        ow, oh = resize, int(resize * h / w)
    else:
        oh, ow = resize, int(resize * w / h)
    return oh, ow, int(round((oh - crop) / 2.0)), int(round((ow - crop) / 2.0))


@functools.lru_cache(maxsize=256)   # ImageNet validation has thousands of distinct (h, w): bound the device allocations
def _coeffs_dev(in_size, out_size, lo, n, dev):
    """(bounds relative to the first input index read, coefficients, taps, first input index, one past the last) of output
    indices lo .. lo+n-1, on `dev`"""
    b, c, k = bilinear_coeffs(in_size, out_size)
    b = np.ascontiguousarray(b[lo:lo + n]).copy()
    first, last = int(b[:, 0].min()), int((b[:, 0] + b[:, 1]).max())
    b[:, 0] -= first
    return (torch.from_numpy(b).to(dev), torch.from_numpy(np.ascontiguousarray(c[lo:lo + n])).to(dev), k, first, last)


def resize_center_crop(img: torch.Tensor, resize: int = 256, crop: int = 224) -> torch.Tensor:
    """uint8 HWC image on the MI355X -> uint8 [crop, crop, C], equal to CenterCrop(crop)(Resize(resize)(PIL image)) as
    restated above.  Only the crop window is computed (same values: the passes are separable and local)."""
    if not img.is_cuda or img.dtype != torch.uint8 or img.dim() != 3:
        raise ValueError("expected a uint8 HWC tensor on the MI355X")
    h, w, ch = img.shape
    oh, ow, top, left = resize_crop_geometry(h, w, resize, crop)
    if oh < crop or ow < crop:
        raise ValueError("image too small for the crop (torchvision pads here; ImageNet validation images never need it)")
    img = img.contiguous()
    dev, sp = img.device, torch.cuda.current_stream(img.device).cuda_stream
    bv, cv, kv, y0, y1 = _coeffs_dev(h, oh, top, crop, str(dev))       # vertical taps of the crop rows: input rows y0 .. y1
    bh, chh, kh, x0, _ = _coeffs_dev(w, ow, left, crop, str(dev))       # horizontal taps: bounds relative to input column x0
    # Pillow runs the horizontal pass first, on the input rows the vertical pass will read
    tmp = torch.empty(y1 - y0, crop, ch, dtype=torch.uint8, device=dev)
    if ow != w:
        _lib.call("hawq_resample_u8", img.data_ptr() + x0 * ch, w, ch, bh.data_ptr(), chh.data_ptr(), kh, crop, 1, y1 - y0, y0, tmp.data_ptr(), sp)
    else:
        tmp.copy_(img[y0:y1, left:left + crop])
    if oh == h:
        return tmp[top - y0:top - y0 + crop].clone()
    out = torch.empty(crop, crop, ch, dtype=torch.uint8, device=dev)
    _lib.call("hawq_resample_u8", tmp.data_ptr(), crop, ch, bv.data_ptr(), cv.data_ptr(), kv, crop, 0, crop, 0, out.data_ptr(), sp)   # tmp starts at input row y0
    return out


def preprocess_batch(images, resize: int = 256, crop: int = 224, fused: bool = False) -> torch.Tensor:
    """List of decoded uint8 HWC images (any sizes, host or device) -> uint8 [N, crop, crop, C] for ``forward_uint8``.
    (resize, crop) per network: ``eval_geometry(arch)``.  ``fused``: the one-launch path, ``preprocess_batch_fused`` (same bytes)."""
    if fused:
        return preprocess_batch_fused(images, resize, crop)
    return torch.stack([resize_center_crop(im.cuda() if not im.is_cuda else im, resize, crop) for im in images])


# ------------------------------------------------------------------------------------------------------------------
# The whole batch in one launch (hawq_image_batch, hawq_amd/csrc/image_batch.hip; DESIGN.md "Batched Resize + CenterCrop")
MAX_TILE_ROWS = 16


@functools.lru_cache(maxsize=4096)
def _coeffs_host(in_size, out_size, lo, n):
    """(bounds int32 [n, 2] with ABSOLUTE first input indices, coefficients int32 [n, ksize], ksize) of output indices lo .. lo+n-1:
    the slices of ``bilinear_coeffs`` a crop window reads.  Host arrays, read-only, cached per geometry."""
    b, c, k = bilinear_coeffs(in_size, out_size)
    b, c = np.ascontiguousarray(b[lo:lo + n]), np.ascontiguousarray(c[lo:lo + n])
    b.setflags(write=False), c.setflags(write=False)
    return b, c, k


class BatchPlan:
    """What ``plan_batch`` returns: the host tables of one ``hawq_image_batch`` launch.
    ``desc``   ctypes array of ``_lib.ImageDesc``, one per image of ``sizes`` (``base`` left 0; ``fallback`` images keep an all-zero
               entry, which the launch leaves alone, and take no tile)
               (``desc_array``: the same memory as a numpy record array)
    ``tiles``  ctypes array of ``_lib.ImageTile`` (image, first crop row, crop rows), row order within an image
    ``coef``   int32 array: every distinct pass's bounds then coefficients, the ``*_off`` fields index it in words
    ``lds_bytes``  dynamic LDS of the launch = the largest band (0 when every image falls back)
    ``fallback``   indices of images whose single-row band exceeds the budget: they take the per-image path"""
    __slots__ = ("sizes", "resize", "crop", "desc", "desc_array", "tiles", "coef", "lds_bytes", "fallback")

    def ok(self) -> bool:
        """``hawq_image_batch_ok`` on these tables (no GPU work); the reason of a refusal is in ``hawq_last_error``."""
        return bool(_lib.load().hawq_image_batch_ok(self.desc, len(self.desc), self.tiles, len(self.tiles), self.coef.ctypes.data, self.coef.size,
                                                    self.crop, self.lds_bytes))


def band_pitch(crop: int) -> int:
    """bytes of one row of the LDS band: crop * 3 rounded up to whole dwords"""
    return (crop * 3 + 3) & ~3


_DESC = np.dtype(_lib.ImageDesc)   # numpy reads the ctypes layout: the tables are assembled as arrays and handed over as ctypes views
_TILE = np.dtype(_lib.ImageTile)


class _ImagePlan:
    """The part of ``plan_batch`` that depends on one image's size alone: ``rec`` the descriptor without base and offsets, as bytes;
    ``tiles`` int32 [k, 3] with the image column 0; ``lds`` the largest band in bytes; ``hkey`` / ``vkey`` the arguments of
    ``_coeffs_host`` for the two passes (None: skipped).  ``tiles`` is None for an image whose single-row band exceeds the budget."""
    __slots__ = ("rec", "tiles", "lds", "hkey", "vkey")


@functools.lru_cache(maxsize=16384)   # a validation set has far fewer sizes than images
def _image_plan(h, w, resize, crop, budget) -> _ImagePlan:
    oh, ow, top, left = resize_crop_geometry(h, w, resize, crop)
    if oh < crop or ow < crop:
        raise ValueError("image too small for the crop (torchvision pads here; ImageNet validation images never need it)")
    skip_h, skip_v = ow == w, oh == h
    g = _ImagePlan()
    g.hkey, g.vkey = (None if skip_h else (w, ow, left, crop)), (None if skip_v else (h, oh, top, crop))
    # input rows a tile of crop rows r0 .. r0+n-1 reads: first[r0] .. last[r0+n-1] (both non-decreasing in r)
    if skip_v:
        first, last = np.arange(top, top + crop), np.arange(top, top + crop) + 1
    else:
        bv = _coeffs_host(*g.vkey)[0]
        first, last = np.minimum.accumulate(bv[::-1, 0])[::-1], np.maximum.accumulate(bv[:, 0] + bv[:, 1])
    pitch = band_pitch(crop)
    rows = next((n for n in range(min(MAX_TILE_ROWS, crop), 0, -1) if int((last[n - 1:] - first[:crop - n + 1]).max()) * pitch <= budget), 0)
    rec = np.zeros(1, _DESC)   # all zero: an image the launch leaves alone
    if rows == 0:
        g.hkey = g.vkey = g.tiles = None
        g.lds = 0
    else:
        for name, v in (("h", h), ("w", w), ("oh", oh), ("ow", ow), ("top", top), ("left", left), ("skip_h", skip_h), ("skip_v", skip_v),
                        ("kh", 0 if skip_h else _coeffs_host(*g.hkey)[2]), ("kv", 0 if skip_v else _coeffs_host(*g.vkey)[2])):
            rec[name] = v
        r0 = np.arange(0, crop, rows, dtype=np.int32)
        n = np.minimum(rows, crop - r0).astype(np.int32)
        g.tiles = np.stack([np.zeros_like(r0), r0, n], 1)
        g.tiles.setflags(write=False)
        g.lds = int((last[r0 + n - 1] - first[r0]).max()) * pitch
    g.rec = rec.view(np.uint8)   # as bytes: numpy concatenates those without looking at the fields
    g.rec.setflags(write=False)
    return g


def plan_batch(sizes, resize: int = 256, crop: int = 224, lds_budget=None) -> BatchPlan:
    """Host plan of the one-launch Resize(resize) + CenterCrop(crop) of images with the given (h, w) (3 channels).  Pure host code.
    Per image: the largest number of crop rows per tile, at most ``MAX_TILE_ROWS``, whose band - the horizontally resampled crop
    columns of every input row those output rows read - fits ``lds_budget`` (default and ceiling: ``hawq_image_batch_lds_budget()``);
    the last tile of an image may be shorter.  Images too small for the crop raise ``ValueError`` as ``resize_center_crop`` does."""
    budget = _lib.load().hawq_image_batch_lds_budget()
    if lds_budget is not None:
        if lds_budget <= 0 or lds_budget > budget:
            raise ValueError(f"lds_budget {lds_budget} outside 1..{budget}")
        budget = int(lds_budget)
    plan = BatchPlan()
    plan.sizes, plan.resize, plan.crop = [(int(h), int(w)) for h, w in sizes], resize, crop
    per = [_image_plan(h, w, resize, crop, budget) for h, w in plan.sizes]
    plan.fallback = [i for i, g in enumerate(per) if g.tiles is None]
    # the packed coefficient table: bounds, then coefficients, of each distinct pass once (a skipped pass has none: offsets 0, never read)
    packed, words, placed, offs_of = [], 0, {None: (0, 0)}, {}
    for g in per:
        if g not in offs_of:
            for key in (g.hkey, g.vkey):
                if key not in placed:
                    bnd, cf, _ = _coeffs_host(*key)
                    placed[key] = (words, words + bnd.size)
                    packed += [bnd.reshape(-1), cf.reshape(-1)]
                    words += bnd.size + cf.size
            offs_of[g] = placed[g.hkey] + placed[g.vkey]
    plan.coef = np.concatenate(packed) if packed else np.zeros(1, np.int32)
    desc = (np.concatenate([g.rec for g in per]) if per else np.zeros(0, np.uint8)).view(_DESC)
    offs = np.array([offs_of[g] for g in per], np.int32).reshape(len(per), 4)
    for k, name in enumerate(("hb_off", "hc_off", "vb_off", "vc_off")):
        desc[name] = offs[:, k]
    tiled = [g.tiles for g in per if g.tiles is not None]
    tiles = np.concatenate(tiled) if tiled else np.zeros((0, 3), np.int32)
    tiles[:, 0] = np.repeat(np.arange(len(per), dtype=np.int32), [0 if g.tiles is None else len(g.tiles) for g in per])
    plan.lds_bytes = max((g.lds for g in per), default=0)
    plan.desc_array, plan.desc = desc, (_lib.ImageDesc * len(desc)).from_buffer(desc)
    plan.tiles = (_lib.ImageTile * len(tiles)).from_buffer(tiles)
    return plan


class _Staging:
    """A pinned host buffer and its device arena, kept and grown between batches.  The upload is one ``non_blocking`` copy on the
    current stream; the event recorded behind it is waited on before the host side is overwritten by the next batch."""

    def __init__(self):
        self.host = self.dev = self.event = None

    def reserve(self, nbytes: int, device):
        if self.event is not None:
            self.event.synchronize()   # the previous batch's copy has read the pinned buffer
            self.event = None
        if self.host is None or self.host.numel() < nbytes:
            self.host = torch.empty(max(nbytes, 2 * (self.host.numel() if self.host is not None else 0)), dtype=torch.uint8).pin_memory()
        if self.dev is None or self.dev.device != device or self.dev.numel() < nbytes:
            self.dev = torch.empty(self.host.numel(), dtype=torch.uint8, device=device)
        return self.host, self.dev

    def upload(self, nbytes: int):
        self.dev[:nbytes].copy_(self.host[:nbytes], non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record()


_STAGING = {}   # (device index, "images" | "tables") -> _Staging


def _align16(n: int) -> int:
    return (n + 15) & ~15


def preprocess_batch_fused(images, resize: int = 256, crop: int = 224, out=None, lds_budget=None, device=None) -> torch.Tensor:
    """``preprocess_batch`` in one launch: list of decoded uint8 HWC RGB images (any sizes; host, device or mixed) -> uint8
    [N, crop, crop, 3] on the MI355X, byte for byte what ``resize_center_crop`` gives per image.  Host images are packed into one pinned
    staging buffer and go up in one copy, device images are read in place, the tables of ``plan_batch`` go up in one more copy, and
    ``hawq_image_batch`` writes every crop straight into ``out`` (a contiguous uint8 [N, crop, crop, 3] device tensor or view, e.g. an
    engine's input buffer; a fresh tensor without it).  Images the plan lists as ``fallback`` take ``resize_center_crop`` into the same
    ``out``.  Work is enqueued on the current stream; the staging buffers are reused, so call it from one stream per device."""
    images = list(images)
    if not images:
        raise ValueError("empty batch")
    for im in images:
        if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3:
            raise ValueError("expected uint8 HWC tensors with 3 channels (other channel counts: resize_center_crop per image)")
    if out is not None:
        dev = out.device
    elif device is not None:
        dev = torch.device(device)
    else:
        dev = next((im.device for im in images if im.is_cuda), torch.device("cuda"))
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    n = len(images)
    if out is None:
        out = torch.empty(n, crop, crop, 3, dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (n, crop, crop, 3) or not out.is_cuda or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint8 [{n}, {crop}, {crop}, 3] tensor on the MI355X")
    plan = plan_batch([im.shape[:2] for im in images], resize, crop, lds_budget)
    fallback = set(plan.fallback)
    with torch.cuda.device(dev):
        if len(fallback) < n:
            # images: device ones in place, host ones packed at 16-byte aligned offsets of the staging buffer -> one copy
            images = [im if im.is_contiguous() else im.contiguous() for im in images]
            host_at, total = {}, 0
            for i, im in enumerate(images):
                if im.is_cuda:
                    if im.device != dev:
                        raise ValueError(f"image {i} is on {im.device}, the batch on {dev}")
                elif i not in fallback:
                    host_at[i], total = total, _align16(total + im.numel())
            if host_at:
                st = _STAGING.setdefault((dev.index, "images"), _Staging())
                hbuf, arena = st.reserve(total, dev)
                for i, off in host_at.items():
                    hbuf[off:off + images[i].numel()].copy_(images[i].reshape(-1))
                st.upload(total)
            base = arena.data_ptr() if host_at else 0
            plan.desc_array["base"] = [0 if i in fallback else base + host_at[i] if i in host_at else images[i].data_ptr() for i in range(n)]
            if not plan.ok():   # on the host tables, before anything is uploaded or launched
                raise RuntimeError("libhawq_mi355: " + _lib.load().hawq_last_error().decode())
            # descriptors | tiles | coefficients -> one copy
            nd, nt, nc = C.sizeof(plan.desc), C.sizeof(plan.tiles), plan.coef.nbytes
            o_t, o_c = _align16(nd), _align16(_align16(nd) + nt)
            st = _STAGING.setdefault((dev.index, "tables"), _Staging())
            hbuf, tab = st.reserve(o_c + nc, dev)
            hnp = hbuf.numpy()
            hnp[:nd] = np.frombuffer(plan.desc, np.uint8)
            hnp[o_t:o_t + nt] = np.frombuffer(plan.tiles, np.uint8)
            hnp[o_c:o_c + nc] = plan.coef.view(np.uint8)
            st.upload(o_c + nc)
            _lib.call("hawq_image_batch", tab.data_ptr(), n, tab.data_ptr() + o_t, len(plan.tiles), tab.data_ptr() + o_c, out.data_ptr(), crop,
                      plan.lds_bytes, torch.cuda.current_stream(dev).cuda_stream)
        for i in plan.fallback:
            out[i].copy_(resize_center_crop(images[i].to(dev), resize, crop))
    return out


# ------------------------------------------------------------------------------------------------------------------
# Host side of the data path (quant_train.py:428-445): the files of an ImageFolder tree, decoded as its pil_loader does
IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")


def decode_image(source, draft=None) -> torch.Tensor:
    """File path, bytes or file object -> uint8 HWC RGB tensor (host), decoded as torchvision's ``pil_loader`` does
    (``Image.open(f).convert('RGB')``).  ``draft``: None, or a (width, height) pair: ``im.draft("RGB", draft)`` first - a JPEG is then
    decoded at the largest of 1/8, 1/4, 1/2 of its size that is still at least that large (``jpeg.draft_scale``), other formats as
    without it.  Needs Pillow - the decoder is not part of the integer hot path."""
    if draft is not None:
        from .jpeg import check_draft
        draft = check_draft(draft)
    try:
        from PIL import Image
    except ImportError as e:   # pragma: no cover - the build container has Pillow
        raise RuntimeError("hawq_amd.image.decode_image needs Pillow; pass decoded uint8 HWC tensors to preprocess_batch instead") from e
    import io
    if isinstance(source, (bytes, bytearray, memoryview)):
        source = io.BytesIO(bytes(source))
    with Image.open(source) as im:
        if draft is not None:
            im.draft("RGB", draft)
        arr = np.array(im.convert("RGB"))   # a copy: Pillow's buffer is read-only
    return torch.from_numpy(arr)


def image_folder(root: str):
    """(path, class index) pairs of an ImageFolder tree: class = sub-directory, indices by sorted directory name, files in
    sorted walk order (torchvision.datasets.folder.make_dataset)."""
    import os
    classes = sorted(d.name for d in os.scandir(root) if d.is_dir())
    if not classes:
        raise FileNotFoundError(f"no class directories under {root}")
    samples = []
    for idx, c in enumerate(classes):
        for dirpath, _, files in sorted(os.walk(os.path.join(root, c), followlinks=True)):
            samples += [(os.path.join(dirpath, f), idx) for f in sorted(files) if f.lower().endswith(IMG_EXTENSIONS)]
    return samples, classes


def decoded_batches(samples, batch_size: int, workers: int = 0, decode=decode_image):
    """The decode stage of ``folder_loader``: ``(list of decoded host images, list of class indices)`` per batch of ``samples`` =
    (path, class index) pairs, in their order.  ``workers`` > 0 (at most 16) decodes with that many threads - Pillow's decoders release
    the GIL - and keeps ONE batch in flight ahead of the one handed out, so the decoding of batch k+1 overlaps whatever the consumer
    does with batch k.  The result does not depend on ``workers``."""
    parts = [samples[i:i + batch_size] for i in range(0, len(samples), batch_size)]
    if workers <= 0:
        for part in parts:
            yield [decode(p) for p, _ in part], [t for _, t in part]
        return
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(int(workers), 16)) as pool:
        ahead = [pool.submit(decode, p) for p, _ in parts[0]] if parts else None
        for k, part in enumerate(parts):
            cur, ahead = ahead, ([pool.submit(decode, p) for p, _ in parts[k + 1]] if k + 1 < len(parts) else None)
            yield [f.result() for f in cur], [t for _, t in part]


def folder_loader(root: str, batch_size: int = 128, resize: int = 256, crop: int = 224, device="cuda", fused: bool = False, workers: int = 0,
                  device_decode: bool = False, entropy: str = "serial", progressive: bool = False, resume=None, front_end: str = "host", draft: bool = False):
    """Iterate an ImageFolder tree as ``(uint8 [n, crop, crop, 3] on the MI355X, int64 targets)`` batches - the validation loader of
    quant_train.py:428-445 (shuffle off) with everything behind the decoder on the device; feed it to ``api.validate(uint8=True)``.
    The defaults are the ResNets' geometry; InceptionV3 wants ``resize=342, crop=299`` (``eval_geometry(arch)``).
    ``fused``: resample each batch in one launch (``preprocess_batch_fused``: one upload instead of one per image).  ``workers``: decode
    with that many threads (at most 16), one batch ahead of the GPU (``decoded_batches``).  ``device_decode``: the threads only read the
    files; baseline JPEGs are decoded on the MI355X and everything else by the host decoder (``jpeg.decode_jpeg_batch``), and the batch is
    resampled in place by ``preprocess_batch_fused`` (implies ``fused``); ``entropy`` goes to ``decode_jpeg_batch`` (``"sync"``: many
    lanes per long restart interval); ``progressive`` (needs ``device_decode``): progressive JPEGs are decoded on the MI355X too, with
    ``"device"`` (needs ``front_end="device"``) from headers the MI355X has walked and a blob it has written itself;
    ``resume`` (needs ``device_decode``): a ``jpeg.ResumeIndex`` or the path of a saved one - the files it has an entry for are decoded
    from their recorded resume points, many waves per long restart interval; ``front_end`` (``"device"`` needs ``device_decode``): the
    MI355X walks the headers of the baseline files and writes their blob itself (``jpeg.decode_jpeg_batch``).  Same order, labels and bytes
    either way.  ``draft``: JPEGs are decoded at a reduced size where that still leaves at least ``resize`` pixels on both sides (Pillow's
    draft mode with the request (resize, resize), so ``Resize(resize)`` never enlarges), on the device with ``device_decode`` and by Pillow
    otherwise: what ``decode_image(f, draft=(resize, resize))`` + ``preprocess_batch_fused`` yield, which for a file of at least twice
    the requested size is NOT what the loader yields without it."""
    if draft not in (False, True):
        raise ValueError(f"draft must be False or True, not {draft!r}")
    if front_end not in ("host", "device"):
        raise ValueError(f"front_end must be 'host' or 'device', not {front_end!r}")
    if front_end == "device" and not device_decode:
        raise ValueError("front_end='device' needs device_decode=True")
    if progressive not in (False, True, "device"):
        raise ValueError(f"progressive must be False, True or 'device', not {progressive!r}")
    if progressive and not device_decode:
        raise ValueError("progressive=True needs device_decode=True")
    if isinstance(progressive, str) and front_end != "device":
        raise ValueError("progressive='device' needs front_end='device'")
    if resume is not None and not device_decode:
        raise ValueError("resume needs device_decode=True")
    samples, _ = image_folder(root)
    if device_decode:
        from . import jpeg
        more = {"progressive": progressive} if progressive else {}
        if resume is not None:
            more["resume"] = resume if isinstance(resume, jpeg.ResumeIndex) else jpeg.ResumeIndex.load(resume)
        if front_end != "host":
            more["front_end"] = front_end
        if draft:
            more["draft"] = (resize, resize)
        for datas, targets in decoded_batches(samples, batch_size, workers, decode=jpeg.read_source):
            imgs, _ = jpeg.decode_jpeg_batch(datas, device, entropy=entropy, **more)
            yield preprocess_batch_fused(imgs, resize, crop, device=device), torch.tensor(targets, dtype=torch.int64)
        return
    for imgs, targets in decoded_batches(samples, batch_size, workers, **({"decode": functools.partial(decode_image, draft=(resize, resize))} if draft else {})):
        if fused:
            batch = preprocess_batch_fused(imgs, resize, crop, device=device)
        else:
            batch = preprocess_batch([im.to(device) for im in imgs], resize, crop)
        yield batch, torch.tensor(targets, dtype=torch.int64)
