"""InceptionV3 from uint8 images on the GPU: hawq_incep_stem_u8 against exact host maths, InceptionEngine.forward_uint8 against the
fp32 plan on the normalised images (calibrated synthetic model and the reference's frozen state), plan behaviour, and the JPEG
folder -> validate path at Resize(342) + CenterCrop(299)."""
import hashlib

import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _normalise(u8, mean=MEAN, std=STD):
    """uint8 NHWC -> the reference pipeline's ToTensor + Normalize (float32 operations on the host), NCHW"""
    t = u8.permute(0, 3, 1, 2).to(torch.float32).div(255)
    return t.sub(torch.tensor(mean).view(1, 3, 1, 1)).div(torch.tensor(std).view(1, 3, 1, 1))


def _u8(n, h=299, w=299, seed=0):
    return torch.randint(0, 256, (n, h, w, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


# ------------------------------------------------------------------ 1. the kernel against host maths
def _dyadic(v, m, e):
    """round_half_even(v * m / 2^e) in exact integers (the rounding of fixedpoint_fn's requant, quant_utils.py:404-408)."""
    v, m = v.astype(np.int64), np.broadcast_to(np.asarray(m, np.int64), v.shape)
    t = v * m
    half = np.int64(1) << (e - 1)
    q = (t + half) >> e
    tie = ((t + half) & ((np.int64(1) << e) - 1)) == 0
    return np.where(tie, q & ~np.int64(1), q)


@pytest.mark.parametrize("shape", [(1, 299, 299), (3, 37, 53), (2, 3, 3), (5, 8, 9)], ids=lambda s: "{}x{}x{}".format(*s))
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("qrange", [(-128, 127), (0, 15)], ids=["int8", "uint4"])
def test_stem_u8_kernel_equals_host_maths(shape, relu, qrange):
    from hawq_amd import _lib
    from hawq_amd.engine_inception import pack_stem_u8_weights
    N, H_, W_ = shape
    Cout, ldo = 32, 48
    g = torch.Generator().manual_seed(N * 1000 + H_ + W_ + relu)
    x = torch.randint(0, 256, (N, H_, W_, 3), generator=g, dtype=torch.uint8)
    lut = torch.randint(-128, 128, (3, 256), generator=g, dtype=torch.int8)
    w = torch.randint(-128, 128, (Cout, 3, 3, 3), generator=g, dtype=torch.int8)
    b = torch.randint(-2 ** 16, 2 ** 16, (Cout,), generator=g, dtype=torch.int32)
    m = torch.randint(2 ** 29, 2 ** 31 - 1, (Cout,), generator=g, dtype=torch.int64).to(torch.int32)
    e = torch.randint(36, 44, (Cout,), generator=g, dtype=torch.int32)
    Ho, Wo = (H_ - 3) // 2 + 1, (W_ - 3) // 2 + 1
    # host: table gather -> int64 conv -> bias -> ReLU -> dyadic -> clamp
    q = torch.gather(lut.long().unsqueeze(0).expand(N * H_ * W_, 3, 256), 2, x.reshape(-1, 3, 1).long()).view(N, H_, W_, 3)
    acc = torch.nn.functional.conv2d(q.permute(0, 3, 1, 2).double(), w.double(), stride=2).round().long()
    v = (acc + b.long().view(1, -1, 1, 1)).numpy()
    if relu:
        v = np.maximum(v, 0)
    want = np.stack([_dyadic(v[:, c], int(m[c]), int(e[c])) for c in range(Cout)], 1)
    want = np.clip(want, *qrange).transpose(0, 2, 3, 1)
    # device
    dev = [t.cuda() for t in (x, lut, torch.from_numpy(pack_stem_u8_weights(w.numpy(), Cout)), b, m, e)]
    out = torch.full((N * Ho * Wo * ldo,), 0x5A, dtype=torch.int8, device="cuda")
    a = _lib.IncepConvArgs()
    a.in_, a.wgt, a.bias, a.out, a.m, a.ek = None, dev[2].data_ptr(), dev[3].data_ptr(), out.data_ptr(), dev[4].data_ptr(), \
        dev[5].data_ptr()
    a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.stride, a.pad_h, a.pad_w = N, H_, W_, 3, Cout, 3, 3, 2, 0, 0
    a.epilogue, a.relu, a.q_lo, a.q_hi, a.out_bits, a.ldo, a.c_off = _lib.INCEP_REQUANT, relu, qrange[0], qrange[1], 8, ldo, 0
    assert _lib.load().hawq_incep_stem_u8_ok(dev[0].data_ptr(), dev[1].data_ptr(), a) == 1
    _lib.call("hawq_incep_stem_u8", dev[0].data_ptr(), dev[1].data_ptr(), a, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().view(N, Ho, Wo, ldo)
    assert np.array_equal(got[..., :Cout].numpy().astype(np.int64), want)
    assert bool((got[..., Cout:] == 0x5A).all())   # the rest of each row is never touched
    assert len(np.unique(want)) > 4                  # the clamp did not flatten the test


def test_stem_u8_launch_refuses_a_bad_description():
    from hawq_amd import _lib
    a = _lib.IncepConvArgs()
    a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.stride = 1, 299, 299, 16, 32, 3, 3, 2
    with pytest.raises(RuntimeError, match="hawq_incep_stem_u8"):
        _lib.call("hawq_incep_stem_u8", None, None, a, None)


# ------------------------------------------------------------------ 2. parity with the fp32 plan, calibrated synthetic model
@pytest.fixture(scope="module")
def model():
    from hawq_amd.api import build_quantized_resnet, calibrate
    from hawq_amd.skeleton import synthetic_images
    q = build_quantized_resnet("inceptionv3", "uniform8", seed=1).cuda()
    calibrate(q, synthetic_images(2, seed=0, size=299).cuda())
    return q


def _units(eng, model):
    return {n: eng.unit_output(n) for n, _ in model.units()}


def _assert_same_as_fp32_plan(model, eng, u8, mean=MEAN, std=STD):
    with torch.no_grad():
        y32 = eng(_normalise(u8, mean, std).cuda())
        u32 = _units(eng, model)
        yu8 = eng.forward_uint8(u8.cuda(), mean, std)
        uu8 = _units(eng, model)
    for n in u32:
        assert np.array_equal(uu8[n], u32[n]), n
    assert torch.equal(yu8, y32)
    assert y32.abs().max() > 0
    return yu8


@pytest.mark.parametrize("batch", [1, 2, 5])
def test_forward_uint8_equals_the_fp32_plan(model, batch):
    _assert_same_as_fp32_plan(model, model.engine(), _u8(batch, seed=batch))


# ------------------------------------------------------------------ 3. the reference's frozen state, both schemes
def _load_reference_state(model, fx):
    """The reference run's frozen ranges and integer buffers (weights patched where torch-CPU's sqrt moved them) into `model`."""
    from hawq_amd.quant_modules import QuantAct, QuantBnConv2d, freeze_model
    acts = [(n, m) for n, m in model.named_modules() if isinstance(m, QuantAct)]
    convs = [(n, m) for n, m in model.named_modules() if isinstance(m, QuantBnConv2d)]
    assert [n for n, _ in acts] == [str(n) for n in fx["act_names"]]
    assert [n for n, _ in convs] == [str(n) for n in fx["conv_names"]]
    for i, (n, m) in enumerate(acts):
        m.x_min.fill_(float(fx["act_x_min"][i])), m.x_max.fill_(float(fx["act_x_max"][i]))
        m.compute_scale()
        assert m.act_scaling_factor.item() == float(fx["act_scale"][i]), n
    freeze_model(model)
    off = 0
    for li, (n, m) in enumerate(convs):
        m.prepare(torch.ones(1))
        w = m.weight_integer.detach().cpu().numpy().copy()
        for l, idx, val in fx["conv_wpatch"]:
            if l == li:
                w.reshape(-1)[idx] = val
        assert hashlib.sha256(np.ascontiguousarray(w.astype(np.int8)).tobytes()).hexdigest() == str(fx["conv_wsha"][li]), n
        co, dev = w.shape[0], m.weight_integer.device
        m.weight_integer = torch.from_numpy(w).to(dev)
        m.convbn_scaling_factor = torch.from_numpy(fx["conv_scale"][off:off + co].copy()).to(dev)
        m.bias_integer = torch.from_numpy(fx["conv_bias"][off:off + co].astype(np.float32)).to(dev)
        m.use_integer_buffers, m._prep_key = True, None
        off += co
    assert off == fx["conv_scale"].size
    return model


@pytest.mark.parametrize("scheme", ["uniform8", "uniform4"])
def test_forward_uint8_on_the_reference_state(scheme):
    from hawq_amd.api import build_quantized_resnet
    fx = H.load(f"net_inceptionv3_{scheme}_b2.npz")
    q = build_quantized_resnet("inceptionv3", scheme, seed=0).cuda()
    _load_reference_state(q, fx)
    q.invalidate_engine()
    _assert_same_as_fp32_plan(q, q.engine(), _u8(2, seed=11))


# ------------------------------------------------------------------ 4. plan behaviour
def test_uint8_plan_graph_eager_alternation_and_table_keys(model):
    from hawq_amd.engine_inception import InceptionEngine
    eng = model.engine()
    u = _u8(2, seed=21)
    uc = u.cuda()
    mean2, std2 = (0.5, 0.5, 0.5), (0.25, 0.3, 0.2)
    with torch.no_grad():
        y = eng.forward_uint8(uc)
        assert eng.n_launches_u8 == eng.n_launches - 2
        assert torch.equal(InceptionEngine(model, use_graph=False).forward_uint8(uc), y)
        # fp32 and uint8 calls alternate on one plan: no rebuild, same results
        x = _normalise(u).cuda()
        y32 = eng(x)
        plan = (eng.x_in.data_ptr(), eng.x_u8.data_ptr(), eng._graph.value, eng._graph_u8.value)
        for _ in range(2):
            assert torch.equal(eng.forward_uint8(uc), y) and torch.equal(eng(x), y32)
        assert plan == (eng.x_in.data_ptr(), eng.x_u8.data_ptr(), eng._graph.value, eng._graph_u8.value)
        assert torch.equal(y, y32)
        # another (mean, std): a new table, the result of a fresh engine and of the fp32 plan on that normalisation
        y2 = eng.forward_uint8(uc, mean2, std2)
        assert not torch.equal(y2, y)
        assert torch.equal(y2, InceptionEngine(model).forward_uint8(uc, mean2, std2))
        assert torch.equal(y2, eng(_normalise(u, mean2, std2).cuda()))
        # a new batch shape rebuilds the plan; its table must be uploaded again for the same (mean, std)
        y2b1 = eng.forward_uint8(uc[:1], mean2, std2)
        assert torch.equal(y2b1, InceptionEngine(model).forward_uint8(uc[:1], mean2, std2))
        assert torch.equal(y2b1, y2[:1])
        assert torch.equal(eng.forward_uint8(uc[:1]), y[:1])
        assert eng.n_launches_u8 == eng.n_launches - 2
    with pytest.raises(ValueError):
        eng.forward_uint8(uc.permute(0, 3, 1, 2).contiguous())
    with pytest.raises(ValueError):
        eng.forward_uint8(uc.float())


# ------------------------------------------------------------------ 5. JPEG folder -> validate at Resize(342) + CenterCrop(299)
def test_validate_from_a_jpeg_folder_at_the_inception_geometry(model, tmp_path):
    pytest.importorskip("PIL")
    from PIL import Image
    from hawq_amd.api import validate
    from hawq_amd.image import eval_geometry, folder_loader
    resize, crop = eval_geometry("inceptionv3")
    rng = np.random.default_rng(6)
    for c in ("a", "b", "c"):
        (tmp_path / c).mkdir()
        for k in range(3):
            h, w = (int(v) for v in rng.integers(320, 601, 2))
            yy, xx = np.mgrid[0:h, 0:w]
            pic = np.stack([(xx * 3 + k * 40) % 256, (yy * 2 + xx) % 256, rng.integers(0, 256, (h, w))], -1).astype(np.uint8)
            Image.fromarray(pic).save(tmp_path / c / f"{k}.jpg", quality=95)
    ref_logits = []
    with torch.no_grad():
        for c in ("a", "b", "c"):
            for k in range(3):
                im = Image.open(tmp_path / c / f"{k}.jpg").convert("RGB")
                w, h = im.size
                ow, oh = (resize, int(resize * h / w)) if w <= h else (int(resize * w / h), resize)
                im = im.resize((ow, oh), Image.BILINEAR)
                top, left = int(round((oh - crop) / 2.0)), int(round((ow - crop) / 2.0))
                a = np.asarray(im)[top:top + crop, left:left + crop]
                ref_logits.append(model(_normalise(torch.from_numpy(a.copy()).unsqueeze(0)).cuda()).cpu())
        ref_logits = torch.cat(ref_logits)
        got = torch.cat([model.engine().forward_uint8(b, MEAN, STD).cpu()
                         for b, _ in folder_loader(str(tmp_path), batch_size=4, resize=resize, crop=crop)])
    assert torch.equal(got, ref_logits)
    pred = ref_logits.argmax(1)

    class Loader:   # folder_loader's batches with labels whose accuracy is known: right for class a, worst-ranked for the rest
        def __iter__(self):
            i = 0
            for b, t in folder_loader(str(tmp_path), batch_size=4, resize=resize, crop=crop):
                lab = pred[i:i + len(t)].clone()
                lab[t != 0] = ref_logits[i:i + len(t)].argmin(1)[t != 0]
                i += len(t)
                yield b, lab
    t1, t5, n = validate(model, Loader(), uint8=True)
    assert n == 9 and abs(t1 - 100.0 * 3 / 9) < 1e-9 and abs(t5 - 100.0 * 3 / 9) < 1e-9
