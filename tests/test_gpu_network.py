"""Whole-network GPU parity: hawq_amd (HIP) vs the live reference's golden fixtures and vs
the CPU oracle.  Bit-exact on int32 accumulators, frozen ranges, logits and top-1."""
import os

import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu


def _images(b=2):
    from hawq_amd.skeleton import synthetic_images
    return synthetic_images(b, 0)


@pytest.mark.parametrize("arch,scheme", H.NET_CONFIGS + H.NET_CONFIGS_EXTRA)
def test_network_matches_reference_golden(arch, scheme):
    from hawq_amd.api import calibrate
    from hawq_amd.engine import IntegerEngine

    fx = H.net_fixture(arch, scheme)
    x = _images()
    assert H.sha(x.numpy()) == str(fx["input_sha"])
    model = H.build_model(arch, scheme)
    xd = x.cuda()
    # On the six base fixtures the IEEE-prepared paths coincide with the reference everywhere; deeper graphs can
    # contain a weight integer flipped by the reference's host-dependent sqrt early enough to move
    # later calibration ranges by an ulp or two - there only the reference-checkpoint comparison (4) is exact.
    strict_ieee = (arch, scheme) in H.NET_CONFIGS
    # 1. range calibration through the module-by-module HIP path reproduces the reference's ranges
    calibrate(model, xd)
    bad = [(n, m.x_min.item(), float(fx["act_x_min"][i]), m.x_max.item(), float(fx["act_x_max"][i]))
           for i, (n, m) in enumerate(H.act_modules(model))
           if m.x_min.item() != float(fx["act_x_min"][i]) or m.x_max.item() != float(fx["act_x_max"][i])]
    assert not (strict_ieee and bad), bad[:4]
    # 2. module-by-module frozen forward == reference logits
    with torch.no_grad():
        y_mod = model.forward_modules(xd)
    # 3. fused integer plan, own (IEEE) preparation
    eng = IntegerEngine(model, keep_accumulators=True, use_graph=False)
    y_int = eng(xd).clone()
    # 4. fused plan on the reference's integer checkpoint: the rigorous comparison
    H.load_reference_ranges(model, fx)
    H.load_reference_integer_ckpt(model, fx)
    eng_ck = IntegerEngine(model, from_buffers=True, keep_accumulators=True, use_graph=False)
    y_ck = eng_ck(xd).clone()
    assert not eng_ck.overflowed()
    ref = fx["logits"]
    assert np.array_equal(y_ck.cpu().numpy(), ref), np.abs(y_ck.cpu().numpy() - ref).max()
    assert np.array_equal(y_ck.argmax(1).cpu().numpy(), fx["top1"])
    for li, n in enumerate(fx["conv_names"]):
        key = "stem" if str(n).startswith("quant_init") else str(n)
        assert np.array_equal(H.digest(eng_ck.accumulators(key)), fx["conv_accdigest"][li]), n
    nout = ref.shape[1]
    assert np.array_equal(eng_ck.accumulators("quant_output").reshape(2, -1)[:, :nout], fx["fc_acc"])
    # the IEEE-prepared paths agree with the reference too on these fixtures (sqrt quirk does not
    # flip any rounding here); top-1 must agree regardless
    if strict_ieee:
        assert np.array_equal(y_int.cpu().numpy(), ref)   # same LOGITS as the reference on the six base fixtures
        assert np.array_equal(y_int.argmax(1).cpu().numpy(), fx["top1"])
        assert np.array_equal(y_mod.argmax(1).cpu().numpy(), fx["top1"])
    assert np.array_equal(y_int.cpu().numpy(), y_mod.cpu().numpy())


def test_real_image_fixture():
    from hawq_amd.api import calibrate
    fx = H.load("net_resnet18_uniform8_realimg.npz")
    x = torch.from_numpy(np.load(H.GOLDEN + "/real_image_nchw.npy"))
    model = H.build_model("resnet18", "uniform8")
    calibrate(model, x.cuda())
    y = model(x.cuda())
    assert np.array_equal(y.cpu().numpy(), fx["logits"])


@pytest.mark.parametrize("arch,scheme,batch", [("resnet18", "uniform8", 1), ("resnet18", "uniform8", 5), ("resnet50", "uniform4", 3),
                                                ("resnet50", "bops_0.5", 4), ("resnet50", "uniform8", 16)])
def test_network_matches_oracle_on_unseen_inputs(arch, scheme, batch):
    """Out-of-calibration inputs (larger magnitude -> un-clamped residuals beyond 32767), batch
    sizes that leave ragged tiles; graph replay must equal eager launches; uint16 and int32
    residual plans must agree."""
    from hawq_amd.api import calibrate
    from hawq_amd.engine import IntegerEngine
    from hawq_amd.skeleton import synthetic_images
    from oracle import oracle

    model = H.build_model(arch, scheme)
    calibrate(model, _images().cuda())
    x = synthetic_images(batch, seed=7) * 1.7 + 0.2
    st = oracle.extract_float_state(model)
    ref, tr = oracle.forward_int(st, x.numpy())
    eng = IntegerEngine(model, use_graph=True)
    y1 = eng(x.cuda()).clone()
    y2 = eng(x.cuda()).clone()  # second call replays the captured hipGraph
    eng32 = IntegerEngine(model, residual_bits=32, use_graph=False)
    y3 = eng32(x.cuda()).clone()
    assert np.array_equal(y1.cpu().numpy(), ref)
    assert torch.equal(y1, y2) and torch.equal(y1, y3)
    assert not eng.overflowed()
    mx = max(int(v.max()) for k, v in tr.items() if k.endswith("quant_act_int32.q"))
    print(f"{arch} {scheme}: max un-clamped residual {mx}")


@pytest.mark.parametrize("arch,scheme", [("resnet101", "uniform8"), ("resnet50b", "uniform4"), ("resnet50", "latency_0.5"),
                                         ("resnet50", "modelsize_0.25"), ("resnet18", "bops_0.5"), ("resnet18", "uniform4")])
def test_other_architectures_and_schedules_match_oracle(arch, scheme):
    """The remaining shipped graphs / bit schedules (ResNet101, the stride-on-3x3 ResNet50b, mixed-width
    schedules with W4A8 / W8A4 layers) against the CPU oracle on unseen inputs."""
    from hawq_amd.api import calibrate
    from hawq_amd.skeleton import synthetic_images
    from oracle import oracle
    model = H.build_model(arch, scheme)
    calibrate(model, _images().cuda())
    x = synthetic_images(3, seed=5) * 1.2
    ref, _ = oracle.forward_int(oracle.extract_float_state(model), x.numpy())
    y = model(x.cuda())
    assert np.array_equal(y.cpu().numpy(), ref)
    assert not model._engine.overflowed()


@pytest.mark.parametrize("batch", [3, 50])
def test_uint8_image_input_equals_the_normalised_fp32_path(batch):
    """forward_uint8 (uint8 NHWC images + host-built look-up table in the stem kernel) against the same engine fed
    with the fp32 tensor the reference's pipeline builds on the host (ToTensor + Normalize, quant_train.py:432-440);
    batch 50 runs as concurrent sub-batches.  Also a second (mean, std) to see the table refresh."""
    from hawq_amd.api import calibrate
    from hawq_amd.engine import IntegerEngine
    model = H.build_model("resnet50", "uniform8")
    calibrate(model, _images().cuda())
    g = torch.Generator().manual_seed(batch)
    xu8 = torch.randint(0, 256, (batch, 224, 224, 3), dtype=torch.uint8, generator=g)
    eng = IntegerEngine(model)
    for mean, std in (((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)), ((0.5, 0.4, 0.45), (0.25, 0.2, 0.3))):
        t = xu8.permute(0, 3, 1, 2).to(torch.float32).div(255)                       # ToTensor
        t = t.sub_(torch.tensor(mean).view(1, 3, 1, 1)).div_(torch.tensor(std).view(1, 3, 1, 1))  # Normalize
        ref = eng(t.cuda()).clone()
        y = eng.forward_uint8(xu8.cuda(), mean, std).clone()
        assert torch.equal(y, ref)
        assert torch.equal(eng.forward_uint8(xu8.cuda(), mean, std), ref)  # graph replay
    assert ref.abs().max() > 0 and not eng.overflowed()


def test_validate_loop_fp32_and_uint8():
    """hawq_amd.api.validate (the body of quant_train.py:validate) on a synthetic labelled set: labels are the
    network's own top-1 on half of the images and its lowest-ranked class on the rest -> exactly 50 % / 50 %; the
    uint8 pipeline must count the same images."""
    from hawq_amd.api import calibrate, validate
    model = H.build_model("resnet18", "uniform8")
    calibrate(model, _images().cuda())
    g = torch.Generator().manual_seed(1)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    batches_u8 = [torch.randint(0, 256, (n, 224, 224, 3), dtype=torch.uint8, generator=g) for n in (6, 4)]
    def norm(xu8):
        t = xu8.permute(0, 3, 1, 2).to(torch.float32).div(255)
        return t.sub_(torch.tensor(mean).view(1, 3, 1, 1)).div_(torch.tensor(std).view(1, 3, 1, 1))
    fp32, u8 = [], []
    for xu8 in batches_u8:
        logits = model(norm(xu8).cuda())
        top = logits.topk(5, 1, True, True)  # same op, same device as validate(): identical tie-breaking
        target = top.indices[:, 0].clone()
        worst = logits.argmin(1)
        assert (logits.gather(1, worst.view(-1, 1)).view(-1) < top.values[:, 4]).all()
        target[::2] = worst[::2]  # every other label is the lowest-ranked class: wrong for top-1 and top-5
        target = target.cpu()
        fp32.append((norm(xu8), target))
        u8.append((xu8, target))
    t1, t5, n = validate(model, fp32)
    assert (t1, t5, n) == (50.0, 50.0, 10)
    assert validate(model, u8, uint8=True) == (50.0, 50.0, 10)   # batch shape changes between the two batches:
    assert validate(model, u8, uint8=True) == (50.0, 50.0, 10)   # the rebuilt engine must re-upload its table


def test_validate_from_a_jpeg_folder_equals_the_reference_pipeline_on_pillow(tmp_path):
    """The validation data path of quant_train.py:428-445 end to end: an ImageFolder tree of JPEGs -> pil_loader decode (host, as in
    the reference's DataLoader workers) -> Resize(256) + CenterCrop(224) + ToTensor + Normalize + input QuantAct on the MI355X
    (folder_loader -> validate(uint8=True)) against the same images put through PILLOW's own resize / crop and the fp32 tensor
    path: identical logits, hence identical accuracy counts.  Needs Pillow (skipped where it is not installed)."""
    pytest.importorskip("PIL")
    from PIL import Image
    from hawq_amd.api import calibrate, validate
    from hawq_amd.image import folder_loader
    model = H.build_model("resnet18", "uniform8")
    calibrate(model, _images().cuda())
    rng = np.random.default_rng(4)
    for c in ("a", "b", "c"):
        (tmp_path / c).mkdir()
        for k in range(3):
            h, w = (int(v) for v in rng.integers(240, 520, 2))
            yy, xx = np.mgrid[0:h, 0:w]
            pic = np.stack([(xx * 3 + k * 40) % 256, (yy * 2 + xx) % 256, rng.integers(0, 256, (h, w))], -1).astype(np.uint8)
            Image.fromarray(pic).save(tmp_path / c / f"{k}.jpg", quality=95)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    ref_logits, paths = [], []
    for c in ("a", "b", "c"):
        for k in range(3):
            im = Image.open(tmp_path / c / f"{k}.jpg").convert("RGB")
            w, h = im.size
            ow, oh = (256, int(256 * h / w)) if w <= h else (int(256 * w / h), 256)
            im = im.resize((ow, oh), Image.BILINEAR)
            top, left = int(round((oh - 224) / 2.0)), int(round((ow - 224) / 2.0))
            a = np.asarray(im)[top:top + 224, left:left + 224]
            t = torch.from_numpy(a.copy()).permute(2, 0, 1).unsqueeze(0).to(torch.float32).div(255)
            t = t.sub_(torch.tensor(mean).view(1, 3, 1, 1)).div_(torch.tensor(std).view(1, 3, 1, 1))
            ref_logits.append(model(t.cuda()).cpu())
    ref_logits = torch.cat(ref_logits)
    got = torch.cat([model.engine().forward_uint8(b, mean, std).cpu() for b, _ in folder_loader(str(tmp_path), batch_size=4)])
    assert torch.equal(got, ref_logits)
    # labels := the reference pipeline's top-1 for class-a files, something else for the rest -> accuracy is known
    pred = ref_logits.argmax(1)
    class Loader:   # folder_loader's batches with the labels swapped for checkable ones
        def __iter__(self):
            i = 0
            for b, t in folder_loader(str(tmp_path), batch_size=4):
                lab = pred[i:i + len(t)].clone()
                lab[t != 0] = ref_logits[i:i + len(t)].argmin(1)[t != 0]
                i += len(t)
                yield b, lab
    t1, t5, n = validate(model, Loader(), uint8=True)
    assert n == 9 and abs(t1 - 100.0 * 3 / 9) < 1e-9 and abs(t5 - 100.0 * 3 / 9) < 1e-9


def test_concurrent_sub_batches_are_bit_identical():
    """The engine may split a batch into 2-3 sub-batches that run concurrently inside one hipGraph (chosen by
    timing at batch >= 48, or forced): logits must not depend on the split (uneven splits included)."""
    from hawq_amd.api import calibrate
    from hawq_amd.engine import IntegerEngine
    from hawq_amd.skeleton import synthetic_images
    model = H.build_model("resnet50", "uniform8")
    calibrate(model, _images().cuda())
    x = (synthetic_images(50, seed=11) * 1.3).cuda()
    ref = IntegerEngine(model, chains=1)(x).clone()
    for chains in (2, 3, 0):
        eng = IntegerEngine(model, chains=chains)
        y = eng(x).clone()
        assert torch.equal(y, ref), chains
        assert torch.equal(eng(x), ref), chains   # graph replay
        if chains == 0:
            assert eng.chains in (1, 2, 3) and set(eng.chain_timing_ms) == {1, 2, 3}
        else:
            assert eng.chains == chains and len(eng.subs) == chains
            # the joint tuning pass leaves every chain with the same tile / fused-variant choice per layer
            for sub in eng.subs[1:]:
                assert [a.tile for a in sub._conv_args] == [a.tile for a in eng.subs[0]._conv_args]
                choice = lambda p: (p.fused, p.er.tile if p.fused else (p.expand.tile, p.reduce.tile if p.reduce is not None else 0))
                assert [choice(p) for p in sub._er_args] == [choice(p) for p in eng.subs[0]._er_args] or \
                       all(p.fused == q.fused for p, q in zip(sub._er_args, eng.subs[0]._er_args))
        assert not eng.overflowed()
    os.environ["HAWQ_JOINT_TUNE"] = "0"   # isolated timing only: another plan, the same logits
    try:
        assert torch.equal(IntegerEngine(model, chains=2)(x), ref)
    finally:
        del os.environ["HAWQ_JOINT_TUNE"]


def test_recorded_plan_replays_without_tuning_and_a_stale_plan_is_refused():
    """IntegerEngine.export_plan() -> IntegerEngine(model, plan=...): the second engine builds the recorded batch shape by REPLAY
    (same tiles / fused variants / chain count, identical logits, no joint timing tables), tunes any other batch shape as usual,
    and a plan recorded for another kernel inventory or launch list falls back to tuning (what bench.py --plan and the multi-GPU
    path rely on)."""
    import json
    from hawq_amd.api import calibrate
    from hawq_amd.engine import IntegerEngine
    from hawq_amd.skeleton import synthetic_images
    model = H.build_model("resnet50", "uniform8")
    calibrate(model, _images().cuda())
    x = (synthetic_images(48, seed=5) * 1.2).cuda()
    tuned = IntegerEngine(model, chains=2)
    ref = tuned(x).clone()
    plan = json.loads(json.dumps(tuned.export_plan()))   # survives a JSON round trip (profiles/plans.json, broadcast_object_list)
    assert plan["batch"] == 48 and plan["chains"] == 2 and len(plan["tiles"].split(".")) == len(plan["conv_launches"])
    assert tuned.plan_source == "tuned in this process"
    rep = IntegerEngine(model, plan=dict(plan, source="replayed unit-test plan"))
    y = rep(x).clone()
    assert torch.equal(y, ref) and torch.equal(rep(x), ref)
    got = rep.export_plan()
    assert {k: got[k] for k in ("batch", "chains", "tiles", "fused_variants", "fused_split_tiles")} == \
           {k: plan[k] for k in ("batch", "chains", "tiles", "fused_variants", "fused_split_tiles")}
    assert rep.plan_source == "replayed unit-test plan"
    assert not any(sub._tile_times or sub._er_times for sub in rep.subs)   # nothing was timed
    # another batch shape on the same engine: tuned, not replayed
    x2 = x[:5]
    assert torch.equal(rep(x2), IntegerEngine(model, chains=1)(x2))
    # stale plans: other tile inventory / other launch list -> tuning, same logits
    for bad in (dict(plan, num_conv_tiles=plan["num_conv_tiles"] + 1), dict(plan, conv_launches=plan["conv_launches"][:-1]),
                dict(plan, pair_variant_counts=[c + 1 for c in plan["pair_variant_counts"]])):
        e = IntegerEngine(model, plan=bad, chains=1)
        assert torch.equal(e(x), ref)
        assert e.plan_source == "tuned in this process"


def _same_plan(a, b):
    skip = ("git_head", "source")
    return {k: v for k, v in a.items() if k not in skip} == {k: v for k, v in b.items() if k not in skip}


def test_committed_two_chain_plan_replays_chain_by_chain():
    """profiles/plans.json["resnet50_uniform8_b32"] (2 chains, `per_chain`) on the model bench.py builds for it: replayed, each chain
    with its own recorded tiles, re-exported unchanged, logits bit-equal to an untuned one-chain engine."""
    import json
    from hawq_amd.api import calibrate
    from hawq_amd.engine import IntegerEngine
    from hawq_amd.skeleton import synthetic_images
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "plans.json")) as f:
        plan = json.load(f)["resnet50_uniform8_b32"]
    assert plan["chains"] == 2 and len(plan["per_chain"]) == 2
    model = H.build_model("resnet50", "uniform8")
    calibrate(model, synthetic_images(8, seed=0).cuda())
    x = synthetic_images(32, seed=1).cuda()
    eng = IntegerEngine(model, plan=dict(plan, source="replayed profiles/plans.json"))
    y = eng(x).clone()
    assert eng.plan_source.startswith("replayed")
    assert _same_plan(eng.export_plan(), plan)
    assert len(eng.subs) == 2
    for sub, rec in zip(eng.subs, plan["per_chain"]):
        assert [a.tile for a in sub._conv_args] == [int(t) for t in rec["tiles"].split(".")]
    assert torch.equal(y, IntegerEngine(model, chains=1, autotune=False)(x))


def test_chains_of_a_tuned_plan_replay_their_own_tiles():
    """Tune two chains at batch 8, give chain 1 another tile (one the tuner timed, so the library takes it) for one conv launch:
    the replay runs that tile in chain 1 only, records the chains one by one and computes the same logits."""
    import json
    from hawq_amd.api import calibrate
    from hawq_amd.engine import IntegerEngine
    from hawq_amd.skeleton import synthetic_images
    model = H.build_model("resnet50", "uniform8")
    calibrate(model, _images().cuda())
    x = (synthetic_images(8, seed=7) * 1.1).cuda()
    tuned = IntegerEngine(model, chains=2)
    ref = tuned(x).clone()
    plan = json.loads(json.dumps(tuned.export_plan()))
    tiles = [[a.tile for a in sub._conv_args] for sub in tuned.subs]
    unsplit = [v == 0 for v in tuned.subs[1].splitk_choice()]   # (a split launch does not run its tile)
    k, other = next((k, t) for k, name in enumerate(tuned.subs[1]._conv_names) if unsplit[k]
                    for t in tuned.subs[1]._tile_times[name] if t > 0 and t != tiles[1][k] and t != tiles[0][k])
    tiles[1][k] = other
    strings = lambda i: {"tiles": ".".join(map(str, tiles[i])), "fused_variants": plan["fused_variants"],
                         "fused_split_tiles": plan["fused_split_tiles"]}
    per = plan.get("per_chain") or [strings(0), strings(1)]
    per[1] = dict(per[1], tiles=strings(1)["tiles"])
    rep = IntegerEngine(model, plan=dict(plan, per_chain=per))
    y = rep(x).clone()
    assert rep.plan_source.startswith("replayed")
    assert [[a.tile for a in sub._conv_args] for sub in rep.subs] == tiles and tiles[0][k] != other
    got = rep.export_plan()
    assert [p["tiles"] for p in got["per_chain"]] == [strings(0)["tiles"], strings(1)["tiles"]] and got["tiles"] == plan["tiles"]
    assert torch.equal(y, ref) and torch.equal(rep(x), ref)


def test_model_call_uses_fused_engine_and_cpu_raises():
    from hawq_amd.api import calibrate
    model = H.build_model("resnet18", "uniform8")
    x = _images()
    with pytest.raises(RuntimeError):
        model.cpu().forward_modules(x)
    model = model.cuda()
    calibrate(model, x.cuda())
    y = model(x.cuda())
    assert model._engine is not None and y.shape == (2, 1000)


@pytest.mark.parametrize("scheme", ["uniform8", "uniform4", "bops_0.5"])
def test_mobilenetv2_matches_reference_golden(scheme):
    """Q_MobileNetV2 (q_mobilenetv2.py: 1x1 expand / 3x3 DEPTHWISE / 1x1 linear-bottleneck units, ReLU6, QuantConv2d classifier)
    module by module through the HIP library against the live reference's fixture: calibrated ranges (device min/max
    kernels), then - on the reference's frozen ranges and integer checkpoint - bit-identical logits."""
    import hashlib
    from hawq_amd.api import build_quantized_model, calibrate
    from hawq_amd.quant_modules import QuantAct, QuantBnConv2d, QuantConv2d
    fx = H.load(f"net_mobilenetv2_w1_{scheme}_b2.npz")
    x = _images()
    assert H.sha(x.numpy()) == str(fx["input_sha"])
    model = build_quantized_model("mobilenetv2_w1", scheme, seed=0).cuda()
    calibrate(model, x.cuda())
    acts = [(n, m) for n, m in model.named_modules() if isinstance(m, QuantAct)]
    assert [n for n, _ in acts] == [str(n) for n in fx["act_names"]]
    convs = [(n, m) for n, m in model.named_modules() if isinstance(m, (QuantBnConv2d, QuantConv2d))]
    assert [n for n, _ in convs] == [str(n) for n in fx["conv_names"]]
    off, same_scales = 0, True
    for n, m in convs:
        sc = (m.convbn_scaling_factor if isinstance(m, QuantBnConv2d) else m.conv_scaling_factor).cpu().numpy().reshape(-1)
        same_scales &= np.array_equal(sc, fx["conv_scale"][off:off + sc.size])
        off += sc.size
    bad = [n for i, (n, m) in enumerate(acts) if float(m.x_min) != float(fx["act_x_min"][i]) or float(m.x_max) != float(fx["act_x_max"][i])]
    assert not (same_scales and bad), bad[:4]   # (a weight scale one ulp off - DESIGN.md 2.2 - may move later ranges)
    with torch.no_grad():
        y_own = model.forward_modules(x.cuda())
    assert np.array_equal(y_own.argmax(1).cpu().numpy(), fx["top1"])
    # the rigorous comparison: the reference's ranges and integer buffers
    for i, (n, m) in enumerate(acts):
        m.x_min.fill_(float(fx["act_x_min"][i])), m.x_max.fill_(float(fx["act_x_max"][i]))
        m.compute_scale()
        assert m.act_scaling_factor.item() == float(fx["act_scale"][i]), n
    off = 0
    for li, (n, m) in enumerate(convs):
        w = m.weight_integer.detach().cpu().numpy().copy()
        for l, idx, val in fx["conv_wpatch"]:
            if l == li:
                w.reshape(-1)[idx] = val
        assert hashlib.sha256(np.ascontiguousarray(w.astype(np.int8)).tobytes()).hexdigest() == str(fx["conv_wsha"][li]), n
        co = w.shape[0]
        dev = m.weight_integer.device
        m.weight_integer = torch.from_numpy(w).to(dev)
        sc = torch.from_numpy(fx["conv_scale"][off:off + co].copy()).to(dev)
        if isinstance(m, QuantBnConv2d):
            m.convbn_scaling_factor = sc
            m.bias_integer = torch.from_numpy(fx["conv_bias"][off:off + co].astype(np.float32)).to(dev)
        else:
            m.conv_scaling_factor = sc
        m.use_integer_buffers = True
        m._prep_key = None
        off += co
    with torch.no_grad():
        y = model.forward_modules(x.cuda()).cpu().numpy()
    # The classifier is a QuantConv2d: the reference runs its fp32 conv on the UN-ROUNDED x / S_a (quant_modules.py:727-736), so
    # its logits carry a float error of the order of an ulp that no integer path reproduces; the integers they stand for
    # - rint(logit / (S_w[c] * S_a)) = the int32 accumulators - must agree, and the logits to within 2 ulp.
    s_out = model.output.conv_scaling_factor.cpu().numpy().reshape(1, -1).astype(np.float64) * float(model.quant_act_output.act_scaling_factor)
    assert np.array_equal(np.rint(y / s_out), np.rint(fx["logits"] / s_out))
    assert np.abs(y - fx["logits"]).max() <= 2 ** -22 * np.abs(fx["logits"]).max()
    assert np.array_equal(y.argmax(1), fx["top1"])
    if same_scales and not bad:
        assert np.array_equal(np.rint(y_own.cpu().numpy() / s_out), np.rint(fx["logits"] / s_out))


def test_mobilenetv2_concurrent_sub_batches_are_bit_identical():
    """MobileNetV2Engine may split a batch into two sub-batches whose chains run concurrently inside one hipGraph (chosen by timing
    at batch >= 16, or forced): logits must not depend on the split (an uneven one included), nor on the per-launch tile tuning."""
    from hawq_amd.api import build_quantized_model, calibrate
    from hawq_amd.engine_mbv2 import MobileNetV2Engine
    from hawq_amd.skeleton import synthetic_images
    model = build_quantized_model("mobilenetv2_w1", "uniform8", seed=0).cuda()
    calibrate(model, _images().cuda())
    x = (synthetic_images(21, seed=5) * 1.2).cuda()
    ref = MobileNetV2Engine(model, chains=1, use_graph=False)(x).clone()
    os.environ["HAWQ_MBV2_TILES"] = "0"     # the library's heuristic tiles, no tuning
    try:
        assert torch.equal(MobileNetV2Engine(model, chains=1)(x), ref)
    finally:
        del os.environ["HAWQ_MBV2_TILES"]
    for chains in (2, 0):
        eng = MobileNetV2Engine(model, chains=chains)
        assert torch.equal(eng(x), ref), chains
        assert torch.equal(eng(x), ref), chains   # graph replay
        if chains == 0:
            assert eng.chains in (1, 2) and set(eng.chain_timing_ms) == {1, 2}
        else:
            assert len(eng.subs) == 2 and [s._batch[0] for s in eng.subs] == [11, 10]


@pytest.mark.parametrize("organisation", ["planar", "pixel_major", "planar_1_group", "planar_2_groups"])
@pytest.mark.parametrize("scheme", ["uniform8", "bops_0.5"])
@pytest.mark.parametrize("hw", [(224, 224), (72, 104)])
def test_mobilenetv2_one_launch_units_equal_three_launches(scheme, hw, organisation, monkeypatch):
    """hawq_linear_bottleneck (one launch per unit: expand 1x1 -> depthwise 3x3 -> project 1x1 + quant_act_int32 + next QuantAct, the
    hidden tensors never leaving the CU) and hawq_stem3x3s2 (the init block as one launch) against the launches they replace: every unit-closing tensor (int8 block input of the next
    unit, int32 carrier where one is written) and the logits bit for bit - on the full 224 x 224 maps and on an odd geometry whose
    tiles hang over every edge (36 x 52 -> 18 x 26 -> 9 x 13 -> 5 x 7 -> 3 x 4 maps)."""
    from hawq_amd.api import build_quantized_model, calibrate
    from hawq_amd.engine_mbv2 import MobileNetV2Engine
    from hawq_amd.skeleton import synthetic_images
    model = build_quantized_model("mobilenetv2_w1", scheme, seed=0).cuda()
    calibrate(model, _images().cuda())
    x = (synthetic_images(3, seed=9) * 1.1).cuda()
    if hw != (224, 224):
        x = torch.nn.functional.interpolate(x, size=hw, mode="bilinear", align_corners=False).contiguous()
    monkeypatch.setenv("HAWQ_MBV2_UNFUSED", "1")
    three = MobileNetV2Engine(model, chains=1, use_graph=False)
    y3 = three(x).clone()
    assert three.n_fused_units == 0
    monkeypatch.delenv("HAWQ_MBV2_UNFUSED")
    # hawq_bottleneck_args.tile: 0 = planar hidden tensor, slice groups by the number of workgroups (4 groups on most units of this
    # small batch); 1 = the launch's first organisation; 2 / 3 = planar with 1 / 2 slice groups
    tile = {"planar": None, "pixel_major": "1", "planar_1_group": "2", "planar_2_groups": "3"}[organisation]
    if tile is not None:
        monkeypatch.setenv("HAWQ_MBV2_UNIT_TILE", tile)
    one = MobileNetV2Engine(model, chains=1, use_graph=False)
    y1 = one(x).clone()
    assert one.n_fused_units >= 7, one.n_fused_units   # units 1-10 of the width-1 network have <= 64-channel inputs and outputs
    assert one._stem_args is not None and three._stem_args is None   # the init block: hawq_stem3x3s2 against im2col + 1x1 conv
    assert len(one._ops) == len(three._ops) - 2 * one.n_fused_units - 1
    for name in sorted(one.taps):
        if name.endswith(":next_q") or name.endswith(":out16"):
            assert np.array_equal(one.tap(name), three.tap(name)), name
    assert torch.equal(y1, y3)


def test_mobilenetv2_uint8_input_equals_the_normalised_tensor_path():
    """MobileNetV2Engine.forward_uint8 (hawq_quantize_im2col3x3s2_u8: ToTensor + Normalize + input QuantAct as a table look-up
    feeding the init conv's im2col rows) == the fp32 path on the tensor the reference's pipeline builds (quant_train.py:428-440),
    one chain and two; api.validate(uint8=True) runs on it."""
    from hawq_amd.api import build_quantized_model, calibrate, validate
    from hawq_amd.engine_mbv2 import MobileNetV2Engine
    model = build_quantized_model("mobilenetv2_w1", "uniform8", seed=0).cuda()
    calibrate(model, _images().cuda())
    g = torch.Generator().manual_seed(7)
    for n, chains in ((3, 1), (18, 2)):
        xu8 = torch.randint(0, 256, (n, 224, 224, 3), dtype=torch.uint8, generator=g)
        xu8[0, :2] = 0
        xu8[0, 2:4] = 255
        eng = MobileNetV2Engine(model, chains=chains)
        for mean, std in (((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)), ((0.5, 0.4, 0.45), (0.25, 0.2, 0.3))):
            t = xu8.permute(0, 3, 1, 2).to(torch.float32).div(255)                       # ToTensor
            t = t.sub_(torch.tensor(mean).view(1, 3, 1, 1)).div_(torch.tensor(std).view(1, 3, 1, 1))  # Normalize
            ref = eng(t.cuda()).clone()
            assert torch.equal(eng.forward_uint8(xu8.cuda(), mean, std), ref), (n, chains, mean)
            assert torch.equal(eng.forward_uint8(xu8.cuda(), mean, std), ref)   # graph replay
        assert ref.abs().max() > 0
    labels = model(t.cuda()).argmax(1).cpu()
    mean, std = (0.5, 0.4, 0.45), (0.25, 0.2, 0.3)
    assert validate(model, [(xu8, labels)], uint8=True, mean=mean, std=std) == (100.0, 100.0, 18)


def _load_mobilenet_reference_state(model, fx):
    """the reference run's frozen ranges and integer checkpoint (tests/golden/net_mobilenetv2_*.npz) into `model`"""
    import hashlib
    from hawq_amd.quant_modules import QuantAct, QuantBnConv2d, QuantConv2d
    acts = [(n, m) for n, m in model.named_modules() if isinstance(m, QuantAct)]
    convs = [(n, m) for n, m in model.named_modules() if isinstance(m, (QuantBnConv2d, QuantConv2d))]
    assert [n for n, _ in acts] == [str(n) for n in fx["act_names"]] and [n for n, _ in convs] == [str(n) for n in fx["conv_names"]]
    for i, (n, m) in enumerate(acts):
        m.x_min.fill_(float(fx["act_x_min"][i])), m.x_max.fill_(float(fx["act_x_max"][i]))
        m.compute_scale()
        assert m.act_scaling_factor.item() == float(fx["act_scale"][i]), n
    off = 0
    for li, (n, m) in enumerate(convs):
        w = m.weight_integer.detach().cpu().numpy().copy()
        for l, idx, val in fx["conv_wpatch"]:
            if l == li:
                w.reshape(-1)[idx] = val
        assert hashlib.sha256(np.ascontiguousarray(w.astype(np.int8)).tobytes()).hexdigest() == str(fx["conv_wsha"][li]), n
        co, dev = w.shape[0], m.weight_integer.device
        m.weight_integer = torch.from_numpy(w).to(dev)
        sc = torch.from_numpy(fx["conv_scale"][off:off + co].copy()).to(dev)
        if isinstance(m, QuantBnConv2d):
            m.convbn_scaling_factor = sc
            m.bias_integer = torch.from_numpy(fx["conv_bias"][off:off + co].astype(np.float32)).to(dev)
        else:
            m.conv_scaling_factor = sc
        off += co
    return acts, convs


@pytest.mark.parametrize("scheme", ["uniform8", "uniform4", "bops_0.5"])
def test_mobilenetv2_integer_plan_matches_reference_golden(scheme):
    """The FUSED INTEGER PLAN of Q_MobileNetV2 (hawq_amd/engine_mbv2.py: int8 between the convs of a unit, int32 for the signed
    16-bit values between units, depthwise 3x3 with a fused requant, linear-bottleneck residuals without ReLU, ReLU6 folded
    into the clamps, channels padded to 64) against the live reference's fixture (tests/golden/make_kat_extra.py --mobilenet):
    on the reference's frozen ranges and integer checkpoint EVERY conv's int32 accumulators (54 convs incl. the 17 depthwise
    layers and the classifier) and EVERY tapped QuantAct's integers (block inputs, quant_act1/2, the 16-bit unit outputs with
    and without identity) must have the fixture's digests; logits as the module path: identical integers, within 2 ulp, same
    top-1.  Also: own preparation, plan vs module path; hipGraph replay."""
    from hawq_amd.api import build_quantized_model, calibrate
    from hawq_amd.engine_mbv2 import MobileNetV2Engine
    from hawq_amd.quant_modules import trust_integer_buffers
    fx = H.load(f"net_mobilenetv2_w1_{scheme}_b2.npz")
    x = _images()
    assert H.sha(x.numpy()) == str(fx["input_sha"])
    model = build_quantized_model("mobilenetv2_w1", scheme, seed=0).cuda()
    calibrate(model, x.cuda())
    with torch.no_grad():
        y_mod = model.forward_modules(x.cuda())
    y_plan = model(x.cuda())                      # frozen + eval + CUDA -> the fused plan (own, IEEE preparation)
    assert model._engine is not None and model._engine.use_graph
    s_own = model.output.conv_scaling_factor.cpu().numpy().reshape(1, -1).astype(np.float64) * float(model.quant_act_output.act_scaling_factor)
    assert np.array_equal(np.rint(y_plan.cpu().numpy() / s_own), np.rint(y_mod.cpu().numpy() / s_own))
    assert torch.equal(model(x.cuda()), y_plan)   # graph replay
    # the rigorous comparison: the reference's ranges and integer buffers, every stage tapped
    acts, convs = _load_mobilenet_reference_state(model, fx)
    trust_integer_buffers(model, True)
    model.invalidate_engine()
    eng = MobileNetV2Engine(model, from_buffers=True, keep_accumulators=True)
    y = eng(x.cuda()).cpu().numpy()
    units = [n[:-len(".quant_act")] for n, _ in acts if n.endswith(".quant_act")]
    unit_of = {u: f"unit{k + 1}" for k, u in enumerate(units)}

    def conv_tap(n):
        if n in ("init_block", "output"):
            return n
        if n == "features.final_block":
            return "final_block"
        u, c = n.rsplit(".", 1)
        return f"{unit_of[u]}.{c}"

    for li, (n, _) in enumerate(convs):
        assert np.array_equal(H.digest(eng.tap(conv_tap(n))), fx["conv_accdigest"][li]), n
    checked = 0
    for ai, (n, _) in enumerate(acts):
        if n == "quant_act_int32":
            tap = "init_block:out16"
        elif n == "quant_act_before_final_block":
            tap = f"unit{len(units)}.conv3:next_q"
        elif n == "quant_act_int32_final":
            tap = "final_block:out16"
        elif n.endswith(".quant_act"):
            k = units.index(n[:-len(".quant_act")])
            tap = "init_block:next_q" if k == 0 else f"unit{k}.conv3:next_q"
        elif n.endswith(".quant_act1") or n.endswith(".quant_act2"):
            tap = f"{unit_of[n.rsplit('.', 1)[0]]}.conv{n[-1]}:q"
        elif n.endswith(".quant_act_int32"):
            tap = f"{unit_of[n.rsplit('.', 1)[0]]}.conv3:out16"
        else:
            continue   # quant_input / quant_act_output: covered by the first conv's accumulators / the classifier's
        assert np.array_equal(H.digest(eng.tap(tap)), fx["act_outdigest"][ai]), (n, tap)
        checked += 1
    assert checked == len(acts) - 2
    s_out = model.output.conv_scaling_factor.cpu().numpy().reshape(1, -1).astype(np.float64) * float(model.quant_act_output.act_scaling_factor)
    assert np.array_equal(np.rint(y / s_out), np.rint(fx["logits"] / s_out))
    assert np.abs(y - fx["logits"]).max() <= 2 ** -22 * np.abs(fx["logits"]).max()
    assert np.array_equal(y.argmax(1), fx["top1"])
    # the same state through the model's own entry point (graph, no taps)
    assert np.array_equal(np.rint(model(x.cuda()).cpu().numpy() / s_out), np.rint(fx["logits"] / s_out))
