"""Whole plans with every activation buffer between guard bands: ``_alloc`` of the ResNet and the MobileNetV2 engine is
replaced, inside the test only, by an allocation from a tests/guard.py arena (tuning launches included: every tile the tuner
times runs under guard).  The logits must equal, bit for bit, those of an engine built without the patch on the same input, and
no guard byte may change - through the captured graph and with HAWQ_NO_GRAPH, at ragged batches."""
import pytest
import torch

import tests.test_gpu_splitk_network as SN
from tests import guard

pytestmark = pytest.mark.gpu


def _patch(mp, cls, arena, slack):
    """cls._alloc from the arena; `slack` elements stay between the view and its tail guard (MobileNetV2Engine._alloc's contract)."""
    def _alloc(self, n, dtype):
        return arena.empty(n + slack, dtype, f"activation {len(arena.bufs)} ({n} x {str(dtype)[6:]})")[:n]
    mp.setattr(cls, "_alloc", _alloc)


def _report(arena, what):
    n = len(arena.bufs)
    print(f"{what}: {n} guarded buffers, {arena.peak_bytes / 2 ** 20:.0f} MiB in the arena, "
          f"torch peak {torch.cuda.max_memory_allocated() / 2 ** 20:.0f} MiB")
    assert n > 20, "the engine did not allocate through the patched _alloc"


@pytest.mark.parametrize("arch,scheme,batch", [("resnet18", "uniform8", 1), ("resnet18", "uniform8", 3), ("resnet50", "uniform8", 3),
                                               ("resnet50", "bops_0.5", 3)])
def test_resnet_plan_under_guard(arch, scheme, batch, monkeypatch):
    from hawq_amd.engine import IntegerEngine
    from hawq_amd.skeleton import synthetic_images
    model = SN._model(arch, scheme)
    x = synthetic_images(batch, seed=5).cuda()
    arena = guard.GuardArena("cuda")
    with monkeypatch.context() as mp:
        _patch(mp, IntegerEngine, arena, 0)
        eng = IntegerEngine(model)           # tuned here: every candidate launch of the tuner runs between guards
        y_graph = eng(x).clone()
        y_replay = eng(x).clone()
        arena.check()
        plan = eng.export_plan()
        mp.setenv("HAWQ_NO_GRAPH", "1")
        direct = IntegerEngine(model, autotune=False, chains=1)
        assert not direct.use_graph
        y_direct = direct(x).clone()
        arena.check()
        assert not eng.overflowed() and not direct.overflowed()
    _report(arena, f"{arch} {scheme} b{batch}")
    ref = IntegerEngine(model, plan=plan)    # the same plan on plain torch.empty buffers
    y_ref = ref(x)
    assert ref.plan_source.startswith("replayed")
    assert torch.equal(y_graph, y_ref) and torch.equal(y_replay, y_ref) and torch.equal(y_direct, y_ref)


def test_resnet50_batch1_with_split_k_forced_under_guard(monkeypatch):
    from hawq_amd.engine import IntegerEngine
    from hawq_amd.skeleton import synthetic_images
    model = SN._model("resnet50", "uniform8")
    x = synthetic_images(1, seed=5).cuda()
    arena = guard.GuardArena("cuda")
    with monkeypatch.context() as mp:
        _patch(mp, IntegerEngine, arena, 0)
        eng, plan, n_split = SN._forced_engine(model, 1)
        y1 = eng(x).clone()
        y2 = eng(x).clone()
        assert eng.plan_source.startswith("replayed") and eng.n_splitk() == n_split > 0
        arena.check()
        mp.setenv("HAWQ_NO_GRAPH", "1")
        direct = IntegerEngine(model, plan=plan)
        y3 = direct(x).clone()
        assert not direct.use_graph and direct.n_splitk() == n_split
        arena.check()
    _report(arena, "resnet50 uniform8 b1 split-K")
    ref = IntegerEngine(model, plan=plan)
    y_ref = ref(x)
    assert ref.n_splitk() == n_split
    assert torch.equal(y1, y_ref) and torch.equal(y2, y_ref) and torch.equal(y3, y_ref)


@pytest.mark.parametrize("scheme", ["uniform8", "bops_0.5"])
@pytest.mark.parametrize("hw", [(224, 224), (72, 104)])
def test_mobilenetv2_plan_under_guard(scheme, hw, monkeypatch):
    from hawq_amd.api import build_quantized_model, calibrate
    from hawq_amd.engine_mbv2 import MobileNetV2Engine
    from hawq_amd.skeleton import synthetic_images
    model = build_quantized_model("mobilenetv2_w1", scheme, seed=0).cuda()
    calibrate(model, synthetic_images(2, 0).cuda())
    x = (synthetic_images(3, seed=9) * 1.1).cuda()
    if hw != (224, 224):
        x = torch.nn.functional.interpolate(x, size=hw, mode="bilinear", align_corners=False).contiguous()
    arena = guard.GuardArena("cuda")
    with monkeypatch.context() as mp:
        _patch(mp, MobileNetV2Engine, arena, 64)
        eng = MobileNetV2Engine(model)
        y_graph = eng(x).clone()
        y_replay = eng(x).clone()
        arena.check()
        assert eng.n_fused_units >= 7 and eng._stem_args is not None   # the one-launch units and stem are what runs
        direct = MobileNetV2Engine(model, chains=1, use_graph=False)   # (this engine has no HAWQ_NO_GRAPH switch: the constructor's)
        y_direct = direct(x).clone()
        arena.check()
    _report(arena, f"mobilenetv2 {scheme} {hw}")
    y_ref = MobileNetV2Engine(model)(x)
    assert torch.equal(y_graph, y_ref) and torch.equal(y_replay, y_ref) and torch.equal(y_direct, y_ref)
