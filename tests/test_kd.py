"""ROI-model knowledge distillation, the parts that need no GPU: the public surface against the reference's
recorded one (tests/golden/kd_surface.json), the wrapper's train / eval / state-dict semantics, the teacher
checkpoint loading (train_advanced.py:428-508) and the student-only save (:1281-1290)."""
import inspect
import json
import os

import pytest
import torch
import torch.nn as nn


@pytest.fixture(scope="module")
def surface(golden_dir):
    with open(os.path.join(golden_dir, "kd_surface.json")) as f:
        return json.load(f)


def _net(cout=4):
    return nn.Sequential(nn.Conv2d(3, cout, 1), nn.BatchNorm2d(cout), nn.Dropout(0.5))


def test_constructor_signatures_equal_reference(surface):
    import hiseg
    sig = inspect.signature(hiseg.DistillationLoss)
    assert list(sig.parameters) == surface["ctor_DistillationLoss"]
    defaults = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == surface["ctor_defaults_DistillationLoss"]
    assert list(inspect.signature(hiseg.DistillationLoss.forward).parameters) == surface["forward_args_DistillationLoss"]
    wsig = inspect.signature(hiseg.DistillationModelWrapper)
    assert list(wsig.parameters) == surface["ctor_DistillationModelWrapper"]
    assert {k: p.default for k, p in wsig.parameters.items() if p.default is not inspect.Parameter.empty} == \
        surface["ctor_defaults_DistillationModelWrapper"]
    for name in surface["wrapper_methods"]:
        assert callable(getattr(hiseg.DistillationModelWrapper, name)), name
    loss = hiseg.DistillationLoss(nn.Identity())
    assert loss.feature_match_layers == surface["feature_match_layers_default"]
    assert (loss.temperature, loss.alpha, loss.distill_logits, loss.distill_features) == (4.0, 0.7, True, False)
    assert hiseg.DistillationLoss(nn.Identity(), feature_match_layers=["a"], distill_features=True) \
        .feature_match_layers == ["a"]


def test_loss_dict_keys_equal_reference(surface):
    """The lazy dict, fed host values directly, yields the reference's keys in the reference's order."""
    from hiseg.kd import NOUT, LazyDistillationLossDict
    from kd_cases import STUB
    heads = {"all": (1, 1, 1), "taux_none": (1, 0, 0), "no_s_bgfg": (1, 0, 1), "no_t_bgfg": (1, 0, 1),
             "no_s_tn": (1, 1, 0), "no_t_tn": (1, 1, 0), "nologits": (0, 1, 1), "bare": (1, 1, 1)}
    for variant, terms in heads.items():
        d = LazyDistillationLossDict(torch.arange(NOUT + 2, dtype=torch.float32), terms, dict(STUB))
        assert list(d.keys()) == surface["dict_keys"][variant], variant
        assert d["total"] == NOUT + 1 and d["base_total"] == NOUT and d["base_ce_loss"] == STUB["ce_loss"]
    none = LazyDistillationLossDict(torch.zeros(NOUT + 2), (0, 0, 0), {})
    assert list(none.keys()) == ["distill_total", "base_total", "total"] and none["distill_total"] == 0


def test_lazy_dict_shares_one_copy_with_the_base_dict(surface):
    """A LazyLossDict base is materialised from the tail of the same host copy, under the base_ prefix."""
    from hiseg.kd import NOUT, LazyDistillationLossDict
    from hiseg.losses import LazyLossDict
    base_out = torch.arange(100, 117, dtype=torch.float32)
    base = LazyLossDict(base_out, [], {})
    vec = torch.cat([torch.arange(NOUT + 2, dtype=torch.float32), base_out])
    d = LazyDistillationLossDict(vec, (1, 1, 1), base)
    assert base._vals is None   # nothing read before the first access
    assert list(d.keys()) == surface["dict_keys"]["refined"]
    assert d["base_bg_fg_loss"] == 101.0 and d["base_dice_loss"] == 105.0 and base["bg_fg_loss"] == 101.0


def test_wrapper_train_eval_state_dict(surface):
    import hiseg
    teacher, student = _net(), _net()
    w = hiseg.DistillationModelWrapper(teacher, student)
    assert w.get_teacher() is teacher and w.get_student() is student
    assert not any(p.requires_grad for p in teacher.parameters())
    assert all(p.requires_grad for p in student.parameters())
    assert not teacher.training
    assert w.train() is w
    assert student.training and not teacher.training and not any(m.training for m in teacher.modules())
    w.train(False)
    assert not student.training and not teacher.training
    w.train()
    assert w.eval() is w
    assert not student.training and not teacher.training
    keys = list(w.state_dict().keys())
    assert keys and all(k.startswith(("teacher.", "student.")) for k in keys)
    assert {k.split(".")[0] for k in keys} == {k.split(".")[0] for k in surface["wrapper_state_keys"]}
    assert sorted(k[len("student."):] for k in keys if k.startswith("student.")) == sorted(student.state_dict())
    with pytest.raises(NotImplementedError):
        hiseg.DistillationModelWrapper(_net(), _net(), freeze_teacher=False)


def test_wrapper_forward_runs_both_models_teacher_without_grad():
    import hiseg
    w = hiseg.DistillationModelWrapper(_net(), _net()).train()
    x = torch.randn(2, 3, 4, 4)
    before = {k: v.clone() for k, v in w.teacher.state_dict().items()}
    s, t = w(x)
    assert s.requires_grad and not t.requires_grad
    with torch.no_grad():
        assert torch.equal(t, w.teacher(x))
    for k, v in w.teacher.state_dict().items():   # eval-mode BN: no running-statistics update
        assert torch.equal(v, before[k]), k


class _Unet(nn.Module):
    def __init__(self):
        super().__init__()
        self.model = nn.Conv2d(3, 1, 1)
        self.output_conv = nn.Conv2d(1, 2, 1)
        self.register_buffer("norm_mean", torch.zeros(3))


class _Teacher(nn.Module):
    def __init__(self, width=4):
        super().__init__()
        self.pretrained_unet = _Unet()
        self.feature_combiner = nn.Conv2d(width, 2, 1)
        self.head = nn.Linear(3, 3)


def _ck(path, sd):
    torch.save({"epoch": 7, "model_state_dict": sd, "best_miou": 0.5}, path)
    return str(path)


def test_load_teacher_checkpoint_remaps_old_format(tmp_path):
    import hiseg
    src = _Teacher()
    new = src.state_dict()
    old = {}
    for k, v in new.items():   # old format: no wrapper level between pretrained_unet and the network
        if k.startswith("pretrained_unet.model."):
            old["pretrained_unet." + k[len("pretrained_unet.model."):]] = v
        elif not k.startswith("pretrained_unet."):
            old[k] = v
    old["pretrained_unet.norm_mean"] = torch.ones(3)   # the marker of the old format
    old["gone.weight"] = torch.zeros(2)                # a key the model does not have
    dst = _Teacher()
    oc_before = dst.pretrained_unet.output_conv.weight.detach().clone()
    info = hiseg.load_teacher_checkpoint(_ck(tmp_path / "old.pth", old), dst)
    assert torch.equal(dst.pretrained_unet.model.weight, src.pretrained_unet.model.weight)
    assert torch.equal(dst.pretrained_unet.model.bias, src.pretrained_unet.model.bias)
    assert torch.equal(dst.head.weight, src.head.weight)
    assert "pretrained_unet.model.weight" in info["loaded"] and "gone.weight" not in info["loaded"]
    # the old key pretrained_unet.norm_mean became pretrained_unet.model.norm_mean, which the model does not have
    assert torch.equal(dst.pretrained_unet.norm_mean, torch.zeros(3))
    # output_conv was not in the checkpoint: (-u, +u), zero bias
    w = dst.pretrained_unet.output_conv.weight.detach()
    assert not torch.equal(w, oc_before)
    assert w.reshape(-1).tolist() == [-1.0, 1.0] and not dst.pretrained_unet.output_conv.bias.any()


def test_load_teacher_checkpoint_filters_shapes_and_keeps_output_conv(tmp_path):
    import hiseg
    src = _Teacher(width=6)   # feature_combiner of another width
    dst = _Teacher(width=4)
    fc_before = dst.feature_combiner.weight.detach().clone()
    sd = {k: v for k, v in src.state_dict().items() if k != "pretrained_unet.norm_mean"}   # new format
    info = hiseg.load_teacher_checkpoint(_ck(tmp_path / "new.pth", sd), dst)
    assert info["skipped"] == ["feature_combiner.weight"]
    assert torch.equal(dst.feature_combiner.weight, fc_before)
    assert torch.equal(dst.feature_combiner.bias, src.feature_combiner.bias)
    assert torch.equal(dst.head.weight, src.head.weight)
    # output_conv came with the checkpoint: loaded, not re-initialised
    assert torch.equal(dst.pretrained_unet.output_conv.weight, src.pretrained_unet.output_conv.weight)
    assert torch.equal(dst.pretrained_unet.output_conv.bias, src.pretrained_unet.output_conv.bias)
    assert "pretrained_unet.norm_mean" in info["missing"]
    # present in the checkpoint with another shape: dropped by the filter, and still not re-initialised (:498)
    dst2 = _Teacher()
    sd2 = dict(sd)
    sd2["pretrained_unet.output_conv.weight"] = torch.zeros(2, 1, 3, 3)
    oc = dst2.pretrained_unet.output_conv.weight.detach().clone()
    info2 = hiseg.load_teacher_checkpoint(_ck(tmp_path / "new2.pth", sd2), dst2)
    assert "pretrained_unet.output_conv.weight" in info2["skipped"]
    assert torch.equal(dst2.pretrained_unet.output_conv.weight, oc)


def test_save_checkpoint_of_wrapper_stores_the_student_only(tmp_path):
    import hiseg
    w = hiseg.DistillationModelWrapper(_net(4), _net(5))
    path = str(tmp_path / "ck.pth")
    hiseg.save_checkpoint(path, w, None, epoch=3)
    sd = torch.load(path, weights_only=True)["model_state_dict"]
    assert sd and not any(k.startswith(("teacher.", "student.")) for k in sd)
    assert sorted(sd) == sorted(w.get_student().state_dict())
    for k, v in w.get_student().state_dict().items():
        assert torch.equal(sd[k], v), k
    fresh = _net(5)
    fresh.load_state_dict(sd)   # strict: the file is a plain student checkpoint


def test_cpu_tensors_are_refused():
    import hiseg

    def base(pred, target, aux=None):
        return torch.tensor(0.5), {"total_loss": 0.5}
    loss = hiseg.DistillationLoss(base)
    s, t = torch.zeros(1, 3, 2, 2), torch.zeros(1, 3, 2, 2)
    with pytest.raises(RuntimeError, match="GPU"):
        loss(s, t, torch.zeros(1, 2, 2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="GPU"):
        loss((s, {"bg_fg_logits": torch.zeros(1, 2, 2, 2)}), (t, {"bg_fg_logits": torch.zeros(1, 2, 2, 2)}),
             torch.zeros(1, 2, 2, dtype=torch.int64))


def test_temperature_and_alpha_are_settable():
    import hiseg
    loss = hiseg.DistillationLoss(nn.Identity(), temperature=3.0, alpha=0.25)
    loss.temperature, loss.alpha = 1.5, 0.5
    assert (loss.temperature, loss.alpha) == (1.5, 0.5)
    with pytest.raises(ValueError):
        loss.temperature = 0.0


def test_create_distilled_model_checks_the_checkpoint_path(tmp_path):
    import hiseg
    with pytest.raises(ValueError):
        hiseg.create_distilled_rgb_hierarchical_model({}, "")
    with pytest.raises(FileNotFoundError):
        hiseg.create_distilled_rgb_hierarchical_model({}, str(tmp_path / "absent.pth"))


def test_kd_symbols_resolve_in_the_library():
    from hiseg import _lib as L
    lib = L.lib()
    for name in ("hiseg_kd_ws", "hiseg_kd_loss_fwd", "hiseg_kd_loss_bwd"):
        assert name in L.EXPORTED and getattr(lib, name) is not None
    assert lib.hiseg_kd_ws(2, 128, 96) == 2 * 12 * 3 + 1
    assert lib.hiseg_kd_ws(1, 1, 1) == 4 and lib.hiseg_kd_ws(0, 4, 4) == 0
    # argument checks need no device: a null student with a teacher, a non-positive temperature
    assert lib.hiseg_kd_loss_fwd(None, None, 8, None, None, None, 1, 2, 2, 1.0, None, 8, 8, None) != 0
    assert lib.hiseg_kd_loss_fwd(None, None, None, None, None, None, 1, 2, 2, 0.0, None, 8, 8, None) != 0
