"""ROI-model knowledge distillation on the GPU against the reference's recorded results (tests/golden/kd.npz,
gen_kd_golden.py; cases and seeded inputs in tests/kd_cases.py).

Bars.  Loss terms 1e-5 relative, gradients 1e-5 of the gradient's largest magnitude (the project's bars for loss
values and gradients, tests/test_gpu_distance.py); the case with the RefinedHierarchicalLoss base uses the bars
of tests/test_gpu_train.py::test_loss_kernel_matches_reference_golden (loss 1e-5, dict 1e-4, gradients 1e-4 of
the largest magnitude).  Raw C-ABI calls start from outputs, workspace and gradients filled with NaN, so a launch
that covers too little fails.  The recorded gradients are d total / d student with the stub base loss, i.e.
alpha * d distill_total / d student: the raw calls pass gscale = alpha."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import filler
from helpers import configs, hiseg_kwargs, load
from kd_cases import ALPHA, AUX, SHAPES, STUB, TEMPS, VARIANTS, call, grad_pixels, kd_inputs, kd_targets, tag, ttag

pytestmark = pytest.mark.gpu
DEV = "cuda"
TERM_KEYS = ("distill_logits", "distill_bg_fg", "distill_target")
NAN = float("nan")


@pytest.fixture(scope="module")
def G():
    return load("kd")


@functools.lru_cache(maxsize=None)
def inputs(shape):
    """Student and teacher tensors of a shape on the device (shared, never modified)."""
    s, t = kd_inputs(shape)
    return [torch.from_numpy(a).to(DEV) for a in s], [torch.from_numpy(a).to(DEV) for a in t]


def raw_kd(s, t, heads, T, dev_T=False, gscale=ALPHA):
    """hiseg_kd_loss_fwd / _bwd into NaN-filled buffers: (out[4], [grad or None] * 3)."""
    from hiseg import _lib as L
    lib = L.lib()
    N, _, H, W = s[0].shape
    ws = torch.full((int(lib.hiseg_kd_ws(N, H, W)),), NAN, dtype=torch.float32, device=DEV)
    out = torch.full((4,), NAN, dtype=torch.float32, device=DEV)
    d = [torch.full_like(s[h], NAN) if heads[h] else None for h in range(3)]
    g = torch.tensor([gscale], dtype=torch.float32, device=DEV)
    tdev = torch.tensor([T], dtype=torch.float32, device=DEV) if dev_T else None
    host_T = 0.0 if dev_T else float(T)
    p = lambda v: None if v is None else v.data_ptr()   # noqa: E731
    ptrs = [p(x[h]) if heads[h] else None for h in range(3) for x in (s, t)]
    L.check(lib.hiseg_kd_loss_fwd(*ptrs, N, H, W, host_T, p(tdev), ws.data_ptr(), out.data_ptr(), L.stream_ptr()),
            "kd_loss_fwd")
    L.check(lib.hiseg_kd_loss_bwd(*ptrs, N, H, W, host_T, p(tdev), g.data_ptr(), p(d[0]), p(d[1]), p(d[2]),
                                  L.stream_ptr()), "kd_loss_bwd")
    return out, d


def recorded(G, key):
    return dict(zip((str(k) for k in G[f"{key}_keys"]), (float(v) for v in G[f"{key}_vals"])))


def check_terms(out, want, heads, what):
    got = out.cpu().tolist()
    assert np.isfinite(got).all(), (what, got)
    print(what, "out", got, "want", [want.get(k) for k in ("distill_total",) + TERM_KEYS], flush=True)
    assert got[0] == pytest.approx(want["distill_total"], rel=1e-5), what
    for h, k in enumerate(TERM_KEYS):
        if heads[h]:
            assert got[1 + h] == pytest.approx(want[k], rel=1e-5), (what, k)
        else:
            assert got[1 + h] == 0.0 and k not in want, (what, k)


def check_grad(got, ref, what, bar=1e-5, pixels=None):
    """max |got - ref| <= bar * max |ref|; ``pixels``: ref holds these pixels of each plane only."""
    assert torch.isfinite(got).all(), what
    got = got.detach().cpu().double()
    ref = torch.from_numpy(np.asarray(ref)).double()
    if pixels is not None:
        got = got.reshape(got.shape[0], got.shape[1], -1)[:, :, torch.from_numpy(pixels)]
    ref = ref.reshape(got.shape)
    err, top = float((got - ref).abs().max()), float(ref.abs().max())
    print(what, "grad err %.3e of max %.3e (%.2e)" % (err, top, err / top if top else 0.0), flush=True)
    assert err <= bar * top, (what, err, top)


def composed_kd(s, t, heads, T):
    """The same term from torch ops on the device (what a user would write without the fused kernels)."""
    total = 0
    for h, w in enumerate((1.0, 0.3, 0.3)):
        if heads[h]:
            total = total + F.kl_div(F.log_softmax(s[h] / T, dim=1), F.softmax(t[h].detach() / T, dim=1),
                                     reduction="batchmean") * (T ** 2) * w
    return total


# ------------------------------------------------------------------------------------------ raw ABI
@pytest.mark.parametrize("shape", SHAPES, ids=tag)
def test_raw_abi_matches_fixture(G, shape):
    s, t = inputs(shape)
    hw = shape[1] * shape[2]
    big = shape == SHAPES[-1]
    for temp in TEMPS:
        for variant in VARIANTS if temp == TEMPS[0] else ("all",):
            key = f"{tag(shape)}_{variant}_{ttag(temp)}"
            heads = [bool(v) for v in G[f"{key}_heads"]]
            want = recorded(G, key)
            outs = []
            for dev_T in (False, True):
                out, d = raw_kd(s, t, heads, temp, dev_T=dev_T)
                check_terms(out, want, heads, (key, dev_T))
                for h in range(3):
                    gk = f"{tag(shape)}_{ttag(temp)}_grad{h}"
                    if heads[h] and gk in G.files:
                        check_grad(d[h], G[gk], (key, h, dev_T), pixels=grad_pixels(hw) if big else None)
                    elif heads[h]:
                        assert torch.isfinite(d[h]).all(), (key, h)
                outs.append((out, d))
            # T from the device scalar: the same bits as T from the host argument
            assert torch.equal(outs[0][0], outs[1][0]), key
            for a, b in zip(outs[0][1], outs[1][1]):
                assert (a is None and b is None) or torch.equal(a, b), key


def test_raw_abi_full_gradient_at_the_mask_size():
    """(2,128,96): the fixture holds a subset of the gradient's pixels; every pixel against the float64 term
    composed from torch ops (the reference's formula), same bar."""
    shape = SHAPES[-1]
    s, t = inputs(shape)
    for temp in (4.0, 0.5):
        s64 = [a.double().requires_grad_(True) for a in s]
        (ALPHA * composed_kd(s64, [a.double() for a in t], (1, 1, 1), temp)).backward()
        _, d = raw_kd(s, t, (1, 1, 1), temp)
        for h in range(3):
            check_grad(d[h], s64[h].grad.cpu().numpy(), ("full", temp, h))


def test_raw_abi_extreme_values(G):
    """q underflowing to exactly 0, +-80 student logits at T = 0.5, a pixel with student == teacher."""
    s = [torch.from_numpy(G[f"extreme_s{h}"]).to(DEV) for h in range(3)]
    t = [torch.from_numpy(G[f"extreme_t{h}"]).to(DEV) for h in range(3)]
    for temp in (0.5, 4.0):
        key = f"extreme_{ttag(temp)}"
        out, d = raw_kd(s, t, (1, 1, 1), temp)
        check_terms(out, recorded(G, key), (1, 1, 1), key)
        for h in range(3):
            check_grad(d[h], G[f"{key}_grad{h}"], (key, h))


def test_raw_abi_misaligned_base_takes_the_scalar_path():
    """H*W a multiple of 4 but a base pointer 4 bytes off a 16-byte boundary: the same values as aligned."""
    shape = (3, 12, 10)
    s, t = inputs(shape)
    want_out, want_d = raw_kd(s, t, (1, 1, 1), 4.0)

    def shifted(a):
        buf = torch.empty(a.numel() + 1, dtype=a.dtype, device=DEV)
        v = buf[1:].view(a.shape)
        v.copy_(a)
        assert v.data_ptr() % 16 == 4
        return v
    out, d = raw_kd([shifted(a) for a in s], [shifted(a) for a in t], (1, 1, 1), 4.0)
    assert out.cpu().tolist() == pytest.approx(want_out.cpu().tolist(), rel=1e-6)
    for a, b in zip(d, want_d):
        assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())


def test_raw_abi_is_deterministic():
    s, t = inputs(SHAPES[-1])
    a_out, a_d = raw_kd(s, t, (1, 1, 1), 4.0, dev_T=True)
    b_out, b_d = raw_kd(s, t, (1, 1, 1), 4.0, dev_T=True)
    assert torch.equal(a_out, b_out)
    for a, b in zip(a_d, b_d):
        assert torch.equal(a, b)


def test_raw_abi_rejects_bad_arguments():
    from hiseg import _lib as L
    lib = L.lib()
    s, t = inputs((2, 7, 5))
    out = torch.zeros(4, device=DEV)
    ws = torch.zeros(int(lib.hiseg_kd_ws(2, 7, 5)), device=DEV)
    p = lambda v: v.data_ptr()   # noqa: E731
    assert lib.hiseg_kd_loss_fwd(p(s[0]), p(t[0]), p(s[1]), None, None, None, 2, 7, 5, 4.0, None, p(ws), p(out),
                                 L.stream_ptr()) != 0
    assert lib.hiseg_kd_loss_fwd(p(s[0]), p(t[0]), None, None, None, None, 2, 7, 5, 0.0, None, p(ws), p(out),
                                 L.stream_ptr()) != 0
    assert lib.hiseg_kd_loss_bwd(p(s[0]), p(t[0]), None, None, None, None, 2, 7, 5, 4.0, None, p(out), None, None,
                                 None, L.stream_ptr()) != 0


# ------------------------------------------------------------------------------------------ module
class StubBase(nn.Module):
    """The fixture's base loss: a recorded constant and a plain dict."""

    def __init__(self):
        super().__init__()
        self.value = torch.tensor(STUB["total_loss"], device=DEV)
        self.calls = []

    def forward(self, pred, target, aux=None):
        self.calls.append(aux)
        return self.value, dict(STUB)


def run_module(variant, base, temp, shape, dtype=torch.float32):
    import hiseg
    s0, t0 = inputs(shape)
    s = [a.to(dtype).clone().requires_grad_(True) for a in s0]
    t = [a.to(dtype) for a in t0]
    loss_fn = hiseg.DistillationLoss(base, temperature=temp, alpha=ALPHA, distill_logits=(variant != "nologits"))
    target = torch.from_numpy(kd_targets(shape)).to(DEV)
    total, d, heads = call(variant, loss_fn, s, t, target)
    total.backward()
    return total, d, heads, s


@pytest.mark.parametrize("shape", SHAPES, ids=tag)
def test_module_matches_fixture(G, shape):
    hw = shape[1] * shape[2]
    big = shape == SHAPES[-1]
    for temp in TEMPS:
        for variant in VARIANTS if temp == TEMPS[0] else ("all",):
            key = f"{tag(shape)}_{variant}_{ttag(temp)}"
            base = StubBase()
            total, d, heads, s = run_module(variant, base, temp, shape)
            want = recorded(G, key)
            assert heads == [bool(v) for v in G[f"{key}_heads"]]
            assert list(d.keys()) == list(want.keys()), key
            for k, v in want.items():
                assert d[k] == pytest.approx(v, rel=1e-5), (key, k)
            assert float(total.detach()) == pytest.approx(want["total"], rel=1e-5), key
            # the base loss saw the student's aux whenever there was one
            assert len(base.calls) == 1 and base.calls[0] is not None
            for h in range(3):
                gk = f"{tag(shape)}_{ttag(temp)}_grad{h}"
                if not heads[h]:
                    assert s[h].grad is None, (key, h)
                elif gk in G.files:
                    check_grad(s[h].grad, G[gk], (key, h), pixels=grad_pixels(hw) if big else None)


@pytest.mark.parametrize("shape", [(2, 7, 5), (3, 12, 10)], ids=tag)
def test_module_with_refined_base_matches_fixture(G, shape):
    """RefinedHierarchicalLoss (fresh EMA state, first call) as the base: key prefixing, alpha mix, and the sum of
    the base and distillation gradients."""
    import hiseg
    assert list(shape) in G["refined_shapes"].tolist()
    key = f"{tag(shape)}_refined"
    total, d, heads, s = run_module("all", hiseg.RefinedHierarchicalLoss(), 4.0, shape)
    want = recorded(G, key)
    assert list(d.keys()) == list(want.keys())
    assert float(total.detach()) == pytest.approx(want["total"], rel=1e-5, abs=1e-6)
    for k, v in want.items():
        print(key, k, d[k], v, flush=True)
        assert d[k] == pytest.approx(v, rel=1e-4, abs=1e-6), k
    for h in range(3):
        ref = G[f"{key}_grad{h}"]
        got = s[h].grad.cpu()
        assert float((got - torch.from_numpy(ref)).abs().max()) <= 1e-7 + 1e-4 * float(np.abs(ref).max()), h


def test_module_dict_is_lazy_and_shares_the_base_copy():
    import hiseg
    from hiseg.losses import LazyLossDict
    _, d, _, _ = run_module("all", hiseg.RefinedHierarchicalLoss(), 4.0, (3, 12, 10))
    assert isinstance(d._base, LazyLossDict) and d._base._vals is None and d._vals is None
    assert d["base_total_loss"] == d._base["total_loss"] and d._base._vals is not None
    assert d["total"] == pytest.approx(ALPHA * d["distill_total"] + (1 - ALPHA) * d["base_total"], rel=1e-6)


def test_module_without_any_term():
    """distill_logits=False and no teacher aux: distill_total is 0 and the total is (1 - alpha) * base."""
    import hiseg
    s, t = inputs((2, 7, 5))
    loss_fn = hiseg.DistillationLoss(StubBase(), temperature=4.0, alpha=ALPHA, distill_logits=False)
    total, d = loss_fn((s[0], dict(zip(AUX, s[1:]))), t[0], None)
    assert list(d.keys()) == ["base_" + k for k in STUB] + ["distill_total", "base_total", "total"]
    assert d["distill_total"] == 0
    assert float(total) == pytest.approx((1 - ALPHA) * STUB["total_loss"], rel=1e-6) and d["total"] == float(total)


def test_module_rejects_shape_mismatch_and_casts_bf16(G):
    import hiseg
    s, t = inputs((2, 7, 5))
    loss_fn = hiseg.DistillationLoss(StubBase())
    with pytest.raises(ValueError):
        loss_fn(s[0], t[0][:1], None)
    with pytest.raises(ValueError):
        loss_fn((s[0], {AUX[0]: s[1]}), (t[0], {AUX[0]: t[1][:, :, :3]}), None)
    with pytest.raises(ValueError):   # an aux head at another size than the logits
        loss_fn((s[0], {AUX[0]: s[1][:, :, :3]}), (t[0], {AUX[0]: t[1][:, :, :3]}), None)
    # bf16 inputs are cast to f32: the result is the f32 loss of the rounded inputs
    total, d, _, sb = run_module("all", StubBase(), 4.0, (2, 7, 5), dtype=torch.bfloat16)
    out, _ = raw_kd([a.detach().float() for a in sb], [a.bfloat16().float() for a in t], (1, 1, 1), 4.0)
    assert d["distill_total"] == float(out[0]) and sb[0].grad.dtype == torch.bfloat16


def test_loss_captured_in_a_graph_follows_temperature_and_alpha():
    """Forward and backward on fixed buffers in one torch.cuda.graph (a single stream), replayed after an in-place
    change of temperature and alpha: the eager results at the new values."""
    import hiseg
    shape = (3, 33, 29)
    s0, t = inputs(shape)
    s = [a.clone().requires_grad_(True) for a in s0]
    loss_fn = hiseg.DistillationLoss(StubBase(), temperature=4.0, alpha=0.7)

    def step():
        total, d = loss_fn((s[0], dict(zip(AUX, s[1:]))), (t[0], dict(zip(AUX, t[1:]))), None)
        return (total.detach(), d._vec) + torch.autograd.grad(total, s)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()   # eager first call: creates the device scalars
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    graph.replay()
    torch.cuda.synchronize()
    first = [v.clone() for v in static]
    for v, e in zip(first, step()):
        assert torch.equal(v, e)
    loss_fn.temperature, loss_fn.alpha = 1.0, 0.4
    graph.replay()
    torch.cuda.synchronize()
    fresh = hiseg.DistillationLoss(StubBase(), temperature=1.0, alpha=0.4)
    total, d = fresh((s[0], dict(zip(AUX, s[1:]))), (t[0], dict(zip(AUX, t[1:]))), None)
    want = (total.detach(), d._vec) + torch.autograd.grad(total, s)
    for v, e, old in zip(static, want, first):
        assert torch.equal(v, e) and not torch.equal(v, old)


# ------------------------------------------------------------------------------------------ wrapped step
def _model(seed, encoder=None):
    import hiseg
    kw = hiseg_kwargs(dict(configs()["b0"]["model_kwargs"]))
    if encoder is not None:
        kw.update(encoder_name=encoder, freeze_pretrained_weights=False)
    m = filler.fill_module(hiseg.create_rgb_hierarchical_model(**kw), seed=seed)
    for mod in m.modules():
        if isinstance(mod, (nn.Dropout, nn.Dropout2d)):
            mod.p = 0.0
    for mm in (m.roi_align_mask, m.roi_align_rgb):
        mm.spatial_scale_h, mm.spatial_scale_w = 96, 128
    return hiseg.set_compute_dtype(m, torch.float32)


@pytest.fixture(scope="module")
def wrapped():
    """One B0 student (train) + B1 teacher (frozen) at the size of test_train_step_f32_matches_oracle: a step with
    the fused loss, the same step with the KD term composed from torch ops (both with the teacher on the side stream, the
    default), a forward with the teacher on the caller's stream, the teacher alone, then one optimiser step."""
    import hiseg
    images = torch.from_numpy(filler.uniform(61, (2, 3, 96, 128))).to(DEV)
    rois = torch.tensor([[0, .10, .10, .40, .90], [1, .35, .15, .80, .95], [0, .55, .05, .95, .70]]).to(DEV)
    tgt = torch.from_numpy(filler.ellipse_targets(63, 3, 128, 96)).to(DEV)
    w = hiseg.DistillationModelWrapper(_model(5, "timm-efficientnet-b1"), _model(0)).to(DEV).train()
    assert w.overlap_teacher is True   # the measured default: the teacher on the side stream
    teacher_before = {k: v.detach().clone() for k, v in w.teacher.state_dict().items()}
    T, alpha = 4.0, 0.7
    res = {"w": w, "teacher_before": teacher_before}
    opt = None
    for mode in ("fused", "composed"):
        base = hiseg.RefinedHierarchicalLoss(use_boundary_aware_loss=True, use_contour_detection=True,
                                             use_distance_transform=True, boundary_aware_weight=0.1,
                                             contour_loss_weight=0.1, distance_loss_weight=0.1)
        (sl, sa), (tl, ta) = w(images, rois)
        heads = [sl, sa[AUX[0]], sa[AUX[1]]]
        for h in heads:
            h.retain_grad()
        if mode == "fused":
            total, d = hiseg.DistillationLoss(base, temperature=T, alpha=alpha)((sl, sa), (tl, ta), tgt)
            res["dict"] = d
        else:
            base_loss, _ = base(sl, tgt, sa)
            total = alpha * composed_kd(heads, [tl, ta[AUX[0]], ta[AUX[1]]], (1, 1, 1), T) + (1 - alpha) * base_loss
        if opt is None:
            opt = hiseg.FusedAdamW(w.student, lr=1e-4)
        opt.zero_grad()
        total.backward()
        res[mode] = {"total": total.detach().clone(), "teacher": (tl, ta),
                     "student": (sl.detach().clone(), {k: v.detach().clone() for k, v in sa.items()}), "grads": [h.grad.detach().clone() for h in heads],
                     "param_grads": {n: p.grad.detach().clone() for n, p in w.student.named_parameters()
                                     if p.grad is not None}}
    w.overlap_teacher = False
    (sl, sa), (tl, ta) = w(images, rois)
    w.overlap_teacher = True
    res["serial"] = {"student": (sl.detach(), {k: v.detach() for k, v in sa.items()}), "teacher": (tl, ta)}
    with torch.no_grad():
        res["teacher_alone"] = w.teacher(images, rois)
    res["teacher_grads"] = [n for n, p in w.teacher.named_parameters() if p.grad is not None or p.requires_grad]
    opt.step()
    torch.cuda.synchronize()
    return res


def _same(a, b):
    (al, aa), (bl, ba) = a, b
    assert torch.equal(al, bl)
    assert list(aa.keys()) == list(ba.keys())
    for k in aa:
        assert torch.equal(aa[k], ba[k]), k


def test_wrapped_step_teacher_outputs(wrapped):
    tl, ta = wrapped["fused"]["teacher"]
    assert not tl.requires_grad and not any(v.requires_grad for v in ta.values())
    assert {AUX[0], AUX[1]} <= set(ta.keys())
    _same(wrapped["fused"]["teacher"], wrapped["teacher_alone"])
    _same(wrapped["composed"]["teacher"], wrapped["teacher_alone"])


def test_wrapped_step_output_gradients_equal_composed(wrapped):
    a, b = wrapped["fused"], wrapped["composed"]
    assert float(a["total"]) == pytest.approx(float(b["total"]), rel=1e-5)
    assert wrapped["dict"]["total"] == pytest.approx(float(a["total"]), rel=1e-6)
    for h, (ga, gb) in enumerate(zip(a["grads"], b["grads"])):
        check_grad(ga, gb.cpu().numpy(), ("wrapped", h))


def test_wrapped_step_parameter_gradients(wrapped):
    a, b = wrapped["fused"]["param_grads"], wrapped["composed"]["param_grads"]
    assert a and set(a) == set(b)
    for n in a:
        assert torch.isfinite(a[n]).all() and torch.isfinite(b[n]).all(), n
    assert any(g.any() for g in a.values())
    assert wrapped["teacher_grads"] == []


def test_wrapped_step_leaves_the_teacher_unchanged(wrapped):
    after = wrapped["w"].teacher.state_dict()
    assert list(after.keys()) == list(wrapped["teacher_before"].keys())
    for k, v in wrapped["teacher_before"].items():
        assert torch.equal(after[k], v), k
    assert not wrapped["w"].teacher.training and wrapped["w"].student.training


def test_wrapped_step_teacher_overlap_is_bit_identical(wrapped):
    """The steps above ran with overlap_teacher=True; the same forward with the teacher on the caller's stream."""
    _same(wrapped["serial"]["teacher"], wrapped["fused"]["teacher"])
    _same(wrapped["serial"]["student"], wrapped["fused"]["student"])
