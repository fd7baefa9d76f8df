"""The EfficientNet stem reading the raw f32 NCHW images (conv_small_kernel's raw staging form,
hiseg_conv2d_desc.raw_src) against the two launches it replaces (hiseg_input_norm_fwd, then the stem conv), bit for bit,
and against float64.

* Bit equality: the raw form stages the halo with input_norm's arithmetic -- v / 255 when the batch maximum is above 1,
  (v - mean) / std, each operation rounded on its own, round-to-nearest-even to bf16, channels 3..7 and every pixel
  outside the image zero -- and everything after the staging is the same code, so `engine.effunet_stem` with
  `engine.STEM_RAW` on and off must store the same bits.  B0 stem weights from the filler.  Shapes (N x 3 x H x W;
  the kernel's tile is 8 output rows x 64 output columns): 2x3x64x96 has Wo 48, less than one tile across, and four
  row tiles; 1x3x32x288 has Wo 144, two full tiles and a partial one; 2x3x96x32 has Ho 48, six row tiles of one
  16-column tile.  Every tile touches an image border, where the halo is zero, not (0 - mean) / std.
* Value classes: U[0, 1) (flag off); U[0, 255) (flag on); U[0, 1) with one value set to exactly 1.0 (flag off: the
  test is `> 1`); N(0, 1) with negative values (flag off) and N(0, 1) * 40 (negative values, flag on); a batch whose
  base address is a 4-byte-offset view of a larger buffer (the form loads plane values one f32 at a time, so it
  takes it).
* Every case asserts the recorded path: ("stem_raw", 1) and one conv launch with the form on, the "small" family
  and one conv launch with it off.
* Float64: the stem on the CPU in float64 over the bf16-rounded normalised images (torch's float32 division and
  subtraction are correctly rounded, as the kernel's are), at 1x3x32x288 with the flag on.  The bar is the one
  tests/test_gpu_conv_kernels.py (check_b) holds every bf16 kernel with a SiLU epilogue to
  (profiles/conv_kernel_errors.txt):
      |k - ref| <= 4 max(e32) + 4 * 2^-23 max|ref| + 2^-8 |ref| + |pre| dsig(pre)
  with e32 the float32 evaluation of the same reference minus the float64 one, pre the value before the activation
  and dsig the sigmoid intrinsic's bound of tests/test_gpu_infer_kernels.py.
* The query refuses f32 compute, C = 4, a non-contiguous batch and a stem that is not 3x3 stride 2; unet_input then
  runs input_norm and the stem takes the old path.
* Whole UNet: engine.unet_logit with the form on == bypassed.
"""
import pytest
import torch
import torch.nn.functional as F

import filler

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = torch.bfloat16
SHAPES = [(2, 3, 64, 96), (1, 3, 32, 288), (2, 3, 96, 32)]


@pytest.fixture(scope="module")
def pre():
    import hiseg
    m = hiseg.PreTrainedPeopleSegmentationUNet(pretrained_weights_path="ext_extractor/best_model_b0_0.8741.pth",
                                               freeze_weights=True, encoder_name="timm-efficientnet-b0")
    return filler.fill_module(m, 7).eval().to(DEV)


def _images(kind, shape, seed=31):
    if kind == "unit":
        x = torch.from_numpy(filler.uniform(seed, shape))
    elif kind == "bytes":
        x = torch.from_numpy(filler.uniform(seed, shape, 0.0, 255.0))
    elif kind == "max_is_one":
        x = torch.from_numpy(filler.uniform(seed, shape))
        x.view(-1)[x.numel() // 3] = 1.0
        assert x.max().item() == 1.0
    elif kind == "negative":
        x = torch.from_numpy(filler.normal(seed, shape)).clamp_(max=1.0)
        assert x.min().item() < -1 and x.max().item() <= 1.0
    elif kind == "negative_wide":
        x = torch.from_numpy(filler.normal(seed, shape)) * 40
    elif kind == "offset4":
        big = torch.zeros(x_numel(shape) + 8, device=DEV)
        x = big[1:1 + x_numel(shape)].view(shape)
        x.copy_(torch.from_numpy(filler.uniform(seed, shape, 0.0, 255.0)))
        assert x.data_ptr() % 16 == 4 and x.is_contiguous()
        return x
    else:
        raise KeyError(kind)
    return x.to(DEV)


def x_numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def _stem(monkeypatch, pre, images, raw, dt=DT):
    """engine.unet_input + engine.effunet_stem with the raw form on / bypassed:
    (output Act, last path, launches per family)."""
    from hiseg import _lib as L, engine
    monkeypatch.setattr(engine, "STEM_RAW", raw)
    E = engine.Ctx(pre, dt, torch.device(DEV))
    L.conv_path_stats(reset=True)
    y = engine.effunet_stem(E, pre.model.encoder, engine.unet_input(E, pre, images))
    torch.cuda.synchronize()
    return y, L.conv_last_path(), L.conv_path_stats(reset=True)


def _same(got, ref):
    assert (got.N, got.H, got.W, got.C, got.cstride, got.coff) == (ref.N, ref.H, ref.W, ref.C, ref.cstride, ref.coff)
    assert torch.isfinite(got.t.float()).all()
    assert torch.equal(got.t, ref.t)


# ---------------------------------------------------------------------------------- bit equality
@pytest.mark.parametrize("kind", ["unit", "bytes", "max_is_one", "negative", "negative_wide", "offset4"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_raw_stem_equals_input_norm_then_stem(monkeypatch, pre, shape, kind):
    images = _images(kind, shape)
    ref, path2, stats2 = _stem(monkeypatch, pre, images, False)
    got, path1, stats1 = _stem(monkeypatch, pre, images, True)
    assert path2[0] == "small" and stats2["stem_raw"] == 0 and sum(stats2.values()) == 1, (path2, stats2)
    assert path1 == ("stem_raw", 1) and stats1["stem_raw"] == 1 and sum(stats1.values()) == 1, (path1, stats1)
    assert (ref.N, ref.H, ref.W, ref.C) == (shape[0], shape[2] // 2, shape[3] // 2, 32)
    _same(got, ref)
    assert got.t.float().abs().max().item() > 0


def test_flag_follows_the_maximum(monkeypatch, pre):
    """The same values with and without one element above 1: the outputs differ (the /255 really switches), and each
    equals the two-launch result."""
    shape = SHAPES[0]
    lo = _images("unit", shape)
    hi = lo.clone()
    hi.view(-1)[5] = 1.0 + 2.0 ** -23
    outs = []
    for images in (lo, hi):
        ref, _, _ = _stem(monkeypatch, pre, images, False)
        got, path, _ = _stem(monkeypatch, pre, images, True)
        assert path == ("stem_raw", 1)
        _same(got, ref)
        outs.append(got.t)
    assert not torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------------------------- float64
def _dexp(x):
    return 1.25 * 2.0 ** -24 * x.abs() + 2.0 ** -23


def _dsig(x):
    assert x.abs().max() <= 16
    s = torch.sigmoid(x)
    return s * (1 - s) * _dexp(x) + 1.5 * 2.0 ** -23 * s


def test_raw_stem_meets_the_conv_bar_against_float64(monkeypatch, pre):
    from hiseg import engine
    shape = SHAPES[1]
    images = _images("bytes", shape)
    got, path, _ = _stem(monkeypatch, pre, images, True)
    assert path == ("stem_raw", 1)
    k = got.t.view(got.N, got.H, got.W, got.cstride)[..., :got.C].permute(0, 3, 1, 2).float().cpu().double()

    enc = pre.model.encoder
    plan = engine.Ctx(pre, DT, torch.device(DEV)).conv(enc.conv_stem, enc.bn1, engine.ACT_SILU)
    x = images.cpu()
    assert x.max().item() > 1.0
    x = x / 255.0
    x = ((x - pre.norm_mean.cpu().view(1, 3, 1, 1)) / pre.norm_std.cpu().view(1, 3, 1, 1)).to(DT)   # f32 ops, then bf16
    w = enc.conv_stem.weight.detach().cpu().to(DT)
    sc, sh = plan.scale[:32].cpu(), plan.shift[:32].cpu()

    def run(dt):
        pre_act = F.conv2d(x.to(dt), w.to(dt), None, stride=2, padding=1) * sc.to(dt).view(1, -1, 1, 1) + \
            sh.to(dt).view(1, -1, 1, 1)
        return pre_act, pre_act * torch.sigmoid(pre_act)

    pre64, ref = run(torch.float64)
    _, r32 = run(torch.float32)
    e32 = (r32.double() - ref).abs().max()
    bound = 4 * e32 + 4 * 2.0 ** -23 * ref.abs().max() + 2.0 ** -8 * ref.abs() + pre64.abs() * _dsig(pre64)
    err = (k - ref).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"stem_raw bf16 {shape}: max err {err.max().item():.3e} ratio {ratio:.3f}")
    assert ratio <= 1.0, f"error / bound = {ratio:.3f} (max err {err.max().item():.3e})"


# ---------------------------------------------------------------------------------- the query and the fall-back
def test_query_refusals(pre):
    from hiseg import engine, ops
    E = engine.Ctx(pre, DT, torch.device(DEV))
    enc = pre.model.encoder
    plan = E.conv(enc.conv_stem, enc.bn1, engine.ACT_SILU)
    x = _images("unit", SHAPES[0])
    assert ops.stem_raw_ok(plan, x, DT)
    assert not ops.stem_raw_ok(plan, x, torch.float32)                                   # f32 compute
    assert not ops.stem_raw_ok(plan, torch.zeros(2, 4, 64, 96, device=DEV), DT)          # C = 4
    assert not ops.stem_raw_ok(plan, x.transpose(2, 3), DT)                              # not contiguous
    assert not ops.stem_raw_ok(plan, x.double(), DT)                                     # not f32
    assert not ops.stem_raw_ok(plan, x.cpu(), DT)
    s1 = torch.nn.Conv2d(3, 32, 3, stride=1, padding=1, bias=False).to(DEV)              # 3x3 stride 1
    assert not ops.stem_raw_ok(E.conv(s1, None, engine.ACT_SILU), x, DT)
    k5 = torch.nn.Conv2d(3, 32, 5, stride=2, padding=2, bias=False).to(DEV)              # 5x5 stride 2
    assert not ops.stem_raw_ok(E.conv(k5, None, engine.ACT_SILU), x, DT)
    # the library's own answer (no launch): yes for this layer; no once the operands reach 2 GiB, for another
    # stride, with a second fused operand, or without the tables
    import ctypes
    from hiseg import _lib as L

    def ask(**fields):
        d = ops._stem_raw_desc(plan, x, plan.scale, plan.scale, plan.scale, None)
        for name, v in fields.items():
            setattr(d, name, v)
        return L.lib().hiseg_conv2d_fused_ok(ctypes.byref(d))

    assert ask() == 1
    assert ask(N=96, H=2368, W=2368, Ho=1184, Wo=1184) == 0
    assert ask(stride=1) == 0
    assert ask(Ca=16, a_cstride=16) == 0
    assert ask(in_scale=plan.scale) == 0
    assert ask(a_gate=plan.scale) == 0
    assert ask(raw_max=None) == 0


def test_refused_inputs_take_the_old_path(monkeypatch, pre):
    """A non-contiguous batch and f32 compute with STEM_RAW on: input_norm + the stem conv run as before (the same
    bits as with the form bypassed), and the raw path is not recorded."""
    base = _images("bytes", (2, 3, 96, 64))
    view = base.transpose(2, 3)   # [2, 3, 64, 96], not contiguous
    ref, _, _ = _stem(monkeypatch, pre, view.contiguous(), False)
    got, path, stats = _stem(monkeypatch, pre, view, True)
    assert path[0] == "small" and stats["stem_raw"] == 0 and sum(stats.values()) == 1, (path, stats)
    _same(got, ref)
    ref32, _, _ = _stem(monkeypatch, pre, base, False, dt=torch.float32)
    got32, path32, stats32 = _stem(monkeypatch, pre, base, True, dt=torch.float32)
    assert path32[0] != "stem_raw" and stats32["stem_raw"] == 0, (path32, stats32)
    _same(got32, ref32)


# ---------------------------------------------------------------------------------- whole UNet
def test_unet_logit_is_unchanged(monkeypatch, pre):
    from hiseg import _lib as L, engine
    images = _images("bytes", (2, 3, 64, 96))
    outs = []
    for raw in (False, True):
        monkeypatch.setattr(engine, "STEM_RAW", raw)
        L.conv_path_stats(reset=True)
        u = engine.unet_logit(engine.Ctx(pre, DT, torch.device(DEV)), pre, images)
        torch.cuda.synchronize()
        assert L.conv_path_stats(reset=True)["stem_raw"] == int(raw)
        outs.append(u)
    assert outs[0].shape == (2, 1, 64, 96) and torch.isfinite(outs[1]).all()
    assert torch.equal(outs[0], outs[1])
