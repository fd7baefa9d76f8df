"""The 64-channel ResidualBlock as one launch (conv_resblock.hip, hiseg_resblock_fwd) against the two launches it
replaces (conv1, then conv2 with the residual), bit for bit, and against float64.

* Bit equality: the fused kernel keeps conv_hwc's accumulation order and epilogue arithmetic and holds the intermediate
  as the bf16 tensor conv1 stores, so `engine.residual_block` with `engine.RESBLOCK_FUSED` on and off must store the
  same bits.  Shapes (N x H x W, C = 64): 3x16x16 is exactly one 16 x 16 tile with all four image borders inside it;
  2x32x48 has tile seams both ways (the recomputed ring crosses them); 2x12x20 is smaller than a tile one way and
  ragged the other; 1x40x24 is ragged both ways; 2x48x64 is the head's own grid.  Both activation forms of
  hiseg.layers.ResidualBlock (activation1 / activation2, and the EnhancedUNet's single activation).
* Border: the intermediate outside the image is conv2's zero padding, not conv1 evaluated there (which is
  act1(shift1) != 0).  One case makes the input large along the image border that falls inside a tile.
* Float64: the block on the CPU in float64 with the intermediate rounded to bf16, at 2x32x48.  The bar is the one
  tests/test_gpu_conv_kernels.py (check_b) holds every bf16 3x3 kernel to:
      |k - ref| <= 4 max(e32) + 4 * 2^-23 max|ref| + 2^-8 |ref|
  with e32 the float32 evaluation of the same reference minus the float64 one.  test_two_launch_arithmetic_meets_the_bar
  first checks on the CPU that the two-launch arithmetic emulated in float32 (tap by tap in the kernels' order, bf16
  intermediate) meets that bar.
* Dispatch: an eligible block reports the path ("resblock", 1); C = 128, f32, LayerNorm2d, `head2` and `out=` run as
  two launches on the old paths.
* Whole model: engine.rgb_model_forward on the golden b0 configuration, fusion on == fusion bypassed.
"""
import pytest
import torch
import torch.nn.functional as F

import filler
from helpers import b0_kwargs, hiseg_kwargs, load

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = torch.bfloat16
SHAPES = [(3, 16, 16), (2, 32, 48), (2, 12, 20), (1, 40, 24), (2, 48, 64)]


def _block(c=64, norm="batchnorm", two_acts=True, seed=0):
    from hiseg.layers import ResidualBlock
    return filler.fill_module(ResidualBlock(c, norm, 8, "relu", 1.0, two_acts=two_acts), seed).eval().to(DEV)


def _x(shape, seed, c=64, dt=DT):
    from hiseg import ops
    N, H, W = shape
    return ops.Act.from_nchw(torch.from_numpy(filler.normal(seed, (N, c, H, W))).to(DEV), dt)


def _run(monkeypatch, blk, x, fused, **kw):
    """engine.residual_block with the fusion on / bypassed: (output Act or None, last path, launches per family)."""
    from hiseg import _lib as L, engine
    monkeypatch.setattr(engine, "RESBLOCK_FUSED", fused)
    L.conv_path_stats(reset=True)
    y = engine.residual_block(engine.Ctx(blk, x.dtype, x.t.device), blk, x, **kw)
    torch.cuda.synchronize()
    return y, L.conv_last_path(), L.conv_path_stats(reset=True)


# ---------------------------------------------------------------------------------- bit equality
@pytest.mark.parametrize("two_acts", [True, False], ids=["two_acts", "unet_act"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_block_equals_two_launches(monkeypatch, shape, two_acts):
    blk = _block(two_acts=two_acts, seed=3)
    x = _x(shape, 71)
    ref, path2, stats2 = _run(monkeypatch, blk, x, False)
    got, path1, stats1 = _run(monkeypatch, blk, x, True)
    assert path2[0] != "resblock" and stats2["resblock"] == 0 and sum(stats2.values()) == 2, (path2, stats2)
    assert path1 == ("resblock", 1) and stats1["resblock"] == 1 and sum(stats1.values()) == 1, (path1, stats1)
    assert torch.isfinite(got.t.float()).all()
    assert (got.N, got.H, got.W, got.C, got.cstride, got.coff) == (ref.N, ref.H, ref.W, ref.C, ref.cstride, ref.coff)
    assert torch.equal(got.t, ref.t)
    assert not torch.equal(got.t, x.t)


def test_intermediate_outside_the_image_is_zero(monkeypatch):
    """2x12x20: the bottom border (row 12) lies inside the first tile row and the right border (column 20) inside the
    second tile column.  The input is large along those borders and BatchNorm 1's shift is large and positive, so
    conv1 evaluated one pixel outside the image would be far from the zero conv2 must read there."""
    blk = _block(seed=5)
    with torch.no_grad():
        blk.norm1.bias.add_(4.0)
    x = _x((2, 12, 20), 72)
    v = x.t.view(2, 12, 20, 64)
    v[:, -2:] *= 32
    v[:, :, -2:] *= 32
    v[:, :2] *= 32
    v[:, :, :2] *= 32
    ref, _, _ = _run(monkeypatch, blk, x, False)
    got, path, _ = _run(monkeypatch, blk, x, True)
    assert path == ("resblock", 1)
    assert torch.isfinite(got.t.float()).all()
    assert torch.equal(got.t, ref.t)


# ---------------------------------------------------------------------------------- float64
def _plans(blk):
    from hiseg import engine
    E = engine.Ctx(blk, DT, torch.device(DEV))
    a1, a2 = engine._block_acts(blk)
    return E.conv(blk.conv1, blk.norm1, a1), E.conv(blk.conv2, blk.norm2, a2)


def _cpu_block(x, plans, dt, tapwise=False):
    """The block on the CPU in `dt` from the packed plans (bf16 weights, f32 scale / shift), the intermediate rounded
    to bf16.  tapwise: each conv as 2 slices x 9 taps accumulated in the kernels' order (slices; kx-major, ky inner)."""
    def conv(v, p):
        w = p.weight.float().cpu().view(64, 3, 3, 64).permute(0, 3, 1, 2).to(dt)
        if not tapwise:
            z = F.conv2d(v, w, padding=1)
        else:
            vp = F.pad(v, (1, 1, 1, 1))
            H, W = v.shape[2:]
            z = torch.zeros(v.shape[0], 64, H, W, dtype=dt)
            for sl in range(2):
                for kx in range(3):
                    for ky in range(3):
                        z = z + torch.einsum("oc,nchw->nohw", w[:, 32 * sl:32 * sl + 32, ky, kx],
                                             vp[:, 32 * sl:32 * sl + 32, ky:ky + H, kx:kx + W])
        return z * p.scale.cpu().to(dt).view(1, -1, 1, 1) + p.shift.cpu().to(dt).view(1, -1, 1, 1)
    p1, p2 = plans
    h = torch.relu(conv(x.to(dt), p1)).to(torch.bfloat16).to(dt)
    return torch.relu(conv(h, p2) + x.to(dt))


@pytest.fixture(scope="module")
def f64_case():
    blk = _block(seed=7)
    x = _x((2, 32, 48), 73)
    plans = _plans(blk)
    xc = x.to_nchw().float().cpu()   # (bf16 values)
    r64 = _cpu_block(xc, plans, torch.float64)
    r32 = _cpu_block(xc, plans, torch.float32)
    e32 = (r32.double() - r64).abs().max()
    bound = 4 * e32 + 4 * 2.0 ** -23 * r64.abs().max() + 2.0 ** -8 * r64.abs()
    return blk, x, plans, xc, r64, bound


def _ratio(k, r64, bound):
    err = (k.double() - r64).abs()
    return torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300)).max().item(), err.max().item()


def test_two_launch_arithmetic_meets_the_bar(f64_case):
    _, _, plans, xc, r64, bound = f64_case
    emu = _cpu_block(xc, plans, torch.float32, tapwise=True).to(torch.bfloat16)
    ratio, err = _ratio(emu, r64, bound)
    print(f"two-launch arithmetic in float32 on the CPU: max err {err:.3e} ratio {ratio:.3f}")
    assert ratio <= 1.0


def test_fused_block_against_float64(monkeypatch, f64_case):
    blk, x, _, _, r64, bound = f64_case
    got, path, _ = _run(monkeypatch, blk, x, True)
    assert path == ("resblock", 1)
    ratio, err = _ratio(got.to_nchw().cpu(), r64, bound)
    print(f"fused block against float64: max err {err:.3e} ratio {ratio:.3f}")
    assert ratio <= 1.0


# ---------------------------------------------------------------------------------- fallback
def test_ineligible_blocks_run_as_two_launches(monkeypatch):
    from hiseg import ops
    shape = (2, 20, 24)

    def two_launches(blk, x, **kw):
        y, path, stats = _run(monkeypatch, blk, x, True, **kw)
        assert stats["resblock"] == 0 and path[0] != "resblock", (path, stats)
        ref, _, _ = _run(monkeypatch, blk, x, False, **kw)
        return y, ref, stats

    # 128 channels
    y, ref, stats = two_launches(_block(128, seed=9), _x(shape, 74, c=128))
    assert sum(stats.values()) == 2 and torch.equal(y.t, ref.t) and torch.isfinite(y.t.float()).all()
    # f32
    y, ref, stats = two_launches(_block(seed=9), _x(shape, 75, dt=torch.float32))
    assert sum(stats.values()) == 2 and torch.equal(y.t, ref.t) and torch.isfinite(y.t).all()
    # LayerNorm2d (per-sample statistics: no folded affine)
    y, ref, stats = two_launches(_block(norm="layernorm2d", seed=9), _x(shape, 76))
    assert sum(stats.values()) == 2 and torch.equal(y.t, ref.t) and torch.isfinite(y.t.float()).all()
    # head2 given (a 64-channel layer has no head2 epilogue: conv2 stores its output as usual)
    blk, x = _block(seed=9), _x(shape, 77)
    h2 = ops.Head2(torch.randn(2, 64, device=DEV) * 0.1, torch.zeros(2, device=DEV))
    y, ref, stats = two_launches(blk, x, head2=h2)
    assert sum(stats.values()) == 2 and y is not None and h2.out is None and torch.equal(y.t, ref.t)
    # out= given: a 64-channel slice of a wider tensor
    wide = ops.Act.new(shape[0], shape[1], shape[2], 128, DT, DEV, zero=True)
    wide2 = ops.Act.new(shape[0], shape[1], shape[2], 128, DT, DEV, zero=True)
    _, path, stats = _run(monkeypatch, blk, x, True, out=wide.slice(64, 64))
    assert stats["resblock"] == 0 and sum(stats.values()) == 2 and path[0] != "resblock"
    _run(monkeypatch, blk, x, False, out=wide2.slice(64, 64))
    plain, _, _ = _run(monkeypatch, blk, x, True)
    assert torch.equal(wide.t, wide2.t)
    assert torch.equal(wide.t.view(-1, 128)[:, 64:].reshape(-1), plain.t)
    assert not wide.t.view(-1, 128)[:, :64].any()


def test_query_refuses_what_the_kernel_does_not_handle():
    import ctypes
    from hiseg import _lib as L, ops
    p1, p2 = _plans(_block(seed=9))
    x = _x((2, 20, 24), 78)
    out = ops.Act.new(2, 20, 24, 64, DT, DEV)

    def ok(x=x, out=out, res=None, edit=None):
        d1 = ops._conv_desc(p1, x, None, None, None, None, out_dtype=DT)
        d2 = ops._conv_desc(p2, x, None, res if res is not None else x, None, out)
        if edit:
            edit(d1, d2)
        return bool(L.lib().hiseg_resblock_fused_ok(ctypes.byref(d1), ctypes.byref(d2)))

    assert ok()
    wide = ops.Act.new(2, 20, 24, 128, DT, DEV)
    assert ok(x=wide.slice(64, 64))                  # a channel view of the input is handled
    assert not ok(out=wide.slice(0, 64))             # an output view is not
    assert not ok(out=x)                             # in place
    assert not ok(res=_x((2, 20, 24), 79))           # a residual that is not the block's input
    assert not ok(edit=lambda d1, d2: setattr(d2, "act", 3))
    assert not ok(edit=lambda d1, d2: setattr(d1, "a_gate", torch.ones(2, 64, device=DEV)))
    def huge(d1, d2):   # operands of 2^31 bytes or more
        d1.N = d2.N = 1 << 16
    assert not ok(edit=huge)


# ---------------------------------------------------------------------------------- the whole model
def test_rgb_model_forward_equals_the_bypassed_fusion(monkeypatch):
    import hiseg
    from hiseg import _lib as L, engine
    m = filler.fill_module(hiseg.create_rgb_hierarchical_model(**hiseg_kwargs(b0_kwargs()))).eval().to(DEV)
    m = hiseg.set_compute_dtype(m, DT)
    for r in (m.roi_align_mask, m.roi_align_rgb):
        r.spatial_scale_h, r.spatial_scale_w = 96, 128
    g = load("variants")
    images, rois, u = (torch.from_numpy(g[k]).to(DEV) for k in ("model_images", "model_rois", "model_u"))

    def run(fused):
        monkeypatch.setattr(engine, "RESBLOCK_FUSED", fused)
        L.conv_path_stats(reset=True)
        logits, aux = engine.rgb_model_forward(m, images, rois, "full", unet_logit_override=u)
        torch.cuda.synchronize()
        return logits, aux, L.conv_path_stats(reset=True)["resblock"]

    old, old_aux, n_old = run(False)
    new, new_aux, n_new = run(True)
    assert n_old == 0 and n_new >= 1, (n_old, n_new)
    assert torch.isfinite(new).all()
    assert torch.equal(new, old)
    for k, v in old_aux.items():
        if torch.is_tensor(v):
            assert torch.equal(new_aux[k], v), k
