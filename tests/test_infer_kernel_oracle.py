"""The hand-written float64 oracles of tests/infer_kernel_oracle.py against independent float64 statements of the
same operations (torch.nn.functional and oracle/rgb_model.py), and the properties of the constructed inputs that the
GPU tests compare exactly on.  CPU only; the bound is float64 rounding (rel_err < 1e-12)."""
import pytest
import torch
import torch.nn.functional as F

import infer_kernel_oracle as O
from oracle import rgb_model as R

TOL = 1e-12
ACT_NAMES = {O.ACT_RELU: "relu", O.ACT_SILU: "silu", O.ACT_SWISH: "swish"}


def rel_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def rnd(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=torch.float64)


def nchw(x):
    return x.permute(0, 3, 1, 2)


def nhwc(x):
    return x.permute(0, 2, 3, 1)


@pytest.mark.parametrize("H,W", [(7, 5), (4, 6)])
def test_maxpool_matches_max_pool2d(H, W):
    x = rnd(torch.Generator().manual_seed(1), 2, H, W, 12) - 3.0
    assert torch.equal(O.maxpool2x2(x), nhwc(F.max_pool2d(nchw(x), 2)))


@pytest.mark.parametrize("k", [3, 7])
@pytest.mark.parametrize("H,W", [(2, 3), (5, 7)])
def test_spatial_attention_matches_conv2d_and_rgb_model(k, H, W):
    g = torch.Generator().manual_seed(2 + k)
    x, w = rnd(g, 2, H, W, 20), rnd(g, 2, k, k)
    r = O.attn_spatial(x, w)
    xn = nchw(x)
    s = torch.cat([xn.mean(1, keepdim=True), xn.max(1, keepdim=True).values], 1)
    arg = F.conv2d(s, w[None], padding=k // 2)[:, 0]
    assert rel_err(r["arg"], arg) < TOL
    assert rel_err(r["att"], torch.sigmoid(arg)) < TOL
    assert torch.equal(r["max"], xn.max(1).values)
    assert rel_err(r["out"], nhwc(R.spatial_attention({"a.conv.weight": w[None]}, "a", xn))) < TOL
    assert rel_err(O.pixel_scale(x, r["att"]), r["out"]) == 0


@pytest.mark.parametrize("act", [O.ACT_RELU, O.ACT_SILU, O.ACT_SWISH])
def test_se_gate_matches_channel_attention(act):
    g = torch.Generator().manual_seed(3)
    N, H, W, C, Cr, beta = 2, 5, 7, 24, 6, 1.5
    x, w1, w2 = rnd(g, N, H * W, C), rnd(g, Cr, C), rnd(g, C, Cr)
    for splits in (1, 4, 35):
        part = O.gap_partials(x, splits)
        assert rel_err(part.sum(1), x.sum(1)) < TOL
        r = O.se_gate(part, H * W, w1, None, w2, None, act, beta)
        out = O.channel_scale(x, r["gate"]).view(N, H, W, C)
        sd = {"a.fc1.weight": w1.view(Cr, C, 1, 1), "a.fc2.weight": w2.view(C, Cr, 1, 1)}
        ref = R.channel_attention(sd, "a", nchw(x.view(N, H, W, C)), f"{ACT_NAMES[act]}:{beta}")
        assert rel_err(out, nhwc(ref)) < TOL


def test_se_gate_with_biases_matches_effnet_se():
    g = torch.Generator().manual_seed(4)
    N, H, W, C, Cr = 3, 4, 5, 16, 4
    x, w1, b1, w2, b2 = rnd(g, N, H * W, C), rnd(g, Cr, C), rnd(g, Cr), rnd(g, C, Cr), rnd(g, C)
    r = O.se_gate(O.gap_partials(x, 2), H * W, w1, b1, w2, b2, O.ACT_SILU)
    sd = {"s.conv_reduce.weight": w1.view(Cr, C, 1, 1), "s.conv_reduce.bias": b1,
          "s.conv_expand.weight": w2.view(C, Cr, 1, 1), "s.conv_expand.bias": b2}
    ref = R._se(sd, "s", nchw(x.view(N, H, W, C)))
    assert rel_err(O.channel_scale(x, r["gate"]).view(N, H, W, C), nhwc(ref)) < TOL


def test_image_max_bits_orders_signed_zeros():
    bits = lambda v: torch.tensor([v], dtype=torch.float32).view(torch.int32).item() & 0xFFFFFFFF
    assert O.image_max_bits(torch.tensor([-3.0, -0.0, -1.0])) == bits(-0.0) == 0x80000000
    assert O.image_max_bits(torch.tensor([-3.0, -0.0, 0.0, -1.0])) == 0
    assert O.image_max_bits(torch.tensor([-3.0, -2.5])) == bits(-2.5)
    x = torch.randn(1000, generator=torch.Generator().manual_seed(5))
    assert O.image_max_bits(x) == bits(x.max().item())


@pytest.mark.parametrize("top,divided", [(1.0, False), (float(torch.nextafter(torch.tensor(1.0), torch.tensor(2.0))), True),
                                         (200.0, True)])
def test_input_norm_matches_rgb_model_prologue(top, divided):
    g = torch.Generator().manual_seed(6)
    x = torch.rand(2, 3, 4, 5, generator=g, dtype=torch.float64) * 0.9
    x[1, 2, 3, 4] = top
    mean, std = rnd(g, 3), rnd(g, 3).abs() + 0.5
    v = x / 255.0 if x.max() > 1.0 else x                      # pretrained_unet_logits' prologue
    ref = (v - mean.view(1, 3, 1, 1)) / std.view(1, 3, 1, 1)
    out = O.input_norm(x, mean, std, 8)
    assert rel_err(out[..., :3], nhwc(ref)) < TOL
    assert (out[..., 3:] == 0).all()
    assert bool(x.max() > 1.0) == divided


def _head(g, N, h, w, Ct, per_sample):
    return dict(low=rnd(g, N, h, w, 2), tfeat=rnd(g, N, 2 * h, 2 * w, Ct), ut_w=rnd(g, 2, 32, 2, 2), ut_b=rnd(g, 32),
                scale=rnd(g, N, 32) if per_sample else rnd(g, 32), shift=rnd(g, N, 32) if per_sample else rnd(g, 32),
                u1_w=rnd(g, 2, 32), u1_b=rnd(g, 2), t_w=rnd(g, 2, Ct), t_b=rnd(g, 2))


@pytest.mark.parametrize("act,beta", [(O.ACT_NONE, 1.0), (O.ACT_RELU, 1.0), (O.ACT_SILU, 1.0), (O.ACT_SWISH, 1.5)])
@pytest.mark.parametrize("per_sample", [False, True])
def test_hier_combine_matches_conv_transpose_and_softmax(act, beta, per_sample):
    g = torch.Generator().manual_seed(7)
    N, h, w, Ct = 3, 3, 5, 12
    c = _head(g, N, h, w, Ct, per_sample)
    r = O.hier_combine(c["low"], c["tfeat"], None, c["ut_w"], c["scale"], c["shift"], act, beta, c["u1_w"], c["u1_b"],
                       c["t_w"], c["t_b"])
    z = F.conv_transpose2d(nchw(c["low"]), c["ut_w"], None, stride=2)
    assert rel_err(O.conv_transpose_2x2(c["low"], c["ut_w"]), z) < TOL
    hs = z * c["scale"].reshape(-1, 32, 1, 1) + c["shift"].reshape(-1, 32, 1, 1)
    hs = hs if act == O.ACT_NONE else R.act(hs, ACT_NAMES[act], beta)
    bgfg = F.conv2d(hs, c["u1_w"].view(2, 32, 1, 1), c["u1_b"])
    tn = F.conv2d(nchw(c["tfeat"]), c["t_w"].view(2, Ct, 1, 1), c["t_b"])
    p_fg = F.softmax(bgfg, dim=1)[:, 1]
    logits = torch.stack([bgfg[:, 0], bgfg[:, 1] + tn[:, 0] * p_fg, bgfg[:, 1] + tn[:, 1] * p_fg], dim=1)   # hier_head
    assert rel_err(r["logits"], logits) < TOL
    assert rel_err(r["bgfg"], bgfg) < TOL
    assert rel_err(r["tn"], tn) < TOL
    r2 = O.hier_combine(c["low"], None, nhwc(tn).contiguous(), c["ut_w"], c["scale"], c["shift"], act, beta, c["u1_w"],
                        c["u1_b"], None, None)
    assert rel_err(r2["logits"], logits) < TOL


@pytest.mark.parametrize("fold_bias", [0, 1])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("affine", [False, True])
def test_ln_tables_match_layer_norm(fold_bias, with_bias, affine):
    g = torch.Generator().manual_seed(8)
    N, h, w, eps = 3, 3, 5, 1e-5
    low, ut_w = rnd(g, N, h, w, 2) + 2.0, rnd(g, 2, 32, 2, 2)
    ut_b = rnd(g, 32) if with_bias else None
    gamma, beta = (rnd(g, 32), rnd(g, 32)) if affine else (None, None)
    r = O.ubf_ln_tables(low, ut_w, ut_b, gamma, beta, eps, fold_bias)
    z = F.conv_transpose2d(nchw(low), ut_w, ut_b, stride=2)
    ref = F.layer_norm(z, z.shape[1:], eps=eps)
    if affine:
        ref = ref * gamma.view(1, 32, 1, 1) + beta.view(1, 32, 1, 1)
        sd = {"n.weight": gamma.view(1, 32, 1, 1), "n.bias": beta.view(1, 32, 1, 1)}
        assert rel_err(R.layernorm2d(sd, "n", z, eps), ref) < TOL
    zin = F.conv_transpose2d(nchw(low), ut_w, None, stride=2) if fold_bias else z   # what the tables are applied to
    out = zin * r["scale"].view(N, 32, 1, 1) + r["shift"].view(N, 32, 1, 1)
    assert rel_err(out, ref) < TOL
    assert rel_err(r["mean"], z.mean(dim=(1, 2, 3))) < TOL
    assert rel_err(r["invstd"], 1 / torch.sqrt(z.var(dim=(1, 2, 3), unbiased=False) + eps)) < TOL


def test_layout_converters_are_permutes():
    x = rnd(torch.Generator().manual_seed(9), 2, 5, 3, 4)
    out = O.nchw_to_nhwc(x, 8)
    assert torch.equal(out[..., :5], nhwc(x)) and (out[..., 5:] == 0).all()
    assert torch.equal(O.nhwc_to_nchw(out, 5, 0), x)
    assert torch.equal(O.nhwc_to_nchw(out, 3, 1), x[:, 1:4])


@pytest.mark.parametrize("N,mh,mw,dil", O.INSTANCE_CASES)
def test_instance_mask_inputs_and_oracle(N, mh, mw, dil):
    lg = O.instance_logits(N, mh, mw, dil)
    assert torch.equal(lg, lg.float().double())
    r = O.instance_masks(lg, dil)
    assert r["gap"].min() >= O.INSTANCE_MARGIN                       # every pixel's top-two logit gap
    if dil > 0:
        assert r["margin"].abs().min() >= O.INSTANCE_MARGIN          # |mx - p1 - 0.1| of every pixel
        assert (r["margin"] > 0).any() and (r["margin"] < 0).any()   # both outcomes of the dilation rule
        probs = F.softmax(lg, dim=1)[:, 1:2]
        dilated = F.max_pool2d(probs, 2 * dil + 1, stride=1, padding=dil)
        assert rel_err(r["margin"], (dilated - probs)[:, 0] - 0.1) < TOL
    assert torch.equal(r["inst"], R.instance_masks(lg, dil).double())
    assert torch.equal(r["inst"], R.instance_masks(lg.float(), dil).double())   # the same decisions in float32
    assert 0 < r["inst"].mean() < 1


def test_instance_mask_ties_take_the_first_maximum():
    lg = O.instance_tie_logits()
    r = O.instance_masks(lg, 0)
    assert r["inst"][0, 0, 0, 0] == 0 and r["inst"][0, 0, 0, 1] == 1
    assert torch.equal(r["inst"], R.instance_masks(lg, 0).double())
    gap = r["gap"].clone()
    gap[0, 0, 0], gap[0, 0, 1] = 1.0, 1.0      # the two hand-set ties; every other pixel keeps its margin
    assert gap.min() >= O.INSTANCE_MARGIN


def test_binary_masks_output_conv_distance_mask():
    g = torch.Generator().manual_seed(10)
    u, w, b, thr = rnd(g, 2, 1, 5, 7), rnd(g, 2), rnd(g, 2), rnd(g, 1)
    sd = {"pretrained_unet.output_conv.weight": w.view(2, 1, 1, 1), "pretrained_unet.output_conv.bias": b}
    assert rel_err(O.binary_masks(u[:, 0], w, b)["binary"], R.binary_masks(sd, u)[:, 0]) < TOL
    assert rel_err(O.output_conv(u[:, 0], w, b), F.conv2d(u, w.view(2, 1, 1, 1), b)) < TOL
    assert rel_err(O.distance_mask(u, thr)["mask"], torch.sigmoid((u - thr) * 10)) < TOL


@pytest.mark.parametrize("H,W,Ho,Wo", [(1, 6, 3, 9), (5, 1, 7, 2), (4, 6, 1, 3), (7, 9, 3, 4), (3, 4, 6, 8)])
def test_resize_bilinear_matches_interpolate(H, W, Ho, Wo):
    x = rnd(torch.Generator().manual_seed(11), 3, H, W)
    ref = F.interpolate(x[None], size=(Ho, Wo), mode="bilinear", align_corners=False)[0]
    assert rel_err(O.resize_bilinear(x, Ho, Wo), ref) < TOL


@pytest.mark.parametrize("dt", list(O.DTYPES))
@pytest.mark.parametrize("name", list(O.SE_CASES) + list(O.SE_PARTIAL_CASES))
def test_se_inputs_keep_relu_units_off_zero(name, dt):
    N, HW, C, Cr, act, beta, bias = {**O.SE_CASES, **O.SE_PARTIAL_CASES}[name]
    x, w1, b1, w2, b2 = O.se_inputs(name, dt)
    assert torch.equal(x, x.to(O.DTYPES[dt]).double()) and torch.equal(w1, w1.float().double())
    r = O.se_gate(O.gap_partials(x, 1), HW, w1, b1, w2, b2, act, beta)
    z1 = r["z1"]
    assert z1.abs().min() >= O.SE_RELU_MARGIN                        # no hidden unit near the ReLU's kink
    assert (z1 > 0).any(1).all() and (z1 < 0).any(1).all()           # every image: a live and a dead unit
    assert not torch.equal(z1[0] > 0, z1[1] > 0)                     # the pattern differs between images
    assert (beta * z1).abs().max() <= 16 and r["z2"].abs().max() <= 16
    assert (b1 is not None) == bias and (b2 is not None) == bias
