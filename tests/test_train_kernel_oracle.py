"""The hand-written float64 oracles of tests/train_kernel_oracle.py against float64 autograd of the plain torch
modules they restate.  CPU only; the bound is float64 rounding (rel_err < 1e-12)."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import train_kernel_oracle as O

TOL = 1e-12


def rel_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def rnd(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=torch.float64)


@pytest.mark.parametrize("k", [7, 3])
@pytest.mark.parametrize("with_mul", [False, True])
def test_spatial_attention_matches_conv2d_module(k, with_mul):
    gen = torch.Generator().manual_seed(10 + k)
    N, H, W, C = 2, 5, 7, 16
    x, dout = rnd(gen, N, H, W, C), rnd(gen, N, H, W, C)
    conv = nn.Conv2d(2, 1, k, padding=k // 2, bias=False).double()
    mul = None
    if with_mul:
        mul = (torch.rand(N, C, generator=gen, dtype=torch.float64) > 0.3).double() / 0.7
    xr = x.clone().requires_grad_(True)
    xn = xr.permute(0, 3, 1, 2)
    att = torch.sigmoid(conv(torch.cat([xn.mean(1, keepdim=True), xn.max(1, keepdim=True).values], 1)))
    out = (xn * att).permute(0, 2, 3, 1)
    if mul is not None:
        out = out * mul[:, None, None, :]
    (out * dout).sum().backward()
    old = rnd(gen, 2, k, k)
    r = O.spatial_attention(x, conv.weight.detach()[0], mul, dout, old)
    assert rel_err(r["out"], out.detach()) < TOL
    assert rel_err(r["att"], att.detach()[:, 0]) < TOL
    assert rel_err(r["dx"], xr.grad) < TOL
    assert rel_err(r["dw7"], conv.weight.grad[0] + old) < TOL
    assert torch.equal(r["argmax"], x.argmax(-1))


def test_first_argmax_takes_the_first_of_tied_maxima():
    x = torch.tensor([[1.0, 3.0, 3.0, 2.0], [5.0, 1.0, 5.0, 5.0], [0.0, 0.0, 0.0, 0.0]])
    assert O.first_argmax(x).tolist() == [1, 0, 0]


@pytest.mark.parametrize("bias,act,beta", [(False, O.ACT_RELU, 1.0), (False, O.ACT_SWISH, 1.5), (True, O.ACT_SILU, 1.0)])
def test_channel_attention_matches_two_linears(bias, act, beta):
    gen = torch.Generator().manual_seed(20)
    N, HW, C, Cr = 2, 130, 24, 6
    x, dout = rnd(gen, N, HW, C), rnd(gen, N, HW, C)
    fc1, fc2 = nn.Linear(C, Cr, bias=bias).double(), nn.Linear(Cr, C, bias=bias).double()
    mul = (torch.rand(N, C, generator=gen, dtype=torch.float64) > 0.3).double() / 0.7
    xr = x.clone().requires_grad_(True)
    h = fc1(xr.mean(1))
    h = {O.ACT_RELU: F.relu(h), O.ACT_SILU: F.silu(h), O.ACT_SWISH: h * torch.sigmoid(beta * h)}[act]
    out = xr * torch.sigmoid(fc2(h)).unsqueeze(1) * mul.unsqueeze(1)
    (out * dout).sum().backward()
    b1 = fc1.bias.detach() if bias else None
    b2 = fc2.bias.detach() if bias else None
    r = O.channel_attention(x, fc1.weight.detach(), b1, fc2.weight.detach(), b2, act, beta, mul, dout)
    assert rel_err(r["out"], out.detach()) < TOL
    assert rel_err(r["dx"], xr.grad) < TOL
    assert rel_err(r["dw1"], fc1.weight.grad) < TOL
    assert rel_err(r["dw2"], fc2.weight.grad) < TOL
    if bias:
        assert rel_err(r["db1"], fc1.bias.grad) < TOL
        assert rel_err(r["db2"], fc2.bias.grad) < TOL


def ubf_inputs(gen, N, h, w, Ct, dtype=torch.float64):
    p = {"ut_w": 0.5 * rnd(gen, 2, 32, 2, 2), "ut_b": 0.1 * rnd(gen, 32), "gamma": 1 + 0.2 * rnd(gen, 32),
         "beta": 0.2 * rnd(gen, 32), "u1_w": 0.3 * rnd(gen, 2, 32), "u1_b": 0.1 * rnd(gen, 2)}
    low = rnd(gen, N, h, w, 2)
    tfeat = rnd(gen, N, 2 * h, 2 * w, Ct)
    t_w, t_b = 0.3 * rnd(gen, 2, Ct), 0.1 * rnd(gen, 2)
    grads = (rnd(gen, N, 3, 2 * h, 2 * w), rnd(gen, N, 2, 2 * h, 2 * w), rnd(gen, N, 2, 2 * h, 2 * w))
    return low, p, tfeat, t_w, t_b, grads


@pytest.mark.parametrize("layernorm", [0, 1])
@pytest.mark.parametrize("act,beta", [(O.ACT_RELU, 1.0), (O.ACT_SWISH, 1.5)])
@pytest.mark.parametrize("ext", [False, True])
def test_ubf_head_matches_torch_modules(layernorm, act, beta, ext):
    gen = torch.Generator().manual_seed(30)
    N, h, w, Ct = 2, 3, 5, 16
    low, p, tfeat, t_w, t_b, grads = ubf_inputs(gen, N, h, w, Ct)
    H, W = 2 * h, 2 * w
    ct = nn.ConvTranspose2d(2, 32, 2, 2).double()
    c1 = nn.Conv2d(32, 2, 1).double()
    norm = nn.LayerNorm((32, H, W), eps=1e-5).double() if layernorm else nn.BatchNorm2d(32).double()
    rm0, rv0 = 0.3 * rnd(gen, 32), 0.5 + torch.rand(32, generator=gen, dtype=torch.float64)
    with torch.no_grad():
        ct.weight.copy_(p["ut_w"]), ct.bias.copy_(p["ut_b"])
        c1.weight.copy_(p["u1_w"].view(2, 32, 1, 1)), c1.bias.copy_(p["u1_b"])
        if layernorm:   # LayerNorm2d: a per-channel affine over the (C, H, W) normalisation
            norm.weight.copy_(p["gamma"].view(32, 1, 1).expand(32, H, W))
            norm.bias.copy_(p["beta"].view(32, 1, 1).expand(32, H, W))
        else:
            norm.weight.copy_(p["gamma"]), norm.bias.copy_(p["beta"])
            norm.running_mean.copy_(rm0), norm.running_var.copy_(rv0)
    norm.train()
    lr = low.clone().requires_grad_(True)
    v = norm(ct(lr.permute(0, 3, 1, 2)))
    a = F.relu(v) if act == O.ACT_RELU else v * torch.sigmoid(beta * v)
    b = c1(a)
    tn = (tfeat @ t_w.t() + t_b).permute(0, 3, 1, 2).detach().requires_grad_(True)
    pf = torch.softmax(b, 1)[:, 1:2]
    logits = torch.cat([b[:, :1], b[:, 1:2] + tn * pf], 1)
    loss = (logits * grads[0]).sum()
    if ext:
        loss = loss + (b * grads[1]).sum() + (tn * grads[2]).sum()
    loss.backward()
    r = O.ubf_head(low, p, tfeat, t_w, t_b, act, beta, layernorm, running=(rm0, rv0),
                   grads=(grads[0], grads[1] if ext else None, grads[2] if ext else None))
    assert rel_err(r["logits"], logits.detach()) < TOL
    assert rel_err(r["bgfg"], b.detach()) < TOL
    assert rel_err(r["tn"], tn.detach()) < TOL
    assert rel_err(r["dlow"], lr.grad) < TOL
    assert rel_err(r["dtn_out"], tn.grad.permute(0, 2, 3, 1).reshape(-1, 2)) < TOL
    assert rel_err(r["dut_w"], ct.weight.grad) < TOL
    # the bias in front of a normalisation has a mathematically zero gradient: compare on the scale of its terms
    assert (r["dut_b"] - ct.bias.grad).abs().max() < TOL * max(1.0, ct.weight.grad.abs().max().item())
    assert rel_err(r["du1_w"], c1.weight.grad.view(2, 32)) < TOL
    assert rel_err(r["du1_b"], c1.bias.grad) < TOL
    if layernorm:
        assert rel_err(r["dgamma"], norm.weight.grad.sum((1, 2))) < TOL
        assert rel_err(r["dbeta"], norm.bias.grad.sum((1, 2))) < TOL
    else:
        assert rel_err(r["dgamma"], norm.weight.grad) < TOL
        assert rel_err(r["dbeta"], norm.bias.grad) < TOL
        assert rel_err(r["running_mean"], norm.running_mean) < TOL
        assert rel_err(r["running_var"], norm.running_var) < TOL


def roi_case(gen, dtype=torch.float64):
    u = torch.randn(2, 1, 9, 13, generator=gen, dtype=dtype)
    rois = torch.tensor([[0, 0.20, 0.25, 0.70, 0.80],      # inside the map
                         [0, -0.15, -0.20, 0.40, 0.50],    # clipped on the left and top
                         [0, 0.55, 0.45, 1.20, 1.25],      # past the right and bottom edges
                         [0, 1.40, 1.50, 1.90, 2.10],      # wholly outside
                         [0, 0.45, 0.55, 0.45, 0.55],      # zero area
                         [1, 0.10, 0.05, 0.90, 0.95]],     # image 1
                        dtype=dtype)
    g = torch.randn(6, 4, 6, 2, generator=gen, dtype=dtype)
    return u, rois, g


@pytest.mark.parametrize("aligned", [0, 1])
def test_roi_align_affine_matches_grid_sample(aligned):
    gen = torch.Generator().manual_seed(40)
    u, rois, g = roi_case(gen)
    H, W, oh, ow = 9, 13, 4, 6
    sh, sw = float(H), float(W)
    w = torch.tensor([0.7, -1.3], dtype=torch.float64, requires_grad=True)
    b = torch.tensor([0.2, -0.4], dtype=torch.float64, requires_grad=True)
    feat = u * w.view(1, 2, 1, 1) + b.view(1, 2, 1, 1)
    ix, iy = O.roi_sample_coords(rois, oh, ow, sh, sw, H, W, aligned)
    if aligned:
        nx, ny = ix / ((W - 1) / 2) - 1, iy / ((H - 1) / 2) - 1
    else:
        nx, ny = (ix + 0.5) / (W / 2) - 1, (iy + 0.5) / (H / 2) - 1
    grid = torch.stack([nx[:, None, :].expand(-1, oh, -1), ny[:, :, None].expand(-1, -1, ow)], dim=-1)
    r = F.grid_sample(feat[rois[:, 0].long()], grid, mode="bilinear", padding_mode="zeros", align_corners=bool(aligned))
    (r.permute(0, 2, 3, 1) * g).sum().backward()
    dw, db = O.roi_align_bwd_affine(u, rois, g, oh, ow, sh, sw, aligned)
    assert rel_err(dw, w.grad) < TOL
    assert rel_err(db, b.grad) < TOL
    # the box wholly outside the map contributes nothing to either gradient (taps outside the map are 0)
    g_out = torch.zeros_like(g)
    g_out[3] = g[3]
    dw0, db0 = O.roi_align_bwd_affine(u, rois, g_out, oh, ow, sh, sw, aligned)
    assert dw0.abs().max() == 0 and db0.abs().max() == 0


RESIZE_CASES = [((16, 12), (32, 24)), ((7, 5), (32, 24)), ((9, 11), (4, 6)), ((1, 1), (5, 3)), ((6, 1), (6, 4))]


@pytest.mark.parametrize("src,dst", RESIZE_CASES)
def test_resize_matches_interpolate(src, dst):
    gen = torch.Generator().manual_seed(50)
    x = rnd(gen, 3, *src).requires_grad_(True)
    g = rnd(gen, 3, *dst)
    y = F.interpolate(x.unsqueeze(0), size=dst, mode="bilinear", align_corners=False)[0]
    (y * g).sum().backward()
    assert rel_err(O.resize_bilinear_fwd(x.detach(), *dst), y.detach()) < TOL
    assert rel_err(O.resize_bilinear_bwd(g, *src), x.grad) < TOL


def test_layernorm2d_matches_layer_norm():
    gen = torch.Generator().manual_seed(60)
    N, HW, C = 3, 35, 5
    z, res, dy = rnd(gen, N, HW, C), rnd(gen, N, HW, C), rnd(gen, N, HW, C)
    gamma, beta = 1 + 0.2 * rnd(gen, C), 0.2 * rnd(gen, C)
    mul = (torch.rand(N, C, generator=gen, dtype=torch.float64) > 0.3).double() / 0.7
    bias = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    zr, rr = z.clone().requires_grad_(True), res.clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    v = F.layer_norm(zr + bias, (HW, C), eps=1e-5) * gr + br + rr
    y = F.gelu(v) * mul.unsqueeze(1)
    (y * dy).sum().backward()
    r = O.layernorm2d(z, gamma, beta, 1e-5, O.ACT_GELU, 1.0, res, mul, dy)
    for name, ref in (("y", y.detach()), ("dz", zr.grad), ("dres", rr.grad), ("dgamma", gr.grad), ("dbeta", br.grad)):
        assert rel_err(r[name], ref) < TOL, name
    assert (r["dconv_bias"] - bias.grad).abs().max() < TOL * zr.grad.abs().sum().item()


def test_maxpool_and_upsample_match_autograd():
    gen = torch.Generator().manual_seed(70)
    x = rnd(gen, 2, 6, 10, 5)
    dy = rnd(gen, 2, 3, 5, 5)
    xr = x.clone().requires_grad_(True)
    (F.max_pool2d(xr.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1) * dy).sum().backward()
    assert torch.equal(O.maxpool2x2_bwd(x, dy), xr.grad)
    # ties: the first of (0,0), (0,1), (1,0), (1,1)
    tie = torch.zeros(1, 2, 2, 1, dtype=torch.float64)
    assert O.maxpool2x2_bwd(tie, torch.ones(1, 1, 1, 1, dtype=torch.float64)).flatten().tolist() == [1, 0, 0, 0]
    tie[0, 0, 1, 0] = tie[0, 1, 0, 0] = 2.0
    assert O.maxpool2x2_bwd(tie, torch.ones(1, 1, 1, 1, dtype=torch.float64)).flatten().tolist() == [0, 1, 0, 0]
    g = rnd(gen, 2, 6, 10, 8)
    lo = rnd(gen, 2, 3, 5, 8).requires_grad_(True)
    up = F.interpolate(lo.permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1)
    (up * g).sum().backward()
    assert rel_err(O.upsample2x_bwd(g), lo.grad) < TOL


@pytest.mark.parametrize("act,beta", [(a, 1.0) for a in range(6)] + [(O.ACT_SWISH, 1.5), (O.ACT_SWISH, 0.75)])
def test_activation_derivatives_closed_forms(act, beta):
    gen = torch.Generator().manual_seed(80)
    z, dy = rnd(gen, 105, 5), rnd(gen, 105, 5)
    s = torch.sigmoid(beta * z)
    closed = {O.ACT_NONE: torch.ones_like(z), O.ACT_RELU: (z > 0).double(), O.ACT_SIGMOID: s * (1 - s),
              O.ACT_SILU: s * (1 + z * (1 - s)), O.ACT_SWISH: s * (1 + beta * z * (1 - s)),
              O.ACT_GELU: 0.5 * (1 + torch.erf(z / 2 ** 0.5)) + z * torch.exp(-z * z / 2) / (2 * torch.pi) ** 0.5}[act]
    assert rel_err(O.act_bwd_pre(dy, z, act, beta), dy * closed) < TOL
    if act in (O.ACT_NONE, O.ACT_RELU, O.ACT_SIGMOID):   # recoverable from the output
        assert rel_err(O.act_bwd_cvt(dy, O.act_fn(z, act), act), dy * closed) < TOL


def test_splitmix64_and_dropout_mask():
    # splitmix64's published first outputs for the state 0 (Vigna's reference implementation)
    assert O.splitmix64(0) == 0xE220A8397B1DCDAF
    assert O.splitmix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    m = O.dropout2d_mask(210, 0.3, 1234)
    keep = np.float32(1.0) / (np.float32(1.0) - np.float32(0.3))
    assert set(np.unique(m).tolist()) == {0.0, float(keep)}
    assert 0.15 < (m == 0).mean() < 0.45
    assert np.all(O.dropout2d_mask(210, 0.0, 1234) == 1.0)
    assert O.dropout2d_dev_seed(5, 7) == (5 * 0x9E3779B1 + 7) & ((1 << 48) - 1)
    assert O.dropout2d_dev_seed(2 ** 40 + 3, 11) == ((2 ** 40 + 3) * 0x9E3779B1 + 11) % 2 ** 48
    assert np.array_equal(O.dropout2d_mask_dev(210, 0.3, 5, 7), O.dropout2d_mask(210, 0.3, O.dropout2d_dev_seed(5, 7)))
