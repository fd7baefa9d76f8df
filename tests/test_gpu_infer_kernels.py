"""Each inference non-convolution kernel of csrc/misc.hip on its own against the float64 oracles of
tests/infer_kernel_oracle.py, called directly through hiseg._lib.

Inputs are rounded to the compute dtype before either side sees them, nothing is excluded from a comparison, every
output buffer is pre-filled with a sentinel (and carries a guard tail that must stay untouched), and every bound is
built from `e32`, the element-wise error of torch's own float32 evaluation of the same oracle:

  f32 output                       |k - ref| <= 4 max(e32) + 4 * 2^-23 max|ref|
  bf16 output written once         2^-8 |ref| + the f32 rule
  through a fast intrinsic         + the term derived below

Max-pool, the layout converters, image_max, the max half of the attention statistics, the instance masks, zero
padding and every "the same bits" claim of the source are exact; bf16 conversions are compared with torch's
`.to(torch.bfloat16)` of the float32 value (round to nearest even).

The fast intrinsics.  __expf(x) is exp2(fl(x * L)) with L = fl(log2 e).  fl(x * L) = x log2(e) (1 + a)(1 + b) with
|a| <= 2^-24 (the product's rounding) and |b| <= 0.22 * 2^-24 (L itself: 1.44269502 against 1.4426950409), and
exp2(y (1 + e)) = exp2(y) exp(ln2 y e), so the argument's error reaches the result as a relative |x| * 1.25 * 2^-24;
the hardware exp2 (v_exp_f32) is documented to 1 ulp, a relative 2^-23:

  dexp(x) = 1.25 * 2^-24 |x| + 2^-23                                   relative error of __expf(x)

sigmoidf_(x) = rcp(fl(1 + __expf(-x))) -- the sum rounds once (2^-24), v_rcp_f32 is 1 ulp (2^-23) -- and with
s = sigmoid(x), d s / d E = -s^2, E / (1 + E) = 1 - s:

  dsig(x) = s (1 - s) dexp(x) + 1.5 * 2^-23 s                          absolute error of sigmoidf_(x)

The two-way softmaxes (hier_combine's p_fg, binary_masks) are e_a / (e_a + e_b) with one of the two exactly
exp(0) = 1 and an IEEE division: the same form with a smaller constant, so dsig(d) of the logit difference d covers
them.  An intrinsic inside a SiLU / Swish adds |v| dsig(beta v) to that activation's value, carried to the outputs
through the absolute values of the weights that follow it.  All arguments are asserted to lie within |x| <= 16.

Entry point -> test
  hiseg_maxpool2x2_fwd                    test_maxpool2x2, test_maxpool2x2_refuses_one_row
  hiseg_attn_map_fwd, hiseg_pixel_scale_fwd, hiseg_attn_spatial_fwd
                                          test_spatial_attention, test_spatial_attention_refuses_even_kernel
  hiseg_se_gate_fwd                       test_se_gate, test_se_gate_refuses_small_partial
  hiseg_se_gate_partials_fwd              test_se_gate_partials, test_se_gate_partials_refuses_swish
  hiseg_channel_scale_fwd                 test_channel_scale, test_channel_scale_refuses_no_channels
  hiseg_image_max_fwd                     test_image_max, test_image_max_four_in_flight
  hiseg_input_norm_fwd                    test_input_norm, test_input_norm_refusals
  hiseg_hier_combine_fwd                  test_hier_combine, test_hier_combine_edges
  hiseg_hier_combine_tn_fwd               test_hier_combine_tn
  hiseg_ubf_ln_tables                     test_ubf_ln_tables
  hiseg_nchw_to_nhwc_fwd                  test_nchw_to_nhwc
  hiseg_nhwc_to_nchw_fwd                  test_nhwc_to_nchw
  hiseg_instance_masks_fwd                test_instance_masks, test_instance_masks_ties
  hiseg_binary_masks_fwd                  test_binary_masks
  hiseg_output_conv_fwd                   test_output_conv
  hiseg_distance_mask_fwd                 test_distance_mask
  hiseg_resize_bilinear_fwd               test_resize_bilinear_fwd

Worst observed ratio of kernel error over bound per kernel and dtype (profiles/infer_kernel_errors.txt):

  kernel                        f32     bf16
  attn_map                      0.129   0.113
  attn_spatial                  0.134   0.995
  attn_spatial_att              0.000   0.000
  attn_spatial_out              0.000   0.000
  attn_spatial_stats            0.000   0.000
  attn_stats_max                0.000   0.000
  attn_stats_mean               0.122   0.050
  binary_masks                  0.098   -
  channel_scale                 0.062   0.995
  distance_mask                 0.088   -
  hier_combine                  0.540   0.796
  hier_combine_tn               0.150   -
  hier_combine_tn_copy          0.000   -
  image_max                     0.000   -
  input_norm                    0.098   0.982
  instance_masks                0.000   -
  maxpool2x2                    0.000   0.000
  nchw_to_nhwc                  0.000   0.000
  nhwc_to_nchw                  0.000   0.000
  output_conv                   0.062   -
  pixel_scale                   0.070   0.995
  resize_bilinear_fwd           0.185   -
  se_gate                       0.194   0.233
  se_gate_alignment             0.000   0.000
  se_gate_partials              0.268   -
  ubf_ln_tables                 0.262   -
  (MI355X.  0.000: compared bit for bit.  A bf16 output written once sits near 1.0 by construction: 2^-8 |ref| is
  exactly the worst case of one round-to-nearest to bf16's 8-bit significand.  The f32 column is where the arithmetic
  itself is measured; the kernels through the fast intrinsics -- attn_map, binary_masks, distance_mask, se_gate,
  hier_combine -- stay well inside the derived term.)
"""
import math
import os

import pytest
import torch

import infer_kernel_oracle as O
from hiseg import _lib as L
from oracle import rgb_model as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = O.DTYPES
HD = {"f32": L.HISEG_F32, "bf16": L.HISEG_BF16}
CHUNK = {"f32": 4, "bf16": 8}
SENTINEL = -7.5          # exact in bf16; no kernel under test produces it
GUARD = 64
RATIOS = {}
OK, BAD_ARG, BAD_SHAPE, BAD_DTYPE = 0, -1, -2, -3


# ------------------------------------------------------------------------------------------- plumbing
def lib():
    return L.lib()


def stream():
    return L.stream_ptr()


def ok(status, what):
    L.check(status, what)
    torch.cuda.synchronize()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(g, dt, *shape, scale=1.0, shift=0.0):
    """float64 values that are exactly representable in the compute dtype."""
    return (shift + scale * torch.randn(*shape, generator=g, dtype=torch.float64)).to(DTYPES[dt]).double()


LIVE = []   # device inputs of the running test: a tensor made inside a call's argument list must outlive the call


def up(t, dtype=torch.float32):
    if t is None:
        return None
    LIVE.append(t.to(dtype).to(DEV).contiguous())
    return LIVE[-1]


@pytest.fixture(autouse=True)
def release_inputs():
    yield
    torch.cuda.synchronize()
    LIVE.clear()


def up_offset(t, floats):
    """t as float32 on the device, `floats` elements past a 16-byte boundary."""
    buf = torch.zeros(t.numel() + 8, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[floats:floats + t.numel()]
    v.copy_(t.reshape(-1).float())
    return v


def ptr(t):
    return None if t is None else t.data_ptr()


class Out:
    """A sentinel-filled output buffer with a guard tail."""

    def __init__(self, *shape, dtype=torch.float32):
        self.shape, self.n = shape, math.prod(shape)
        self.buf = torch.full((self.n + GUARD,), SENTINEL, dtype=dtype, device=DEV)

    def ptr(self):
        return self.buf.data_ptr()

    def get(self):
        torch.cuda.synchronize()
        assert bool((self.buf[self.n:] == SENTINEL).all()), "a store past the end of the output"
        return self.buf[:self.n].view(*self.shape).cpu()

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf == SENTINEL).all())


def both(fn, *args, **kw):
    """The oracle in float64 and in float32 on the same inputs."""
    def cast(a, dtype):
        if isinstance(a, torch.Tensor) and a.is_floating_point():
            return a.to(dtype)
        if isinstance(a, (tuple, list)):
            return type(a)(cast(v, dtype) for v in a)
        return a
    return fn(*cast(args, torch.float64), **cast(kw, torch.float64)), fn(*cast(args, torch.float32), **cast(kw, torch.float32))


def dexp(x):
    return 1.25 * 2.0 ** -24 * x.abs() + 2.0 ** -23


def dsig(x):
    """The absolute error bound of sigmoidf_(x) derived in the module docstring (x float64, |x| <= 16)."""
    assert x.abs().max() <= 16
    s = torch.sigmoid(x)
    return s * (1 - s) * dexp(x) + 1.5 * 2.0 ** -23 * s


def dact(pre, act, beta):
    """The intrinsic's share of the error of act(pre)."""
    if act in (O.ACT_SILU, O.ACT_SWISH):
        return pre.abs() * dsig((beta if act == O.ACT_SWISH else 1.0) * pre)
    return torch.zeros_like(pre)


def check(kernel, dt, what, k, r64, r32, mode="f32", extra=None):
    """Assert the bound of the module docstring; record the ratio error / bound."""
    k = k.detach().double().cpu().reshape(r64.shape)
    r64, r32 = r64.double(), r32.double()
    bound = (4 * (r32 - r64).abs().max() + 4 * 2.0 ** -23 * r64.abs().max()).expand_as(r64)
    if mode == "once":
        bound = bound + 2.0 ** -8 * r64.abs()
    if extra is not None:
        bound = bound + extra.double().reshape(r64.shape)
    err = (k - r64).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300)).max().item()
    key = (kernel, dt)
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    print(f"{kernel} {dt} {what}: max err {err.max().item():.3e} ratio {ratio:.3f}")
    assert ratio <= 1.0, f"{kernel} {dt} {what}: error / bound = {ratio:.3f} (max err {err.max().item():.3e})"


def exact(kernel, dt, what, k, ref):
    """Bit-for-bit equality (both sides in the same dtype)."""
    k, ref = k.detach().cpu().contiguous(), ref.detach().cpu().contiguous().reshape(k.shape)
    assert k.dtype == ref.dtype
    same = torch.equal(k.view(torch.uint8), ref.view(torch.uint8))
    RATIOS.setdefault((kernel, dt), 0.0)
    assert same, f"{kernel} {dt} {what}: {(k.view(torch.uint8) != ref.view(torch.uint8)).sum().item()} bytes differ"


def out_mode(dt):
    return "f32" if dt == "f32" else "once"


def refused(status, code, name, *outs):
    """A refusal: the status, a message of this call, and nothing written."""
    assert status == code, f"{name}: status {status}, expected {code}"
    msg = lib().hiseg_last_error_string().decode(errors="replace")
    assert msg.startswith(name), f"{name}: last error is {msg!r}"
    for o in outs:
        assert o.untouched(), f"{name}: a refused call wrote to an output"


@pytest.fixture(scope="module", autouse=True)
def ratio_report():
    yield
    path = os.environ.get("HISEG_INFER_KERNEL_ERRORS")
    if path:
        with open(path, "w") as f:
            f.write("# worst |kernel - float64 oracle| / bound per kernel and dtype (tests/test_gpu_infer_kernels.py);\n"
                    "# 0.000: compared bit for bit\n")
            for (kern, dt), r in sorted(RATIOS.items()):
                f.write(f"{kern:28s} {dt:5s} {r:.3f}\n")


@pytest.fixture(params=["se2", "se3"])
def se_mode(request, monkeypatch):
    """HISEG_SE2 unset (two launches where they fit) and HISEG_SE2=0 (three launches); read by the library per call."""
    if request.param == "se3":
        monkeypatch.setenv("HISEG_SE2", "0")
    else:
        monkeypatch.delenv("HISEG_SE2", raising=False)
    return request.param


# ------------------------------------------------------------------------------------------- 1. max-pool
# (N, H, W, nch): odd sizes drop the last row / column; 3 x 6 x 5 x 3 = 270 chunks span two blocks, the second partly
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("N,H,W,nch", [(2, 7, 5, 1), (2, 7, 5, 3), (3, 12, 10, 3), (1, 2, 2, 1)])
@pytest.mark.parametrize("negative", [True, False])
def test_maxpool2x2(dt, N, H, W, nch, negative):
    C = nch * CHUNK[dt]
    x = rnd(gen(1), dt, N, H, W, C)
    if negative:     # a running maximum that starts at zero would win everywhere
        x = (-0.5 - x.abs()).to(DTYPES[dt]).double()
        assert x.max() < 0
    out = Out(N, H // 2, W // 2, C, dtype=DTYPES[dt])
    ok(lib().hiseg_maxpool2x2_fwd(HD[dt], ptr(up(x, DTYPES[dt])), N, H, W, C, out.ptr(), stream()), "maxpool2x2")
    exact("maxpool2x2", dt, f"{N}x{H}x{W}x{C}", out.get(), O.maxpool2x2(x).to(DTYPES[dt]))


def test_maxpool2x2_refuses_one_row():
    x, out = up(torch.zeros(1, 1, 4, 4)), Out(8)
    refused(lib().hiseg_maxpool2x2_fwd(HD["f32"], ptr(x), 1, 1, 4, 4, out.ptr(), stream()), BAD_SHAPE, "maxpool2x2", out)


# ------------------------------------------------------------------------------------------- 2. spatial attention
# nch 1: 15 of the 16 lanes of a pixel idle; 16: one pass; 17: lane 0 makes a second pass.  2 x 2 x 3: every window is
# clipped on all sides and 16 P = 192 threads; 1 x 5 x 7: 16 P = 560, two full blocks and a part.
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("nch", [1, 16, 17])
@pytest.mark.parametrize("k", [3, 7])
@pytest.mark.parametrize("N,H,W", [(2, 2, 3), (1, 5, 7)])
def test_spatial_attention(dt, nch, k, N, H, W):
    g = gen(20 + nch + k)
    C, P = nch * CHUNK[dt], N * H * W
    x = rnd(g, dt, N, H, W, C)
    x[:, ::2, ::2] = (-1.0 - x[:, ::2, ::2].abs()).to(DTYPES[dt]).double()      # all-negative pixels: max_c < 0
    x[:, 0, 0, C - 1] = -0.25                                                   # the maximum in the last lane's chunk
    w = rnd(g, "f32", 2, k, k, scale=0.1)
    r64, r32 = both(O.attn_spatial, x, w)
    assert (r64["max"] < 0).any() and (r64["max"] > 0).any() and r64["arg"].abs().max() <= 16
    xd, wd = up(x, DTYPES[dt]), up(w)
    stats, att, ps = Out(P, 2), Out(P), Out(P, C, dtype=DTYPES[dt])
    ok(lib().hiseg_attn_map_fwd(HD[dt], ptr(xd), N, H, W, C, ptr(wd), k, stats.ptr(), att.ptr(), stream()), "attn_map")
    att_k = att.get()
    ok(lib().hiseg_pixel_scale_fwd(HD[dt], ptr(xd), P, C, att.ptr(), ps.ptr(), stream()), "pixel_scale")
    stats2, att2, sp = Out(P, 2), Out(P), Out(P, C, dtype=DTYPES[dt])
    ok(lib().hiseg_attn_spatial_fwd(HD[dt], ptr(xd), N, H, W, C, ptr(wd), k, stats2.ptr(), att2.ptr(), sp.ptr(), stream()),
       "attn_spatial")
    what = f"nch={nch} k={k} {N}x{H}x{W}"
    exact("attn_stats_max", dt, what, stats.get()[:, 1], r64["max"].float())
    check("attn_stats_mean", dt, what, stats.get()[:, 0], r64["mean"], r32["mean"])
    check("attn_map", dt, what, att_k, r64["att"], r32["att"], extra=dsig(r64["arg"]))
    exact("attn_spatial_att", dt, what, att2.get(), att_k)
    exact("attn_spatial_stats", dt, what, stats2.get(), stats.get())
    exact("attn_spatial_out", dt, what, sp.get(), ps.get())
    check("pixel_scale", dt, what, ps.get(), *both(O.pixel_scale, x, att_k.double().view(N, H, W)), out_mode(dt))
    check("attn_spatial", dt, what, sp.get(), r64["out"], r32["out"], out_mode(dt),
          extra=x.abs() * dsig(r64["arg"]).unsqueeze(-1))


def test_spatial_attention_refuses_even_kernel():
    x, w = up(torch.zeros(1, 2, 2, 4)), up(torch.zeros(2, 4, 4))
    stats, att, out = Out(8), Out(4), Out(16)
    refused(lib().hiseg_attn_map_fwd(HD["f32"], ptr(x), 1, 2, 2, 4, ptr(w), 4, stats.ptr(), att.ptr(), stream()),
            BAD_ARG, "attn_map", stats, att)
    refused(lib().hiseg_attn_spatial_fwd(HD["f32"], ptr(x), 1, 2, 2, 4, ptr(w), 4, stats.ptr(), att.ptr(), out.ptr(),
                                         stream()), BAD_ARG, "attn_spatial", stats, att, out)


# ------------------------------------------------------------------------------------------- 3. SqueezeExcite
def se_extra(r64, w2, act, beta):
    """The intrinsics' share of the gate's error: the hidden activation's, through |W2|, and the gate's own sigmoid."""
    s = r64["gate"]
    return s * (1 - s) * (dact(r64["z1"], act, beta) @ w2.abs().t()) + dsig(r64["z2"])


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", list(O.SE_CASES))
def test_se_gate(name, dt, se_mode):
    N, HW, C, Cr, act, beta, bias = O.SE_CASES[name]
    x, w1, b1, w2, b2 = O.se_inputs(name, dt)
    splits = lib().hiseg_gap_splits(HW)
    r64, r32 = both(lambda *a: O.se_gate(O.gap_partials(a[0], 1), HW, *a[1:], act, beta), x, w1, b1, w2, b2)
    xd, b1d, b2d = up(x, DTYPES[dt]), up(b1), up(b2)
    gates = {}
    for o1, o2 in ((0, 0), (1, 0), (0, 1), (1, 1)):     # W1 / W2 on and one float off a 16-byte boundary
        partial, gate = Out(N, splits, C), Out(N, C)
        w1d, w2d = up_offset(w1, o1), up_offset(w2, o2)
        ok(lib().hiseg_se_gate_fwd(HD[dt], ptr(xd), N, HW, C, ptr(w1d), ptr(b1d), Cr, ptr(w2d), ptr(b2d), act, beta,
                                   partial.ptr(), gate.ptr(), stream()), "se_gate")
        partial.get()
        gates[o1, o2] = gate.get()
    check("se_gate", dt, f"{name} {se_mode}", gates[0, 0], r64["gate"], r32["gate"], extra=se_extra(r64, w2, act, beta))
    for key in ((1, 0), (0, 1), (1, 1)):   # the vector and scalar instantiations are ordered identically
        exact("se_gate_alignment", dt, f"{name} {se_mode} offsets {key}", gates[key], gates[0, 0])


def test_se_gate_refuses_small_partial():
    N, HW, C, Cr = 1, 4, 8, 16           # splits * C = 8 < Cr: the hidden units do not fit the partial buffer
    x, w1, w2 = up(torch.zeros(N, HW, C)), up(torch.zeros(Cr, C)), up(torch.zeros(C, Cr))
    partial, gate = Out(N, 1, C), Out(N, C)
    st = lib().hiseg_se_gate_fwd(HD["f32"], ptr(x), N, HW, C, ptr(w1), None, Cr, ptr(w2), None, O.ACT_RELU, 1.0,
                                 partial.ptr(), gate.ptr(), stream())
    refused(st, BAD_SHAPE, "se_gate", partial, gate)


@pytest.mark.parametrize("name", list(O.SE_PARTIAL_CASES))
def test_se_gate_partials(name, se_mode):
    N, HW, C, Cr, act, beta, bias = O.SE_PARTIAL_CASES[name]
    splits = O.SE_PARTIAL_SPLITS[name]
    x, w1, b1, w2, b2 = O.se_inputs(name, "f32")
    part = O.gap_partials(x, splits).float().double()       # the kernel's input: float32 per-split sums
    r64, r32 = both(O.se_gate, part, HW, w1, b1, w2, b2, act, beta)
    assert O.se_inputs_ok(r64, beta)
    pd, gate = up(part), Out(N, C)
    ok(lib().hiseg_se_gate_partials_fwd(ptr(pd), splits, N, HW, C, ptr(up(w1)), ptr(up(b1)), Cr, ptr(up(w2)), ptr(up(b2)),
                                        act, gate.ptr(), stream()), "se_gate_partials")
    check("se_gate_partials", "f32", f"{name} {se_mode}", gate.get(), r64["gate"], r32["gate"],
          extra=se_extra(r64, w2, act, beta))


def test_se_gate_partials_refuses_swish():
    N, HW, C, Cr = 1, 4, 8, 4
    part, gate = Out(N, 1, C), Out(N, C)
    w1, w2 = up(torch.zeros(Cr, C)), up(torch.zeros(C, Cr))
    st = lib().hiseg_se_gate_partials_fwd(part.ptr(), 1, N, HW, C, ptr(w1), None, Cr, ptr(w2), None, O.ACT_SWISH,
                                          gate.ptr(), stream())
    refused(st, BAD_ARG, "se_gate_partials", part, gate)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("HW", [1, 35])
@pytest.mark.parametrize("nch", [1, 5])
def test_channel_scale(dt, HW, nch):
    g = gen(40 + HW + nch)
    N, C = 3, nch * CHUNK[dt]
    x = rnd(g, dt, N, HW, C)
    gate = torch.rand(N, C, generator=g, dtype=torch.float64).float().double()
    gate[torch.rand(N, C, generator=g) < 0.25] = 0.0
    gate[0, 0], gate[N - 1, C - 1] = 0.0, 1.0
    assert not torch.equal(gate[0], gate[1]) and not torch.equal(gate[1], gate[2])
    out = Out(N, HW, C, dtype=DTYPES[dt])
    ok(lib().hiseg_channel_scale_fwd(HD[dt], ptr(up(x, DTYPES[dt])), N, HW, C, ptr(up(gate)), out.ptr(), stream()),
       "channel_scale")
    check("channel_scale", dt, f"HW={HW} nch={nch}", out.get(), *both(O.channel_scale, x, gate), out_mode(dt))


def test_channel_scale_refuses_no_channels():
    x, gate, out = up(torch.zeros(8)), up(torch.zeros(8)), Out(8)
    refused(lib().hiseg_channel_scale_fwd(HD["f32"], ptr(x), 1, 2, 0, ptr(gate), out.ptr(), stream()), BAD_ARG,
            "channel_scale", out)


# ------------------------------------------------------------------------------------------- 4. input prologue
def image_max(xd, n):
    buf = Out(1)
    ok(lib().hiseg_image_max_fwd(xd.data_ptr(), n, buf.ptr(), stream()), "image_max")
    return O.key_to_bits(buf.get().view(torch.int32).item() & 0xFFFFFFFF), buf      # the buffer holds the ordered key


# n 1, 3: tail only; 5: one 16-byte load and a tail; 1027: more than one block.  offset 1: the scalar fallback.
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 5, 1027])
def test_image_max(n, offset):
    x = -1.0 - torch.randn(n, generator=gen(50 + n)).abs()       # all negative
    places = sorted({n - 1, 0, (n // 4) * 4 - 1 if n >= 4 else 0})     # the last tail element; the vector body
    for place in [None] + places:
        for top in (-0.5, 3.25):
            v = x.clone()
            if place is not None:
                v[place] = top
            bits, _ = image_max(up_offset(v, offset), n)
            assert bits == O.image_max_bits(v), f"n={n} offset={offset} max at {place}: {bits:#x}"
    for zeros, want in (((-0.0,), 0x80000000), ((-0.0, 0.0), 0), ((0.0, -0.0), 0)):     # -0.0 is below +0.0
        if n >= len(zeros):
            v = x.clone()
            v[n - 1] = zeros[0]
            v[0] = zeros[-1]
            bits, _ = image_max(up_offset(v, offset), n)
            assert bits == O.image_max_bits(v) == want, f"n={n} offset={offset} zeros {zeros}: {bits:#x}"
    RATIOS.setdefault(("image_max", "f32"), 0.0)


def test_image_max_four_in_flight():
    """The grid is capped at 2048 blocks; past n / 4 > 3 * 2048 * 256 the first threads take the loop with four
    16-byte loads in flight.  The maximum is placed once in each of the four strided loads, in the single-load loop
    and in the tail."""
    stride, gid = 2048 * 256, 5
    n = 4 * (3 * stride + 1000) + 3
    xd = torch.full((n,), -2.0, device=DEV)
    places = [4 * (gid + j * stride) + (j + 1) % 4 for j in range(4)] + [4 * (1500 + 2 * stride) + 2, n - 1]
    for i, p in enumerate(places):
        xd[p] = 1.0 + i
        bits, _ = image_max(xd, n)
        assert bits == O.image_max_bits(torch.tensor([1.0 + i])), f"maximum at {p}: {bits:#x}"
        xd[p] = -2.0
    bits, _ = image_max(xd, n)
    assert bits == O.image_max_bits(torch.tensor([-2.0]))


NEXT_AFTER_ONE = float(torch.nextafter(torch.tensor(1.0), torch.tensor(2.0)))


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("top", [1.0, NEXT_AFTER_ONE, 200.0])
@pytest.mark.parametrize("cpad", [3, 8])
def test_input_norm(dt, top, cpad):
    g = gen(60)
    B, C, H, W = 2, 3, 5, 7
    x = (torch.rand(B, C, H, W, generator=g, dtype=torch.float64) * 0.9 * min(top, 200.0)).float().double()
    x[1, 2, 3, 4] = top
    assert x.max() == top
    mean = torch.tensor([0.485, 0.456, 0.406]).double()
    std = torch.tensor([0.229, 0.224, 0.225]).double()
    xd = up(x)
    bits, mbuf = image_max(xd, x.numel())
    assert bits == O.image_max_bits(x.float())
    out = Out(B, H, W, cpad, dtype=DTYPES[dt])
    ok(lib().hiseg_input_norm_fwd(HD[dt], ptr(xd), B, C, H, W, mbuf.ptr(), ptr(up(mean)), ptr(up(std)), out.ptr(), cpad,
                                  stream()), "input_norm")
    k = out.get()
    r64, r32 = both(O.input_norm, x, mean, std, cpad)
    assert bool((k[..., C:] == 0).all()), "padding channels are not zero"
    check("input_norm", dt, f"top={top} cpad={cpad}", k, r64, r32, out_mode(dt))


def test_input_norm_refusals():
    x, m, out = up(torch.zeros(1, 3, 2, 2)), up(torch.ones(3)), Out(12)
    args = lambda C, H, W, cpad: (HD["f32"], ptr(x), 1, C, H, W, ptr(m), ptr(m), ptr(m), out.ptr(), cpad, stream())
    refused(lib().hiseg_input_norm_fwd(*args(3, 2, 2, 2)), BAD_ARG, "input_norm", out)      # cpad < C
    refused(lib().hiseg_input_norm_fwd(*args(3, 0, 2, 3)), BAD_ARG, "input_norm", out)      # no pixels: an empty grid


# ------------------------------------------------------------------------------------------- 5. hierarchical head
ACTS = {"none": (O.ACT_NONE, 1.0), "relu": (O.ACT_RELU, 1.0), "silu": (O.ACT_SILU, 1.0), "swish": (O.ACT_SWISH, 1.5)}


def head_inputs(dt, N, h, w, Ct, per_sample, seed=70):
    g = gen(seed)
    c = dict(low=rnd(g, "f32", N, h, w, 2), tfeat=rnd(g, dt, N, 2 * h, 2 * w, Ct), ut_w=rnd(g, "f32", 2, 32, 2, 2, scale=0.5),
             scale=rnd(g, "f32", *((N, 32) if per_sample else (32,)), scale=0.3, shift=1.0),
             shift=rnd(g, "f32", *((N, 32) if per_sample else (32,)), scale=0.3),
             u1_w=rnd(g, "f32", 2, 32, scale=0.3), u1_b=rnd(g, "f32", 2, scale=0.3),
             t_w=rnd(g, "f32", 2, Ct, scale=1.0 / Ct ** 0.5), t_b=rnd(g, "f32", 2, scale=0.3))
    if per_sample:
        assert not torch.equal(c["scale"][0], c["scale"][1]) and not torch.equal(c["shift"][1], c["shift"][2])
    return c


def head_check(kernel, dt, what, r64, r32, u1_w, act, beta, logits, bgfg, tn):
    assert r64["d"].abs().max() <= 16
    ex_b = torch.einsum("kc,nchw->nkhw", u1_w.abs(), dact(r64["pre"], act, beta))       # [N, 2, H, W]
    ex_p = dsig(r64["d"]) + 0.25 * (ex_b[:, 0] + ex_b[:, 1])
    t = r64["tn"]
    ex_l = torch.stack([ex_b[:, 0], ex_b[:, 1] + t[:, 0].abs() * ex_p, ex_b[:, 1] + t[:, 1].abs() * ex_p], dim=1)
    check(kernel, dt, what + " logits", logits.get(), r64["logits"], r32["logits"], extra=ex_l)
    if bgfg is not None:
        check(kernel, dt, what + " bgfg", bgfg.get(), r64["bgfg"], r32["bgfg"], extra=ex_b)
    if tn is not None:
        check(kernel, dt, what + " tn", tn.get(), r64["tn"], r32["tn"])


# 3 x 5 low pixels: all four output parities next to every border; Ct of one chunk and of the LDS table's 512
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("chunks", [1, 0])
@pytest.mark.parametrize("per_sample", [0, 1])
@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("aux", [False, True])
def test_hier_combine(dt, chunks, per_sample, act, aux):
    N, h, w = 3, 3, 5
    Ct = chunks * CHUNK[dt] if chunks else 512
    code, beta = ACTS[act]
    c = head_inputs(dt, N, h, w, Ct, per_sample)
    r64, r32 = both(O.hier_combine, c["low"], c["tfeat"], None, c["ut_w"], c["scale"], c["shift"], code, beta, c["u1_w"],
                    c["u1_b"], c["t_w"], c["t_b"])
    logits = Out(N, 3, 2 * h, 2 * w)
    bgfg, tn = (Out(N, 2, 2 * h, 2 * w), Out(N, 2, 2 * h, 2 * w)) if aux else (None, None)
    d = {k: up(v) for k, v in c.items() if k != "tfeat"}
    tf = up(c["tfeat"], DTYPES[dt])
    ok(lib().hiseg_hier_combine_fwd(HD[dt], ptr(d["low"]), N, h, w, ptr(tf), Ct, ptr(d["ut_w"]), ptr(d["scale"]),
                                    ptr(d["shift"]), code, beta, per_sample, ptr(d["u1_w"]), ptr(d["u1_b"]), ptr(d["t_w"]),
                                    ptr(d["t_b"]), logits.ptr(), bgfg and bgfg.ptr(), tn and tn.ptr(), stream()),
       "hier_combine")
    head_check("hier_combine", dt, f"Ct={Ct} ps={per_sample} {act}", r64, r32, c["u1_w"], code, beta, logits, bgfg, tn)


def test_hier_combine_edges():
    N, h, w, Ct = 3, 5, 7, 8                         # 420 output pixels: two blocks
    c = head_inputs("f32", N, h, w, Ct, 1, seed=71)
    d = {k: up(v) for k, v in c.items()}
    code, beta = ACTS["silu"]

    def call(n, ct, logits):
        return lib().hiseg_hier_combine_fwd(HD["f32"], ptr(d["low"]), n, h, w, ptr(d["tfeat"]), ct, ptr(d["ut_w"]),
                                            ptr(d["scale"]), ptr(d["shift"]), code, beta, 1, ptr(d["u1_w"]), ptr(d["u1_b"]),
                                            ptr(d["t_w"]), ptr(d["t_b"]), logits.ptr(), None, None, stream())
    logits = Out(N, 3, 2 * h, 2 * w)
    ok(call(N, Ct, logits), "hier_combine")
    r64, r32 = both(O.hier_combine, c["low"], c["tfeat"], None, c["ut_w"], c["scale"], c["shift"], code, beta, c["u1_w"],
                    c["u1_b"], c["t_w"], c["t_b"])
    head_check("hier_combine", "f32", "two blocks", r64, r32, c["u1_w"], code, beta, logits, None, None)
    empty = Out(N, 3, 2 * h, 2 * w)
    assert call(0, Ct, empty) == OK and empty.untouched()                   # N = 0: nothing to do
    refused(call(N, 516, empty), BAD_SHAPE, "hier_combine", empty)         # past the 512-channel LDS table


@pytest.mark.parametrize("per_sample", [0, 1])
@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("aux", [False, True])
def test_hier_combine_tn(per_sample, act, aux):
    N, h, w = 3, 3, 5
    code, beta = ACTS[act]
    c = head_inputs("f32", N, h, w, 8, per_sample, seed=72)
    tn2 = O.hier_combine(c["low"], c["tfeat"], None, c["ut_w"], c["scale"], c["shift"], code, beta, c["u1_w"], c["u1_b"],
                         c["t_w"], c["t_b"])["tn"].permute(0, 2, 3, 1).float().double().contiguous()
    r64, r32 = both(O.hier_combine, c["low"], None, tn2, c["ut_w"], c["scale"], c["shift"], code, beta, c["u1_w"],
                    c["u1_b"], None, None)
    d = {k: up(v) for k, v in c.items()}
    tnd = up_offset(tn2, 0)

    def call(tn_ptr, logits, bgfg, tn):
        return lib().hiseg_hier_combine_tn_fwd(ptr(d["low"]), N, h, w, tn_ptr, ptr(d["ut_w"]), ptr(d["scale"]),
                                               ptr(d["shift"]), code, beta, per_sample, ptr(d["u1_w"]), ptr(d["u1_b"]),
                                               logits.ptr(), bgfg and bgfg.ptr(), tn and tn.ptr(), stream())
    logits = Out(N, 3, 2 * h, 2 * w)
    bgfg, tn = (Out(N, 2, 2 * h, 2 * w), Out(N, 2, 2 * h, 2 * w)) if aux else (None, None)
    ok(call(ptr(tnd), logits, bgfg, tn), "hier_combine_tn")
    head_check("hier_combine_tn", "f32", f"ps={per_sample} {act}", r64, r32, c["u1_w"], code, beta, logits, bgfg, tn)
    if tn is not None:
        exact("hier_combine_tn_copy", "f32", "tn", tn.get(), r64["tn"].float())
    fresh = Out(N, 3, 2 * h, 2 * w)
    refused(call(ptr(tnd) + 4, fresh, None, None), BAD_SHAPE, "hier_combine_tn", fresh)     # float2 loads: 8-byte aligned


# h * w of 1 and 3: fewer low pixels than the 8 pixel rows of a block; 21 = 8 * 2 + 5: a remainder
LN_NULLS = ["all", "no_ut_b", "no_affine", "no_stats"]
LN_CASES = [(hw, fold, nulls, "random") for hw in ((1, 1), (1, 3), (3, 7)) for fold in (0, 1) for nulls in LN_NULLS]
LN_CASES += [((3, 7), fold, "all", kind) for fold in (0, 1) for kind in ("constant", "offset")]


@pytest.mark.parametrize("hw,fold,nulls,kind", LN_CASES)
def test_ubf_ln_tables(hw, fold, nulls, kind):
    g = gen(80)
    (h, w), N, eps = hw, 3, 1e-5
    low, ut_w = rnd(g, "f32", N, h, w, 2), rnd(g, "f32", 2, 32, 2, 2, scale=0.5)
    ut_b = None if nulls == "no_ut_b" else rnd(g, "f32", 32, scale=0.5)
    gamma, beta = (None, None) if nulls == "no_affine" else (rnd(g, "f32", 32, shift=1.0, scale=0.3), rnd(g, "f32", 32))
    if kind == "constant":       # every z equal: the variance clamps at zero and invstd = 1 / sqrt(eps)
        low, ut_b = torch.zeros_like(low), torch.full((32,), 0.3).double()
    if kind == "offset":         # mean 50, spread 0.01
        low, ut_b = (0.01 * low).float().double(), torch.full((32,), 50.0).double()
    r64, r32 = both(O.ubf_ln_tables, low, ut_w, ut_b, gamma, beta, eps, fold)
    if kind == "constant":
        assert (r64["invstd"] * eps ** 0.5 - 1).abs().max() < 1e-9
    mean, inv = (None, None) if nulls == "no_stats" else (Out(N), Out(N))
    scale, shift = Out(N, 32), Out(N, 32)
    ok(lib().hiseg_ubf_ln_tables(ptr(up(low)), N, h, w, ptr(up(ut_w)), ptr(up(ut_b)), ptr(up(gamma)), ptr(up(beta)), eps,
                                 fold, mean and mean.ptr(), inv and inv.ptr(), scale.ptr(), shift.ptr(), stream()),
       "ubf_ln_tables")
    what = f"{h}x{w} fold={fold} {nulls} {kind}"
    check("ubf_ln_tables", "f32", what + " scale", scale.get(), r64["scale"], r32["scale"])
    check("ubf_ln_tables", "f32", what + " shift", shift.get(), r64["shift"], r32["shift"])
    if mean is not None:
        check("ubf_ln_tables", "f32", what + " mean", mean.get(), r64["mean"], r32["mean"])
        check("ubf_ln_tables", "f32", what + " invstd", inv.get(), r64["invstd"], r32["invstd"])


# ------------------------------------------------------------------------------------------- 6. layout
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("cpad", [5, 8])
def test_nchw_to_nhwc(dt, cpad):
    N, C, H, W = 2, 5, 11, 13                                    # 286 pixels: two blocks
    x = torch.randn(N, C, H, W, generator=gen(90))              # float32 in, rounded by the kernel
    xd = up(x)
    out = Out(N, H, W, cpad, dtype=DTYPES[dt])
    ok(lib().hiseg_nchw_to_nhwc_fwd(HD[dt], ptr(xd), N, C, H, W, out.ptr(), cpad, stream()), "nchw_to_nhwc")
    exact("nchw_to_nhwc", dt, f"cpad={cpad}", out.get(), O.nchw_to_nhwc(x, cpad).to(DTYPES[dt]))
    empty = Out(8, dtype=DTYPES[dt])
    assert lib().hiseg_nchw_to_nhwc_fwd(HD[dt], ptr(xd), 0, C, H, W, empty.ptr(), cpad, stream()) == OK and empty.untouched()
    refused(lib().hiseg_nchw_to_nhwc_fwd(HD[dt], ptr(xd), N, C, H, W, empty.ptr(), C - 1, stream()), BAD_ARG,
            "nchw_to_nhwc", empty)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("cstride,coff", [(5, 0), (16, 3), (16, 8), (8, 3)])
def test_nhwc_to_nchw(dt, cstride, coff):
    N, C, H, W = 2, 5, 5, 7                                      # 350 outputs: two blocks
    buf = rnd(gen(91), dt, N, H, W, cstride)
    bd = up(buf, DTYPES[dt])
    out = Out(N, C, H, W)
    ok(lib().hiseg_nhwc_to_nchw_fwd(HD[dt], ptr(bd), N, H, W, C, cstride, coff, out.ptr(), stream()), "nhwc_to_nchw")
    exact("nhwc_to_nchw", dt, f"cstride={cstride} coff={coff}", out.get(), O.nhwc_to_nchw(buf, C, coff).float())
    empty = Out(8)
    assert lib().hiseg_nhwc_to_nchw_fwd(HD[dt], ptr(bd), 0, H, W, C, cstride, coff, empty.ptr(), stream()) == OK
    assert empty.untouched()
    for bad_stride, bad_off in ((coff + C - 1, coff), (cstride, -1)):      # the slice leaves the pixel's channels
        refused(lib().hiseg_nhwc_to_nchw_fwd(HD[dt], ptr(bd), N, H, W, C, bad_stride, bad_off, empty.ptr(), stream()),
                BAD_ARG, "nhwc_to_nchw", empty)


# ------------------------------------------------------------------------------------------- 7. export masks
def run_instance_masks(lg, dil):
    N, _, mh, mw = lg.shape
    out = Out(N, 1, mh, mw)
    ok(lib().hiseg_instance_masks_fwd(ptr(up(lg)), N, mh, mw, dil, out.ptr(), stream()), "instance_masks")
    return out.get()


@pytest.mark.parametrize("N,mh,mw,dil", O.INSTANCE_CASES)
def test_instance_masks(N, mh, mw, dil):
    lg = O.instance_logits(N, mh, mw, dil)         # margins asserted in tests/test_infer_kernel_oracle.py
    k = run_instance_masks(lg, dil)
    exact("instance_masks", "f32", f"dilation {dil}", k, R.instance_masks(lg, dil).float())
    exact("instance_masks", "f32", f"dilation {dil}", k, O.instance_masks(lg, dil)["inst"].float())


def test_instance_masks_ties():
    lg = O.instance_tie_logits()
    k = run_instance_masks(lg, 0)
    assert k[0, 0, 0, 0] == 0 and k[0, 0, 0, 1] == 1          # l0 == l1 -> class 0; l1 == l2 -> class 1
    exact("instance_masks", "f32", "ties", k, R.instance_masks(lg, 0).float())


@pytest.mark.parametrize("cs", [1, 3])
def test_binary_masks(cs):
    g = gen(100)
    B, H, W = 2, 11, 13
    u = rnd(g, "f32", B, H, W, cs).clamp(-3.5, 3.5)
    w, b = rnd(g, "f32", 2).clamp(-1.5, 1.5), rnd(g, "f32", 2, scale=0.5)
    r64, r32 = both(O.binary_masks, u[..., 0], w, b)
    out = Out(B, 1, H, W)
    args = (ptr(up(u)), cs, B, H, W, ptr(up(w)), ptr(up(b)), out.ptr(), stream())
    ok(lib().hiseg_binary_masks_fwd(HD["f32"], *args), "binary_masks")
    check("binary_masks", "f32", f"cstride {cs}", out.get(), r64["binary"], r32["binary"], extra=dsig(r64["d"]))
    fresh = Out(B, 1, H, W)
    refused(lib().hiseg_binary_masks_fwd(HD["bf16"], *args[:7], fresh.ptr(), stream()), BAD_DTYPE, "binary_masks", fresh)


def test_output_conv():
    g = gen(101)
    B, H, W = 3, 11, 13
    u, w, b = rnd(g, "f32", B, H, W, scale=2.0), rnd(g, "f32", 2), rnd(g, "f32", 2)
    out = Out(B, 2, H, W)
    ok(lib().hiseg_output_conv_fwd(ptr(up(u)), B, H, W, ptr(up(w)), ptr(up(b)), out.ptr(), stream()), "output_conv")
    check("output_conv", "f32", "", out.get(), *both(O.output_conv, u, w, b))


def test_distance_mask():
    g = gen(102)
    n = 300
    thr = torch.tensor([0.125]).double()
    x = (thr + 1.5 * (2 * torch.rand(n, generator=g, dtype=torch.float64) - 1)).float().double()    # |arg| <= 15
    r64, r32 = both(O.distance_mask, x, thr)
    out = Out(n)
    ok(lib().hiseg_distance_mask_fwd(ptr(up(x)), n, ptr(up(thr)), out.ptr(), stream()), "distance_mask")
    check("distance_mask", "f32", "", out.get(), r64["mask"], r32["mask"], extra=dsig(r64["arg"]))
    empty = Out(8)
    assert lib().hiseg_distance_mask_fwd(ptr(up(x)), 0, ptr(up(thr)), empty.ptr(), stream()) == OK and empty.untouched()


# H = 1 / W = 1: the +1 neighbour clamps; Ho = 1; 7 x 9 -> 3 x 4: a non-integer downscale
@pytest.mark.parametrize("H,W,Ho,Wo", [(1, 6, 3, 9), (5, 1, 7, 2), (4, 6, 1, 3), (7, 9, 3, 4)])
def test_resize_bilinear_fwd(H, W, Ho, Wo):
    NC = 3
    x = rnd(gen(103), "f32", NC, H, W)
    out = Out(NC, Ho, Wo)
    ok(lib().hiseg_resize_bilinear_fwd(ptr(up(x)), NC, H, W, out.ptr(), Ho, Wo, stream()), "resize_bilinear")
    check("resize_bilinear_fwd", "f32", f"{H}x{W}->{Ho}x{Wo}", out.get(), *both(O.resize_bilinear, x, Ho, Wo))
