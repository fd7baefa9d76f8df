"""Every forward convolution kernel behind hiseg_conv2d_fwd on its own against the float64 oracle of
tests/conv_kernel_oracle.py, through hiseg.ops.conv2d(..., variant=v), with the path the library reports
(hiseg._lib.conv_last_path) asserted after every call: a forced variant that declines the layer falls through to the
generic kernel, and without the path such a run compares the generic kernel with itself.

Every run pre-fills `out` / `out2` with the sentinel -7.5 behind a 64-element guard tail and afterwards requires the
pad channels, the untouched part of an offset view and the tail to still hold it.

Tier A, exact.  Activations, weights, residual and mul are integers in {-2..2}, shift integers, scale from
{+-0.5, +-1, +-2}, gates from {0.5, 1, 2}, the activation none or ReLU: every partial sum in any order is exactly
representable in float32 (conv_kernel_oracle.make_inputs; tests/test_conv_kernel_oracle.py proves the premise per case),
so the kernel equals the oracle bit for bit -- f32 outputs the exact value, bf16 outputs torch's round-to-nearest-even
of it.  A dropped or doubled tap, channel, halo row, tile edge or K tail changes an integer and cannot hide.

Tier B, rounding.  Normal inputs rounded to the compute dtype, weights scaled by 1 / sqrt(K), gates of 8 significant
bits.  The bound is the rule of tests/test_gpu_infer_kernels.py: |k - ref| <= 4 max(e32) + 4 * 2^-23 max|ref| with
e32 torch's float32 evaluation of the oracle, + 2^-8 |ref| for a bf16 output written once, + the sigmoid intrinsic's
dsig term derived in that file's docstring for sigmoid / SiLU / Swish epilogues (times |mul|).

Worst observed error / bound per kernel family, compute dtype and output dtype in tier B
(profiles/conv_kernel_errors.txt; tier A is bit for bit everywhere):

  family           compute  output  ratio
  fast             bf16     bf16    0.993
  generic          bf16     bf16    0.994
  generic          bf16     f32     0.315
  generic          f32      bf16    0.993
  generic          f32      f32     0.496
  generic_splitk   bf16     bf16    0.993
  hw               bf16     bf16    0.995
  hwc              bf16     bf16    0.995
  hwr              bf16     bf16    0.993
  hwt              bf16     bf16    0.993
  pw               bf16     bf16    0.994
  rows             bf16     bf16    0.993
  rows             bf16     f32     0.097
  small            bf16     bf16    0.995
  small            bf16     f32     0.106
  wide             bf16     bf16    0.992
  hwc_stats        bf16     f32     0.127   (the fused statistics of variants 104 / 107, both tiers)
  hwc_bnb          bf16     f32     0.017   (their BatchNorm-backward sums)
  (MI355X.  A bf16 output written once sits near 1.0 by construction: 2^-8 |ref| is exactly the worst case of one
  round-to-nearest to bf16, so those rows say nothing about the arithmetic's margin.  The f32-output rows do: only
  the generic, small and rows kernels store f32, and there the 4 max(e32) + 4 * 2^-23 max|ref| term alone holds with
  a factor of two to ten to spare.  The other families write bf16 only; their accumulation is measured by tier A,
  bit for bit.  No family needed the derived (K + 8) 2^-23 S term.)
"""
import ctypes
import functools
import os

import pytest
import torch

import conv_kernel_oracle as O
from hiseg import _lib as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -7.5          # exact in bf16; tier A outputs are multiples of 1/4
GUARD = 64
RATIOS = {}
CHUNK = {"f32": 4, "bf16": 8}


def rup(x, m):
    return (x + m - 1) // m * m


# ------------------------------------------------------------------------------------------- plumbing
def to_act(x, dt, cread, view=None):
    """NCHW float64 -> an NHWC Act whose buffer holds the sentinel outside the `cread` channels the layer reads (the
    real ones, then zero pads) and in a guard tail."""
    from hiseg import ops
    N, C, H, W = x.shape
    cs, coff = view or (cread, 0)
    n = N * H * W * cs
    buf = torch.full((n + GUARD,), SENTINEL, dtype=torch.float64)
    v = buf[:n].view(N, H, W, cs)
    v[..., coff:coff + cread] = 0
    v[..., coff:coff + C] = x.permute(0, 2, 3, 1)
    return ops.Act(buf.to(O.DTYPES[dt]).to(DEV), N, H, W, C, cs, coff)


class OutBuf:
    """A sentinel-filled output view with a guard tail."""

    def __init__(self, N, H, W, C, dt, view=None):
        from hiseg import ops
        self.dims = (N, H, W, C)
        self.cs, self.coff = view or (rup(C, CHUNK[dt]), 0)
        self.n = N * H * W * self.cs
        self.act = ops.Act(torch.full((self.n + GUARD,), SENTINEL, dtype=O.DTYPES[dt], device=DEV), N, H, W, C,
                           self.cs, self.coff)

    def get(self, what):
        """The real channels as NCHW; everything else must still be the sentinel."""
        torch.cuda.synchronize()
        N, H, W, C = self.dims
        host = self.act.t.cpu()
        assert bool((host[self.n:] == SENTINEL).all()), f"{what}: a store past the end of the buffer"
        body = host[:self.n].view(N, H, W, self.cs)
        rest = torch.ones(self.cs, dtype=torch.bool)
        rest[self.coff:self.coff + C] = False
        assert bool((body[..., rest] == SENTINEL).all()), f"{what}: a store outside the view's {C} channels"
        return body[..., self.coff:self.coff + C].permute(0, 3, 1, 2).contiguous()


@functools.lru_cache(maxsize=None)
def reference(key, tier, dt, out_dt):
    """(case, tensors, float64 result, float32 result) of a case, computed once and shared."""
    c, t = O.make_inputs(dict(key), tier, dt)
    r64 = O.run(c, t, dt, out_dt)
    r32 = O.run(c, t, dt, out_dt, compute=torch.float32) if tier == "B" else None
    return c, t, r64, r32


def plan_for(c, t, dt):
    from hiseg import ops
    act = L.ActCode(O.ACT_SWISH, c["beta"]) if c["act"] == O.ACT_SWISH else c["act"]
    if c["convT"]:
        p = ops.pack_convT2x2(t["w"].float(), None, None, act, O.DTYPES[dt], DEV)
        rep = 4
    else:
        p = ops.pack_conv(t["w"].float(), None, None, act, O.DTYPES[dt], DEV, stride=c["stride"], pad=c["pad"],
                          split=(c["Ca"], c["Cb"]) if c["Cb"] else None)
        rep = 1
    cols = rep * c["Cout"]
    p.scale[:cols] = t["scale"].float().repeat(rep).to(DEV)     # written after packing: any per-channel table
    p.shift[:cols] = t["shift"].float().repeat(rep).to(DEV)
    if c.get("no_frag"):
        p.weight_frag = None
    return p


def launch(case, variant, tier, dt="bf16", out_dt=None, fused=None):
    """Run the case on the GPU; returns (c, t, r64, r32, out NCHW, out2 NCHW or None, path) -- with `fused`
    ("stats" / "bnb": the fused-statistics forms, launch_fused) an eighth entry, what launch_fused returns."""
    from hiseg import ops
    key = tuple(sorted(case.items()))
    out_dt = out_dt or dt
    c, t, r64, r32 = reference(key, tier, dt, out_dt)
    p = plan_for(c, t, dt)
    xa = to_act(t["xa"], dt, p.ca, c["a_view"])
    xb = to_act(t["xb"], dt, p.cb) if c["Cb"] else None
    gate = None
    if t["gate"] is not None:
        gate = torch.ones(c["N"], p.ca)
        gate[:, :c["Ca"]] = t["gate"].float()
        gate = gate.to(DEV)
    N, Co, oH, oW = r64["v"].shape
    R = to_act(t["residual"], dt, rup(Co, CHUNK[dt])) if c["residual"] else None
    M = to_act(t["mul"], dt, rup(Co, CHUNK[dt])) if c["mul"] else None
    out = OutBuf(N, oH, oW, Co, out_dt, c["out_view"])
    out2 = OutBuf(N, oH, oW, Co, dt) if c["out2"] else None
    kw = dict(a_up=c["a_up"], residual=R, mul=M, out2=out2.act if out2 else None, in_scale=gate,
              split_k_3x3=c["split_k_3x3"])
    what = f"{case} variant {variant} tier {tier} {dt}->{out_dt}"
    if fused:
        extra = launch_fused(fused, p, xa, xb, out, variant, kw, what)
        return c, t, r64, r32, out.get(what), None, L.conv_last_path(), extra
    ops.conv2d(p, xa, xb, out.act, variant=variant, **kw)
    torch.cuda.synchronize()
    path = L.conv_last_path()
    return c, t, r64, r32, out.get(what), out2.get(what + " out2") if out2 else None, path


def stat_tables(C, seed):
    """The BatchNorm whose backward reduction the bnb form computes: its input z (integers), its folded affine and its
    batch statistics, all such that z * scale + shift and xhat = (z - mean) * invstd are exact in float32 (fused or
    not), so the ReLU mask and xhat are the same numbers on both sides and only the sums round."""
    g = O.gen(seed)
    return {"scale": O.pick(g, O.TIER_A_SCALES, C), "shift": O.ints(g, C, lo=-3, hi=3) + 0.5,
            "mean": O.ints(g, C, lo=-1, hi=1) * 0.5, "invstd": O.pick(g, (0.5, 1.0, 2.0), C)}


def launch_fused(kind, p, xa, xb, out, variant, kw, what):
    """The fused-statistics forms of conv_hwc (hiseg_conv2d_desc.stats_partial / bnb_partial, include/hiseg.h) have no
    hiseg.ops.conv2d argument -- the train engine fills the descriptor itself -- so: the descriptor ops.conv2d builds
    for the layer (ops.RECORD, from a run of the generic kernel), the partials buffer added, through the C entry.
    Returns (partials [S][3][Cout] float64, z NCHW float64 or None, the tables or None)."""
    from hiseg import ops
    ops.RECORD = rec = []
    try:
        ops.conv2d(p, xa, xb, out.act, variant=-1, **kw)
    finally:
        ops.RECORD = None
    torch.cuda.synchronize()
    out.act.t.fill_(SENTINEL)
    d = rec[0][0]
    N, H, W, C = out.dims
    z = tab = None
    if kind == "bnb":
        tab = stat_tables(C, 7)
        z = O.ints(O.gen(8), N, C, H, W)
        zact = to_act(z, "bf16", C)
        d.bnb_z, d.bnb_z_cstride, d.bnb_z_coff = zact, C, 0
        for f in ("scale", "shift", "mean", "invstd"):
            setattr(d, "bnb_" + f, tab[f].float().to(DEV))
        d.bnb_act = O.ACT_RELU
        d.bnb_partial = zact     # (any buffer: hiseg_conv2d_stats_tiles asks for the bnb form when it is set)
    tiles = L.lib().hiseg_conv2d_stats_tiles(ctypes.byref(d))
    tw = 16 if C % 128 == 0 else 32    # conv_hwc_stats_tiles: (16 x tw pixel tile, wave) splits, four waves
    assert tiles == N * ((H + 15) // 16) * ((W + tw - 1) // tw) * 4, f"{what}: {tiles} statistics splits"
    part = torch.full((tiles * 3 * C + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    setattr(d, "bnb_partial" if kind == "bnb" else "stats_partial", part)
    if variant:
        L.check(L.lib().hiseg_conv2d_fwd_variant(ctypes.byref(d), variant, L.stream_ptr()), "conv2d")
    else:
        L.check(L.lib().hiseg_conv2d_fwd(ctypes.byref(d), L.stream_ptr()), "conv2d")
    torch.cuda.synchronize()
    host = part.cpu()
    assert bool((host[tiles * 3 * C:] == SENTINEL).all()), f"{what}: a store past the end of the partials"
    return host[:tiles * 3 * C].view(tiles, 3, C).double(), z, tab


def dexp(x):
    return 1.25 * 2.0 ** -24 * x.abs() + 2.0 ** -23


def dsig(x):
    """The absolute error bound of sigmoidf_(x) derived in tests/test_gpu_infer_kernels.py (|x| <= 16)."""
    assert x.abs().max() <= 16
    s = torch.sigmoid(x)
    return s * (1 - s) * dexp(x) + 1.5 * 2.0 ** -23 * s


def check_b(family, dt, what, k, r64, r32, c, t, once):
    ref, e32 = r64["v"], (r32["v"].double() - r64["v"]).abs().max()
    bound = (4 * e32 + 4 * 2.0 ** -23 * ref.abs().max()).expand_as(ref)
    if once:
        bound = bound + 2.0 ** -8 * ref.abs()
    pre = r64["pre"]
    if c["act"] in (O.ACT_SIGMOID, O.ACT_SILU, O.ACT_SWISH):
        d = dsig(pre) if c["act"] == O.ACT_SIGMOID else pre.abs() * dsig((c["beta"] if c["act"] == O.ACT_SWISH else 1.0) * pre)
        bound = bound + d * (t["mul"].abs() if c["mul"] else 1.0)
    err = (k.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300)).max().item()
    key = (family, dt, "bf16" if once else "f32")   # (an f32 output measures the arithmetic alone)
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    print(f"{family} {dt} {what}: max err {err.max().item():.3e} ratio {ratio:.3f}")
    assert ratio <= 1.0, f"{family} {dt} {what}: error / bound = {ratio:.3f} (max err {err.max().item():.3e})"


def bits(x):
    return x.reshape(-1).clone().view(torch.uint8)


def check(case, variant, expect, dt="bf16", out_dt=None, tiers="AB"):
    """Both tiers of one (case, variant): the reported path, then tier A bit for bit and tier B within the bound.
    `expect`: (family, variant) or a family name alone."""
    case = dict(case)
    out_dt = out_dt or ("f32" if case.pop("f32_out", False) else dt)
    for tier in tiers:
        if tier == "A" and case.get("act", O.ACT_NONE) not in (O.ACT_NONE, O.ACT_RELU):
            continue   # (tier A needs an exact activation)
        c, t, r64, r32, y, y2, path = launch(case, variant, tier, dt, out_dt)
        what = f"{case} variant {variant} tier {tier} {dt}->{out_dt}"
        assert path is not None and (path == expect or path[0] == expect), f"{what}: ran {path}, expected {expect}"
        if tier == "A":
            assert r64["S"].max() < 2 ** 22
            assert torch.equal(bits(y), bits(r64["out"])), \
                f"{what} {path}: {(y != r64['out']).sum().item()} of {y.numel()} outputs differ from the exact value"
            if y2 is not None:
                assert torch.equal(bits(y2), bits(r64["out2"])), f"{what}: out2 differs"
        else:
            check_b(path[0], dt, what, y, r64, r32, c, t, out_dt == "bf16")
            if y2 is not None:
                check_b(path[0], dt, what + " out2", y2, r64, r32, c, t, dt == "bf16")


@pytest.fixture(scope="module", autouse=True)
def ratio_report():
    yield
    path = os.environ.get("HISEG_CONV_KERNEL_ERRORS")
    if path:
        with open(path, "w") as f:
            f.write("# worst |kernel - float64 oracle| / bound per forward conv kernel family, compute dtype and output\n"
                    "# dtype, tier B (tests/test_gpu_conv_kernels.py); tier A is bit for bit.  hwc_stats / hwc_bnb: the\n"
                    "# fused statistics of variants 104 / 107 against float64 sums, both tiers\n")
            for (fam, dt, odt), r in sorted(RATIOS.items()):
                f.write(f"{fam:16s} {dt:5s} {odt:5s} {r:.3f}\n")


def C(**kw):
    return kw


def ids(cases):
    return [n for n in cases]


# ------------------------------------------------------------------------------------------- generic kernel
# name: (case, Cout tile of igemm_bco / splitk_bco (csrc/conv_igemm.hip) for this Cout_pad)
GENERIC = {
    "3x3_3to16_5x7": (C(Ca=3, Cout=16, H=5, W=7), 16),
    "3x3_s2_24to40_9x11": (C(Ca=24, Cout=40, H=9, W=11, stride=2, residual=True, act=1), 64),
    "1x1_16to1": (C(Ca=16, Cout=1, H=6, W=5, k=1, pad=0), 16),
    "3x3_72to144_6x5_fits_neither": (C(Ca=72, Cout=144, H=6, W=5, act=1), 64),
    "1x1_8to32_tile32": (C(Ca=8, Cout=32, H=9, W=31, k=1, pad=0), 32),
    "1x1_8to64_tile64": (C(Ca=8, Cout=64, H=9, W=31, k=1, pad=0, act=1), 64),
    "3x3_8to128_tile128": (C(Ca=8, Cout=128, H=9, W=15), 128),
    "two_sources_up2_res_mul_out2": (C(Ca=32, Cb=24, Cout=48, H=12, W=10, a_up=2, residual=True, mul=True, out2=True,
                                       act=1, out_view=(64, 8)), 64),
    "1x1_gate_64to40": (C(N=3, Ca=64, Cout=40, H=7, W=5, k=1, pad=0, gate=True), 64),   # (gated: the split-K tiles)
    "convT_64to32": (C(N=3, Ca=64, Cout=32, H=7, W=5, k=1, pad=0, convT=True, act=1), 128),
    "offset_input_view": (C(Ca=16, Cout=24, H=5, W=9, a_view=(48, 16), out_view=(40, 8), act=1), 32),
}


@pytest.mark.parametrize("out_dt", ["f32", "bf16"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("name", ids(GENERIC))
def test_generic(name, dt, out_dt):
    case, tile = GENERIC[name]
    check(case, -1, ("generic", tile), dt, out_dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("act,beta", [(O.ACT_SIGMOID, 1.0), (O.ACT_SILU, 1.0), (O.ACT_SWISH, 1.5)])
def test_generic_activations(act, beta, dt):
    """Sigmoid, SiLU and Swish epilogues (none and ReLU run in every other case), with mul."""
    check(C(Ca=16, Cout=24, H=7, W=9, act=act, beta=beta, mul=True, out2=True), -1, ("generic", 32), dt, tiers="B")


@pytest.mark.parametrize("lin", ["0", "1", "2"])
@pytest.mark.parametrize("name", ["1x1_16to1", "3x3_72to144_6x5_fits_neither", "3x3_s2_24to40_9x11", "1x1_gate_64to40"])
def test_generic_gather_forms(name, lin, monkeypatch):
    """HISEG_IGEMM_LIN (read per call): the (n, y, x) gather (0), the linear 1x1 gather (1) and the tap form (2)."""
    monkeypatch.setenv("HISEG_IGEMM_LIN", lin)
    case, tile = GENERIC[name]
    check(case, -1, ("generic", tile), "bf16", tiers="A")


def workspace_bytes(case, dt="bf16"):
    from hiseg import ops
    c, t, _, _ = reference(tuple(sorted(case.items())), "A", dt, dt)
    p = plan_for(c, t, dt)
    d = L.Conv2dDesc()
    d.dtype = d.out_dtype = L.HISEG_BF16
    d.N, d.H, d.W, d.Ho, d.Wo = c["N"], c["H"], c["W"], c["H"], c["W"]
    d.KH = d.KW = c["k"]
    d.stride, d.pad = 1, c["pad"]
    d.Ca, d.a_cstride, d.a_up = p.ca, p.ca, 1
    d.Cout, d.Cout_pad, d.K_pad = p.gemm_cols, p.cout_pad, p.k_pad
    with L.raw_pointers():   # planning only, never launched
        d.srcA = d.weight = d.scale = d.shift = d.out = 1 << 20
        d.in_scale = (1 << 20) if c["gate"] else None
    return L.lib().hiseg_conv2d_workspace_bytes(ctypes.byref(d)), p


# splitk_plan (csrc/conv_igemm.hip): a 1x1 layer splits only with >= 6 K blocks and, ungated, >= 24 -- so the 384 -> 48
# layer carries an SE gate: nK = 6, nK / 4 = 1 -> 2 splits.  The 3x3 layer: nK = 9 * 192 / 64 = 27 >= 24 over 64 <= 256
# pixels: 27 / 4 = 6 splits of ceil(27 / 6) = 5 K blocks (the last of 2).  Tiles: splitk_bco(48) = splitk_bco(64) = 64.
SPLITK = {
    "1x1_gate_384to48_5x4": (C(Ca=384, Cout=48, H=5, W=4, k=1, pad=0, gate=True, residual=True), 2),
    "3x3_192to64_8x8": (C(Ca=192, Cout=64, H=8, W=8, split_k_3x3=True, act=1), 6),
}


@pytest.mark.parametrize("variant", [99, 0])
@pytest.mark.parametrize("name", ids(SPLITK))
def test_generic_splitk(name, variant):
    case, splits = SPLITK[name]
    nbytes, p = workspace_bytes(case)
    assert nbytes == splits * case.get("N", 2) * case["H"] * case["W"] * p.cout_pad * 4
    check(case, variant, ("generic_splitk", 64))


# ------------------------------------------------------------------------------------------- fast (LDS-DMA ring)
# conv_fast_try: Ca, Cb multiples of 64 (1x1: a source-B tail of 8k < 64 channels), K_pad the 64-rounded K, no gate,
# no upsampling, bf16 out; per variant a Cout_pad multiple
FAST_CMUL = {1: 128, 2: 128, 3: 64, 4: 128, 5: 256, 6: 128, 7: 256, 8: 64, 60: 128, 61: 128, 62: 128, 63: 128, 64: 256,
             65: 64, 66: 128, 67: 64, 68: 64, 69: 128}
FAST = {
    "3x3_64to64_7x5_res": C(Ca=64, Cout=64, H=7, W=5, residual=True, act=1),
    "1x1_64to64_7x5": C(Ca=64, Cout=64, H=7, W=5, k=1, pad=0, mul=True, out2=True),
    "3x3_128to128_7x5": C(Ca=128, Cout=128, H=7, W=5, act=1, mul=True, out2=True),
    "1x1_128to128_7x5_res": C(Ca=128, Cout=128, H=7, W=5, k=1, pad=0, residual=True),
    "1x1_256+8to256_tail": C(Ca=256, Cb=8, Cout=256, H=9, W=7, k=1, pad=0, residual=True, act=1),
    "3x3_64+64to256_17x9": C(Ca=64, Cb=64, Cout=256, H=17, W=9, act=1),
}


@pytest.mark.parametrize("variant", sorted(FAST_CMUL))
@pytest.mark.parametrize("name", ids(FAST))
def test_fast(name, variant):
    case = FAST[name]
    takes = case["Cout"] % FAST_CMUL[variant] == 0
    # (a Cout that is no multiple of the variant's tile: `if (d.Cout_pad % ..) return 0` in conv_fast_try's switch)
    check(case, variant, ("fast", variant) if takes else "generic", tiers="AB" if variant in (61, 68, 5) else "A")


# ------------------------------------------------------------------------------------------- wide
# conv_wide_try: Ca, Cb multiples of 64, K_pad = K >= 128, Cout a multiple of 128 (70 / 71 / 74: 256), ReLU / none, no
# mul / out2 / gate / upsampling
WIDE = {
    "3x3_64+64to256_9x7": C(Ca=64, Cb=64, Cout=256, H=9, W=7, act=1),
    "3x3_64+64to256_9x7_res": C(Ca=64, Cb=64, Cout=256, H=9, W=7, residual=True, act=1),
    "3x3_128to128_9x7": C(Ca=128, Cout=128, H=9, W=7),
    "3x3_128to128_9x7_res": C(Ca=128, Cout=128, H=9, W=7, residual=True, act=1),
}


@pytest.mark.parametrize("variant", [70, 71, 72, 74])
@pytest.mark.parametrize("name", ids(WIDE))
def test_wide(name, variant):
    case = WIDE[name]
    takes = variant == 72 or case["Cout"] % 256 == 0    # (`case 70: if (d.Cout % 256) return 0`, also 71 / 74)
    check(case, variant, ("wide", variant) if takes else "generic")


# ------------------------------------------------------------------------------------------- halo kernels
# conv_hw_try / conv_hwr_try / conv_hwt_try / conv_hwc_applies: 3x3, stride 1, pad 1, ReLU / none, optional residual,
# Ca >= 64, sources in whole 32-channel slices; the fragment kernels (hwr / hwt / hwc) need weight_frag (64-multiple
# sources) and Cout_pad = Cout.  Cout multiple per variant:
HALO_CMUL = {80: 256, 82: 128, 84: 256, 86: 128, 88: 64, 89: 64,
             92: 128, 93: 128, 94: 128, 95: 128, 96: 128, 97: 128, 100: 64, 101: 128, 103: 128,
             102: 64, 104: 128, 105: 256, 106: 128, 107: 64, 108: 128, 109: 128}
HALO_FAMILY = {v: "hw" if v < 90 else "hwt" if v == 103 else "hwr" if v <= 101 and v != 102 else "hwc" for v in HALO_CMUL}
HALO_FAMILY[102] = "hwc"
# the upsampled source: conv_hw any variant; conv_hwr 97 / 100 / 101 (`d.a_up == 2 && variant < 97`); conv_hwc all but
# the multi-tile 109 / 102; conv_hwt none -- ReLU and no residual everywhere
HALO_UP2 = {80, 82, 84, 86, 88, 89, 97, 100, 101, 104, 105, 106, 107, 108}
HALO = {   # Cout: the variant's multiple
    "16x16_one_tile_64": C(Ca=64, H=16, W=16, act=1),
    "17x33_past_both_tiles_128_res": C(Ca=128, H=17, W=33, residual=True, act=1),
    "1x1_pixel_128+64": C(Ca=128, Cb=64, H=1, W=1),
    "3x40_64_res_noact": C(Ca=64, H=3, W=40, residual=True),
    "up2_64+64_18x34": C(Ca=64, Cb=64, H=18, W=34, a_up=2, act=1),
    "offset_views_5x9": C(N=3, Ca=64, H=5, W=9, a_view=(128, 32), residual=True, act=1),   # (+ an output view)
    "offset_view64_128_20x17": C(N=1, Ca=128, H=20, W=17, a_view=(256, 64), act=1),
}


def halo_case(name, variant):
    case = dict(HALO[name], Cout=HALO_CMUL[variant])
    if name == "offset_views_5x9":
        case["out_view"] = (case["Cout"] + 64, 32)
    return case


@pytest.mark.parametrize("variant", sorted(HALO_CMUL))
@pytest.mark.parametrize("name", ids(HALO))
def test_halo(name, variant):
    case = halo_case(name, variant)
    takes = case.get("a_up", 1) == 1 or variant in HALO_UP2
    check(case, variant, (HALO_FAMILY[variant], variant) if takes else "generic")


HALO_PARTIAL_COUTS = (16, 32, 48)


def halo_partial_cases(cout):
    return [C(Ca=64, Cout=cout, H=17, W=33, residual=True, act=1), C(Ca=96, Cout=64 + cout, H=5, W=18)]


@pytest.mark.parametrize("variant", [88, 89])
@pytest.mark.parametrize("cout", HALO_PARTIAL_COUTS)
def test_halo_partial_cout_tile(cout, variant):
    """conv_hw's BCO-64 configurations over fewer than 64 output columns (`narrow` in conv_hw_try)."""
    for case in halo_partial_cases(cout):
        check(case, variant, ("hw", variant))


def f32_rule(name, what, k, ref, r32):
    """|k - ref| <= 4 max|r32 - ref| + 4 * 2^-23 max|ref| (the f32 rule above), r32 torch's float32 evaluation."""
    bound = 4 * (r32.double() - ref).abs().max() + 4 * 2.0 ** -23 * ref.abs().max()
    ratio = ((k - ref).abs().max() / bound).item()
    RATIOS[(name, "bf16", "f32")] = max(RATIOS.get((name, "bf16", "f32"), 0.0), ratio)
    print(f"{name} {what}: max err {(k - ref).abs().max().item():.3e} ratio {ratio:.3f}")
    assert ratio <= 1.0, f"{name} {what}: error / bound = {ratio:.3f}"


# conv_hwc's fused-statistics forms (train mode): conv2d_impl's first branch (csrc/conv_dispatch.cpp).  It picks the
# kernel by Cout alone -- `d->Cout % 128 == 0 ? 104 : 107` -- whichever of 0 / 104 / 107 the caller passed; no
# activation, no residual; the upsampled source with stats_partial only (`d.bnb_partial && (... || d.a_up != 1 ...)` in conv_hwc_applies).
STATS = {
    "64to128_17x33": C(Ca=64, Cout=128, H=17, W=33),
    "128to256_two_cout_tiles_16x16": C(Ca=128, Cout=256, H=16, W=16),
    "64to64_17x33": C(Ca=64, Cout=64, H=17, W=33),
    "64+64to192_3x40": C(N=3, Ca=64, Cb=64, Cout=192, H=3, W=40),
    "up2_64+64to128_18x34": C(Ca=64, Cb=64, Cout=128, H=18, W=34, a_up=2),
    "up2_64+64to64_18x34": C(Ca=64, Cb=64, Cout=64, H=18, W=34, a_up=2),
}


@pytest.mark.parametrize("variant", [0, 104, 107])
@pytest.mark.parametrize("name,kind", [(n, k) for n in STATS for k in ("stats", "bnb")
                                       if k == "stats" or STATS[n].get("a_up", 1) == 1])
def test_hwc_fused_statistics(name, kind, variant):
    """Variants 104 / 107 with stats_partial (count, mean, M2 of the stored bf16 output per split and channel) and
    bnb_partial (sum g, sum g * xhat, sum xhat with g the output masked by the BatchNorm's ReLU): the conv output as
    everywhere (tier A bit for bit, tier B within the bound), the partials merged in float64 against float64 sums
    over the kernel's own output under the f32 rule, the counts exactly."""
    case = STATS[name]
    sv = 104 if case["Cout"] % 128 == 0 else 107
    for tier in "AB":
        c, t, r64, r32, y, _, path, (part, z, tab) = launch(case, variant, tier, fused=kind)
        what = f"{name} {kind} variant {variant} tier {tier}"
        assert path == ("hwc", sv), f"{what}: ran {path}"
        if tier == "A":
            assert r64["S"].max() < 2 ** 22
            assert torch.equal(bits(y), bits(r64["out"])), f"{what}: the conv output differs from the exact value"
        else:
            check_b("hwc", "bf16", what, y, r64, r32, c, t, True)
        N, Co, H, W = y.shape
        v = y.double().permute(1, 0, 2, 3).reshape(Co, -1)          # the stored bf16 output, [Cout][pixels]
        if kind == "stats":
            n, mu, q = part[:, 0], part[:, 1], part[:, 2]
            assert bool((n.sum(0) == N * H * W).all()), f"{what}: counts"
            mean = (n * mu).sum(0) / n.sum(0)
            m2 = q.sum(0) + (n * (mu - mean) ** 2).sum(0)              # Chan's merge, in float64
            rmean, v32 = v.mean(1), v.float()
            m32 = v32.mean(1)
            f32_rule("hwc_stats", what + " mean", mean, rmean, m32)
            f32_rule("hwc_stats", what + " M2", m2, ((v - rmean[:, None]) ** 2).sum(1),
                     ((v32 - m32[:, None]) ** 2).sum(1))
        else:
            col = lambda x: x.double()[:, None]
            zz = z.permute(1, 0, 2, 3).reshape(Co, -1)
            live = zz * col(tab["scale"]) + col(tab["shift"]) > 0
            g = torch.where(live, v, torch.zeros_like(v))
            xh = (zz - col(tab["mean"])) * col(tab["invstd"])
            got = part.sum(0)
            for i, (nm, r) in enumerate((("sum g", g), ("sum g xhat", g * xh), ("sum xhat", xh))):
                r32s = r.float().sum(1) if i != 1 else (g.float() * xh.float()).sum(1)
                f32_rule("hwc_bnb", f"{what} {nm}", got[i], r.sum(1), r32s)


# ------------------------------------------------------------------------------------------- pointwise
# pw_plan (csrc/conv_pw.hip): 1x1, bf16 out, <= 10 k-steps of 32 channels, no out2, not residual and mul together
PW = {
    "128to256_4_ksteps": C(Ca=128, Cout=256, H=9, W=7, k=1, pad=0, act=1),
    "256to256_8_ksteps_res": C(N=3, Ca=256, Cout=256, H=13, W=11, k=1, pad=0, residual=True, act=1),
    "convT_128to64": C(Ca=128, Cout=64, H=6, W=5, k=1, pad=0, convT=True, act=1),
    "one_pixel": C(N=1, Ca=128, Cout=256, H=1, W=1, k=1, pad=0),
    "mul_noact": C(Ca=128, Cout=256, H=5, W=7, k=1, pad=0, mul=True),
    "mul_sigmoid": C(Ca=128, Cout=256, H=5, W=7, k=1, pad=0, mul=True, act=2),
    "narrow_gate_96to24": C(Ca=96, Cout=24, H=9, W=11, k=1, pad=0, gate=True, residual=True),
    "narrow_silu_40to240": C(Ca=40, Cout=240, H=11, W=13, k=1, pad=0, act=3),
}


@pytest.mark.parametrize("name", ids(PW))
def test_pointwise(name):
    check(PW[name], 90, ("pw", 90))


PW_GATE_RANGES = C(N=172, Ca=96, Cout=24, H=2, W=3, k=1, pad=0, gate=True, residual=True)


def test_pointwise_gate_image_ranges():
    """An SE gate table past kPwGateBytes = 64 KiB (conv_pw.hip): N * Ca * 4 = 172 * 96 * 4 = 66048 bytes.  Forced, the
    pointwise kernel declines (`N * Ca * 4 > kPwGateBytes` in pw_plan); the automatic choice runs image ranges of
    65536 / (4 * 96) = 170 images on it (conv_pw_gate_images): two launches, the second of 2 images."""
    case = PW_GATE_RANGES
    check(case, 90, "generic", tiers="A")
    L.conv_path_stats(reset=True)
    check(case, 0, ("pw", 90), tiers="A")
    stats = L.conv_path_stats(reset=True)
    assert stats["pw"] == 2 and sum(stats.values()) == 2, stats


# ------------------------------------------------------------------------------------------- small / rows
# conv_small_try: bf16, 1x1 / 3x3 "same", <= 256 input channels, 64-pixel strips; 51 / 52 / 54 / 58 force 1 / 2 / 4 / 8
# output rows per workgroup.  Stride 2 runs under the automatic choice alone (`if (stamp || variant != 0) return 0`).
SMALL = {
    "3x3_8to64_9x13": C(Ca=8, Cout=64, H=9, W=13, act=1),
    "3x3_8to64_5x63": C(Ca=8, Cout=64, H=5, W=63, act=1),
    "3x3_8to64_5x64": C(Ca=8, Cout=64, H=5, W=64, act=1),
    "3x3_8to64_5x65": C(Ca=8, Cout=64, H=5, W=65, act=1),
    "3x3_16to1_f32": C(Ca=16, Cout=1, H=11, W=40, f32_out=True),
    "up2_32to16": C(Ca=32, Cout=16, H=10, W=70, a_up=2, act=1),
    "1x1_24to144_gate_res": C(N=3, Ca=24, Cout=144, H=7, W=9, k=1, pad=0, gate=True, residual=True, act=1),
}


@pytest.mark.parametrize("variant", [50, 51, 52, 54, 58])
@pytest.mark.parametrize("name", ids(SMALL))
def test_small(name, variant):
    check(SMALL[name], variant, ("small", variant))


SMALL_GATE_TWO_SOURCES = C(Ca=64, Cb=8, Cout=64, H=6, W=7, gate=True, mul=True, out2=True, act=1)


def test_small_gate_two_sources():
    """64 + 8 -> 64 with an SE gate, mul and out2.  72 channels x 10 halo rows x 66 columns plus the weights pass the
    160 KiB of LDS at 8 rows per workgroup (`lds_for(th) > 160 * 1024` in pick_th): variant 58 declines."""
    case = SMALL_GATE_TWO_SOURCES
    for v in (50, 51, 52, 54):
        check(case, v, ("small", v))
    check(case, 58, "generic", tiers="A")


SMALL_S2_SIZES = [(9, 21), (8, 8), (5, 129)]


def small_s2_case(H, W, act):
    return C(Ca=3, Cout=32, H=H, W=W, stride=2, act=act)


@pytest.mark.parametrize("H,W", SMALL_S2_SIZES)
def test_small_stride2(H, W):
    check(small_s2_case(H, W, O.ACT_SILU), 0, ("small", 0), tiers="B")
    check(small_s2_case(H, W, O.ACT_RELU), 0, ("small", 0))


# conv_rows_try: 3x3 "same", 16 / 32 output columns, Cin / 8 in {2, 4} (16 columns) or {4, 12, 16} (32), ReLU / none,
# no residual / mul / out2 / gate
ROWS = {
    "16to16_3x5": C(N=1, Ca=16, Cout=16, H=3, W=5, act=1),
    "16to16_20x70": C(Ca=16, Cout=16, H=20, W=70, act=1),
    "up2_64+32to32": C(Ca=64, Cb=32, Cout=32, H=12, W=20, a_up=2, act=1),
    "16to1_f32": C(Ca=16, Cout=1, H=9, W=33, f32_out=True),
    "32to32_7x130": C(N=3, Ca=32, Cout=32, H=7, W=130),
}


@pytest.mark.parametrize("variant", [98, 0])
@pytest.mark.parametrize("name", ids(ROWS))
def test_rows(name, variant):
    check(ROWS[name], variant, ("rows", 98))


# ------------------------------------------------------------------------------------------- automatic choice
# The path the candidate list of auto_candidates (csrc/conv_dispatch.cpp) gives each layer class, read from the code:
AUTO = {
    "pw_1x1_256to256": (C(Ca=256, Cout=256, H=9, W=7, k=1, pad=0, act=1), ("pw", 90), "bf16"),
    "rows_3x3_16to16": (C(Ca=16, Cout=16, H=9, W=21, act=1), ("rows", 98), "bf16"),
    # fragment-packed weights, Cout % 128 == 0: conv_hwc 108 (HISEG_CONV_HWC_R3 unset, no multi-tile default)
    "hwc108_128to128": (C(Ca=128, Cout=128, H=17, W=18, residual=True, act=1), ("hwc", 108), "bf16"),
    "hwc108_up2_64+64to128": (C(Ca=64, Cb=64, Cout=128, H=18, W=20, a_up=2, act=1), ("hwc", 108), "bf16"),
    "hwc107_64to64": (C(Ca=64, Cout=64, H=17, W=34, residual=True, act=1), ("hwc", 107), "bf16"),
    # no fragments (a 96-channel source is no 64 multiple): conv_hw 86 / 89
    "hw86_96to128": (C(Ca=96, Cout=128, H=9, W=18, act=1), ("hw", 86), "bf16"),
    "hw89_96to80": (C(Ca=96, Cout=80, H=9, W=18, act=1), ("hw", 89), "bf16"),
    # stride 2 is no halo-kernel layer: the wide tile at Cout % 256 == 0, else the ring kernel's 61 / 68
    "wide70_s2_64to256": (C(Ca=64, Cout=256, H=9, W=7, stride=2, act=1), ("wide", 70), "bf16"),
    "fast61_s2_64to128": (C(Ca=64, Cout=128, H=9, W=7, stride=2, act=1), ("fast", 61), "bf16"),
    "fast68_s2_64to64": (C(Ca=64, Cout=64, H=9, W=7, stride=2, act=1), ("fast", 68), "bf16"),
    "small_3x3_8to64": (C(Ca=8, Cout=64, H=9, W=13, act=1), ("small", 0), "bf16"),
    "generic_5x5_24to32": (C(Ca=24, Cout=32, H=10, W=14, k=5, pad=2, act=1), ("generic", 32), "bf16"),
    "generic_f32": (C(Ca=12, Cout=20, H=7, W=9, act=1), ("generic", 32), "f32"),
}


@pytest.mark.parametrize("name", ids(AUTO))
def test_automatic_choice(name):
    case, path, dt = AUTO[name]
    check(case, 0, path, dt, tiers="A")


# The toggles auto_candidates reads per call, on layers of the HALO table (test_halo forces the same variants on them):
# (variable, value, HALO layer, Cout, path)
AUTO_TOGGLES = [
    ("HISEG_CONV_HWC_R3", "0", "17x33_past_both_tiles_128_res", 128, ("hwc", 104)),   # two halo buffers, not 108's ring
    ("HISEG_CONV_HWC64", "0", "16x16_one_tile_64", 64, ("hwr", 100)),                 # conv_hwr, not conv_hwc 107
    ("HISEG_CONV_HWC_MTW", "1", "17x33_past_both_tiles_128_res", 128, ("hwc", 109)),  # the multi-tile forms
    ("HISEG_CONV_HWC_MTW", "1", "16x16_one_tile_64", 64, ("hwc", 102)),
]


@pytest.mark.parametrize("var,value,name,cout,path", AUTO_TOGGLES,
                         ids=[f"{t[0]}={t[1]}_cout{t[3]}" for t in AUTO_TOGGLES])
def test_automatic_choice_toggles(var, value, name, cout, path, monkeypatch):
    """HISEG_CONV_HWC_R3 / HISEG_CONV_HWC64 / HISEG_CONV_HWC_MTW move the automatic choice of a 128- / 64-Cout
    fragment layer to another bit-identical kernel (HISEG_CONV_HALO and HISEG_CONV_WAVES are read once per process
    and cannot be set here)."""
    monkeypatch.setenv(var, value)
    check(dict(HALO[name], Cout=cout), 0, path, "bf16", tiers="A")


# ------------------------------------------------------------------------------------------- declines
# One layer just outside each family's rule: it reports the generic kernel and is still exact.
DECLINES = {
    "pw_on_3x3": (C(Ca=128, Cout=256, H=5, W=7), 90),                        # pw_plan: `d.KH != 1`
    # a finding: pw_plan builds the 256 + 8 combiner's 9-k-step form (`comb`), but `(rb > 4 && nks > 8)` two lines
    # above refuses rb == 16 with 9 k-steps first, so no layer reaches it (the combiner runs on the ring kernel)
    "pw_256+8_combiner_9_ksteps": (C(Ca=256, Cb=8, Cout=256, H=9, W=7, k=1, pad=0, act=1), 90),
    "pw_with_out2": (C(Ca=128, Cout=256, H=5, W=7, k=1, pad=0, out2=True, mul=True), 90),   # pw_plan: `if (d.out2)`
    "wide_cout120": (C(Ca=256, Cout=120, H=5, W=7), 70),                     # conv_wide_try: `d.Cout & 127`
    "fast_ca40": (C(Ca=40, Cout=240, H=6, W=7), 61),                         # conv_fast_try: `d.Ca % 64 != 0`
    "hw_ca32": (C(Ca=32, Cout=128, H=6, W=7), 86),                           # conv_hw_try: `d.Ca < 64`
    "hwr_no_frag": (C(Ca=64, Cout=128, H=6, W=7, no_frag=True), 97),         # conv_hwr_try: `d.weight_frag == nullptr`
    "hwt_no_frag": (C(Ca=64, Cout=128, H=6, W=7, no_frag=True), 103),        # conv_hwt_try: the same
    "hwc_cout64_at_108": (C(Ca=64, Cout=64, H=6, W=7), 108),                 # conv_hwc_applies: `d.Cout & 127`
    "rows_with_residual": (C(Ca=16, Cout=16, H=6, W=7, residual=True), 98),  # conv_rows_try: `d.residual`
    "small_cin264": (C(Ca=264, Cout=16, H=4, W=5, k=1, pad=0), 50),          # conv_small_try: `a.Cin > 256`
}


@pytest.mark.parametrize("name", ids(DECLINES))
def test_declined_variant_runs_the_generic_kernel(name):
    case, variant = DECLINES[name]
    check(case, variant, "generic", tiers="A")
