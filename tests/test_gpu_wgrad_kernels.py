"""Every weight-gradient kernel behind hiseg_conv2d_wgrad (csrc/train_conv.hip, wgrad_wide.hip, wgrad_hwc.hip), both
split reducers behind hiseg_conv2d_wgrad_reduce and hiseg_pack_weights, each on its own against the float64 oracle of
tests/wgrad_oracle.py.  The three entry points are called directly through hiseg._lib with hand-built descriptors; the
kernel the library reports (hiseg._lib.wgrad_last_path) is asserted after every weight gradient, since a layer a tile
declines falls through to another kernel and would otherwise be compared with the wrong name on it.

Inputs are rounded to the compute dtype before either side sees them.  Source and dy buffers hold the sentinel -7.5
outside the channels the layer reads; `ws`, `gw` and `gb` are pre-filled with it and end in a 64-element guard tail
that must still hold it.  `ws` itself is compared on j < Cout, k < Ktot + bias, split by split (the pixel partition
of wgrad_geometry, the halo tile's own tile partition), then reduced by the library onto old values and compared again.

Tier A, exact.  X and dy are integers in {-2..2}: every partial sum of every element is an integer below 4 M < 2^22
(tests/test_wgrad_oracle.py proves the premise per case from its shape), exact in f32 and in the MFMA's accumulator, so
a correct kernel equals float64 bit for bit under any tile, split and reduction order.  A dropped ragged pixel block,
a wrong bias column, a missed 8-channel chunk of a K tile, one mis-scattered tap or a stale padded column changes an
integer and cannot hide.  The reducers are also run on synthetic integer partials at pinned split counts, and the
packing kernel bit for bit against wgrad_oracle.pack (bf16 by round-to-nearest-even), with the data gradient closed
on the GPU: hiseg_conv2d_fwd over dy with the mode-1 / mode-3 pack and the descriptor train_engine.conv_bwd builds
equals float64 autograd's dx.

Tier B, rounding.  Normal values rounded to the compute dtype, dy scaled by 1 / sqrt(M).  The reduced f32 gradient
obeys the f32 rule of tests/test_gpu_train_kernels.py, |k - ref| <= 4 max(e32) + 4 * 2^-23 max|ref| with e32 the
oracle run in float32 over the same splits.  Worst observed error / bound per kernel family and compute dtype
(profiles/wgrad_kernel_errors.txt, MI355X; tier A is bit for bit everywhere):

  family            dtype  ratio
  f32               f32    0.204
  halo              bf16   0.132
  transposed_read   bf16   0.114
  wide              bf16   0.111
  (The generic bf16 kernel and the far-apart forms run in child processes, tier A only.  No family needed the derived
  (M + splits) 2^-24 S term; against it the worst element sits at 0.08.)
"""
import ctypes
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

import conv_kernel_oracle as O
import wgrad_oracle as W
from hiseg import _lib as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SENTINEL = -7.5          # exact in bf16; tier A values are integers
GUARD = 64
RATIOS = {}


def C(**kw):
    return kw


# ------------------------------------------------------------------------------------------- case tables
# A case: conv_kernel_oracle's vocabulary plus bias (the GEMM-bias column), a_view / dy_view = (cstride, coff).
# Halo tile (wgrad_hwc_shape_ok: bf16, 3x3 stride 1 pad 1, Ca / Cb / Cout multiples of 64; 8 x 16 pixel tiles)
HALO = {
    "64to64_9x17_one_past_the_tile": C(Ca=64, Cout=64, H=9, W=17),
    "64to64_7x5_smaller_than_a_tile": C(Ca=64, Cout=64, H=7, W=5),
    "128to128_2x2_tiles": C(Ca=128, Cout=128, H=9, W=17),
    "64+64to64_one_resource_per_source": C(Ca=64, Cb=64, Cout=64, H=9, W=17),
    "dy_view": C(Ca=64, Cout=64, H=9, W=17, dy_view=(80, 8)),
    "source_view": C(Ca=64, Cout=64, H=9, W=17, a_view=(80, 8)),
    "N8_more_than_one_split": C(N=8, Ca=64, Cout=64, H=9, W=17),
}

# Wide tile (wgrad_wide_bc: Cin % 256 == 0, Cg % 256 == 0, Kg >= 256; the halo tile off).  SHT: the shared-tap
# addressing form wgrad_wide_try picks (2: stride 1 full resolution, 1: stride 2 / upsampled, 0: two sources)
WIDE = {
    "3x3_M96_ragged_block_sht2": C(N=1, Ca=256, Cout=256, H=8, W=12),
    "1x1_Kg256_lower_bound": C(N=1, Ca=256, Cout=256, H=8, W=12, k=1, pad=0),
    "3x3_bias_64_more_columns": C(N=1, Ca=256, Cout=256, H=8, W=12, bias=True),
    "stride2_sht1": C(N=2, Ca=256, Cout=256, H=16, W=12, stride=2),
    "up2_sht1": C(N=1, Ca=256, Cout=256, H=8, W=12, a_up=2, bias=True),
    "128+128to256_sht0": C(N=1, Ca=128, Cb=128, Cout=256, H=8, W=12, bias=True),
    "ragged_last_split": C(N=2, Ca=256, Cout=256, H=32, W=27, bias=True),
}
WIDE_RAGGED = "ragged_last_split"

# Transposed-read tile (conv_wgrad_tr_kernel: column tiles 128 / 64 / 32 / 16 by Cg; INC: stride 1 full resolution)
TR = {
    "128to128_3x3_bias_in_its_own_ktile": C(Ca=128, Cout=128, H=9, W=7, bias=True),     # Ktot = 1152 = 9 x 128
    "128to128_1x1_tile128": C(Ca=128, Cout=128, H=9, W=7, k=1, pad=0),
    "stride2_64to32_not_incremental": C(Ca=64, Cout=32, H=10, W=9, stride=2, bias=True),
    "up2_64to64_not_incremental": C(Ca=64, Cout=64, H=10, W=8, a_up=2),
    "convT_64to16_4x16_columns": C(Ca=64, Cout=16, H=7, W=5, k=1, pad=0, convT=True, bias=True),
    "two_near_64+64to128_3x3": C(Ca=64, Cb=64, Cout=128, H=9, W=7, bias=True),
    "two_near_32+24to16_1x1": C(Ca=32, Cb=24, Cout=16, H=9, W=7, k=1, pad=0),
}
for _co, _tile in ((64, 64), (48, 32), (32, 32), (16, 16), (8, 16)):
    for _k in (1, 3):
        TR[f"64to{_co}_{_k}x{_k}_tile{_tile}"] = C(N=3, Ca=64, Cout=_co, H=9, W=7, k=_k, pad=_k // 2, bias=_co != 32)

# f32 kernel (conv_wgrad_kernel<float>: 32-pixel blocks; wgrad_typed's four tiles by Cg)
F32 = {
    "8to128_tile128x128": C(Ca=8, Cout=128, H=5, W=7, bias=True),
    "8to64_1x1_tile128x64": C(Ca=8, Cout=64, H=5, W=7, k=1, pad=0),
    "12to32_tile128x32": C(Ca=12, Cout=32, H=5, W=7),
    "ca4_real3_to4_tile64x16": C(Ca=3, Cout=4, H=9, W=5, bias=True),
    "two_sources_5+4to20": C(Ca=5, Cb=4, Cout=20, H=6, W=7, bias=True),
    "stride2_8to16": C(Ca=8, Cout=16, H=9, W=11, stride=2),
    "convT_8to4": C(Ca=8, Cout=4, H=5, W=3, k=1, pad=0, convT=True, bias=True),
}

# Two sources, near (this process) and far apart (child process B, HISEG_PLACEMENT_FAR=1): (case, HISEG_WGRAD_INC,
# x_tile_src of the far-apart run, kernel near); far apart every one runs the transposed-read tile.  x_tile_src 1:
# Ca % 128 == 0 and (1x1 or Cb % 128 == 0), else 2.
FAR = {
    "src1_128+128to64_3x3_inc": (C(Ca=128, Cb=128, Cout=64, H=9, W=7, bias=True), "1", 1, "transposed_read"),
    "src1_128+128to64_3x3_noinc": (C(Ca=128, Cb=128, Cout=64, H=9, W=7, bias=True), "0", 1, "transposed_read"),
    "src1_128+64to128_1x1_inc": (C(Ca=128, Cb=64, Cout=128, H=9, W=7, k=1, pad=0), "1", 1, "transposed_read"),
    "src2_64+64to128_3x3_inc": (C(Ca=64, Cb=64, Cout=128, H=9, W=7, bias=True), "1", 2, "transposed_read"),
    "src2_64+64to128_3x3_noinc": (C(Ca=64, Cb=64, Cout=128, H=9, W=7, bias=True), "0", 2, "transposed_read"),
    "src2_64+64to64_3x3_inc": (C(Ca=64, Cb=64, Cout=64, H=9, W=7), "1", 2, "transposed_read"),
    "src2_64+64to64_up2_noinc": (C(Ca=64, Cb=64, Cout=64, H=10, W=8, a_up=2), "1", 2, "transposed_read"),
    "src2_64+32to32_1x1_tile32": (C(Ca=64, Cb=32, Cout=32, H=9, W=7, k=1, pad=0, bias=True), "1", 2, "transposed_read"),
    "src2_64+64to16_3x3_tile16": (C(Ca=64, Cb=64, Cout=16, H=9, W=7), "1", 2, "transposed_read"),
    # near: the wide tile; far apart it declines (`hiseg_force_far()` in wgrad_wide_bc) and the transposed-read tile runs
    "wide_declines_128+128to256": (C(Ca=128, Cb=128, Cout=256, H=8, W=12, bias=True), "1", 1, "wide"),
}

# Reducers on synthetic integer partials in {-3..3}: hiseg_wgrad_map fields, then (splits, accumulate, gb given)
QUAD_MAP = dict(Cout=7, KH=3, KW=3, ca=8, ca_real=5, cb=8, cb_real=3, convT=0, want_bias=1)    # 7 x 37 quads: 259 items
QUAD_CONVT = dict(Cout=32, KH=1, KW=1, ca=16, ca_real=13, cb=0, cb_real=0, convT=1, want_bias=1)
TAPS_MAP = dict(Cout=5, KH=3, KW=3, ca=12, ca_real=12, cb=0, cb_real=0, convT=0, want_bias=1)    # 15 items
QUAD_SPLITS = (1, 5, 33, 70)          # 33: the `sp += 32` wrap; 70: two wraps and a ragged group
TAPS_SPLITS = (1, 64, 65, 130)        # <64, 4> up to 64 splits, <16, 16> past them
REDUCE_ABS = 3
REDUCE_OLD = 100                      # |old gradient| of the accumulate runs


def all_wgrad_cases():
    """(table, name, case, dtype) of every tier A weight-gradient case, for tests/test_wgrad_oracle.py."""
    out = []
    for tab, cases, dt in (("halo", HALO, "bf16"), ("wide", WIDE, "bf16"), ("tr", TR, "bf16"), ("f32", F32, "f32")):
        for n, c in cases.items():
            out += [(tab, n, dict(c, bias=b), dt) for b in ((False, True) if tab == "halo" else (c.get("bias", False),))]
    out += [("far", n, v[0], "bf16") for n, v in FAR.items()]
    return out


# ------------------------------------------------------------------------------------------- plumbing
def nhwc(x, dt, cread, view=None):
    """NCHW float64 -> (device buffer, cstride, coff): NHWC, the sentinel outside the `cread` channels the layer reads
    (the real ones, then zero pads) and in a guard tail."""
    N, Cr, H, Wd = x.shape
    cs, coff = view or (cread, 0)
    n = N * H * Wd * cs
    buf = torch.full((n + GUARD,), SENTINEL, dtype=torch.float64)
    v = buf[:n].view(N, H, Wd, cs)
    v[..., coff:coff + cread] = 0
    v[..., coff:coff + Cr] = x.permute(0, 2, 3, 1)
    return buf.to(O.DTYPES[dt]).to(DEV), cs, coff


def filled(n, value=SENTINEL, dtype=torch.float32):
    return torch.full((n + GUARD,), value, dtype=dtype, device=DEV)


def tail_ok(buf, n):
    return bool((buf[n:] == SENTINEL).all().item())


@functools.lru_cache(maxsize=None)
def inputs(key, tier, dt):
    return W.make_inputs(dict(key), tier, dt)


def hdt(dt):
    return L.HISEG_BF16 if dt == "bf16" else L.HISEG_F32


def wgrad_desc(c, g, dt, xa, xb):
    """The forward descriptor's input side, as train_engine._desc fills it."""
    d = L.Conv2dDesc()
    d.dtype = d.out_dtype = hdt(dt)
    d.N, d.H, d.W, d.Ho, d.Wo = c["N"], c["H"], c["W"], g["Ho"], g["Wo"]
    d.KH, d.KW = g["KH"], g["KW"]
    d.stride, d.pad = (1, 0) if c["convT"] else (c["stride"], c["pad"])
    d.srcA, d.a_cstride, d.a_coff, d.Ca, d.a_up = xa[0], xa[1], xa[2], g["ca"], c["a_up"]
    if xb is not None:
        d.srcB, d.b_cstride, d.b_coff, d.Cb = xb[0], xb[1], xb[2], g["cb"]
    d.Cout, d.Cout_pad, d.convT = g["cols"], g["Cg"], int(c["convT"])
    return d


def map_struct(m):
    s = L.WgradMap()
    for k, v in m.items():
        setattr(s, k, v)
    return s


def run_reduce(ws_dev, splits, m, old_gw, old_gb, accumulate):
    """hiseg_conv2d_wgrad_reduce onto sentinel-tailed gw / gb holding `old`; returns (gw, gb, tails intact)."""
    gw = filled(old_gw.numel())
    gw[:old_gw.numel()] = old_gw.reshape(-1).float().to(DEV)
    gb = None
    if old_gb is not None:
        gb = filled(old_gb.numel())
        gb[:old_gb.numel()] = old_gb.float().to(DEV)
    L.check(L.lib().hiseg_conv2d_wgrad_reduce(ws_dev.data_ptr(), splits, ctypes.byref(map_struct(m)), gw.data_ptr(),
                                              gb.data_ptr() if gb is not None else None, accumulate, L.stream_ptr()),
            "wgrad_reduce")
    torch.cuda.synchronize()
    ok = tail_ok(gw, old_gw.numel()) and (gb is None or tail_ok(gb, old_gb.numel()))
    return (gw[:old_gw.numel()].cpu().double().view(old_gw.shape),
            gb[:old_gb.numel()].cpu().double() if gb is not None else None, ok)


def evaluate(case, dt, tier):
    """One weight gradient and its reduction on the GPU against the oracle; returns a dict of plain values (the child
    processes send it back as JSON): the recorded path, the partition, and per comparison the number of differing
    elements (tier A) or error / bound (tier B)."""
    case = dict(case)
    bias = int(case.pop("bias", False))
    a_view, dy_view = case.pop("a_view", None), case.pop("dy_view", None)
    c, xa, xb, dy = inputs(tuple(sorted(case.items())), tier, dt)
    g = W.geometry(c, dt, bias)
    A = nhwc(xa, dt, g["ca"], a_view)
    B = nhwc(xb, dt, g["cb"]) if xb is not None else None
    if B is not None:
        # both sources in one allocation: near each other wherever the caching allocator has got to (late in a long
        # process it hands out blocks more than 2^31 bytes apart, and the layer would take the far-apart form)
        both = torch.cat([A[0], B[0]])
        assert A[0].numel() * A[0].element_size() % 16 == 0
        A, B = (both[:A[0].numel()],) + A[1:], (both[A[0].numel():],) + B[1:]
    Y = nhwc(dy, dt, W.rup(c["Cout"], W.CHUNK[dt]), dy_view)
    d = wgrad_desc(c, g, dt, A, B)
    Cg, Kg, sp = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    L.check(L.lib().hiseg_conv2d_wgrad_dims(ctypes.byref(d), bias, ctypes.byref(Cg), ctypes.byref(Kg), ctypes.byref(sp)),
            "wgrad_dims")
    assert (Cg.value, Kg.value) == (g["Cg"], g["Kg"]), (Cg.value, Kg.value, g)
    splits = sp.value
    nblocks = (g["M"] + g["PB"] - 1) // g["PB"]
    bps = (nblocks + splits - 1) // splits     # (wgrad_geometry: splits = ceil(nblocks / bps) with this bps)
    n = splits * g["Cg"] * g["Kg"]
    ws = filled(n)
    placed = L.placement_stats(reset=True)
    L.check(L.lib().hiseg_conv2d_wgrad(ctypes.byref(d), Y[0].data_ptr(), Y[1], Y[2], bias, ws.data_ptr(), splits,
                                       L.stream_ptr()), "wgrad")
    torch.cuda.synchronize()
    path = L.wgrad_last_path()
    declined, far = L.placement_stats(reset=True)
    res = dict(path=path, splits=splits, bps=bps, nblocks=nblocks, M=g["M"], declined=declined, far=far,
               ws_tail=tail_ok(ws, n))
    X = O.gather_input(xa, xb, c["a_up"], None, dt)
    part = W.halo_partition(c["N"], c["H"], c["W"], splits) if path == "halo" else None
    ref = W.partials(c, X, dy, bias, splits, bps, dt, partition=part)
    ncol = g["Ktot"] + bias
    got = ws[:n].view(splits, g["Cg"], g["Kg"])[:, :g["cols"], :ncol].cpu().double()
    m = W.wgrad_map(c, dt, bias)
    gen = O.gen(7)
    gshape = (g["ca_real"], c["Cout"], 2, 2) if g["convT"] else (c["Cout"], c["Ca"] + c["Cb"], g["KH"], g["KW"])
    if tier == "A":
        res["ws_diff"] = int((got != ref).sum())
        old_w, old_b = O.ints(gen, *gshape, lo=-3, hi=3), (O.ints(gen, c["Cout"], lo=-3, hi=3) if bias else None)
        gw, gb, ok = run_reduce(ws, splits, m, old_w, old_b, 1)
        rw, rb = W.reduce(ref, m, (old_w, old_b))
        res.update(gw_diff=int((gw != rw).sum()), gb_diff=int((gb != rb).sum()) if bias else 0, g_tail=ok)
    else:
        zw, zb = torch.full(gshape, 5.0, dtype=torch.float64), (torch.full((c["Cout"],), 5.0) if bias else None)
        gw, gb, ok = run_reduce(ws, splits, m, zw, zb, 0)
        rw, rb = W.reduce(ref, m)
        ew, eb = W.reduce(W.partials(c, X, dy, bias, splits, bps, dt, compute=torch.float32, partition=part), m)
        Sw, Sb = W.reduce(W.S(c, X, dy, bias, dt)[None], dict(m))
        ratio = derived = 0.0
        for k, r, e, s in ((gw, rw, ew, Sw), (gb, rb, eb, Sb)):
            if k is None:
                continue
            bound = 4 * (e.double() - r).abs().max() + 4 * 2.0 ** -23 * r.abs().max()
            ratio = max(ratio, ((k - r).abs().max() / bound).item())
            dbound = ((g["M"] + splits) * 2.0 ** -24 * s).clamp_min(1e-300)
            derived = max(derived, ((k - r).abs() / dbound).max().item())
        res.update(ratio=ratio, derived=derived, g_tail=ok)
    return res


def require(res, expect, what, tier="A", far=None):
    assert res["path"] == expect, f"{what}: ran {res['path']}, expected {expect}"
    assert res["ws_tail"] and res["g_tail"], f"{what}: a store past the end of ws / gw / gb"
    if far is not None:   # (declined or None = not looked at, far): the placement events this launch recorded
        assert res["far"] == far[1] and far[0] in (None, res["declined"]), \
            f"{what}: placement (declined, far) {res['declined'], res['far']}"
    if tier == "A":
        assert res["ws_diff"] == 0, f"{what} {res['path']}: {res['ws_diff']} partial sums differ from the exact value"
        assert res["gw_diff"] == 0 and res["gb_diff"] == 0, \
            f"{what}: {res['gw_diff']} weight and {res['gb_diff']} bias gradients differ after the reduce"
    else:
        key = (res["path"], what.split()[-1])
        RATIOS[key] = max(RATIOS.get(key, 0.0), res["ratio"])
        print(f"{what}: f32-rule ratio {res['ratio']:.3f}, derived-bound ratio {res['derived']:.3f}")
        assert res["ratio"] <= 1.0, f"{what}: error / bound = {res['ratio']:.3f}"


def check(case, dt, expect, what, tiers="AB"):
    out = None
    for tier in tiers:
        if tier == "A":
            assert W.tier_a_bound(case, dt, case.get("bias", False)) < 2 ** 22
        out = evaluate(case, dt, tier)
        require(out, expect, f"{what} tier {tier} {dt}", tier)
    return out


@pytest.fixture(scope="module", autouse=True)
def ratio_report():
    yield
    path = os.environ.get("HISEG_WGRAD_KERNEL_ERRORS")
    if path:
        with open(path, "w") as f:
            f.write("# worst |kernel - float64 oracle| / bound of the reduced f32 gradient per weight-gradient kernel and\n"
                    "# compute dtype, tier B (tests/test_gpu_wgrad_kernels.py: 4 max(e32) + 4 * 2^-23 max|ref|); tier A is\n"
                    "# bit for bit\n")
            for (fam, dt), r in sorted(RATIOS.items()):
                f.write(f"{fam:17s} {dt:5s} {r:.3f}\n")


# ------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("name", list(HALO))
def test_halo(name, bias):
    res = check(dict(HALO[name], bias=bias), "bf16", "halo", f"halo {name} bias {bias}")
    if name == "N8_more_than_one_split":
        assert res["splits"] > 1, res


@pytest.mark.parametrize("name", list(WIDE))
def test_wide(name, monkeypatch):
    monkeypatch.setenv("HISEG_WGRAD_HWC", "0")
    res = check(WIDE[name], "bf16", "wide", f"wide {name}")
    if name == WIDE_RAGGED:   # more than one block per split and a shorter last split
        assert res["bps"] > 1 and res["nblocks"] % res["bps"] != 0, res


@pytest.mark.parametrize("knob,value", [("HISEG_WGRAD_SHT", "2"), ("HISEG_WGRAD_SHT", "1"), ("HISEG_WGRAD_SHT", "0"),
                                        ("HISEG_WGRAD_TOG", "1"), ("HISEG_WGRAD_TOG", "0")])
@pytest.mark.parametrize("name", ["3x3_M96_ragged_block_sht2", "3x3_bias_64_more_columns", WIDE_RAGGED])
def test_wide_addressing_knobs_bit_equal(name, knob, value, monkeypatch):
    """Every shared-tap / toggled-ring form of the wide tile gives the exact value, hence the same bits."""
    monkeypatch.setenv("HISEG_WGRAD_HWC", "0")
    monkeypatch.setenv(knob, value)
    check(WIDE[name], "bf16", "wide", f"wide {name} {knob}={value}", tiers="A")


@pytest.mark.parametrize("name", list(TR))
def test_transposed_read(name, monkeypatch):
    monkeypatch.setenv("HISEG_WGRAD_HWC", "0")
    check(TR[name], "bf16", "transposed_read", f"tr {name}")


@pytest.mark.parametrize("knob", ["HISEG_WGRAD_INC", "HISEG_WGRAD_TOG"])
@pytest.mark.parametrize("name", ["128to128_3x3_bias_in_its_own_ktile", "64to64_3x3_tile64", "two_near_64+64to128_3x3"])
def test_transposed_read_plain_addressing(name, knob, monkeypatch):
    """The non-incremental / untoggled instantiations of the 128- and 64-column tiles on stride-1 layers."""
    monkeypatch.setenv("HISEG_WGRAD_HWC", "0")
    monkeypatch.setenv(knob, "0")
    check(TR[name], "bf16", "transposed_read", f"tr {name} {knob}=0", tiers="A")


@pytest.mark.parametrize("name", list(F32))
def test_f32_kernel(name):
    check(F32[name], "f32", "f32", f"f32 {name}")


@pytest.mark.parametrize("name", list(FAR))
def test_two_sources_near(name, monkeypatch):
    """The two-source cases of child process B with both sources in one allocation (near): the same exact value as
    far apart, so the two placements agree bit for bit."""
    case, inc, _, near = FAR[name]
    monkeypatch.setenv("HISEG_WGRAD_HWC", "0")
    monkeypatch.setenv("HISEG_WGRAD_INC", inc)
    res = evaluate(case, "bf16", "A")
    require(res, near, f"near {name}", far=(0, 0))


# ------------------------------------------------------------------------------------------- child processes
_CHILD = r"""
import json, sys
sys.path[:0] = [sys.argv[1] + "/human-instance-segmentation_amd", sys.argv[1] + "/tests"]
import test_gpu_wgrad_kernels as T
print("RESULT " + json.dumps(T.child(sys.argv[2])))
"""


def child(which):
    """Runs in a fresh process whose environment selects kernels this process cannot reach."""
    out = {}
    if which == "generic":
        for name, case in TR.items():
            out[name] = evaluate(case, "bf16", "A")
    else:
        for name, (case, inc, _, _) in FAR.items():
            os.environ["HISEG_WGRAD_INC"] = inc
            out[name] = evaluate(case, "bf16", "A")
    return out


def run_child(which, env):
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, which], env=dict(os.environ, **env), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_generic_bf16_kernel_in_a_child_process():
    """HISEG_WGRAD_TR / _WIDE are read once per process and no shape reaches the generic bf16 kernel: the
    transposed-read table with all three tiles off records generic_bf16 and is exact."""
    res = run_child("generic", {"HISEG_WGRAD_TR": "0", "HISEG_WGRAD_WIDE": "0", "HISEG_WGRAD_HWC": "0"})
    assert set(res) == set(TR)
    for name, r in res.items():
        require(r, "generic_bf16", f"generic {name}")


def test_far_apart_sources_in_a_child_process():
    """HISEG_PLACEMENT_FAR=1 (read once per process): x_tile_src 1 and 2 with and without incremental offsets, and the
    layer the wide tile declines; each records the far-apart form once (that layer the decline too: wgrad_wide_bc notes
    one for any far-apart layer of 128-multiple columns, taken or not) and the exact value."""
    res = run_child("far", {"HISEG_PLACEMENT_FAR": "1", "HISEG_WGRAD_HWC": "0"})
    assert set(res) == set(FAR)
    for name, r in res.items():
        declines = FAR[name][3] == "wide"
        require(r, "transposed_read", f"far {name}", far=(1, 1) if declines else (None, 1))


# ------------------------------------------------------------------------------------------- reducers
def reduce_case(m, splits, accumulate, with_gb, monkeypatch=None, taps=None):
    m = dict(m)
    Ktot = m["KH"] * m["KW"] * (m["ca"] + m["cb"])
    ncol = Ktot + m["want_bias"]
    m["Cg"], m["Kg"] = W.rup(m["Cout"], 16), W.rup(ncol, 64)
    assert splits * REDUCE_ABS * (4 if m["convT"] else 1) + REDUCE_OLD < 2 ** 23
    gen = O.gen(31 * splits + accumulate)
    ws = torch.full((splits, m["Cg"], m["Kg"]), 1e30, dtype=torch.float64)      # (what the reducers must not add)
    ws[:, :m["Cout"], :ncol] = O.ints(gen, splits, m["Cout"], ncol, lo=-REDUCE_ABS, hi=REDUCE_ABS)
    dev = filled(ws.numel())
    dev[:ws.numel()] = ws.reshape(-1).float().to(DEV)
    cr = m["ca_real"] + m["cb_real"]
    gshape = (m["ca_real"], m["Cout"] // 4, 2, 2) if m["convT"] else (m["Cout"], cr, m["KH"], m["KW"])
    nb = m["Cout"] // 4 if m["convT"] else m["Cout"]
    old_w = O.ints(gen, *gshape, lo=-REDUCE_OLD, hi=REDUCE_OLD)
    old_b = O.ints(gen, nb, lo=-REDUCE_OLD, hi=REDUCE_OLD) if with_gb else None
    if taps is not None:
        monkeypatch.setenv("HISEG_WGRAD_REDUCE_TAPS", taps)
    gw, gb, ok = run_reduce(dev, splits, m, old_w, old_b, accumulate)
    rw, rb = W.reduce(ws[:, :m["Cout"], :ncol], m, (old_w, old_b) if accumulate else None)
    what = f"{m} splits {splits} accumulate {accumulate} gb {with_gb} taps {taps}"
    assert ok and tail_ok(dev, ws.numel()), f"{what}: a store past the end"
    assert torch.equal(gw, rw), f"{what}: {(gw != rw).sum().item()} of {gw.numel()} weight gradients differ"
    if with_gb:   # (want_bias = 0 with a gb buffer: untouched)
        assert torch.equal(gb, rb if m["want_bias"] else old_b), f"{what}: the bias gradient differs"


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("splits", QUAD_SPLITS)
def test_reduce_quad_of_k(splits, accumulate):
    """wgrad_reduce_kernel: two sources with pad channels on both (ca_real < ca, cb_real < cb), 259 items."""
    reduce_case(QUAD_MAP, splits, accumulate, True)


@pytest.mark.parametrize("m,with_gb", [(QUAD_CONVT, True), (QUAD_CONVT, False), (dict(QUAD_CONVT, want_bias=0), True),
                                       (QUAD_MAP, False), (dict(QUAD_MAP, want_bias=0), True)],
                         ids=["convT_bias", "convT_gb_null", "convT_no_bias", "conv_gb_null", "conv_no_bias"])
@pytest.mark.parametrize("splits", [5, 33])
def test_reduce_quad_of_k_forms(m, with_gb, splits):
    """The ConvTranspose scatter and its 4-sub-pixel bias sum, gb = NULL, want_bias = 0."""
    for accumulate in (0, 1):
        reduce_case(m, splits, accumulate, with_gb)


@pytest.mark.parametrize("taps", ["1", "0"])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("splits", TAPS_SPLITS)
def test_reduce_tap_major(splits, accumulate, taps, monkeypatch):
    """wgrad_reduce_taps_kernel<64, 4> (splits <= 64) and <16, 16>, 15 items; HISEG_WGRAD_REDUCE_TAPS=0 (the quad-of-K
    kernel on the same map) gives the same exact value."""
    reduce_case(TAPS_MAP, splits, accumulate, True, monkeypatch, taps)
    if splits == 65:
        reduce_case(dict(TAPS_MAP, want_bias=0), splits, accumulate, False, monkeypatch, taps)


# ------------------------------------------------------------------------------------------- weight packing
def pack_entries():
    """Every mode in both dtypes.  conv 5 + 3 -> 20 (ca_real < ca, cb_real < cb, cop = 24 > Cout), ConvTranspose
    13 -> 8, the biases, and a 256 -> 64 3x3 layer of 147 456 elements (past the 512 x 256 threads of one sweep) row-major
    and in fragment order."""
    conv = dict(Cout=20, Cin_real=8, KH=3, KW=3, ca=8, ca_real=5, cb=8, cb_real=3, cop=24)
    convT = dict(Cout=8, Cin_real=13, KH=2, KW=2, ca=16, ca_real=13, cb=0, cb_real=0, cop=8)
    big = dict(Cout=64, Cin_real=256, KH=3, KW=3, ca=256, ca_real=256, cb=0, cb_real=0, cop=64)
    out = []
    for dt in ("f32", "bf16"):
        out += [dict(conv, mode=0, rows=32, K_pad=192, dt=dt), dict(conv, mode=1, rows=16, K_pad=256, dt=dt),
                dict(convT, mode=2, rows=32, K_pad=64, dt=dt), dict(convT, mode=3, rows=16, K_pad=64, dt=dt),
                dict(big, mode=0, rows=64, K_pad=2304, dt=dt), dict(big, mode=1, rows=256, K_pad=576, dt=dt)]
    out += [dict(conv, mode=W.PACK_BIAS, rows=1, K_pad=20, dt="f32"), dict(convT, mode=W.PACK_BIAS, rows=1, K_pad=32, dt="f32"),
            dict(big, mode=0 | W.PACK_FRAG, rows=64, K_pad=2304, dt="bf16"),
            dict(big, mode=1 | W.PACK_FRAG, rows=256, K_pad=576, dt="bf16")]
    for e in out:
        e["total"] = e["rows"] * e["K_pad"]
    return out


def pack_src(e, gen, integers=False):
    if (e["mode"] & 7) == W.PACK_BIAS:
        shape = (e["Cout"],)
    elif (e["mode"] & 7) in (2, 3):
        shape = (e["Cin_real"], e["Cout"], 2, 2)
    else:
        shape = (e["Cout"], e["Cin_real"], e["KH"], e["KW"])
    if integers:
        return O.ints(gen, *shape).float()
    return torch.randn(*shape, generator=gen, dtype=torch.float64).float()


def run_pack(entries):
    """One hiseg_pack_weights launch over the table; returns each entry's destination (with its tail) on the host."""
    structs, dsts = [], []
    for e in entries:
        s = L.PackEntry()
        s.src = e["src"].contiguous().to(DEV)
        dst = filled(e["total"], dtype=O.DTYPES[e["dt"]])
        s.dst, s.dtype, s.mode = dst, hdt(e["dt"]), e["mode"]
        for f in ("Cout", "Cin_real", "KH", "KW", "ca", "ca_real", "cb", "cb_real", "rows", "K_pad", "cop", "total"):
            setattr(s, f, e[f])
        structs.append(s)
        dsts.append(dst)
    tab = torch.frombuffer(bytearray(b"".join(bytes(s) for s in structs)), dtype=torch.uint8).to(DEV)
    L.check(L.lib().hiseg_pack_weights(tab.data_ptr(), len(structs), max(e["total"] for e in entries), L.stream_ptr()),
            "pack_weights")
    torch.cuda.synchronize()
    return dsts


def test_pack_weights_every_mode():
    gen = O.gen(5)
    entries = pack_entries()
    assert max(e["total"] for e in entries) > 512 * 256 and min(e["total"] for e in entries) == 20
    for e in entries:
        e["src"] = pack_src(e, gen)
    for e, dst in zip(entries, run_pack(entries)):
        what = f"mode {e['mode']} {e['dt']} {e['rows']}x{e['K_pad']}"
        ref = W.pack(e).float().to(O.DTYPES[e["dt"]])        # (torch rounds to nearest even)
        host = dst.cpu()
        assert bool((host[e["total"]:] == SENTINEL).all()), f"{what}: a store past `total`"
        raw = torch.int16 if e["dt"] == "bf16" else torch.int32
        assert torch.equal(host[:e["total"]].view(raw), ref.view(raw)), \
            f"{what}: {(host[:e['total']] != ref).sum().item()} of {e['total']} packed values differ"


DGRAD = {   # the data-gradient forms train_engine.conv_bwd launches: stride-1 convs (mode 1), ConvTranspose 2x2 (mode 3)
    "conv_3x3_12to20": C(N=2, Ca=12, Cout=20, H=6, W=7),
    "conv_1x1_16to8": C(N=2, Ca=16, Cout=8, H=5, W=7, k=1, pad=0),
    "conv_3x3_5+3to20": C(N=2, Ca=5, Cb=3, Cout=20, H=6, W=7),
    "convT_13to8": C(N=2, Ca=13, Cout=8, H=4, W=5, k=1, pad=0, convT=True),
}


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(DGRAD))
def test_packed_dgrad_weights_give_autograd_dx(name, dt):
    """The loop closed on the GPU, tier A: the mode-1 / mode-3 pack of integer weights through hiseg_conv2d_fwd over an
    integer dy, with the descriptor train_engine.conv_bwd builds, equals float64 autograd's dx (bf16: its
    round-to-nearest-even)."""
    import torch.nn.functional as F
    from hiseg import ops
    c = dict(O.CASE_DEFAULTS, **DGRAD[name])
    g = W.geometry(c, dt, False)
    ce = W.CHUNK[dt]
    gen = O.gen(9)
    cop = W.rup(c["Cout"], ce)
    cinp, cinr = g["ca"] + g["cb"], c["Ca"] + c["Cb"]
    k = 2 if c["convT"] else c["k"]
    e = dict(Cout=c["Cout"], Cin_real=cinr, KH=k, KW=k, ca=g["ca"], ca_real=c["Ca"], cb=g["cb"], cb_real=c["Cb"],
             cop=cop, mode=3 if c["convT"] else 1, dt=dt)
    e["rows"] = W.rup(cinp, 64) if cinp > 64 else W.rup(cinp, 16)      # dg_cout_pad
    e["K_pad"] = W.rup(k * k * cop, 64)                                # dg_k_pad
    e["total"] = e["rows"] * e["K_pad"]
    e["src"] = pack_src(e, gen, integers=True)
    wd = run_pack([e])[0]
    x = O.ints(gen, c["N"], cinr, c["H"], c["W"]).requires_grad_(True)
    dshape = (c["N"], c["Cout"], 2 * c["H"], 2 * c["W"]) if c["convT"] else (c["N"], c["Cout"], c["H"], c["W"])
    dy = O.ints(gen, *dshape)
    if c["convT"]:
        y = F.conv_transpose2d(x, e["src"].double(), stride=2)
    else:
        y = F.conv2d(x, e["src"].double(), padding=c["pad"])
    (y * dy).sum().backward()
    assert x.grad.abs().max() * 1 < 2 ** 22
    dz, dcs, dco = nhwc(dy, dt, cop)
    n = c["N"] * c["H"] * c["W"] * cinp
    out = filled(n, dtype=O.DTYPES[dt])
    dg = L.Conv2dDesc()
    dg.dtype = dg.out_dtype = hdt(dt)
    dg.N, dg.H, dg.W, dg.Ho, dg.Wo = c["N"], dshape[2], dshape[3], c["H"], c["W"]
    dg.KH, dg.KW, dg.stride, dg.pad = (2, 2, 2, 0) if c["convT"] else (k, k, 1, k - 1 - c["pad"])
    dg.srcA, dg.a_cstride, dg.a_coff, dg.Ca, dg.a_up = dz, dcs, dco, cop, 1
    dg.weight, dg.Cout, dg.Cout_pad, dg.K_pad = wd, cinp, e["rows"], e["K_pad"]
    dg.scale = torch.ones(max(e["rows"], 16), dtype=torch.float32, device=DEV)
    dg.shift = torch.zeros(max(e["rows"], 16), dtype=torch.float32, device=DEV)
    dg.act = O.ACT_NONE
    dg.out, dg.o_cstride, dg.o_coff = out, cinp, 0
    L.check(L.lib().hiseg_conv2d_fwd(ctypes.byref(dg), L.stream_ptr()), "conv2d(dgrad)")
    torch.cuda.synchronize()
    host = out.cpu()
    assert bool((host[n:] == SENTINEL).all()), "a store past the end of dx"
    got = host[:n].view(c["N"], c["H"], c["W"], cinp)
    ref = torch.zeros(c["N"], c["H"], c["W"], cinp, dtype=torch.float64)
    ref[..., :c["Ca"]] = x.grad[:, :c["Ca"]].permute(0, 2, 3, 1)
    ref[..., g["ca"]:g["ca"] + c["Cb"]] = x.grad[:, c["Ca"]:].permute(0, 2, 3, 1)
    ref = ref.float().to(O.DTYPES[dt])
    assert torch.equal(got, ref), f"{name} {dt}: {(got != ref).sum().item()} of {ref.numel()} data gradients differ"
