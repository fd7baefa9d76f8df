"""Each non-convolution training kernel on its own against the float64 oracles of tests/train_kernel_oracle.py.

Inputs are rounded to the compute dtype before either side sees them, nothing is excluded from a comparison, and
every bound is built from `e32`, the element-wise error of torch's own float32 evaluation of the same oracle:

  f32 output / gradient            |k - ref| <= 4 max(e32) + 4 * 2^-23 max|ref|
  bf16 output written once         2^-8 |ref| + the f32 rule
  bf16 output with accumulate      2^-7 max(|old|, |ref|) + the f32 rule

Masks, sentinels on dead channels, argmax, tie routing and the dropout masks are exact.

Entry point -> test
  hiseg_relu_bwd                          test_relu_bwd
  hiseg_sigmoid_bwd, hiseg_gate_fwd       test_sigmoid_bwd_and_gate_fwd
  hiseg_gate_bwd                          test_gate_bwd
  hiseg_act_bwd_pre                       test_act_bwd_pre
  hiseg_act_bwd_cvt                       test_act_bwd_cvt
  hiseg_add_inplace                       test_add_inplace
  hiseg_maxpool2x2_bwd                    test_maxpool2x2_bwd
  hiseg_upsample2x_bwd                    test_upsample2x_bwd, test_upsample2x_bwd_rejects_misaligned_view
  hiseg_resize_bilinear_bwd (and _fwd)    test_resize_bilinear_bwd
  hiseg_attn_spatial_train_fwd / _bwd     test_spatial_attention, test_spatial_attention_tied_maximum,
                                          test_spatial_attention_sum_rows_threshold
  hiseg_attn_channel_train_fwd / _bwd     test_channel_attention
  hiseg_se_train_fwd / _bwd               test_squeeze_excite
  hiseg_ubf_train_fwd / _bwd              test_ubf_head
  hiseg_pw2_bwd                           test_pw2_bwd
  hiseg_roi_align_bwd_affine              test_roi_align_bwd_affine
  hiseg_ln_fwd_stats, hiseg_ln_bwd        test_layernorm2d
  hiseg_dropout2d_mask / _dev, hiseg_seed_advance   test_dropout_masks
  hiseg_attn_spatial_ws, hiseg_attn_channel_ws, hiseg_se_train_ws, hiseg_ubf_ws, hiseg_pw2_ws
                                          test_workspace_extents (the sizes themselves: tests/test_abi.py, no GPU)

Worst observed ratio of kernel error over bound per kernel and dtype (profiles/train_kernel_errors.txt):

  kernel                        f32     bf16
  act_bwd_cvt                   0.097   0.982
  act_bwd_pre                   0.228   0.988
  add_inplace                   0.072   0.498
  attn_channel_bwd              0.225   0.995
  attn_channel_train_fwd        0.186   0.994
  attn_spatial_bwd              0.277   0.982
  attn_spatial_train_fwd        0.163   0.984
  gate_bwd                      0.108   0.976
  gate_fwd                      0.051   0.973
  ln_bwd                        0.233   0.968
  ln_fwd_stats                  0.105   0.074
  maxpool2x2_bwd                0.081   0.498
  pw2_bwd                       0.089   0.973
  relu_bwd                      0.065   0.947
  resize_bilinear_bwd           0.209   -
  roi_align_bwd_affine          0.245   0.331
  se_train_bwd                  0.159   0.991
  se_train_fwd                  0.165   0.975
  sigmoid_bwd                   0.119   0.979
  ubf_train_bwd                 0.306   0.432
  ubf_train_fwd                 0.207   0.279
  upsample2x_bwd                0.134   0.996
  (MI355X.  A bf16 output written once sits near 1.0 by construction: 2^-8 |ref| is exactly the worst case of
  one round-to-nearest to bf16's 8-bit significand, and the kernels' f32 arithmetic adds only the small f32 term.
  The f32 column is where the arithmetic itself is measured.)
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import train_kernel_oracle as O
from hiseg import _lib as L
from hiseg.ops import Act
from hiseg.train_engine import ew

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
HD = {"f32": L.HISEG_F32, "bf16": L.HISEG_BF16}
SENTINEL = -7.5          # exact in bf16; no kernel under test produces it on a dead channel
RATIOS = {}


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


def rnd(g, dt, *shape, scale=1.0):
    """float64 values that are exactly representable in the compute dtype."""
    return (scale * torch.randn(*shape, generator=g, dtype=torch.float64)).to(DTYPES[dt]).double()


def rnd32(g, *shape, scale=1.0):
    return rnd(g, "f32", *shape, scale=scale)


def away_from_zero(g, dt, *shape):
    """|v| >= 2^-6 with mixed signs, after rounding: an unambiguous ReLU pattern."""
    v = torch.randn(*shape, generator=g, dtype=torch.float64)
    v = (torch.sign(v) * (2.0 ** -6 + v.abs())).to(DTYPES[dt]).double()
    assert v.abs().min() >= 2.0 ** -6 and (v > 0).any() and (v < 0).any()
    return v


def chan_table(g, N, C):
    """A Dropout2d-like [N][C] f32 table with zeros, different for every image."""
    m = torch.rand(N, C, generator=g, dtype=torch.float64) + 0.5
    m[torch.rand(N, C, generator=g) < 0.3] = 0.0
    m[0, 0], m[N - 1, C - 1] = 0.0, 1.0 / 0.7
    return m.float().double()


def up(t, dtype=torch.float32):
    return t.to(dtype).to(DEV).contiguous()


def ptr(t):
    return None if t is None else t.data_ptr()


def workspace(n):
    """A kernel's float workspace of the size its *_ws entry point gave (test_workspace_extents guards it)."""
    return torch.empty(n, device=DEV)


class GuardedWorkspaces:
    """workspace() with NaN contents and 64 sentinel floats behind each buffer."""
    GUARD = 64

    def __init__(self):
        self.bufs = []

    def __call__(self, n):
        buf = torch.full((n + self.GUARD,), float("nan"), device=DEV)
        buf[n:] = SENTINEL
        self.bufs.append(buf)
        return buf[:n]

    def assert_guards_untouched(self):
        assert self.bufs, "no workspace was allocated"
        want = torch.full((self.GUARD,), SENTINEL, device=DEV).view(torch.int32)
        for buf in self.bufs:
            assert torch.equal(buf[-self.GUARD:].view(torch.int32), want), "a kernel wrote past its workspace"


class View:
    """[P][cstride] buffer with channels [coff, coff + C) live and the sentinel everywhere else."""

    def __init__(self, vals, dtype, cstride, coff):
        self.P, self.C = vals.shape
        self.cstride, self.coff = cstride, coff
        buf = torch.full((self.P, cstride), SENTINEL, dtype=torch.float64)
        buf[:, coff:coff + self.C] = vals
        self.t = buf.to(dtype).to(DEV).contiguous()
        self.before = self.t.clone()

    def ew(self):
        return ew(Act(self.t, 1, 1, self.P, self.C, self.cstride, self.coff))

    def live(self):
        return self.t[:, self.coff:self.coff + self.C].double().cpu()

    def assert_dead_untouched(self):
        dead = torch.ones(self.cstride, dtype=torch.bool)
        dead[self.coff:self.coff + self.C] = False
        a, b = self.t[:, dead.to(DEV)], self.before[:, dead.to(DEV)]
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "a dead channel was written"

    def assert_unchanged(self):
        assert torch.equal(self.t.view(torch.uint8), self.before.view(torch.uint8))


VIEWS = {"dense": lambda C: (C, 0), "off8": lambda C: (C + 8, 8), "off3": lambda C: (C + 8, 3)}


def view(vals, dt, layout):
    cs, co = VIEWS[layout](vals.shape[1])
    return View(vals, DTYPES[dt], cs, co)


def both(fn, *args, **kw):
    """The oracle in float64 and in float32 on the same inputs."""
    def cast(a, dtype):
        if isinstance(a, torch.Tensor) and a.is_floating_point():
            return a.to(dtype)
        if isinstance(a, dict):
            return {k: cast(v, dtype) for k, v in a.items()}
        if isinstance(a, (tuple, list)):
            return type(a)(cast(v, dtype) for v in a)
        return a
    r64 = fn(*cast(args, torch.float64), **cast(kw, torch.float64))
    r32 = fn(*cast(args, torch.float32), **cast(kw, torch.float32))
    return r64, r32


def check(kernel, dt, what, k, r64, r32, mode="f32", old=None):
    """Assert the bound of the module docstring; record the ratio error / bound."""
    k = k.detach().double().cpu().reshape(r64.shape)
    r64, r32 = r64.double(), r32.double()
    base = 4 * (r32 - r64).abs().max() + 4 * 2.0 ** -23 * r64.abs().max()
    if mode == "f32":
        bound = base.expand_as(r64)
    elif mode == "once":
        bound = 2.0 ** -8 * r64.abs() + base
    else:
        bound = 2.0 ** -7 * torch.maximum(old.double().reshape(r64.shape).abs(), r64.abs()) + base
    err = (k - r64).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300)).max().item()
    key = (kernel, dt)
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    print(f"{kernel} {dt} {what}: max err {err.max().item():.3e} ratio {ratio:.3f}")
    assert ratio <= 1.0, f"{kernel} {dt} {what}: error / bound = {ratio:.3f} (max err {err.max().item():.3e})"


def out_mode(dt, acc=False):
    return "f32" if dt == "f32" else ("acc" if acc else "once")


@pytest.fixture(scope="module", autouse=True)
def ratio_report():
    yield
    path = os.environ.get("HISEG_TRAIN_KERNEL_ERRORS")
    if path:
        with open(path, "w") as f:
            f.write("# worst |kernel - float64 oracle| / bound per kernel and dtype (tests/test_gpu_train_kernels.py)\n")
            for (kern, dt), r in sorted(RATIOS.items()):
                f.write(f"{kern:28s} {dt:5s} {r:.3f}\n")


# ------------------------------------------------------------------------------------------- 1. element-wise
N1, HW1 = 3, 35
P1 = N1 * HW1
EW_PARAMS = [(dt, C, lay) for dt in DTYPES for C in (8, 12, 5) for lay in VIEWS]
ew_cases = pytest.mark.parametrize("dt,C,lay", EW_PARAMS)


@ew_cases
@pytest.mark.parametrize("with_mul", [False, True])
def test_relu_bwd(dt, C, lay, with_mul):
    g = gen(100 + C)
    dy, y = rnd(g, dt, P1, C), away_from_zero(g, dt, P1, C)
    mul = chan_table(g, N1, C) if with_mul else None
    vdy, vy, vdz = view(dy, dt, lay), view(y, dt, lay), view(rnd(g, dt, P1, C), dt, lay)
    mul_d = None if mul is None else up(mul)
    ok(lib().hiseg_relu_bwd(HD[dt], P1, HW1, C, vdy.ew(), vy.ew(), ptr(mul_d), vdz.ew(), stream()), "relu_bwd")
    r64, r32 = both(O.relu_bwd, dy, y, mul, HW1)
    check("relu_bwd", dt, f"C={C} {lay}", vdz.live(), r64, r32, out_mode(dt))
    vdz.assert_dead_untouched()
    if with_mul:   # image n's row of the table scales image n's pixels: rows differ, so a wrong p / HW shows
        assert not torch.equal(mul[0], mul[1]) and not torch.equal(mul[1], mul[2])


@ew_cases
def test_sigmoid_bwd_and_gate_fwd(dt, C, lay):
    g = gen(110 + C)
    dy, a = rnd(g, dt, P1, C), rnd(g, dt, P1, C)
    s = torch.sigmoid(torch.randn(P1, C, generator=g, dtype=torch.float64)).to(DTYPES[dt]).double()
    vdy, va, vs = view(dy, dt, lay), view(a, dt, lay), view(s, dt, lay)
    vdz, vout = view(rnd(g, dt, P1, C), dt, lay), view(rnd(g, dt, P1, C), dt, lay)
    ok(lib().hiseg_sigmoid_bwd(HD[dt], P1, C, vdy.ew(), vs.ew(), vdz.ew(), stream()), "sigmoid_bwd")
    ok(lib().hiseg_gate_fwd(HD[dt], P1, C, va.ew(), vs.ew(), vout.ew(), stream()), "gate_fwd")
    check("sigmoid_bwd", dt, f"C={C} {lay}", vdz.live(), *both(O.sigmoid_bwd, dy, s), out_mode(dt))
    check("gate_fwd", dt, f"C={C} {lay}", vout.live(), *both(O.gate_fwd, a, s), out_mode(dt))
    vdz.assert_dead_untouched()
    vout.assert_dead_untouched()


@ew_cases
@pytest.mark.parametrize("which", ["da", "dzg", "both"])
@pytest.mark.parametrize("acc", [0, 1])
def test_gate_bwd(dt, C, lay, which, acc):
    g = gen(120 + C)
    dy, a = rnd(g, dt, P1, C), rnd(g, dt, P1, C)
    gt = torch.sigmoid(torch.randn(P1, C, generator=g, dtype=torch.float64)).to(DTYPES[dt]).double()
    da_old, dzg_old = rnd(g, dt, P1, C), rnd(g, dt, P1, C)
    vdy, va, vg = view(dy, dt, lay), view(a, dt, lay), view(gt, dt, lay)
    vda, vdzg = view(da_old, dt, lay), view(dzg_old, dt, lay)
    e_da = vda.ew() if which != "dzg" else L.EwView()
    e_dzg = vdzg.ew() if which != "da" else L.EwView()
    ok(lib().hiseg_gate_bwd(HD[dt], P1, C, vdy.ew(), va.ew(), vg.ew(), e_da, acc, e_dzg, stream()), "gate_bwd")
    (da64, dzg64), (da32, dzg32) = both(O.gate_bwd, dy, a, gt)
    if which != "dzg":
        if acc:
            da64, da32 = da64 + da_old, da32 + da_old.float()
        check("gate_bwd", dt, f"da C={C} {lay} acc={acc}", vda.live(), da64, da32, out_mode(dt, acc), da_old)
        vda.assert_dead_untouched()
    else:
        vda.assert_unchanged()
    if which != "da":
        check("gate_bwd", dt, f"dzg C={C} {lay}", vdzg.live(), dzg64, dzg32, out_mode(dt))
        vdzg.assert_dead_untouched()
    else:
        vdzg.assert_unchanged()


ACTS = [(0, 1.0), (1, 1.0), (2, 1.0), (3, 1.0), (4, 1.0), (5, 1.5), (5, 0.75)]


@ew_cases
def test_act_bwd_pre(dt, C, lay):
    g = gen(130 + C)
    dy, z, old = rnd(g, dt, P1, C), away_from_zero(g, dt, P1, C), rnd(g, dt, P1, C)
    vdy, vz = view(dy, dt, lay), view(z, dt, lay)
    for act, beta in ACTS:
        for acc in (0, 1):
            vdz = view(old, dt, lay)
            ok(lib().hiseg_act_bwd_pre(HD[dt], P1, C, vdy.ew(), vz.ew(), act, beta, vdz.ew(), acc, stream()),
               "act_bwd_pre")
            r64, r32 = both(O.act_bwd_pre, dy, z, act, beta)
            if acc:
                r64, r32 = r64 + old, r32 + old.float()
            check("act_bwd_pre", dt, f"act={act} beta={beta} C={C} {lay} acc={acc}", vdz.live(), r64, r32,
                  out_mode(dt, acc), old)
            vdz.assert_dead_untouched()


@ew_cases
def test_act_bwd_cvt(dt, C, lay):
    """dy and y are f32 views whatever the dtype of dz.  The derivative is taken from the output y, which only
    none / ReLU / sigmoid allow: the smooth codes are refused (they used to return dy unchanged, silently)."""
    g = gen(140 + C)
    dy, old = rnd32(g, P1, C), rnd(g, dt, P1, C)
    ys = {0: rnd32(g, P1, C), 1: O.act_fn(away_from_zero(g, "f32", P1, C), 1),
          2: torch.sigmoid(rnd32(g, P1, C)).float().double()}
    cs, co = VIEWS[lay](C)
    vdy = View(dy, torch.float32, cs, co)
    for act in range(6):
        vy = View(ys.get(act, ys[0]), torch.float32, cs, co)
        for acc in (0, 1):
            vdz = view(old, dt, lay)
            st = lib().hiseg_act_bwd_cvt(HD[dt], P1, C, vdy.ew(), vy.ew(), act, vdz.ew(), acc, stream())
            torch.cuda.synchronize()
            if act >= 3:
                assert st == -1, f"act_bwd_cvt accepted activation {act}"     # HISEG_ERR_BAD_ARG
                vdz.assert_unchanged()
                continue
            assert st == 0
            r64, r32 = both(O.act_bwd_cvt, dy, ys[act], act)
            if acc:
                r64, r32 = r64 + old, r32 + old.float()
            check("act_bwd_cvt", dt, f"act={act} C={C} {lay} acc={acc}", vdz.live(), r64, r32, out_mode(dt, acc), old)
            vdz.assert_dead_untouched()


@ew_cases
def test_add_inplace(dt, C, lay):
    g = gen(150 + C)
    dst, src = rnd(g, dt, P1, C), rnd(g, dt, P1, C)
    vdst, vsrc = view(dst, dt, lay), view(src, dt, lay)
    ok(lib().hiseg_add_inplace(HD[dt], P1, C, vdst.ew(), vsrc.ew(), stream()), "add_inplace")
    check("add_inplace", dt, f"C={C} {lay}", vdst.live(), *both(O.add, dst, src), out_mode(dt, True), dst)
    vdst.assert_dead_untouched()


# ------------------------------------------------------------------------------------------- 2. max-pool
def pool_input(g, kind, N, H, W, C):
    """Windows of four exactly representable levels scaled by a power of two per window."""
    Ho, Wo = H // 2, W // 2
    sc = 2.0 ** torch.randint(-2, 3, (N, Ho, Wo, C), generator=g).double()
    if kind == "unique":
        perm = torch.argsort(torch.rand(N, Ho, Wo, C, 4, generator=g), dim=-1)
        lv = torch.tensor([-1.5, -0.5, 0.5, 1.5], dtype=torch.float64)[perm]
    elif kind == "equal":
        lv = torch.tensor([0.5, -1.5, 1.5], dtype=torch.float64)[torch.randint(0, 3, (N, Ho, Wo, C, 1), generator=g)]
        lv = lv.expand(-1, -1, -1, -1, 4)
    else:   # the maximum shared by positions 1 = (0,1) and 2 = (1,0)
        lv = torch.tensor([-0.5, 1.5, 1.5, 0.5], dtype=torch.float64).expand(N, Ho, Wo, C, 4)
    w = lv * sc.unsqueeze(-1)
    x = torch.empty(N, H, W, C, dtype=torch.float64)
    for k, (i, j) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        x[:, i::2, j::2, :] = w[..., k]
    if kind == "unique":
        top2 = w.topk(2, dim=-1).values
        assert (top2[..., 0] > top2[..., 1]).all()
    return x


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("C", [5, 8])
@pytest.mark.parametrize("kind", ["unique", "equal", "tie12"])
@pytest.mark.parametrize("acc", [0, 1])
def test_maxpool2x2_bwd(dt, C, kind, acc):
    g = gen(200 + C)
    N, H, W = 2, 6, 10
    x = pool_input(g, kind, N, H, W, C)
    assert torch.equal(x.to(DTYPES[dt]).double(), x)
    dy, old = rnd(g, dt, N, H // 2, W // 2, C), rnd(g, dt, N, H, W, C)
    xd, dyd, dxd = up(x, DTYPES[dt]), up(dy, DTYPES[dt]), up(old, DTYPES[dt])
    ok(lib().hiseg_maxpool2x2_bwd(HD[dt], ptr(xd), N, H, W, C, ptr(dyd), ptr(dxd), acc, stream()), "maxpool2x2_bwd")
    r64, r32 = both(O.maxpool2x2_bwd, x, dy)
    if kind == "equal":     # the whole gradient lands on position (0,0)
        assert r64[:, 1::2].abs().max() == 0 and r64[:, :, 1::2].abs().max() == 0
    if kind == "tie12":     # ... on (0,1), the first of the two maxima
        assert torch.equal(r64[:, 0::2, 1::2], dy) and r64[:, 1::2, 0::2].abs().max() == 0
    if acc:
        r64, r32 = r64 + old, r32 + old.float()
    check("maxpool2x2_bwd", dt, f"C={C} {kind} acc={acc}", dxd, r64, r32, out_mode(dt, acc), old)
    if not acc:             # routing is exact: the kernel moves values, it does not compute
        assert torch.equal(dxd.double().cpu(), r64)


# ------------------------------------------------------------------------------------------- 3. nearest x2 backward
@pytest.mark.parametrize("dt,C", [("f32", 8), ("f32", 4), ("bf16", 8)])
@pytest.mark.parametrize("acc", [0, 1])
def test_upsample2x_bwd(dt, C, acc):
    g = gen(300 + C)
    N, h, w = 2, 3, 5
    dy, old = rnd(g, dt, N, 2 * h, 2 * w, C), rnd(g, dt, N, h, w, C)
    vdy, vdx = view(dy.reshape(-1, C), dt, "off8"), view(old.reshape(-1, C), dt, "off8")
    ok(lib().hiseg_upsample2x_bwd(HD[dt], N, h, w, C, vdy.ew(), vdx.ew(), acc, stream()), "upsample2x_bwd")
    r64, r32 = both(O.upsample2x_bwd, dy)
    if acc:
        r64, r32 = r64 + old, r32 + old.float()
    check("upsample2x_bwd", dt, f"C={C} acc={acc}", vdx.live(), r64.reshape(-1, C), r32.reshape(-1, C),
          out_mode(dt, acc), old.reshape(-1, C))
    vdx.assert_dead_untouched()
    vdy.assert_unchanged()


@pytest.mark.parametrize("dt", DTYPES)
def test_upsample2x_bwd_rejects_misaligned_view(dt):
    g = gen(310)
    N, h, w, C = 2, 3, 5, 8
    vdy = view(rnd(g, dt, N * 4 * h * w, C), dt, "off8")
    vdx = view(rnd(g, dt, N * h * w, C), dt, "off3")
    st = lib().hiseg_upsample2x_bwd(HD[dt], N, h, w, C, vdy.ew(), vdx.ew(), 0, stream())
    torch.cuda.synchronize()
    assert st == -2      # HISEG_ERR_BAD_SHAPE
    vdx.assert_unchanged()


# ------------------------------------------------------------------------------------------- 4. bilinear resize backward
@pytest.mark.parametrize("src,dst", [((16, 12), (32, 24)), ((7, 5), (32, 24)), ((9, 11), (4, 6)), ((1, 1), (5, 3)),
                                     ((6, 1), (6, 4))])
def test_resize_bilinear_bwd(src, dst):
    g = gen(400)
    NC, (h, w), (H, W) = 3, src, dst
    x, gy = rnd32(g, NC, h, w), rnd32(g, NC, H, W)
    xd, gd = up(x), up(gy)
    dx = torch.full((NC, h, w), SENTINEL, device=DEV)
    y = torch.full((NC, H, W), SENTINEL, device=DEV)
    ok(lib().hiseg_resize_bilinear_bwd(ptr(gd), NC, h, w, H, W, ptr(dx), stream()), "resize_bilinear_bwd")
    ok(lib().hiseg_resize_bilinear_fwd(ptr(xd), NC, h, w, ptr(y), H, W, stream()), "resize_bilinear_fwd")
    xr = x.clone().requires_grad_(True)
    (torch.nn.functional.interpolate(xr[None], size=dst, mode="bilinear", align_corners=False)[0] * gy).sum().backward()
    r64, r32 = both(O.resize_bilinear_bwd, gy, h, w)
    assert (r64 - xr.grad).abs().max() <= 1e-12 * xr.grad.abs().max()      # the oracle is F.interpolate's adjoint
    check("resize_bilinear_bwd", "f32", f"{src}->{dst}", dx, r64, r32)
    # adjoint identity with the project's own forward, dot products in float64.  Each side is a sum of products of
    # f32 interpolation weights (<= 3 roundings: scale, source coordinate, fraction) and <= 4 taps per axis pair
    # (<= 5 more roundings): 8 ulp of the magnitude sum per side
    lhs = (y.double().cpu() * gy).sum()
    rhs = (x * dx.double().cpu()).sum()
    mag = (O.resize_bilinear_fwd(x.abs(), H, W) * gy.abs()).sum()
    assert (lhs - rhs).abs() <= 16 * 2.0 ** -23 * mag, f"adjoint identity: {lhs.item()} vs {rhs.item()}"


# ------------------------------------------------------------------------------------------- 5. spatial attention
def run_spatial(dt, x, w7, mul, dout, dw_old):
    N, H, W, C = x.shape
    k = w7.shape[-1]
    P = N * H * W
    T = DTYPES[dt]
    xd, dd, wd = up(x, T), up(dout, T), up(w7)
    md = None if mul is None else up(mul)
    stats = torch.empty(P, 2, device=DEV)
    am = torch.full((P,), -1, dtype=torch.int32, device=DEV)
    att = torch.empty(P, device=DEV)
    out, dx = torch.empty_like(xd), torch.empty_like(xd)
    ok(lib().hiseg_attn_spatial_train_fwd(HD[dt], ptr(xd), N, H, W, C, ptr(wd), k, ptr(md), ptr(stats), ptr(am),
                                          ptr(att), ptr(out), stream()), "attn_spatial_train_fwd")
    ws = workspace(lib().hiseg_attn_spatial_ws(N, H, W, k))
    dw = up(dw_old)
    ok(lib().hiseg_attn_spatial_bwd(HD[dt], ptr(xd), N, H, W, C, ptr(wd), k, ptr(md), ptr(stats), ptr(am), ptr(att),
                                    ptr(dd), ptr(dx), ptr(ws), ptr(dw), stream()), "attn_spatial_bwd")
    return dict(stats=stats, argmax=am, att=att, out=out, dx=dx, dw7=dw)


def check_spatial(dt, tag, x, w7, mul, dout, dw_old, kr):
    r64, r32 = both(O.spatial_attention, x, w7, mul, dout, dw_old)
    N, H, W, C = x.shape
    assert torch.equal(kr["argmax"].cpu().long().view(N, H, W), O.first_argmax(x)), "argmax is not the first maximum"
    check("attn_spatial_train_fwd", dt, tag + " mean", kr["stats"][:, 0], r64["mean"], r32["mean"])
    assert torch.equal(kr["stats"][:, 1].double().cpu().view(N, H, W), r64["max"])
    check("attn_spatial_train_fwd", dt, tag + " att", kr["att"], r64["att"], r32["att"])
    check("attn_spatial_train_fwd", dt, tag + " out", kr["out"], r64["out"], r32["out"], out_mode(dt))
    check("attn_spatial_bwd", dt, tag + " dx", kr["dx"], r64["dx"], r32["dx"], out_mode(dt))
    check("attn_spatial_bwd", dt, tag + " dw7", kr["dw7"], r64["dw7"], r32["dw7"])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("k", [7, 3])
@pytest.mark.parametrize("with_mul", [False, True])
def test_spatial_attention(dt, k, with_mul):
    g = gen(500 + k)
    N, H, W, C = 2, 5, 7, 16
    x, dout = rnd(g, dt, N, H, W, C), rnd(g, dt, N, H, W, C)
    w7, dw_old = rnd32(g, 2, k, k, scale=0.3), rnd32(g, 2, k, k)
    mul = chan_table(g, N, C) if with_mul else None
    check_spatial(dt, f"k={k} mul={with_mul}", x, w7, mul, dout, dw_old, run_spatial(dt, x, w7, mul, dout, dw_old))


def test_spatial_attention_tied_maximum():
    """Two channels share the maximum at every pixel: the saved argmax and the gradient take the first."""
    g = gen(510)
    N, H, W, C = 2, 5, 7, 16
    x, dout = rnd(g, "bf16", N, H, W, C), rnd(g, "bf16", N, H, W, C)
    top = x.max(dim=-1).values + 1.0
    hi = torch.randint(4, C, (N, H, W), generator=g)
    lo = torch.randint(0, 4, (N, H, W), generator=g)
    x.scatter_(-1, hi.unsqueeze(-1), top.unsqueeze(-1))
    x.scatter_(-1, lo.unsqueeze(-1), top.unsqueeze(-1))
    x = x.to(torch.bfloat16).double()
    assert torch.equal(O.first_argmax(x), lo) and torch.equal(x.gather(-1, hi.unsqueeze(-1)), x.gather(-1, lo.unsqueeze(-1)))
    w7, dw_old = rnd32(g, 2, 7, 7, scale=0.3), rnd32(g, 2, 7, 7)
    check_spatial("bf16", "tied", x, w7, None, dout, dw_old, run_spatial("bf16", x, w7, None, dout, dw_old))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("H", [64, 65])
def test_spatial_attention_sum_rows_threshold(dt, H):
    """dw7 is summed over N * H partial rows by sum_rows: 64 rows take its single kernel, 65 the split path (R = 64,
    S = 2) with a last split of one row."""
    g = gen(520 + H)
    N, W, C, k = 1, 3, 8, 3
    x, dout = rnd(g, dt, N, H, W, C), rnd(g, dt, N, H, W, C)
    w7, dw_old = rnd32(g, 2, k, k, scale=0.3), rnd32(g, 2, k, k)
    check_spatial(dt, f"rows={N * H}", x, w7, None, dout, dw_old, run_spatial(dt, x, w7, None, dout, dw_old))


# ------------------------------------------------------------------------------------------- 6. channel attention, SE
CA_SHAPES = [(3, 20, 16, 2), (2, 130, 24, 6)]
# input seeds whose ReLU hidden units are mixed live / dead with one live in every image (asserted in channel_case)
CA_SEEDS = {CA_SHAPES[0]: 604, CA_SHAPES[1]: 601}


def run_channel(dt, se, x, w1, b1, w2, b2, act, beta, mul, dout, old):
    N, HW, C = x.shape
    Cr = w1.shape[0]
    T = DTYPES[dt]
    xd, dd = up(x, T), up(dout, T)
    w1d, w2d = up(w1), up(w2)
    md = None if mul is None else up(mul)
    gap, hpre, gate = torch.empty(N, C, device=DEV), torch.empty(N, Cr, device=DEV), torch.empty(N, C, device=DEV)
    out, dx = torch.empty_like(xd), torch.empty_like(xd)
    gr = {n: up(old[n]) for n in old}
    if se:
        b1d, b2d = up(b1), up(b2)
        ws = workspace(lib().hiseg_se_train_ws(N, C, Cr))
        ok(lib().hiseg_se_train_fwd(HD[dt], ptr(xd), N, HW, C, ptr(w1d), ptr(b1d), Cr, ptr(w2d), ptr(b2d), act,
                                    ptr(ws), ptr(gap), ptr(hpre), ptr(gate), ptr(out), stream()), "se_train_fwd")
        ok(lib().hiseg_se_train_bwd(HD[dt], ptr(xd), N, HW, C, ptr(w1d), Cr, ptr(w2d), act, ptr(gap), ptr(hpre),
                                    ptr(gate), ptr(dd), ptr(dx), ptr(ws), ptr(gr["dw1"]), ptr(gr["db1"]),
                                    ptr(gr["dw2"]), ptr(gr["db2"]), stream()), "se_train_bwd")
    else:
        ws = workspace(lib().hiseg_attn_channel_ws(N, C, Cr))
        ok(lib().hiseg_attn_channel_train_fwd(HD[dt], ptr(xd), N, HW, C, ptr(w1d), Cr, ptr(w2d), act, beta, ptr(md),
                                              ptr(ws), ptr(gap), ptr(hpre), ptr(gate), ptr(out), stream()),
           "attn_channel_train_fwd")
        ok(lib().hiseg_attn_channel_bwd(HD[dt], ptr(xd), N, HW, C, ptr(w1d), Cr, ptr(w2d), act, beta, ptr(md),
                                        ptr(gap), ptr(hpre), ptr(gate), ptr(dd), ptr(dx), ptr(ws), ptr(gr["dw1"]),
                                        ptr(gr["dw2"]), stream()), "attn_channel_bwd")
    return dict(gap=gap, hpre=hpre, gate=gate, out=out, dx=dx, **gr)


def channel_case(dt, se, shape, act, beta, with_mul, seed):
    g = gen(seed)
    N, HW, C, Cr = shape
    x, dout = rnd(g, dt, N, HW, C), rnd(g, dt, N, HW, C)
    w1, w2 = rnd32(g, Cr, C, scale=0.5), rnd32(g, C, Cr, scale=0.5)
    b1, b2 = (rnd32(g, Cr, scale=0.3), rnd32(g, C, scale=0.3)) if se else (None, None)
    mul = chan_table(g, N, C) if with_mul else None
    if act == O.ACT_RELU:     # the hidden pre-activation stays away from the ReLU kink (checked in float64), and
        hp = O.channel_attention(x, w1, b1, w2, b2, act, beta, mul)["hpre"]     # every image has a live hidden unit:
        assert hp.abs().min() >= 1e-3, hp.abs().min()                          # each contributes to dw1
        assert (hp > 0).any(dim=1).all() and (hp < 0).any()
    old = {"dw1": rnd32(g, Cr, C), "dw2": rnd32(g, C, Cr)}
    if se:
        old.update(db1=rnd32(g, Cr), db2=rnd32(g, C))
    kr = run_channel(dt, se, x, w1, b1, w2, b2, act, beta, mul, dout, old)
    r64, r32 = both(O.channel_attention, x, w1, b1, w2, b2, act, beta, mul, dout, old)
    fwd, bwd = ("se_train_fwd", "se_train_bwd") if se else ("attn_channel_train_fwd", "attn_channel_bwd")
    tag = f"{shape} act={act}"
    for n in ("gap", "hpre", "gate"):
        check(fwd, dt, f"{tag} {n}", kr[n], r64[n], r32[n])
    check(fwd, dt, f"{tag} out", kr["out"], r64["out"], r32["out"], out_mode(dt))
    check(bwd, dt, f"{tag} dx", kr["dx"], r64["dx"], r32["dx"], out_mode(dt))
    for n in old:
        check(bwd, dt, f"{tag} {n}", kr[n], r64[n], r32[n])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", CA_SHAPES)
@pytest.mark.parametrize("act,beta", [(O.ACT_RELU, 1.0), (O.ACT_SWISH, 1.5)])
@pytest.mark.parametrize("with_mul", [False, True])
def test_channel_attention(dt, shape, act, beta, with_mul):
    channel_case(dt, False, shape, act, beta, with_mul, CA_SEEDS[shape])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", CA_SHAPES)
def test_squeeze_excite(dt, shape):
    channel_case(dt, True, shape, O.ACT_SILU, 1.0, False, 650 + shape[1])


# ------------------------------------------------------------------------------------------- 7. upsample_bg_fg head, pw2
def ubf_inputs(g, dt, N, h, w, Ct):
    p = {"ut_w": rnd32(g, 2, 32, 2, 2, scale=0.5), "ut_b": rnd32(g, 32, scale=0.1),
         "gamma": (1 + 0.2 * torch.randn(32, generator=g, dtype=torch.float64)).float().double(),
         "beta": rnd32(g, 32, scale=0.2), "u1_w": rnd32(g, 2, 32, scale=0.3), "u1_b": rnd32(g, 2, scale=0.1)}
    low = rnd32(g, N, h, w, 2)
    tfeat = rnd(g, dt, N, 2 * h, 2 * w, Ct)
    t_w, t_b = rnd32(g, 2, Ct, scale=0.3), rnd32(g, 2, scale=0.1)
    grads = tuple(rnd32(g, N, c, 2 * h, 2 * w) for c in (3, 2, 2))
    running = (rnd32(g, 32, scale=0.3), (0.5 + torch.rand(32, generator=g, dtype=torch.float64)).float().double())
    old = {"d" + n: rnd32(g, *p[n].shape) for n in O.UBF_PARAMS}
    return low, p, tfeat, t_w, t_b, grads, running, old


# input seeds per (N, layernorm) whose ReLU pre-activations all keep |pre| >= 1e-4 (asserted in the test, in float64)
UBF_SEEDS = {(2, 0): 700, (2, 1): 700, (1, 0): 710, (1, 1): 711}
UBF_CASES = [(shape, ln, O.ACT_RELU, 1.0, ext) for shape in ((2, 3, 5), (1, 1, 2)) for ln in (0, 1)
             for ext in (False, True)] + [((2, 3, 5), ln, O.ACT_SWISH, 1.5, True) for ln in (0, 1)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape,ln,act,beta,ext", UBF_CASES)
def test_ubf_head(dt, shape, ln, act, beta, ext):
    N, h, w = shape
    Ct, H, W = 16, 2 * shape[1], 2 * shape[2]
    P = N * H * W
    low, p, tfeat, t_w, t_b, grads, running, old = ubf_inputs(gen(UBF_SEEDS[N, ln]), dt, N, h, w, Ct)
    g3 = (grads[0], grads[1] if ext else None, grads[2] if ext else None)
    r64, r32 = both(O.ubf_head, low, p, tfeat, t_w, t_b, act, beta, ln, running=running, grads=g3, old=old)
    if act == O.ACT_RELU:     # an unambiguous live pattern: no pre-activation near the kink (float64, on the CPU)
        assert r64["pre"].abs().min() >= 1e-4, r64["pre"].abs().min()
        assert torch.equal(r64["pre"] > 0, r32["pre"] > 0)
    d = L.UbfDesc()
    d.dtype, d.N, d.h, d.w, d.Ct = HD[dt], N, h, w, Ct
    d.low = up(low)
    for n in ("ut_w", "ut_b", "gamma", "beta", "u1_w", "u1_b"):
        setattr(d, n, up(p[n]))
    ns = N if ln else 32
    d.mean, d.invstd = torch.empty(ns, device=DEV), torch.empty(ns, device=DEV)
    d.scale, d.shift = torch.empty(N * 32 if ln else 32, device=DEV), torch.empty(N * 32 if ln else 32, device=DEV)
    d.tfeat, d.t_w, d.t_b = up(tfeat, DTYPES[dt]), up(t_w), up(t_b)
    d.logits, d.bgfg, d.tn = (torch.empty(N, c, H, W, device=DEV) for c in (3, 2, 2))
    d.act, d.act_beta, d.layernorm = act, beta, ln
    rm, rv = up(running[0]), up(running[1])
    ws = workspace(lib().hiseg_ubf_ws(N))
    ok(lib().hiseg_ubf_train_fwd(ctypes.byref(d), 1e-5, 0.1, ptr(rm), ptr(rv), ptr(ws), stream()), "ubf_train_fwd")
    held = d.held()
    tag = f"{shape} ln={ln} act={act} ext={ext}"
    for n in ("logits", "bgfg", "tn", "mean", "invstd", "scale", "shift"):
        check("ubf_train_fwd", dt, f"{tag} {n}", held[n], r64[n], r32[n])
    if ln:
        assert torch.equal(rm.cpu().double(), running[0]) and torch.equal(rv.cpu().double(), running[1])
    else:
        check("ubf_train_fwd", dt, f"{tag} running_mean", rm, r64["running_mean"], r32["running_mean"])
        check("ubf_train_fwd", dt, f"{tag} running_var", rv, r64["running_var"], r32["running_var"])
    gr = L.UbfGrads()
    for n in O.UBF_PARAMS:
        setattr(gr, "d" + n, up(old["d" + n]))
    dl = [None if t is None else up(t) for t in g3]
    db_buf, dtn_out = torch.empty(P, 2, device=DEV), torch.empty(P, 2, device=DEV)
    dlow = torch.empty(N, h, w, 2, device=DEV)
    ok(lib().hiseg_ubf_train_bwd(ctypes.byref(d), ptr(dl[0]), ptr(dl[1]), ptr(dl[2]), ptr(db_buf), ptr(dtn_out),
                                 ptr(dlow), ptr(ws), ctypes.byref(gr), stream()), "ubf_train_bwd")
    check("ubf_train_bwd", dt, f"{tag} dlow", dlow, r64["dlow"], r32["dlow"])
    check("ubf_train_bwd", dt, f"{tag} dtn_out", dtn_out, r64["dtn_out"], r32["dtn_out"])
    for n in O.UBF_PARAMS:
        check("ubf_train_bwd", dt, f"{tag} d{n}", gr.held()["d" + n], r64["d" + n], r32["d" + n])


@pytest.mark.parametrize("dt,Ct", [("f32", c) for c in (8, 16, 24, 40)] + [("bf16", c) for c in (8, 16, 24, 40)])
@pytest.mark.parametrize("P", [120, 7])
def test_pw2_bwd(dt, Ct, P):
    g = gen(750 + Ct)
    tfeat, dtn, w = rnd(g, dt, P, Ct), rnd32(g, P, 2), rnd32(g, 2, Ct, scale=0.5)
    old_dw, old_db = rnd32(g, 2, Ct), rnd32(g, 2)
    td, dd, wd = up(tfeat, DTYPES[dt]), up(dtn), up(w)
    dtd = torch.empty_like(td)
    dw, db = up(old_dw), up(old_db)
    ws = workspace(lib().hiseg_pw2_ws(Ct))
    ok(lib().hiseg_pw2_bwd(HD[dt], ptr(td), P, Ct, ptr(dd), ptr(wd), ptr(dtd), ptr(ws), ptr(dw), ptr(db), stream()),
       "pw2_bwd")
    (dt64, dw64, db64), (dt32, dw32, db32) = both(O.pw2_bwd, tfeat, dtn, w, old_dw, old_db)
    check("pw2_bwd", dt, f"Ct={Ct} P={P} dt", dtd, dt64, dt32, out_mode(dt))
    check("pw2_bwd", dt, f"Ct={Ct} P={P} dw", dw, dw64, dw32)
    check("pw2_bwd", dt, f"Ct={Ct} P={P} db", db, db64, db32)


# the smallest case of each family that owns a workspace, forward and backward, with every oracle check of its test
WS_CASES = {
    "spatial": lambda dt: test_spatial_attention(dt, 3, False),
    "channel": lambda dt: test_channel_attention(dt, CA_SHAPES[0], O.ACT_RELU, 1.0, False),
    "se": lambda dt: test_squeeze_excite(dt, CA_SHAPES[0]),
    "ubf-bn-n1": lambda dt: test_ubf_head(dt, (1, 1, 2), 0, O.ACT_RELU, 1.0, False),
    "ubf-ln-n1": lambda dt: test_ubf_head(dt, (1, 1, 2), 1, O.ACT_RELU, 1.0, False),
    "ubf-bn-n2": lambda dt: test_ubf_head(dt, (2, 3, 5), 0, O.ACT_RELU, 1.0, False),
    "ubf-ln-n2": lambda dt: test_ubf_head(dt, (2, 3, 5), 1, O.ACT_RELU, 1.0, False),
    "pw2": lambda dt: test_pw2_bwd(dt, 8, 7),
}


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("family", WS_CASES)
def test_workspace_extents(monkeypatch, dt, family):
    """The *_ws size is enough and is respected: on a NaN-filled workspace of exactly that size the results still meet
    the oracle (nothing is read before it is written), and the 64 floats behind it keep their bits."""
    guarded = GuardedWorkspaces()
    monkeypatch.setattr(sys.modules[__name__], "workspace", guarded)
    WS_CASES[family](dt)
    guarded.assert_guards_untouched()


# ------------------------------------------------------------------------------------------- 8. RoIAlign -> output_conv
ROIS = [[0, 0.20, 0.25, 0.70, 0.80],      # inside the map
        [0, -0.15, -0.20, 0.40, 0.50],    # clipped on the left and top (negative coordinates)
        [0, 0.55, 0.45, 1.20, 1.25],      # past the right and bottom edges
        [0, 1.40, 1.50, 1.90, 2.10],      # wholly outside: contributes 0 to dw and, its taps being 0, to db
        [0, 0.45, 0.55, 0.45, 0.55],      # zero area
        [1, 0.10, 0.05, 0.90, 0.95]]      # image 1


@pytest.mark.parametrize("aligned", [0, 1])
@pytest.mark.parametrize("gdt", ["f32", "bf16"])
def test_roi_align_bwd_affine(aligned, gdt):
    g = gen(800)
    B, H, W, oh, ow, N = 2, 9, 13, 4, 6, len(ROIS)
    u = rnd32(g, B, 1, H, W)
    rois = torch.tensor(ROIS, dtype=torch.float32).double()
    gy = rnd(g, gdt, N, oh, ow, 2)
    old_dw, old_db = rnd32(g, 2), rnd32(g, 2)
    cs = 2 if gdt == "f32" else 8          # the engine hands over the padded bf16 activation
    vg = View(gy.reshape(-1, 2), DTYPES[gdt], cs, 0)
    d = L.RoiAlignDesc()
    d.feat, d.B, d.C, d.H, d.W = up(u), B, 1, H, W
    d.rois, d.N, d.oh, d.ow = up(rois), N, oh, ow
    d.scale_h, d.scale_w, d.aligned = float(H), float(W), aligned
    d.aff_w, d.aff_b, d.n_aff = up(torch.tensor([0.7, -1.3])), up(torch.tensor([0.2, -0.4])), 2
    ws = torch.empty(lib().hiseg_roi_align_ws(N), device=DEV)
    dw, db = up(old_dw), up(old_db)
    ok(lib().hiseg_roi_align_bwd_affine(ctypes.byref(d), ptr(vg.t), HD[gdt], cs, 0, ptr(ws), ptr(dw), ptr(db),
                                        stream()), "roi_align_bwd_affine")
    (dw64, db64), (dw32, db32) = both(O.roi_align_bwd_affine, u, rois, gy, oh, ow, float(H), float(W), aligned,
                                      old_dw, old_db)
    check("roi_align_bwd_affine", gdt, f"aligned={aligned} dw", dw, dw64, dw32)
    check("roi_align_bwd_affine", gdt, f"aligned={aligned} db", db, db64, db32)
    vg.assert_unchanged()


# ------------------------------------------------------------------------------------------- 9. LayerNorm2d
#            N  HW  C  layout   act beta   res    mul    dres_acc dcb    accp
LN_CASES = [(2, 12, 8, "dense", 0, 1.0, False, False, None, False, 0),      # sp = 1
            (1, 80, 8, "dense", 4, 1.0, True, True, 0, True, 1),            # sp = 5
            (3, 35, 5, "dense", 5, 0.75, True, False, 1, True, 0),          # scalar path
            (2, 12, 8, "off3", 4, 1.0, False, True, None, True, 1)]         # unaligned view


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,HW,C,lay,act,beta,res,with_mul,dres_acc,dcb,accp", LN_CASES)
def test_layernorm2d(dt, N, HW, C, lay, act, beta, res, with_mul, dres_acc, dcb, accp):
    g = gen(900 + HW)
    P = N * HW
    z, dy = rnd(g, dt, N, HW, C), rnd(g, dt, N, HW, C)
    gamma = (1 + 0.2 * torch.randn(C, generator=g, dtype=torch.float64)).float().double()
    bt = rnd32(g, C, scale=0.2)
    resid = rnd(g, dt, N, HW, C) if res else None
    mul = chan_table(g, N, C) if with_mul else None
    dres_old, dz_old = rnd(g, dt, N, HW, C), rnd(g, dt, N, HW, C)
    old = {n: rnd32(g, C) for n in ("dgamma", "dbeta", "dconv_bias")}
    vz, vdy = view(z.reshape(P, C), dt, lay), view(dy.reshape(P, C), dt, lay)
    vdz = view(dz_old.reshape(P, C), dt, lay)
    vres = view(resid.reshape(P, C), dt, lay) if res else None
    vdres = view(dres_old.reshape(P, C), dt, lay) if dres_acc is not None else None
    gd, bd = up(gamma), up(bt)
    ws = torch.empty(lib().hiseg_ln_ws(N, HW, C), device=DEV)
    mean, invstd = torch.empty(N, device=DEV), torch.empty(N, device=DEV)
    scale, shift = torch.empty(N, C, device=DEV), torch.empty(N, C, device=DEV)
    ok(lib().hiseg_ln_fwd_stats(HD[dt], ptr(vz.t), N, HW, C, vz.cstride, vz.coff, ptr(gd), ptr(bd), 1e-5, ptr(ws),
                                ptr(mean), ptr(invstd), ptr(scale), ptr(shift), stream()), "ln_fwd_stats")
    r64, r32 = both(O.layernorm2d, z, gamma, bt, 1e-5, act, beta, resid, mul, dy)
    tag = f"N={N} HW={HW} C={C} {lay} act={act}"
    for n, k in (("mean", mean), ("invstd", invstd), ("scale", scale), ("shift", shift)):
        check("ln_fwd_stats", dt, f"{tag} {n}", k, r64[n], r32[n])
    d = L.LnBwdDesc()
    d.dtype, d.N, d.HW, d.C = HD[dt], N, HW, C
    d.dy, d.dy_cstride, d.dy_coff = vdy.t, vdy.cstride, vdy.coff
    d.z, d.z_cstride, d.z_coff = vz.t, vz.cstride, vz.coff
    if res:
        d.residual, d.r_cstride, d.r_coff = vres.t, vres.cstride, vres.coff
    if with_mul:
        d.chan_mul = up(mul)
    d.act, d.act_beta = act, beta
    d.mean, d.invstd, d.scale, d.shift, d.gamma = mean, invstd, scale, shift, gd
    d.dgamma, d.dbeta = up(old["dgamma"]), up(old["dbeta"])
    if dcb:
        d.dconv_bias = up(old["dconv_bias"])
    d.accumulate_params = accp
    d.dz, d.dz_cstride, d.dz_coff = vdz.t, vdz.cstride, vdz.coff
    if vdres is not None:
        d.dres, d.dres_cstride, d.dres_coff, d.dres_accumulate = vdres.t, vdres.cstride, vdres.coff, dres_acc
    d.ws = ws
    ok(lib().hiseg_ln_bwd(ctypes.byref(d), stream()), "ln_bwd")
    check("ln_bwd", dt, f"{tag} dz", vdz.live(), r64["dz"].reshape(P, C), r32["dz"].reshape(P, C), out_mode(dt))
    vdz.assert_dead_untouched()
    if vdres is not None:
        a, b = r64["dres"].reshape(P, C), r32["dres"].reshape(P, C)
        if dres_acc:
            a, b = a + dres_old.reshape(P, C), b + dres_old.reshape(P, C).float()
        check("ln_bwd", dt, f"{tag} dres", vdres.live(), a, b, out_mode(dt, dres_acc), dres_old.reshape(P, C))
        vdres.assert_dead_untouched()
    for n in ("dgamma", "dbeta") + (("dconv_bias",) if dcb else ()):
        a, b = r64[n], r32[n]
        if accp:
            a, b = a + old[n], b + old[n].float()
        check("ln_bwd", dt, f"{tag} {n}", d.held()[n], a, b)


# ------------------------------------------------------------------------------------------- 10. dropout masks
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_dropout_masks(p):
    N, C = 3, 70
    n = N * C
    seed, base, offset = 0x1234_5678_9ABC, 2 ** 40 + 12345, 17
    out = torch.full((n + 46,), SENTINEL, device=DEV)
    ok(lib().hiseg_dropout2d_mask(N, C, p, seed, ptr(out), stream()), "dropout2d_mask")
    assert np.array_equal(out[:n].cpu().numpy(), O.dropout2d_mask(n, p, seed))
    assert (out[n:] == SENTINEL).all()
    sb = torch.tensor([base], dtype=torch.int64, device=DEV)
    out2 = torch.full((n + 46,), SENTINEL, device=DEV)
    ok(lib().hiseg_dropout2d_mask_dev(N, C, p, ptr(sb), offset, ptr(out2), stream()), "dropout2d_mask_dev")
    assert np.array_equal(out2[:n].cpu().numpy(), O.dropout2d_mask_dev(n, p, base, offset))
    assert (out2[n:] == SENTINEL).all()
    ok(lib().hiseg_seed_advance(ptr(sb), stream()), "seed_advance")
    assert sb.item() == base + 1
    ok(lib().hiseg_dropout2d_mask_dev(N, C, p, ptr(sb), offset, ptr(out2), stream()), "dropout2d_mask_dev")
    assert np.array_equal(out2[:n].cpu().numpy(), O.dropout2d_mask_dev(n, p, base + 1, offset))
    if p > 0:
        keep = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
        for m in (out[:n], out2[:n]):
            assert set(m.cpu().unique().tolist()) == {0.0, keep}
        assert not np.array_equal(O.dropout2d_mask_dev(n, p, base, offset), O.dropout2d_mask_dev(n, p, base + 1, offset))
    else:
        assert (out[:n] == 1).all() and (out2[:n] == 1).all()
