"""tests/bn_kernel_oracle.py against float64 torch (F.batch_norm in training mode plus autograd, F.layer_norm for the
per-sample tables), and the exactness premise of every exact case of tests/test_gpu_bn_kernels.py, proved on the CPU
from that module's case tables.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_kernel_oracle as B
import test_gpu_bn_kernels as G
from train_kernel_oracle import act_fn

pytestmark = []          # (the imported module's gpu mark does not apply here)

N, H, W, C = 3, 5, 4, 6
HW, P = H * W, N * H * W
EPS, MOM = 1e-5, 0.1
ACTS = [(0, 1.0), (1, 1.0), (2, 1.0), (3, 1.0), (4, 1.0), (5, 1.5)]


def nchw(t):
    return t.reshape(N, H, W, -1).permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).reshape(P, -1)


def close(a, b, tol=1e-11):
    assert (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item()), (a - b).abs().max().item()


@pytest.mark.parametrize("act,beta", ACTS)
@pytest.mark.parametrize("with_res,with_mul", [(False, False), (True, True), (True, False), (False, True)])
def test_oracle_matches_batch_norm_autograd(act, beta, with_res, with_mul):
    g = torch.Generator().manual_seed(10 * act + with_res)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    z, dy, gamma, bet = 1.5 * r(P, C) + 0.3, r(P, C), 1 + 0.3 * r(C), 0.5 * r(C)
    res = r(P, C) if with_res else None
    mul = G.chan_table(g, N, C) if with_mul else None
    rm, rv = r(C), r(C).abs() + 0.5

    # torch: bias (the conv bias in front of BN) -> batch_norm -> + residual -> act -> * chan_mul
    zl, gl, bl, bias = (t.clone().requires_grad_(True) for t in (z, gamma, bet, torch.zeros(C, dtype=torch.float64)))
    rl = res.clone().requires_grad_(True) if with_res else None
    trm, trv = rm.clone(), rv.clone()
    v = nhwc(F.batch_norm(nchw(zl + bias), trm, trv, gl, bl, True, MOM, EPS))
    if with_res:
        v = v + rl
    y_t = act_fn(v, act, beta)
    if with_mul:
        y_t = y_t * mul.repeat_interleave(HW, dim=0)
    wrt = [zl, gl, bl, bias] + ([rl] if with_res else [])
    grads = torch.autograd.grad((y_t * dy).sum(), wrt)

    n, mean, m2 = B.bn_stats(z)
    mean, inv, scale, shift, rm2, rv2 = B.bn_finalize(n, mean, m2, gamma, bet, EPS, MOM, rm, rv, P)
    close(rm2, trm)
    close(rv2, trv)                       # the unbiased variance
    y = B.bn_apply(z, scale, shift, res, act, beta, mul, HW, 0)
    close(y, y_t.detach())

    # every source of act'(.) the header allows for this activation
    forms = [dict(fwd_scale=scale, fwd_shift=shift, residual=res, wants_dres=with_res)] if act else [dict()]
    if act == 1:
        forms.append(dict(y=y, wants_dres=with_res))
    if act == 2:                          # sigmoid is always taken from y, tables or not
        forms = [dict(y=y, wants_dres=with_res), dict(y=y, fwd_scale=scale, fwd_shift=shift, wants_dres=with_res)]
    if act == 3 and not with_res:
        forms.append(dict())              # SiLU folds xhat gamma + beta itself
    for kw in forms:
        if act == 2 and with_mul:
            continue                      # sigmoid' from y needs the unscaled output
        dz, dres, dgamma, dbeta, dcb = B.bn_bwd(dy, z, mean, inv, gamma, bet, act, beta, mul, HW, **kw)
        close(dz, grads[0])
        close(dgamma, grads[1])
        close(dbeta, grads[2])
        close(dcb, grads[3], 1e-9)
        if with_res:
            close(dres, grads[4])


def test_gamma_beta_none_and_biased_variance_at_one_pixel():
    z = torch.tensor([[1.5, -2.0]], dtype=torch.float64)
    n, mean, m2 = B.bn_stats(z)
    rv = torch.tensor([2.0, 3.0], dtype=torch.float64)
    mean, inv, scale, shift, _, rv2 = B.bn_finalize(n, mean, m2, None, None, EPS, MOM, None, rv, 1)
    assert torch.equal(m2, torch.zeros(2, dtype=torch.float64))
    close(inv, torch.full((2,), EPS ** -0.5, dtype=torch.float64))
    close(scale, inv)
    close(shift, -z[0] * inv)
    close(rv2, 0.9 * rv)                  # var = 0, biased: P / (P - 1) would divide by zero


def test_per_sample_tables_match_layer_norm():
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    z, w, b = r(P, C) + 0.4, 1 + 0.3 * r(C), r(C)
    x = nchw(z)
    ref = F.layer_norm(x, x.shape[1:], eps=EPS) * w.view(1, C, 1, 1) + b.view(1, C, 1, 1)
    mu = x.mean(dim=(1, 2, 3))
    inv = 1.0 / torch.sqrt(x.var(dim=(1, 2, 3), unbiased=False) + EPS)
    scale = w[None] * inv[:, None]
    shift = b[None] - mu[:, None] * scale
    close(B.bn_apply(z, scale, shift, None, 0, 1.0, None, HW, 1), nhwc(ref))


def test_merge_is_the_statistics_of_the_whole():
    g = torch.Generator().manual_seed(4)
    z = torch.randn(50, C, generator=g, dtype=torch.float64) * 2 + 1
    cuts = [0, 7, 7, 20, 21, 50]          # one empty split
    rows = torch.zeros(len(cuts) - 1, 3, C, dtype=torch.float64)
    for s in range(len(cuts) - 1):
        seg = z[cuts[s]:cuts[s + 1]]
        if len(seg):
            rows[s, 0], rows[s, 1], rows[s, 2] = B.bn_stats(seg)
    for a, b in zip(B.merge(rows), B.bn_stats(z)):
        close(a, b)


def test_path_decode():
    from hiseg import _lib as L
    assert L.bn_path_decode(-1) is None
    d = L.bn_path_decode(3 | 4 | 8 | (2 << 5) | 128)
    assert d == dict(entry="bwd", vec=True, par=True, premerge=False, mode="relu_pre", reduce=True, u2=False)
    assert L.bn_path_decode(1 | 16)["premerge"] and L.bn_path_decode(2 | 256)["u2"]


# ------------------------------------------------------------------------------------------- exactness premises
def same_in_f32(fn, *args, **kw):
    """The float32 evaluation equals the float64 one bit for bit, and so does every intermediate the caller lists."""
    r64, r32 = G.both(fn, *args, **kw)
    r64, r32 = (r64, r32) if isinstance(r64, tuple) else ((r64,), (r32,))
    for a, b in zip(r64, r32):
        assert torch.equal(a, b.double())
    return r64


@pytest.mark.parametrize("dt,Cc,layout,per_sample", G.APPLY_EXACT)
def test_apply_exact_premise(dt, Cc, layout, per_sample):
    """z scale, + shift, + residual, ReLU, * chan_mul: every step is exact in f32 and the result is representable in
    the output dtype, so one rounding changes nothing."""
    z, res, scale, shift, mul = G.apply_exact_inputs(dt, Cc, per_sample)
    for t in (z, res):
        assert torch.equal(t, t.to(G.DTYPES[dt]).double())
    for act in (0, 1):
        for r, m in ((None, None), (res, mul), (res, None), (None, mul)):
            (y,) = same_in_f32(B.bn_apply, z, scale, shift, r, act, 1.0, m, G.HW_EX, per_sample)
            assert torch.equal(y, y.to(G.DTYPES[dt]).double())
    P_ = z.shape[0]
    sc = scale.repeat_interleave(G.HW_EX, 0)[:P_] if per_sample else scale
    assert torch.equal((z * sc).float().double(), z * sc)


def welford_f32(xs):
    n = np.float32(0)
    mean = np.float32(0)
    m2 = np.float32(0)
    for x in xs:
        n += np.float32(1)
        d = x - mean
        mean = mean + d * (np.float32(1) / n)        # the reciprocal form; d / n gives the same for d == 0 or n == 1
        m2 = m2 + d * (x - mean)
    return n, mean, m2


@pytest.mark.parametrize("dt,Cc,P_,layout", G.CONST_CASES)
def test_constant_channel_premise(dt, Cc, P_, layout):
    """Welford over a constant v: the first update gives mean = v exactly (v / 1), every later d is 0; a Chan merge of
    two such partials has d = 0.  v, v^2 n and 1 - momentum are exact in double, so the finalize is the header's."""
    v = np.float32(G.CONST_V)
    assert float(v) == G.CONST_V and torch.tensor(G.CONST_V).to(G.DTYPES[dt]).item() == G.CONST_V
    for count in (1, 2, 33, -(-P_ // G.splits_of(P_))):
        n, mean, m2 = welford_f32([v] * count)
        assert (n, mean, m2) == (count, v, 0)
    rows = torch.tensor([[[3.0], [G.CONST_V], [0.0]], [[0.0], [0.0], [0.0]], [[5.0], [G.CONST_V], [0.0]]])
    n, mean, m2 = B.merge(rows)
    assert (n.item(), mean.item(), m2.item()) == (8, G.CONST_V, 0)
    assert P_ * G.CONST_V ** 2 < 2 ** 53


@pytest.mark.parametrize("Cc", sorted({c for _, c in G.BWD_EXACT}))
@pytest.mark.parametrize("act,fwd,with_res,want_dres", G.BWD_EXACT_MODES)
def test_bwd_exact_premise(Cc, act, fwd, with_res, want_dres):
    """P is a power of two <= 64, dy, z, mean integers, invstd and gamma powers of two: g and xhat are multiples of
    1/2, every sum stays far below 2^24 granules in any order, the / P coefficients are dyadic and dz needs fewer than
    24 bits.  The float32 evaluation of the oracle therefore equals the float64 one bit for bit."""
    inp = G.bwd_exact_inputs(Cc, act, fwd, with_res)
    P_ = G.N_BX * G.HW_BX
    assert P_ & (P_ - 1) == 0 and P_ <= 64
    args = (inp["dy"], inp["z"], inp["mean"], inp["invstd"], inp["gamma"], inp["beta"], act, 1.0, inp["mul"], G.HW_BX)
    src = B.deriv_source(act, fwd, with_res, want_dres)
    kw = dict(y=inp["y"] if src == "y" else None, fwd_scale=inp["fwd_scale"], fwd_shift=inp["fwd_shift"],
              residual=inp["res"], wants_dres=want_dres)
    assert G.expected_mode(act, src) in ("none", "y", "relu_pre")
    for t in (inp["invstd"], inp["gamma"]):
        m, _ = torch.frexp(t.abs())
        assert torch.equal(m, torch.full_like(m, 0.5)), "not a power of two"
    if src == "pre":
        pre = inp["z"] * inp["fwd_scale"] + inp["fwd_shift"] + (inp["res"] if with_res else 0)
        assert pre.abs().min() >= 0.5 and torch.equal(pre.float().double(), pre)
    g, xh = same_in_f32(B.bn_g, *args, **kw)
    gran = 0.5
    for t in (g, xh, g * xh):
        assert torch.equal(t / gran, torch.round(t / gran))
        assert (t.abs().sum(0) / gran).max() < 2 ** 24
    dz, dres, dgamma, dbeta, dcb = same_in_f32(B.bn_bwd, *args, **kw)
    # dz before the power-of-two factor: multiples of 2^-8 below 2^24 granules
    core = dz / (inp["gamma"] * inp["invstd"])
    assert torch.equal(core * 256, torch.round(core * 256)) and (core.abs() * 256).max() < 2 ** 24
    # accumulating small integers keeps everything exact in the output dtypes' f32 arithmetic
    assert (dres.abs().max() + 3) < 2 ** 8 and torch.equal(dres, torch.round(dres))
