"""Plain torch restatement of train-mode BatchNorm as include/hiseg_train.h declares it: hiseg_bn_stats,
hiseg_bn_finalize / _finalize_n, hiseg_bn_apply and hiseg_bn_bwd.  Written from the header's formulas, not from
csrc/bn_train.hip.

Every function is dtype-generic (it computes in the dtype of its floating inputs), so the GPU tests evaluate each
one in float64 -- the reference -- and in float32, whose distance from the float64 result (`e32`) is the yardstick
of the bounds.  Activations are [P][C] (the live channels of an NHWC view); chan_mul and per-sample tables are
[N][C], pixel p belongs to image p // HW.
"""
import torch

from train_kernel_oracle import ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SILU, ACT_GELU, ACT_SWISH, act_bwd_pre, act_fn

SMOOTH = (ACT_SILU, ACT_GELU, ACT_SWISH)


def bn_stats(z):
    """Per-channel (n, mean, M2) of z[P][C]: count, mean and sum of squared deviations."""
    P = z.shape[0]
    mean = z.sum(0) / P
    return torch.full_like(mean, P), mean, ((z - mean) ** 2).sum(0)


def merge(partials):
    """Chan's merge of [S][3][C] partials (rows n, mean, M2; empty splits have n = 0) -> (n, mean, M2)."""
    n, mean, m2 = (partials[0][i].clone() for i in range(3))
    for s in range(1, partials.shape[0]):
        nb, mb, qb = partials[s]
        nt = n + nb
        w = torch.where(nt > 0, nb / nt.clamp_min(1), torch.zeros_like(nt))
        d = mb - mean
        d = torch.where(nb > 0, d, torch.zeros_like(d))
        mean = mean + d * w
        m2 = m2 + torch.where(nb > 0, qb, torch.zeros_like(qb)) + d * d * n * w
        n = nt
    return n, mean, m2


def bn_finalize(n, mean, m2, gamma, beta, eps, momentum, rm, rv, P):
    """mean, invstd, the fold scale = gamma invstd, shift = beta - mean gamma invstd, and the running update (the
    unbiased variance when P > 1, the biased one when P == 1).  gamma / beta None: 1 / 0."""
    var = m2 / n
    invstd = 1.0 / torch.sqrt(var + eps)
    g = torch.ones_like(mean) if gamma is None else gamma
    b = torch.zeros_like(mean) if beta is None else beta
    scale = g * invstd
    shift = b - mean * g * invstd
    rm2 = None if rm is None else (1.0 - momentum) * rm + momentum * mean
    rv2 = None if rv is None else (1.0 - momentum) * rv + momentum * (var * P / (P - 1) if P > 1 else var)
    return mean, invstd, scale, shift, rm2, rv2


def _rows(table, HW, P):
    return table.repeat_interleave(HW, dim=0)[:P]


def bn_apply(z, scale, shift, residual, act, act_beta, chan_mul, HW, per_sample):
    """y = act(z scale + shift [+ residual]) * chan_mul; scale / shift [C], or [N][C] with per_sample."""
    P = z.shape[0]
    if per_sample:
        scale, shift = _rows(scale, HW, P), _rows(shift, HW, P)
    v = z * scale + shift
    if residual is not None:
        v = v + residual
    y = act_fn(v, act, act_beta)
    if chan_mul is not None:
        y = y * _rows(chan_mul, HW, P)
    return y


def deriv_source(act, has_fwd, has_residual, wants_dres):
    """Where the header takes act'(.): 'none', 'y' (the stored output), 'pre' (z fwd_scale + fwd_shift + residual)
    or 'fold' (SiLU without the forward's tables: xhat gamma + beta)."""
    if act == ACT_NONE:
        return "none"
    if has_fwd and (act in SMOOTH or (act == ACT_RELU and (not wants_dres or has_residual))):
        return "pre"
    if act == ACT_SILU:
        return "fold"
    if act in (ACT_RELU, ACT_SIGMOID):
        return "y"
    raise ValueError("GELU / Swish need fwd_scale / fwd_shift")


def bn_g(dy, z, mean, invstd, gamma, beta, act, act_beta, chan_mul, HW, y=None, fwd_scale=None, fwd_shift=None,
         residual=None, wants_dres=False):
    """g = dy * chan_mul * act'(.) and xhat = (z - mean) invstd."""
    P = z.shape[0]
    xhat = (z - mean) * invstd
    g = dy if chan_mul is None else dy * _rows(chan_mul, HW, P)
    src = deriv_source(act, fwd_scale is not None, residual is not None, wants_dres)
    if src == "pre":
        v = z * fwd_scale + fwd_shift
        if residual is not None:
            v = v + residual
        g = act_bwd_pre(g, v, act, act_beta)
    elif src == "fold":
        v = xhat * (1.0 if gamma is None else gamma) + (0.0 if beta is None else beta)
        g = act_bwd_pre(g, v, act, act_beta)
    elif src == "y":
        g = torch.where(y > 0, g, torch.zeros_like(g)) if act == ACT_RELU else g * y * (1 - y)
    return g, xhat


def bn_bwd_from_sums(g, xhat, s1, s2, invstd, gamma, P):
    """dz from the two per-channel sums s1 = sum g, s2 = sum g xhat."""
    k = invstd if gamma is None else gamma * invstd
    return k * (g - s1 / P - xhat * s2 / P)


def bn_bwd(dy, z, mean, invstd, gamma, beta, act, act_beta, chan_mul, HW, y=None, fwd_scale=None, fwd_shift=None,
           residual=None, wants_dres=False):
    """dz, dres (= g), dgamma (= sum g xhat), dbeta (= sum g), dconv_bias (= sum dz)."""
    P = z.shape[0]
    g, xhat = bn_g(dy, z, mean, invstd, gamma, beta, act, act_beta, chan_mul, HW, y, fwd_scale, fwd_shift, residual,
                   wants_dres)
    s1, s2 = g.sum(0), (g * xhat).sum(0)
    dz = bn_bwd_from_sums(g, xhat, s1, s2, invstd, gamma, P)
    return dz, g, s2, s1, dz.sum(0)
