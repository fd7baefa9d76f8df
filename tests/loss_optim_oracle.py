"""Plain numpy restatement of the two ends of the training step, with no GPU code:

  loss       RefinedHierarchicalLoss as include/hiseg_loss.h declares it and the pass description at the top of
             csrc/train_loss.hip lays it out: the per-pixel target maps (boundary weight, raw and dilated contour
             target, five-iteration distance target), the class counts, the dynamic class weights and their EMA state
             (double[8]), every loss term with its clamp, the 16 outputs and the gradients with respect to the five
             inputs.  Written from the header and from oracle/train.py's reading of the reference, not from the kernel.
  optimiser  clip_grad_norm_ + torch.optim.AdamW on a flat parameter space with per-segment step counts
             (include/hiseg_train.h: hiseg_grad_norm_partials, hiseg_adamw_step_segmented / _segmented_dev, _guarded,
             hiseg_adamw_step).

Every evaluation takes `dt`: numpy.float64 is the reference; numpy.float32 evaluates the same formulas with every
operation rounded to f32 (numpy rounds after each array operation when all operands are f32), exp(x) formed as
exp2(float32(x * log2(e))) so it carries the argument rounding a fast exponential has, and sums taken in f32 in
numpy's fixed pairwise order.  The distance of the two (`e32`) only sizes the bounds of the GPU tests.

The per-batch class weight is an f32 value in either mode, as in the reference (the .item() of an f32 tensor); the
EMA over it is double, and the loss terms take the EMA as f32 again (the reference's weight tensor, the header's f32
weight outputs).
"""
import math

import numpy as np

F32, F64 = np.float32, np.float64
LOG2E = 1.4426950408889634

OUT_NAMES = ("total", "bgfg", "tn", "final", "cons", "dice", "ba", "contour", "dist", "acc", "iou", "w_bg", "w_fg",
             "w_t", "w_nt", "base_total")
NOUT = len(OUT_NAMES)            # HISEG_LOSS_NOUT + 1
CLAMP = 10.0
CFG_FLOATS = ("bg_weight", "fg_weight", "target_weight", "consistency_weight", "dice_weight", "ce_weight",
              "boundary_aware_weight", "contour_weight", "distance_weight")
CFG_INTS = ("use_dynamic_weights", "use_boundary_aware", "use_contour", "use_distance", "contour_ks")


def make_cfg(**kw):
    """The hiseg_loss_cfg fields as a dict, the float ones rounded to f32 (they are c_float arguments); defaults are the
    training script's weights with every term on and no dilation."""
    c = dict(bg_weight=1.5, fg_weight=1.5, target_weight=1.2, consistency_weight=0.3, dice_weight=1.0, ce_weight=1.0,
             boundary_aware_weight=0.1, contour_weight=0.1, distance_weight=0.1, use_dynamic_weights=1,
             use_boundary_aware=1, use_contour=1, use_distance=1, contour_ks=1)
    for k, v in kw.items():
        assert k in c, k
        c[k] = v
    for k in CFG_FLOATS:
        c[k] = float(F32(c[k]))
    return c


def state_init():
    """ema_bg, ema_fg, ema_t, ema_nt, tn_initialised, last_t, last_nt, calls"""
    return np.array([1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 1.0, 0.0], dtype=F64)


# ------------------------------------------------------------------------------------------------ target maps
def _shifts3(a, pad_value=None):
    """The nine 3x3-neighbourhood views of a[N][H][W]; outside the image: the nearest pixel, or pad_value."""
    if pad_value is None:
        p = np.pad(a, ((0, 0), (1, 1), (1, 1)), mode="edge")
    else:
        p = np.pad(a, ((0, 0), (1, 1), (1, 1)), mode="constant", constant_values=pad_value)
    H, W = a.shape[1:]
    return [p[:, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)]


def boundary_weight(tg, dt=F64):
    """2 where the 3x3 window, clipped to the image, holds at least two labels, else 1.  (Replicating the edge adds no
    label the clipped window lacks.)"""
    s = np.stack(_shifts3(tg))
    return np.where(s.max(0) != s.min(0), 2.0, 1.0).astype(dt)


def contour_raw(tg, dt=F64):
    """max(|dy|, |dx|) of the class-1 mask; the last row / column repeats the one before it (0 when H or W is 1)."""
    t = (tg == 1).astype(dt)
    N, H, W = t.shape
    dy, dx = np.zeros_like(t), np.zeros_like(t)
    if H > 1:
        dy[:, :-1] = np.abs(t[:, 1:] - t[:, :-1])
        dy[:, -1] = dy[:, -2]
    if W > 1:
        dx[:, :, :-1] = np.abs(t[:, :, 1:] - t[:, :, :-1])
        dx[:, :, -1] = dx[:, :, -2]
    return np.maximum(dy, dx)


def contour_target(tg, ks, dt=F64):
    """The raw contour for ks <= 1; else 1 where the zero-padded ks x ks box mean of the raw contour exceeds 0.1, taken
    with integer counts: 10 * count > ks * ks."""
    raw = contour_raw(tg, dt)
    if ks <= 1:
        return raw
    r = ks // 2
    N, H, W = raw.shape
    c = np.pad(raw.astype(np.int64), ((0, 0), (r + 1, r), (r + 1, r))).cumsum(1).cumsum(2)
    cnt = c[:, ks:ks + H, ks:ks + W] - c[:, :H, ks:ks + W] - c[:, ks:ks + H, :W] + c[:, :H, :W]
    return (10 * cnt > ks * ks).astype(dt)


def distance_target(tg, dt=F64):
    """d0 = (target == 1); five times d += (1 - d) * maxpool3(d) * 0.5 (the pool's window clipped to the image)."""
    d = (tg == 1).astype(dt)
    one, half = dt(1.0), dt(0.5)
    for _ in range(5):
        m = np.stack(_shifts3(d, -np.inf)).max(0)
        d = d + (one - d) * m * half
    return d


def class_counts(tg):
    """bg, fg, target, non-target pixel counts (double[4])."""
    return np.array([(tg == 0).sum(), (tg > 0).sum(), (tg == 1).sum(), (tg == 2).sum()], dtype=F64)


# ------------------------------------------------------------------------------------------------ class weights
def _clamp(v, lo, hi):
    return min(max(v, lo), hi)


def raw_class_weights(counts, target_weight):
    """The four per-batch weights before their clamp, as f32 values: tot / (2 max(c, 1)) [* target_weight for fg]."""
    bg, fg, tc, nt = (float(v) for v in counts)
    tot, ftot = bg + fg, tc + nt
    return (float(F32(tot / (2.0 * max(bg, 1.0)))),
            float(F32(F32(tot / (2.0 * max(fg, 1.0))) * F32(target_weight))),
            float(F32(ftot / (2.0 * max(tc, 1.0)))),
            float(F32(ftot / (2.0 * max(nt, 1.0)))))


def class_weights(cfg, counts, state):
    """-> (w_bg, w_fg, w_t, w_nt as doubles, target/non-target term active, new state).  `counts` are the counts the
    weights follow (this batch's, or the all-reduced ones)."""
    st = np.array(state, dtype=F64)
    bg, fg, tc, nt = (float(v) for v in counts)
    rb, rf, rt, rn = raw_class_weights(counts, cfg["target_weight"])
    if cfg["use_dynamic_weights"]:
        st[0] = 0.9 * st[0] + 0.1 * _clamp(rb, 0.5, 3.0)
        st[1] = 0.9 * st[1] + 0.1 * _clamp(rf, 0.5, 3.0)
        wb, wf = st[0], st[1]
    else:
        wb, wf = 1.0, cfg["target_weight"]
    active = fg > 0 and tc + nt > 0
    wt = wn = 1.0
    if active:
        if cfg["use_dynamic_weights"]:
            tw, ntw = _clamp(rt, 0.5, 3.0), _clamp(rn, 0.5, 3.0)
            if st[4] == 0.0:
                st[2], st[3], st[4] = tw, ntw, 1.0
            else:
                st[2], st[3] = 0.9 * st[2] + 0.1 * tw, 0.9 * st[3] + 0.1 * ntw
            st[5], st[6] = st[2], st[3]
            wt, wn = st[2], st[3]
        else:
            st[5] = st[6] = 1.0
    st[7] += 1.0
    return float(wb), float(wf), float(wt), float(wn), active, st


# ------------------------------------------------------------------------------------------------ the loss
def _exp(x, dt):
    if dt is F32:
        return np.exp2(x * F32(LOG2E))
    return np.exp(x)


def _softmax(v, dt, axis=1):
    e = _exp(v - v.max(axis=axis, keepdims=True), dt)
    return e / e.sum(axis=axis, keepdims=True)


def _lse(v, dt, axis=1):
    m = v.max(axis=axis)
    return m + np.log(_exp(v - np.expand_dims(m, axis), dt).sum(axis=axis))


def _sum(x, dt, axis=None):
    return x.sum(axis=axis, dtype=dt)


def _pick(v, idx):
    """v[N][C][H][W] at channel idx[N][H][W]."""
    return np.take_along_axis(v, idx[:, None], axis=1)[:, 0]


def loss_terms(cfg, pred, bgfg, tn, cont, dist, tg, wts, active, dt=F64, ks=None):
    """The per-pixel terms and what the magnitudes of the bounds need.  Returns a dict of arrays [N][H][W]:
    term_* are the summands of each loss, mag_* the sum of the absolute operands of a term's last addition (for a
    cross entropy: |logsumexp| + |logit|)."""
    wb, wf, wt, wn = (dt(w) for w in wts)
    ks = cfg["contour_ks"] if ks is None else ks
    pred, bgfg, tn = pred.astype(dt), bgfg.astype(dt), tn.astype(dt)
    fg = (tg > 0)
    fgi, yt = fg.astype(np.int64), (tg == 2).astype(np.int64)
    T = {}
    lse_b, g_y = _lse(bgfg, dt), _pick(bgfg, fgi)
    w_y = np.where(fg, wf, wb).astype(dt)
    T["w_y"] = w_y
    T["term_bf"] = w_y * (lse_b - g_y)
    T["mag_bf"] = w_y * (np.abs(lse_b) + np.abs(g_y))
    lse_t, t_y = _lse(tn, dt), _pick(tn, yt)
    w_t = np.where(yt == 1, wn, wt).astype(dt)
    on = fg if active else np.zeros_like(fg)
    T["term_tn"] = np.where(on, w_t * (lse_t - t_y), dt(0))
    T["mag_tn"] = np.where(on, w_t * (np.abs(lse_t) + np.abs(t_y)), dt(0))
    T["w_t"] = w_t
    lse_f, v_y = _lse(pred, dt), _pick(pred, tg)
    T["term_fin"] = lse_f - v_y
    T["mag_fin"] = np.abs(lse_f) + np.abs(v_y)
    pf, pb = _softmax(pred, dt), _softmax(bgfg, dt)
    T["pf"], T["pb"] = pf, pb
    dcon = pb[:, 1] - (pf[:, 1] + pf[:, 2])
    T["dcon"] = dcon
    T["term_cons"] = dcon * dcon
    t1 = (tg == 1).astype(dt)
    T["t1"] = t1
    if cfg["use_boundary_aware"]:
        T["bw"] = boundary_weight(tg, dt)
        T["term_ba"] = T["term_fin"] * T["bw"]
        T["mag_ba"] = T["mag_fin"] * T["bw"]
    if cfg["use_contour"] and cont is not None:
        x = cont.astype(dt)[:, 0]
        ct = contour_target(tg, ks, dt)
        T["ct"], T["x"] = ct, x
        a, b, c = np.maximum(x, dt(0)), x * ct, np.log1p(_exp(-np.abs(x), dt))
        T["term_ct"] = a - b + c
        T["mag_ct"] = np.abs(a) + np.abs(b) + np.abs(c)
    if cfg["use_distance"] and dist is not None:
        dtg = distance_target(tg, dt)
        T["dtg"] = dtg
        T["r"] = dist.astype(dt)[:, 0] - dtg
        T["term_d"] = np.abs(T["r"])
    g0, g1 = bgfg[:, 0], bgfg[:, 1]
    pr = g1 > g0                        # argmax: a tie goes to index 0
    T["n_acc"], T["n_inter"], T["n_union"] = int((pr == fg).sum()), int((pr & fg).sum()), int((pr | fg).sum())
    return T


def loss_eval(cfg, pred, bgfg, tn, cont, dist, tg, state, counts=None, grad_out=1.0, dt=F64):
    """One call of the loss and its backward.  pred [N][3][H][W], bgfg / tn [N][2][H][W], cont / dist [N][1][H][W] or
    None, tg int64 [N][H][W]; `counts` (optional) are external class counts the weights follow, the
    target/non-target normalisation stays with this batch's own foreground count.

    Returns (out[16] in OUT_NAMES order, grads dict pred/bgfg/tn/cont/dist, new state, extras)."""
    N, _, H, W = pred.shape
    P = dt(N * H * W)
    local = class_counts(tg)
    wb, wf, wt, wn, active, st = class_weights(cfg, local if counts is None else counts, state)
    wb, wf, wt, wn = (float(F32(w)) for w in (wb, wf, wt, wn))     # the terms take the weights as an f32 tensor
    fgl = dt(max(local[1], 1.0))
    T = loss_terms(cfg, pred, bgfg, tn, cont, dist, tg, (wb, wf, wt, wn), active, dt)
    c = {k: dt(cfg[k]) for k in CFG_FLOATS}
    go = dt(grad_out)
    sw = _sum(T["w_y"], dt)
    bf = _sum(T["term_bf"], dt) / sw
    tnl = _sum(T["term_tn"], dt) / fgl if active else dt(0)
    fin = _sum(T["term_fin"], dt) / P
    cons = _sum(T["term_cons"], dt) / P
    pf1, t1 = T["pf"][:, 1], T["t1"]
    sm = dt(1e-6)
    I, Ps, Ts = _sum(pf1 * t1, dt, (1, 2)), _sum(pf1, dt, (1, 2)), _sum(t1, dt, (1, 2))
    D = Ps + Ts + sm
    q = (dt(2) * I + sm) / D
    dice = _sum(dt(1) - q, dt) / dt(N)
    base = c["bg_weight"] * bf + c["fg_weight"] * tnl + c["ce_weight"] * fin + c["dice_weight"] * dice + \
        c["consistency_weight"] * cons
    total = base
    ba = ctl = dl = dt(0)
    mba = mct = md = dt(0)
    raw = {}
    if cfg["use_boundary_aware"]:
        raw["ba"] = _sum(T["term_ba"], dt) / P
        mba, ba = dt(raw["ba"] <= CLAMP), min(raw["ba"], dt(CLAMP))
        total = total + c["boundary_aware_weight"] * ba
    if cfg["use_contour"]:
        raw["contour"] = _sum(T["term_ct"], dt) / P
        mct, ctl = dt(raw["contour"] <= CLAMP), min(raw["contour"], dt(CLAMP))
        total = total + c["contour_weight"] * ctl
    if cfg["use_distance"]:
        raw["dist"] = _sum(T["term_d"], dt) / P
        md, dl = dt(raw["dist"] <= CLAMP), min(raw["dist"], dt(CLAMP))
        total = total + c["distance_weight"] * dl
    out = np.zeros(NOUT, dtype=dt)
    out[:9] = [total, bf, tnl, fin, cons, dice, ba, ctl, dl]
    out[9] = dt(T["n_acc"]) / P
    out[10] = dt(T["n_inter"]) / dt(max(T["n_union"], 1))
    out[11:15] = [wb if cfg["use_dynamic_weights"] else 1.0, wf if cfg["use_dynamic_weights"] else cfg["target_weight"],
                  st[5], st[6]]
    out[15] = base

    # ---- gradients of grad_out * total
    one, zero = dt(1), dt(0)
    fg = tg > 0
    pb, pf, dcon = T["pb"], T["pf"], T["dcon"]
    kcons = dt(2) * c["consistency_weight"] / P * dcon           # d total / d pb1 ; d total / d (pf1 + pf2) = -kcons
    oh_b = np.stack([~fg, fg], 1).astype(dt)
    dbgfg = (c["bg_weight"] / sw) * T["w_y"][:, None] * (pb - oh_b)
    j = kcons * pb[:, 1] * pb[:, 0]
    dbgfg[:, 0] -= j
    dbgfg[:, 1] += j
    dtn = np.zeros_like(pb)
    if active:
        pt = _softmax(tn.astype(dt), dt)
        oh_t = np.stack([tg != 2, tg == 2], 1).astype(dt)
        dtn = np.where(fg[:, None], (c["fg_weight"] / fgl) * T["w_t"][:, None] * (pt - oh_t), zero)
    kf = c["ce_weight"] / P
    if cfg["use_boundary_aware"]:
        kf = kf + (c["boundary_aware_weight"] * mba / P) * T["bw"]
    oh_f = np.stack([tg == 0, tg == 1, tg == 2], 1).astype(dt)
    dpred = (kf * np.ones_like(dcon))[:, None] * (pf - oh_f)
    e0 = np.zeros_like(pf)
    e0[:, 0] = one
    dpred += (kcons * pf[:, 0])[:, None] * (e0 - pf)             # -kcons * d(1 - pf0)/dv
    dq_dpf1 = -(dt(2) * t1) / D[:, None, None] + (q / D)[:, None, None]   # d dice_n / d pf1 at a pixel
    e1 = np.zeros_like(pf)
    e1[:, 1] = one
    dpred += (c["dice_weight"] / dt(N) * dq_dpf1 * pf1)[:, None] * (e1 - pf)
    grads = {"pred": go * dpred, "bgfg": go * dbgfg, "tn": go * dtn,
             "cont": np.zeros((N, 1, H, W), dt), "dist": np.zeros((N, 1, H, W), dt)}
    if cfg["use_contour"] and cont is not None:
        sig = one / (one + _exp(-T["x"], dt))
        grads["cont"] = (go * ((c["contour_weight"] * mct / P) * (sig - T["ct"])))[:, None]
    if cfg["use_distance"] and dist is not None:
        grads["dist"] = (go * ((c["distance_weight"] * md / P) * np.sign(T["r"])))[:, None]
    extras = dict(terms=T, raw=raw, counts=local, active=active, sw=sw, I=I, Ps=Ps, Ts=Ts, D=D, q=q,
                  raw_weights=raw_class_weights(local if counts is None else counts, cfg["target_weight"]))
    return out, grads, st, extras


# ------------------------------------------------------------------------------------------------ optimiser
EPS_NORM = float(F32(1e-6))
OPT_BLOCKS, OPT_THREADS = 1024, 256


def hyper(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01, exact=False):
    """The scalar arguments as the kernels receive them (f32 values held as python floats): lr, beta1, beta2,
    1 - beta1, 1 - beta2, 1 - lr wd (the complements formed in double, then rounded), eps, wd.  exact: unrounded
    doubles, for comparisons with a float64 optimiser."""
    f = (lambda x: float(x)) if exact else (lambda x: float(F32(x)))
    return dict(lr=f(lr), b1=f(b1), b2=f(b2), omb1=f(1.0 - b1), omb2=f(1.0 - b2), decay=f(1.0 - lr * wd), eps=f(eps),
                wd=f(wd))


def grad_norm_partials_ref(g):
    """float64 sum of squares per block of the 1024 x 256 grid-stride launch: element i belongs to block
    (i // 256) % 1024."""
    g = np.asarray(g, dtype=F64)
    blk = (np.arange(g.size) // OPT_THREADS) % OPT_BLOCKS
    return np.bincount(blk, weights=g * g, minlength=OPT_BLOCKS)


def norm_from_partials(partials):
    """f32(sqrt(float64 sum of the partials in index order))."""
    s = 0.0
    for v in np.asarray(partials, dtype=F64).tolist():
        s += v
    with np.errstate(invalid="ignore", over="ignore"):
        return F32(np.sqrt(F64(s)))


def clip_coef(norm, max_norm, dt):
    """min(1, max_norm / (norm + 1e-6)); 1 when clipping is off."""
    if not max_norm > 0:
        return dt(1)
    cc = dt(max_norm) / (dt(norm) + dt(EPS_NORM))
    return cc if cc < 1 else dt(1)


def seg_index(seg_start, n):
    """Segment of every flat index: the last non-empty segment s with seg_start[s] <= i (segments may be empty)."""
    seg_start = np.asarray(seg_start, dtype=np.int64)
    nseg = len(seg_start) - 1
    return np.clip(np.searchsorted(seg_start[1:nseg], np.arange(n), side="right"), 0, nseg - 1)


def bias_corrections(h, steps, dt):
    """Per-segment lr / (1 - b1^t) and sqrt(1 - b2^t) for t = steps + 1, formed in double then cast."""
    t = np.asarray(steps, dtype=F64) + 1.0
    bc1, bc2 = 1.0 - np.power(h["b1"], t), 1.0 - np.power(h["b2"], t)
    return (h["lr"] / bc1).astype(dt), np.sqrt(bc2).astype(dt)


def adamw_segmented(p, g, m, v, h, norm, max_norm, seg_start, steps, dt=F64):
    """One hiseg_adamw_step_segmented step.  norm: the total gradient norm (an f32 value).  Returns
    (p, g, m, v, steps, skipped) -- unchanged inputs and skipped = 1 when the norm is not finite.  dt = float32 rounds
    after every operation in the order the comment in adamw_seg_kernel gives: p *= decay; m = lerp(m, g, 1 - b1) (both
    branches of torch's lerp); v = v b2 + ((1 - b2) g) g; p += -(lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps))."""
    steps = np.asarray(steps, dtype=np.int64)
    if not np.isfinite(norm):
        return p.astype(dt), g.astype(dt), m.astype(dt), v.astype(dt), steps.copy(), 1
    p, g, m, v = p.astype(dt), g.astype(dt), m.astype(dt), v.astype(dt)
    if max_norm > 0:
        g = g * clip_coef(norm, max_norm, dt)
    sg = seg_index(seg_start, p.size)
    step, sbc2 = bias_corrections(h, steps, dt)
    step, sbc2 = step[sg], sbc2[sg]
    omb1, omb2, b2, decay, eps = (dt(h[k]) for k in ("omb1", "omb2", "b2", "decay", "eps"))
    p = p * decay
    if h["omb1"] < 0.5:
        m = m + omb1 * (g - m)
    else:
        m = g - (g - m) * (dt(1) - omb1)
    v = v * b2 + (omb2 * g) * g
    den = np.sqrt(v) / sbc2 + eps
    p = p + (-step) * (m / den)
    return p, g, m, v, steps + 1, 0


def adamw_plain(p, g, m, v, h, bc1, bc2, norm, max_norm, dt=F64):
    """hiseg_adamw_step: p *= 1 - lr wd; m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g g;
    p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps).  norm None: no partials given, so no clipping."""
    p, g, m, v = p.astype(dt), g.astype(dt), m.astype(dt), v.astype(dt)
    lr, b1, b2, eps, wd = (dt(h[k]) for k in ("lr", "b1", "b2", "eps", "wd"))
    one = dt(1)
    if norm is not None and max_norm > 0:
        g = g * clip_coef(norm, max_norm, dt)
    p = p * (one - lr * wd)
    m = b1 * m + (one - b1) * g
    v = b2 * v + (one - b2) * g * g
    p = p - (lr / dt(bc1)) * m / (np.sqrt(v) / np.sqrt(dt(bc2)) + eps)
    return p, g, m, v


def adamw_guarded(p, g, m, v, h, norm, max_norm, step, dt=F64):
    """hiseg_adamw_step_guarded: hiseg_adamw_step with the bias corrections of t = step + 1 formed in double, skipped
    as a whole when the norm is not finite.  Returns (p, g, m, v, step, skipped)."""
    if not np.isfinite(norm):
        return p.astype(dt), g.astype(dt), m.astype(dt), v.astype(dt), step, 1
    t = step + 1
    bc1, bc2 = 1.0 - math.pow(h["b1"], t), 1.0 - math.pow(h["b2"], t)
    p, g, m, v = p.astype(dt), g.astype(dt), m.astype(dt), v.astype(dt)
    lr, b1, b2, eps, wd = (dt(h[k]) for k in ("lr", "b1", "b2", "eps", "wd"))
    one = dt(1)
    if max_norm > 0:
        g = g * clip_coef(norm, max_norm, dt)
    p = p * (one - lr * wd)
    m = b1 * m + (one - b1) * g
    v = b2 * v + (one - b2) * g * g
    p = p - dt(h["lr"] / bc1) * m / (np.sqrt(v) / dt(math.sqrt(bc2)) + eps)
    return p, g, m, v, t, 0
