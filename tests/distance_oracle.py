"""Brute-force numpy restatement of the distance-aware loss (test infrastructure only: no scipy, no reference import).

Site rule, squared distance, weight map, loss values and the loss gradient as include/hiseg_distance.h states them;
the virtual site of a mask without sites is a branch of the restatement, as it is in the kernel."""
import numpy as np


def sites(mask):
    """Boolean site map of one class mask [H,W]; None when the mask has no site."""
    mask = np.asarray(mask)
    if len(np.unique(mask)) > 2:
        s = np.zeros(mask.shape, bool)
        s[1:, :] |= mask[1:, :] != mask[:-1, :]
        s[:, 1:] |= mask[:, 1:] != mask[:, :-1]
    else:
        s = mask == 1
    return s if s.any() else None


def d2_map(mask, radius=None):
    """Exact squared Euclidean distance [H,W] int64 to the nearest site of one mask.  ``radius``: look only at sites
    with |dy|, |dx| <= radius (pixels that see none get 2^40); None looks at every site."""
    mask = np.asarray(mask)
    H, W = mask.shape
    yy, xx = np.mgrid[0:H, 0:W]
    s = sites(mask)
    if s is None:   # scipy 1.15.3's distance_transform_edt on an input without background: a site at (-1, 0)
        return ((yy + 1) ** 2 + xx ** 2).astype(np.int64)
    far = np.int64(1) << 40
    best = np.full((H, W), far, np.int64)
    if radius is None:
        ys, xs = np.nonzero(s)
        for y0 in range(0, H, 8):   # row blocks keep the [pixels, sites] table small
            py, px = yy[y0:y0 + 8].reshape(-1, 1), xx[y0:y0 + 8].reshape(-1, 1)
            d = (py - ys[None]) ** 2 + (px - xs[None]) ** 2
            best[y0:y0 + 8] = d.min(1).reshape(-1, W)
        return best
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            sh = np.zeros((H, W), bool)   # sh[y, x] = s[y + dy, x + dx]
            ya, yb = max(0, -dy), min(H, H - dy)
            xa, xb = max(0, -dx), min(W, W - dx)
            if ya >= yb or xa >= xb:
                continue
            sh[ya:yb, xa:xb] = s[ya + dy:yb + dy, xa + dx:xb + dx]
            best = np.where(sh, np.minimum(best, dy * dy + dx * dx), best)
    return best


def clipped_d2(mask, width):
    return np.minimum(d2_map(mask, width - 1), width * width).astype(np.int32)


def weight_map(masks, width, boundary_weight, instance_sep_weight=3.0, inst=None, present=None):
    """(weights f32 [N,H,W], d2 int32 [N,H,W]) of a batch of masks."""
    masks = np.asarray(masks)
    d2 = np.stack([clipped_d2(m, width) for m in masks])
    dist = np.sqrt(d2.astype(np.float64))
    scale = 1.0 + (float(boundary_weight) - 1.0) * (1.0 - dist / width)
    w = np.where(d2 < width * width, scale.astype(np.float32), np.float32(1.0)).astype(np.float32)
    if inst is not None:
        inst = np.asarray(inst, np.float32)
        present = np.ones(len(masks), bool) if present is None else np.asarray(present, bool)
        close = (inst < np.float32(50.0)) & present[:, None, None]
        w = np.where(close, w * np.float32(instance_sep_weight), w).astype(np.float32)
    return w, d2


def boundary_distance(mask, max_distance):
    return np.minimum(np.sqrt(d2_map(mask).astype(np.float64)), max_distance)


def loss(pred, target, w, class_weights=None, use_focal=False, gamma=2.0, ce_weight=1.0, dice_weight=1.0):
    """(dict of the five loss-dict values, d total / d pred) in float64."""
    x = np.asarray(pred, np.float64)
    t = np.asarray(target)
    w = np.asarray(w, np.float64)
    N, C, H, W = x.shape
    P = N * H * W
    z = x - x.max(1, keepdims=True)
    logp = z - np.log(np.exp(z).sum(1, keepdims=True))
    p = np.exp(logp)
    onehot = np.stack([t == c for c in range(3)], 1).astype(np.float64)
    ce = -(logp * onehot).sum(1)
    K = 1.0
    alpha_t = np.ones_like(ce)
    if class_weights is not None:
        cw = np.asarray(class_weights, np.float64)
        K = cw[t].mean()
        alpha_t = cw[t]
    if use_focal:
        pt = np.exp(-ce)
        wce = (alpha_t * (1 - pt) ** gamma * ce).mean() * w.mean() * K
        with np.errstate(invalid="ignore", divide="ignore"):
            dce = ce_weight * K * w.mean() / P * alpha_t * (gamma * (1 - pt) ** (gamma - 1) * pt * ce + (1 - pt) ** gamma)
    else:
        wce = (ce * w).mean() * K
        dce = ce_weight * K / P * w
    p1, t1 = p[:, 1], onehot[:, 1]
    inter, den = (p1 * t1).sum((1, 2)), p1.sum((1, 2)) + t1.sum((1, 2)) + 1e-6
    num = 2 * inter + 1e-6
    dice = (1 - num / den).mean()
    dp1 = -(dice_weight / N) * (2 * t1 / den[:, None, None] - (num / den ** 2)[:, None, None])
    grad = dce[:, None] * (p - onehot)
    e1 = np.zeros_like(p)
    e1[:, 1] = 1.0
    grad += (dp1 * p1)[:, None] * (e1 - p)
    b = np.asarray(w, np.float32) > np.float32(1.5)
    am = np.asarray(pred).argmax(1)   # ties go to the lowest index
    vals = {"total_loss": ce_weight * wce + dice_weight * dice, "ce_loss": wce, "dice_loss": dice,
            "boundary_accuracy": float((am[b] == t[b]).mean()) if b.any() else 0.0, "avg_boundary_weight": w.mean()}
    return vals, grad


def class_weights_from_ratios(pixel_ratios):
    """losses.py:236-263: log-scaled inverse ratios (f32 arithmetic), normalised to sum 3."""
    logs = [np.log(np.float32(1.0 / (pixel_ratios[k] + 1e-3))) for k in ("background", "target", "non_target")]
    s = np.float32(0.0)
    for v in logs:
        s = np.float32(s + v)
    return np.array([np.float32(np.float32(v / s) * np.float32(3.0)) for v in logs], np.float32)
