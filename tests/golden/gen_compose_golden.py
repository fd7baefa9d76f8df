"""Golden vectors of the reference's full-frame instance composition (test_hierarchical_instance_peopleseg_onnx.py:
process_mask_output :230-291, visualize_instance_segmentation :336-402, denormalize_bbox :144-161,
generate_instance_colors :106-115).

Run in the build container only (the reference is at /root/reference and never leaves it):
    python tests/golden/gen_compose_golden.py
Runs the reference's own functions on the CPU (one thread, seeded) and writes tests/golden/compose.npz.

The reference script imports cv2, onnxruntime and pycocotools, which are not installed here.  Stand-in modules are put
into sys.modules before the import: empty ones for onnxruntime and pycocotools.coco, and a cv2 with INTER_NEAREST,
resize (OpenCV's resizeNN index map, in float64) and addWeighted (f32 weights, two products and a sum in f32, round
half to even, saturate).  So the RESIZE and BLEND arithmetic is a restatement and is NOT pinned against cv2 itself;
the thresholding, the score, the box arithmetic, the paint order and the colours are the reference's own code.

Per case <c> (tiny, odd_12x10, odd_10x12, c2, many):
  <c>_logits f16 [N,3,mh,mw] (widen to f32: the values the reference saw), <c>_rois f32 [N,5], <c>_frame (B, H, W)
  <c>_mask / <c>_mask_t0 u8 [N,mh,mw], <c>_score / <c>_score_t0 f32 [N]: target mask and mean confidence at
      score_threshold 0.5 / 0 (from the reference's raw_mask, class_probs and score)
  <c>_label / <c>_label_t0 u8 [B,H,W]: 0 background, k + 1 = ROI k owns the pixel.  Derived here from the reference's
      mask_results (its full_mask sequence, :369-385, replayed) and checked against the reference's own picture at
      alpha = 1, where the blend returns the overlay itself.
  <c>_image u8 [B,H,W,3], <c>_colors u8 [N,3] (the colour the reference gave ROI k: it numbers the ROIs one frame
      keeps), <c>_overlay_a50 / <c>_overlay_a30 u8 [B,H,W,3] at score_threshold 0.5
  many_label_rev: the label map of `many` with the ROI tensor (and the logits) reversed.
colors_<n> for n = 1, 2, 9, 70: generate_instance_colors(n).
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "compose.npz")


# ---------------------------------------------------------------------------------------------- stand-ins
def _cv2_resize(src, dsize, interpolation=None):
    assert interpolation == 0
    dw, dh = dsize
    sh, sw = src.shape[:2]
    ifx, ify = 1.0 / (dw / float(sw)), 1.0 / (dh / float(sh))
    xs = np.minimum(np.floor(np.arange(dw, dtype=np.float64) * ifx).astype(np.int64), sw - 1)
    ys = np.minimum(np.floor(np.arange(dh, dtype=np.float64) * ify).astype(np.int64), sh - 1)
    return src[ys][:, xs]


def _cv2_add_weighted(src1, alpha, src2, beta, gamma):
    a, b = np.float32(alpha), np.float32(beta)
    t = src1.astype(np.float32) * a + src2.astype(np.float32) * b + np.float32(gamma)
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)


def import_reference():
    cv2 = types.ModuleType("cv2")
    cv2.INTER_NEAREST = 0
    cv2.resize = _cv2_resize
    cv2.addWeighted = _cv2_add_weighted
    sys.modules["cv2"] = cv2
    ort = types.ModuleType("onnxruntime")
    ort.InferenceSession = object      # named in an annotation of the script; never used here
    sys.modules["onnxruntime"] = ort
    pyc = types.ModuleType("pycocotools")
    coco = types.ModuleType("pycocotools.coco")
    coco.COCO = object
    pyc.coco = coco
    sys.modules["pycocotools"], sys.modules["pycocotools.coco"] = pyc, coco
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, "/root/reference")
    import test_hierarchical_instance_peopleseg_onnx as R
    return R


# ---------------------------------------------------------------------------------------------- inputs
def make_logits(rng, N, mh, mw, n_ties, empty=()):
    """f16-representable f32 logits: noise plus a class-1 ellipse, `n_ties` exact ties of each kind (class 0 = class 1
    on top: the first maximum is 0; class 1 = class 2 on top: it is 1); ROIs in `empty` have class 0 on top."""
    yy, xx = np.mgrid[0:mh, 0:mw]
    l = rng.normal(0.0, 1.5, (N, 3, mh, mw))
    for k in range(N):
        cy, cx = rng.uniform(0.3, 0.7) * mh, rng.uniform(0.3, 0.7) * mw
        inside = ((yy - cy) / (0.45 * mh)) ** 2 + ((xx - cx) / (0.45 * mw)) ** 2 < 1.0
        l[k, 1] += np.where(inside, 2.5, -1.0)
        if k in empty:
            l[k, 0] = np.abs(l[k]).max(0) + 1.0
    l = l.astype(np.float16).astype(np.float32)
    for _ in range(4):       # near zero f16 is finer than 1e-3: lift a maximum that leads by less (2^-4, then re-round)
        s = np.sort(l, axis=1)
        close = (s[:, 2] - s[:, 1] > 0) & (s[:, 2] - s[:, 1] < 1e-3)
        e = np.exp(l.astype(np.float64) - s[:, 2:3])
        near = np.abs(1.0 / e.sum(1) - 0.5) < 1e-4          # a softmax maximum at the 0.5 threshold: lift it too
        if not (close.any() or near.any()):
            break
        top = (l == s[:, 2:3]) & (close | near)[:, None]
        l = np.where(top, l + np.float32(2.0 ** -4), l).astype(np.float16).astype(np.float32)
    live = [k for k in range(N) if k not in empty]
    for t in range(2 * n_ties):
        k, i, j = live[int(rng.integers(len(live)))], int(rng.integers(mh)), int(rng.integers(mw))
        top = np.float32(np.float16(rng.uniform(1.0, 3.0)))
        low = np.float32(np.float16(top - rng.uniform(1.0, 2.0)))
        l[k, :, i, j] = (top, top, low) if t % 2 == 0 else (low, top, top)
    return l


def tricky_coord(p, size):
    """A normalised coordinate whose f32 product with `size` truncates to p but whose exact product is below p."""
    x = np.float32(p / size)
    for _ in range(4):
        if float(x) * size < p and int(x * size) == p and int(float(x) * size) == p - 1:
            return x
        x = np.nextafter(x, np.float32(0))
    return None


def boxes_px(rois_px, B, H, W, tricky=()):
    """rois f32 [N,5] from (batch, x1, y1, x2, y2) in pixels; coordinates listed in `tricky` as (row, col) are replaced
    by a value that truncates differently in f32 and float64 where one exists."""
    r = np.zeros((len(rois_px), 5), np.float32)
    for k, (b, x1, y1, x2, y2) in enumerate(rois_px):
        r[k] = (b, (x1 + 0.5) / W, (y1 + 0.5) / H, (x2 + 0.5) / W, (y2 + 0.5) / H)
        for c, (v, s) in enumerate(((x1, W), (y1, H), (x2, W), (y2, H))):
            if v == s:
                r[k, 1 + c] = 1.0
            if (k, c) in tricky:
                t = tricky_coord(v, s)
                if t is not None:
                    r[k, 1 + c] = t
    return r


# ---------------------------------------------------------------------------------------------- the reference
def roi_outputs(R, logits, thr):
    """Per-ROI target mask, score: process_mask_output with a full-frame box for every ROI."""
    N = logits.shape[0]
    dummy = np.tile(np.array([0, 0, 0, 1, 1], np.float32), (N, 1))
    res = R.process_mask_output(logits, dummy, 8, 8, thr)
    assert len(res) == N
    mask = np.stack([(r["raw_mask"] == 1) & (r["class_probs"].max(0) > thr) for r in res])
    score = np.array([r["score"] for r in res], np.float32)
    return mask, score


def compose(R, logits, rois, frame, thr, image=None, alphas=()):
    """Label map (and the reference's pictures) of every frame."""
    B, H, W = frame
    N = len(rois)
    label = np.zeros((B, H, W), np.int64)
    colors = np.zeros((N, 3), np.uint8)
    pics = {a: np.zeros((B, H, W, 3), np.uint8) for a in alphas}
    for b in range(B):
        idx = np.nonzero(rois[:, 0] == b)[0]
        res = R.process_mask_output(logits[idx], rois[idx], W, H, thr)
        kept = []
        for k in idx:                      # the ROIs process_mask_output keeps (:272), by its own box arithmetic
            x1, y1, x2, y2 = R.denormalize_bbox(rois[k, 1:5], W, H)
            if x2 - x1 > 0 and y2 - y1 > 0:
                kept.append(k)
        assert len(kept) == len(res)
        cols = R.generate_instance_colors(len(res)) if res else np.zeros((0, 3))
        for pos, (k, r) in enumerate(zip(kept, res)):
            assert r["bbox"] == R.denormalize_bbox(rois[k, 1:5], W, H)
            colors[k] = cols[pos]
            if r["score"] > 0:             # :367-374
                full_mask = np.zeros((H, W), np.uint8)
                x1, y1, x2, y2 = r["bbox"]
                if x2 > x1 and y2 > y1:
                    full_mask[y1:y2, x1:x2] = r["mask"]
                label[b][full_mask > 0] = k + 1
        # the reference's own picture at alpha = 1 is its overlay: it must be the colour of the owner
        img = image[b] if image is not None else np.zeros((H, W, 3), np.uint8)
        own = R.visualize_instance_segmentation(img, res, alpha=1.0)
        want = np.where(label[b][..., None] > 0, colors[np.maximum(label[b] - 1, 0)], 0)
        assert np.array_equal(own, want), "label map disagrees with the reference's overlay"
        for a in alphas:
            pics[a][b] = R.visualize_instance_segmentation(image[b], res, alpha=a)
    return label, colors, pics


def fix_image(image, label, colors, alpha, margin):
    """Move image bytes (+1, wrapping) until no float64 pre-rounding value of the blend is within `margin` of a tie."""
    wi, wo = float(np.float32(1 - alpha)), float(np.float32(alpha))
    over = np.where(label[..., None] > 0, colors[np.maximum(label - 1, 0)], 0).astype(np.float64)
    for _ in range(16):
        v = image.astype(np.float64) * wi + over * wo
        bad = np.abs(v - np.floor(v) - 0.5) < margin
        if not bad.any():
            return image
        image = np.where(bad, (image.astype(np.int64) + 1) % 256, image).astype(np.uint8)
    raise AssertionError("fix_image did not converge")


# ---------------------------------------------------------------------------------------------- checks
def check_logits(logits, thr=0.5):
    s = np.sort(logits, axis=1)
    gap = s[:, 2] - s[:, 1]
    assert ((gap == 0) | (gap >= 1e-3)).all(), "two largest logits closer than 1e-3 without being equal"
    tie = gap == 0
    t01 = tie & (logits[:, 0] == logits[:, 1]) & (logits[:, 2] < logits[:, 0])
    t12 = tie & (logits[:, 1] == logits[:, 2]) & (logits[:, 0] < logits[:, 1])
    l64 = logits.astype(np.float64)
    e = np.exp(l64 - l64.max(1, keepdims=True))
    pmax = (e / e.sum(1, keepdims=True)).max(1)
    assert (np.abs(pmax - thr) > 1e-5).all(), "a softmax maximum within 1e-5 of the threshold"
    return int(t01.sum()), int(t12.sum())


def box_stats(R, rois, frame, mh, mw):
    """(coordinates that truncate differently in f32 and float64, box columns / rows that map differently under the
    double map and under dx * m // b)."""
    _, H, W = frame
    trunc = maps = 0
    for r in rois:
        px = R.denormalize_bbox(r[1:5], W, H)
        px64 = [int(float(r[1]) * W), int(float(r[2]) * H), int(float(r[3]) * W), int(float(r[4]) * H)]
        trunc += sum(a != b for a, b in zip(px, px64))
        for lo, hi, m in ((px[0], px[2], mw), (px[1], px[3], mh)):
            bsz = hi - lo
            if bsz > 0:
                d = np.arange(bsz)
                dbl = np.minimum(np.floor(d * (1.0 / (bsz / float(m)))).astype(np.int64), m - 1)
                maps += int((dbl != d * m // bsz).sum())
    return trunc, maps


def coverage(mask, rois, frame, R):
    """Per frame, the largest number of set resized masks over one pixel."""
    B, H, W = frame
    cov = np.zeros((B, H, W), np.int64)
    for k, r in enumerate(rois):
        x1, y1, x2, y2 = R.denormalize_bbox(r[1:5], W, H)
        if x2 > x1 and y2 > y1 and mask[k].any():
            cov[int(r[0]), y1:y2, x1:x2] += _cv2_resize(mask[k].astype(np.uint8), (x2 - x1, y2 - y1), 0)
    return cov.reshape(B, -1).max(1)


# ---------------------------------------------------------------------------------------------- cases
def cases(rng):
    out = {}
    out["tiny"] = dict(frame=(1, 5, 7), mask=(2, 3), ties=1,
                       rois=boxes_px([(0, 0, 0, 5, 4), (0, 2, 1, 7, 5)], 1, 5, 7))
    # (frames 0 and 1 hold three painting ROIs each; frame 2 holds the empty one, the zero-width one and one more)
    odd_px = [(1, 3, 2, 37, 30),      # 34 wide, 28 high
              (0, 0, 0, 53, 37),      # the whole frame, x2 == y2 == 1.0
              (1, 10, 5, 40, 30),
              (0, 20, 3, 53, 37),     # ends at x2 == 1.0; 34 high
              (2, 8, 6, 30, 25),      # no target pixel (make_logits empty=)
              (1, 15, 10, 45, 36),
              (2, 5, 8, 5, 30),       # zero width
              (2, 12, 0, 46, 34),     # 34 wide, 34 high
              (0, 12, 8, 38, 33)]
    odd = boxes_px(odd_px, 3, 37, 53, tricky={(0, 0), (2, 1), (4, 2), (5, 3), (7, 1), (8, 0), (2, 2), (5, 0)})
    for name, m in (("odd_12x10", (12, 10)), ("odd_10x12", (10, 12))):
        out[name] = dict(frame=(3, 37, 53), mask=m, ties=6, rois=odd, empty=(4,))
    c2_px = [(0, 20, 10, 54, 108),    # 34 wide, 98 high
             (1, 0, 0, 160, 120),     # enlarged in x, shrunk in y
             (0, 30, 12, 130, 112),
             (1, 50, 20, 84, 118)]    # 34 wide, 98 high
    out["c2"] = dict(frame=(2, 120, 160), mask=(128, 96), ties=10,
                     rois=boxes_px(c2_px, 2, 120, 160, tricky={(0, 0), (2, 1), (3, 2), (2, 3)}))
    many_px = []
    for k in range(70):
        x1, y1 = int(rng.integers(0, 10)), int(rng.integers(0, 10))
        many_px.append((0, x1, y1, x1 + int(rng.integers(3, 17 - x1)), y1 + int(rng.integers(3, 17 - y1))))
    out["many"] = dict(frame=(1, 16, 16), mask=(4, 4), ties=6, rois=boxes_px(many_px, 1, 16, 16))
    return out


def main():
    torch.set_num_threads(1)
    R = import_reference()
    rng = np.random.default_rng(20261019)
    out = {}
    ties01 = ties12 = trunc = maps = exact_half = 0
    for name, c in cases(rng).items():
        frame, (mh, mw), rois = c["frame"], c["mask"], c["rois"]
        B, H, W = frame
        N = len(rois)
        logits = make_logits(rng, N, mh, mw, c["ties"], c.get("empty", ()))
        a, b = check_logits(logits)
        ties01, ties12 = ties01 + a, ties12 + b
        t, m = box_stats(R, rois, frame, mh, mw)
        trunc, maps = trunc + t, maps + m
        out[f"{name}_logits"] = logits.astype(np.float16)
        assert np.array_equal(out[f"{name}_logits"].astype(np.float32), logits)
        out[f"{name}_rois"] = rois
        out[f"{name}_frame"] = np.array(frame, np.int64)
        for tag, thr in (("", 0.5), ("_t0", 0.0)):
            mask, score = roi_outputs(R, logits, thr)
            out[f"{name}_mask{tag}"] = mask.astype(np.uint8)
            out[f"{name}_score{tag}"] = score
            if thr == 0.0:
                assert np.array_equal(mask, logits.argmax(1) == 1)    # the pack front end sees these planes
                label, _, _ = compose(R, logits, rois, frame, thr)
                out[f"{name}_label{tag}"] = label.astype(np.uint8)
            else:
                assert ((score == 0) | ((score > 0.5) & (score <= 1))).all()
                if name.startswith("odd") or name == "many":
                    # nine ROIs, one of them empty and one zero-width, cannot put three set masks over a pixel in
                    # each of three frames: the third frame of `odd` is exempt
                    cov = coverage(mask, rois, frame, R)[:2]
                    assert (cov >= 3).all(), f"{name}: no pixel under three masks"
                if name.startswith("odd"):
                    assert score[4] == 0 and not mask[4].any()
                label, colors, _ = compose(R, logits, rois, frame, thr)
                image = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
                image = fix_image(image, label, colors, 0.3, 1e-3)
                label2, colors2, pics = compose(R, logits, rois, frame, thr, image, (0.5, 0.3))
                assert np.array_equal(label, label2) and np.array_equal(colors, colors2)
                over = np.where(label[..., None] > 0, colors[np.maximum(label - 1, 0)], 0).astype(np.int64)
                exact_half += int(((image.astype(np.int64) + over) % 2 == 1).sum())
                out[f"{name}_label"] = label.astype(np.uint8)
                out[f"{name}_image"], out[f"{name}_colors"] = image, colors
                out[f"{name}_overlay_a50"], out[f"{name}_overlay_a30"] = pics[0.5], pics[0.3]
        if name == "many":
            rev, _, _ = compose(R, logits[::-1].copy(), rois[::-1].copy(), frame, 0.5)
            assert not np.array_equal(rev, np.where(label > 0, N + 1 - label, 0)), "reversal changed no owner"
            out["many_label_rev"] = rev.astype(np.uint8)
    assert ties01 >= 10 and ties12 >= 10 and ties01 + ties12 >= 20, (ties01, ties12)
    assert trunc >= 4, f"{trunc} box coordinates truncate differently in f32 and float64"
    assert maps >= 3, f"{maps} box columns / rows map differently under the double and the integer map"
    assert exact_half >= 100, exact_half
    for n in (1, 2, 9, 70):
        out[f"colors_{n}"] = R.generate_instance_colors(n).astype(np.uint8).reshape(n, 3)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes; ties {ties01}+{ties12}, f32/f64 truncations {trunc}, "
          f"double/integer map differences {maps}, exact .5 blends {exact_half}")


if __name__ == "__main__":
    main()
