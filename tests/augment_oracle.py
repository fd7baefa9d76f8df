"""Plain numpy restatement of include/hiseg_augment.h -- TEST INFRASTRUCTURE ONLY.

``augment`` follows the header's five steps on one 8-bit image: integer arithmetic for RGB -> HSV, float32 (each
operation rounded on its own, as numpy does) for HSV -> RGB, float64 for the filter sum.  ``flipped_item`` is the
dataset's handling of a flipped sample (dataset.py:180-212: pad the ROI mask to the full image, flip, crop at the
new box) built from oracle/data.py's helpers.  Like the kernel, this restates albumentations / cv2 and is unpinned
against them.
"""
from __future__ import annotations

import numpy as np

import oracle.data as OD

F = np.float32
SDIV = np.zeros(256, np.int64)
HDIV = np.zeros(256, np.int64)
for _i in range(1, 256):
    SDIV[_i] = int(np.rint((255 << 12) / float(_i)))
    HDIV[_i] = int(np.rint((180 << 12) / (6.0 * _i)))
SECTOR = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])   # (b, g, r) = t[idx]


def rgb2hsv(img: np.ndarray) -> np.ndarray:
    """cv2's 8-bit RGB2HSV (H 0..179) of uint8 [..., 3] -> int64 [..., 3]."""
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    v = np.maximum(r, np.maximum(g, b))
    d = v - np.minimum(r, np.minimum(g, b))
    s = (d * SDIV[v] + 2048) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * d, r - g + 4 * d))
    h = (h * HDIV[d] + 2048) >> 12
    h = np.where(h < 0, h + 180, h)
    return np.stack([h, s, v], -1)


def hsv2rgb(hsv: np.ndarray) -> np.ndarray:
    """cv2's 8-bit HSV2RGB in float32 of int [..., 3] -> uint8 [..., 3]."""
    h, s, v = (hsv[..., c] for c in range(3))
    inv = F(1) / F(255)
    S, V = s.astype(F) * inv, v.astype(F) * inv
    hh = h.astype(F) * (F(6) / F(180))
    while (hh >= F(6)).any():
        hh = np.where(hh >= F(6), hh - F(6), hh)
    k = np.floor(hh)
    f = hh - k
    one = F(1)
    t = np.stack([V, V * (one - S), V * (one - S * f), V * ((one - S) + S * f)], -1).astype(F)
    idx = SECTOR[k.astype(np.int64)]                      # [..., 3] as (b, g, r)
    bgr = np.take_along_axis(t, idx, -1)
    bgr = np.where((s == 0)[..., None], V[..., None], bgr)
    q = np.clip(np.rint(bgr * F(255)), 0, 255).astype(np.uint8)
    return q[..., ::-1]


def colour(img: np.ndarray, sample) -> np.ndarray:
    """Steps 1-3: flip, HSV round trip, channel tables; ``sample`` is one element of AugParams.host."""
    p = img[:, ::-1] if sample["flip"] else img
    if sample["hsv"]:
        hsv = rgb2hsv(p)
        lut = sample["hsv_lut"]
        p = hsv2rgb(np.stack([lut[c][hsv[..., c]] for c in range(3)], -1).astype(np.int64))
    return np.stack([sample["rgb_lut"][c][p[..., c]] for c in range(3)], -1)


def filter_sum(p: np.ndarray, sample) -> np.ndarray:
    """Step 4 before rounding: float64 [H, W, 3] correlation sums with reflect-101 borders."""
    ks = int(sample["ksize"])
    r = ks // 2
    k = sample["kernel"][:ks * ks].astype(np.float64).reshape(ks, ks)
    H, W = p.shape[:2]
    pad = np.pad(p.astype(np.float64), ((r, r), (r, r), (0, 0)), mode="reflect")
    acc = np.zeros(p.shape, np.float64)
    for i in range(ks):
        for j in range(ks):
            acc += k[i, j] * pad[i:i + H, j:j + W]
    return acc


def augment(img: np.ndarray, sample, table: np.ndarray, with_sum: bool = False):
    """All five steps: float32 [3, H, W] (and the filter's float64 sums, None without a filter)."""
    p = colour(img, sample)
    acc = None
    if sample["ksize"]:
        acc = filter_sum(p, sample)
        p = np.clip(np.rint(acc), 0, 255).astype(np.uint8)
    out = table[p].transpose(2, 0, 1)
    return (out, acc) if with_sum else out


def roi_box(bboxes, target, orig_hw, image_size, roi_padding=0.0, min_roi_size=16):
    """dataset.py:121-152, as oracle.data.get_item computes it."""
    orig_h, orig_w = orig_hw
    x, y, w, h = bboxes[target]
    x, y = x * image_size[0] / orig_w, y * image_size[1] / orig_h
    w, h = w * image_size[0] / orig_w, h * image_size[1] / orig_h
    pad_x, pad_y = w * roi_padding, h * roi_padding
    x1, y1 = max(0, int(x - pad_x)), max(0, int(y - pad_y))
    x2, y2 = min(image_size[0], int(x + w + pad_x)), min(image_size[1], int(y + h + pad_y))
    if x2 - x1 < min_roi_size:
        cx = (x1 + x2) // 2
        x1 = max(0, cx - min_roi_size // 2)
        x2 = min(image_size[0], x1 + min_roi_size)
    if y2 - y1 < min_roi_size:
        cy = (y1 + y2) // 2
        y1 = max(0, cy - min_roi_size // 2)
        y2 = min(image_size[1], y1 + min_roi_size)
    return x1, y1, x2, y2


def roi_crop(instance_masks, target, box, image_size):
    """dataset.py:117, 155-170: the 3-class ROI crop at ``box`` of the instance masks resized to the image size."""
    x1, y1, x2, y2 = box
    masks = [OD.cv2_nearest(m, image_size) for m in instance_masks]
    roi = np.zeros((y2 - y1, x2 - x1), np.uint8)
    roi[masks[target][y1:y2, x1:x2] > 0] = 1
    for i, m in enumerate(masks):
        if i != target:
            roi[(m[y1:y2, x1:x2] > 0) & (roi == 0)] = 2
    return roi


def flipped_target(instance_masks, target, box, mask_size, image_size):
    """dataset.py:180-212 + 222-229 for a flipped sample whose UNFLIPPED box is ``box``: (target int64 [mh, mw],
    the flipped box)."""
    x1, y1, x2, y2 = box
    W = image_size[0]
    full = np.zeros((image_size[1], W), np.uint8)
    full[y1:y2, x1:x2] = roi_crop(instance_masks, target, box, image_size)
    full = full[:, ::-1]
    nx1, nx2 = W - x2, W - x1
    roi = full[y1:y2, nx1:nx2]
    return OD.cv2_nearest(roi, (int(mask_size[1]), int(mask_size[0]))).astype(np.int64), (nx1, y1, nx2, y2)


def unflipped_target(instance_masks, target, box, mask_size, image_size):
    roi = roi_crop(instance_masks, target, box, image_size)
    return OD.cv2_nearest(roi, (int(mask_size[1]), int(mask_size[0]))).astype(np.int64)


def ellipses(rng, k, h, w):
    """k overlapping elliptical instance masks uint8 [k, h, w] and their COCO boxes."""
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((k, h, w), np.uint8)
    boxes = []
    for i in range(k):
        cy, cx = rng.uniform(0.2 * h, 0.8 * h), rng.uniform(0.2 * w, 0.8 * w)
        ry, rx = rng.uniform(0.1 * h, 0.4 * h), rng.uniform(0.1 * w, 0.4 * w)
        m[i] = (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1).astype(np.uint8)
        ys, xs = np.nonzero(m[i])
        boxes.append([float(xs.min()), float(ys.min()), float(xs.max() - xs.min() + 1), float(ys.max() - ys.min() + 1)])
    return m, boxes
