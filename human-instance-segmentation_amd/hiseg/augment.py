"""ROI-safe training augmentation on the GPU (include/hiseg_augment.h): the pipeline train_advanced.py:1031-1049
installs with ``config.data.use_augmentation`` (augmentations.py:158-257 get_roi_safe_transforms) -- a horizontal
flip that also moves the ROI box and the ROI mask, colour transforms, blur, ``Normalize`` -- for images that are
already on the device (hiseg.data.GpuRoiBatchBuilder).

The host draws the random parameters (a few numbers per sample) and turns them into what one fused HIP launch
applies to every pixel: 8-bit tables for the colour transforms (two table transforms in a row compose exactly
into one table, ``compose_luts``), cv2's 8-bit RGB -> HSV -> RGB round trip with per-channel tables for
HueSaturationValue, and a k x k correlation kernel (k <= 7) for the blurs.

albumentations 2.0.8 and OpenCV 4.12 (the reference's pins) are restated, unpinned: the arithmetic follows their
published sources -- the f32 table builders with truncating ``astype(uint8)``, cv2's fixed-point RGB2HSV and f32
HSV2RGB, reflect-101 borders -- but neither library is available to compare against, so parity with them is not
tested; include/hiseg_augment.h is the contract the kernel and tests/augment_oracle.py are held to.

Every function fails loudly without the HIP library; nothing falls back to the CPU.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L

SAMPLE_DTYPE = np.dtype(L.AugSample)     # one hiseg_aug_sample
KSIZES = (0, 3, 5, 7)


# ---- host table builders -------------------------------------------------------------------------------------------

def _ramp() -> np.ndarray:
    return np.arange(256, dtype=np.float32)


def brightness_contrast_lut(alpha: float, beta: float) -> np.ndarray:
    """RandomBrightnessContrast on uint8 (brightness_by_max): ``clip(i * alpha + beta * 255)`` in f32, truncated."""
    lut = _ramp() * np.float32(alpha) + np.float32(beta * 255)
    return np.clip(lut, 0, 255).astype(np.uint8)


def rgb_shift_lut(r: float, g: float, b: float) -> np.ndarray:
    """RGBShift: uint8 [3, 256], ``clip(i + shift)`` per channel in f32, truncated."""
    return np.stack([np.clip(_ramp() + np.float32(s), 0, 255).astype(np.uint8) for s in (r, g, b)])


def gamma_lut(gamma: float) -> np.ndarray:
    """RandomGamma on uint8: ``(i / 255) ** gamma * 255`` in float64, truncated."""
    return ((np.arange(256) / 255.0) ** float(gamma) * 255).astype(np.uint8)


def hsv_shift_luts(hue: float, sat: float, val: float) -> np.ndarray:
    """HueSaturationValue on uint8: tables [3, 256] for cv2's 8-bit H (0..179, wraps), S and V (clipped)."""
    i = _ramp()
    h = np.mod(i + np.float32(hue), np.float32(180)).astype(np.uint8)
    s = np.clip(i + np.float32(sat), 0, 255).astype(np.uint8)
    v = np.clip(i + np.float32(val), 0, 255).astype(np.uint8)
    return np.stack([h, s, v])


def gaussian_kernel(ksize: int, sigma: float) -> np.ndarray:
    """f32 [ksize, ksize]: the outer product of exp(-x^2 / 2 sigma^2), normalised to sum 1 in float64."""
    x = np.arange(ksize, dtype=np.float64) - ksize // 2
    g = np.exp(-(x * x) / (2.0 * float(sigma) ** 2))
    k = np.outer(g, g)
    return (k / k.sum()).astype(np.float32)


def compose_luts(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """The table of "a, then b" (per channel where either is [3, 256]): exact for 8-bit tables."""
    a, b = np.asarray(a, np.uint8), np.asarray(b, np.uint8)
    if a.ndim == 1 and b.ndim == 1:
        return b[a]
    a3, b3 = np.broadcast_to(a, (3, 256)), np.broadcast_to(b, (3, 256))
    return np.stack([b3[c][a3[c]] for c in range(3)])


_IDENTITY = np.arange(256, dtype=np.uint8)


# ---- a batch of hiseg_aug_sample --------------------------------------------------------------------------------------

class AugParams:
    """A batch of ``hiseg_aug_sample`` as one packed host buffer (``.host``, a numpy structured array [B]) and,
    after ``.to(device)``, one device buffer (``.buf`` uint8) plus the flip vector (``.flip`` int32 [B]).

    The device storage is static: ``copy_(other)`` overwrites it in place, so a captured graph that holds
    its addresses replays with the new parameters."""

    def __init__(self, B: int):
        if B <= 0:
            raise ValueError("AugParams: empty batch")
        self.host = np.zeros(B, SAMPLE_DTYPE)
        self.host["hsv_lut"][:] = _IDENTITY
        self.host["rgb_lut"][:] = _IDENTITY
        self.ran = np.zeros((B, 3), bool)     # which groups (colour, lighting, blur) a sampler ran, per sample
        self.buf: Optional[torch.Tensor] = None
        self.flip: Optional[torch.Tensor] = None

    def __len__(self) -> int:
        return self.host.shape[0]

    def set(self, i: int, flip: bool = False, hsv_luts: Optional[np.ndarray] = None,
            rgb_lut: Optional[np.ndarray] = None, kernel: Optional[np.ndarray] = None) -> "AugParams":
        """Fill sample ``i``: ``hsv_luts`` uint8 [3, 256] turns the HSV stage on; ``rgb_lut`` uint8 [256] or
        [3, 256]; ``kernel`` f32 [k, k] with k in 3, 5, 7."""
        s = self.host[i]
        s["flip"], s["hsv"], s["ksize"], s["reserved"] = int(bool(flip)), int(hsv_luts is not None), 0, 0
        s["hsv_lut"][:] = _IDENTITY if hsv_luts is None else np.asarray(hsv_luts, np.uint8).reshape(3, 256)
        s["rgb_lut"][:] = _IDENTITY if rgb_lut is None else np.broadcast_to(np.asarray(rgb_lut, np.uint8), (3, 256))
        s["kernel"][:] = 0
        if kernel is not None:
            k = np.asarray(kernel, np.float32)
            if k.ndim != 2 or k.shape[0] != k.shape[1] or k.shape[0] not in KSIZES[1:]:
                raise ValueError(f"AugParams: kernel must be 3x3, 5x5 or 7x7, got {k.shape}")
            s["ksize"] = k.shape[0]
            s["kernel"][:k.size] = k.reshape(-1)
        return self

    def validate(self) -> None:
        """The library's check of the packed samples (ksize in 0/3/5/7, flip and hsv 0/1)."""
        host = np.ascontiguousarray(self.host)
        L.check(L.lib().hiseg_aug_validate(host.ctypes.data, len(self)), "aug_validate")

    def _bytes(self) -> torch.Tensor:
        return torch.from_numpy(np.ascontiguousarray(self.host).view(np.uint8).copy())

    def to(self, device) -> "AugParams":
        self.validate()
        self.buf = self._bytes().to(device)
        self.flip = torch.from_numpy(self.host["flip"].astype(np.int32)).to(device)
        return self

    def copy_(self, other: "AugParams") -> "AugParams":
        """Overwrite these parameters (host and, in place, device) with ``other``'s."""
        if len(other) != len(self):
            raise ValueError(f"AugParams.copy_: batch {len(other)} into {len(self)}")
        other.validate()
        self.host[...] = other.host
        self.ran[...] = other.ran
        if self.buf is not None:
            self.buf.copy_(self._bytes())
            self.flip.copy_(torch.from_numpy(self.host["flip"].astype(np.int32)))
        return self


_OUT_TABLES: Dict[Tuple[str, str], torch.Tensor] = {}


def out_table(mode: str) -> np.ndarray:
    """f32 [256]: "normalize" = ``i * f32(1 / 255)`` (albumentations Normalize(mean 0, std 1), a multiply by the
    f32 reciprocal); "div255" = ``i / 255`` in f32 (dataset.py:238, what resize_bilinear_pil writes)."""
    if mode == "normalize":
        return np.arange(256, dtype=np.float32) * np.float32(1.0 / 255.0)
    if mode == "div255":
        return np.arange(256, dtype=np.float32) / np.float32(255)
    raise ValueError(f"augment_images: mode {mode!r} (normalize or div255)")


def augment_images(images: torch.Tensor, params: AugParams, mode: str = "normalize",
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Flip, HSV round trip, channel tables, filter and float store of uint8 ``[B, H, W, 3]`` in one launch;
    returns float32 ``[B, 3, H, W]`` (``out`` if given).  No synchronisation: capturable in a graph."""
    if not images.is_cuda:
        raise RuntimeError("hiseg data path runs on the GPU only (got a CPU tensor)")
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
        raise ValueError(f"augment_images: expected uint8 [B, H, W, 3], got {images.dtype} {tuple(images.shape)}")
    B, H, W, _ = images.shape
    if len(params) != B:
        raise ValueError(f"augment_images: {len(params)} parameter sets for {B} images")
    if params.buf is None or params.buf.device != images.device:
        raise ValueError("augment_images: params are not on the images' device (AugParams.to)")
    params.validate()
    key = (str(images.device), mode)
    tab = _OUT_TABLES.get(key)
    if tab is None:
        tab = _OUT_TABLES[key] = torch.from_numpy(out_table(mode)).to(images.device)
    src = images.contiguous()
    if out is None:
        out = torch.empty(B, 3, H, W, dtype=torch.float32, device=images.device)
    elif (out.dtype != torch.float32 or tuple(out.shape) != (B, 3, H, W) or not out.is_contiguous()
          or out.device != images.device):
        raise ValueError("augment_images: out must be contiguous float32 [B, 3, H, W] on the images' device")
    L.check(L.lib().hiseg_augment_fwd(src.data_ptr(), params.buf.data_ptr(), tab.data_ptr(), B, H, W, out.data_ptr(),
                                      L.stream_ptr()), "augment_fwd")
    return out


# ---- the reference's policies ------------------------------------------------------------------------------------------

class RoiSafeAugmentation:
    """The random policy of get_roi_safe_transforms, drawn on the host from one ``numpy.random.Generator``.

    ``sample(B)`` draws, for each sample in turn and always in this order (so a seed fixes the batch):
    the flip (one uniform, flip if < 0.5); then for each kept group of the policy one uniform (the group runs if it
    is below the group's probability), one integer choosing the member, and the member's parameters by
    ``uniform`` in the order listed below.  A group that does not run draws nothing further.

    ``light`` (get_roi_safe_light_transforms, complete): colour group p 0.8 -- brightness-contrast
    (alpha = 1 + U(-.2, .2), beta = U(-.2, .2)) or HSV shift (U(-10, 10), U(-20, 20), U(-20, 20)); blur p 0.1 --
    Gaussian, ksize from {3, 5}, sigma = U(0.5, 3).

    ``heavy-subset`` (the table and filter members of get_roi_safe_heavy_transforms; group probabilities as the
    reference's, members uniform over those kept): colour p 0.8 -- HSV shift (20, 30, 20) or RGB shift (+-15 per
    channel); lighting p 0.5 -- brightness-contrast (0.3) or gamma U(80, 120) / 100; blur p 0.05 -- Gaussian,
    ksize from {3, 5, 7}, sigma = U(0.5, 3).  Not restated (they stay on the host): ColorJitter, CLAHE, rain, fog,
    sun flare, median blur, the noises, JPEG compression, downscale, and motion blur's line sampler (the kernel
    takes any 7 x 7, so a caller can pass a motion kernel through AugParams.set)."""

    POLICIES = {
        "light": dict(colour=(0.8, (("bc", 0.2), ("hsv", (10, 20, 20)))), lighting=None, blur=(0.1, (3, 5))),
        "heavy-subset": dict(colour=(0.8, (("hsv", (20, 30, 20)), ("rgb", 15))),
                             lighting=(0.5, (("bc", 0.3), ("gamma", (80, 120)))), blur=(0.05, (3, 5, 7))),
    }

    def __init__(self, policy: str = "light", seed: Optional[int] = None):
        if policy not in self.POLICIES:
            raise ValueError(f"RoiSafeAugmentation: policy {policy!r} (light or heavy-subset)")
        self.policy = policy
        self.rng = np.random.default_rng(seed)

    def _member(self, group):
        """(hsv_luts or None, rgb_lut or None) of one colour / lighting group, or (None, None)."""
        p, members = group
        if not self.rng.random() < p:
            return None, None
        kind, arg = members[int(self.rng.integers(len(members)))]
        u = self.rng.uniform
        if kind == "bc":
            alpha = 1.0 + u(-arg, arg)
            return None, brightness_contrast_lut(alpha, u(-arg, arg))
        if kind == "hsv":
            return hsv_shift_luts(u(-arg[0], arg[0]), u(-arg[1], arg[1]), u(-arg[2], arg[2])), None
        if kind == "rgb":
            return None, rgb_shift_lut(u(-arg, arg), u(-arg, arg), u(-arg, arg))
        return None, gamma_lut(u(arg[0], arg[1]) / 100.0)

    def sample(self, B: int) -> AugParams:
        pol = self.POLICIES[self.policy]
        params = AugParams(B)
        for i in range(B):
            flip = bool(self.rng.random() < 0.5)
            hsv, rgb = self._member(pol["colour"])
            colour, light = hsv is not None or rgb is not None, None
            if pol["lighting"] is not None:
                _, light = self._member(pol["lighting"])
                if light is not None:
                    rgb = light if rgb is None else compose_luts(rgb, light)
            kernel = None
            p_blur, sizes = pol["blur"]
            if self.rng.random() < p_blur:
                ks = sizes[int(self.rng.integers(len(sizes)))]
                kernel = gaussian_kernel(ks, self.rng.uniform(0.5, 3.0))
            params.set(i, flip=flip, hsv_luts=hsv, rgb_lut=rgb, kernel=kernel)
            params.ran[i] = (colour, light is not None, kernel is not None)
        return params


def flip_box(box: Sequence[int], image_w: int) -> Tuple[int, int, int, int]:
    """The ROI box of the mirrored image, in exact integers: (W - x2, y1, W - x1, y2)."""
    x1, y1, x2, y2 = box
    return image_w - x2, y1, image_w - x1, y2
