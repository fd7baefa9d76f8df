"""Golden vectors of the reference's mask post-processing (src/human_edge_detection/edge_smoothing.py and
bilateral_filter.py).

Run in the build container only (the reference is at /root/reference and never leaves it):
    python tests/golden/gen_post_golden.py
Runs the reference's own classes on the CPU in f32 and writes
  tests/golden/post.npz              inputs and outputs (0/1 planes as uint8), the modules' buffer values
  tests/golden/state_keys_post.json  constructor arguments, state_dict keys and shapes per module configuration
The run is deterministic (seeded torch.Generator, one thread): a second run reproduces post.npz bit for bit.

Conditions on the fixtures, asserted here (change SEED if one fails, never the margin):
  * every thresholded output on a soft input, and the binary-bilateral and morphological outputs on binary
    inputs: the pre-threshold field, evaluated in float64 by the formulas below, has no pixel within MARGIN of
    the threshold -- an f32 implementation with another summation order decides every pixel the same way;
  * edge smoothing on binary inputs asks for no margin: at least MIN_HALF pixels of odd + roi + big have a float64
    blend within 1e-6 of 0.5 (a one-pixel line's centre: sigmoid(18) rounds to 1.0f, the f32 blend is exactly 0.5,
    not > 0.5) so that the f32 rounding rule is what the fixtures test.
"""
import io
import json
import os
import sys
import zipfile

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
from src.human_edge_detection.bilateral_filter import (  # noqa: E402
    BilateralFilter, BinaryMaskBilateralFilter, FastBilateralFilter, MorphologicalBilateralFilter)
from src.human_edge_detection.edge_smoothing import BinaryMaskEdgeSmoothing, MultiClassEdgeSmoothing  # noqa: E402

SEED = 14
MARGIN = 1e-5
MIN_HALF = 40

SHAPES = {"tiny": (2, 1, 2, 3), "odd": (3, 1, 37, 53), "roi": (2, 1, 48, 64), "big": (1, 1, 200, 264)}

# constructor arguments per configuration; "iterations" of the edge sets is how often the module is applied
# (MultiClassEdgeSmoothing's loop, edge_smoothing.py:147)
EDGE = {"def": dict(kw={}, iterations=1), "alt": dict(kw=dict(threshold=0.4, blur_strength=1.5), iterations=3)}
BINBIL = {"def": {}, "alt": dict(kernel_size=5, sigma_spatial=1.0, num_iterations=1)}
MORPH = {"def": {}, "alt": dict(kernel_size=3, morph_size=5)}
FAST = {"def": {}, "alt": dict(sigma_range=0.05, num_iterations=3)}
BIL = {"k5": {}, "k3": dict(kernel_size=3)}
MC_ITERATIONS = 2


def ellipse_field(g, shape):
    n, c, h, w = shape
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, h), torch.linspace(-1, 1, w), indexing="ij")
    r = torch.rand(n, c, 2, generator=g) * 0.3 + 0.4
    return 1 - ((yy / r[..., 0, None, None]) ** 2 + (xx / r[..., 1, None, None]) ** 2)


def binary_input(g, shape):
    """Ellipse masks, 8 % of the pixels flipped, one full-width one-pixel line through the middle row."""
    m = ellipse_field(g, shape) > 0
    m = m ^ (torch.rand(shape, generator=g) < 0.08)
    m[:, :, shape[2] // 2, :] = True
    return m.float()


def soft_input(g, shape):
    """Sigmoid of the ellipse field plus Gaussian noise (values leave [0, 1]: the clamps are exercised)."""
    return (torch.sigmoid(4 * ellipse_field(g, shape)) + 0.1 * torch.randn(shape, generator=g)).float()


# ---- float64 pre-threshold fields (formulas of the reference's forwards, for the margin checks only)

def edge_field64(x, blur_strength):
    x = x.double()
    lap = F.conv2d(x, torch.tensor([[-1., -1, -1], [-1, 8, -1], [-1, -1, -1]], dtype=torch.float64)[None, None],
                   padding=1)
    blur = F.conv2d(x, torch.tensor([[1., 2, 1], [2, 4, 2], [1, 2, 1]], dtype=torch.float64)[None, None] / 16,
                    padding=1)
    e = torch.sigmoid(lap.abs() * blur_strength)
    return x * (1 - e) + blur * e


def binbil_field64(mod, x):
    x = x.double().clamp(0, 1)
    k = mod.gaussian_kernel.double()
    for _ in range(mod.num_iterations):
        f = F.conv2d(x, k, padding=mod.padding)
        v = (F.conv2d(x * x, k, padding=mod.padding) - f * f).clamp(min=0)
        w = torch.exp(-v * 10)
        x = w * f + (1 - w) * x
    return x


def morph_field64(mod, x):
    def pool(t):
        return F.max_pool2d(t, mod.morph_size, stride=1, padding=mod.morph_padding)
    x = x.double().clamp(0, 1)
    x = pool(-pool(-x))
    x = F.conv2d(x, mod.bilateral_kernel.double(), padding=mod.padding)
    return -pool(-pool(x))


def check_margin(field, threshold, what):
    d = (field - threshold).abs().min().item()
    assert d > MARGIN, f"{what}: a pixel lies {d:.3e} from the threshold {threshold} (margin {MARGIN}); change SEED"
    return d


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps and order: the same arrays give the same file bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(),
                       compress_type=zipfile.ZIP_DEFLATED)


def main():
    torch.manual_seed(SEED)
    torch.set_num_threads(1)
    g = torch.Generator().manual_seed(SEED)
    arrays, keys = {}, {}
    inputs = {}
    for name, shape in SHAPES.items():
        inputs[f"bin_{name}"] = binary_input(g, shape)
        inputs[f"soft_{name}"] = soft_input(g, shape)
    closest = {}
    half = 0

    def record(cfg, mod):
        keys[cfg] = {"class": type(mod).__name__,
                     "keys": {k: list(v.shape) for k, v in mod.state_dict().items()}}
        for k, v in mod.state_dict().items():
            arrays[f"buf/{cfg}/{k}"] = v.numpy()

    with torch.no_grad():
        # edge smoothing
        for tag, spec in EDGE.items():
            mod = BinaryMaskEdgeSmoothing(**spec["kw"]).eval()
            keys_cfg = f"BinaryMaskEdgeSmoothing/{tag}"
            record(keys_cfg, mod)
            keys[keys_cfg]["kwargs"] = spec["kw"]
            keys[keys_cfg]["iterations"] = spec["iterations"]
            for iname, x in inputs.items():
                y = x
                for it in range(spec["iterations"]):
                    field = edge_field64(y, mod.blur_strength)
                    if iname.startswith("soft") and it == 0:
                        d = check_margin(field, mod.threshold, f"edge/{tag}/{iname}")
                        closest[f"edge/{tag}/{iname}"] = d
                    elif tag == "def" and iname in ("bin_odd", "bin_roi", "bin_big"):
                        half += int(((field - 0.5).abs() < 1e-6).sum())
                    y = mod(y)
                assert set(np.unique(y.numpy())) <= {0.0, 1.0}
                arrays[f"edge/{tag}/{iname}"] = y.numpy().astype(np.uint8)
        assert half >= MIN_HALF, f"only {half} binary pixels blend to 0.5; change SEED"

        # binary-mask bilateral and morphological filters: thresholded, margin on every input
        for cls, sets, field_fn, thr in ((BinaryMaskBilateralFilter, BINBIL, binbil_field64, None),
                                         (MorphologicalBilateralFilter, MORPH, morph_field64, 0.5)):
            short = "binbil" if cls is BinaryMaskBilateralFilter else "morph"
            for tag, kw in sets.items():
                mod = cls(**kw).eval()
                record(f"{cls.__name__}/{tag}", mod)
                keys[f"{cls.__name__}/{tag}"]["kwargs"] = kw
                for iname, x in inputs.items():
                    t = mod.threshold if thr is None else thr
                    closest[f"{short}/{tag}/{iname}"] = check_margin(field_fn(mod, x), t, f"{short}/{tag}/{iname}")
                    y = mod(x)
                    assert set(np.unique(y.numpy())) <= {0.0, 1.0}
                    arrays[f"{short}/{tag}/{iname}"] = y.numpy().astype(np.uint8)

        # fast bilateral: soft output, no threshold.  `big` only with the defaults on the soft input (file size)
        for tag, kw in FAST.items():
            mod = FastBilateralFilter(**kw).eval()
            record(f"FastBilateralFilter/{tag}", mod)
            keys[f"FastBilateralFilter/{tag}"]["kwargs"] = kw
            for iname, x in inputs.items():
                if iname.endswith("big") and not (tag == "def" and iname == "soft_big"):
                    continue
                arrays[f"fast/{tag}/{iname}"] = mod(x).numpy()

        # the true bilateral filter (a Python loop over pixels in the reference: a small plane)
        bil_x = soft_input(g, (2, 2, 9, 11))
        inputs["bil_x"] = bil_x
        for tag, kw in BIL.items():
            mod = BilateralFilter(**kw).eval()
            record(f"BilateralFilter/{tag}", mod)
            keys[f"BilateralFilter/{tag}"]["kwargs"] = kw
            arrays[f"bil/{tag}"] = mod(bil_x).numpy()

        # multi-class path: randn scores, iterations = 2; the second input exercises the batch-1 squeeze
        mc = MultiClassEdgeSmoothing(iterations=MC_ITERATIONS, device="cpu")
        for name, b in (("mc_a", 2), ("mc_b", 1)):
            s = torch.randn(b, 3, 37, 53, generator=g)
            inputs[name] = s
            y = mc.smooth_predictions(s)
            assert y.shape == ((b, 3, 37, 53) if b > 1 else (3, 37, 53))
            arrays[f"mc/{name}"] = y.numpy().astype(np.uint8)

    for k, v in inputs.items():
        arrays[f"in/{k}"] = v.numpy().astype(np.uint8) if k.startswith("bin_") else v.numpy()
    save_npz(os.path.join(HERE, "post.npz"), arrays)
    keys["_meta"] = {"seed": SEED, "margin": MARGIN, "mc_iterations": MC_ITERATIONS, "half_pixels": half}
    with open(os.path.join(HERE, "state_keys_post.json"), "w") as f:
        json.dump(keys, f, indent=1, sort_keys=True)
        f.write("\n")
    worst = min(closest, key=closest.get)
    print(f"post.npz: {len(arrays)} arrays, {os.path.getsize(os.path.join(HERE, 'post.npz'))} bytes; "
          f"{half} binary pixels blend to 0.5; closest margin {closest[worst]:.3e} at {worst}")


if __name__ == "__main__":
    main()
