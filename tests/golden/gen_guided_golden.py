"""Golden vectors of the reference's guided filter (EdgePreservingFilter, src/human_edge_detection/
bilateral_filter.py:219-296).

Run in the build container only (the reference is at /root/reference and never leaves it):
    python tests/golden/gen_guided_golden.py
Runs the reference's own class on the CPU and writes tests/golden/guided.npz.  For every case:
  gold/<case>   the reference's forward on float64 copies of the module and the inputs, rounded to f32
  err32/<case>  scalar: max |the reference's f32 forward - that float64 forward| (before the rounding)
and once: in/soft_<shape> (f32), in/rgb_<shape> (uint8), buf/box_kernel/<radius>, and `cases`, the list of case
names.  The run is deterministic (seeded torch.Generator, one thread).

Inputs, derived by guided_inputs() below -- tests/test_gpu_guided.py calls it too, with what the file stores:
  soft  [N,1,H,W]  sigmoid of an ellipse field: a smooth blob mask.  Its flat parts have a variance far below eps,
                   where the f32 cancellation in box(x*g) - box(x)*box(g) is divided by little more than eps
  bin   [N,1,H,W]  soft > 0.5
  rgb   [N,3,H,W]  uint8 / 255, uniform noise: an 8-bit image as the guide
  rot   [N,3,H,W]  rgb with its channels rotated by one
Modes (a case is <mode>/<kind>/<setting>/<shape>, kind = soft or bin naming the mask):
  self  x = mask, no guide            m1g3  x = mask, guide = rgb  (1 -> 3 channels)
  x3g1  x = rgb, guide = mask         x3g3  x = rgb, guide = rot   (3 with 3)
Settings (radius, eps): def (2, 0.01), r4 (4, 1e-3), r8 (8, 1e-4).  On tiny the window of r8 is larger than the
plane.

What is recorded.  guided.npz is a committed file and must stay under 1 MiB, and its f32 planes do not compress.
tiny: every mode x kind x setting.  odd and roi: the self-guided mode with the soft mask at all three settings,
and every other mode, the binary mask and every setting at least once across the two (RECORD below).  big (the
tiled form past the resident limit): self-guided, soft, r8 -- the case whose f32 reference is furthest from
float64.  test_gpu_guided.py checks the two forms against each other on tiny, odd and roi at every setting.
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

SEED = 23
SHAPES = {"tiny": (2, 1, 2, 3), "odd": (3, 1, 37, 53), "roi": (2, 1, 48, 64), "big": (1, 1, 200, 264)}
SETTINGS = {"def": (2, 0.01), "r4": (4, 1e-3), "r8": (8, 1e-4)}
MODES = ("self", "m1g3", "x3g1", "x3g3")
KINDS = ("soft", "bin")

RECORD = {
    "tiny": [(m, k, s) for m in MODES for k in KINDS for s in SETTINGS],
    "odd": [("self", "soft", "def"), ("self", "soft", "r4"), ("self", "soft", "r8"), ("self", "bin", "r4"),
            ("m1g3", "bin", "def"), ("m1g3", "soft", "r4"), ("x3g1", "soft", "r8"), ("x3g3", "soft", "def")],
    "roi": [("self", "soft", "def"), ("self", "soft", "r4"), ("self", "soft", "r8"), ("self", "bin", "def"),
            ("m1g3", "soft", "r8"), ("x3g1", "bin", "def"), ("x3g3", "soft", "r4")],
    "big": [("self", "soft", "r8")],
}


def guided_inputs(soft, rgb_u8, mode, kind):
    """(x, guide or None) of a case from the stored arrays (numpy in, f32 numpy out)."""
    soft = np.asarray(soft, np.float32)
    mask = soft if kind == "soft" else (soft > 0.5).astype(np.float32)
    if mode == "self":
        return mask, None
    rgb = rgb_u8.astype(np.float32) / np.float32(255)
    if mode == "m1g3":
        return mask, rgb
    if mode == "x3g1":
        return rgb, mask
    if mode == "x3g3":
        return rgb, np.ascontiguousarray(rgb[:, [1, 2, 0]])
    raise ValueError(mode)


def case_name(mode, kind, setting, shape):
    return f"{mode}/{kind}/{setting}/{shape}"


def soft_input(g, shape):
    n, c, h, w = shape
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, h), torch.linspace(-1, 1, w), indexing="ij")
    r = torch.rand(n, c, 2, generator=g) * 0.3 + 0.4
    field = 1 - ((yy / r[..., 0, None, None]) ** 2 + (xx / r[..., 1, None, None]) ** 2)
    return torch.sigmoid(4 * field).float()


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps and order: the same arrays give the same file bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(),
                       compress_type=zipfile.ZIP_DEFLATED)


def main():
    sys.path.insert(0, "/root/reference")
    from src.human_edge_detection.bilateral_filter import EdgePreservingFilter

    torch.manual_seed(SEED)
    torch.set_num_threads(1)
    g = torch.Generator().manual_seed(SEED)
    arrays, names = {}, []
    lo, hi = None, None
    with torch.no_grad():
        for tag, (radius, eps) in SETTINGS.items():
            arrays[f"buf/box_kernel/{radius}"] = EdgePreservingFilter(radius, eps).state_dict()["box_kernel"].numpy()
        for shape_name, shape in SHAPES.items():
            soft = soft_input(g, shape).numpy()
            arrays[f"in/soft_{shape_name}"] = soft
            rgb = None
            if any(m != "self" for m, _, _ in RECORD[shape_name]):
                n, _, h, w = shape
                rgb = torch.randint(0, 256, (n, 3, h, w), generator=g).to(torch.uint8).numpy()
                arrays[f"in/rgb_{shape_name}"] = rgb
            for mode, kind, tag in RECORD[shape_name]:
                radius, eps = SETTINGS[tag]
                x, guide = guided_inputs(soft, rgb, mode, kind)
                x = torch.from_numpy(x)
                guide = None if guide is None else torch.from_numpy(guide)
                mod32 = EdgePreservingFilter(radius, eps).eval()
                mod64 = EdgePreservingFilter(radius, eps).double().eval()
                y32 = mod32(x, guide)
                y64 = mod64(x.double(), None if guide is None else guide.double())
                assert y32.dtype == torch.float32 and y64.dtype == torch.float64 and y32.shape == y64.shape
                err = (y32.double() - y64).abs().max().item()
                name = case_name(mode, kind, tag, shape_name)
                names.append(name)
                arrays[f"gold/{name}"] = y64.float().numpy()
                arrays[f"err32/{name}"] = np.float64(err)
                lo = (err, name) if lo is None or err < lo[0] else lo
                hi = (err, name) if hi is None or err > hi[0] else hi
                print(f"{name}: out {tuple(y64.shape)} max |out| {y64.abs().max().item():.3f} ref32_err {err:.3e}")
    arrays["cases"] = np.array(names)
    path = os.path.join(HERE, "guided.npz")
    save_npz(path, arrays)
    size = os.path.getsize(path)
    assert size < 1 << 20, f"guided.npz is {size} bytes: record fewer cases"
    print(f"guided.npz: {len(names)} cases, {size} bytes; ref32_err from {lo[0]:.3e} ({lo[1]}) to {hi[0]:.3e} ({hi[1]})")


if __name__ == "__main__":
    main()
