"""ROI-safe training augmentation on the GPU (hiseg.augment over include/hiseg_augment.h) against the numpy
restatement tests/augment_oracle.py: every byte equal for flip, HSV and tables; the filter equal except at
rounding ties of the oracle's float64 sum; flipped ROI targets equal; the builder and graph capture."""
import numpy as np
import pytest
import torch

import augment_oracle as AO

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _run(imgs, params, mode="normalize"):
    from hiseg.augment import augment_images
    return augment_images(torch.from_numpy(imgs).to(DEV), params.to(DEV), mode=mode).cpu().numpy()


def _oracle(imgs, params, mode="normalize"):
    from hiseg.augment import out_table
    tab = out_table(mode)
    return np.stack([AO.augment(imgs[i], params.host[i], tab) for i in range(len(imgs))])


def _batch(seed, B=4, H=45, W=70):
    return np.random.default_rng(seed).integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)


def test_identity_equals_the_resize_output_and_the_normalize_table():
    from hiseg.augment import AugParams
    from hiseg.data import resize_bilinear_pil
    x = torch.from_numpy(_batch(5, 3, 61, 83)).to(DEV)
    want = resize_bilinear_pil(x, (40, 97)).cpu().numpy()
    u8 = resize_bilinear_pil(x, (40, 97), out_f32=False)
    assert tuple(u8.shape) == (3, 97, 40, 3)
    got = _run(u8.cpu().numpy(), AugParams(3), "div255")
    np.testing.assert_array_equal(got, want)
    norm = _run(u8.cpu().numpy(), AugParams(3), "normalize")
    np.testing.assert_array_equal(norm, (u8.cpu().numpy().astype(np.float32) * np.float32(1.0 / 255.0))
                                  .transpose(0, 3, 1, 2))


def test_hsv_lattice_every_byte():
    """Every (r, g, b) with each channel in {0, 5, ..., 250, 255}: greys, v = 0, all six sectors and their
    boundaries, under three shifts (one sample each)."""
    from hiseg.augment import AugParams, hsv_shift_luts
    v = np.concatenate([np.arange(0, 255, 5), [255]]).astype(np.uint8)
    assert len(v) == 52
    img = np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(338, 416, 3)
    imgs = np.stack([img] * 3)
    p = AugParams(3)
    for i, shift in enumerate(((0, 0, 0), (10, -20, 20), (-20, 30, -20))):
        p.set(i, hsv_luts=hsv_shift_luts(*shift))
    got, want = _run(imgs, p), _oracle(imgs, p)
    for i in range(3):
        np.testing.assert_array_equal(got[i], want[i], err_msg=f"shift {i}")
    assert not np.array_equal(want[0], want[1])


def test_tables_and_flip_every_byte():
    from hiseg.augment import (AugParams, brightness_contrast_lut, compose_luts, gamma_lut, hsv_shift_luts,
                               rgb_shift_lut)
    imgs = _batch(7)
    p = AugParams(4)
    p.set(1, flip=True, rgb_lut=brightness_contrast_lut(1.15, -0.08))
    p.set(2, rgb_lut=compose_luts(rgb_shift_lut(12, -15, 7), gamma_lut(0.9)))
    p.set(3, flip=True, hsv_luts=hsv_shift_luts(-7, 15, -12))
    got, want = _run(imgs, p), _oracle(imgs, p)
    for i in range(4):
        np.testing.assert_array_equal(got[i], want[i], err_msg=f"sample {i}")
    np.testing.assert_array_equal(got[0], imgs[0].transpose(2, 0, 1).astype(np.float32) * np.float32(1.0 / 255.0))


def _check_filter(imgs, p):
    """Equal to the float64 oracle except where its sum lies within 1e-3 of a rounding tie (f32 accumulation of
    49 taps is off by at most 50 * 2^-24 * 255 = 7.6e-4): there one code value, on at most 1 % of the image."""
    from hiseg.augment import out_table
    tab = out_table("normalize")
    got = _run(imgs, p)
    for i in range(len(imgs)):
        want, acc = AO.augment(imgs[i], p.host[i], tab, with_sum=True)
        if acc is None:
            np.testing.assert_array_equal(got[i], want)
            continue
        code = np.rint(got[i].astype(np.float64) * 255).astype(np.int64)
        np.testing.assert_array_equal(tab[code], got[i])             # the output is a table entry
        ref = np.clip(np.rint(acc), 0, 255).astype(np.int64).transpose(2, 0, 1)
        near_tie = (np.abs(acc - (np.floor(acc) + 0.5)) < 1e-3).transpose(2, 0, 1)
        diff = np.abs(code - ref)
        share = float((diff != 0).mean())
        print(f"filter sample {i} ksize {int(p.host[i]['ksize'])}: {int((diff != 0).sum())} pixels differ "
              f"({share:.4%}), near ties {float(near_tie.mean()):.4%}")
        assert diff.max() <= 1
        assert not (diff != 0)[~near_tie].any(), f"sample {i}: differs away from a tie"
        assert share <= 0.01


def test_filter_gaussians_and_an_asymmetric_kernel():
    from hiseg.augment import AugParams, gaussian_kernel, out_table
    imgs = _batch(9)
    diag = np.eye(7, dtype=np.float32) / 7
    p = AugParams(4)
    p.set(0, kernel=gaussian_kernel(3, 0.8))
    p.set(1, flip=True, kernel=gaussian_kernel(5, 1.7))
    p.set(2, kernel=gaussian_kernel(7, 2.6))
    p.set(3, flip=True, kernel=diag)
    _check_filter(imgs, p)
    # the diagonal kernel is not its own mirror: these inputs tell "filter the flipped image" from "flip the kernel"
    tab = out_table("normalize")
    mirrored = AugParams(1).set(0, flip=True, kernel=diag[:, ::-1].copy())
    assert not np.array_equal(AO.augment(imgs[3], p.host[3], tab), AO.augment(imgs[3], mirrored.host[0], tab))


def test_filter_reflect_border_at_its_tightest():
    from hiseg.augment import AugParams, gaussian_kernel
    imgs = _batch(10, 2, 9, 5)
    p = AugParams(2)
    p.set(0, kernel=gaussian_kernel(7, 3.0))
    p.set(1, flip=True, kernel=np.eye(7, dtype=np.float32) / 7)
    _check_filter(imgs, p)
    small = _batch(11, 1, 4, 4)
    _check_filter(small, AugParams(1).set(0, kernel=gaussian_kernel(7, 2.0)))


SIZES = [(180, 240), (180, 240), (97, 131), (300, 200), (97, 131), (180, 240)]
IMAGE_SIZE = (320, 240)
# unflipped ROIs in image pixels: odd and even widths, one touching the left border, one the right
BOXES = [(40, 30, 171, 200), (0, 10, 77, 150), (227, 5, 320, 231), (60, 40, 200, 180), (10, 20, 151, 220),
         (100, 0, 260, 240)]
FLIPS = [1, 1, 1, 1, 0, 0]


@pytest.fixture(scope="module")
def instances():
    rng = np.random.default_rng(17)
    out = []
    for h, w in SIZES:
        k = int(rng.integers(2, 5))
        m, boxes = AO.ellipses(rng, k, h, w)
        out.append((m, boxes, int(rng.integers(0, k))))
    return out


@pytest.mark.parametrize("mask_size", [(56, 56), (128, 96)])
def test_flipped_targets_equal_the_dataset_restatement(instances, mask_size):
    from hiseg.data import roi_targets
    descs_f, descs_u, chunks, off = [], [], [], 0
    for (m, _, t), box, f in zip(instances, BOXES, FLIPS):
        k, h0, w0 = m.shape
        x1, y1, x2, y2 = box
        fb = (IMAGE_SIZE[0] - x2, y1, IMAGE_SIZE[0] - x1, y2) if f else box
        descs_f.append((off, k, t, h0, w0, *fb))
        descs_u.append((off, k, t, h0, w0, *box))
        chunks.append(torch.from_numpy(m.reshape(-1)))
        off += m.size
    masks = torch.cat(chunks).to(DEV)
    flip = torch.tensor(FLIPS, dtype=torch.int32, device=DEV)
    got = roi_targets(masks, descs_f, mask_size, IMAGE_SIZE, flip).cpu().numpy()
    plain = roi_targets(masks, descs_u, mask_size, IMAGE_SIZE).cpu().numpy()
    none = roi_targets(masks, descs_u, mask_size, IMAGE_SIZE, torch.zeros_like(flip)).cpu().numpy()
    np.testing.assert_array_equal(none, plain)
    mirror_differs = 0
    for i, ((m, _, t), box, f) in enumerate(zip(instances, BOXES, FLIPS)):
        if f:
            want, _ = AO.flipped_target(m, t, box, mask_size, IMAGE_SIZE)
            mirror_differs += int(not np.array_equal(want, plain[i][:, ::-1]))
        else:
            want = AO.unflipped_target(m, t, box, mask_size, IMAGE_SIZE)
            np.testing.assert_array_equal(plain[i], want)
        np.testing.assert_array_equal(got[i], want, err_msg=f"sample {i}")
    assert mirror_differs >= 1          # the flipped target is not the mirrored unflipped one
    assert set(np.unique(got)) == {0, 1, 2}


def _samples(instances):
    rng = np.random.default_rng(23)
    return [{"image": rng.integers(0, 256, size=(*m.shape[1:], 3), dtype=np.uint8), "instance_masks": m,
             "bboxes": boxes, "target": t, "image_id": i} for i, (m, boxes, t) in enumerate(instances)]


def test_builder_with_augmentation_equals_the_oracle_pipeline(instances):
    import oracle.data as OD
    from hiseg.augment import RoiSafeAugmentation, out_table
    from hiseg.data import GpuRoiBatchBuilder
    samples = _samples(instances)
    mask_size, pad = (56, 56), 0.1
    b = GpuRoiBatchBuilder(DEV, mask_size=mask_size, image_size=IMAGE_SIZE, roi_padding=pad,
                           augment=RoiSafeAugmentation("light", seed=3)).build(samples)
    params = b["aug_params"]
    flips = params.host["flip"]
    assert 0 < flips.sum() < len(samples) and params.ran[:, 0].any()    # seed 3 draws both kinds
    np.testing.assert_array_equal(params.flip.cpu().numpy(), flips)
    tab = out_table("normalize")
    W = IMAGE_SIZE[0]
    for i, s in enumerate(samples):
        img = OD.pil_resize(s["image"], IMAGE_SIZE)
        want, acc = AO.augment(img, params.host[i], tab, with_sum=True)
        assert acc is None, "seed 3 draws no blur for these six samples (byte equality below)"
        np.testing.assert_array_equal(b["image"][i].cpu().numpy(), want, err_msg=f"image {i}")
        box = AO.roi_box(s["bboxes"], s["target"], s["image"].shape[:2], IMAGE_SIZE, pad)
        if flips[i]:
            target, box = AO.flipped_target(s["instance_masks"], s["target"], box, mask_size, IMAGE_SIZE)
        else:
            target = AO.unflipped_target(s["instance_masks"], s["target"], box, mask_size, IMAGE_SIZE)
        np.testing.assert_array_equal(b["roi_masks"][i].cpu().numpy(), target, err_msg=f"roi mask {i}")
        norm = np.array([i, box[0] / W, box[1] / IMAGE_SIZE[1], box[2] / W, box[3] / IMAGE_SIZE[1]], np.float32)
        np.testing.assert_array_equal(b["roi_boxes"][i].cpu().numpy(), norm)


def test_builder_without_augmentation_is_unchanged(instances):
    import oracle.data as OD
    from hiseg.data import GpuRoiBatchBuilder
    samples = _samples(instances)
    b = GpuRoiBatchBuilder(DEV, mask_size=(56, 56), image_size=IMAGE_SIZE, augment=None).build(samples)
    assert "aug_params" not in b
    for i, s in enumerate(samples):
        img, roi_mask, norm = OD.get_item(s["image"], s["instance_masks"], s["bboxes"], s["target"], (56, 56),
                                          IMAGE_SIZE, 0.0)
        np.testing.assert_array_equal(b["image"][i].cpu().numpy(), img)
        np.testing.assert_array_equal(b["roi_masks"][i].cpu().numpy(), roi_mask)
        np.testing.assert_array_equal(b["roi_boxes"][i].cpu().numpy(), np.array([i, *norm], np.float32))


def test_graph_capture_replays_with_new_parameters_and_bad_arguments_raise():
    from hiseg import _lib as L
    from hiseg.augment import AugParams, RoiSafeAugmentation, augment_images, gaussian_kernel, hsv_shift_luts
    imgs = torch.from_numpy(_batch(13)).to(DEV)
    first = AugParams(4).set(1, flip=True, hsv_luts=hsv_shift_luts(5, 5, 5)).set(2, kernel=gaussian_kernel(5, 1.0))
    second = RoiSafeAugmentation("heavy-subset", seed=1).sample(4).set(0, flip=True, kernel=gaussian_kernel(7, 2.0))
    static = AugParams(4).copy_(first).to(DEV)
    out = torch.empty(4, 3, 45, 70, dtype=torch.float32, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        augment_images(imgs, static, out=out)                       # warm-up: tables cached before the capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        augment_images(imgs, static, out=out)
    for src in (first, second):
        static.copy_(src)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        eager = augment_images(imgs, AugParams(4).copy_(src).to(DEV))
        assert torch.equal(out, eager)
    assert not torch.equal(out, augment_images(imgs, AugParams(4).copy_(first).to(DEV)))
    bad = AugParams(4)
    bad.host["ksize"][2] = 4
    with pytest.raises(L.HisegError, match="ksize"):
        bad.to(DEV)
    with pytest.raises(L.HisegError, match="ksize"):
        static.copy_(bad)
    static.host["ksize"][0] = 9
    with pytest.raises(L.HisegError, match="ksize"):
        augment_images(imgs, static)
    with pytest.raises(L.HisegError, match="shape"):
        augment_images(imgs[:, :3].contiguous(), AugParams(4).to(DEV))
