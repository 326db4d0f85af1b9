"""Shared makers of the calibration tests (test_calibration_cpu.py, test_calibration_gpu.py): predicted labels, their
confidences and ground truth in raw values, and the check that a reference table is worth comparing against."""
import torch

from test_pseudo_gpu import flat_labels, make_conf  # noqa: F401  (runs of one class or a class per pixel; the special values)


def gt_dtype(n, dtype=None):
    return dtype if dtype is not None else (torch.uint8 if n < 255 else torch.int16)


def ground_truth(labels, n, dtype, seed, raw_labels=True):
    """ground truth of the labels' shape in the rule's encoding: the label's own class on a random half of the pixels, a
    random class elsewhere, sprinkled with the two ignore values and, for int16, values outside the classes"""
    g = torch.Generator().manual_seed(6000 + seed)
    lab = labels.long()
    shift = 1 if raw_labels else 0
    own = lab.clamp(0, n - 1) + shift
    other = torch.randint(0, n, lab.shape, generator=g) + shift
    gt = torch.where(torch.rand(lab.shape, generator=g) < 0.5, own, other)
    if dtype == torch.uint8:
        gt = torch.where(gt == 255, torch.full_like(gt, shift), gt)       # 255 is an ignore value, not class 254
    ign = (0, 255) if raw_labels else (n, 255)
    sprinkle = list(ign) + ([n + 2, -1, 600, -32768, 32767] if dtype == torch.int16 else [])
    sprinkle = [v for v in sprinkle if dtype == torch.int16 or v <= 255]
    npix = lab.numel()
    if npix > 16:
        flat = gt.reshape(-1)
        where = torch.randint(0, npix, (max(npix // 16, len(sprinkle)),), generator=g)
        flat[where] = torch.tensor(sprinkle)[torch.arange(where.numel()) % len(sprinkle)]
    return gt.to(dtype)


def maps(npix, n, label_dtype, gdt, seed, random=False, raw_labels=True):
    """-> (labels, conf, gt), flat, on the host"""
    labels = flat_labels(npix, n, label_dtype, seed, random)
    return labels, make_conf((npix,), seed + 1), ground_truth(labels, n, gdt, seed + 2, raw_labels)


def telling(calibration, tally):
    """a reference table that a comparison can fail against: hits and misses in more than one bin each, and scored pixels
    with a label outside the classes"""
    hits, misses = calibration[..., 1].sum(0), calibration[..., 0].sum(0)
    return int((hits > 0).sum()) > 1 and int((misses > 0).sum()) > 1 and int(tally[1]) > 0
