"""Inputs shared by test_boundary_cpu.py and test_boundary_gpu.py: block label maps whose contours do not coincide, and the
reference's answer for each, computed once per process.

TABLE holds (h, w, d, bh, bw).  The ground truth's raw values 1 .. n fill blocks of (bh, bw) pixels (n = the number of blocks),
with a few 0 and 255 pixels; the prediction is the same blocks shifted by (2, 3) pixels, as class ids.  The shapes cut into
several ragged 16 x 64 tiles on both axes; d sits on both sides of the small label halo's limit (4), at 16 / 17, and at the
kernel's maximum (64).  For every entry the gt band, the pred band, both interiors among the scored pixels and bareas[0] are
non-empty: `nonempty` states that, and the tests assert it on the reference before they compare anything."""
import functools

import torch

TABLE = [(37, 91, 1, 8, 12), (37, 91, 2, 12, 20), (33, 130, 4, 16, 30), (70, 150, 5, 24, 40), (96, 200, 16, 48, 90),
         (96, 200, 17, 48, 90), (150, 260, 33, 75, 120), (300, 400, 64, 140, 180)]
IDS = ["%dx%d_d%d" % e[:3] for e in TABLE]
DTYPES = {"u8": torch.uint8, "i16": torch.int16}


def classes(entry):
    h, w, _, bh, bw = entry
    return -(-h // bh) * -(-w // bw)


def _blocks(h, w, bh, bw, dy=0, dx=0):
    """raw values 1 .. n in blocks of (bh, bw), the block grid shifted down by dy and right by dx (the first block grows)"""
    y = (torch.arange(h) - dy).clamp(min=0) // bh
    x = (torch.arange(w) - dx).clamp(min=0) // bw
    return 1 + y[:, None] * -(-w // bw) + x[None, :]


def maps(entry, ldt=torch.uint8, gdt=torch.uint8, raw=True, outside=False):
    """-> (labels [h, w] of ldt, gt [h, w] of gdt, n)"""
    h, w, _, bh, bw = entry
    n = classes(entry)
    gt = _blocks(h, w, bh, bw)
    for k, (y, x) in enumerate(((0, 0), (h - 1, w - 1), (h // 2, 0), (0, w // 2), (h - 1, w // 3), (h // 3, w - 1))):
        gt[y, x] = 0 if k % 2 == 0 else 255                     # ignore values, values of their own for the band
    labels = _blocks(h, w, bh, bw, 2, 3) - 1
    if outside:       # labels outside [0, n): a run along a row, and single pixels
        values = [n, 255] + ([-1, 32767] if ldt == torch.int16 else [])
        for k, v in enumerate(values):
            labels[(5 + 7 * k) % h, w // 4:w // 4 + 9] = v
            labels[(11 + 5 * k) % h, (w // 2 + 13 * k) % w] = v
    if not raw:       # class ids: n and 255 are the ignore values
        gt = torch.where(gt == 0, torch.full_like(gt, n), torch.where(gt == 255, gt, gt - 1))
    return labels.to(ldt), gt.to(gdt), n


@functools.lru_cache(maxsize=None)
def reference(k, ldt="u8", raw=True, outside=False):
    """entry k of TABLE -> (bareas, band, areas) of the specification; the ground truth's dtype does not change the values"""
    from ifseg_amd.predict import areas_reference, boundary_areas_reference
    labels, gt, n = maps(TABLE[k], DTYPES[ldt], torch.int16, raw, outside)
    bareas, band = boundary_areas_reference(labels, gt, n, TABLE[k][2], raw)
    return bareas, band, areas_reference(labels, gt, n, raw)[0]


def nonempty(k, ldt="u8", raw=True, outside=False):
    """the condition on the inputs: both bands, both interiors among the scored pixels, and the intersection row are there"""
    bareas, band, areas = reference(k, ldt, raw, outside)
    return (bool((band & 1).any()) and bool((band & 2).any()) and int(bareas[2].sum()) < int(areas[2].sum())
            and int(bareas[1].sum()) < int(areas[1].sum()) and int(bareas[0].sum()) > 0 and int(bareas[1].sum()) > 0
            and int(bareas[2].sum()) > 0)
