"""Inputs shared by test_score_cpu.py and test_score_gpu.py: ground truth for the scoring counters of ifseg_amd/predict.py
(`areas_reference` is the specification; the counters are integers, so every comparison is exact).

`ground_truth` draws valid classes with about 10 % ignore values (both ignore values of the rule in turn), `every_kind` lists one
value of each kind the rule tells apart, `kind` is the rule written out value by value, independently of `areas_reference`."""
import torch

IGNORE_SHARE = 0.1


def kind(v, n, raw_labels):
    """one ground-truth value -> its class, -1 (ignored) or -2 (out of range)"""
    if raw_labels:
        if v in (0, 255):
            return -1
        c = v - 1
    else:
        if v in (n, 255):
            return -1
        c = v
    return c if 0 <= c < n else -2


def valid_values(n, raw_labels, dtype):
    """every value of `dtype` that names a class"""
    lo, hi = (0, 255) if dtype == torch.uint8 else (-300, 600)
    return [v for v in range(lo, hi + 1) if kind(v, n, raw_labels) >= 0]


def ground_truth(shape, n, raw_labels=True, seed=0, dtype=torch.uint8, ignore=IGNORE_SHARE):
    """random ground truth of `shape`: classes of [0, n) in the rule's encoding, a share `ignore` of ignore values"""
    g = torch.Generator().manual_seed(4000 + seed)
    vals = torch.tensor(valid_values(n, raw_labels, dtype))
    out = vals[torch.randint(0, len(vals), shape, generator=g)]
    ign = torch.tensor([0, 255] if raw_labels else [n, 255])
    ign = ign[ign <= (255 if dtype == torch.uint8 else 32767)]
    drop = torch.rand(shape, generator=g) < ignore
    out = torch.where(drop, ign[torch.randint(0, len(ign), shape, generator=g)], out)
    return out.to(dtype)


def every_kind(n, raw_labels, dtype):
    """one value of every kind: both ignore values, n and n + 1, the first and the last class, out of range on both sides"""
    vals = [0, 255, n, n + 1, 1, n - 1, n + 2, 254] + ([-1, -7, 300, 600] if dtype == torch.int16 else [])
    hi = 255 if dtype == torch.uint8 else 32767
    return [v for v in vals if (0 if dtype == torch.uint8 else -32768) <= v <= hi]


def labels_and_gt(n, raw_labels, dtype, seed=0, size=(37, 29)):
    """random predictions in [0, n) and ground truth holding every kind of value among random classes -> (labels int64, gt)"""
    g = torch.Generator().manual_seed(5000 + seed + n)
    labels = torch.randint(0, n, size, generator=g)
    gt = ground_truth(size, n, raw_labels, seed + n, dtype).reshape(-1)
    special = torch.tensor(every_kind(n, raw_labels, dtype)).repeat(3).to(dtype)
    gt[torch.randperm(gt.numel(), generator=g)[:special.numel()]] = special
    # half of the scored pixels agree with the prediction, so that the intersection is not nearly empty
    gt = gt.reshape(size)
    cls = torch.tensor([kind(int(v), n, raw_labels) for v in gt.reshape(-1)]).reshape(size)
    agree = (cls >= 0) & (torch.rand(size, generator=g) < 0.5)
    labels = torch.where(agree, cls, labels)
    return labels, gt


def by_hand(labels, gt, n, raw_labels):
    """the counters by the value-by-value rule: (scored mask, class per pixel, out-of-range count)"""
    cls = torch.tensor([kind(int(v), n, raw_labels) for v in gt.reshape(-1)]).reshape(gt.shape)
    return cls >= 0, cls, int((cls == -2).sum())
