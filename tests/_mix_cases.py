"""Inputs shared by test_mix_cpu.py and test_mix_gpu.py: batches in `train_sample`'s layout (images, target, weight plane) for
the batch mix (`ifseg_amd.augment`: mix_draw_reference / mix_apply_reference; csrc/mix.hip), built on the host from a seed,
computed once per case and never written to.

The shapes are the smallest at which the kernels can go wrong: P = 16 (256 pixels: 32 of a workgroup's 256 threads hold a run
of 8 pixels) with B = 1, 2, 3 (an odd row of the target starts 8 bytes off a 16-byte boundary), and P = 48 (2304 pixels: 288
runs, a second, ragged workgroup)."""
import functools

import torch

SEG0 = 1000
EOS = 2
IMPOSTOR = SEG0 + 2 ** 32 + 3                   # class 3 in 32 bits, no class in 64
SHAPES = [(1, 16), (2, 16), (3, 16), (3, 48)]   # (B, P)
NSEGS = [1, 15, 33, 255]
SEED = 5


def _with_eos(body):
    return torch.cat([body, torch.full((body.shape[0], 1), EOS, dtype=torch.int64)], 1)


@functools.lru_cache(maxsize=None)
def block_target(B, P, nseg, seed=0):
    """int64 [B, P*P + 1]: 4 x 4 blocks of classes in [0, nseg] ('unknown' included), a few single pixels of other classes, a
    poisoned -1 and the 64-bit impostor"""
    g = torch.Generator().manual_seed(100 * P + 10 * nseg + seed)
    cls = torch.randint(0, nseg + 1, (B, P // 4, P // 4), generator=g).repeat_interleave(4, 1).repeat_interleave(4, 2).clone()
    cls[:, 1, 2] = (cls[:, 1, 2] + 1) % (nseg + 1)
    cls[:, P - 1, P - 1] = (cls[:, P - 1, P - 1] + 1) % (nseg + 1)
    tgt = cls.reshape(B, P * P) + SEG0
    tgt[:, 5] = -1
    tgt[:, 6] = IMPOSTOR
    return _with_eos(tgt)


@functools.lru_cache(maxsize=None)
def special_target(P=16):
    """int64 [3, P*P + 1] for nseg = 33: sample 0 holds classes 31 and 32 (the choice crosses the word boundary) and 3 others,
    sample 1 'unknown' only, sample 2 the impostor, -1, an id below seg_id_offset and nothing else"""
    n = P * P
    t = torch.full((3, n), SEG0 + 33, dtype=torch.int64)
    for k, c in enumerate((31, 32, 0, 7, 30)):
        t[0, k * 40:(k + 1) * 40] = SEG0 + c
    t[2, : n // 3] = IMPOSTOR
    t[2, n // 3: 2 * n // 3] = -1
    t[2, 2 * n // 3:] = SEG0 - 1
    return _with_eos(t)


@functools.lru_cache(maxsize=None)
def full_target():
    """int64 [1, 257] for nseg = 255 at P = 16: 255 distinct classes, one pixel each, and one pixel of 'unknown'"""
    g = torch.Generator().manual_seed(255)
    return _with_eos((torch.randperm(256, generator=g) + SEG0)[None])


def class_target(classes, P=16):
    """int64 [1, P*P + 1] holding exactly the given classes (and 'unknown' = the id behind the largest possible class, 255)"""
    t = torch.full((P * P,), SEG0 + 255, dtype=torch.int64)
    for k, c in enumerate(classes):
        t[k] = SEG0 + c
    return _with_eos(t[None])


@functools.lru_cache(maxsize=None)
def images(B, P, dtype, seed):
    """[B, 3, P, P] with NaNs of several payloads, -0.0 and infinities among random values"""
    g = torch.Generator().manual_seed(7 * P + B + 1000 * seed)
    x = torch.randn(B, 3, P, P, generator=g)
    bits = x.view(torch.int32)
    flat = bits.view(-1)
    flat[0::97] = 0x7fc00000 + seed                 # quiet NaNs, the payload names the batch
    flat[1::101] = -0x00400000 + 0x10000 * seed     # 0xffc.....: negative NaNs with a payload in the upper half (survives bf16)
    flat[2::89] = -0x80000000                       # -0.0
    flat[3::83] = 0x7f800000
    if dtype == torch.bfloat16:
        return (bits >> 16).to(torch.int16).view(torch.bfloat16)
    return x


@functools.lru_cache(maxsize=None)
def weights(B, P, seed):
    g = torch.Generator().manual_seed(31 * P + B + seed)
    w = torch.randint(0, 256, (B, P * P), generator=g, dtype=torch.uint8)
    w[:, :8] = 255 if seed else 0
    return w


def as_int(img):
    """the integer view images are compared through"""
    return img.contiguous().view(torch.int32 if img.dtype == torch.float32 else torch.int16)


def both_record(B, P, class_records):
    """a caller's records: the drawn classes AND a box, which for odd b reaches outside the image on every side it can"""
    rec = class_records.clone()
    for b in range(B):
        rec[b, 8:12] = torch.tensor([-5, P - 7, 9, P + 10] if b % 2 else [3, 2, P // 2 + 1, P // 2 - 3], dtype=torch.int32)
    return rec
