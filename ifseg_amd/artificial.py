"""Image-free training samples without a data loader: the `rand_k-L-R` artificial image of the reference
(data/mm_data/segmentation_dataset.py:303-345) in its collater layout (:85-107).

A sample is a random `sh x sw` class map (sh, sw uniform in [L, R), classes uniform in [0, nseg): never the 'unknown'
class), nearest-resized to the patch grid -- the EmbeddingBag ids / ends of the class names and `prev_output_tokens` -- and
to the image -- `text2seg_target`.  On the device it is three launches of csrc/imfree.hip (`ifseg_imfree_draw`,
`ifseg_imfree_expand`); with ``device="cpu"`` this module computes the SAME stream and the SAME index rule in numpy /
torch.  That CPU path is the specification the kernels are compared against bit for bit.

The random stream (the counter generator of the dropout masks, csrc/common.h `splitmix64`), for sample ordinal n:

    u(n, i)      = splitmix64(seed + (n << 32) + i)              mod 2^64
    sh           = l + (((u(n, 0) >> 32) * (r - l)) >> 32)
    sw           = l + (((u(n, 1) >> 32) * (r - l)) >> 32)
    coarse[y][x] = ((u(n, 2 + y*sw + x) >> 32) * nseg) >> 32

The resize is PyTorch's ``nearest``: ``src = min(int(floorf(dst * scale)), in - 1)``, ``scale = float32(in) / float32(out)``
(what torchvision's tensor ``Resize(NEAREST)`` of the reference runs).  The integer rule ``dst * in // out`` is a different
map (in = 84, out = 40 or 640).
"""
import numpy as np
import torch

from . import hip

MAX_NAME_LEN = 16        # csrc/imfree.hip: Lmax
MAX_SIDE = 128           # r <= 129
MAX_PATCHES = 4096
_M64 = (1 << 64) - 1


def parse_artificial_image_type(s):
    """`--artificial-image-type` -> (l, r) of the coarse map's sides, or None for "none" (segmentation_dataset.py:295-323).
    "norand_k" is refused by name: the reference cannot run it either (`artificial_image_prev` is undefined at :329)."""
    s = str(s).strip()
    if s == "none":
        return None
    if s == "rand_k":
        return 1, 33
    parts = s.split("-")
    if parts[0] == "rand_k" and len(parts) == 3:
        try:
            l, r = int(parts[1]), int(parts[2])
        except ValueError:
            raise ValueError("artificial_image_type %r: L and R of rand_k-L-R must be integers" % s)
        if not 1 <= l < r <= MAX_SIDE + 1:
            raise ValueError("artificial_image_type %r: needs 1 <= L < R <= %d" % (s, MAX_SIDE + 1))
        return l, r
    if s == "norand_k":
        raise NotImplementedError("artificial_image_type 'norand_k' is not supported (the reference's own branch fails: "
                                  "artificial_image_prev is never defined for it)")
    raise NotImplementedError("artificial_image_type %r is not supported on the device: rand_k | rand_k-L-R | none" % s)


def splitmix64(z):
    """numpy uint64 -> uint64 (wrapping), csrc/common.h"""
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def nearest_index(n_in, n_out):
    """int64 [n_out]: PyTorch's `nearest` source index for every destination index, in fp32 like the kernels"""
    scale = np.float32(n_in) / np.float32(n_out)
    src = np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(src, n_in - 1)


def trainer_first_ordinal(update, micro, rank, n_micro, world, batch):
    """The ordinal of sample 0 of micro-batch `micro` of rank `rank` in update `update` (0-based):

        ((update * n_micro + micro) * world + rank) * batch

    with n_micro micro-batches per update, `world` ranks and `batch` samples per micro-batch, all fixed for a run.  Sample b
    adds b < batch, so (update, micro, rank, b) -> ordinal is a mixed-radix number: no two samples of a run share one.  It
    depends on nothing but the update counter and the run's shape, so a run resumed at update k draws what the uninterrupted
    run would."""
    assert 0 <= micro < n_micro and 0 <= rank < world and batch >= 1 and update >= 0
    return ((update * n_micro + micro) * world + rank) * batch


class ArtificialImageSampler:
    def __init__(self, names, seg_id_offset, hp, wp, l=1, r=33, seed=1, device="cpu", bos=0, eos=2, pad=1):
        """names: nseg + 1 token-id tensors (the category names, then 'unknown': the reference's `id2text`)."""
        names = [torch.as_tensor(t, dtype=torch.long).reshape(-1).cpu() for t in names]
        self.nseg = len(names) - 1
        if self.nseg < 1 or self.nseg > 65535:
            raise ValueError("ArtificialImageSampler: %d names (needs nseg + 1 with 1 <= nseg <= 65535)" % len(names))
        if not 1 <= l < r <= MAX_SIDE + 1:
            raise ValueError("ArtificialImageSampler: needs 1 <= l < r <= %d, got (%d, %d)" % (MAX_SIDE + 1, l, r))
        if hp < 1 or wp < 1 or hp * wp > MAX_PATCHES or wp > 2048:
            raise ValueError("ArtificialImageSampler: patch grid %dx%d (1 <= hp * wp <= %d)" % (hp, wp, MAX_PATCHES))
        self.Lmax = max(1, max(t.numel() for t in names))
        if self.Lmax > MAX_NAME_LEN:
            raise ValueError("ArtificialImageSampler: a category name of %d tokens (at most %d)" % (self.Lmax, MAX_NAME_LEN))
        self.seg_id_offset, self.hp, self.wp, self.l, self.r = int(seg_id_offset), int(hp), int(wp), int(l), int(r)
        self.seed, self.bos, self.eos, self.pad = int(seed) & _M64, int(bos), int(eos), int(pad)
        self.device = torch.device(device)
        name_ids = torch.full((self.nseg + 1, self.Lmax), self.pad, dtype=torch.long)
        for i, t in enumerate(names):
            name_ids[i, : t.numel()] = t
        self.name_ids = name_ids.to(self.device)
        self.name_len = torch.tensor([t.numel() for t in names], dtype=torch.int32, device=self.device)

    @property
    def max_side(self):
        return self.r - 1

    # ------------------------------------------------------------------ draw
    def draw(self, B, first_ordinal):
        """-> shapes int32 [B, 2], coarse int32 [B, (r-1)^2] of sample ordinals first_ordinal .. first_ordinal + B - 1.
        On the device `first_ordinal` may be an int64 device word, read when the kernel runs."""
        cs = self.max_side * self.max_side
        if self.device.type != "cpu":
            shapes = torch.empty(B, 2, dtype=torch.int32, device=self.device)
            coarse = torch.empty(B, cs, dtype=torch.int32, device=self.device)
            return hip.imfree_draw(self.seed, first_ordinal, B, self.l, self.r, self.nseg, shapes, coarse)
        first = int(first_ordinal)
        if first < 0 or first + B > 1 << 32:
            raise ValueError("ArtificialImageSampler.draw: ordinals must lie in [0, 2^32)")
        shapes = np.zeros((B, 2), dtype=np.int32)
        coarse = np.zeros((B, cs), dtype=np.int32)
        span, nseg = np.uint64(self.r - self.l), np.uint64(self.nseg)
        for b in range(B):
            base = (self.seed + ((first + b) << 32)) & _M64
            with np.errstate(over="ignore"):
                u = splitmix64(np.uint64(base) + np.arange(2, dtype=np.uint64))
                sh, sw = (self.l + int(v) for v in ((u >> np.uint64(32)) * span) >> np.uint64(32))
                u = splitmix64(np.uint64(base) + np.arange(2, 2 + sh * sw, dtype=np.uint64))
                coarse[b, : sh * sw] = (((u >> np.uint64(32)) * nseg) >> np.uint64(32)).astype(np.int32)
            shapes[b] = (sh, sw)
        return torch.from_numpy(shapes), torch.from_numpy(coarse)

    # ---------------------------------------------------------------- expand
    def expand(self, shapes, coarse):
        """shapes int32 [B, 2], coarse int32 [B, max_side^2] (drawn, or the caller's: sides are clamped to [1, max_side],
        classes to [0, nseg]) -> {"ids" [B, P*Lmax], "ends" [B*P], "prev_output_tokens" [B, P+1],
        "text2seg_target" [B, 256*P + 1]}, all int64.  `ids` has the static width P * Lmax (no host sync for the batch
        maximum the reference's collater pads to); everything behind ends[b, P-1] is `pad` and is never read."""
        B, P, Lmax = shapes.shape[0], self.hp * self.wp, self.Lmax
        S_h, S_w = 16 * self.hp, 16 * self.wp
        if tuple(coarse.shape) != (B, self.max_side ** 2):
            raise ValueError("ArtificialImageSampler.expand: coarse must be [B, %d]" % self.max_side ** 2)
        if self.device.type != "cpu":
            new = lambda *s: torch.empty(*s, dtype=torch.long, device=self.device)
            out = {"ids": new(B, P * Lmax), "ends": new(B * P), "prev_output_tokens": new(B, P + 1),
                   "text2seg_target": new(B, S_h * S_w + 1)}
            hip.imfree_expand(shapes.to(self.device, torch.int32).contiguous(), coarse.to(self.device, torch.int32).contiguous(),
                              self.name_ids, self.name_len, self.hp, self.wp, self.seg_id_offset, self.bos, self.eos, self.pad,
                              out["ids"], out["ends"], out["prev_output_tokens"], out["text2seg_target"])
            return out
        ids = torch.full((B, P * Lmax), self.pad, dtype=torch.long)
        ends = torch.empty(B, P, dtype=torch.long)
        prev = torch.empty(B, P + 1, dtype=torch.long)
        target = torch.empty(B, S_h * S_w + 1, dtype=torch.long)
        name_len = self.name_len.long().clamp(0, Lmax)
        for b in range(B):
            sh, sw = (min(max(int(v), 1), self.max_side) for v in shapes[b])
            cm = coarse[b, : sh * sw].long().clamp(0, self.nseg).reshape(sh, sw)
            pick = lambda h, w: cm[torch.from_numpy(nearest_index(sh, h))][:, torch.from_numpy(nearest_index(sw, w))].reshape(-1)
            low = pick(self.hp, self.wp)
            lens = name_len[low]
            ends[b] = lens.cumsum(0)
            keep = torch.arange(Lmax).unsqueeze(0) < lens.unsqueeze(1)          # [P, Lmax]: the tokens of every bag, in order
            toks = self.name_ids[low][keep]
            ids[b, : toks.numel()] = toks
            prev[b, 0] = self.bos
            prev[b, 1:] = self.seg_id_offset + low
            target[b, :-1] = self.seg_id_offset + pick(S_h, S_w)
            target[b, -1] = self.eos
        return {"ids": ids, "ends": ends.reshape(-1), "prev_output_tokens": prev, "text2seg_target": target}

    # ---------------------------------------------------------------- sample
    def sample(self, B, first_ordinal, src_tokens, src_lengths=None):
        """The image-free half of a batch, as `SegOFAModel.forward(aux_input=...)` and the criterion consume it.  The prompt of
        the artificial image is the prompt of the real one (segmentation_dataset.py:272-281 == :331-339)."""
        shapes, coarse = self.draw(B, first_ordinal)
        x = self.expand(shapes, coarse)
        if src_lengths is None:
            src_lengths = src_tokens.ne(self.pad).sum(1)
        return {"aux_input": {"src_tokens": src_tokens, "src_lengths": src_lengths, "patch_images": x["ids"],
                              "patch_masks": x["ends"], "prev_output_tokens": x["prev_output_tokens"]},
                "text2seg_target": x["text2seg_target"]}
