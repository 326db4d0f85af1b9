"""Inputs, references and the comparison rule shared by test_predict_cpu.py and test_predict_gpu.py.

Exact family: integer scores in [-8, 8] at x16.  Every bilinear weight is a multiple of 1/32 per axis, so every product is a
multiple of 1/1024 and every sum is exact in fp32: fp32 == fp64 and any summation order or FMA contraction gives the same
bits.  Many pixels are exact ties, which exercises the first-maximum rule.

General family: randn scores (raw, and softmaxed), arbitrary ratios.  The reference is the fp64 specification; `e` is
max |fp32 specification - fp64 specification| on the same input, computed by the test.  Values must agree within 4 e (the
kernel's flat four-weight rule in fp32 has the error of the fp32 specification; the factor covers FMA contraction and the
differently rounded coordinate); labels must agree wherever the reference's top-2 margin is >= 32 e; the pixels below that
margin are left out, and must be at most 1 % of the case (MARGIN_CAP) -- the CPU file asserts that for every case.
"""
import torch

from ifseg_amd.predict import upsample_argmax_reference

EXACT_SHAPES = [(2, 3, 5, 15), (1, 2, 2, 150), (3, 4, 3, 257), (1, 2, 3, 512), (1, 1, 1, 1)]       # (B, hp, wp, n), h = 16 hp
GENERAL_SHAPES = [(8, 8, 15, 100, 75), (4, 6, 150, 37, 91), (8, 12, 5, 127, 200), (2, 2, 15, 33, 31), (8, 8, 15, 5, 3),
                  (1, 1, 7, 9, 4), (32, 32, 150, 500, 375)]                                         # (hp, wp, n, h, w)
# a footprint no staging buffer holds (the whole 40 x 40 grid of 512 classes under one tile): the direct path without a switch
DIRECT_SHAPES = [(40, 40, 512, 20, 20), (24, 20, 257, 9, 70)]
SEEDS = tuple(range(1, 8))
VALUE_FACTOR, MARGIN_FACTOR, MARGIN_CAP = 4.0, 32.0, 0.01


def exact_scores(shape):
    B, hp, wp, n = shape
    g = torch.Generator().manual_seed(1000 + 7 * n + hp)
    return torch.randint(-8, 9, (B, hp * wp, n), generator=g).float()


def general_scores(shape, seed, softmaxed, batch=1):
    hp, wp, n, h, w = shape
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(batch, hp * wp, n, generator=g)
    return s.softmax(-1) if softmaxed else s


class Reference:
    """fp64 specification of one case + the error scale e and the mask of the pixels whose label is decided"""

    def __init__(self, scores, hp, wp, h, w):
        scores = scores.detach().float().cpu()
        self.labels, self.conf, self.probs = upsample_argmax_reference(scores, hp, wp, h, w, torch.float64)
        p32 = upsample_argmax_reference(scores, hp, wp, h, w, torch.float32)[2]
        self.e = (p32.double() - self.probs).abs().max().item()
        if self.probs.shape[1] > 1:
            top2 = self.probs.topk(2, dim=1).values
            self.decided = (top2[:, 0] - top2[:, 1]) >= MARGIN_FACTOR * self.e
        else:
            self.decided = torch.ones_like(self.labels, dtype=torch.bool)
        self.undecided_share = 1.0 - self.decided.float().mean().item()

    def check(self, labels, conf=None, probs=None, what=""):
        """asserts the comparison rule on device results"""
        assert self.undecided_share <= MARGIN_CAP, (what, self.undecided_share)
        tol = VALUE_FACTOR * self.e
        lab = labels.cpu().long()
        assert lab.shape == self.labels.shape, (what, lab.shape, self.labels.shape)
        bad = (lab != self.labels) & self.decided
        assert not bad.any(), (what, int(bad.sum()), "label mismatches on decided pixels")
        if probs is not None:
            d = (probs.cpu().double() - self.probs).abs().max().item()
            assert d <= tol, (what, "probs", d, tol)
        if conf is not None:
            # the winning value: within tol of the reference's maximum everywhere (an undecided pixel may name another class,
            # whose value then lies within 32 e + tol of the maximum -- compare against the reference value OF THE NAMED class)
            ref = self.probs.gather(1, lab[:, None]).squeeze(1)
            d = (conf.cpu().double() - ref).abs().max().item()
            assert d <= tol, (what, "conf", d, tol)


# ---- the end-to-end fixture: the segofa_tiny 128 x 128, 5-class model of tests/test_model_gpu.py, B = 2
E2E_SEED = 777
E2E_PROMPT = (17, 23, 42, 8)                                   # ids inside the fixture's 100-token vocabulary
E2E_NAMES = [[31], [32, 33], [34], [35, 36, 37], [38]]         # five "category names"


def e2e_fixture():
    """-> (oracle config, state dict with a diversified seg projection, normalised images [2, 3, 128, 128], source tokens [L])"""
    import segofa_ref as O
    from ifseg_amd.predict import source_tokens
    ocfg = O.fixture_config()
    sd = O.procedural_state_dict(ocfg)
    img = O.synthetic_batch(ocfg, 2, 12, seed=E2E_SEED)["patch_images"]
    src = source_tokens(E2E_NAMES, E2E_PROMPT, ocfg.num_seg_tokens)
    sd = O.diversify_seg_projection(sd, ocfg, {"src_tokens": src[None].repeat(2, 1), "patch_images": img})
    return ocfg, sd, img, src
