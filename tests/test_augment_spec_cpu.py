"""CPU: the specification of the augmentation family (`ifseg_amd.augment`) against records and images written down before its
shared pieces were folded (tests/golden/augment_spec.npz: the outputs of `draw_params`, `strong_draw_reference` and
`strong_apply_reference` on the inputs this module builds), and the two rules the shared pieces must keep: the photometric
gate closes the four "on" words only, and `photometric` reads a strong record at its own base."""
import os

import numpy as np
import torch

from ifseg_amd import augment as A

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment_spec.npz")
SEEDS, ORDINALS, SAMPLES = (5, 2 ** 64 - 3), (0, 2 ** 32 - 8), 8
P, NSEG = 16, 7


def label_maps():
    """eight uint8 label maps of different sizes, blocks of 9 raw values (0 and 255 among them: 'unknown')"""
    out = []
    for b in range(SAMPLES):
        H0, W0 = 24 + 5 * b, 61 - 4 * b
        y, x = torch.arange(H0)[:, None], torch.arange(W0)[None, :]
        v = ((y // 7) * 3 + (x // 5) * 5 + b) % 9
        out.append(torch.where(v == 8, torch.full_like(v, 255), v).to(torch.uint8))
    return out


def strong_records():
    """int32 [2, 16]: a valid record with every operation on, a blur and a negative delta; the same with a flag of 2"""
    rec = A.strong_draw_reference(1, 5, 0, 256, 256)[0].tolist()
    rec[A.S_BRIGHT:A.S_HUE + 1] = [1, 1, 1, 1]
    rec[A.S_DELTA] = -7
    rec[A.S_SIGMA], rec[A.S_W0:A.S_W0 + 5] = 40, A.BLUR_WEIGHTS[40].tolist()
    bad = list(rec)
    bad[A.S_BRIGHT] = 2
    return torch.tensor([rec, bad], dtype=torch.int32)


def strong_images(dtype):
    """[2, 3, 16, 16] of table values"""
    lut = A.normalisation_table()
    b, c, y, x = (torch.arange(n).reshape(s) for n, s in ((2, (2, 1, 1, 1)), (3, (1, 3, 1, 1)), (16, (1, 1, 16, 1)), (16, (1, 1, 1, 16))))
    q = (37 * y + 11 * x * x + 83 * c + 129 * b + (x // 4) * (y // 4) * 19) % 256
    return torch.stack([lut[k][q[:, k]] for k in range(3)], 1).to(dtype).contiguous()


def compute():
    """every array of the golden file, from the module as it stands"""
    labels = label_maps()
    shapes = [tuple(l.shape) for l in labels]
    out = {}
    for i, seed in enumerate(SEEDS):
        for j, first in enumerate(ORDINALS):
            out["train_%d_%d" % (i, j)] = A.draw_params(shapes, labels, P, NSEG, seed, first).numpy()
            out["strong_%d_%d" % (i, j)] = A.strong_draw_reference(SAMPLES, seed, first).numpy()
    rec = strong_records()
    out["apply_fp32"] = A.strong_apply_reference(rec, strong_images(torch.float32)).numpy().view(np.int32)
    out["apply_bf16"] = A.strong_apply_reference(rec, strong_images(torch.bfloat16)).view(torch.int16).numpy()
    return out


def test_specification_gives_the_recorded_bits():
    want = np.load(GOLDEN)
    got = compute()
    assert sorted(want.files) == sorted(got)
    for k in want.files:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    # what was recorded is worth comparing: a valid sample without a NaN, a poisoned one that is nothing else
    for k, nan in (("apply_fp32", lambda a: np.isnan(a.view(np.float32))), ("apply_bf16", lambda a: (a & 0x7fff) > 0x7f80)):
        assert not nan(want[k][0]).any() and nan(want[k][1]).all(), k


def test_photometric_gate_closes_the_four_on_words_only():
    labels = label_maps()
    shapes = [tuple(l.shape) for l in labels]
    on = A.draw_params(shapes, labels, P, NSEG, SEEDS[0], 0)
    off = A.draw_params(shapes, labels, P, NSEG, SEEDS[0], 0, photometric=False)
    assert bool((off[:, A.R_BRIGHT:A.R_HUE + 1] == 0).all()) and bool((on[:, A.R_BRIGHT:A.R_HUE + 1] != 0).any())
    assert torch.equal(off[:, A.R_MODE:A.R_DELTA + 1], on[:, A.R_MODE:A.R_DELTA + 1])      # words 10-14 are still drawn
    assert torch.equal(off[:, :A.R_BRIGHT], on[:, :A.R_BRIGHT]) and bool((on[:, A.R_MODE:A.R_DELTA + 1] != 0).any())


def test_photometric_reads_a_strong_record_at_its_own_base():
    rec = strong_records()[0].tolist()
    train = [0] * A.RECORD
    for k_train, k in ((A.R_BRIGHT, A.S_BRIGHT), (A.R_CONTRAST, A.S_CONTRAST), (A.R_SAT, A.S_SAT), (A.R_HUE, A.S_HUE), (A.R_MODE, A.S_MODE),
                       (A.R_BETA, A.S_BETA), (A.R_ALPHA_C, A.S_ALPHA_C), (A.R_ALPHA_S, A.S_ALPHA_S), (A.R_DELTA, A.S_DELTA)):
        train[k_train] = rec[k]
    train[A.R_DELTA] %= 180
    y, x = np.arange(16)[:, None], np.arange(16)[None, :]
    rgb = np.stack([(37 * y + 11 * x) % 256, (5 * y * y + 3 * x) % 256, (91 * x + y) % 256], -1)
    for mode in (0, 1):
        rec[A.S_MODE] = train[A.R_MODE] = mode
        want = A.photometric(rgb, train)
        assert np.array_equal(A.photometric(rgb, rec, base=A.S_BRIGHT), want) and np.array_equal(A.photometric(rgb, train, base=A.R_BRIGHT), want)
        assert not np.array_equal(want, rgb.astype(np.uint8))
