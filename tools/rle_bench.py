"""Run-length label maps on the device (csrc/rle.hip: hip.seg_rle_encode / seg_rle_decode; Segmenter.export_raw) against what
a user does without them, per call as enqueued from Python.  One 512 x 683 uint8 map:
  piecewise      classes in blocks of 32 x 32 pixels with 2 % of the pixels flipped to another class: what a segmenter gives
  random         an independent class per pixel, over 5 values
  checkerboard   a run per pixel but at the 682 column seams (H is even): the most stores a map of this size can ask for
and per map
  encode       hip.seg_rle_encode(labels, max_runs=R), R = 2^16 (the piecewise map's runs fit) or 2^19 (every run of the
               other two fits); three launches and two allocations (the segment counts; the zero-filled table)
  cpu+numpy    what a user writes today: labels.cpu() and numpy's flatnonzero(diff(labels.T.ravel())); the copy WAITS for the
               device, which is part of what it costs
  torch        the device composition: labels.t().contiguous().flatten(), !=, nonzero, a gather.  Its nonzero SYNCHRONISES with
               the host (the size of its result is read back), so it cannot be enqueued ahead either
  decode       hip.seg_rle_decode of the encoder's table: one launch
  torch decode the composition the decoder replaces: the lengths by diff, repeat_interleave (which synchronises: the output's
               size is read back) and the transpose back
and `Segmenter.export_raw` against `segment_raw` on SegOFA-Base, per image (--no-model leaves it out), with the bytes of
runs[:count] against the dense map.  The variants of a row alternate window by window in one process; a window is at least
0.5 s of enqueued calls between two device events after a warm-up; the figure is the median over the windows, [min, max] its
run-to-run spread: a difference inside the spread is no difference.  The encoder is checked against the specification, and the
compositions against the encoder, before anything is timed.

    python tools/rle_bench.py [--windows 5] [--window-s 0.5] [--no-model] [--out profiles/rle_bench.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from evaluate_bench import row
from predict_tta_bench import H, P, W
from region_table_bench import maps


def numpy_runs(labels):
    """what a user writes today -> (starts, values) on the host"""
    import numpy as np
    f = labels.cpu().numpy().T.ravel()
    starts = np.concatenate([[0], np.flatnonzero(np.diff(f)) + 1])
    return starts, f[starts]


def torch_runs(labels):
    """the device composition -> (starts, values) on the device; nonzero synchronises"""
    f = labels.t().contiguous().flatten()
    change = torch.ones_like(f, dtype=torch.bool)
    change[1:] = f[1:] != f[:-1]
    starts = change.nonzero().flatten()
    return starts, f[starts]


def torch_decode(starts, values, dtype):
    lengths = torch.diff(starts, append=starts.new_full((1,), H * W))
    return torch.repeat_interleave(values, lengths).reshape(W, H).t().contiguous().to(dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ifseg_amd import hip
    from ifseg_amd.predict import rle_encode_reference
    dev = torch.device("cuda:0")
    lines = ["run-length label maps on the device vs labels.cpu() + numpy (it waits for the device) and vs the device composition "
             "t().contiguous / != / nonzero / gather (its nonzero synchronises): median [min, max] microseconds over %d alternating "
             "windows of >= %.1f s" % (a.windows, a.window_s),
             "one %d x %d uint8 map (%d bytes dense); x = the second variant / the first" % (H, W, H * W), ""]
    for name, lab in maps():
        d = lab.to(dev)
        R = 1 << 16 if name == "piecewise" else 1 << 19
        want = rle_encode_reference(d, R)
        runs, count = hip.seg_rle_encode(d, R)
        k = int(want[1])
        assert k <= R, (name, k, R)
        assert torch.equal(count, want[1]) and torch.equal(runs, want[0]), name
        starts, values = torch_runs(d)
        assert torch.equal(starts, runs[:k, 0].long()) and torch.equal(values.int(), runs[:k, 1]), name
        n_starts, n_values = numpy_runs(d)
        assert n_starts.tolist() == starts.tolist() and n_values.tolist() == values.tolist(), name
        out, flag = hip.seg_rle_decode(runs, count, H, W)
        assert torch.equal(out, d) and int(flag) == 0 and torch.equal(torch_decode(starts, values, d.dtype), d), name
        what = "%-12s %6d runs %7d B" % (name, k, 8 * k)
        row(lines, what + " encode", [lambda: hip.seg_rle_encode(d, R), lambda: numpy_runs(d), lambda: torch_runs(d)],
            ("encode", "cpu+numpy", "torch"), a)
        row(lines, what + " decode", [lambda: hip.seg_rle_decode(runs, count, H, W), lambda: torch_decode(starts, values, d.dtype)],
            ("decode", "torch decode"), a)
    if not a.no_model:
        from ifseg_amd.tasks.mm_tasks.segmentation import SegmentationTask
        lines += ["", "end to end, SegOFA-Base, one raw uint8 %d x %d image; x = segment_raw / export_raw" % (H, W)]
        n = 150
        torch.manual_seed(0)
        g = torch.Generator().manual_seed(7)
        names = [torch.randint(4, 50000, (int(k),), generator=g) for k in torch.randint(1, 4, (n,), generator=g)]
        task = SegmentationTask(num_seg_tokens=n, patch_image_size=P, arch="segofa_base", category_token_ids=names)
        model = task.build_model().to(dev).eval()
        seg = task.build_segmenter(model)
        img = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).to(dev)
        export = lambda: seg.export_raw(img)
        plain = lambda: seg.segment_raw(img)
        m, r = export()[0], plain()[0]
        want = rle_encode_reference(r.labels, 65536)
        k = int(want[1])
        assert k <= 65536 and torch.equal(m.count, want[1]) and torch.equal(m.runs, want[0]) and torch.equal(m.decode(), r.labels)
        row(lines, "n %3d, %6d runs %7d B of %d" % (n, k, 8 * k, H * W), [export, plain], ("export_raw", "segment_raw"), a)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
