"""hip.image_load (csrc/imgload.hip) against the composition a user had before it, on the same device:

    x = images.permute(0, 3, 1, 2).float()
    x = F.interpolate(x, (oh, ow), mode="bilinear", align_corners=False).add(0.5).floor().clamp(0, 255)
    x = ((x / 255 - mean) / std).to(dtype)

for fp32 and bf16 output.  Two figures per variant, both microseconds PER CALL, neither a kernel time:
  call   eager calls enqueued from Python between two device events (tools/predict_bench.py's windows: the variants alternate
         window by window in one process, a window is at least 0.5 s, the figure is the median).  It is the larger of the
         host's enqueue time and the device's time per call, so a short kernel reads as the host's ~16-20 us here; the
         direct-global variant also makes two more host calls per iteration (it sets and restores the staging limit).
  graph  the same call captured 20 times into one HIP graph and replayed: no host enqueue between the launches, the
         launch-to-launch gap of the device stays in.  This is the figure to compare the staged and the direct path by.
Every row carries its bytes -- the source once (B H0 W0 3) + the output once (B 3 oh ow element size) -- and the bytes per
second they amount to over the graph figure.

    python tools/image_load_bench.py [--windows 5] [--window-s 0.5] [--out profiles/image_load_bench.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import torch.nn.functional as F

from predict_bench import alternate, window          # the same windows and alternation as tools/predict_bench.py

SHAPES = [(8, 480, 640, 512, 683), (8, 1200, 1600, 512, 683)]        # (B, H0, W0, oh, ow): eval_size(., ., 512) of both sources


GRAPH_CALLS = 20


def graph_us(fn, windows, seconds):
    """-> median microseconds per call of `fn` captured GRAPH_CALLS times into one graph, over `windows` windows of replays"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(GRAPH_CALLS):
            fn()
    return statistics.median(window(g.replay, seconds) for _ in range(windows)) / GRAPH_CALLS


def torch_side(images, oh, ow, mean, std, dtype):
    x = images.permute(0, 3, 1, 2).float()
    x = F.interpolate(x, size=(oh, ow), mode="bilinear", align_corners=False).add(0.5).floor().clamp(0, 255)
    return ((x / 255 - mean) / std).to(dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ifseg_amd import hip
    from ifseg_amd.imageio import eval_size
    dev = torch.device("cuda:0")
    mean = torch.full((1, 3, 1, 1), 0.5, device=dev)
    std = torch.full((1, 3, 1, 1), 0.5, device=dev)
    lines = ["%s" % torch.cuda.get_device_name(0),
             "hip.image_load vs permute -> float -> F.interpolate -> round -> normalise -> cast: median [min, max] microseconds over "
             "%d alternating windows of >= %.1f s" % (a.windows, a.window_s),
             "call = eager calls from Python (host enqueue or device, whichever is slower; the direct variant makes two more host calls); "
             "graph = per call inside a replayed graph of %d calls (no host enqueue)" % GRAPH_CALLS,
             "bytes = source once + output once; GB/s = bytes / graph time"]
    for (B, H0, W0, oh, ow) in SHAPES:
        assert (oh, ow) == eval_size(H0, W0, 512)
        img = torch.randint(0, 256, (B, H0, W0, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).to(dev)
        lines.append("")
        lines.append("B %d  %d x %d -> %d x %d" % (B, H0, W0, oh, ow))
        for dt in (torch.bfloat16, torch.float32):
            nbytes = B * H0 * W0 * 3 + B * 3 * oh * ow * (2 if dt == torch.bfloat16 else 4)
            agree = (hip.image_load(img, oh, ow, dtype=dt) == torch_side(img, oh, ow, mean, std, dt)).float().mean().item()
            out = torch.empty(B, 3, oh, ow, dtype=dt, device=dev)
            fns = [lambda: hip.image_load(img, oh, ow, dtype=dt, out=out), lambda: torch_side(img, oh, ow, mean, std, dt),
                   lambda: hip.image_load(img, oh, ow, dtype=dt, staging_bytes=0, out=out)]
            (k, kmin, kmax), (t, tmin, tmax), (d, dmin, dmax) = alternate(fns, a.windows, a.window_s)
            gk, gt, gd = (graph_us(f, a.windows, a.window_s) for f in fns)
            lines.append("  %-5s staged: call %6.1f [%6.1f, %6.1f] graph %6.1f us %7.1f GB/s   direct-global: call %6.1f [%6.1f, %6.1f] graph %6.1f us "
                         "%7.1f GB/s   torch: call %6.1f [%6.1f, %6.1f] graph %6.1f us %7.1f GB/s   torch / staged: call x%5.2f graph x%5.2f   "
                         "bytes %6.2f MB   elements equal to torch's %.4f %%"
                         % ("bf16" if dt == torch.bfloat16 else "fp32", k, kmin, kmax, gk, nbytes / gk / 1e3, d, dmin, dmax, gd, nbytes / gd / 1e3,
                            t, tmin, tmax, gt, nbytes / gt / 1e3, t / k, gt / gk, nbytes / 1e6, 100 * agree))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
