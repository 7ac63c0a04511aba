"""Time of one BatchPreparer.prepare() call (ms, median of 50 eager calls after warm-up, one
process on the GPU) at the two shapes of the shipped configs:

  train  B = 8, N = 1000, 128x128, no pooling, augmentation on          (configs/train_SNN.yml)
  eval   B = 1, N = 15000, 256x256 -> 128x128, hot filter on, full-resolution gtflow
                                                                        (configs/eval_MVSEC.yml)

    python tools/loader_time.py

Each call is timed with a HIP event pair on the launch stream, so the figure includes the
host's launch overhead whenever the host is the slower side (it is: 2-5 small kernels).
"""
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "snn_event-based_optical_flow_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import snnflow  # noqa: E402

MECH = ["Horizontal", "Vertical", "Polarity"]


def window(prep, B, N, gen, dev, busy, gt):
    """One window of raw events: uniform pixels, a quarter of the events on the `busy` pixels."""
    H0, W0 = prep.resolution
    xs = torch.randint(0, W0, (B, N), generator=gen, device=dev).float()
    ys = torch.randint(0, H0, (B, N), generator=gen, device=dev).float()
    if busy is not None:
        pick = busy[torch.arange(N // 4, device=dev) % busy.numel()]
        xs[:, :N // 4], ys[:, :N // 4] = (pick % W0).float(), (pick // W0).float()
    ts = torch.rand(B, N, generator=gen, device=dev).sort(dim=1).values
    ps = torch.randint(0, 2, (B, N), generator=gen, device=dev).float()
    gtflow = torch.randn(B, 2, H0, W0, generator=gen, device=dev) if gt else None
    return xs, ys, ts, ps, None, gtflow


def measure(name, cfg, num_bins, B, N, gt, launches, pool=8, calls=50, warmup=10):
    """pool: distinct windows cycled through.  With the hot filter on, 300 pixels fire in every
    window (more candidates than max_px: the selection runs on every call); pool = 1 repeats one
    window, which makes every pixel it hits a candidate of rate 1 -- the selection's worst case,
    thousands of candidates tied at the cut."""
    dev = torch.device("cuda:0")
    np.random.seed(0)
    prep = snnflow.BatchPreparer(cfg, num_bins, device=dev)
    H0, W0 = prep.resolution
    gen = torch.Generator(device=dev).manual_seed(1)
    busy = torch.randint(0, H0 * W0, (300,), generator=gen, device=dev) if prep.hot_enabled else None
    wins = [window(prep, B, N, gen, dev, busy, gt) for _ in range(pool)]
    times = []
    for i in range(warmup + calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        prep.prepare(*wins[i % pool])
        b.record()
        torch.cuda.synchronize(dev)
        if i >= warmup:
            times.append(a.elapsed_time(b))
    ms = statistics.median(times)
    print(f"{name}: {ms:.4f} ms per prepare (median of {calls}, min {min(times):.4f}, max {max(times):.4f}), "
          f"{launches} kernel launches per call")
    return ms


def main():
    train = {"data": {"mode": "events"},
             "loader": {"resolution": [128, 128], "std_resolution": [256, 256], "batch_size": 8, "augment": MECH,
                        "augment_prob": [0.5, 0.5, 0.5]},
             "hot_filter": {"enabled": False}}
    evalc = {"data": {"mode": "gtflow_dt1"},
             "loader": {"resolution": [128, 128], "std_resolution": [256, 256], "batch_size": 1, "augment": [],
                        "augment_prob": [], "keep_gt_full_res": True},
             "hot_filter": {"enabled": True, "max_px": 100, "min_obvs": 5, "max_rate": 0.8}}
    measure("train B=8 N=1000 128x128", train, 2, 8, 1000, False, 2)
    measure("eval  B=1 N=15000 256x256->128x128 hot", evalc, 2, 1, 15000, True, 5)
    measure("eval  the same, one window repeated (worst-case selection)", evalc, 2, 1, 15000, True, 5, pool=1)


if __name__ == "__main__":
    main()
