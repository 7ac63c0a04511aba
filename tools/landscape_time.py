"""Time of the contrast-maximisation heatmap at the reference demo's shape (tools/demo_iwe.py defaults:
B = 1, N = 40000 events, 180 x 240, 50 x 50 candidates over +-64 px), two ways, on one process on the GPU:

  landscape  one snnflow.flow_heatmap call (2 kernel launches + a few torch ops)
  loop       what the heatmap cost before: a Python loop of snnflow.EventWarping over the same 2500
             candidates (constant flow map, event_flow_association, forward, reset, one .item() each)

    python tools/landscape_time.py [--calls 20] [--loop-calls 3]

Each call is timed with a HIP event pair on the launch stream and ends in a synchronise, so the figure
includes the host's launch overhead wherever the host is the slower side (the loop: always).  Medians
over the repeated calls after warm-up; the two heatmaps are compared before anything is timed.
"""
import argparse
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
from snnflow import contrast  # noqa: E402

B, N, H, W, R, MAXDISP = 1, 40000, 180, 240, 50, 64
TRUE_FLOW = (20.0, -12.0)


def window(dev):
    """400 points of random polarity translating with TRUE_FLOW px per window plus 25 % uniform noise
    events; events that leave the frame are masked out (pol = 0)."""
    gen = torch.Generator().manual_seed(3)
    ts = torch.sort(torch.rand(B, N, generator=gen), dim=1).values
    ts = (ts - ts[:, :1]) / (ts[:, -1:] - ts[:, :1])
    npts = 400
    y0, x0 = torch.rand(B, npts, generator=gen) * H, torch.rand(B, npts, generator=gen) * W
    pp = torch.randint(0, 2, (B, npts), generator=gen).float() * 2 - 1
    which = torch.randint(0, npts, (B, N), generator=gen)
    ys = torch.floor(torch.gather(y0, 1, which) + TRUE_FLOW[1] * ts)
    xs = torch.floor(torch.gather(x0, 1, which) + TRUE_FLOW[0] * ts)
    ps = torch.gather(pp, 1, which)
    noise = torch.rand(B, N, generator=gen) < 0.25
    ys = torch.where(noise, torch.randint(0, H, (B, N), generator=gen).float(), ys)
    xs = torch.where(noise, torch.randint(0, W, (B, N), generator=gen).float(), xs)
    inside = ((ys >= 0) & (ys < H) & (xs >= 0) & (xs < W)).float()
    ys, xs = ys * inside, xs * inside
    ev = torch.stack([ts, ys, xs, ps], dim=2)
    pol = torch.stack([(ps > 0).float() * inside, (ps < 0).float() * inside], dim=2)
    mask = torch.zeros(B, 1, H, W)
    mask[0, 0, ys[0].long(), xs[0].long()] = 1
    return ev.to(dev), pol.to(dev), mask.to(dev)


def loop_heatmap(loss_fn, ev, pol, mask, cand, dev):
    """demo_iwe.py:70-85 on snnflow.EventWarping."""
    heat = np.zeros(len(cand), dtype=np.float32)
    flowmap = torch.ones(B, 2, H, W, device=dev)
    for k, (u, v) in enumerate(cand):
        flow = flowmap.clone()
        flow[:, 0, :, :] *= float(u)
        flow[:, 1, :, :] *= float(v)
        loss_fn.event_flow_association([flow], ev, pol, mask)
        heat[k] = loss_fn().item()
        loss_fn.reset()
    return heat.reshape(R, R)


def timed(fn, calls, warmup, dev):
    times = []
    for i in range(warmup + calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize(dev)
        if i >= warmup:
            times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--loop-calls", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = {"loader": {"resolution": [H, W]}, "loss": {"flow_regul_weight": 0.001}, "model": {"mask_output": True}}
    ev, pol, mask = window(dev)
    _, _, cand = contrast.grid_candidates(MAXDISP, MAXDISP, R)
    loss_fn = snnflow.EventWarping(cfg, dev, flow_scaling=1)

    heat = snnflow.flow_heatmap(ev, pol, mask, cfg, MAXDISP, MAXDISP, R).cpu().numpy()
    want = loop_heatmap(loss_fn, ev, pol, mask, cand, dev)
    dev_rel = float(np.abs(heat / want - 1).max())
    j, i = np.unravel_index(np.argmin(heat), heat.shape)
    print(f"heatmaps agree to {dev_rel:.2e} (relative, max over {R * R} candidates); argmin "
          f"({cand[j * R + i][0]:.2f}, {cand[j * R + i][1]:.2f}) px, true flow {TRUE_FLOW}")
    assert dev_rel < 2e-5, dev_rel

    ms, lo, hi = timed(lambda: snnflow.flow_heatmap(ev, pol, mask, cfg, MAXDISP, MAXDISP, R), args.calls, 3, dev)
    print(f"landscape: {ms:.3f} ms per heatmap (median of {args.calls}, min {lo:.3f}, max {hi:.3f})")
    ms_l, lo_l, hi_l = timed(lambda: loop_heatmap(loss_fn, ev, pol, mask, cand, dev), args.loop_calls, 1, dev)
    print(f"loop:      {ms_l:.1f} ms per heatmap (median of {args.loop_calls}, min {lo_l:.1f}, max {hi_l:.1f})")
    print(f"ratio:     {ms_l / ms:.1f} x")
    snnflow.check_device_errors()


if __name__ == "__main__":
    main()
