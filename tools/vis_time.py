"""Time of rendering one stored frame of a visual evaluation (ms, median of 30 frames after
warm-up, one process on the GPU), B = 1, at 128x128 and 260x346: five flow_to_image, three
events_to_image and one error_to_image, the calls the reference's Visualization.store makes
per frame (utils/visualization.py:287-459).

    python tools/vis_time.py

  device  snnflow.vis on device tensors, finished frames copied to the host (HIP event pair on
          the launch stream around the nine calls and their nine copies, so the host's launch
          overhead counts whenever the host is the slower side)
  host    the numpy path (tests/vis_ref.py, the reference's arithmetic) on the same machine,
          including the device->host copies of the raw flow / count / error tensors it needs
          (wall clock)
"""
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "snn_event-based_optical_flow_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import vis_ref  # noqa: E402
from snnflow import vis  # noqa: E402


def frame_inputs(H, W, gen, dev):
    flows = [torch.randn(1, 2, H, W, generator=gen, device=dev) * s for s in (0.5, 1.0, 2.0, 4.0, 8.0)]
    flows[0][:, :, torch.rand(H, W, generator=gen, device=dev) < 0.3] = 0.0   # masked flow: true zeros
    cnts = [torch.poisson(torch.full((1, 2, H, W), lam, device=dev), generator=gen) for lam in (0.3, 0.7, 1.5)]
    err = torch.rand(1, H, W, generator=gen, device=dev) * 3.14
    return flows, cnts, err


def device_frame(flows, cnts, err):
    out = [vis.flow_to_image(f) for f in flows] + [vis.events_to_image(c) for c in cnts] + [vis.error_to_image(err)]
    return [o.cpu() for o in out]


def host_frame(flows, cnts, err):
    out = []
    for f in flows:
        f = f.cpu().numpy()
        out.append(vis_ref.flow_to_image(f[0, 0], f[0, 1]))
    for c in cnts:
        out.append(vis_ref.events_to_image(c.cpu().numpy()[0].transpose(1, 2, 0)))
    out.append(vis_ref.error_to_image(err.cpu().numpy()))
    return out


def measure(H, W, frames=30, warmup=5):
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(H)
    flows, cnts, err = frame_inputs(H, W, gen, dev)
    t_dev, t_host = [], []
    for i in range(warmup + frames):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        device_frame(flows, cnts, err)
        b.record()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        host_frame(flows, cnts, err)
        t1 = time.perf_counter()
        if i >= warmup:
            t_dev.append(a.elapsed_time(b))
            t_host.append(1e3 * (t1 - t0))
    d, h = statistics.median(t_dev), statistics.median(t_host)
    print(f"{H}x{W}: device {d:.3f} ms per frame (min {min(t_dev):.3f}, max {max(t_dev):.3f}), "
          f"host {h:.3f} ms per frame (min {min(t_host):.3f}, max {max(t_host):.3f}), host / device = {h / d:.1f}")
    # where the device time goes: each renderer alone, kernels only (no copies)
    for name, fn, arg in (("flow_to_image", vis.flow_to_image, flows[2]), ("events_to_image", vis.events_to_image, cnts[1]),
                          ("error_to_image", vis.error_to_image, err)):
        ts = []
        for i in range(warmup + frames):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(arg)
            b.record()
            torch.cuda.synchronize(dev)
            if i >= warmup:
                ts.append(a.elapsed_time(b))
        print(f"    {name}: {statistics.median(ts):.4f} ms per call")
    return d, h


def main():
    measure(128, 128)
    measure(260, 346)


if __name__ == "__main__":
    main()
