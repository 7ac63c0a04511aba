"""Time per window of snnflow.SequenceLoader (ms, median over the timed windows after warm-up, one
process on the GPU) at the two shapes of the shipped configs, with prefetch on and off, next to
the only way to get the same batches without it: the numpy restatement of the reference's window
logic on host arrays (tests/sequence_ref.py RefSequenceReader), a host-to-device copy of the
padded window and BatchPreparer.prepare().

  train  B = 8, events mode, window 1000, 128x128 crop of 256x256, augmentation on
  eval   B = 1, gtflow_dt1, 256x256 -> 128x128, about 15 000 events per window, hot filter on,
         full-resolution gtflow

    python tools/sequence_time.py [--windows 100]

A window's time is a host clock from the request for the batch to the end of a device
synchronise after it (the consumer's view: with prefetch the selection of the next window is
already in flight on the side stream when the clock stops).  Synthetic recordings from a seed:
uniform pixels and timestamps.
"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "snn_event-based_optical_flow_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import snnflow  # noqa: E402
from sequence_ref import RefSequenceReader  # noqa: E402

MECH = ["Horizontal", "Vertical", "Polarity"]
H0 = W0 = 256


def recording(rng, n, nflow=0):
    ts = np.sort(10.0 + rng.random(n))
    s = dict(xs=rng.integers(0, W0, n).astype(np.int16), ys=rng.integers(0, H0, n).astype(np.int16), ts=ts,
             ps=rng.integers(0, 2, n).astype(np.uint8), t0=10.0, duration=1.0, flow_ts=None, flow_maps=None)
    if nflow:
        s["flow_ts"] = 10.0 + (np.arange(nflow) + 0.5) / nflow
        s["flow_maps"] = rng.standard_normal((nflow, 2, H0, W0)).astype(np.float32)
    return s


def upload(seqs, dev):
    return [snnflow.EventSequence(s["xs"], s["ys"], s["ts"], s["ps"], s["t0"], s["duration"], s["flow_ts"],
                                  s["flow_maps"], device=dev) for s in seqs]


def timed(step, dev, windows, warmup):
    times = []
    for i in range(warmup + windows):
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        step()
        torch.cuda.synchronize(dev)
        if i >= warmup:
            times.append(1e3 * (time.perf_counter() - t))
    return statistics.median(times), min(times), max(times)


def host_path(cfg, seqs, num_bins, max_events, dev):
    """RefSequenceReader on the host arrays -> H2D -> prepare, resets as SequenceLoader makes them."""
    rd = RefSequenceReader(cfg, seqs, max_events)
    prep = snnflow.BatchPreparer(cfg, num_bins, device=dev)

    def step():
        w = rd.next()
        for slot, n in enumerate(w["restarts"]):
            for _ in range(int(n)):
                prep.reset_sequence(slot)
        t = {k: torch.from_numpy(w[k]).to(dev) for k in ("xs", "ys", "ts", "ps", "counts")}
        gt = torch.from_numpy(w["gtflow"]).to(dev) if "gtflow" in w else None
        return prep.prepare(t["xs"], t["ys"], t["ts"], t["ps"], t["counts"], gt)

    return step


def measure(name, cfg, seqs, num_bins, max_events, windows, warmup=10):
    dev = torch.device("cuda:0")
    out = {}
    for label, prefetch in (("prefetch", True), ("in order", False)):
        np.random.seed(0)
        ld = snnflow.SequenceLoader(cfg, upload(seqs, dev), num_bins, prefetch=prefetch, device=dev, max_events=max_events)
        out[label] = timed(lambda: next(ld), dev, windows, warmup)
        ld.reader.check()
    np.random.seed(0)
    out["host reader + H2D + prepare"] = timed(host_path(cfg, seqs, num_bins, max_events, dev), dev, windows, warmup)
    for label, (med, lo, hi) in out.items():
        print(f"{name}: {label}: {med:.4f} ms per window (median of {windows}, min {lo:.4f}, max {hi:.4f})")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=100)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    train = {"data": {"mode": "events", "window": 1000},
             "loader": {"resolution": [128, 128], "std_resolution": [H0, W0], "batch_size": 8, "augment": MECH,
                        "augment_prob": [0.5, 0.5, 0.5]},
             "hot_filter": {"enabled": False}}
    evalc = {"data": {"mode": "gtflow_dt1", "window": 1},
             "loader": {"resolution": [128, 128], "std_resolution": [H0, W0], "batch_size": 1, "augment": [],
                        "augment_prob": [], "keep_gt_full_res": True},
             "hot_filter": {"enabled": True, "max_px": 100, "min_obvs": 5, "max_rate": 0.8}}
    n_train = 4200 * (a.windows + 20)   # a quarter of the events fall inside the crop
    measure("train B=8 window=1000 128x128 of 256x256", train, [recording(rng, n_train) for _ in range(8)], 2, None,
            a.windows)
    nflow = a.windows + 20
    measure("eval  B=1 gtflow_dt1 256x256->128x128 ~15000 events", evalc,
            [recording(rng, 15000 * nflow, nflow) for _ in range(2)], 2, 20480, a.windows)


if __name__ == "__main__":
    main()
