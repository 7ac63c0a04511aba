"""Cost of membrane profiling (ms, median of 50 calls after warm-up, HIP events around each call, the
variants interleaved round by round in one process on the GPU) for one forward_sequence of T = 10 windows
at 128x128 through a LIFFireNet:

  eval   B = 1, C = 8      eval   B = 1, C = 32      train  B = 8, C = 8

    python tools/profile_time.py

Per shape: the forward alone; with a VoltageProfiler attached, histogram on (counts by global integer atomics,
and through the LDS sub-table: snnflow_vstats_hist_mode) and off; the hook route (forward hooks on the cells
that copy membrane and spikes to the host, which also drops the model to one cell call per layer); and the
update kernels alone over the window's T x L states, with their read rate (2*B*C*H*W*4 bytes per state).
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
from snnflow import _lib  # noqa: E402
from snnflow.synthetic import make_window  # noqa: E402

T, H, W = 10, 128, 128
DEFAULT_MODE = _lib.lib.snnflow_vstats_hist_mode(-1)


def model_kwargs(C):
    return {"name": "LIFFireNet", "encoding": "cnt", "round_encoding": False, "norm_input": False, "num_bins": 2,
            "base_num_channels": C, "kernel_size": 3, "activations": ["arctanspike", "arctanspike"],
            "mask_output": True, "quantization": {"enabled": False, "PTQ": False, "Conv_only": False},
            "tebn": {"enabled": False}, "mpbn": {"enabled": False},
            "spiking_neuron": {"leak": [0.0, 1.0], "thresh": [0.0, 0.8], "learn_leak": True, "learn_thresh": True,
                               "hard_reset": True}}


class HostHooks:
    """The hook route: a forward hook per cell that brings the state's membrane and spikes to the host and
    updates streaming sums there."""

    def __init__(self, model):
        self.sums = {}
        self.handles = [getattr(model, n).register_forward_hook(self.hook(n)) for n, _ in model.layer_spec]

    def hook(self, name):
        def fn(module, inputs, output):
            state = output[1]
            mem, spk = state[0].detach().cpu().numpy(), state[1].detach().cpu().numpy()
            s = self.sums.setdefault(name, [0, 0.0, 0.0, np.inf, -np.inf, 0.0])
            s[0] += mem.size
            s[1] += mem.sum()
            s[2] += (mem ** 2).sum()
            s[3], s[4] = min(s[3], mem.min()), max(s[4], mem.max())
            s[5] += spk.sum()
        return fn

    def remove(self):
        for h in self.handles:
            h.remove()
        self.handles = []


def measure(label, C, B, train, calls=50, warmup=5):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = snnflow.LIFFireNet(model_kwargs(C)).to(dev)
    model = model.train() if train else model.eval()
    gen = torch.Generator(device=dev).manual_seed(1)
    wins = [make_window(B, 2000 * B, H, W, gen, dev) for _ in range(T)]
    vox, cnt = [w["event_voxel"] for w in wins], [w["event_cnt"] for w in wins]
    profs = {"hist": snnflow.VoltageProfiler(None, dev, histogram=True),
             "nohist": snnflow.VoltageProfiler(None, dev, histogram=False)}
    names = [n for n, _ in model.layer_spec]

    def forward():
        model.reset_states()
        with torch.set_grad_enabled(train):
            model.forward_sequence(vox, cnt)

    def with_profiler(key, mode):
        def run():
            _lib.lib.snnflow_vstats_hist_mode(mode)
            model._profiler = profs[key]
            try:
                forward()
            finally:
                model._profiler = None
                _lib.lib.snnflow_vstats_hist_mode(DEFAULT_MODE)
        return run

    def hooks():
        h = HostHooks(model)
        try:
            forward()
        finally:
            h.remove()

    # the window's states, kept once, for the kernels alone
    model.engine.capture_states = True
    forward()
    states = [st for sts in model.engine.seq_states for st in sts]
    model.engine.capture_states = False
    model.engine.seq_states = None

    def kernels(key, mode):
        def run():
            _lib.lib.snnflow_vstats_hist_mode(mode)
            profs[key].update_many(names * T, states)
            _lib.lib.snnflow_vstats_hist_mode(DEFAULT_MODE)
        return run

    variants = {"forward alone": forward,
                "forward + profiler, histogram by global atomics": with_profiler("hist", 0),
                "forward + profiler, histogram through LDS": with_profiler("hist", 1),
                "forward + profiler, histogram off": with_profiler("nohist", 0),
                "forward + host-copy hooks (cell-wise)": hooks,
                "update kernels alone, global atomics": kernels("hist", 0),
                "update kernels alone, LDS": kernels("hist", 1),
                "update kernels alone, histogram off": kernels("nohist", 0)}
    times = {k: [] for k in variants}
    for i in range(warmup + calls):
        for k, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize(dev)
            if i >= warmup:
                times[k].append(a.elapsed_time(b))
    nbytes = len(states) * 2 * B * C * H * W * 4
    print(f"{label}: T = {T}, L = {len(names)}, {len(states)} states, {nbytes / 1e6:.1f} MB per window")
    for k, v in times.items():
        ms = statistics.median(v)
        rate = f", {nbytes / ms / 1e6:.0f} GB/s read" if k.startswith("update") else ""
        print(f"  {k}: {ms:.4f} ms (median of {calls}, min {min(v):.4f}, max {max(v):.4f}){rate}")


def main():
    measure("eval  B=1 C=8  128x128", 8, 1, False)
    measure("eval  B=1 C=32 128x128", 32, 1, False)
    measure("train B=8 C=8  128x128", 8, 8, True)


if __name__ == "__main__":
    main()
