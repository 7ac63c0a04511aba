"""Writes tests/golden/profile_case.npz: the reference's VoltageProfiler driven over recorded states.

    python tests/golden/make_golden_profile.py REFERENCE_ROOT

Imports the reference's ``analyze_voltage_dynamics`` (with empty stand-ins for the modules its script part
imports and the class never touches), attaches the real ``VoltageProfiler`` to a two-cell module whose
cells replay recorded states through forward hooks' ``(spk, state)`` outputs, and stores the replayed
states with the profiler's ``voltage_stats`` and ``compute_statistics()`` per layer:

    {case}_{layer}_states          float32 [T, 2, B, C, H, W]   (membrane, spikes)
    {case}_{layer}_vs_{key}        voltage_stats[layer][key]
    {case}_{layer}_cs_{key}        compute_statistics()[layer][key]   (numeric keys)

Cases (2 layers, T = 5 steps, B = 2, C = 4, 6 x 10):
    dyadic   membranes are multiples of 2^-4 in [-4, 4] and 0 where the neuron spiked; the reference's
             float32 sums are exact.  Channel 3 never spikes.
    generic  normal(0, 1) membranes, |mean| < 0.1 std per layer.
"""
import contextlib
import io
import math
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

T, B, C, H, W = 5, 2, 4, 6, 10
RATES = (0.03, 0.15, 0.4, 0.0)   # spike probability per channel; the last channel is dead


def import_reference(root):
    for name, attrs in (("configs", ()), ("configs.parser", ("YAMLParser",)), ("dataloader", ()),
                        ("dataloader.h5", ("H5Loader",)), ("models", ()),
                        ("models.model", ("LIFFireNet", "LIFFireNet_short", "LIFFireFlowNet", "LIFFireFlowNet_short")),
                        ("utils", ()), ("utils.utils", ("load_model",))):
        mod = types.ModuleType(name)
        for a in attrs:
            setattr(mod, a, None)
        sys.modules[name] = mod
    sys.path.insert(0, root)
    import analyze_voltage_dynamics
    return analyze_voltage_dynamics


class SNNtorch_ConvLIF(nn.Module):
    """Replays recorded states: forward returns the reference cell's (spk, state)."""

    def __init__(self, states):
        super().__init__()
        self.seq, self.t = torch.from_numpy(states), 0

    def forward(self, x):
        st = self.seq[self.t]
        self.t += 1
        return st[1], st


class SNNtorch_ConvLIFRecurrent(SNNtorch_ConvLIF):
    pass


class Replay(nn.Module):
    def __init__(self, head, g1):
        super().__init__()
        self.head, self.G1 = SNNtorch_ConvLIF(head), SNNtorch_ConvLIFRecurrent(g1)

    def forward(self, x):
        self.head(x)
        self.G1(x)


def make_states(rng, dyadic):
    spk = np.zeros((T, B, C, H, W), dtype=np.float32)
    for c, r in enumerate(RATES):
        spk[:, :, c] = rng.random((T, B, H, W)) < r
    if dyadic:
        mem = (rng.integers(-64, 65, size=spk.shape) / 16.0).astype(np.float32)
        mem[spk != 0] = 0.0
    else:
        mem = rng.normal(0.0, 1.0, size=spk.shape).astype(np.float32)
    return np.ascontiguousarray(np.stack([mem, spk], axis=1))


def main(root):
    avd = import_reference(root)
    rng = np.random.default_rng(20240611)
    out = {}
    for case in ("dyadic", "generic"):
        states = {"head": make_states(rng, case == "dyadic"), "G1": make_states(rng, case == "dyadic")}
        model = Replay(states["head"], states["G1"])
        prof = avd.VoltageProfiler(model, torch.device("cpu"))
        assert len(prof.hooks) == 2 and sorted(prof.layer_names.values()) == ["G1", "head"]
        with torch.no_grad():
            for _ in range(T):
                model(None)
        with contextlib.redirect_stdout(io.StringIO()):
            stats = prof.compute_statistics()
        prof.remove_hooks()
        assert list(stats) == ["G1", "head"]
        for layer, st in states.items():
            pre = f"{case}_{layer}"
            out[f"{pre}_states"] = st
            vs, cs = prof.voltage_stats[layer], stats[layer]
            for k, v in vs.items():
                out[f"{pre}_vs_{k}"] = np.asarray(v, dtype=np.float64)
            for k, v in cs.items():
                if v is None or isinstance(v, str):
                    continue
                out[f"{pre}_cs_{k}"] = np.asarray(v, dtype=np.float64)
            # the branches the case exists for
            rates, ch = cs["per_neuron_spike_rates"], cs["channel_spike_rates"]
            assert cs["channels_dead"] >= 1 and ch[3] == 0 and (ch[:3] > 0).all()
            for thr in (0.01, 0.05, 0.20):
                assert (rates < thr).any() and (rates >= thr).any(), (case, layer, thr)
                assert (ch < thr).any() and (ch >= thr).any(), (case, layer, thr)
            assert 0 < cs["neurons_dead"] <= cs["neurons_low"] < cs["neurons_moderate"] < cs["total_neurons"]
            mem = st[:, 0].astype(np.float64)
            if case == "dyadic":
                assert float(vs["voltage_sum"]) == math.fsum(mem.ravel())
                assert float(vs["voltage_sum_sq"]) == math.fsum((mem * mem).ravel())
                assert (mem[st[:, 1] != 0] == 0).all() and np.abs(mem).max() <= 4 and (mem * 16 == np.round(mem * 16)).all()
            else:
                assert abs(cs["voltage_mean"]) < 0.1 * cs["voltage_std"], (cs["voltage_mean"], cs["voltage_std"])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profile_case.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1])
