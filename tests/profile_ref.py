"""Numpy restatement of the membrane-profiling accumulators (csrc/profile.hip, include/snnflow.h
snnflow_vstats_args): what a list of states [2, B, C, H, W] (membrane, spikes) folds into, the histogram
key and the bin edges.  Written from the header's definitions, independent of snnflow/profile.py."""
import math

import numpy as np

BINS = 65536


def key16(x):
    """bin of float32 values: b = bits(x + 0.0f); key = (b >> 31) ? ~b : (b | 0x80000000); bin = key >> 16"""
    x = (np.asarray(x, dtype=np.float32) + np.float32(0.0)).astype(np.float32)
    b = x.view(np.uint32).astype(np.uint64)
    key = np.where(b >> 31 != 0, (~b) & 0xFFFFFFFF, b | 0x80000000)
    return (key >> 16).astype(np.int64)


def bin_hi(j):
    """largest float32 whose bin is j (a finite-value bin)"""
    j = int(j)
    if j >= 0x8000:
        bits = ((j & 0x7FFF) << 16) | 0xFFFF
    else:
        bits = (0xFFFF - j) << 16
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


def bin_lo(j):
    """smallest float32 whose bin is j"""
    j = int(j)
    if j >= 0x8000:
        bits = (j & 0x7FFF) << 16
    else:
        bits = ((0xFFFF - j) << 16) | 0xFFFF
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


def accumulate(states):
    """Accumulators of one slot from its states (numpy [2, B, C, H, W] each), as the header defines them."""
    C, H, W = states[0].shape[2:]
    acc = {"count": 0, "nonfinite": 0, "samples": 0,
           "chan_sum": [[] for _ in range(C)], "chan_sumsq": [[] for _ in range(C)],
           "chan_min": np.full(C, np.inf, dtype=np.float32), "chan_max": np.full(C, -np.inf, dtype=np.float32),
           "chan_spikes": np.zeros(C, dtype=np.uint64), "neuron_spikes": np.zeros((C, H * W), dtype=np.uint32),
           "hist": np.zeros(BINS, dtype=np.uint64)}
    for st in states:
        mem = (st[0].astype(np.float32) + np.float32(0.0)).astype(np.float32)
        spk = st[1]
        B = mem.shape[0]
        fin = np.isfinite(mem)
        acc["count"] += int(fin.sum())
        acc["nonfinite"] += int((~fin).sum())
        acc["samples"] += B
        for c in range(C):
            v = mem[:, c][fin[:, c]].astype(np.float64)
            acc["chan_sum"][c].append(v)
            acc["chan_sumsq"][c].append(v * v)
            if v.size:
                acc["chan_min"][c] = min(acc["chan_min"][c], np.float32(v.min()))
                acc["chan_max"][c] = max(acc["chan_max"][c], np.float32(v.max()))
        nz = spk != 0
        acc["chan_spikes"] += nz.sum(axis=(0, 2, 3)).astype(np.uint64)
        acc["neuron_spikes"] += nz.sum(axis=0).reshape(C, H * W).astype(np.uint32)
        acc["hist"] += np.bincount(key16(mem[fin]), minlength=BINS).astype(np.uint64)
    # exactly rounded fp64 sums (math.fsum) and the sum of absolute addends (for error bounds)
    acc["chan_abs"] = np.array([math.fsum(np.abs(np.concatenate(v))) for v in acc["chan_sum"]])
    acc["chan_abs_sq"] = np.array([math.fsum(np.concatenate(v)) for v in acc["chan_sumsq"]])
    acc["chan_n"] = np.array([sum(x.size for x in v) for v in acc["chan_sum"]])
    acc["chan_sum"] = np.array([math.fsum(np.concatenate(v)) for v in acc["chan_sum"]])
    acc["chan_sumsq"] = acc["chan_abs_sq"].copy()
    return acc


def streaming(acc):
    """The reference's streaming dict (analyze_voltage_dynamics.py:50-65, 107-135) from the accumulators."""
    C, HW = acc["neuron_spikes"].shape
    return {"count": acc["count"], "voltage_sum": float(acc["chan_sum"].sum()),
            "voltage_sum_sq": float(acc["chan_sumsq"].sum()), "voltage_min": float(acc["chan_min"].min()),
            "voltage_max": float(acc["chan_max"].max()), "spike_sum": float(acc["chan_spikes"].sum()),
            "per_neuron_spike_sums": acc["neuron_spikes"].astype(np.float64),
            "per_neuron_counts": np.full((C, HW), float(acc["samples"])),
            "channel_spike_sums": acc["chan_spikes"].astype(np.float64), "channel_counts": acc["samples"] * HW,
            "num_channels": C}


def statistics(acc):
    """The fields of compute_statistics (analyze_voltage_dynamics.py:145-241) the tests compare, in float64."""
    d = streaming(acc)
    n = d["count"]
    mean = d["voltage_sum"] / n
    std = math.sqrt(max(d["voltage_sum_sq"] / n - mean ** 2, 0.0))
    ch = d["channel_spike_sums"] / d["channel_counts"]
    nr = d["per_neuron_spike_sums"] / np.maximum(d["per_neuron_counts"], 1)
    out = {"voltage_min": d["voltage_min"], "voltage_max": d["voltage_max"], "voltage_mean": mean, "voltage_std": std,
           "spike_rate_global": d["spike_sum"] / n, "channel_spike_rates": ch, "per_neuron_spike_rates": nr,
           "num_channels": d["num_channels"], "spatial_size": nr.shape[1], "total_neurons": nr.size}
    for key, r in (("channels", ch), ("neurons", nr)):
        out[f"{key}_dead"] = int((r == 0).sum())
        out[f"{key}_very_low"] = int((r < 0.01).sum())
        out[f"{key}_low"] = int((r < 0.05).sum())
        out[f"{key}_moderate"] = int((r < 0.20).sum())
    return out


STREAM_EXACT = ("count", "voltage_min", "voltage_max", "spike_sum", "per_neuron_spike_sums", "per_neuron_counts",
                "channel_spike_sums", "channel_counts", "num_channels")
STATS_EXACT = ("voltage_min", "voltage_max", "channel_spike_rates", "per_neuron_spike_rates", "num_channels",
               "spatial_size", "total_neurons", "channels_dead", "channels_very_low", "channels_low",
               "channels_moderate", "neurons_dead", "neurons_very_low", "neurons_low", "neurons_moderate")
STATS_CLOSE = ("voltage_mean", "voltage_std", "spike_rate_global")   # 2^-21 relative on `generic`
CASES = ("dyadic", "generic")
LAYERS = ("G1", "head")   # the fixture's two layers, in the reference's sorted order


def golden_states(g, case, layer):
    """the fixture's replayed states of a layer: [T, 2, B, C, H, W]"""
    return g[f"{case}_{layer}_states"]


def check_against_golden(g, case, layer, stream, stats, inexact=True):
    """`stream` / `stats` (a profiler's voltage_stats[layer] / compute_statistics()[layer], or the restatement's)
    against the reference's recorded output.  Exact: integer fields, extrema, rates, dead / low counts and, on
    `dyadic`, the sums.  With `inexact`: on `generic` the sums within N * 2^-23 * sum|x| (N addends; twice the
    first-order worst case of the reference's fp32 summation in any order), and voltage_mean / voltage_std /
    spike_rate_global within 2^-21 relative (at most 4 fp32 roundings in the reference's last operations,
    times 2).  Prints each inexact figure before asserting it."""
    pre = f"{case}_{layer}"
    st = golden_states(g, case, layer)
    for k in STREAM_EXACT:
        np.testing.assert_array_equal(np.asarray(stream[k], dtype=np.float64), g[f"{pre}_vs_{k}"].astype(np.float64),
                                      err_msg=f"{pre} voltage_stats[{k}]")
    for k in STATS_EXACT:
        np.testing.assert_array_equal(np.asarray(stats[k], dtype=np.float64), g[f"{pre}_cs_{k}"].astype(np.float64),
                                      err_msg=f"{pre} compute_statistics[{k}]")
    mem = st[:, 0].astype(np.float64)
    N = mem.size
    for k, addends in (("voltage_sum", mem), ("voltage_sum_sq", mem * mem)):
        ref, got = float(g[f"{pre}_vs_{k}"]), float(stream[k])
        if case == "dyadic":
            assert got == ref, (pre, k, got, ref)
        else:
            bound = N * 2.0 ** -23 * math.fsum(np.abs(addends).ravel())
            print(f"{pre} {k}: got {got!r} reference {ref!r} |diff| {abs(got - ref):.3e} bound {bound:.3e}")
            assert not inexact or abs(got - ref) <= bound, (pre, k, got, ref, bound)
    for k in STATS_CLOSE:
        ref, got = float(g[f"{pre}_cs_{k}"]), float(stats[k])
        rel = abs(got - ref) / abs(ref) if ref != 0 else abs(got)
        print(f"{pre} {k}: got {got!r} reference {ref!r} relative {rel:.3e} bound {2.0 ** -21:.3e}")
        assert not inexact or rel <= 2.0 ** -21, (pre, k, got, ref, rel)
