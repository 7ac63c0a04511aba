"""On-device membrane profiling: the reference's two membrane-dynamics tools on ``snnflow_vstats_update``.

``VoltageProfiler`` keeps the surface of ``analyze_voltage_dynamics.py:33-241`` (``hooks``, ``layer_names``,
``voltage_stats``, ``remove_hooks()``, ``compute_statistics()``) and ``membrane_ranges()`` returns what
``eval_flow_quant.py:186-463`` ``profile_membrane_ranges`` returns.  Nothing is hooked and nothing is copied
to the host while the model runs: the profiler attaches itself to the model, which hands it every step's
new cell states (already in HBM, in the engine's layout), and one streaming pass per hand-over folds them
into exact integer counts, exact extrema, fp64 sums and a 65536-bin histogram of every membrane value
(csrc/profile.hip).  The fused and wavefront launches keep running; statistics cross to the host once, when
they are asked for.
"""
import collections.abc
import math

import numpy as np
import torch

from . import _lib
from ._lib import lib
from .engine import nhwc_state_strides

BINS = _lib.VSTATS_BINS

# eval_flow_quant.py:412-434: the percentile pair recommended per layer (others: P1-P99)
LAYER_STRATEGIES = {"head": ("p2_5", "p99"), "G1": ("p1", "p99"), "R1a": ("p1", "p99"), "R1b": ("p2_5", "p99"),
                    "G2": ("p1", "p99"), "R2a": ("p1", "p99"), "R2b": ("p6", "p99")}
_LOW_KEYS = (("p1", 1), ("p2_5", 2.5), ("p5", 5), ("p6", 6), ("p25", 25))
_HIGH_KEYS = (("p75", 75), ("p95", 95), ("p99", 99), ("p999", 99.9))


def key16(x):
    """Histogram bin of float32 values: with b the bits of ``x + 0.0`` (-0.0 counts as +0.0),
    ``key = ~b if b >> 31 else b | 0x80000000`` and the bin is ``key >> 16``.  Order-preserving; a bin is
    the set of floats that share a bf16 truncation."""
    x = np.asarray(x, dtype=np.float32) + np.float32(0.0)
    b = x.view(np.uint32)
    key = np.where(b >> np.uint32(31), ~b, b | np.uint32(0x80000000))
    return (key >> np.uint32(16)).astype(np.int64)


def bin_edges(j):
    """(smallest, largest) float32 of histogram bin(s) j."""
    j = np.asarray(j, dtype=np.int64)
    pos = j >= 0x8000
    h = np.where(pos, j & 0x7FFF, 0xFFFF - j).astype(np.uint32) << np.uint32(16)
    full = h | np.uint32(0xFFFF)
    lo = np.where(pos, h, full).astype(np.uint32).view(np.float32)
    hi = np.where(pos, full, h).astype(np.uint32).view(np.float32)
    return lo, hi


def quantile_bracket_from_hist(hist, q):
    """(lo, hi) float32 bounds of ``np.percentile(values, q)`` from the values' histogram: with n values,
    ``k = floor(q/100 * (n-1))`` and ``k1 = min(k+1, n-1)``, lo is the smallest float of the bin that holds
    the k-th smallest value and hi the largest float of the bin that holds the k1-th, so
    ``lo <= x_(k) <= percentile <= x_(k1) <= hi``."""
    hist = np.asarray(hist).astype(np.int64).ravel()
    n = int(hist.sum())
    if n == 0:
        return np.float32(np.nan), np.float32(np.nan)
    k = int(math.floor((q / 100.0) * (n - 1)))
    k = min(max(k, 0), n - 1)
    k1 = min(k + 1, n - 1)
    cum = np.cumsum(hist)
    bk, bk1 = (int(np.searchsorted(cum, r, side="right")) for r in (k, k1))
    return bin_edges(bk)[0][()], bin_edges(bk1)[1][()]


def _same_strides(t, strides):
    return all(n == 1 or a == b for n, a, b in zip(t.shape, t.stride(), strides))


class _Group:
    """Accumulators of the layers that share (C, H, W): [slots] x the shapes of snnflow_vstats_args."""

    def __init__(self, C, H, W, device, histogram, cap=8):
        self.C, self.H, self.W, self.device, self.histogram = C, H, W, device, histogram
        self.names = []
        self.cap = 0
        self.t = {}
        self.scratch = None
        self._grow(cap)

    def _fresh(self, cap):
        C, HW, dev = self.C, self.H * self.W, self.device
        t = {"count": torch.zeros(cap, dtype=torch.int64, device=dev),
             "nonfinite": torch.zeros(cap, dtype=torch.int64, device=dev),
             "chan_sum": torch.zeros(cap, C, dtype=torch.float64, device=dev),
             "chan_sumsq": torch.zeros(cap, C, dtype=torch.float64, device=dev),
             "chan_min": torch.full((cap, C), float("inf"), dtype=torch.float32, device=dev),
             "chan_max": torch.full((cap, C), float("-inf"), dtype=torch.float32, device=dev),
             "chan_spikes": torch.zeros(cap, C, dtype=torch.int64, device=dev),
             "neuron_spikes": torch.zeros(cap, HW, C, dtype=torch.int32, device=dev)}
        if self.histogram:
            t["hist"] = torch.zeros(cap, BINS, dtype=torch.int64, device=dev)
        return t

    def _grow(self, cap):
        new = self._fresh(cap)
        for k, v in self.t.items():
            new[k][:self.cap].copy_(v)
        self.t, self.cap = new, cap

    def slot(self, name):
        if name not in self.names:
            if len(self.names) == self.cap:
                self._grow(2 * self.cap)
            self.names.append(name)
        return self.names.index(name)

    def reset(self):
        self.t = self._fresh(self.cap)


class _StatsView(collections.abc.Mapping):
    """``profiler.voltage_stats``: layer name -> the reference's streaming dict, built on access."""

    def __init__(self, prof):
        self._p = prof

    def __getitem__(self, name):
        return self._p._streaming(name)

    def __iter__(self):
        return iter(self._p._where)

    def __len__(self):
        return len(self._p._where)


class VoltageProfiler:
    """Drop-in for the reference's ``VoltageProfiler(model, device)``.

    Registers no hooks (``hooks`` stays ``[]``): while attached, the model hands every step's new states
    to ``update_many`` (``_FireNetBase._step`` / ``forward_sequence``), so ``model._cellwise()`` stays False.
    ``remove_hooks()`` detaches it.  ``update`` / ``update_many`` also take any ``[2, B, C, H, W]`` device
    tensor (stacked membrane and spikes of a cell).  With ``histogram=False`` the 65536-bin table is not
    kept and the quantile fields stay ``nan``."""

    def __init__(self, model=None, device=None, histogram=True):
        self.model = model
        self.device = device
        self.histogram = bool(histogram)
        self.hooks = []
        self.spike_stats = collections.defaultdict(dict)
        self.layer_names = {}
        self._groups = {}
        self._where = {}      # layer name -> (group, slot)
        self._samples = {}    # layer name -> states' batch entries seen (the reference's per_neuron_counts)
        if model is not None:
            for name, module in model.named_modules():
                if "ConvLIF" in module.__class__.__name__:
                    self.layer_names[id(module)] = name
            if hasattr(model, "_profiler"):
                model._profiler = self

    @property
    def voltage_stats(self):
        return _StatsView(self)

    def remove_hooks(self):
        if self.model is not None and getattr(self.model, "_profiler", None) is self:
            self.model._profiler = None
        self.hooks = []

    def reset(self):
        for g in self._groups.values():
            g.reset()
        self._samples = {n: 0 for n in self._samples}

    # ---- device side ----
    def update(self, name, state):
        self.update_many([name], [state])

    def update_many(self, names, states):
        """Fold the states (each ``[2, B, C, H, W]``: membrane, spikes) into the accumulators of their layers, in
        as few launches as SNNFLOW_VSTATS_MAX_TENSORS allows.  Storage in the engine's order
        (``engine.nhwc_state_strides``) or contiguous is read in place; anything else is made contiguous."""
        if len(names) != len(states):
            raise ValueError("update_many: one name per state")
        runs = {}
        nhwc = {}   # shape -> the engine's strides for it
        for name, s in zip(names, states):
            shp = s.shape
            if len(shp) != 5 or shp[0] != 2:
                raise _lib.SnnflowError(f"{name}: a state is [2, B, C, H, W] (membrane, spikes), got {tuple(shp)}")
            if not s.is_cuda or s.dtype != torch.float32:
                _lib.require_device(s, name)
            want = nhwc.get(shp)
            if want is None:
                want = nhwc[shp] = nhwc_state_strides(*shp[1:])
            if (s.stride() == want or _same_strides(s, want)) and s.data_ptr() % 16 == 0:
                layout = _lib.LAYOUT_NHWC
            else:
                layout = _lib.LAYOUT_NCHW
                if not s.is_contiguous():
                    s = s.detach().contiguous()
            runs.setdefault((*shp[1:], layout, s.device), []).append((name, s))
        for (B, C, H, W, layout, dev), items in runs.items():
            g = self._groups.get((C, H, W, dev))
            if g is None:
                g = self._groups[(C, H, W, dev)] = _Group(C, H, W, dev, self.histogram)
            for name, _ in items:
                where = self._where.get(name)
                if where is None:
                    self._where[name] = (g, g.slot(name))
                    self._samples[name] = 0
                elif where[0] is not g:
                    raise _lib.SnnflowError(f"{name}: profiled as C, H, W = {where[0].C, where[0].H, where[0].W} before")
            for i0 in range(0, len(items), _lib.VSTATS_MAX_TENSORS):
                self._launch(g, B, layout, items[i0:i0 + _lib.VSTATS_MAX_TENSORS])

    def _launch(self, g, B, layout, items):
        a = _lib.VstatsArgs()
        a.n, a.B, a.C, a.H, a.W, a.layout, a.nslots = len(items), B, g.C, g.H, g.W, layout, g.cap
        slots = set()
        for i, (name, s) in enumerate(items):
            a.state[i] = s.data_ptr()
            a.slot[i] = slot = self._where[name][1]
            slots.add(slot)
            self._samples[name] += B
        need = lib.snnflow_vstats_scratch_bytes(len(slots), B, g.C, g.H, g.W, layout)
        if need < 0:
            raise _lib.SnnflowError(f"membrane profiling: no kernel for C = {g.C} (4, 8, 16, 32 or 64)")
        if g.scratch is None or g.scratch.numel() * 8 < need:
            g.scratch = torch.empty((need + 7) // 8, dtype=torch.float64, device=g.device)
        for k, v in g.t.items():
            setattr(a, k, v.data_ptr())
        a.scratch, a.scratch_bytes = g.scratch.data_ptr(), g.scratch.numel() * 8
        _lib.call("vstats_update", lib.snnflow_vstats_update, a, _lib.stream_ptr(g.device))

    # ---- host side ----
    def accumulators(self, name):
        """Numpy copies of the layer's accumulators (one device-to-host copy each): ``count``, ``nonfinite``,
        ``chan_sum``, ``chan_sumsq`` (float64 [C]), ``chan_min``, ``chan_max`` (float32 [C]), ``chan_spikes``
        (uint64 [C]), ``neuron_spikes`` (uint32 [C, H*W]), ``hist`` (uint64 [65536], or None) and ``samples``
        (batch entries seen)."""
        g, slot = self._where[name]
        out = {k: v[slot].cpu().numpy() for k, v in g.t.items()}
        out["count"], out["nonfinite"] = int(out["count"]), int(out["nonfinite"])
        out["chan_spikes"] = out["chan_spikes"].view(np.uint64)
        out["neuron_spikes"] = np.ascontiguousarray(out["neuron_spikes"].view(np.uint32).T)
        out["hist"] = out["hist"].view(np.uint64) if "hist" in out else None
        out["samples"] = self._samples[name]
        out["shape"] = (g.C, g.H, g.W)
        return out

    def _streaming(self, name, acc=None):
        acc = acc or self.accumulators(name)
        C, H, W = acc["shape"]
        return {"count": acc["count"],
                "voltage_sum": float(acc["chan_sum"].sum()),
                "voltage_sum_sq": float(acc["chan_sumsq"].sum()),
                "voltage_min": float(acc["chan_min"].min()),
                "voltage_max": float(acc["chan_max"].max()),
                "spike_sum": float(acc["chan_spikes"].sum()),
                "per_neuron_spike_sums": acc["neuron_spikes"].astype(np.float64),
                "per_neuron_counts": np.full((C, H * W), float(acc["samples"])),
                "channel_spike_sums": acc["chan_spikes"].astype(np.float64),
                "channel_counts": acc["samples"] * H * W,
                "num_channels": C}

    def quantile_bracket(self, name, q):
        """(lo, hi) float32 with ``lo <= np.percentile(all finite membrane values of the layer, q) <= hi``
        (``quantile_bracket_from_hist``); needs ``histogram=True``."""
        if not self.histogram:
            raise _lib.SnnflowError("quantile_bracket needs VoltageProfiler(histogram=True)")
        g, slot = self._where[name]
        return quantile_bracket_from_hist(g.t["hist"][slot].cpu().numpy(), q)

    def compute_statistics(self):
        """``analyze_voltage_dynamics.py:145-241``: the same keys, layers sorted by name, every formula in
        float64.  Three differences: ``channel_voltage_mins/maxs/means/stds`` and ``channel_voltage_ranges``
        are per channel (the reference fills them with the global value or None); with the histogram on,
        ``voltage_median`` / ``voltage_q5`` / ``voltage_q95`` are the midpoints of their quantile brackets
        (the reference: nan); ``nonfinite`` (NaN / inf membrane values, left out of everything else) is
        new.  The dict feeds the reference's ``generate_visualizations`` / ``save_statistics_csv``."""
        stats = {}
        for name in sorted(self._where):
            acc = self.accumulators(name)
            data = self._streaming(name, acc)
            count = data["count"]
            mean = data["voltage_sum"] / count if count > 0 else 0
            var = (data["voltage_sum_sq"] / count) - (mean ** 2) if count > 0 else 0
            std = np.sqrt(max(var, 0))
            C = data["num_channels"]
            ch_rates = (data["channel_spike_sums"] / data["channel_counts"] if data["channel_counts"] > 0
                        else np.zeros(C))
            n_rates = data["per_neuron_spike_sums"] / np.maximum(data["per_neuron_counts"], 1)
            # per-channel voltage statistics (finite values of a channel: count / C when none is non-finite;
            # else the per-channel counts are not kept and the means use the global share)
            per_ch = count / C if count > 0 else 0
            with np.errstate(invalid="ignore", divide="ignore"):
                ch_mean = acc["chan_sum"] / per_ch if per_ch else np.zeros(C)
                ch_var = acc["chan_sumsq"] / per_ch - ch_mean ** 2 if per_ch else np.zeros(C)
            med = q5 = q95 = np.nan
            if self.histogram and count > 0:
                med, q5, q95 = (float(np.mean(np.float64(quantile_bracket_from_hist(acc["hist"], q))))
                                for q in (50, 5, 95))
            stats[name] = {
                "num_samples": "N/A (streaming)",
                "num_channels": C,
                "spatial_size": n_rates.shape[1],
                "voltage_min": float(data["voltage_min"]),
                "voltage_max": float(data["voltage_max"]),
                "voltage_mean": float(mean),
                "voltage_std": float(std),
                "voltage_median": med,
                "voltage_q5": q5,
                "voltage_q95": q95,
                "channel_voltage_mins": acc["chan_min"].astype(np.float64),
                "channel_voltage_maxs": acc["chan_max"].astype(np.float64),
                "channel_voltage_means": ch_mean,
                "channel_voltage_stds": np.sqrt(np.maximum(ch_var, 0)),
                "spike_rate_global": float(data["spike_sum"] / count if count > 0 else 0),
                "channel_spike_rates": ch_rates,
                "per_neuron_spike_rates": n_rates,
                "channels_dead": int((ch_rates == 0).sum()),
                "channels_very_low": int((ch_rates < 0.01).sum()),
                "channels_low": int((ch_rates < 0.05).sum()),
                "channels_moderate": int((ch_rates < 0.20).sum()),
                "neurons_dead": int((n_rates == 0).sum()),
                "neurons_very_low": int((n_rates < 0.01).sum()),
                "neurons_low": int((n_rates < 0.05).sum()),
                "neurons_moderate": int((n_rates < 0.20).sum()),
                "total_neurons": n_rates.size,
                "channel_voltage_ranges": acc["chan_max"].astype(np.float64) - acc["chan_min"].astype(np.float64),
                "voltages_raw": np.array([]),
                "spikes_raw": np.array([]),
                "nonfinite": acc["nonfinite"],
            }
        return stats

    def membrane_ranges(self):
        """``eval_flow_quant.py:314-463`` per layer: ``min``, ``max``, ``mean``, ``median``, ``std``, ``p1``,
        ``p2_5``, ``p5``, ``p6``, ``p25``, ``p75``, ``p95``, ``p99``, ``p999``, ``iqr``, ``lower_fence``,
        ``upper_fence``, ``total_samples`` and ``recommended_min`` / ``recommended_max`` by the reference's
        per-layer strategy table -- over ALL finite membrane values profiled, not the reference's 10 000
        random samples per batch.  Percentiles come from the histogram and are rounded outward: p1 .. p25
        are the lower end of their bracket (``quantile_bracket``), p75 .. p999 the upper end, the median the
        midpoint, so a recommended range never covers less than the true percentile span.  ``robust_min`` /
        ``robust_max`` / ``outlier_count`` / ``outlier_percent`` need the raw values and are left out."""
        if not self.histogram:
            raise _lib.SnnflowError("membrane_ranges needs VoltageProfiler(histogram=True)")
        out = {}
        for name in sorted(self._where):
            acc = self.accumulators(name)
            n = acc["count"]
            if n == 0:
                continue
            mean = float(acc["chan_sum"].sum()) / n
            var = float(acc["chan_sumsq"].sum()) / n - mean ** 2
            r = {"min": float(acc["chan_min"].min()), "max": float(acc["chan_max"].max()), "mean": mean,
                 "median": float(np.mean(np.float64(quantile_bracket_from_hist(acc["hist"], 50)))),
                 "std": float(np.sqrt(max(var, 0.0)))}
            for key, q in _LOW_KEYS:
                r[key] = float(quantile_bracket_from_hist(acc["hist"], q)[0])
            for key, q in _HIGH_KEYS:
                r[key] = float(quantile_bracket_from_hist(acc["hist"], q)[1])
            r["iqr"] = r["p75"] - r["p25"]
            r["lower_fence"] = r["p25"] - 1.5 * r["iqr"]
            r["upper_fence"] = r["p75"] + 1.5 * r["iqr"]
            r["total_samples"] = n
            lo_key, hi_key = LAYER_STRATEGIES.get(name.split(".")[-1], ("p1", "p99"))
            r["recommended_min"], r["recommended_max"] = r[lo_key], r[hi_key]
            out[name] = r
        return out
