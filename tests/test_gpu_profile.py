"""On-device membrane profiling (snnflow_vstats_update, snnflow.VoltageProfiler) against the reference's
VoltageProfiler as recorded in tests/golden/profile_case.npz, against fp64 numpy (tests/profile_ref.py), on
special values, for run-to-run reproducibility, attached to a LIFFireNet, and for the quantile ranges."""
import copy
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import profile_ref  # noqa: E402

import snnflow  # noqa: E402
from oracle import lif_ref  # noqa: E402
from snnflow import _lib  # noqa: E402
from snnflow.engine import nhwc_state_strides  # noqa: E402
from snnflow.synthetic import make_window  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4, 1, 1), (2, 4, 6, 10), (3, 8, 5, 7), (1, 32, 9, 11), (2, 16, 3, 130), (1, 64, 2, 3), (4, 8, 64, 64)]
MODES = ("one", "five", "chunk")
LAYOUTS = ("nhwc", "nchw")
RANGE_KEYS_LOW = (("p1", 1), ("p2_5", 2.5), ("p5", 5), ("p6", 6), ("p25", 25))
RANGE_KEYS_HIGH = (("p75", 75), ("p95", 95), ("p99", 99), ("p999", 99.9))


@pytest.fixture(scope="module")
def g(golden):
    return golden("profile_case.npz")


def upload(st, layout, dev):
    """numpy [2, B, C, H, W] -> device tensor stored contiguous (nchw) or in the engine's order (nhwc)"""
    t = torch.from_numpy(np.ascontiguousarray(st)).to(dev)
    if layout == "nchw":
        return t
    _, B, C, H, W = t.shape
    out = torch.empty_strided(tuple(t.shape), nhwc_state_strides(B, C, H, W), device=dev, dtype=torch.float32)
    out.copy_(t)
    return out


def assert_acc_equal(got, ref, what):
    """device accumulators against the restatement's: sums within N * 2^-52 * sum|x| of the exactly rounded sum
    (twice the first-order worst case of fp64 summation in any order), everything else exact"""
    assert got["count"] == ref["count"] and got["nonfinite"] == ref["nonfinite"], what
    assert got["samples"] == ref["samples"], what
    for k in ("chan_min", "chan_max", "chan_spikes", "neuron_spikes", "hist"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=f"{what} {k}")
    for k, absk in (("chan_sum", "chan_abs"), ("chan_sumsq", "chan_abs_sq")):
        bound = ref["chan_n"] * 2.0 ** -52 * ref[absk]
        assert (np.abs(got[k] - ref[k]) <= bound).all(), (what, k, np.abs(got[k] - ref[k]).max(), bound.min())


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", profile_ref.CASES)
def test_golden_matches_reference_profiler(g, dev, case, layout):
    prof = snnflow.VoltageProfiler(None, dev)
    names, states = [], []
    T = profile_ref.golden_states(g, case, "head").shape[0]
    for t in range(T):
        for layer in ("head", "G1"):
            names.append(layer)
            states.append(upload(profile_ref.golden_states(g, case, layer)[t], layout, dev))
    prof.update_many(names, states)
    stats = prof.compute_statistics()
    assert list(stats) == list(profile_ref.LAYERS) and prof.hooks == []
    for layer in profile_ref.LAYERS:
        assert stats[layer]["nonfinite"] == 0
        profile_ref.check_against_golden(g, case, layer, prof.voltage_stats[layer], stats[layer])
        # the fields the reference only approximates are per channel here
        mem = profile_ref.golden_states(g, case, layer)[:, 0].astype(np.float64)
        np.testing.assert_array_equal(stats[layer]["channel_voltage_mins"], mem.min(axis=(0, 1, 3, 4)))
        np.testing.assert_array_equal(stats[layer]["channel_voltage_maxs"], mem.max(axis=(0, 1, 3, 4)))
        np.testing.assert_allclose(stats[layer]["channel_voltage_means"], mem.mean(axis=(0, 1, 3, 4)), rtol=1e-12,
                                   atol=1e-15)
        np.testing.assert_allclose(stats[layer]["channel_voltage_stds"], mem.std(axis=(0, 1, 3, 4)), rtol=1e-9)
        for key, q in (("voltage_median", 50), ("voltage_q5", 5), ("voltage_q95", 95)):
            lo, hi = prof.quantile_bracket(layer, q)
            assert lo <= np.percentile(mem, q) <= hi and lo <= stats[layer][key] <= hi


@functools.lru_cache(maxsize=None)
def numpy_case(shape, mode):
    """states (numpy), their slots and the restatement's accumulators per slot; computed once per (shape, mode)"""
    B, C, H, W = shape
    rng = np.random.default_rng([*shape, MODES.index(mode)])
    n = {"one": 1, "five": 5, "chunk": _lib.VSTATS_MAX_TENSORS + 3}[mode]
    slots = [0] * n if mode == "one" else [(3 * i + 1) % 2 for i in range(n)]
    states = []
    for _ in range(n):
        mem = (rng.standard_normal((B, C, H, W)) * rng.choice([1e-3, 1.0, 50.0])).astype(np.float32)
        spk = (rng.random((B, C, H, W)) < 0.25).astype(np.float32)
        mem[spk != 0] = 0.0
        spk[rng.random((B, C, H, W)) < 0.01] = 3.0   # any non-zero value counts as a spike
        states.append(np.stack([mem, spk]))
    refs = {s: profile_ref.accumulate([st for st, k in zip(states, slots) if k == s]) for s in sorted(set(slots))}
    return states, slots, refs


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_accumulators_match_fp64_numpy(dev, shape, mode, layout):
    states, slots, refs = numpy_case(shape, mode)
    prof = snnflow.VoltageProfiler(None, dev)
    names = [f"layer{s}" for s in slots]
    dev_states = [upload(st, layout, dev) for st in states]
    if mode == "one":
        prof.update(names[0], dev_states[0])
    else:
        prof.update_many(names, dev_states)
    for s, ref in refs.items():
        assert_acc_equal(prof.accumulators(f"layer{s}"), ref, f"{shape} {mode} {layout} slot {s}")


@pytest.mark.parametrize("hist_mode", [0, 1], ids=["global", "lds"])
def test_histogram_modes_give_the_same_table(dev, hist_mode):
    """snnflow_vstats_hist_mode: direct global atomics and the LDS sub-table (bins of 2^-6 <= |v| < 4; the
    tensors' scales 1e-3, 1 and 50 fall below, inside and above it) fill the same table."""
    old = _lib.lib.snnflow_vstats_hist_mode(-1)
    try:
        assert _lib.lib.snnflow_vstats_hist_mode(hist_mode) == hist_mode
        for shape in ((2, 4, 6, 10), (1, 32, 9, 11), (4, 8, 64, 64)):
            for layout in LAYOUTS:
                states, slots, refs = numpy_case(shape, "five")
                prof = snnflow.VoltageProfiler(None, dev)
                prof.update_many([f"layer{s}" for s in slots], [upload(st, layout, dev) for st in states])
                for s, ref in refs.items():
                    assert_acc_equal(prof.accumulators(f"layer{s}"), ref, f"{shape} {layout} hist mode {hist_mode}")
    finally:
        _lib.lib.snnflow_vstats_hist_mode(old)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_special_values(dev, layout):
    B, C, H, W = 1, 4, 2, 5
    mem = np.full((B, C, H, W), 0.5, dtype=np.float32)
    flt_max, denorm = np.finfo(np.float32).max, np.float32(1e-42)
    mem[0, 0, 0, :5] = [np.nan, np.inf, -np.inf, -0.0, denorm]
    mem[0, 1, 1, 2] = flt_max
    st = np.stack([mem, np.zeros_like(mem)])
    prof = snnflow.VoltageProfiler(None, dev)
    prof.update("x", upload(st, layout, dev))
    acc = prof.accumulators("x")
    assert acc["nonfinite"] == 3 and acc["count"] == mem.size - 3
    # -0.0 lands in +0.0's bin (0x8000, which the positive denormal shares), not in the negative zero's (0x7FFF)
    assert profile_ref.key16(np.float32(0.0)) == profile_ref.key16(denorm) == 0x8000
    assert acc["hist"][0x8000] == 2 and acc["hist"][0x7FFF] == 0
    assert acc["hist"][profile_ref.key16(flt_max)] == 1 and acc["hist"].sum() == mem.size - 3
    assert_acc_equal(acc, profile_ref.accumulate([st]), f"special {layout}")
    assert acc["chan_min"][0] == 0.0 and acc["chan_max"][0] == 0.5 and acc["chan_max"][1] == flt_max
    assert np.isfinite(acc["chan_sum"]).all() and np.isfinite(acc["chan_sumsq"]).all()
    assert acc["chan_sum"][0] == 0.5 * (H * W - 5) + float(denorm)
    assert prof.compute_statistics()["x"]["nonfinite"] == 3


def test_same_calls_give_identical_bytes(dev):
    states, slots, _ = numpy_case((4, 8, 64, 64), "five")
    accs = []
    for _ in range(2):
        prof = snnflow.VoltageProfiler(None, dev)
        ts = [upload(st, "nhwc", dev) for st in states]
        prof.update_many([f"l{s}" for s in slots], ts)
        prof.update("l0", ts[2])
        prof.update_many(["l1", "l0"], [upload(states[0], "nchw", dev), upload(states[1], "nchw", dev)])
        accs.append([prof.accumulators(n) for n in ("l0", "l1")])
    for a, b in zip(*accs):
        for k in ("chan_sum", "chan_sumsq", "chan_min", "chan_max", "chan_spikes", "neuron_spikes", "hist"):
            assert a[k].tobytes() == b[k].tobytes(), k
        assert (a["count"], a["nonfinite"]) == (b["count"], b["nonfinite"])


def test_reset_clears(dev):
    states, slots, refs = numpy_case((2, 4, 6, 10), "five")
    prof = snnflow.VoltageProfiler(None, dev, histogram=False)
    names = [f"layer{s}" for s in slots]
    prof.update_many(names, [upload(st, "nhwc", dev) for st in states])
    prof.reset()
    assert prof.accumulators("layer0")["count"] == 0 and prof.accumulators("layer0")["hist"] is None
    prof.update_many(names, [upload(st, "nchw", dev) for st in states])
    got = prof.accumulators("layer1")
    got["hist"] = refs[1]["hist"]   # (histogram off)
    assert_acc_equal(got, refs[1], "after reset")
    assert np.isnan(prof.compute_statistics()["layer1"]["voltage_median"])
    with pytest.raises(snnflow.SnnflowError):
        prof.membrane_ranges()


def _model_and_windows(dev, train):
    torch.manual_seed(3)
    model = snnflow.LIFFireNet(dict(lif_ref.make_unet_kwargs(base_num_channels=8))).to(dev)
    model = model.train() if train else model.eval()
    gen = torch.Generator(device=dev).manual_seed(7)
    wins = [make_window(2, 400, 16, 16, gen, dev) for _ in range(3)]
    return model, wins


def _np_states(states):
    return [s.detach().cpu().numpy() for s in states]


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_model_per_window_calls(dev, train):
    model, wins = _model_and_windows(dev, train)
    plain = copy.deepcopy(model)
    prof = snnflow.VoltageProfiler(model, dev)
    names = [n for n, _ in model.layer_spec]
    seen = {n: [] for n in names}
    with torch.set_grad_enabled(train):
        flows, flows_plain = [], []
        for w in wins:
            flows.append(model(w["event_voxel"], w["event_cnt"])["flow"][0])
            for n, s in zip(names, _np_states(model.states)):
                seen[n].append(s)
            flows_plain.append(plain(w["event_voxel"], w["event_cnt"])["flow"][0])
    assert prof.hooks == [] and not model._cellwise()
    assert not any(m._forward_hooks or m._forward_pre_hooks for m in model.modules())
    for a, b in zip(flows, flows_plain):
        assert torch.equal(a, b)
    assert sorted(prof.voltage_stats) == sorted(names)
    for n in names:
        assert_acc_equal(prof.accumulators(n), profile_ref.accumulate(seen[n]), f"model() {n}")
    before = prof.accumulators("head")["count"]
    prof.remove_hooks()
    assert model._profiler is None
    with torch.set_grad_enabled(train):
        a = model(wins[0]["event_voxel"], wins[0]["event_cnt"])["flow"][0]
        b = plain(wins[0]["event_voxel"], wins[0]["event_cnt"])["flow"][0]
    assert torch.equal(a, b) and prof.accumulators("head")["count"] == before


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_model_forward_sequence(dev, train):
    model, wins = _model_and_windows(dev, train)
    plain = copy.deepcopy(model)
    prof = snnflow.VoltageProfiler(model, dev)
    names = [n for n, _ in model.layer_spec]
    model.engine.capture_states = True
    vox, cnt = [w["event_voxel"] for w in wins], [w["event_cnt"] for w in wins]
    with torch.set_grad_enabled(train):
        outs = model.forward_sequence(vox, cnt)
        outs_plain = plain.forward_sequence(vox, cnt)
    assert not model._cellwise() and prof.hooks == []
    for a, b in zip(outs, outs_plain):
        assert torch.equal(a["flow"][0], b["flow"][0])
    sts = model.engine.seq_states
    assert len(sts) == len(wins) and len(sts[0]) == len(names)
    for l, n in enumerate(names):
        ref = profile_ref.accumulate(_np_states([sts[t][l] for t in range(len(wins))]))
        assert_acc_equal(prof.accumulators(n), ref, f"forward_sequence {n}")
    prof.remove_hooks()
    assert model._profiler is None


def _check_ranges(r, mem):
    mem = mem.astype(np.float64).ravel()
    assert r["total_samples"] == mem.size and r["min"] == mem.min() and r["max"] == mem.max()
    for key, q in RANGE_KEYS_LOW:
        assert r[key] <= np.percentile(mem, q), key
    for key, q in RANGE_KEYS_HIGH:
        assert r[key] >= np.percentile(mem, q), key
    assert r["iqr"] == r["p75"] - r["p25"]
    assert r["lower_fence"] == r["p25"] - 1.5 * r["iqr"] and r["upper_fence"] == r["p75"] + 1.5 * r["iqr"]
    np.testing.assert_allclose(r["mean"], mem.mean(), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(r["std"], mem.std(), rtol=1e-9)


def test_membrane_ranges(g, dev):
    prof = snnflow.VoltageProfiler(None, dev)
    mems = {}
    for case in profile_ref.CASES:
        for layer in ("head", "G1", "R2b"):
            st = profile_ref.golden_states(g, case, "head" if layer == "R2b" else layer)
            name = f"{case}.{layer}"
            prof.update_many([name] * len(st), [upload(s, "nhwc", dev) for s in st])
            mems[name] = st[:, 0]
    big, _, _ = numpy_case((4, 8, 64, 64), "one")
    prof.update("big", upload(big[0], "nhwc", dev))
    mems["big"] = big[0][0]
    ranges = prof.membrane_ranges()
    assert list(ranges) == sorted(mems)
    for name, mem in mems.items():
        r = ranges[name]
        _check_ranges(r, mem)
        flat = mem.astype(np.float64).ravel()
        for q in (0, 1, 2.5, 5, 6, 25, 50, 75, 95, 99, 99.9, 100):
            lo, hi = prof.quantile_bracket(name, q)
            assert lo <= np.percentile(flat, q) <= hi, (name, q)
        lo, hi = prof.quantile_bracket(name, 50)
        assert r["median"] == (float(lo) + float(hi)) / 2
        lo_key, hi_key = {"head": ("p2_5", "p99"), "R2b": ("p6", "p99")}.get(name.split(".")[-1], ("p1", "p99"))
        assert (r["recommended_min"], r["recommended_max"]) == (r[lo_key], r[hi_key])
        assert not {"robust_min", "robust_max", "outlier_count", "outlier_percent"} & set(r)
