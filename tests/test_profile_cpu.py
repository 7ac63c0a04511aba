"""CPU-side checks of the membrane profiling (no GPU compute): the numpy restatement (tests/profile_ref.py)
reproduces the reference's VoltageProfiler as recorded in tests/golden/profile_case.npz, the histogram key is
monotone and the quantile brackets always contain np.percentile, snnflow_vstats_args has the declared layout
and snnflow_vstats_update validates its arguments before any launch."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import profile_ref  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "snnflow.h")
QS = (0, 1, 2.5, 5, 6, 25, 50, 75, 95, 99, 99.9, 100)
SIZES = (1, 2, 3, 64, 1000, 4097, 50000)


@pytest.fixture(scope="module")
def g(golden):
    return golden("profile_case.npz")


@pytest.mark.parametrize("layer", profile_ref.LAYERS)
@pytest.mark.parametrize("case", profile_ref.CASES)
def test_restatement_reproduces_reference(g, case, layer):
    acc = profile_ref.accumulate(list(profile_ref.golden_states(g, case, layer)))
    assert acc["nonfinite"] == 0
    profile_ref.check_against_golden(g, case, layer, profile_ref.streaming(acc), profile_ref.statistics(acc),
                                     inexact=False)


def test_fixture_holds_the_branches_it_exists_for(g):
    for case in profile_ref.CASES:
        for layer in profile_ref.LAYERS:
            pre = f"{case}_{layer}"
            assert g[f"{pre}_states"].shape == (5, 2, 2, 4, 6, 10)
            assert g[f"{pre}_cs_channels_dead"] >= 1
            r = g[f"{pre}_cs_per_neuron_spike_rates"]
            for thr in (0.01, 0.05, 0.20):
                assert (r < thr).any() and (r >= thr).any()
            if case == "generic":
                assert abs(g[f"{pre}_cs_voltage_mean"]) < 0.1 * g[f"{pre}_cs_voltage_std"]


def _planes():
    rng = np.random.default_rng(11)
    for n in SIZES:
        x = rng.normal(0, 1, n).astype(np.float32)
        yield f"normal{n}", x
        z = x.copy()
        z[rng.random(n) < 0.3] = 0.0
        z[::7] *= -0.0   # some -0.0 among the zeros
        yield f"zeros{n}", z
        yield f"cluster{n}", (1.0 + 1e-4 * rng.random(n)).astype(np.float32) * np.float32(rng.choice([-1.0, 1.0]))


def test_key16_is_monotone_and_edges_bound_their_bin():
    from snnflow import profile

    for name, x in _planes():
        xs = np.sort(x)
        k = profile_ref.key16(xs)
        assert (np.diff(k) >= 0).all(), name
        assert (k == profile.key16(xs)).all(), name
        lo, hi = profile.bin_edges(k)
        assert (lo <= xs).all() and (xs <= hi).all(), name
        assert (profile_ref.key16(lo) == k).all() and (profile_ref.key16(hi) == k).all(), name
    assert profile_ref.key16(np.float32(-0.0)) == profile_ref.key16(np.float32(0.0)) == 0x8000
    for j in (0x8000, 0x7FFF, 0xBF80, 0x4000, 0xFF7F, 0x0080):
        lo, hi = profile.bin_edges(j)
        assert lo == profile_ref.bin_lo(j) and hi == profile_ref.bin_hi(j)


def test_quantile_brackets_contain_numpy_percentile():
    from snnflow.profile import quantile_bracket_from_hist

    for name, x in _planes():
        n = x.size
        xs = np.sort(x)
        hist = np.bincount(profile_ref.key16(x), minlength=profile_ref.BINS)
        for q in QS:
            lo, hi = quantile_bracket_from_hist(hist, q)
            k = int(np.floor(q / 100.0 * (n - 1)))
            assert lo <= xs[k] <= profile_ref.bin_hi(profile_ref.key16(xs[k])), (name, q)
            p = np.percentile(x.astype(np.float64), q)
            assert lo <= p <= hi, (name, q, lo, p, hi)
            assert lo == profile_ref.bin_lo(profile_ref.key16(xs[k])), (name, q)
            assert hi == profile_ref.bin_hi(profile_ref.key16(xs[min(k + 1, n - 1)])), (name, q)


def test_vstats_args_layout_matches_c(tmp_path):
    from snnflow import _lib

    c = "snnflow_vstats_args"
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
             f'printf("size %zu\\n", sizeof({c}));']
    for fname, _ in _lib.VstatsArgs._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof({c}, {fname}));')
    lines += ['printf("abi %d\\n", SNNFLOW_ABI_VERSION);',
              'printf("consts %d %d %d %d\\n", SNNFLOW_VSTATS_MAX_TENSORS, SNNFLOW_VSTATS_BINS, SNNFLOW_LAYOUT_NHWC, '
              'SNNFLOW_LAYOUT_NCHW);', "return 0;}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = dict(line.split(" ", 1) for line in out if line)
    assert int(got["size"]) == ctypes.sizeof(_lib.VstatsArgs)
    for fname, _ in _lib.VstatsArgs._fields_:
        assert int(got[fname]) == getattr(_lib.VstatsArgs, fname).offset, fname
    assert int(got["abi"]) == _lib.ABI_VERSION == 41
    assert got["consts"] == f"{_lib.VSTATS_MAX_TENSORS} {_lib.VSTATS_BINS} {_lib.LAYOUT_NHWC} {_lib.LAYOUT_NCHW}"
    assert _lib.VSTATS_MAX_TENSORS >= 32 and "snnflow_vstats_update" in _lib.EXPORTS


def _good_args(_lib):
    a, PTR = _lib.VstatsArgs(), 64
    a.n, a.B, a.C, a.H, a.W, a.layout, a.nslots = 2, 1, 8, 4, 4, _lib.LAYOUT_NHWC, 3
    a.state[0], a.state[1] = PTR, PTR
    a.slot[0], a.slot[1] = 0, 2
    for f in ("count", "nonfinite", "chan_sum", "chan_sumsq", "chan_min", "chan_max", "chan_spikes", "neuron_spikes",
              "hist", "scratch"):
        setattr(a, f, PTR)
    a.scratch_bytes = _lib.lib.snnflow_vstats_scratch_bytes(2, 1, 8, 4, 4, _lib.LAYOUT_NHWC)
    return a


def test_vstats_update_validates_before_any_launch():
    from snnflow import _lib

    lib, E_ARG, E_CHANNELS = _lib.lib, -1, -2

    def refused(mutate, what, code=E_ARG):
        a = _good_args(_lib)
        mutate(a)
        assert lib.snnflow_vstats_update(ctypes.byref(a), None) == code, what
        assert b"vstats" in lib.snnflow_last_error(), what

    assert lib.snnflow_vstats_update(None, None) == E_ARG and b"vstats" in lib.snnflow_last_error()
    refused(lambda a: ctypes.memset(ctypes.byref(a), 0, ctypes.sizeof(a)), "all zero")
    assert _good_args(_lib).scratch_bytes > 0
    refused(lambda a: setattr(a, "n", 0), "n = 0")
    refused(lambda a: setattr(a, "n", _lib.VSTATS_MAX_TENSORS + 1), "n > MAX")
    refused(lambda a: a.slot.__setitem__(1, 3), "slot == nslots")
    refused(lambda a: a.slot.__setitem__(0, -1), "negative slot")
    refused(lambda a: setattr(a, "layout", 2), "unknown layout")
    for f in ("B", "H", "W"):
        refused(lambda a, f=f: setattr(a, f, 0), f"{f} = 0")
        refused(lambda a, f=f: setattr(a, f, -3), f"{f} < 0")
    refused(lambda a: a.state.__setitem__(1, None), "NULL state")
    for f in ("count", "nonfinite", "chan_sum", "chan_sumsq", "chan_min", "chan_max", "chan_spikes", "neuron_spikes",
              "scratch"):
        refused(lambda a, f=f: setattr(a, f, None), f"NULL {f}")
    refused(lambda a: setattr(a, "scratch_bytes", a.scratch_bytes - 1), "scratch too small")
    for c in (0, 2, 12, 128):
        refused(lambda a, c=c: setattr(a, "C", c), f"C = {c}", E_CHANNELS)
        assert lib.snnflow_vstats_scratch_bytes(1, 1, c, 4, 4, _lib.LAYOUT_NHWC) == -1
    for c in (4, 8, 16, 32, 64):
        assert lib.snnflow_vstats_scratch_bytes(_lib.VSTATS_MAX_TENSORS, 2, c, 5, 7, _lib.LAYOUT_NCHW) > 0


def test_profiler_surface_without_a_device():
    import torch

    import snnflow
    from oracle import lif_ref

    model = snnflow.LIFFireNet(dict(lif_ref.make_unet_kwargs(base_num_channels=8)))
    assert model._profiler is None
    prof = snnflow.VoltageProfiler(model, torch.device("cpu"))
    assert prof.hooks == [] and model._profiler is prof
    assert sorted(prof.layer_names.values()) == sorted(n for n, _ in model.layer_spec)
    assert not model._cellwise() and not any(m._forward_hooks for m in model.modules())
    assert len(prof.voltage_stats) == 0 and prof.compute_statistics() == {} and prof.membrane_ranges() == {}
    with pytest.raises(snnflow.SnnflowError):   # no CPU fallback
        prof.update("head", torch.zeros(2, 1, 8, 4, 4))
    prof.remove_hooks()
    assert model._profiler is None and prof.hooks == []
