"""CPU-side checks of the batch preparation (no GPU compute): the numpy restatement
(tests/loader_ref.py) reproduces the reference's loader as recorded in
tests/golden/loader_case.npz, BatchPreparer draws the reference's augmentation flags, and the
new C-ABI entry point has the declared layout and validates its arguments."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loader_ref  # noqa: E402
from loader_ref import CASES, TENSORS, assert_bit_equal, case_inputs, config  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "snnflow.h")
MECH = list(loader_ref.MECH)


@pytest.fixture(scope="module")
def g(golden):
    return golden("loader_case.npz")


@pytest.mark.parametrize("case", ["A", "Bk", "Bp"])
def test_restatement_reproduces_reference_bitwise(g, case):
    _, mode, pooled, keep = CASES[case]
    xs, ys, ts, ps, counts, gt = case_inputs(g, case)
    ref = loader_ref.RefPreparer(config(g, mode, pooled, 3, keep=keep), int(g["num_bins"]), flags=g[f"{case}_flags"])
    out = ref.prepare(xs, ys, ts, ps, counts, gt)
    for k in TENSORS + (("gtflow",) if gt is not None else ()):
        assert_bit_equal(out[k], g[f"{case}_{k}"], f"{case} {k}")


def test_restatement_reproduces_hot_filter_sequence(g):
    T, B = g["C_xs"].shape[:2]
    ref = loader_ref.RefPreparer(config(g, "gtflow_dt1", True, B, keep=True, hot=True), int(g["num_bins"]))
    for t in range(T):
        if t == int(g["C_reset_before"]):
            ref.reset_sequence(int(g["C_reset_slot"]))
        ref.flags = g["C_flags"][t]
        out = ref.prepare(g["C_xs"][t], g["C_ys"][t], g["C_ts"][t], g["C_ps"][t], g["C_counts"][t])
        for k in TENSORS:
            assert_bit_equal(out[k], g[f"C_{k}"][t], f"C window {t} {k}")
        assert_bit_equal(ref.hot_events, g["C_hot_events"][t], f"C window {t} hot_events")
        assert (ref.hot_idx == g["C_hot_idx"][t]).all()


def test_restatement_generic_timestamps(g):
    xs, ys, ts, ps, counts, _ = case_inputs(g, "D")
    ref = loader_ref.RefPreparer(config(g, "events", False, 3), int(g["num_bins"]), flags=g["D_flags"])
    out = ref.prepare(xs, ys, ts, ps, counts)
    for k in TENSORS:
        if k != "event_voxel":
            assert_bit_equal(out[k], g[f"D_{k}"], f"D {k}")
    err = np.abs(out["event_voxel"].astype(np.float64) - g["D_event_voxel"])
    assert (err <= loader_ref.voxel_bound(out)).all(), err.max()


def test_flags_follow_the_reference_draws(g):
    import snnflow

    F = g["F_flags"]
    B = F.shape[1]
    np.random.seed(int(g["F_seed"]))
    prep = snnflow.BatchPreparer(config(g, "events", False, B, prob=tuple(float(v) for v in g["F_prob"])), 3)

    def flags():
        return np.array([[prep.batch_augmentation[m][b] for m in MECH] for b in range(B)])

    assert (flags() == F[0]).all()
    for slot in range(B):
        prep.reset_sequence(slot)
        assert (flags() == F[slot + 1]).all(), slot


def test_loader_args_layout_matches_c(tmp_path):
    from snnflow import _lib

    py = _lib.LoaderArgs
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(snnflow_loader_args));']
    for fname, _ in py._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(snnflow_loader_args, {fname}));')
    lines += ['printf("abi %d\\n", SNNFLOW_ABI_VERSION);',
              'printf("aug %d %d %d\\n", SNNFLOW_AUG_H, SNNFLOW_AUG_V, SNNFLOW_AUG_P);', "return 0;}"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", str(c), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = dict(line.split(" ", 1) for line in out if line)
    assert int(got["size"]) == ctypes.sizeof(py)
    for fname, _ in py._fields_:
        assert int(got[fname]) == getattr(py, fname).offset, fname
    assert int(got["abi"]) == 41 == _lib.ABI_VERSION
    assert got["aug"] == f"{_lib.AUG_H} {_lib.AUG_V} {_lib.AUG_P}"


def test_loader_prepare_validates_before_any_launch():
    from snnflow import _lib

    lib = _lib.lib
    assert "snnflow_loader_prepare" in _lib.EXPORTS and "snnflow_loader_scratch_floats" in _lib.EXPORTS
    a = _lib.LoaderArgs()
    assert lib.snnflow_loader_prepare(ctypes.byref(a), None) == -1
    assert b"loader_prepare" in lib.snnflow_last_error()
    a.B, a.N, a.H0, a.W0, a.Ht, a.Wt, a.num_bins = 1, 4, 18, 16, 7, 8, 2   # 18 % 7 != 0
    for f in ("xs", "ys", "ts", "ps", "event_cnt", "event_voxel", "event_mask", "event_list", "pol_mask", "scratch"):
        setattr(a, f, 64)
    assert lib.snnflow_loader_prepare(ctypes.byref(a), None) == -1
    assert b"loader_prepare" in lib.snnflow_last_error() and b"divide" in lib.snnflow_last_error()
    a.Ht, a.hot_enabled = 6, 1                                               # hot filter without state
    assert lib.snnflow_loader_prepare(ctypes.byref(a), None) == -1
    assert lib.snnflow_loader_scratch_floats(0, 4, 18, 16, 6, 8, 2, 0, 0) == -1
    # min/max partials (2 floats, rounded up to 4) + full-resolution cnt, voxel, mask
    # + hot mask, candidate rates, candidate pixels + candidate counters (1, rounded up to 4)
    assert lib.snnflow_loader_scratch_floats(1, 4, 18, 16, 6, 8, 2, 1, 0) == 4 + (2 + 2 + 1 + 3) * 18 * 16 + 4
    assert lib.snnflow_loader_scratch_floats(1, 4, 18, 16, 18, 16, 2, 0, 0) == 4


def test_construction_refuses_a_non_divisible_resolution(g):
    import snnflow

    cfg = config(g, "gtflow_dt1", True, 2)
    cfg["loader"]["resolution"] = [7, 8]
    with pytest.raises(snnflow.SnnflowError):
        snnflow.BatchPreparer(cfg, 2)
    cfg["data"]["mode"] = "events"   # events mode never pools: full resolution = loader.resolution
    assert snnflow.BatchPreparer(cfg, 2).out_resolution == [7, 8]


def test_prepare_refuses_host_tensors(g):
    import torch

    import snnflow

    prep = snnflow.BatchPreparer(config(g, "events", False, 3), 3)
    xs, ys, ts, ps, _, _ = case_inputs(g, "A")
    with pytest.raises(snnflow.SnnflowError):
        prep.prepare(*(torch.from_numpy(v.astype(np.float32)) for v in (xs, ys, ts, ps)))
