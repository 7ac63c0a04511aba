"""CPU-side checks of the visual evaluation (no GPU compute): the numpy restatement
(tests/vis_ref.py) reproduces the reference's renderers as recorded in tests/golden/vis_case.npz
bit for bit, the percentile kernel's interpolation arithmetic reproduces np.percentile bit for
bit, the new C-ABI entry points have the declared layouts and validate their arguments, and
save_error_heatmap draws on the host."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vis_ref  # noqa: E402
from vis_ref import assert_bit_equal  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "snnflow.h")
FLOW_CASES = [("flow_zeros", "flow_zeros_img", None), ("flow_odd", "flow_odd_img", None), ("flow_b2", "flow_b2_img", None),
              ("flow_uni", "flow_uni_none", None), ("flow_uni", "flow_uni_half", 0.5), ("flow_uni", "flow_uni_fifth", 0.2),
              ("flow_allzero", "flow_allzero_img", None)]


@pytest.fixture(scope="module")
def g(golden):
    return golden("vis_case.npz")


@pytest.mark.parametrize("case,key,uv", FLOW_CASES, ids=[c[1] for c in FLOW_CASES])
def test_restated_flow_to_image_bitwise(g, case, key, uv):
    flow = g[f"{case}_in"]
    got = np.stack([vis_ref.flow_to_image(f[0], f[1], uv) for f in flow])
    assert_bit_equal(got, g[key], key)


@pytest.mark.parametrize("case", ["ev_poisson", "ev_frac", "ev_flat"])
@pytest.mark.parametrize("scheme", ["green_red", "gray"])
def test_restated_events_to_image_bitwise(g, case, scheme):
    assert_bit_equal(vis_ref.events_to_image(g[f"{case}_in"], scheme), g[f"{case}_{scheme}"], f"{case} {scheme}")


def test_restated_error_and_minmax_bitwise(g):
    assert_bit_equal(vis_ref.error_to_image(g["err_in"]), g["err_img"], "err batched")
    assert_bit_equal(vis_ref.error_to_image(g["err_in"][1]), g["err_img1"], "err 2-D")
    for k in ("mm_generic", "mm_const"):
        assert_bit_equal(vis_ref.minmax_norm(g[f"{k}_in"]), g[f"{k}_out"], k)


def test_percentile_arithmetic_reproduces_numpy_bitwise():
    rng = np.random.default_rng(5)
    planes = [rng.normal(0, 3, n).astype(np.float32) for n in (1, 2, 3, 63, 64, 65, 1023, 1025, 4097, 260 * 346)]
    planes += [rng.poisson(0.7, 999).astype(np.float32), (1 + 1e-3 * rng.random(777)).astype(np.float32),
               np.full(50, -2.5, dtype=np.float32)]
    for x in planes:
        for q in (0, 1, 5, 50, 95, 99, 100):
            a, b = vis_ref.percentile_model(x, q, True), np.percentile(x.astype(np.float64), q)
            assert np.float64(a).tobytes() == np.float64(b).tobytes(), (x.size, q, a, b)
            a, b = vis_ref.percentile_model(x, q, False), np.percentile(x, q)
            assert type(b) is np.float32 and np.float32(a).tobytes() == b.tobytes(), (x.size, q, a, b)


@pytest.mark.parametrize("name", vis_ref.METRICS)
def test_restated_error_maps_match_reference(g, name):
    """The float32 restatement of the kernel's expressions against the reference's torch maps, under the
    bound tests/test_gpu_vis.py derives for the device (the validity masks are exact)."""
    nb = g[f"met_{name}_err"].shape[1]
    for k in range(g["met_flow"].shape[0]):
        args = (g["met_flow"][k][:nb], g["met_gtflow"][k][:nb], g["met_event_mask"][k][:nb, 0],
                np.broadcast_to(g["met_dt_gt"][k] / g["met_dt_input"][k], (nb,)), 128.0, name)
        e, valid, _, _ = vis_ref.error_maps(*args)
        assert (valid == (g[f"met_{name}_valid"][k] != 0)).all()
        bound = vis_ref.error_map_bound(g[f"met_{name}_err"][k], *args)
        assert (np.abs(e.astype(np.float64) - g[f"met_{name}_err"][k]) <= bound).all()


STRUCTS = [("PercentilesArgs", "snnflow_percentiles_args"), ("FlowToImageArgs", "snnflow_flow_to_image_args"),
           ("EventsToImageArgs", "snnflow_events_to_image_args"), ("MinmaxNormArgs", "snnflow_minmax_norm_args"),
           ("ErrorMapsArgs", "snnflow_error_maps_args")]


def test_vis_args_layouts_match_c(tmp_path):
    from snnflow import _lib

    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){"]
    for py, c in STRUCTS:
        lines.append(f'printf("{c}.size %zu\\n", sizeof({c}));')
        for fname, _ in getattr(_lib, py)._fields_:
            lines.append(f'printf("{c}.{fname} %zu\\n", offsetof({c}, {fname}));')
    lines += ['printf("abi %d\\n", SNNFLOW_ABI_VERSION);', 'printf("maxq %d\\n", SNNFLOW_VIS_MAX_Q);',
              'printf("em %d %d %d\\n", SNNFLOW_EM_AEE, SNNFLOW_EM_AAE, SNNFLOW_EM_NAAE);', "return 0;}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = dict(line.split(" ", 1) for line in out if line)
    for py, c in STRUCTS:
        cls = getattr(_lib, py)
        assert int(got[f"{c}.size"]) == ctypes.sizeof(cls), c
        for fname, _ in cls._fields_:
            assert int(got[f"{c}.{fname}"]) == getattr(cls, fname).offset, (c, fname)
    assert int(got["abi"]) == _lib.ABI_VERSION and int(got["maxq"]) == _lib.VIS_MAX_Q
    assert got["em"] == f"{_lib.EM_AEE} {_lib.EM_AAE} {_lib.EM_NAAE}"


def test_vis_entries_validate_before_any_launch():
    from snnflow import _lib

    lib, E_ARG, PTR = _lib.lib, -1, 64

    def refused(fn, a, what):
        assert fn(ctypes.byref(a), None) == E_ARG, what
        assert what.encode() in lib.snnflow_last_error()

    for name in ("snnflow_percentiles", "snnflow_flow_to_image", "snnflow_events_to_image", "snnflow_minmax_norm",
                 "snnflow_error_to_image", "snnflow_error_maps"):
        assert name in _lib.EXPORTS
    assert lib.snnflow_percentiles(None, None) == E_ARG and lib.snnflow_error_maps(None, None) == E_ARG

    a = _lib.PercentilesArgs()
    refused(lib.snnflow_percentiles, a, "percentiles")            # all zero / NULL
    a.nplanes, a.n, a.nq, a.x, a.out = 1, 16, 1, PTR, PTR
    a.q[0] = 101.0
    refused(lib.snnflow_percentiles, a, "percentiles")            # q out of range
    a.q[0], a.nq = 50.0, 5
    refused(lib.snnflow_percentiles, a, "percentiles")            # more than SNNFLOW_VIS_MAX_Q
    a.nq, a.n = 1, 0
    refused(lib.snnflow_percentiles, a, "percentiles")            # empty planes
    a.n, a.out = 16, None
    refused(lib.snnflow_percentiles, a, "percentiles")

    a = _lib.FlowToImageArgs()
    refused(lib.snnflow_flow_to_image, a, "flow_to_image")
    a.B, a.H, a.W, a.flow, a.stats = 1, 4, 4, PTR, PTR              # out NULL
    refused(lib.snnflow_flow_to_image, a, "flow_to_image")
    a.out, a.W = PTR, 0
    refused(lib.snnflow_flow_to_image, a, "flow_to_image")

    a = _lib.EventsToImageArgs()
    refused(lib.snnflow_events_to_image, a, "events_to_image")
    a.B, a.H, a.W, a.cnt, a.out = 1, 4, 4, PTR, PTR                 # stats NULL
    refused(lib.snnflow_events_to_image, a, "events_to_image")

    a = _lib.MinmaxNormArgs()
    refused(lib.snnflow_minmax_norm, a, "minmax_norm")
    a.B, a.n, a.x, a.stats = 1, 0, PTR, PTR
    refused(lib.snnflow_minmax_norm, a, "minmax_norm")

    assert lib.snnflow_error_to_image(None, 4, PTR, None) == E_ARG
    assert lib.snnflow_error_to_image(PTR, 0, PTR, None) == E_ARG
    assert b"error_to_image" in lib.snnflow_last_error()

    a = _lib.ErrorMapsArgs()
    refused(lib.snnflow_error_maps, a, "error_maps")
    a.B, a.H, a.W = 1, 4, 4
    for f in ("flow", "gtflow", "event_mask", "dt_ratio", "err", "sum"):
        setattr(a, f, PTR)
    refused(lib.snnflow_error_maps, a, "error_maps")              # sum without count
    a.count, a.metric = PTR, 3
    refused(lib.snnflow_error_maps, a, "error_maps")              # unknown metric
    a.metric, a.H = 0, 0
    refused(lib.snnflow_error_maps, a, "error_maps")


def test_save_error_heatmap_on_host_made_maps(tmp_path):
    import torch

    import snnflow

    cfg = {"loader": {"resolution": [18, 16]}, "loss": {}}
    m = snnflow.AEE(cfg, torch.device("cpu"))
    assert m.error_maps is False and m.get_error_map() is None
    assert snnflow.AAE(dict(cfg, metrics={"heat_map": True}), "cpu").error_maps is True
    assert snnflow.AAE(dict(cfg, vis={"store": True}), "cpu").error_maps is True
    assert snnflow.AAE(dict(cfg, vis={"enabled": True, "store": False}), "cpu").error_maps is True
    assert snnflow.AAE(dict(cfg, vis={"enabled": False}, metrics={}), "cpu").error_maps is False
    path = tmp_path / "heat.png"
    assert m.get_final_error_heatmap() == (None, None)
    assert m.save_error_heatmap(str(path)) is False and not path.exists()
    rng = np.random.default_rng(0)
    err = torch.from_numpy(rng.random((2, 18, 16)).astype(np.float32))
    mask = torch.from_numpy((rng.random((2, 18, 16)) < 0.5).astype(np.float32))
    m.accumulate_error_heatmap(err, mask)
    m.accumulate_error_heatmap(err, mask)
    avg, count = m.get_final_error_heatmap()
    np.testing.assert_array_equal(count.numpy(), 2 * mask.sum(0).numpy())
    np.testing.assert_allclose(avg.numpy(), (2 * (err * mask).sum(0) / (2 * mask.sum(0) + 1e-9)).numpy(), rtol=1e-6)
    # the keywords eval_flow.py passes beyond the reference's own signature are accepted
    assert m.save_error_heatmap(save_path=str(path), title="AEE", cmap="jet", mag_threshold=0.5,
                                show_magnitude_overlay=False) is True
    assert path.stat().st_size > 0 and path.read_bytes()[:4] == b"\x89PNG"
    m.reset()
    assert m.get_final_error_heatmap()[0] is not None   # reset() keeps the aggregate
    m.reset_error_heatmap()
    assert m.get_final_error_heatmap() == (None, None) and m.save_error_heatmap(str(path)) is False
