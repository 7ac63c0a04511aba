"""CPU-side checks of the contrast-maximisation landscape (no GPU compute): the oracle's EventWarpingRef,
looped like the reference's demo, reproduces tests/golden/landscape_case.npz; the regulariser constant of
flow_heatmap is the oracle's smoothness term on a constant map; snnflow_landscape_args has the declared layout
(ABI still 41); and every unsupported argument is refused before any launch."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "snnflow.h")
CASES = ("a", "b")


@pytest.fixture(scope="module")
def g(golden):
    return golden("landscape_case.npz")


def case_config(g, case, weight=None):
    H, W, _, _, w, mask_output = g[f"{case}_meta"]
    return {"loader": {"resolution": [int(H), int(W)]},
            "loss": {"flow_regul_weight": float(w) if weight is None else weight},
            "model": {"mask_output": bool(mask_output)}}


def oracle_heatmap(g, case, weight=None, dtype=torch.float32):
    """The demo's loop (demo_iwe.py:71-85) on oracle.iwe_ref.EventWarpingRef; [R, R] float64."""
    from oracle import iwe_ref

    cfg = case_config(g, case, weight)
    H, W = cfg["loader"]["resolution"]
    R = int(g[f"{case}_meta"][3])
    ev, pol, mask = (torch.from_numpy(g[f"{case}_{k}"]).to(dtype) for k in ("events", "pol", "mask"))
    ref = iwe_ref.EventWarpingRef([H, W], flow_scaling=1, weight=cfg["loss"]["flow_regul_weight"],
                                  smoothing_mask=cfg["model"]["mask_output"])
    out = np.zeros((R, R))
    for k, (u, v) in enumerate(g[f"{case}_cand"]):
        flow = torch.ones(ev.shape[0], 2, H, W, dtype=dtype)
        flow[:, 0] *= float(u)
        flow[:, 1] *= float(v)
        ref.event_flow_association([flow], ev, pol, mask)
        out[k // R, k % R] = float(ref())
        ref.reset()
    return out


@pytest.mark.parametrize("case", CASES)
def test_oracle_loop_reproduces_fixture(g, case):
    np.testing.assert_allclose(oracle_heatmap(g, case), g[f"{case}_heatmap"].astype(np.float64), rtol=1e-6, atol=0)


def test_fixture_holds_what_it_exists_for(g):
    from snnflow import contrast

    for case, (H, W, maxdisp, R) in (("a", (12, 20, 4, 9)), ("b", (40, 72, 8, 9))):
        assert tuple(g[f"{case}_meta"][:4]) == (H, W, maxdisp, R)
        xs, ys, cand = contrast.grid_candidates(maxdisp, maxdisp, R)
        assert (xs == g[f"{case}_x_scale"]).all() and (ys == g[f"{case}_y_scale"]).all()
        assert (cand == g[f"{case}_cand"]).all() and cand.dtype == np.float32
        ev = g[f"{case}_events"]
        assert (ev[:, 0, 0] == 0).all() and (ev[:, -1, 0] == 1).all()       # exact-integer warps
        assert np.isfinite(g[f"{case}_heatmap"]).all()
    assert g["a_events"].shape == (2, 300, 4) and g["b_events"].shape == (1, 1500, 4)
    assert (g["b_pol"].sum(axis=2) == 0).any()                                # events that left the frame
    heat = g["b_heatmap"]
    j, i = np.unravel_index(np.argmin(heat), heat.shape)
    assert (g["b_x_scale"][i], g["b_y_scale"][j]) == (6.0, -4.0)              # the known answer
    assert np.sort(heat.ravel())[1] > 1.1 * heat.min()                        # and a clear one


def test_regulariser_constant(g):
    """flow_heatmap adds weight * smoothness_constant.  Two references:
    the oracle in float64 with and without the weight (their difference is the term itself, exact to
    ~1e-12; the float32 oracle is pinned to the fixture above): rtol 1e-5;
    the fixture heatmap minus the float32 oracle's data term.  The reference rounds data + term to float32
    once, so that difference carries up to half a float32 spacing of the heatmap value (6e-8 at 1.x, 3e-4 of
    the 1.8e-4 term): the bound is that half spacing plus rtol 1e-5 of the term."""
    from snnflow import contrast

    cfg = case_config(g, "a")
    weight = cfg["loss"]["flow_regul_weight"]
    assert weight == 0.001 and cfg["model"]["mask_output"]
    term = weight * float(contrast.smoothness_constant(torch.from_numpy(g["a_mask"]), cfg))
    exact = oracle_heatmap(g, "a", dtype=torch.float64) - oracle_heatmap(g, "a", weight=0.0, dtype=torch.float64)
    print("term", term, "float64 oracle", exact.min(), exact.max())
    np.testing.assert_allclose(np.full_like(exact, term), exact, rtol=1e-5, atol=0)
    heat = g["a_heatmap"]
    diff = heat.astype(np.float64) - oracle_heatmap(g, "a", weight=0.0)
    print("fixture - data", diff.min(), diff.max())
    assert (np.abs(diff - term) <= 0.5 * np.spacing(heat).astype(np.float64) + 1e-5 * term).all()
    # without the event mask every pair counts
    H, W = cfg["loader"]["resolution"]
    plain = float(contrast.smoothness_constant(torch.from_numpy(g["a_mask"]), {"model": {}}))
    pairs = 2 * (H * (W - 1) + (H - 1) * W + 2 * (H - 1) * (W - 1))
    assert plain == pytest.approx(pairs * 1e-3 / 5, rel=1e-5)


def test_landscape_args_layout_matches_c(tmp_path):
    from snnflow import _lib

    c = "snnflow_landscape_args"
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
             f'printf("size %zu\\n", sizeof({c}));']
    for fname, _ in _lib.LandscapeArgs._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof({c}, {fname}));')
    lines += ['printf("abi %d\\n", SNNFLOW_ABI_VERSION);', "return 0;}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = dict(line.split(" ", 1) for line in out if line)
    assert int(got["size"]) == ctypes.sizeof(_lib.LandscapeArgs)
    for fname, _ in _lib.LandscapeArgs._fields_:
        assert int(got[fname]) == getattr(_lib.LandscapeArgs, fname).offset, fname
    assert int(got["abi"]) == _lib.ABI_VERSION == 41
    assert "snnflow_iwe_landscape" in _lib.EXPORTS and "snnflow_iwe_landscape_scratch_floats" in _lib.EXPORTS


def _good_args(_lib):
    a, PTR = _lib.LandscapeArgs(), 64
    a.B, a.N, a.K, a.H, a.W, a.loss_scaling, a.flow_scaling = 2, 100, 7, 37, 53, 1, 1.0
    a.events = a.pol = a.cand = a.out = a.scratch = PTR
    a.scratch_floats = _lib.lib.snnflow_iwe_landscape_scratch_floats(2, 100, 7, 37, 53)
    return a


def test_c_entry_validates_before_any_launch():
    from snnflow import _lib

    lib, E_ARG = _lib.lib, -1

    def refused(mutate, what):
        a = _good_args(_lib)
        mutate(a)
        assert lib.snnflow_iwe_landscape(ctypes.byref(a), None) == E_ARG, what
        assert b"iwe_landscape" in lib.snnflow_last_error(), what

    assert lib.snnflow_iwe_landscape(None, None) == E_ARG
    assert _good_args(_lib).scratch_floats > 0
    for f in ("B", "N", "K", "H", "W"):
        refused(lambda a, f=f: setattr(a, f, 0), f"{f} = 0")
        refused(lambda a, f=f: setattr(a, f, -2), f"{f} < 0")
    refused(lambda a: (setattr(a, "H", 2048), setattr(a, "W", 1025)), "H * W > 2^21")
    refused(lambda a: (setattr(a, "B", 1 << 16), setattr(a, "K", 1 << 15)), "B * K past the grid")
    for f in ("events", "pol", "cand", "out", "scratch"):
        refused(lambda a, f=f: setattr(a, f, None), f"NULL {f}")
    refused(lambda a: setattr(a, "events", 72), "events not 16-byte aligned")
    refused(lambda a: setattr(a, "scratch", 72), "scratch not 16-byte aligned")
    refused(lambda a: setattr(a, "scratch_floats", a.scratch_floats - 1), "scratch too small")
    assert lib.snnflow_iwe_landscape_scratch_floats(1, 10, 1, 2048, 1025) == -1
    assert lib.snnflow_iwe_landscape_scratch_floats(1, 10, 0, 8, 8) == -1
    assert lib.snnflow_iwe_landscape_scratch_floats(1, 0, 1, 8, 8) == -1
    # the scratch holds the binned events: it does not grow with the number of candidates
    assert (lib.snnflow_iwe_landscape_scratch_floats(1, 40000, 2500, 180, 240)
            == lib.snnflow_iwe_landscape_scratch_floats(1, 40000, 1, 180, 240) < 6 * 40000)


def test_python_entries_validate_before_any_launch():
    import snnflow

    ev, pol = torch.zeros(2, 50, 4), torch.zeros(2, 50, 2)
    mask = torch.zeros(2, 1, 12, 20)
    cfg = {"loader": {"resolution": [12, 20]}, "loss": {"flow_regul_weight": 0.001}, "model": {"mask_output": True}}
    cand = np.zeros((3, 2), dtype=np.float32)
    err = snnflow.SnnflowError
    with pytest.raises(err, match="HIP device"):          # a CPU tensor: no CPU fallback
        snnflow.loss_landscape(ev, pol, (12, 20), cand)
    with pytest.raises(err, match="HIP device"):
        snnflow.flow_heatmap(ev, pol, mask, cfg, 4, 4, 3)
    with pytest.raises(err, match="HIP device"):
        snnflow.best_global_flow(ev, pol, mask, cfg, 4, 4, 3)
    with pytest.raises(err, match="float32"):             # a non-float32 tensor
        snnflow.loss_landscape(ev.double(), pol, (12, 20), cand)
    with pytest.raises(err, match="float32"):
        snnflow.loss_landscape(ev, pol.to(torch.int32), (12, 20), cand)
    with pytest.raises(err, match=r"candidates \(3, 3\)"):  # [K, 3] candidates
        snnflow.loss_landscape(ev, pol, (12, 20), np.zeros((3, 3), dtype=np.float32))
    with pytest.raises(err, match="candidates"):
        snnflow.loss_landscape(ev, pol, (12, 20), torch.zeros(0, 2))
    with pytest.raises(err, match="event_mask"):          # a resolution that disagrees with the event mask
        snnflow.flow_heatmap(ev, pol, mask, dict(cfg, loader={"resolution": [20, 12]}), 4, 4, 3)
    with pytest.raises(err, match="event_mask"):
        snnflow.best_global_flow(ev, pol, mask[:1], cfg, 4, 4, 3)
    with pytest.raises(err, match="2\\^21"):               # H * W > 2^21
        snnflow.loss_landscape(ev, pol, (2048, 1025), cand)
    with pytest.raises(err, match="2\\^21"):
        snnflow.flow_heatmap(ev, pol, mask, dict(cfg, loader={"resolution": [2048, 1025]}), 4, 4, 3)
    with pytest.raises(err, match="polarity masks"):
        snnflow.loss_landscape(ev, pol[:, :40], (12, 20), cand)
    with pytest.raises(err, match="events"):
        snnflow.loss_landscape(ev[:, :, :3], pol, (12, 20), cand)
    with pytest.raises(NotImplementedError):
        snnflow.flow_heatmap(ev, pol, mask, dict(cfg, loss={"flow_regul_weight": 0.0, "overwrite_intermediate": True}))
