"""Writes tests/golden/vis_case.npz: what the reference's static renderers and error-map
bookkeeping make of small inputs.

    python tests/golden/make_golden_vis.py REFERENCE_ROOT

Runs on the CPU.  The renderers are the reference's own Visualization.flow_to_image /
events_to_image / error_to_image / minmax_norm (utils/visualization.py; the module imports cv2 and
pandas, which its static renderers never touch: empty modules stand in when they are absent); the
metric cases run the reference's loss/flow.py AEE / AAE / NAAE.

Cases (prefix of the keys; every case stores its inputs and the reference's outputs):
  flow_zeros   18x16, ~30 % exact-zero vectors (percentile branch, true zeros black)
  flow_odd     37x53 (odd sizes)
  flow_b2      B = 2, two 18x16 images of different statistics (per-image statistics)
  flow_uni     18x16, every vector of magnitude exactly 5, uniform_v None ("_none"), 0.5 ("_half": still
               clipped to full brightness) and 0.2 ("_fifth")
  flow_allzero 18x16 of zeros
  ev_poisson   Poisson counts, ev_frac a fractional IWE-like plane, ev_flat a plane with
               pos_min == max; each in "green_red" and "gray"
  err          radians over [0, pi] with 0 and values above pi, 2-D and batched
  mm_generic / mm_const   minmax_norm of a generic and of a constant plane
  met          18x16, B = 2 (AAE: sample 0 alone, the reference's AAE cannot take a batch): three
               successive forward() calls of AEE, AAE and NAAE (ground truth
               with exact zeros, event masks with holes): every call's error map and validity mask,
               the metric values, the final (average, count); compute_window_events and
               compute_masked_window_flow after two associations, in both overwrite modes
The script asserts the branch each case exists for.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
H, W = 18, 16
FLOW_SCALING = 128


def import_reference(ref_root):
    sys.path.insert(0, ref_root)
    for name in ("cv2", "pandas"):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    import matplotlib

    matplotlib.use("Agg")
    import loss.flow as ref_flow
    import utils.visualization as ref_vis
    return ref_vis.Visualization, ref_flow


def flow_cases(Vis, rng, out):
    def put(name, flow, uniform_v=None, key=None):
        out[f"{name}_in"] = flow
        imgs = np.stack([Vis.flow_to_image(f[0], f[1], uniform_v) for f in flow])
        assert imgs.dtype == np.uint8 and imgs.shape == flow.shape[:1] + flow.shape[2:] + (3,)
        out[key or f"{name}_img"] = imgs
        return imgs

    f = rng.normal(0, 2, (1, 2, H, W)).astype(np.float32)
    zero = rng.random((H, W)) < 0.3
    f[0, :, zero] = 0.0
    img = put("flow_zeros", f)
    mag = np.sqrt(f[0, 0] ** 2 + f[0, 1] ** 2)
    assert 0.2 < zero.mean() < 0.4 and (img[0][mag == 0] == 0).all() and (img[0][mag > 0].max(axis=-1) >= 38).all()

    put("flow_odd", (rng.normal(0, 1, (1, 2, 37, 53)) * rng.gamma(2.0, 1.0, (1, 1, 37, 53))).astype(np.float32))

    b2 = np.stack([rng.normal(0, 0.05, (2, H, W)), rng.normal(3, 6, (2, H, W))]).astype(np.float32)
    img = put("flow_b2", b2)
    # per-image statistics: each image equals its own single-image rendering
    assert (img[0] == Vis.flow_to_image(b2[0, 0], b2[0, 1])).all() and (img[0] != img[1]).any()

    vecs = np.array([(3, 4), (-3, 4), (3, -4), (-3, -4), (4, 3), (-4, 3), (4, -3), (-4, -3), (5, 0), (-5, 0), (0, 5),
                     (0, -5)], dtype=np.float32)
    uni = vecs[rng.integers(0, len(vecs), (H, W))].transpose(2, 0, 1)[None].copy()
    m = np.linalg.norm(np.stack((uni[0, 0], uni[0, 1]), axis=2), axis=2)
    assert (m == 5.0).all()
    a = put("flow_uni", uni, None, "flow_uni_none")
    b = put("flow_uni", uni, 0.5, "flow_uni_half")
    c = put("flow_uni", uni, 0.2, "flow_uni_fifth")
    # uniform branch: sqrt(0.5)*1.3 + 0.15 still clips to full brightness, sqrt(0.2)*1.3 + 0.15 = 0.73 does not
    assert a.max() == 255 and (a == b).all() and c.max() == int(255 * (np.sqrt(0.2) * 1.3 + 0.15))
    assert (uni[0, 1] == 0).any() and (uni[0, 0] < 0).any()     # hue 1.0 (atan2 = pi) occurs

    img = put("flow_allzero", np.zeros((1, 2, H, W), dtype=np.float32))
    assert (img == 0).all()


def event_cases(Vis, rng, out):
    pois = rng.poisson(0.7, (H, W, 2)).astype(np.float32)
    frac = (rng.gamma(0.6, 1.5, (37, 53, 2)) * (rng.random((37, 53, 2)) < 0.6)).astype(np.float32)
    flat = np.zeros((H, W, 2), dtype=np.float32)
    flat[:, :, 0] = 2.0                                  # pos_min == pos_max == max
    flat[:, :, 1] = rng.integers(0, 3, (H, W))
    for name, cnt in (("ev_poisson", pois), ("ev_frac", frac), ("ev_flat", flat)):
        out[f"{name}_in"] = cnt
        for scheme in ("green_red", "gray"):
            img = Vis.events_to_image(cnt.copy(), scheme)
            assert img.dtype == np.float64
            out[f"{name}_{scheme}"] = img
    assert np.percentile(flat[:, :, 0], 1) == max(np.percentile(flat[:, :, 0], 99), np.percentile(flat[:, :, 1], 99))
    assert (out["ev_flat_green_red"][:, :, 1] == 1.0).all()          # the raw 2.0, clipped
    assert np.percentile(pois[:, :, 0], 1) != np.percentile(pois[:, :, 0], 99)
    g = out["ev_poisson_green_red"]
    assert ((g[:, :, 0] > 0) & (g[:, :, 1] > 0)).any() and (g[:, :, 2] == 0).all()


def error_cases(Vis, rng, out):
    e = rng.uniform(0, np.pi, (2, H, W)).astype(np.float32)
    e[0, 0, :4] = (0.0, np.pi, 3.5, 7.0)
    e[1, 0, :2] = (0.0, 4.0)
    out["err_in"] = e
    out["err_img"] = Vis.error_to_image(e)               # the reference draws sample 0 of a batch
    out["err_img1"] = Vis.error_to_image(e[1])
    assert out["err_img"][0, 0, 0] == 0 and (out["err_img"][0, 2:4, 0] == 255).all()
    assert (out["err_img"] == Vis.error_to_image(e[0])).all() and (out["err_img"][:, :, 1:] == 0).all()


def minmax_cases(Vis, rng, out):
    x = rng.normal(1, 3, (37, 53)).astype(np.float32)
    c = np.full((H, W), 0.25, dtype=np.float32)
    out["mm_generic_in"], out["mm_generic_out"] = x, Vis.minmax_norm(x)
    out["mm_const_in"], out["mm_const_out"] = c, Vis.minmax_norm(c)
    assert out["mm_generic_out"].dtype == np.float32 and 0 < out["mm_generic_out"].mean() < 1
    assert (out["mm_generic_out"] == 0).any() and (out["mm_generic_out"] == 1).any()
    assert (out["mm_const_out"] == 0.25).all()           # den == 0: values pass through the clip


def metric_cases(ref_flow, rng, out):
    B, N, CALLS = 2, 60, 3
    dev = torch.device("cpu")

    def window():
        ev = np.zeros((B, N, 4), dtype=np.float32)
        ev[:, :, 0] = rng.random((B, N))
        ev[:, :, 1] = rng.integers(0, H, (B, N))
        ev[:, :, 2] = rng.integers(0, W, (B, N))
        ev[:, :, 3] = rng.choice([-1.0, 1.0], (B, N))
        ev[1, N - 7:] = 0.0                               # padding events of the shorter sample
        pol = np.stack([ev[:, :, 3] > 0, ev[:, :, 3] < 0], axis=2).astype(np.float32)
        mask = (rng.random((B, 1, H, W)) < 0.6).astype(np.float32)      # holes
        gt = rng.normal(0, 4, (B, 2, H, W)).astype(np.float32)
        gt[:, :, rng.random((H, W)) < 0.2] = 0.0                          # invalid ground truth
        gt[0, 0, 0, :5] = 0.0                                             # one component zero: still valid
        flow = (rng.normal(0, 4, (B, 2, H, W)) / FLOW_SCALING).astype(np.float32)
        flow[:, :, 3, :4] = (gt[:, :, 3, :4] / FLOW_SCALING / 0.8).astype(np.float32)  # near-parallel: the acos clamp
        flow[:, :, 5, :3] = 0.0                                           # zero prediction
        return {"event_list": ev, "event_list_pol_mask": pol, "event_mask": mask, "gtflow": gt, "flow": flow,
                "dt_input": np.array([1.0], dtype=np.float32), "dt_gt": np.array([0.8], dtype=np.float32)}

    wins = [window() for _ in range(CALLS)]
    for k in wins[0]:
        out[f"met_{k}"] = np.stack([w[k] for w in wins])

    def feed(m, w, nb=B):
        inputs = {k: torch.from_numpy(v[:nb].copy() if k[:2] != "dt" else v.copy()) for k, v in w.items() if k != "flow"}
        m.event_flow_association([torch.from_numpy(w["flow"][:nb].copy())], inputs)

    def cfg(overwrite):
        return {"loader": {"resolution": [H, W]}, "loss": {"overwrite_intermediate": overwrite}}

    for name in ("AEE", "AAE", "NAAE"):
        m = getattr(ref_flow, name)(cfg(False), dev, flow_scaling=FLOW_SCALING)
        seen = []
        m.accumulate_error_heatmap = (lambda e, k, _orig=m.accumulate_error_heatmap, _s=seen:
                                      (_s.append((e.clone().numpy().reshape(k.shape), k.clone().numpy())), _orig(e, k))[1])
        vals = []
        # the reference's AAE divides a [B,1,H,W] product by a [B,H,W] dot product, which only lines
        # up for B = 1: its case is sample 0 of every window
        nb = 1 if name == "AAE" else B
        for w in wins:
            feed(m, w, nb)
            r = m()
            vals.append(np.stack([t.numpy() for t in r]) if isinstance(r, tuple) else r.numpy()[None])
            m.reset()
        assert len(seen) == CALLS
        out[f"met_{name}_err"] = np.stack([s[0] for s in seen])           # [CALLS][B][H][W]
        out[f"met_{name}_valid"] = np.stack([s[1] for s in seen])
        out[f"met_{name}_values"] = np.stack(vals)                        # [CALLS][1 or 2][B]
        avg, count = m.get_final_error_heatmap()                          # reset() kept the aggregate
        out[f"met_{name}_avg"], out[f"met_{name}_count"] = avg.numpy(), count.numpy()
        assert out[f"met_{name}_err"].dtype == np.float32 and np.isfinite(out[f"met_{name}_err"]).all()
        v = out[f"met_{name}_valid"]
        assert 0.2 < v.mean() < 0.7 and count.max() >= 2 and (count == 0).any() and (count == 1).any()
        if name == "AAE":
            assert (m.get_error_map() == seen[-1][0]).all()
            e = out["met_AAE_err"]
            assert (e == e.min()).sum() > 8          # pixels at the upper clamp of the cosine
    g0 = wins[0]["gtflow"]
    assert ((g0[:, 0] == 0) & (g0[:, 1] == 0)).any() and ((g0[:, 0] == 0) & (g0[:, 1] != 0)).any()

    for overwrite in (False, True):
        m = ref_flow.AEE(cfg(overwrite), dev, flow_scaling=FLOW_SCALING)
        feed(m, wins[0])
        feed(m, wins[1])
        if overwrite:
            m.overwrite_intermediate_flow([torch.from_numpy(wins[1]["flow"].copy())])
        tag = "ow" if overwrite else "avg"
        out[f"met_win_events_{tag}"] = m.compute_window_events().numpy()
        out[f"met_win_flow_{tag}"] = m.compute_masked_window_flow().numpy()
        assert out[f"met_win_events_{tag}"].sum() == 2 * (2 * N - 7)
    assert (out["met_win_events_avg"] == out["met_win_events_ow"]).all() and out["met_win_events_avg"].max() >= 2
    assert (out["met_win_flow_avg"] != out["met_win_flow_ow"]).any()


def main():
    Vis, ref_flow = import_reference(os.path.abspath(sys.argv[1]))
    rng = np.random.default_rng(20260101)
    torch.manual_seed(0)
    out = {}
    flow_cases(Vis, rng, out)
    event_cases(Vis, rng, out)
    error_cases(Vis, rng, out)
    minmax_cases(Vis, rng, out)
    metric_cases(ref_flow, rng, out)
    path = os.path.join(HERE, "vis_case.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
