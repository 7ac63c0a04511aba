"""On-device visual evaluation (snnflow.vis, csrc/vis.hip and the error maps of snnflow.metrics)
against the reference's recorded outputs (tests/golden/vis_case.npz), live numpy and the numpy
restatement (tests/vis_ref.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vis_ref  # noqa: E402
from vis_ref import assert_bit_equal  # noqa: E402

pytestmark = pytest.mark.gpu
QS = (1, 5, 95, 99)
FS = 128


@pytest.fixture(scope="module")
def g(golden):
    return golden("vis_case.npz")


def _patterns(n, rng):
    tied = rng.normal(0, 1, n).astype(np.float32)
    tied[rng.permutation(n)[: max(1, n // 3)]] = 0.25
    signs = rng.normal(0, 1e-3, n).astype(np.float32)
    signs[::3] = 0.0
    signs[1::5] = -0.0
    return {"normal": rng.normal(0, 3, n).astype(np.float32), "tied": tied,
            "equal": np.full(n, -1.75, dtype=np.float32), "poisson": rng.poisson(0.7, n).astype(np.float32),
            "signs": signs, "narrow": (1 + 1e-3 * rng.random(n)).astype(np.float32)}


def _check_percentiles(dev, planes):
    """Planes of one size in one call, both modes, against live np.percentile: equal values."""
    from snnflow import vis

    x = torch.from_numpy(np.stack(planes)).to(dev)
    got32 = vis.percentile(x, QS).cpu().numpy()
    got64 = vis.percentile(x, QS, fp64=True).cpu().numpy()
    assert got32.dtype == np.float32 and got64.dtype == np.float64 and got32.shape == (len(planes), len(QS))
    for i, p in enumerate(planes):
        for k, q in enumerate(QS):
            want32, want64 = np.percentile(p, q), np.percentile(p.astype(np.float64), q)
            assert want32.dtype == np.float32
            assert got32[i, k] == want32, (p.size, i, q, got32[i, k], want32)
            assert got64[i, k] == want64, (p.size, i, q, got64[i, k], want64)


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 4097])
def test_percentiles_equal_numpy(dev, n):
    """Every value pattern as one plane of a single call (several planes with different answers)."""
    _check_percentiles(dev, list(_patterns(n, np.random.default_rng(100 + n)).values()))


def test_percentiles_equal_numpy_full_plane(dev):
    rng = np.random.default_rng(7)
    pats = _patterns(260 * 346, rng)
    _check_percentiles(dev, [pats[k].reshape(260, 346) for k in ("normal", "poisson", "narrow", "tied")])


def test_percentiles_trailing_dims_and_refusals(dev):
    import snnflow
    from snnflow import vis

    x = torch.from_numpy(np.random.default_rng(3).normal(0, 1, (2, 3, 5, 7)).astype(np.float32)).to(dev)
    got = vis.percentile(x, [50]).cpu().numpy()
    want = np.array([[np.percentile(p, 50)] for p in x.cpu().numpy()])
    assert_bit_equal(got, want, "planes flattened over the trailing dims")
    with pytest.raises(snnflow.SnnflowError):
        vis.percentile(x, [1, 2, 3, 4, 5])
    with pytest.raises(snnflow.SnnflowError):
        vis.percentile(x, [101])
    with pytest.raises(snnflow.SnnflowError):
        vis.percentile(x.cpu(), [50])


def _hw2(cnt):
    """[B, 2, H, W] device layout of the reference's [H, W, 2] count image."""
    return np.ascontiguousarray(cnt.transpose(2, 0, 1))[None]


@pytest.mark.parametrize("case", ["ev_poisson", "ev_frac", "ev_flat"])
def test_events_to_image_bit_equal_golden(g, dev, case):
    from snnflow import vis

    cnt = torch.from_numpy(_hw2(g[f"{case}_in"])).to(dev)
    for scheme in ("green_red", "gray"):
        got = vis.events_to_image(cnt, scheme).cpu().numpy()
        assert_bit_equal(got[0], g[f"{case}_{scheme}"].astype(np.float32), f"{case} {scheme}")


def test_events_and_minmax_bit_equal_restatement(g, dev):
    from snnflow import vis

    rng = np.random.default_rng(11)
    cnt = (rng.poisson(1.2, (3, 2, 37, 53)) * rng.random((3, 2, 37, 53)) * np.array([1, 5, 0.2]).reshape(3, 1, 1, 1))
    cnt = cnt.astype(np.float32)
    d = torch.from_numpy(cnt).to(dev)
    for scheme in ("green_red", "gray"):
        got = vis.events_to_image(d, scheme).cpu().numpy()
        for b in range(3):
            want = vis_ref.events_to_image(cnt[b].transpose(1, 2, 0), scheme).astype(np.float32)
            assert_bit_equal(got[b], want, f"random {scheme} {b}")
    x = (rng.normal(0, 2, (3, 37, 53)) * np.array([1, 30, 0.01]).reshape(3, 1, 1)).astype(np.float32)
    got = vis.minmax_norm(torch.from_numpy(x).to(dev)).cpu().numpy()
    for b in range(3):
        assert_bit_equal(got[b], vis_ref.minmax_norm(x[b]), f"minmax random {b}")
    for k in ("mm_generic", "mm_const"):
        got = vis.minmax_norm(torch.from_numpy(g[f"{k}_in"][None]).to(dev)).cpu().numpy()
        assert_bit_equal(got[0], g[f"{k}_out"], k)


def _assert_image_close(got, want, what):
    """uint8 frames: every channel within 1 level and at most max(2, 0.2 %) of the pixels differing
    at all.  The cap is a condition, not a measurement: the device's atan2f (hue), fp64 sqrt against
    numpy's power(., 0.5) and the fp32 degrees constant are the only operations that may differ from
    the host's by an ulp or two; a 2-ulp hue error moves 255*c by < 2e-4 levels, so a pixel changes only
    when 255*c lies that close to an integer: a share of ~4e-4 of channel values at most, against which
    the cap leaves an order of magnitude."""
    assert got.shape == want.shape and got.dtype == np.uint8 == want.dtype, (what, got.shape, want.shape)
    diff = np.abs(got.astype(np.int16) - want.astype(np.int16))
    npix = diff.reshape(-1, 3).max(axis=1)
    print(f"{what}: {int((npix > 0).sum())} of {npix.size} pixels differ, max {int(diff.max())} level(s)")
    assert diff.max() <= 1, what
    assert (npix > 0).sum() <= max(2, 0.002 * npix.size), what


FLOW_CASES = [("flow_zeros", "flow_zeros_img", None), ("flow_odd", "flow_odd_img", None), ("flow_b2", "flow_b2_img", None),
              ("flow_uni", "flow_uni_none", None), ("flow_uni", "flow_uni_half", 0.5), ("flow_uni", "flow_uni_fifth", 0.2),
              ("flow_allzero", "flow_allzero_img", None)]


@pytest.mark.parametrize("case,key,uv", FLOW_CASES, ids=[c[1] for c in FLOW_CASES])
def test_flow_to_image_vs_golden(g, dev, case, key, uv):
    from snnflow import vis

    got = vis.flow_to_image(torch.from_numpy(g[f"{case}_in"]).to(dev), uniform_v=uv).cpu().numpy()
    _assert_image_close(got, g[key], key)


@pytest.mark.parametrize("H,W", [(37, 53), (128, 128)])
def test_flow_and_error_to_image_vs_restatement(dev, H, W):
    from snnflow import vis

    rng = np.random.default_rng(H)
    flow = (rng.normal(0, 1, (2, 2, H, W)) * rng.gamma(2.0, 1.0, (2, 1, H, W))).astype(np.float32)
    flow[0, :, rng.random((H, W)) < 0.25] = 0.0
    flow[1] *= 40.0
    got = vis.flow_to_image(torch.from_numpy(flow).to(dev)).cpu().numpy()
    want = np.stack([vis_ref.flow_to_image(f[0], f[1]) for f in flow])
    _assert_image_close(got, want, f"flow {H}x{W}")
    err = rng.uniform(-0.1, 3.5, (2, H, W)).astype(np.float32)
    got = vis.error_to_image(torch.from_numpy(err).to(dev)).cpu().numpy()
    want = np.stack([vis_ref.error_to_image(e) for e in err])
    _assert_image_close(got, want, f"error {H}x{W}")


def test_error_to_image_vs_golden(g, dev):
    from snnflow import vis

    e = torch.from_numpy(g["err_in"]).to(dev)
    got = vis.error_to_image(e).cpu().numpy()
    assert got.shape == g["err_in"].shape + (3,)
    _assert_image_close(got[0], g["err_img"], "err batched [0]")     # [0] is the reference's image
    _assert_image_close(got[1], g["err_img1"], "err batched [1]")
    _assert_image_close(vis.error_to_image(e[1]).cpu().numpy(), g["err_img1"], "err 2-D")


def test_flow_to_image_graph_capture(dev):
    """Captured once, replayed on new input in the same buffer: equal to the eager result bit for bit."""
    from snnflow import vis

    rng = np.random.default_rng(2)
    a = torch.from_numpy(rng.normal(0, 2, (1, 2, 37, 53)).astype(np.float32)).to(dev)
    b = torch.from_numpy(rng.normal(1, 5, (1, 2, 37, 53)).astype(np.float32)).to(dev)
    buf = a.clone()
    vis.flow_to_image(buf)  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = vis.flow_to_image(buf)
    buf.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    replayed = out.cpu().numpy().copy()
    eager = vis.flow_to_image(b).cpu().numpy()
    assert_bit_equal(replayed, eager, "graph replay")
    assert (replayed != vis.flow_to_image(a).cpu().numpy()).any()


# ---- error maps ----

def _cfg(overwrite=False, **extra):
    return dict({"loader": {"resolution": [18, 16]}, "loss": {"overwrite_intermediate": overwrite}}, **extra)


def _feed(m, g, k, dev, nb):
    t = {key: torch.from_numpy(g[f"met_{key}"][k][:nb]).to(dev)
         for key in ("event_list", "event_list_pol_mask", "event_mask", "gtflow")}
    t["dt_input"], t["dt_gt"] = torch.from_numpy(g["met_dt_input"][k]), torch.from_numpy(g["met_dt_gt"][k])
    m.event_flow_association([torch.from_numpy(g["met_flow"][k][:nb]).to(dev)], t)


def _bound_args(g, k, nb, name):
    return (g["met_flow"][k][:nb], g["met_gtflow"][k][:nb], g["met_event_mask"][k][:nb, 0],
            np.broadcast_to(g["met_dt_gt"][k] / g["met_dt_input"][k], (nb,)), float(FS), name)


@pytest.mark.parametrize("name", vis_ref.METRICS)
def test_error_maps_vs_golden(g, dev, name):
    """Three successive forward() calls with error maps on, against the reference's recorded maps.

    Tolerances.  AEE is sqrt / multiply / add only, all correctly rounded on both sides: within one
    float32 ulp of the reference.  AAE / NAAE: |d| <= 1e-5 |ref| + 8 eps32 (1 + 1/sqrt(max(1 - c^2, 2e-5))),
    for NAAE the second term divided by (|flow'| + 1e-9), c the clamped cosine recomputed in float64.
    The first term is the project's metric tolerance (the rtol of test_flow_metrics_vs_golden).  The
    second is the conditioning of acos: d acos(c)/dc = -1/sqrt(1 - c^2), so a cosine carrying a few
    float32 roundings (norms, dot product, division: within 8 eps32 relative, |c| <= 1) moves the angle
    by at most 8 eps32 / sqrt(1 - c^2), plus 8 eps32 for acosf's own result; the clamp at +-(1 - 1e-5)
    keeps 1 - c^2 >= 2e-5, the floor of the square root.  NAAE divides the angle by |flow'| + 1e-9, and
    so its error.  (The reference's AAE cannot take a batch -- a [B,1,H,W] by [B,H,W] broadcast -- so its
    recorded case is sample 0 alone; test_error_maps_batch_vs_restatement covers AAE at B = 3.)"""
    import snnflow

    want_err, want_valid = g[f"met_{name}_err"], g[f"met_{name}_valid"]
    calls, nb = want_err.shape[:2]
    on = getattr(snnflow, name)(_cfg(metrics={"heat_map": True}), dev, flow_scaling=FS)
    off = getattr(snnflow, name)(_cfg(), dev, flow_scaling=FS)
    assert on.error_maps and not off.error_maps
    worst, avg_bound = 0.0, np.zeros((18, 16))
    for k in range(calls):
        _feed(on, g, k, dev, nb)
        _feed(off, g, k, dev, nb)
        r_on, r_off = on(), off()
        r_on, r_off = (r_on if isinstance(r_on, tuple) else (r_on,)), (r_off if isinstance(r_off, tuple) else (r_off,))
        for a, b in zip(r_on, r_off):
            assert_bit_equal(a.cpu().numpy(), b.cpu().numpy(), f"{name} values, flag on vs off")
        assert off.get_error_map() is None and off.get_final_error_heatmap() == (None, None)
        assert off.last_error_map() is None
        err = on.last_error_map()
        if name == "AAE":
            assert_bit_equal(on.get_error_map(), err.cpu().numpy(), "get_error_map")
        else:
            assert on.get_error_map() is None      # as in the reference, only AAE keeps a host-readable map
        err = err.cpu().numpy()
        assert err.shape == (nb, 18, 16)
        bound = vis_ref.error_map_bound(want_err[k], *_bound_args(g, k, nb, name))
        d = np.abs(err.astype(np.float64) - want_err[k])
        worst = max(worst, float((d / np.maximum(bound, 1e-300)).max()))
        assert (d <= bound).all(), (name, k, float((d / np.maximum(bound, 1e-300)).max()))
        avg_bound += (bound * want_valid[k]).sum(0)
        # the map and the metric agree: sum(err * mask) / sum(mask) per sample is the returned value
        v = want_valid[k].reshape(nb, -1)
        mean = (err.reshape(nb, -1).astype(np.float64) * v).sum(1) / (v.sum(1) + 1e-9)
        np.testing.assert_allclose(mean, r_on[0].cpu().numpy().astype(np.float64), rtol=1e-5)
        on.reset()
        off.reset()
    print(f"{name}: largest |error| / bound over {calls} calls = {worst:.3f}")
    avg, count = on.get_final_error_heatmap()      # reset() kept the aggregate
    assert not avg.is_cuda and not count.is_cuda
    assert_bit_equal(count.numpy(), g[f"met_{name}_count"], f"{name} count")
    d = np.abs(avg.numpy().astype(np.float64) - g[f"met_{name}_avg"])
    # the summed per-call bounds over the count, plus the float32 roundings of the sums and the division
    tol = avg_bound / (count.numpy() + 1e-9) + 8 * vis_ref.EPS32 * np.abs(g[f"met_{name}_avg"])
    assert (d <= tol).all(), (name, float((d / np.maximum(tol, 1e-300)).max()))
    on.reset_error_heatmap()
    assert on.get_final_error_heatmap() == (None, None)


@pytest.mark.parametrize("name", vis_ref.METRICS)
def test_error_maps_batch_vs_restatement(dev, name):
    """B = 3 at 37x53 (more than one block, a tail) with per-sample dt ratios, against the float64
    restatement under the same bound; the aggregate is the in-order float32 sum of the device's maps."""
    import snnflow

    rng = np.random.default_rng(9)
    B, H, W = 3, 37, 53
    flow = (rng.normal(0, 4, (B, 2, H, W)) / FS).astype(np.float32)
    gt = rng.normal(0, 4, (B, 2, H, W)).astype(np.float32)
    gt[:, :, rng.random((H, W)) < 0.2] = 0.0
    flow[:, :, 5, :9] = gt[:, :, 5, :9] / FS
    mask = (rng.random((B, 1, H, W)) < 0.6).astype(np.float32)
    dt_in, dt_gt = np.array([0.5, 0.25, 1.0], dtype=np.float32), np.array([1.0, 1.0, 0.5], dtype=np.float32)
    m = getattr(snnflow, name)({"loader": {"resolution": [H, W]}, "loss": {}}, dev, flow_scaling=FS)
    m.error_maps = True                            # switched by assignment
    z = torch.zeros(B, 1, 4, device=dev)
    for _ in range(3):
        m.event_flow_association([torch.from_numpy(flow).to(dev)],
                                 {"event_list": z, "event_list_pol_mask": z[:, :, :2], "gtflow": torch.from_numpy(gt).to(dev),
                                  "event_mask": torch.from_numpy(mask).to(dev), "dt_input": torch.from_numpy(dt_in),
                                  "dt_gt": torch.from_numpy(dt_gt)})
        m()
        m.reset()
    err = m.last_error_map().cpu().numpy()
    args = (flow, gt, mask[:, 0], dt_gt / dt_in, float(FS), name)
    # AEE is correctly rounded operations only: its reference is the float32 restatement (one ulp);
    # the angular metrics are held against float64
    ref, valid, _, _ = vis_ref.error_maps(*args, dtype=np.float32 if name == "AEE" else np.float64)
    bound = np.maximum(vis_ref.error_map_bound(ref, *args), 1e-300)
    d = np.abs(err.astype(np.float64) - ref)
    print(f"{name} B=3: largest |error| / bound = {float((d / bound).max()):.3f}")
    assert (d <= bound).all()
    avg, count = m.get_final_error_heatmap()
    assert_bit_equal(count.numpy(), (3 * valid.sum(0)).astype(np.float32), "count")
    s = np.zeros((H, W), dtype=np.float32)
    for b in range(B):
        s = s + err[b] * valid[b].astype(np.float32)
    acc = np.zeros((H, W), dtype=np.float32)
    for _ in range(3):
        acc = acc + s
    assert_bit_equal(avg.numpy(), (torch.from_numpy(acc) / (count + 1e-9)).numpy(), "aggregate")


@pytest.mark.parametrize("tag", ["avg", "ow"])
def test_window_images_vs_golden(g, dev, tag):
    import snnflow

    m = snnflow.AEE(_cfg(overwrite=tag == "ow"), dev, flow_scaling=FS)
    _feed(m, g, 0, dev, 2)
    _feed(m, g, 1, dev, 2)
    if tag == "ow":
        m.overwrite_intermediate_flow([torch.from_numpy(g["met_flow"][1]).to(dev)])
    assert_bit_equal(m.compute_window_events().cpu().numpy(), g[f"met_win_events_{tag}"], "window events")
    np.testing.assert_allclose(m.compute_masked_window_flow().cpu().numpy(), g[f"met_win_flow_{tag}"], rtol=1e-6)
