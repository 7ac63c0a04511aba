"""On-device batch preparation (snnflow.BatchPreparer -> snnflow_loader_prepare) against the
reference loader's recorded outputs (tests/golden/loader_case.npz) and the numpy restatement
(tests/loader_ref.py).  Everything is compared bit for bit except a voxel grid built from generic
timestamps, whose sums follow the atomic arrival order: there the bound is the worst-case
difference between two fp32 summation orders of the same terms (loader_ref.voxel_bound)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loader_ref  # noqa: E402
from loader_ref import CASES, MECH, TENSORS, assert_bit_equal, case_inputs, config  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g(golden):
    return golden("loader_case.npz")


def set_flags(prep, flags):
    for i, m in enumerate(MECH):
        prep.batch_augmentation[m] = [bool(f[i]) for f in flags]


def to_dev(dev, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def run(prep, dev, xs, ys, ts, ps, counts=None, gt=None):
    out = prep.prepare(*to_dev(dev, xs, ys, ts, ps), *to_dev(dev, None if counts is None else counts.astype(np.int32), gt))
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_voxel_bound(got, ref, what):
    err = np.abs(got.astype(np.float64) - ref["event_voxel"].astype(np.float64))
    bound = loader_ref.voxel_bound(ref)
    print(f"{what}: max voxel error {err.max():.3e}, smallest slack {np.min(bound - err):.3e}")
    assert (err <= bound).all(), (what, float(err.max()))


@pytest.mark.parametrize("case", ["A", "Bk", "Bp"])
def test_fixture_cases_bitwise(g, dev, case):
    import snnflow

    _, mode, pooled, keep = CASES[case]
    xs, ys, ts, ps, counts, gt = case_inputs(g, case)
    prep = snnflow.BatchPreparer(config(g, mode, pooled, 3, keep=keep), int(g["num_bins"]), device=dev)
    set_flags(prep, g[f"{case}_flags"])
    out = run(prep, dev, xs, ys, ts, ps, counts, gt)
    assert set(out) == set(TENSORS) | ({"gtflow"} if gt is not None else set())
    for k in out:
        assert_bit_equal(out[k], g[f"{case}_{k}"], f"{case} {k}")


def test_fixture_hot_filter_sequence_bitwise(g, dev):
    import snnflow

    T, B = g["C_xs"].shape[:2]
    prep = snnflow.BatchPreparer(config(g, "gtflow_dt1", True, B, keep=True, hot=True), int(g["num_bins"]), device=dev)
    assert prep.hot_events.shape == (B, 18, 16) and prep.hot_idx.dtype == torch.int32
    for t in range(T):
        if t == int(g["C_reset_before"]):
            prep.reset_sequence(int(g["C_reset_slot"]))
        set_flags(prep, g["C_flags"][t])
        out = run(prep, dev, g["C_xs"][t], g["C_ys"][t], g["C_ts"][t], g["C_ps"][t], g["C_counts"][t])
        for k in TENSORS:
            assert_bit_equal(out[k], g[f"C_{k}"][t], f"C window {t} {k}")
        assert_bit_equal(prep.hot_events.cpu().numpy(), g["C_hot_events"][t], f"C window {t} hot_events")
        assert (prep.hot_idx.cpu().numpy() == g["C_hot_idx"][t]).all(), t


def test_fixture_generic_timestamps(g, dev):
    import snnflow

    xs, ys, ts, ps, counts, _ = case_inputs(g, "D")
    prep = snnflow.BatchPreparer(config(g, "events", False, 3), int(g["num_bins"]), device=dev)
    set_flags(prep, g["D_flags"])
    out = run(prep, dev, xs, ys, ts, ps, counts)
    for k in TENSORS:
        if k != "event_voxel":
            assert_bit_equal(out[k], g[f"D_{k}"], f"D {k}")
    ref = loader_ref.RefPreparer(config(g, "events", False, 3), int(g["num_bins"]), flags=g["D_flags"])
    r = ref.prepare(xs, ys, ts, ps, counts)
    r["event_voxel"] = g["D_event_voxel"]  # the reference's own sums; K and S from the restatement
    check_voxel_bound(out["event_voxel"], r, "D")


def _big_config(hot=True, keep=False):
    return {"data": {"mode": "gtflow_dt1"},
            "loader": {"resolution": [32, 32], "std_resolution": [64, 64], "batch_size": 4, "augment": list(MECH),
                       "augment_prob": [0.5, 0.5, 0.5], "keep_gt_full_res": keep},
            "hot_filter": {"enabled": hot, "max_px": 100, "min_obvs": 2, "max_rate": 0.5}}


def _big_windows(T=7, B=4, N=3000, H=64, W=64):
    """About 200 busy pixels, each firing in a window with its own probability (many distinct and
    many equal rates, more than max_px of them above max_rate), plus a uniform background."""
    rng = np.random.default_rng(5)
    busy = rng.choice(H * W, 200, replace=False)
    prob = rng.choice([0.45, 0.6, 0.75, 0.9, 1.0], 200)
    wins = []
    for _ in range(T):
        pix = np.empty((B, N), np.int64)
        for b in range(B):
            on = busy[rng.random(200) < prob]
            pix[b] = np.where(rng.random(N) < 0.85, rng.choice(on, N), rng.integers(0, H * W, N))
        ts = np.sort(3.0 + 0.02 * rng.random((B, N)), axis=1)
        wins.append(((pix % W).astype(np.int16), (pix // W).astype(np.int16), ts,
                     rng.integers(0, 2, (B, N)).astype(np.int8), rng.standard_normal((B, 2, H, W)).astype(np.float32)))
    return wins


def test_larger_random_case_against_restatement(dev):
    """Multi-block min/max (N > 2048), contended scatter, a selection that cuts inside a run of
    equal rates on 4096 pixels, a short slot and an empty one, pooled mask and gtflow."""
    import snnflow

    cfg = _big_config()
    counts = np.array([3000, 2999, 64, 0], np.int32)
    flags = np.array([[0, 0, 0], [1, 0, 1], [0, 1, 0], [1, 1, 1]], bool)
    prep = snnflow.BatchPreparer(cfg, 5, device=dev)
    ref = loader_ref.RefPreparer(cfg, 5, flags=flags)
    set_flags(prep, flags)
    cut = 0
    for t, (xs, ys, ts, ps, gt) in enumerate(_big_windows()):
        out = run(prep, dev, xs, ys, ts, ps, counts, gt)
        r = ref.prepare(xs, ys, ts, ps, counts, gt)
        for k in ("event_cnt", "event_mask", "event_list", "event_list_pol_mask", "gtflow"):
            assert_bit_equal(out[k], r[k], f"window {t} {k}")
        check_voxel_bound(out["event_voxel"], r, f"window {t}")  # 2x2 window: the division by 4 is exact
        assert_bit_equal(prep.hot_events.cpu().numpy(), ref.hot_events, f"window {t} hot_events")
        assert (prep.hot_idx.cpu().numpy() == ref.hot_idx).all()
        if ref.hot_idx[0] > 2:
            rate = ref.hot_events[0] / np.float32(ref.hot_idx[0])
            c = np.sort(rate[rate > np.float32(0.5)])[::-1]
            cut += int(len(c) > 100 and c[99] == c[100])
    assert cut > 0, "no window cut inside a run of equal rates"
    assert not out["event_cnt"][3].any() and not out["event_list"][3].any() and (ref.hot_idx == 7).all()


def test_unpooled_hot_filter_rounding_and_gtflow(dev):
    """The paths the fixture does not take: hot filter without pooling (in-place multiply),
    round_encoding (0 / 1 voxel weights: exact sums, so bit-equal), gtflow at full resolution."""
    import snnflow

    cfg = {"data": {"mode": "events"},
           "loader": {"resolution": [18, 16], "std_resolution": [18, 16], "batch_size": 2, "augment": list(MECH),
                      "augment_prob": [0.5, 0.5, 0.5]},
           "hot_filter": {"enabled": True, "max_px": 2, "min_obvs": 1, "max_rate": 0.6}}
    flags = np.array([[1, 1, 0], [0, 0, 1]], bool)
    prep = snnflow.BatchPreparer(cfg, 4, round_encoding=True, device=dev)
    ref = loader_ref.RefPreparer(cfg, 4, round_encoding=True, flags=flags)
    set_flags(prep, flags)
    rng = np.random.default_rng(11)
    busy = rng.choice(18 * 16, 6, replace=False)
    for t in range(4):
        pix = np.where(rng.random((2, 77)) < 0.5, rng.choice(busy, (2, 77)), rng.integers(0, 18 * 16, (2, 77)))
        xs, ys = (pix % 16).astype(np.int16), (pix // 16).astype(np.int16)
        ts = np.sort(rng.random((2, 77)), axis=1)
        ps = rng.integers(0, 2, (2, 77)).astype(np.int8)
        gt = rng.standard_normal((2, 2, 18, 16)).astype(np.float32)
        out = run(prep, dev, xs, ys, ts, ps, None, gt)
        r = ref.prepare(xs, ys, ts, ps, None, gt)
        for k in out:
            assert_bit_equal(out[k], r[k], f"window {t} {k}")
        assert_bit_equal(prep.hot_events.cpu().numpy(), ref.hot_events, f"window {t} hot_events")
    assert ref.hot_idx[0] == 4 and (ref.hot_events[0] == 4).sum() > 2  # more always-on pixels than max_px: a tie at the cut


def test_graph_capture_matches_eager(dev):
    """prepare() captured on one stream and replayed three times (new inputs copied into the static
    tensors, state carried on the device) equals three eager calls on a twin object."""
    import snnflow

    cfg = _big_config()
    rng = np.random.default_rng(6)
    wins = []
    for xs, ys, _, ps, gt in _big_windows(T=4, N=600):
        # integer timestamps spanning 64 over each slot's valid events: every voxel term is dyadic, so
        # the sums do not depend on the atomic arrival order and the whole dict can be compared exactly
        k = np.sort(rng.integers(0, 65, (4, 600)), axis=1).astype(np.float64)
        k[:, 0], k[0, 599], k[1, 598], k[2, 63] = 0, 64, 64, 64
        wins.append((xs, ys, 7.0 + k, ps, gt))
    flags = np.array([[0, 1, 0], [1, 0, 1], [0, 0, 0], [1, 1, 0]], bool)
    twin = snnflow.BatchPreparer(cfg, 3, device=dev)
    prep = snnflow.BatchPreparer(cfg, 3, device=dev)
    set_flags(twin, flags)
    set_flags(prep, flags)
    counts = torch.tensor([600, 599, 64, 0], dtype=torch.int32, device=dev)
    static = [a.float() for a in to_dev(dev, *wins[3])]
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):  # warm-up: scratch and flag upload happen outside the capture
        prep.prepare(*static[:4], counts, static[4])
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    prep.hot_events.zero_()
    prep.hot_idx.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = prep.prepare(*static[:4], counts, static[4])
    for t in range(3):
        new = [a.float() for a in to_dev(dev, *wins[t])]
        for s, n in zip(static, new):
            s.copy_(n)
        graph.replay()
        want = twin.prepare(*new[:4], counts, new[4])
        torch.cuda.synchronize(dev)
        for k in want:
            assert torch.equal(out[k], want[k]), (t, k)
        assert torch.equal(prep.hot_events, twin.hot_events) and torch.equal(prep.hot_idx, twin.hot_idx), t
    assert prep.hot_idx.tolist() == [3, 3, 3, 3]


def _loss_cfg(H, W):
    return {"loader": {"resolution": [H, W]}, "loss": {"flow_regul_weight": 0.001, "overwrite_intermediate": False},
            "model": {"mask_output": True}}


def _dyadic_events(rng, B, N, H, W, counts=None):
    """Integer timestamps spanning 64 over each slot's valid events: exact voxel sums in any order."""
    k = np.sort(rng.integers(0, 65, (B, N)), axis=1).astype(np.float64)
    k[:, 0] = 0
    for b in range(B):
        k[b, (N if counts is None else counts[b]) - 1] = 64
    return (rng.integers(0, W, (B, N)).astype(np.int16), rng.integers(0, H, (B, N)).astype(np.int16), 50.0 + k,
            rng.integers(0, 2, (B, N)).astype(np.int8))


def test_end_to_end_train_step_events_mode(dev):
    """Prepared batches (16x16, flips on) through LIFFireNet + EventWarping forward and backward:
    the loss equals, bit for bit, the run fed by the restatement's tensors (dyadic timestamps, so
    the voxel grid is exact too)."""
    import snnflow
    from oracle import lif_ref

    B, N, H, W = 2, 96, 16, 16
    cfg = {"data": {"mode": "events"},
           "loader": {"resolution": [H, W], "std_resolution": [H, W], "batch_size": B, "augment": list(MECH),
                      "augment_prob": [0.5, 0.5, 0.5]}, "hot_filter": {"enabled": False}}
    flags = np.array([[1, 0, 1], [0, 1, 0]], bool)
    rng = np.random.default_rng(3)
    counts = np.array([N, N - 30], np.int32)
    windows = [_dyadic_events(rng, B, N, H, W, counts) for _ in range(2)]
    prep = snnflow.BatchPreparer(cfg, 2, device=dev)
    set_flags(prep, flags)
    ref = loader_ref.RefPreparer(cfg, 2, flags=flags)

    def train_step(batches):
        torch.manual_seed(0)
        model = snnflow.LIFFireNet(dict(lif_ref.make_unet_kwargs(base_num_channels=8))).to(dev).train()
        loss_fn = snnflow.EventWarping(_loss_cfg(H, W), dev)
        for w in batches:
            flow = model(w["event_voxel"], w["event_cnt"])["flow"]
            loss_fn.event_flow_association(flow, w["event_list"], w["event_list_pol_mask"], w["event_mask"])
        loss = loss_fn()
        loss.backward()
        torch.cuda.synchronize(dev)
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
        return loss.item()

    ours = [prep.prepare(*to_dev(dev, *w), *to_dev(dev, counts)) for w in windows]
    theirs = [{k: torch.from_numpy(v).to(dev) for k, v in ref.prepare(*w, counts).items() if k in TENSORS}
              for w in windows]
    for o, r in zip(ours, theirs):
        for k in TENSORS:
            assert torch.equal(o[k], r[k]), k
    a, b = train_step(ours), train_step(theirs)
    assert np.isfinite(a) and a == b, (a, b)


def test_end_to_end_eval_pooled_full_res_gt(dev):
    """Pooled mode with keep_gt_full_res: the model runs at 16x16, its last flow is upsampled
    (snnflow.iwe.upsample_flow) to the 32x32 gtflow and mask of the prepared batch; AEE equals
    the same computation on the restatement's tensors."""
    import snnflow
    from oracle import lif_ref
    from snnflow.iwe import upsample_flow

    B, N = 2, 128
    cfg = {"data": {"mode": "gtflow_dt1"},
           "loader": {"resolution": [16, 16], "std_resolution": [32, 32], "batch_size": B, "augment": list(MECH),
                      "augment_prob": [0.5, 0.5, 0.5], "keep_gt_full_res": True},
           "hot_filter": {"enabled": True, "max_px": 4, "min_obvs": 0, "max_rate": 0.5}}
    flags = np.array([[0, 1, 0], [1, 0, 0]], bool)
    rng = np.random.default_rng(4)
    xs, ys, ts, ps = _dyadic_events(rng, B, N, 32, 32)
    gt = rng.standard_normal((B, 2, 32, 32)).astype(np.float32)
    prep = snnflow.BatchPreparer(cfg, 2, device=dev)
    set_flags(prep, flags)
    ref = loader_ref.RefPreparer(cfg, 2, flags=flags)
    ours = prep.prepare(*to_dev(dev, xs, ys, ts, ps), None, *to_dev(dev, gt))
    theirs = {k: torch.from_numpy(v).to(dev) for k, v in ref.prepare(xs, ys, ts, ps, None, gt).items()}
    assert ours["event_mask"].shape == (B, 1, 32, 32) and ours["gtflow"].shape == (B, 2, 32, 32)
    assert ours["event_cnt"].shape == (B, 2, 16, 16)

    def aee(batch):
        torch.manual_seed(0)
        model = snnflow.LIFFireNet(dict(lif_ref.make_unet_kwargs(base_num_channels=8))).to(dev).eval()
        with torch.no_grad():
            flow = model(batch["event_voxel"], batch["event_cnt"])["flow"][-1]
        m = snnflow.AEE(_loss_cfg(32, 32), dev, flow_scaling=128)
        one = torch.ones(1)
        m.event_flow_association([upsample_flow(flow, 32, 32)], {
            "event_list": batch["event_list"], "event_list_pol_mask": batch["event_list_pol_mask"],
            "event_mask": batch["event_mask"], "gtflow": batch["gtflow"], "dt_input": one, "dt_gt": one})
        val, pct = m()
        return val.cpu().numpy(), pct.cpu().numpy()

    (a, ap), (b, bp) = aee(ours), aee(theirs)
    assert np.isfinite(a).all() and (a > 0).all()
    assert (a == b).all() and (ap == bp).all(), (a, b)
