"""The contrast-maximisation landscape (snnflow.contrast, csrc/landscape.hip) on the GPU: against the
reference's heatmaps (tests/golden/landscape_case.npz), the known answer, bit-reproducibility and candidate
independence, the existing HIP loss on constant flow maps at a ragged shape, and masked / empty input."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL = 2e-5   # the loss against its golden value (tests/test_gpu_parity.py)


@pytest.fixture(scope="module")
def g(golden):
    return golden("landscape_case.npz")


@pytest.fixture(scope="module", autouse=True)
def no_device_faults(dev):
    import snnflow

    snnflow.check_device_errors()
    yield
    snnflow.check_device_errors()


def case_inputs(g, case, dev):
    H, W, maxdisp, R, weight, mask_output = g[f"{case}_meta"]
    cfg = {"loader": {"resolution": [int(H), int(W)]}, "loss": {"flow_regul_weight": float(weight)},
           "model": {"mask_output": bool(mask_output)}}
    ev, pol, mask = (torch.from_numpy(g[f"{case}_{k}"]).to(dev) for k in ("events", "pol", "mask"))
    return ev, pol, mask, cfg, float(maxdisp), int(R)


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("case", ("a", "b"))
def test_heatmap_matches_reference(g, dev, case):
    import snnflow

    ev, pol, mask, cfg, maxdisp, R = case_inputs(g, case, dev)
    heat = snnflow.flow_heatmap(ev, pol, mask, cfg, maxdisp, maxdisp, R)
    assert heat.shape == (R, R) and heat.device.type == "cuda" and heat.dtype == torch.float32
    want = g[f"{case}_heatmap"]
    got = heat.cpu().numpy()
    print(case, "max relative deviation", np.abs(got / want - 1).max())
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=0)


def test_known_answer(g, dev):
    import snnflow
    from snnflow.iwe import compute_pol_iwe

    ev, pol, mask, cfg, maxdisp, R = case_inputs(g, "b", dev)
    flow, loss, iwe = snnflow.best_global_flow(ev, pol, mask, cfg, maxdisp, maxdisp, R)
    H, W = cfg["loader"]["resolution"]
    assert flow.shape == (1, 2) and loss.shape == (1,) and iwe.shape == (1, 2, H, W)
    assert flow.cpu().tolist() == [[6.0, -4.0]]                  # (u, v): the true motion of the fixture
    assert loss.item() == pytest.approx(float(g["b_heatmap"].min()), rel=RTOL)
    const = torch.ones(1, 2, H, W, device=dev)
    const[:, 0] *= 6.0
    const[:, 1] *= -4.0
    want = compute_pol_iwe(const, ev, (H, W), pol[:, :, 0:1], pol[:, :, 1:2], flow_scaling=1, round_idx=True)
    assert torch.equal(iwe, want)
    assert iwe.sum().item() > 0
    # NaN counts as +inf and ties go to the lowest flat index: with every event masked out the whole
    # landscape is NaN and the first candidate wins
    flow0, loss0, iwe0 = snnflow.best_global_flow(ev, torch.zeros_like(pol), mask, cfg, maxdisp, maxdisp, R)
    assert flow0.cpu().tolist() == [[-maxdisp, -maxdisp]] and torch.isnan(loss0).all() and not iwe0.any()


def test_deterministic_and_candidate_independent(g, dev):
    import snnflow

    ev, pol, _, cfg, _, _ = case_inputs(g, "b", dev)
    res = cfg["loader"]["resolution"]
    cand = torch.from_numpy(g["b_cand"]).to(dev)
    first = bits(snnflow.loss_landscape(ev, pol, res, cand))
    assert first.shape == (1, 81)
    assert (bits(snnflow.loss_landscape(ev, pol, res, cand)) == first).all()
    assert (bits(snnflow.loss_landscape(ev, pol, res, cand.flip(0)))[:, ::-1] == first).all()
    single = torch.cat([snnflow.loss_landscape(ev, pol, res, cand[k:k + 1]) for k in range(81)], dim=1)
    assert (bits(single) == first).all()
    assert (bits(snnflow.loss_landscape(ev, pol, res, g["b_cand"])) == first).all()      # a numpy array


@pytest.fixture(scope="module")
def ragged(dev):
    """37 x 53 (two bands), B = 2, N = 1001 uniform events; timestamps 0 and 1 present."""
    gen = torch.Generator().manual_seed(5)
    B, N, H, W = 2, 1001, 37, 53
    ts = torch.sort(torch.rand(B, N, generator=gen), dim=1).values
    ts = (ts - ts[:, :1]) / (ts[:, -1:] - ts[:, :1])
    ys = torch.randint(0, H, (B, N), generator=gen).float()
    xs = torch.randint(0, W, (B, N), generator=gen).float()
    ps = torch.randint(0, 2, (B, N), generator=gen).float() * 2 - 1
    ev = torch.stack([ts, ys, xs, ps], dim=2).to(dev)
    pol = torch.stack([(ps > 0).float(), (ps < 0).float()], dim=2).to(dev)
    # the last one: a large vertical flow (every row group can reach every band)
    cand = torch.tensor([[0, 0], [2.5, -1.25], [-2.5, 1.25], [7, 0], [0, -7], [1000, 1000], [-3, 64]], dtype=torch.float32)
    return ev, pol, cand.to(dev), (H, W)


def test_matches_the_loss_on_constant_maps(ragged, dev):
    import snnflow

    ev, pol, cand, (H, W) = ragged
    got = snnflow.loss_landscape(ev, pol, (H, W), cand).cpu().numpy()
    cfg = {"loader": {"resolution": [H, W]}, "loss": {"flow_regul_weight": 0.0}, "model": {"mask_output": False}}
    loss_fn = snnflow.EventWarping(cfg, dev, flow_scaling=1)
    want = np.zeros_like(got)
    for b in range(ev.shape[0]):
        mask = torch.zeros(1, 1, H, W, device=dev)
        for k, (u, v) in enumerate(cand.cpu().tolist()):
            flow = torch.ones(1, 2, H, W, device=dev)
            flow[:, 0] *= u
            flow[:, 1] *= v
            loss_fn.event_flow_association([flow], ev[b:b + 1], pol[b:b + 1], mask)
            want[b, k] = loss_fn().item()
            loss_fn.reset()
    print("max relative deviation", np.abs(got / want - 1).max())
    assert np.isfinite(want).all()
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=0)


def test_masked_and_empty_input(g, ragged, dev):
    import snnflow

    ev, pol, cand, res = ragged
    full = snnflow.loss_landscape(ev, pol, res, cand)
    assert torch.isfinite(full).all()
    pol0 = pol.clone()
    pol0[1] = 0
    out = snnflow.loss_landscape(ev, pol0, res, cand)
    assert torch.isnan(out[1]).all()
    assert (bits(out[0]) == bits(full[0])).all()
    # padding: 37 events of pol = 0 appended to case a
    ev_a, pol_a, _, cfg, _, _ = case_inputs(g, "a", dev)
    cand_a = torch.from_numpy(g["a_cand"]).to(dev)
    base = snnflow.loss_landscape(ev_a, pol_a, cfg["loader"]["resolution"], cand_a)
    pad_ev = torch.zeros(2, 37, 4, device=dev)
    pad_ev[:, :, 0] = 0.5
    pad_pol = torch.zeros(2, 37, 2, device=dev)
    padded = snnflow.loss_landscape(torch.cat([ev_a, pad_ev], dim=1), torch.cat([pol_a, pad_pol], dim=1),
                                    cfg["loader"]["resolution"], cand_a)
    assert (bits(padded) == bits(base)).all()
    # loss_scaling off: the unscaled sums (an empty sample then gives 0, not NaN)
    raw = snnflow.loss_landscape(ev, pol0, res, cand, loss_scaling=False)
    assert (raw[1] == 0).all() and (raw[0] >= full[0]).all() and (raw[0, 0] > full[0, 0]).all()
