"""CPU-side validation of the loss edge harness (tests/loss_harness.py; no GPU compute).

* The conditions on the committed seeds: the guard of the safe cases changes at most 5 % of a case's
  events and the fp32 corner set (oracle.iwe_ref.warp_corners_np, the kernels' operation order) equals the
  fp64 one for every remaining event; the exact cases' fp32 warped coordinates equal the fp64 ones bit for
  bit; with loss_scaling every sample's fp64 nz is > 0 in both directions.
* That every case reaches what it is there for (band and limit sizes, ties, landings, padding rows, ...).
* Reference against reference: the fp32 CPU oracle in the role of "ours" against the fp64 oracle, through
  the compare / limits / assert_case functions test_gpu_loss_edges.py uses -- the comparisons are passable,
  and the figures the limits rest on (loss_harness.REF_LOSS) are recomputed and checked.
* EventWarpingRef.terms() against __call__, and the C entry points' refusals (they return before any
  launch, so they run here on host buffers as well)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_harness as lh  # noqa: E402

from oracle import iwe_ref  # noqa: E402


@pytest.mark.parametrize("cid", lh.ALL_CASES)
def test_case_conditions(cid):
    case = lh.get_case(cid)
    assert case.changed <= lh.GUARD_CAP, (cid, case.changed)
    for i in range(case.nmaps):
        fevs = lh.event_flows(case, i)
        for k, (ev, pol, _) in enumerate(case.windows):
            if not ev.shape[1]:
                continue
            assert bool(((ev[:, :, 1] >= 0) & (ev[:, :, 1] < case.H) & (ev[:, :, 2] >= 0) & (ev[:, :, 2] < case.W)).all())
            live = (pol.numpy() != 0).any(2)
            evk = ev.numpy().copy()
            evk[:, :, 0] += np.float32(k)
            for tref in (case.T, 0):
                w32 = lh.warped(case, k, fevs[k], tref, np.float32)
                w64 = lh.warped(case, k, fevs[k], tref, np.float64)
                if case.exact:
                    for a, b in zip(w32, w64):
                        assert np.array_equal(a.astype(np.float64), b), (cid, k, tref)
                idx32, _, inb32 = iwe_ref.warp_corners_np(evk, fevs[k].numpy(), tref, [case.H, case.W], case.s)
                idx64, inb64 = lh.corners64(case, k, fevs[k], tref)
                live4 = np.concatenate([live] * 4, 1)
                assert np.array_equal(inb32[live4], inb64[live4]), (cid, k, tref)
                assert np.array_equal(idx32[live4], idx64[live4]), (cid, k, tref)
    want = lh.oracle64(cid)
    if case.loss_scaling and case.nmaps == 1:
        assert (want["persample"][:, :, 2] > 0).all(), (cid, want["persample"][:, :, 2])
    assert np.isfinite(want["loss"])
    print(f"\n[{cid}] guard changed {100 * case.changed:.2f} % of the events")


def _landings(case, tref):
    fevs = lh.event_flows(case)
    k = case.T - 1
    wy, wx = lh.warped(case, k, fevs[k], tref, np.float64)
    return wy, wx


def test_cases_reach_their_edges():
    from snnflow import _lib

    g = lh.get_case
    assert g("band-w1").H * g("band-w1").W == 1024 and g("band-w1").exact and g("band-w1").s == 64
    r = g("ragged-uneven-w1")
    assert r.H * r.W == 1024 + 57 == 512 + 512 + 57 and 1024 % r.W != 0 and 512 % r.W != 0
    assert [w[0].shape[1] for w in r.windows] == [300, 0, 2100] and 2100 > 2048
    assert float(r.windows[1][2].abs().max()) == 0.0
    assert len({w[0].shape[1] for w in g("ragged-equal-w1").windows}) == 1
    assert g("batch17-w1").B == 17 and g("batch64-w1").B == 64 and g("batch64-w1").T == 1 and g("tiny-w1").T == 1
    w = g("windows-w1")
    assert w.T == _lib.MAX_WINDOWS == 64 and g("windows-overwrite-w1").overwrite
    base = w.B * ((w.H * w.W + 255) // 256)
    assert (1024 + base - 1) // base == 61  # loss_tsplit(1, 64 * 68, 64): uneven groups of one and two windows
    for cid, W_, recs in (("wide1791-w1", 1791, 5), ("wide600-w1", 600, 3)):
        assert g(cid).W == W_ and (2 * W_ + 2) // 1024 + 2 == recs
    assert 3 * (512 + 2 * 1791 + 2) * 4 == 48 * 1024  # the backward's dynamic LDS at the W limit
    n = g("none-w1")
    assert all(w[0].shape[1] == 0 for w in n.windows) and not n.loss_scaling
    # exact cases: flow == 0 everywhere; landings exactly on H - 1, H, -1 (rows) and W - 1, W, -1 (columns)
    assert all(float(f[0].abs().max()) == 0.0 for f in g("ties-band-zero").flows)
    for cid in ("ties-band-sparse", "ties-band-dense", "ties-tiny-sparse", "ties-tiny-dense", "band-w1"):
        c = g(cid)
        wy, wx = _landings(c, c.T)
        for v in (c.H - 1, c.H, -1):
            assert (wy == v).any(), (cid, "row", v)
        for v in (c.W - 1, c.W, -1):
            assert (wx == v).any(), (cid, "column", v)
        ts = torch.cat([w[0][:, :, 0].flatten() for w in c.windows])
        assert bool((ts == 0).any()) and bool((ts == 1).any()) and bool((ts * 8 == (ts * 8).round()).all())
        half = np.concatenate([(2 * a) % 2 for a in _landings(c, 0)])
        assert (half == 1).any() and (half == 0).any()  # half-integer and integer displacements
    assert g("ties-tiny-sparse").windows[0][0].shape[1] == 9
    # event contents
    p = g("content-padding")
    for ev, pol, _ in p.windows:
        npad = int(round(0.3 * ev.shape[1]))
        if npad:
            assert float(ev[:, -npad:].abs().max()) == 0.0 and float(pol[:, -npad:].abs().max()) == 0.0
    c = g("content-patch")
    for ev, _, _ in c.windows:
        if ev.shape[1]:
            assert len(torch.unique(ev[:, :, 1] * c.W + ev[:, :, 2])) <= 9
    c = g("content-far")
    far = max(float(np.abs(lh.warped(c, k, f, tref, np.float64)[1] - c.windows[k][0][:, :, 2].numpy()).max())
              for k, f in enumerate(lh.event_flows(c)) if f.shape[1] for tref in (c.T, 0))
    assert far >= 0.9 * 2 * c.W, far
    c = g("content-border")
    ys = torch.cat([w[0][:, :, 1].flatten() for w in c.windows])
    xs = torch.cat([w[0][:, :, 2].flatten() for w in c.windows])
    for y, x in ((0, 0), (0, c.W - 1), (c.H - 1, 0), (c.H - 1, c.W - 1)):
        assert bool(((ys == y) & (xs == x)).any())
    out = set()
    for k, f in enumerate(lh.event_flows(c)):
        if not f.shape[1]:
            continue
        for tref in (c.T, 0):
            wy, wx = lh.warped(c, k, f, tref, np.float64)
            out |= {s for s, m in (("top", wy < -1), ("bottom", wy > c.H), ("left", wx < -1), ("right", wx > c.W)) if m.any()}
    assert out == {"top", "bottom", "left", "right"}, out


@pytest.mark.parametrize("cid", lh.ALL_CASES)
def test_fp32_oracle_vs_fp64(cid):
    """The fp32 oracle as "ours" through the GPU file's comparisons; its figures against REF_LOSS: each
    within a factor 2 of the committed one, or both below one fp32 rounding of the quantity's magnitude."""
    case = lh.get_case(cid)
    fig, r = lh.ref_figures(cid)
    lh.compare(case, lh.run_oracle(case, torch.float32), lh.oracle64(cid), tag="cpu32")
    ref = lh.REF_LOSS[cid]
    assert set(ref) == set(fig), cid
    for q, v in fig.items():
        floor = lh.EPS32 * (r["mag"][q] if q in r["mag"] else 1.0)
        assert abs(v - ref[q]) <= max(ref[q], floor), (cid, q, v, ref[q])
    lh.assert_case(case, r, lh.limits(cid, r["mag"], lh.ref_wide(cid)))


def test_terms_are_what_call_computes():
    case = lh.get_case("ragged-equal-w1")
    ref = iwe_ref.EventWarpingRef([case.H, case.W], weight=case.weight)
    for (ev, pol, mask), maps in zip(case.windows, case.flows):
        ref.event_flow_association(maps, ev, pol, mask)
    t = ref.terms()
    assert float(t["loss"]) == float(ref())
    B, HW = case.B, case.H * case.W
    assert tuple(t["images"].shape) == (2, 4, B, HW) and tuple(t["persample"].shape) == (2, B, 4)
    for d in range(2):
        cp, cn, tp, tn = t["images"][d]
        sp = ((tp / (cp + 1e-9) / case.T) ** 2).sum(1)
        assert torch.equal(sp, t["persample"][d, :, 0])
        assert torch.equal(((cp + cn) > 0).float().sum(1), t["persample"][d, :, 2])
        assert torch.equal((t["persample"][d, :, 0] + t["persample"][d, :, 1]) / t["persample"][d, :, 2],
                           t["persample"][d, :, 3])
    loss = t["persample"][:, :, 3].sum() + case.weight * (t["smooth"].sum() / 5 / case.T)
    np.testing.assert_allclose(float(loss), float(t["loss"]), rtol=1e-6)


def test_entry_points_refuse_before_any_launch():
    assert lh.assert_refusals("cpu") == 9
