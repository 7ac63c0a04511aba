"""The evaluation and encoding kernels (csrc/eval.hip, csrc/encode.hip) at band, slice and batch edges
against the references of tests/eval_harness.py (test_eval_edges_cpu.py drives the same compare
functions with the fp32 oracle as "ours" and proves that the seeded cases reach these edges).

pol-IWE / deblur: two bands with a partial last one, corners of one event in two bands, warps that
leave the image, exactly one full band with N one past the block size, a wide image, N == 0 (zeros
written by the banded kernel itself) and the global-atomic kernel above 65536 events with B = 2; rounded
images equal to the exact sum, bilinear images within n_p 2^-23 S_p per pixel; the in-place stride-2
mask columns and two separate masks bit-identical when rounded.  AEE: two slices, B at its limit of 1024
and one past it, a scratch that grows and is reused, zero-gt rows and a fully masked sample.  All flow
metrics: 67 chunks and six samples (the finalize kernel's second chunk iteration and second sample round),
B at its limit of 256 and one past it; fp64 reference, rtol 2e-5 / atol 1e-6.  Encodings: a batch at a
ragged size, num_bins == 1 on a one-row image, N == 0, the grid-stride loop's second pass, events outside
the image dropped while their polarity mask is still written, ts exactly 0 and 1.

Each test prints its worst err / bound or worst relative error; DESIGN.md records them."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_harness as eh  # noqa: E402

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------
# pol-IWE / deblur
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", eh.POL_CASES, ids=eh.pol_id)
def test_pol_iwe_and_deblur_vs_exact_sum(dev, c):
    cid = eh.pol_id(c)
    d = eh.pol_data(c)
    for rnd in (True, False):
        for masks in eh.POL_MASKS:
            ref = eh.pol_reference(c, d, rnd, masks)
            ours = eh.pol_hip(c, d, dev, rnd, masks)
            eh.compare_scatter(f"{cid} {masks} round={int(rnd)}", ours, ref, exact=rnd)
            if c["shape"][3] == 0:
                assert not ours.any()
            if masks == "pol":
                # two separately allocated masks: the concatenation path
                sep = eh.pol_hip(c, d, dev, rnd, masks, separate=True)
                eh.compare_scatter(f"{cid} separate masks round={int(rnd)}", sep, ref, exact=rnd)
                if rnd:
                    assert ours.tobytes() == sep.tobytes()


# ---------------------------------------------------------------------------
# AEE
# ---------------------------------------------------------------------------
def _aee_check(tag, m, d, dts, dev):
    res = eh.aee_hip(m, d, dts, dev)
    eh.compare_metrics(tag, eh.aee_dict(res), eh.met_reference(d, dts), keys=("aee", "aee_pct"))
    again = m()
    assert torch.equal(again[0], res[0]) and torch.equal(again[1], res[1]), tag  # identical bits
    return res


@pytest.mark.parametrize("per_sample", [False, True], ids=["one_dt", "B_dts"])
def test_aee_two_slices(dev, per_sample):
    c = eh.MET_CASES["5x67x70"]
    B, H, W = c["shape"]
    d = eh.met_data(c)
    res = _aee_check(f"AEE 5x67x70 per-sample dt {per_sample}", eh.new_aee(dev, H, W), d, eh.met_dts(B, per_sample), dev)
    assert float(res[0][B - 1]) == 0.0  # the fully masked sample: 0 / (0 + 1e-9)


def test_aee_batch_limit(dev):
    from snnflow._lib import SnnflowError

    c = eh.MET_CASES["1024x3x3"]
    B, H, W = c["shape"]
    d = eh.met_data(c)
    m = eh.new_aee(dev, H, W)
    _aee_check("AEE 1024x3x3", m, d, eh.met_dts(B, True), dev)
    over = {k: torch.cat([v, v[:1]]) for k, v in d.items()}  # B = 1025
    with pytest.raises(SnnflowError):
        eh.aee_hip(m, over, eh.met_dts(B + 1, True), dev)
    _aee_check("AEE 1024x3x3 after the refused call", m, d, eh.met_dts(B, False), dev)


def test_aee_scratch_grows_and_is_reused(dev):
    small, large = eh.MET_CASES["2x20x24"], eh.MET_CASES["5x67x70"]
    ds, dl = eh.met_data(small), eh.met_data(large)
    m = eh.new_aee(dev, 20, 24)
    first = _aee_check("AEE scratch 2x20x24", m, ds, eh.met_dts(2, True), dev)
    n_small = next(iter(m._aee_acc.values())).numel()
    _aee_check("AEE scratch 5x67x70", m, dl, eh.met_dts(5, True), dev)
    n_large = next(iter(m._aee_acc.values())).numel()
    assert n_large > n_small and len(m._aee_acc) == 1
    third = _aee_check("AEE scratch 2x20x24 again", m, ds, eh.met_dts(2, True), dev)
    assert next(iter(m._aee_acc.values())).numel() == n_large  # reused, not shrunk
    assert torch.equal(first[0], third[0]) and torch.equal(first[1], third[1])


# ---------------------------------------------------------------------------
# all flow metrics
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["6x130x130", "256x2x2"])
def test_flow_metrics_vs_fp64(dev, name):
    from snnflow import _lib

    c = eh.MET_CASES[name]
    d = eh.met_data(c)
    dts = eh.met_dts(c["shape"][0], True)
    ours = eh.metrics_hip(d, dts, dev)
    assert sorted(ours) == sorted(_lib.METRICS)
    eh.compare_metrics(f"flow metrics {name}", ours, eh.met_reference(d, dts))
    again = eh.metrics_hip(d, dts, dev)
    assert all(ours[k].tobytes() == again[k].tobytes() for k in ours)  # fixed-order sums


def test_flow_metrics_batch_over_limit_raises(dev):
    from snnflow._lib import SnnflowError

    d = eh.met_data(eh.MET_CASES["256x2x2"])
    over = {k: torch.cat([v, v[:1]]) for k, v in d.items()}  # B = 257
    with pytest.raises(SnnflowError):
        eh.metrics_hip(over, eh.met_dts(257, True), dev)


# ---------------------------------------------------------------------------
# encodings
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", eh.ENC_CASES, ids=lambda c: c["id"])
def test_encodings_vs_exact_sum(dev, c):
    ev = eh.enc_data(c)
    for rnd in (False, True):
        ref = eh.enc_reference(c, ev, rnd)
        ours = eh.enc_hip_batch(c, ev, dev, rnd)
        eh.compare_enc(f"{c['id']} encode_batch round_ts={int(rnd)}", ours, ref, rnd)
        if c["N"] == 0:
            assert ours["pol"].shape == (c["B"], 0, 2) and not any(ours[k].any() for k in ("cnt", "voxel", "mask"))
        if c.get("single"):
            eh.compare_enc(f"{c['id']} single-sample functions round_ts={int(rnd)}",
                           eh.enc_hip_single(c, ev, dev, rnd), ref, rnd)


@pytest.mark.parametrize("c", [c for c in eh.ENC_CASES if c.get("single")], ids=lambda c: c["id"])
def test_events_to_image_vs_oracle(dev, c):
    """events_to_image accumulating (an exact integer sum) and assigning (values that are a function of
    the pixel: last-writer-wins is order-free), events outside the image dropped."""
    from oracle import encodings_ref
    from snnflow import encodings as E

    ev = eh.enc_data(c)
    res = (c["H"], c["W"])
    for b in range(c["B"]):
        xs, ys, ps_acc, ps_set, ins = eh.image_data(c, ev, b)
        for ps, acc in ((ps_acc, True), (ps_set, False)):
            eh.poison(dev, res)
            ours = E.events_to_image(*(torch.from_numpy(v).to(dev) for v in (xs, ys, ps)), res, accumulate=acc)
            ref = encodings_ref.events_to_image(*(torch.from_numpy(v[ins]) for v in (xs, ys, ps)), res, accumulate=acc)
            np.testing.assert_array_equal(ours.cpu().numpy(), ref.numpy(), err_msg=f"{c['id']} b={b} accumulate={acc}")
