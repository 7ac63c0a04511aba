"""tests/eval_harness.py without a GPU: the fp32 CPU oracle in the role of "ours" through the compare
functions test_gpu_eval_edges.py uses (so the harness is known to be able to pass: the references, the
derived bound n_p 2^-23 S_p and the metric tolerances are met by a second, independent fp32
implementation), and the conditions on the seeded inputs, asserted on the references alone: the cases
reach the band crossings, the out-of-image share, the threshold distances and the timestamps 0 and 1
their names promise, and the kernel paths restated from the host code."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_harness as eh  # noqa: E402


# ---------------------------------------------------------------------------
# pol-IWE / deblur
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", eh.POL_CASES, ids=eh.pol_id)
def test_pol_iwe_oracle32_within_bound(c):
    d = eh.pol_data(c)
    for masks in eh.POL_MASKS:
        for rnd in (True, False):
            ref = eh.pol_reference(c, d, rnd, masks)
            ours = eh.pol_oracle32(c, d, rnd, masks)
            eh.compare_scatter(f"{eh.pol_id(c)} {masks} round={int(rnd)} (fp32 oracle)", ours, ref, exact=rnd)


@pytest.mark.parametrize("c", eh.POL_CASES, ids=eh.pol_id)
def test_pol_iwe_cases_reach_their_edges(c):
    B, H, W, N = c["shape"]
    d = eh.pol_data(c)
    s = eh.pol_stats(c, d)
    print(f"[eval-edges] {eh.pol_id(c)}: {s}, path {eh.pol_path(c)}")
    names = c["names"]
    # events inside the image at exactly representable pixel indices: the flow gather stays in bounds
    assert (d["ev"][:, :, 1] >= 0).all() and (d["ev"][:, :, 1] <= H - 1).all()
    assert (d["ev"][:, :, 2] >= 0).all() and (d["ev"][:, :, 2] < W).all()
    assert eh.pol_path(c) == ("global" if "global_atomics" in names else "band")
    if "two_bands" in names:
        assert s["bands"] == 2 and 0 < s["last_band"] < eh.POLB_BAND
    if "one_full_band" in names:
        assert s["bands"] == 1 and s["last_band"] == eh.POLB_BAND and N == 1025
    if "wide" in names:
        assert s["bands"] == 2 and W > 2 * 32 and H < 32  # the +-32-pixel warps leave the image vertically
    if "band_crossing" in names:
        assert s["crossing"] >= 1
    if "out_of_image" in names:
        assert 0.10 <= s["outside"] <= 0.80
    if "no_events" in names:
        assert N == 0 and B > 1
    if "global_atomics" in names:
        assert N > eh.POL_BANDED_MAX_N and B > 1
    if N:  # both polarities, and column fractions, so truncating differs from rounding the gather index
        assert d["pol"][:, :, 0].any() and d["pol"][:, :, 1].any()
        assert (d["ev"][:, :, 2] % 1 == 0.5).any()


# ---------------------------------------------------------------------------
# flow metrics and AEE
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(eh.MET_CASES))
def test_metric_seeds_keep_their_distance_from_thresholds(name):
    c = eh.MET_CASES[name]
    B, H, W = c["shape"]
    d = eh.met_data(c)
    for per_sample in (False, True):
        dts = eh.met_dts(B, per_sample)
        m = eh.threshold_margin(d, dts)
        print(f"[eval-edges] {name} per-sample dt {per_sample}: threshold margin {m:.3g}")
        assert m > eh.MARGIN
        a = eh.angle_margin(c, d, dts)
        print(f"[eval-edges] {name} per-sample dt {per_sample}: angle margin {a:.3g}")
        assert a > eh.ANGLE_MARGIN
    t = eh.flow_metrics_terms(d["flow"], d["gt"], d["mask"], *eh.met_dts(B, True), eh.FLOW_SCALING, dtype=torch.float64)
    nv = t["m"].sum(1)
    assert bool((nv > 0).any())
    if B > 1:
        assert float(nv[B - 1]) == 0.0  # a fully masked sample
    assert bool(((d["gt"][:, 0] == 0) & (d["gt"][:, 1] == 0) & (d["mask"][:, 0] > 0)).any())  # gt == 0 under an event
    # both sides of every counting threshold occur among the valid pixels
    v = t["m"] > 0
    for a, thr in ((t["ae"], 3.0), (t["ne"], 0.5), (t["fn"], 0.5)):
        assert bool((a[v] > thr).any()) and bool((a[v] < thr).any()), name


def test_metric_cases_reach_their_edges():
    def blocks(name, per_block):
        B, H, W = eh.MET_CASES[name]["shape"]
        return -(-H * W // per_block)

    assert blocks("2x20x24", eh.AEE_SLICE) == 1 and blocks("5x67x70", eh.AEE_SLICE) == 2
    assert 67 * 70 % eh.AEE_SLICE == 594
    assert eh.MET_CASES["1024x3x3"]["shape"][0] == eh.AEE_MAX_B
    assert blocks("6x130x130", eh.FM_CHUNK) == 67 > 64 and eh.MET_CASES["6x130x130"]["shape"][0] > 4
    assert eh.MET_CASES["256x2x2"]["shape"][0] == eh.FM_MAX_B


@pytest.mark.parametrize("name", sorted(eh.MET_CASES))
def test_metrics_oracle32_vs_fp64(name):
    c = eh.MET_CASES[name]
    d = eh.met_data(c)
    for per_sample in (False, True):
        dts = eh.met_dts(c["shape"][0], per_sample)
        eh.compare_metrics(f"{name} per-sample dt {per_sample} (fp32 oracle)",
                           eh.met_reference(d, dts, torch.float32), eh.met_reference(d, dts))


# ---------------------------------------------------------------------------
# encodings
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", eh.ENC_CASES, ids=lambda c: c["id"])
def test_encodings_oracle32_within_bound(c):
    ev = eh.enc_data(c)
    for rnd in (False, True):
        eh.compare_enc(f"{c['id']} round_ts={int(rnd)} (fp32 oracle)", eh.enc_oracle32(c, ev, rnd),
                       eh.enc_reference(c, ev, rnd), rnd)


@pytest.mark.parametrize("c", eh.ENC_CASES, ids=lambda c: c["id"])
def test_encoding_cases_reach_their_edges(c):
    ev = eh.enc_data(c)
    B, N, H, W = c["B"], c["N"], c["H"], c["W"]
    ins = eh.enc_inside(c, ev)
    if N:
        assert (ev[:, :, 0] == 0).any() and (ev[:, :, 0] == 1).any()
        assert (ev[:, :, 0] >= 0).all() and (ev[:, :, 0] <= 1).all()
        assert (ev[:, :, 3] > 0).any() and (ev[:, :, 3] < 0).any()
    if c.get("outside"):
        # per sample: four events dropped, of which each violates another side of the guard, and
        # y == -0.5 kept at row 0
        assert ((~ins).sum(1) == 4).all()
        out = ev[0][~ins[0]]
        assert sorted(map(tuple, out[:, 1:3].tolist())) == sorted(
            (float(np.float32(y)), float(np.float32(x))) for y, x in eh.outside_yx(H, W)[:4])
        assert ((ev[:, :, 1] == -0.5) & ins).sum() == B
    else:
        assert ins.all()
    if c["id"].startswith("grid_stride"):
        assert B * N > eh.ENC_FIRST_PASS
        # the events of the second pass change the result: the reference of the first pass alone differs
        first = dict(c, N=eh.ENC_FIRST_PASS)
        a = eh.enc_reference(c, ev, True)
        b = eh.enc_reference(first, ev[:, :eh.ENC_FIRST_PASS], True)
        assert not np.array_equal(a["cnt"], b["cnt"]) and not np.array_equal(a["voxel"]["sum"], b["voxel"]["sum"])
    if c["id"].startswith("batch"):  # events that share a pixel, fractions that truncation removes
        ref = eh.enc_reference(c, ev, False)
        assert ref["voxel"]["n"].max() >= 2 and (ev[:, :, 1:3] % 1 != 0).any()


def test_voxel_contrib_is_the_oracles_arithmetic():
    """The numpy fp32 restatement of the voxel weight equals oracle.encodings_ref's torch arithmetic bit
    for bit (one event per pixel: no summation)."""
    from oracle import encodings_ref

    r = np.random.default_rng(3)
    H, W, nb = 16, 16, 5
    ts = r.random(H * W, dtype=np.float32)
    ts[:2] = 0.0, 1.0
    ps = np.where(r.random(H * W) < 0.5, 1.0, -1.0).astype(np.float32)
    ys, xs = np.divmod(np.arange(H * W), W)
    for rnd in (False, True):
        v = encodings_ref.events_to_voxel(torch.from_numpy(xs.astype(np.float32)), torch.from_numpy(ys.astype(np.float32)),
                                          torch.from_numpy(ts), torch.from_numpy(ps), nb, (H, W), rnd).numpy()
        for k in range(nb):
            np.testing.assert_array_equal(v[k].reshape(-1), eh.voxel_contrib(ts, ps, k, nb, rnd))
