"""Shared harness (a plain helper module, imported like firenet_harness.py / unet_harness.py): the
evaluation and encoding kernels (csrc/eval.hip, csrc/encode.hip) at band, slice and batch edges against
high-precision references.  test_gpu_eval_edges.py runs the HIP kernels through it; test_eval_edges_cpu.py
runs the fp32 CPU oracle in the role of "ours" through the same compare functions and asserts, on the
references alone, that the seeded inputs reach the edges the case names promise.

Scattered images (pol-IWE, deblur, voxel grids): every contribution is taken in fp32, bit-exact with the
kernel (corners and weights from oracle.iwe_ref.warp_corners_np, the per-event flow gathered at
(int)(y*W + x), voxel weights restated in encode.hip's operation order), and accumulated in fp64 with
np.add.at.  Alongside the sum the reference records, per pixel, the number n_p of non-zero contributions
and the sum S_p of their absolute values.  The kernel then differs from the reference only by the order
of its fp32 additions: any order of n_p fp32 additions is, to first order, within (n_p - 1) 2^-24 S_p of
the exact sum; the bound asserted is twice that, n_p 2^-23 S_p per pixel -- derived, not measured.
Rounded images, counts, masks, polarity masks and voxel grids of rounded timestamps are sums of +-1 below
2^24, exact in any order: compared for equality.

Flow metrics and AEE: oracle.metrics_ref.flow_metrics_ref in fp64, rtol 2e-5 / atol 1e-6 (the bounds of
test_flow_metrics_vs_oracle_random).  One pixel on the other side of a threshold already exceeds that
for the counting metrics, so the seeds are chosen such that, in the fp64 reference, no valid pixel lies
within relative 1e-4 of a threshold (``threshold_margin``), and every angle whose acos is a sample's
result stays away from 0 and pi, where acos is ill-conditioned in fp32 (``angle_margin``); both are
asserted by test_eval_edges_cpu.py.
"""
import numpy as np
import torch

from oracle import encodings_ref, iwe_ref
from oracle.metrics_ref import flow_metrics_ref, flow_metrics_terms

F32 = np.float32
POLB_BAND = 4096          # csrc/eval.hip: pixels per block of k_pol_iwe_band
POL_BANDED_MAX_N = 65536  # above: the global-atomic k_pol_iwe
AEE_SLICE = 1024 * 4      # AEE_NT * AEE_PPT pixels per k_aee block
AEE_MAX_B = 1024          # AEE_NT
FM_CHUNK = 256            # NT pixels per k_flow_metrics block
FM_MAX_B = 256            # NT
ENC_FIRST_PASS = 8192 * 256  # events k_encode's grid covers before its grid-stride loop repeats
FLOW_SCALING = 128
EPS_ORDER = 2.0 ** -23    # per-pixel bound n_p * EPS_ORDER * S_p
MARGIN = 1e-4             # relative distance every valid pixel keeps from every metric threshold
RTOL, ATOL = 2e-5, 1e-6   # test_flow_metrics_vs_oracle_random


def report(tag, what, value):
    print(f"[eval-edges] {tag}: {what} {value:.3g}")


def poison(dev, *shapes):
    """NaN-filled device tensors of the given shapes, freed again.  The caching allocator hands the same
    blocks to the next torch.empty of those sizes, so an output element that a kernel fails to write shows
    up as NaN, not as a chance zero."""
    t = [torch.full(s, float("nan"), device=dev) for s in shapes if int(np.prod(s)) > 0]
    del t


# ---------------------------------------------------------------------------
# exact-sum scatter reference and its compare
# ---------------------------------------------------------------------------
def scatter_exact(idx, val, size):
    """fp64 sum of the fp32 contributions val at idx, with n (non-zero contributions) and S (sum of
    their absolute values) per pixel."""
    v = np.asarray(val, dtype=np.float64).reshape(-1)
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    s, n, a = np.zeros(size), np.zeros(size), np.zeros(size)
    np.add.at(s, idx, v)
    np.add.at(n, idx, (v != 0).astype(np.float64))
    np.add.at(a, idx, np.abs(v))
    return s, n, a


def compare_scatter(tag, ours, ref, exact=False):
    """ours fp32 array against ref {"sum", "n", "S"}; returns the worst per-pixel err / bound."""
    ours = np.asarray(ours)
    assert ours.dtype == np.float32 and ours.shape == ref["sum"].shape, (tag, ours.dtype, ours.shape)
    if exact:
        np.testing.assert_array_equal(ours, ref["sum"], err_msg=tag)
        return 0.0
    err = np.abs(ours.astype(np.float64) - ref["sum"])  # NaN (an unwritten element) fails both asserts
    bound = ref["n"] * EPS_ORDER * ref["S"]
    assert np.isfinite(err).all(), (tag, "non-finite output")
    pos = bound > 0
    assert (err[~pos] == 0).all(), (tag, "a pixel without contributions is not zero", float(err[~pos].max()))
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    report(tag, "worst err/bound", ratio)
    assert ratio <= 1.0, (tag, ratio)
    return ratio


# ---------------------------------------------------------------------------
# pol-IWE / deblur
# ---------------------------------------------------------------------------
# (B, H, W, N); the names say which edges the seeded data must reach (asserted in test_eval_edges_cpu.py)
POL_CASES = [
    dict(shape=(2, 67, 70, 1500), seed=101, names=("two_bands", "band_crossing", "out_of_image")),
    dict(shape=(2, 64, 64, 1025), seed=102, names=("one_full_band",)),
    dict(shape=(1, 5, 900, 700), seed=103, names=("wide", "out_of_image")),
    dict(shape=(3, 20, 24, 0), seed=104, names=("no_events",)),
    dict(shape=(2, 20, 24, 65537), seed=105, names=("global_atomics",)),
]
POL_MASKS = ("pol", "none", "pos")  # compute_pol_iwe; deblur_events without / with a polarity mask


def pol_id(c):
    return "x".join(str(v) for v in c["shape"][:3]) + f"-n{c['shape'][3]}-" + "-".join(c["names"])


def pol_path(c):
    """The kernel snnflow_pol_iwe selects (restated from its host code)."""
    B, H, W, N = c["shape"]
    nbands = (H * W + POLB_BAND - 1) // POLB_BAND
    return "band" if B * nbands <= 65535 * 64 and N <= POL_BANDED_MAX_N else "global"


def pol_data(c):
    """Events at integer rows and at columns that are integers or integer + 0.5 (the flow gather
    truncates), flows uniform in +-0.25 (warps of up to 32 pixels at flow_scaling 128), +-1 polarities."""
    B, H, W, N = c["shape"]
    r = np.random.default_rng(c["seed"])
    ev = np.zeros((B, N, 4), F32)
    ev[:, :, 0] = r.random((B, N), dtype=F32)
    ev[:, :, 1] = r.integers(0, H, (B, N))
    ev[:, :, 2] = r.integers(0, W, (B, N)) + 0.5 * (r.random((B, N)) < 0.25)
    ev[:, :, 3] = np.where(r.random((B, N)) < 0.5, 1.0, -1.0)
    flow = ((r.random((B, 2, H, W), dtype=F32) - F32(0.5)) * F32(0.5)).astype(F32)
    pol = np.stack([(ev[:, :, 3] > 0), (ev[:, :, 3] < 0)], axis=2).astype(F32)
    return {"ev": ev, "flow": flow, "pol": pol}


def _pol_columns(d, masks):
    if masks == "pol":
        return [d["pol"][:, :, 0], d["pol"][:, :, 1]]
    if masks == "pos":
        return [d["pol"][:, :, 0]]
    return [np.ones(d["ev"].shape[:2], F32)]


def pol_corners(c, d, round_idx):
    """(idx, wt, inb) [B, K*N] of oracle.iwe_ref.warp_corners_np at the gathered per-event flows."""
    B, H, W, N = c["shape"]
    pix = iwe_ref.event_pixel_index_np(d["ev"], (H, W))
    fl = d["flow"].reshape(B, 2, H * W)
    fev = np.stack([np.take_along_axis(fl[:, 1], pix, 1), np.take_along_axis(fl[:, 0], pix, 1)], axis=2)
    return iwe_ref.warp_corners_np(d["ev"], fev, 1.0, (H, W), FLOW_SCALING, round_idx=round_idx)


def pol_reference(c, d, round_idx, masks):
    B, H, W, N = c["shape"]
    idx, wt, _ = pol_corners(c, d, round_idx)
    K = idx.shape[1] // N if N else 1
    cols = _pol_columns(d, masks)
    out = {k: np.zeros((B, len(cols), H, W)) for k in ("sum", "n", "S")}
    for b in range(B):
        for k, m in enumerate(cols):
            v = (wt[b] * np.tile(m[b], K)).astype(F32)  # the kernel's c.wt * m[k] (mk * m[k] when rounded)
            s, n, a = scatter_exact(idx[b], v, H * W)
            out["sum"][b, k], out["n"][b, k], out["S"][b, k] = (x.reshape(H, W) for x in (s, n, a))
    return out


def pol_stats(c, d):
    """Share of the bilinear corners that lie outside the image; number of events whose non-zero
    corners lie in two different bands of POLB_BAND pixels; number of bands; pixels of the last band."""
    B, H, W, N = c["shape"]
    idx, wt, inb = pol_corners(c, d, False)
    band = (idx // POLB_BAND).reshape(B, 4, N).astype(np.float64)
    nz = (wt != 0).reshape(B, 4, N)
    lo = np.where(nz, band, np.inf).min(1)
    hi = np.where(nz, band, -np.inf).max(1)
    nb = (H * W + POLB_BAND - 1) // POLB_BAND
    return {"outside": float((~inb).mean()) if N else 0.0, "crossing": int((hi > lo).sum()), "bands": nb,
            "last_band": H * W - (nb - 1) * POLB_BAND}


def pol_oracle32(c, d, round_idx, masks):
    """The fp32 CPU oracle (compute_pol_iwe_t / deblur_events_t) in the role of "ours"."""
    B, H, W, N = c["shape"]
    t = {k: torch.from_numpy(v) for k, v in d.items()}
    if masks == "pol":
        out = iwe_ref.compute_pol_iwe_t(t["flow"], t["ev"], [H, W], t["pol"][:, :, 0:1], t["pol"][:, :, 1:2],
                                        FLOW_SCALING, round_idx)
    else:
        out = iwe_ref.deblur_events_t(t["flow"], t["ev"], [H, W], FLOW_SCALING, round_idx,
                                      t["pol"][:, :, 0:1] if masks == "pos" else None)
    return out.numpy()


def pol_hip(c, d, dev, round_idx, masks, separate=False):
    """snnflow.iwe on the device.  masks "pol": the two columns of one [B,N,2] tensor (read in place,
    stride 2), or with ``separate`` two tensors of their own (the concatenation path)."""
    from snnflow import iwe

    B, H, W, N = c["shape"]
    t = {k: torch.from_numpy(v).to(dev) for k, v in d.items()}
    poison(dev, (B, 2 if masks == "pol" else 1, H, W))
    if masks == "pol":
        p, n = t["pol"][:, :, 0:1], t["pol"][:, :, 1:2]
        if separate:
            p, n = p.clone(), n.clone()
        out = iwe.compute_pol_iwe(t["flow"], t["ev"], [H, W], p, n, flow_scaling=FLOW_SCALING, round_idx=round_idx)
    else:
        out = iwe.deblur_events(t["flow"], t["ev"], [H, W], flow_scaling=FLOW_SCALING, round_idx=round_idx,
                                polarity_mask=t["pol"][:, :, 0:1] if masks == "pos" else None)
    return out.cpu().numpy()


# ---------------------------------------------------------------------------
# flow metrics and AEE
# ---------------------------------------------------------------------------
# shape (B, H, W); density: share of pixels with events; rot: see met_data.  The seeds satisfy
# threshold_margin > MARGIN and angle_margin > ANGLE_MARGIN for every dt variant (the first that do,
# counting up from 1; asserted in test_eval_edges_cpu.py).
MET_CASES = {
    "2x20x24": dict(shape=(2, 20, 24), seed=1, density=0.5),        # one AEE slice, two chunks
    "5x67x70": dict(shape=(5, 67, 70), seed=1, density=0.15),       # two AEE slices, the second of 594 pixels
    "1024x3x3": dict(shape=(1024, 3, 3), seed=1, density=0.5, rot=True),  # AEE's B limit
    "6x130x130": dict(shape=(6, 130, 130), seed=3, density=0.15),   # 67 chunks; samples 4, 5: the waves' second round
    "256x2x2": dict(shape=(256, 2, 2), seed=1, density=0.5, rot=True),    # the finalize table's B limit
}
_DT_IN, _DT_GT = (0.5, 0.25, 1.0), (1.0, 1.0, 0.5)  # ratios 2, 4, 0.5
ANGLE_MARGIN = 0.15  # see angle_margin


def met_dts(B, per_sample):
    """(dt_input, dt_gt): one value each, or B values each."""
    if not per_sample:
        return torch.tensor([0.5]), torch.tensor([1.0])
    return (torch.tensor([_DT_IN[b % 3] for b in range(B)]), torch.tensor([_DT_GT[b % 3] for b in range(B)]))


def met_data(c):
    """Ground truth in +-5 with a zero first row and scattered zero pixels (invalid); a sparse event mask
    and -- for B > 1 -- the last sample fully masked (nvalid == 0).  Predicted flows: small and random
    (magnitudes on both sides of the filter threshold after scaling), three in ten of them the ground truth
    plus an offset of up to 1.5 per component (errors on both sides of the outlier thresholds).
    ``rot`` (samples of a few pixels, where one pixel's angle is a sample's result): the prediction is the
    ground truth rotated by the sample's own angle in +-[0.3, pi - 0.3] and scaled by the sample's own
    factor in [0.05, 2], so every angle a metric takes the acos of is well conditioned by construction."""
    B, H, W = c["shape"]
    gen = torch.Generator().manual_seed(c["seed"])
    rnd = lambda *s: torch.rand(*s, generator=gen)  # noqa: E731
    flow = (rnd(B, 2, H, W) - 0.5) * 0.08
    gt = (rnd(B, 2, H, W) - 0.5) * 10
    gt[:, :, 0] = 0.0
    gt = gt * (rnd(B, 1, H, W) < 0.9)
    if c.get("rot"):
        th = ((0.3 + (np.pi - 0.6) * rnd(B)) * torch.where(rnd(B) < 0.5, -1.0, 1.0)).view(B, 1, 1)
        s = (0.05 + 1.95 * rnd(B)).view(B, 1, 1)
        fx = s * (torch.cos(th) * gt[:, 0] - torch.sin(th) * gt[:, 1])
        fy = s * (torch.sin(th) * gt[:, 0] + torch.cos(th) * gt[:, 1])
        zero = ((gt[:, 0] == 0) & (gt[:, 1] == 0)).unsqueeze(1)
        flow = torch.where(zero, flow, torch.stack([fx, fy], dim=1) / (FLOW_SCALING * 2.0))
    else:
        near = (gt + (rnd(B, 2, H, W) - 0.5) * 3.0) / (FLOW_SCALING * 2.0)
        flow = torch.where(rnd(B, 1, H, W) < 0.3, near, flow)
    mask = (rnd(B, 1, H, W) < c["density"]).float()
    if B > 1:
        mask[B - 1] = 0.0
    return {"flow": flow, "gt": gt, "mask": mask}


def met_reference(d, dts, dtype=torch.float64):
    r = flow_metrics_ref(d["flow"], d["gt"], d["mask"], dts[0], dts[1], FLOW_SCALING, 0.5, dtype=dtype)
    return {k: v.numpy().astype(np.float64) for k, v in r.items()}


def threshold_margin(d, dts):
    """Smallest relative distance, over the valid pixels of the fp64 reference, between a compared
    quantity and its threshold: ae | 3, ae | 0.05 |f'|, ne | 0.5, aa | pi/6, |f'| | mag_threshold."""
    t = flow_metrics_terms(d["flow"], d["gt"], d["mask"], dts[0], dts[1], FLOW_SCALING, dtype=torch.float64)
    v = t["m"] > 0
    if not bool(v.any()):
        return float("inf")

    def dist(a, b):
        b = torch.as_tensor(b, dtype=torch.float64).expand_as(a)
        return float(((a - b).abs() / b.abs().clamp_min(1e-300))[v].min())

    return min(dist(t["ae"], 3.0), dist(t["ae"], 0.05 * t["fn"]), dist(t["ne"], 0.5), dist(t["aa"], np.pi / 6),
               dist(t["fn"], 0.5))


def angle_margin(c, d, dts):
    """Smallest distance from 0 and pi of the angles whose acos is a sample's result in the fp64 reference:
    ae_of_means of every sample with valid pixels and, for ``rot`` cases, the angular error of every pixel
    with a non-zero ground truth.  acos turns an error dc of its argument into dc / sin(angle); with dc a
    few 2^-24 from the fp32 dot product and norms, a relative error below RTOL needs angle * sin(angle)
    above about 1e-2, i.e. an angle above 0.1: the seeds keep ANGLE_MARGIN = 0.15.  (Sums over thousands
    of pixels are not bound by this: their ill-conditioned terms are small against the sum.)"""
    t = flow_metrics_terms(d["flow"], d["gt"], d["mask"], dts[0], dts[1], FLOW_SCALING, dtype=torch.float64)
    r = flow_metrics_ref(d["flow"], d["gt"], d["mask"], dts[0], dts[1], FLOW_SCALING, 0.5, dtype=torch.float64)
    ang = [r["ae_of_means"][t["m"].sum(1) > 0]]
    if c.get("rot"):
        ang.append(t["ang"][(t["gn"] > 0) & (t["fn"] > 0)])
    a = torch.cat([x.reshape(-1) for x in ang])
    return float(torch.minimum(a, np.pi - a).min()) if a.numel() else float("inf")


def compare_metrics(tag, ours, ref, keys=None):
    """ours / ref {name: [B] array}; returns the worst relative error over entries above ATOL."""
    worst = 0.0
    for k in keys or sorted(ref):
        o, r = np.asarray(ours[k], np.float64).reshape(-1), ref[k].reshape(-1)
        assert o.shape == r.shape, (tag, k, o.shape, r.shape)
        big = np.abs(r) > ATOL
        if big.any():
            worst = max(worst, float((np.abs(o - r)[big] / np.abs(r)[big]).max()))
    report(tag, "worst metric rel. error", worst)
    for k in keys or sorted(ref):
        np.testing.assert_allclose(np.asarray(ours[k], np.float64).reshape(-1), ref[k].reshape(-1), rtol=RTOL,
                                   atol=ATOL, err_msg=f"{tag} {k}")
    return worst


def _cfg(H, W):
    return {"loader": {"resolution": [H, W]}, "loss": {"overwrite_intermediate": False}}


def new_aee(dev, H, W):
    import snnflow

    return snnflow.AEE(_cfg(H, W), dev, flow_scaling=FLOW_SCALING)


def aee_hip(m, d, dts, dev):
    """One call of a snnflow.AEE object (its resolution follows the data); returns device tensors."""
    B, _, H, W = d["flow"].shape
    m.res = [H, W]
    m.reset()
    m.event_flow_association([d["flow"].to(dev)], {
        "event_list": torch.zeros(B, 1, 4, device=dev), "event_list_pol_mask": torch.zeros(B, 1, 2, device=dev),
        "event_mask": d["mask"].to(dev), "gtflow": d["gt"].to(dev), "dt_input": dts[0], "dt_gt": dts[1]})
    return m()


def aee_dict(res):
    return {"aee": res[0].cpu().numpy(), "aee_pct": res[1].cpu().numpy()}


def metrics_hip(d, dts, dev):
    from snnflow import metrics

    class _M:
        pass

    m = _M()
    m._flow_map, m._gtflow, m._event_mask = [d["flow"].to(dev)], d["gt"].to(dev), d["mask"].to(dev)
    m._dt_input, m._dt_gt, m.flow_scaling = dts[0], dts[1], FLOW_SCALING
    return {k: v.cpu().numpy() for k, v in metrics._flow_metrics(m, mag_threshold=0.5).items()}


# ---------------------------------------------------------------------------
# encodings
# ---------------------------------------------------------------------------
# out-of-image events (y, x) appended to every sample of an "outside" case: four that the kernel must
# drop and one (y = -0.5 truncates to row 0) that stays
def outside_yx(H, W):
    return [(H, 3.0), (2.0, W), (-1.0, 3.0), (2.0, W + 0.9), (-0.5, 4.0)]


ENC_CASES = [
    dict(id="batch-3x257-13x17-bins5", B=3, N=257, H=13, W=17, bins=5, seed=201, single=True),
    dict(id="one_bin-2x1-1x19-bins1", B=2, N=1, H=1, W=19, bins=1, seed=202),
    dict(id="no_events-3x0-13x17-bins2", B=3, N=0, H=13, W=17, bins=2, seed=203),
    dict(id="grid_stride-1x2200000-64x64-bins2", B=1, N=2_200_000, H=64, W=64, bins=2, seed=204),
    dict(id="out_of_image-2x69-13x17-bins5", B=2, N=69, H=13, W=17, bins=5, seed=205, outside=True, single=True),
]


def enc_data(c):
    """[B, N, 4] (ts, y, x, p): in-image coordinates, a third of them with a fraction (.long() truncates);
    p = +-1; ts in [0, 1) with one event at exactly 0 and one at exactly 1 per sample (N == 1: sample b has
    ts = b % 2 and p = 1 - 2 (b % 2)); with ``outside`` the last five events of every sample are outside_yx."""
    B, N, H, W = c["B"], c["N"], c["H"], c["W"]
    r = np.random.default_rng(c["seed"])
    ev = np.zeros((B, N, 4), F32)
    ev[:, :, 0] = r.random((B, N), dtype=F32)
    ev[:, :, 1] = r.integers(0, H, (B, N)) + 0.75 * (r.random((B, N)) < 1 / 3)
    ev[:, :, 2] = r.integers(0, W, (B, N)) + 0.75 * (r.random((B, N)) < 1 / 3)
    ev[:, :, 3] = np.where(r.random((B, N)) < 0.5, 1.0, -1.0)
    if N >= 2:
        ev[:, 0, 0], ev[:, 1, 0] = 0.0, 1.0
    elif N == 1:
        ev[:, 0, 0] = np.arange(B) % 2
        ev[:, 0, 3] = 1.0 - 2.0 * (np.arange(B) % 2)
    if c.get("outside"):
        for j, (y, x) in enumerate(outside_yx(H, W)):
            ev[:, N - 5 + j, 1], ev[:, N - 5 + j, 2] = y, x
    return ev


def enc_inside(c, ev):
    """[B, N] bool: the truncated coordinates are in the image (the kernel's guard)."""
    yi, xi = ev[:, :, 1].astype(np.int64), ev[:, :, 2].astype(np.int64)
    return (yi >= 0) & (yi < c["H"]) & (xi >= 0) & (xi < c["W"])


def voxel_contrib(ts, ps, k, nb, round_ts):
    """encode.hip's p * max(0, 1 - |t - k|), t = ts * (nb - 1), in numpy fp32 in its operation order."""
    t = (ts * F32(nb - 1)).astype(F32)
    if round_ts:
        t = np.rint(t).astype(F32)
    w = np.maximum(F32(0), (F32(1) - np.abs((t - F32(k)).astype(F32))).astype(F32)).astype(F32)
    return (ps * w).astype(F32)


def enc_reference(c, ev, round_ts):
    """cnt, mask (oracle.encodings_ref on the in-image events), pol (every event) and the exact-sum
    voxel grid {"sum", "n", "S"}."""
    B, N, H, W, nb = c["B"], c["N"], c["H"], c["W"], c["bins"]
    ins = enc_inside(c, ev)
    ref = {"cnt": np.zeros((B, 2, H, W), F32), "mask": np.zeros((B, 1, H, W), F32), "pol": np.zeros((B, N, 2), F32),
           "voxel": {k: np.zeros((B, nb, H, W)) for k in ("sum", "n", "S")}}
    for b in range(B):
        e = ev[b][ins[b]]
        ts, ys, xs, ps = (torch.from_numpy(np.ascontiguousarray(e[:, j])) for j in range(4))
        ref["cnt"][b] = encodings_ref.events_to_channels(xs, ys, ps, (H, W)).numpy()
        ref["mask"][b] = encodings_ref.create_mask_encoding(xs, ys, ps, (H, W)).numpy()
        ref["pol"][b] = encodings_ref.create_polarity_mask(torch.from_numpy(ev[b, :, 3].copy())).t().numpy()
        pix = e[:, 1].astype(np.int64) * W + e[:, 2].astype(np.int64)
        for k in range(nb):
            s, n, a = scatter_exact(pix, voxel_contrib(e[:, 0], e[:, 3], k, nb, round_ts), H * W)
            for key, x in zip(("sum", "n", "S"), (s, n, a)):
                ref["voxel"][key][b, k] = x.reshape(H, W)
    return ref


def compare_enc(tag, ours, ref, round_ts):
    """ours {"cnt", "voxel", "mask", "pol"} fp32 arrays; returns the voxel grid's worst err / bound."""
    for k in ("cnt", "mask", "pol"):
        assert ours[k].dtype == np.float32 and ours[k].shape == ref[k].shape, (tag, k, ours[k].shape)
        np.testing.assert_array_equal(ours[k], ref[k], err_msg=f"{tag} {k}")
    return compare_scatter(f"{tag} voxel", ours["voxel"], ref["voxel"], exact=round_ts)


def enc_oracle32(c, ev, round_ts):
    """The fp32 CPU oracle (oracle.encodings_ref; its index_put_ raises outside the image, so on the
    in-image events) in the role of "ours"."""
    B, N, H, W, nb = c["B"], c["N"], c["H"], c["W"], c["bins"]
    ins = enc_inside(c, ev)
    out = {"cnt": np.zeros((B, 2, H, W), F32), "mask": np.zeros((B, 1, H, W), F32), "pol": np.zeros((B, N, 2), F32),
           "voxel": np.zeros((B, nb, H, W), F32)}
    for b in range(B):
        e = ev[b][ins[b]]
        ts, ys, xs, ps = (torch.from_numpy(np.ascontiguousarray(e[:, j])) for j in range(4))
        out["cnt"][b] = encodings_ref.events_to_channels(xs, ys, ps, (H, W)).numpy()
        out["mask"][b] = encodings_ref.create_mask_encoding(xs, ys, ps, (H, W)).numpy()
        out["pol"][b] = encodings_ref.create_polarity_mask(torch.from_numpy(ev[b, :, 3].copy())).t().numpy()
        out["voxel"][b] = encodings_ref.events_to_voxel(xs, ys, ts, ps, nb, (H, W), round_ts).numpy()
    return out


def _enc_shapes(c):
    B, N, H, W, nb = c["B"], c["N"], c["H"], c["W"], c["bins"]
    return (B, 2, H, W), (B, nb, H, W), (B, 1, H, W), (B, N, 2)


def enc_hip_batch(c, ev, dev, round_ts):
    from snnflow import encodings

    poison(dev, *_enc_shapes(c))
    out = encodings.encode_batch(torch.from_numpy(ev).to(dev), (c["H"], c["W"]), num_bins=c["bins"], round_ts=round_ts)
    return {"cnt": out["event_cnt"].cpu().numpy(), "voxel": out["event_voxel"].cpu().numpy(),
            "mask": out["event_mask"].cpu().numpy(), "pol": out["event_list_pol_mask"].cpu().numpy()}


def enc_hip_single(c, ev, dev, round_ts):
    """The single-sample functions, sample by sample, assembled into encode_batch's layout."""
    from snnflow import encodings as E

    H, W, nb = c["H"], c["W"], c["bins"]
    out = {k: [] for k in ("cnt", "voxel", "mask", "pol")}
    for b in range(c["B"]):
        ts, ys, xs, ps = (torch.from_numpy(np.ascontiguousarray(ev[b, :, j])).to(dev) for j in range(4))
        poison(dev, (2, H, W), (nb, H, W), (1, H, W), (ev.shape[1], 2))
        out["cnt"].append(E.events_to_channels(xs, ys, ps, (H, W)).cpu().numpy())
        out["voxel"].append(E.events_to_voxel(xs, ys, ts, ps, nb, (H, W), round_ts).cpu().numpy())
        out["mask"].append(E.create_mask_encoding(xs, ys, ps, (H, W)).cpu().numpy())
        out["pol"].append(E.create_polarity_mask(ps).t().cpu().numpy())
    return {k: np.stack(v) for k, v in out.items()}


def image_data(c, ev, b):
    """(xs, ys, ps_acc, ps_set, inside) of sample b for events_to_image: ps_acc the +-1 polarities
    (accumulated: an exact integer sum); ps_set a value that is a function of the truncated pixel, so that
    events sharing a pixel agree and last-writer-wins is order-free; inside: the kernel's in-image guard
    (the reference raises on the others and is given the inside events only)."""
    e = ev[b]
    yi, xi = e[:, 1].astype(np.int64), e[:, 2].astype(np.int64)
    ps_set = (((yi * 7 + xi * 3) % 5) - 2).astype(F32)
    return e[:, 2].copy(), e[:, 1].copy(), e[:, 3].copy(), ps_set, enc_inside(c, ev)[b]
