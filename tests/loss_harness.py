"""Harness of the contrast-maximisation loss edge suite (test_loss_edges_cpu.py, test_gpu_loss_edges.py):
csrc/iwe_loss.hip through snnflow.EventWarping against oracle.iwe_ref.EventWarpingRef in fp64, term by term.

Cases are drawn on the CPU from seeds (numpy RandomState) as fp32 tensors and moved to the device.  The
kernels and the fp64 oracle must take the same ``floor`` at every corner, so a case is of one of two kinds:

  safe   random events and flows; every event whose warped y or x (fp64, either direction: tref = T and 0)
         lies within GUARD = 1e-3 of an integer gets polarity mask (0, 0) -- it stays in the list as a
         padding event.  At most GUARD_CAP = 5 % of a case's events may be changed that way.
  exact  timestamps multiples of 1/8, flow_scaling a power of two, flows multiples of 2^-9: (tref - ts) f s
         and the warped coordinate are exact in fp32, so fp32 and fp64 agree bit for bit even on the ties
         (integer landings, flow == 0) where relu_tie, sgnf and the d(nz) term decide the gradient.

Both conditions, and nz > 0 for every sample and direction where loss_scaling is on (else the reference is
NaN), are asserted by test_loss_edges_cpu.py on the committed seeds.

What is compared (compare / assert_case), always "ours" against the fp64 oracle:
  images    the eight IWEs [2 dir][4 img][B][H W], elementwise
  Sp Sn lb  per direction and sample S+, S-, loss_b; nz must be equal
  smooth    the five Charbonnier sums, one by one
  loss      relative error
  grad      every window's (and flow map's) dL/dflow as a relative L2; exactly 0 where the oracle's is
  gfree     dL/dflow elementwise on the pixels that hold no event (smoothness only)
The forward's intermediate results are read from ``loss.grad_fn.saved_tensors``: (images scratch -- the
IWEs are its first 8 B H W floats --, persample [2][B][4], smooth [8]: five sums and their combination).

Limits.  loss and grad keep the project's (rtol 2e-5, relative L2 1e-4, as in
test_event_warping_bands_and_empty_windows_vs_oracle), widened per case only by test_gpu_ragged.py's rule:
4 x the error of the fp32 CPU oracle against the fp64 oracle at that case (REF_LOSS below), where the GPU
exceeded the limit and stayed within that.  The elementwise quantities have no project limit: theirs is
4 x the fp32 oracle's own worst absolute error for that quantity and case (REF_LOSS), never below two fp32
roundings of the quantity's largest magnitude (the kernels round their exact fixed-point sums once).
``python tests/loss_harness.py`` prints the REF_LOSS table."""
import os
import sys

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(_HERE), os.path.join(os.path.dirname(_HERE), "snn_event-based_optical_flow_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import iwe_ref  # noqa: E402

GUARD, GUARD_CAP = 1e-3, 0.05
LOSS_RTOL, GRAD_TOL = 2e-5, 1e-4
EPS32 = 2.0 ** -23
QUANTS = ("images", "Sp", "Sn", "lb", "smooth", "gfree")


class Case:
    """windows: [(events [B,N,4], pol [B,N,2], mask [B,1,H,W])] per window (mask: the pixels that hold an
    event and 70 % of the others; all zeros for a window without events; all ones with M = 0); flows: per
    window a list of nmaps [B,2,H,W] maps (all fp32, CPU).  free(): [B,H,W] bool per window, the pixels that
    hold no event row."""

    def __init__(self, cid, B, H, W, windows, flows, exact=False, weight=0.001, smoothing_mask=True, overwrite=False,
                 loss_scaling=True, flow_scaling=None, g=1.0, noncontig=False, changed=0.0):
        self.cid, self.B, self.H, self.W = cid, B, H, W
        self.windows, self.flows, self.exact = windows, flows, exact
        self.weight, self.smoothing_mask, self.overwrite = weight, smoothing_mask, overwrite
        self.loss_scaling, self.flow_scaling, self.g, self.noncontig = loss_scaling, flow_scaling, g, noncontig
        self.changed = changed  # fraction of events the guard turned into padding
        self.T, self.nmaps = len(windows), len(flows[0])
        self.s = float(flow_scaling if flow_scaling is not None else max(H, W))

    def cfg(self):
        return {"loader": {"resolution": [self.H, self.W]},
                "loss": {"flow_regul_weight": self.weight, "overwrite_intermediate": self.overwrite},
                "model": {"mask_output": self.smoothing_mask}}

    def free(self):
        out = []
        for ev, _, _ in self.windows:
            f = torch.ones(self.B, self.H * self.W, dtype=torch.bool)
            if ev.shape[1]:
                f.scatter_(1, (ev[:, :, 1] * self.W + ev[:, :, 2]).long(), False)
            out.append(f.view(self.B, self.H, self.W))
        if self.overwrite:  # one flow map carries every window's events
            allw = torch.stack(out).all(0)
            out = [allw] * self.T
        return out


# ---------------------------------------------------------------------------
# warped coordinates on the CPU: fp64, and fp32 in the kernels' operation order
# ---------------------------------------------------------------------------
def event_flows(case, i=0):
    """Per window the flow (fy, fx) [B,N,2] at every event's pixel, from map i of that window (of the last
    window with overwrite_intermediate)."""
    out = []
    for k, (ev, _, _) in enumerate(case.windows):
        fl = case.flows[-1 if case.overwrite else k][i].reshape(case.B, 2, -1)
        pix = (ev[:, :, 1] * case.W + ev[:, :, 2]).long()
        out.append(torch.stack([torch.gather(fl[:, 1], 1, pix), torch.gather(fl[:, 0], 1, pix)], dim=2))
    return out


def warped(case, k, fev, tref, dtype):
    """(wy, wx) [B,N] of window k's events: pos + ((tref - (ts + k)) * f) * s in ``dtype`` (numpy)."""
    ev = case.windows[k][0].numpy().astype(dtype)
    f = fev.numpy().astype(dtype)
    ts = (ev[:, :, 0] + dtype(k)).astype(dtype)
    dt = (dtype(tref) - ts).astype(dtype)
    wy = (ev[:, :, 1] + ((dt * f[:, :, 0]).astype(dtype) * dtype(case.s)).astype(dtype)).astype(dtype)
    wx = (ev[:, :, 2] + ((dt * f[:, :, 1]).astype(dtype) * dtype(case.s)).astype(dtype)).astype(dtype)
    return wy, wx


def corners64(case, k, fev, tref):
    """The fp64 corner set of window k: flat indices (0 where out of the image) and in-image flags,
    corner-major like iwe_ref.warp_corners_np."""
    wy, wx = warped(case, k, fev, tref, np.float64)
    y0, y1, x0, x1 = np.floor(wy), np.floor(wy + 1), np.floor(wx), np.floor(wx + 1)
    idx, inb = [], []
    for cy, cx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)):
        m = (cy >= 0) & (cy < case.H) & (cx >= 0) & (cx < case.W)
        idx.append(np.where(m, cy * case.W + cx, 0).astype(np.int64))
        inb.append(m)
    return np.concatenate(idx, 1), np.concatenate(inb, 1)


def _apply_guard(case):
    """Safe cases: polarity mask (0, 0) for every event with a warped coordinate within GUARD of an integer."""
    hit = tot = 0
    for i in range(case.nmaps):
        fevs = event_flows(case, i)
        for k, (ev, pol, _) in enumerate(case.windows):
            if not ev.shape[1]:
                continue
            near = np.zeros(ev.shape[:2], bool)
            for tref in (case.T, 0):
                for w in warped(case, k, fevs[k], tref, np.float64):
                    near |= np.abs(w - np.rint(w)) < GUARD
            near &= (pol.numpy() != 0).any(2)
            pol[torch.from_numpy(near)] = 0.0
            hit += int(near.sum())
            if i == 0:
                tot += int((pol.numpy() != 0).any(2).sum()) + int(near.sum())
    case.changed = hit / max(tot, 1)
    return case


# ---------------------------------------------------------------------------
# case generators
# ---------------------------------------------------------------------------
def _window(rng, B, N, H, W, place="uniform", pad=0.0):
    if place == "patch":  # every event on one 3 x 3 patch
        y0, x0 = H // 2 - 1, W // 2 - 1
        ys, xs = rng.randint(y0, y0 + 3, (B, N)), rng.randint(x0, x0 + 3, (B, N))
    elif place == "border":  # the four corners, the four borders, and the interior in equal parts
        ys, xs = rng.randint(0, H, (B, N)), rng.randint(0, W, (B, N))
        side = rng.randint(0, 8, (B, N))
        ys = np.where(side == 0, 0, np.where(side == 1, H - 1, ys))
        xs = np.where(side == 2, 0, np.where(side == 3, W - 1, xs))
        cy, cx = rng.randint(0, 2, (B, N)) * (H - 1), rng.randint(0, 2, (B, N)) * (W - 1)
        ys, xs = np.where(side == 4, cy, ys), np.where(side == 4, cx, xs)
    else:
        ys, xs = rng.randint(0, H, (B, N)), rng.randint(0, W, (B, N))
    ts = np.sort(rng.rand(B, N), axis=1)
    ps = rng.randint(0, 2, (B, N)) * 2 - 1
    ev = np.stack([ts, ys, xs, ps], 2).astype(np.float32)
    pol = np.stack([ps > 0, ps < 0], 2).astype(np.float32)
    npad = int(round(pad * N))
    if npad:  # trailing padding rows of a collated batch: all zeros, polarity mask (0, 0)
        ev[:, N - npad:], pol[:, N - npad:] = 0.0, 0.0
    mask = np.zeros((B, H * W), np.float32)
    for b in range(B):
        real = pol[b].any(1)
        mask[b, (ys[b][real] * W + xs[b][real])] = 1.0
    if N:  # and 70 % of the other pixels, so that event-free pixels carry a smoothness gradient
        mask = np.maximum(mask, (rng.rand(B, H * W) < 0.7).astype(np.float32))
    return torch.from_numpy(ev), torch.from_numpy(pol), torch.from_numpy(mask).view(B, 1, H, W)


def safe_case(cid, B, H, W, counts, seed, amp_px=None, place="uniform", pad=0.0, nmaps=1, **opts):
    """Random events (counts[k] per sample in window k) and flows uniform in +- amp_px pixels per unit time
    (in flow units of the default flow_scaling max(H, W))."""
    rng = np.random.RandomState(seed)
    T = len(counts)
    if amp_px is None:
        amp_px = min(3.0, 0.25 * max(H, W) / T)
    windows = [_window(rng, B, n, H, W, place, pad) for n in counts]
    flows = []
    for _ in range(T):
        maps = []
        for _ in range(nmaps):
            f = (rng.rand(B, 2, H, W) * 2 - 1) * (amp_px / max(H, W))
            maps.append(torch.from_numpy(f.astype(np.float32)))
        flows.append(maps)
    return _apply_guard(Case(cid, B, H, W, windows, flows, **opts))


def exact_case(cid, B, H, W, T, n, seed, flow_scaling, variant, **opts):
    """variant: "sparse" / "dense" (n events per window and sample, six of them planted, see below) or "zero"
    (flow exactly 0 everywhere).  Flows are m 2^-9 with half of the m giving whole or half pixels per unit
    time; timestamps j / 8 with 0 and 1 over-represented.  Planted in the last window at ts = 0 (forward
    dt = 1): landings exactly on row H - 1, row H, row -1, column W - 1, column W and column -1."""
    rng = np.random.RandomState(seed)
    s = float(flow_scaling)
    unit = 512.0 / s  # m per (pixel per unit time)
    assert s <= 512 and unit == int(unit) and unit % 2 == 0
    planted = [(H - 2, 3, 1, 0), (H - 2, 4, 2, 0), (0, 4, -1, 0), (2, W - 2, 0, 1), (1, W - 2, 0, 2), (1, 0, 0, -1)]
    windows, flows = [], []
    for k in range(T):
        half = rng.randint(-4, 5, (B, 2, H, W)) * (unit / 2)
        anym = rng.randint(-2 * int(unit), 2 * int(unit) + 1, (B, 2, H, W))
        m = np.where(rng.rand(B, 2, H, W) < 0.5, half, anym)
        if variant == "zero":
            m = np.zeros_like(m)
        ys, xs = rng.randint(0, H, (B, n)), rng.randint(0, W, (B, n))
        ts = rng.choice(np.arange(9) / 8.0, size=(B, n), p=[0.2] + [0.6 / 7] * 7 + [0.2])
        if k == T - 1 and variant != "zero":
            for j, (y, x, py, px) in enumerate(planted):
                ys[:, j], xs[:, j], ts[:, j] = y, x, 0.0
                m[:, 1, y, x], m[:, 0, y, x] = py * unit, px * unit
        order = np.argsort(ts, axis=1, kind="stable")
        ys, xs, ts = (np.take_along_axis(a, order, 1) for a in (ys, xs, ts))
        ps = rng.randint(0, 2, (B, n)) * 2 - 1
        ev = np.stack([ts, ys, xs, ps], 2).astype(np.float32)
        pol = np.stack([ps > 0, ps < 0], 2).astype(np.float32)
        mask = np.zeros((B, H * W), np.float32)
        for b in range(B):
            mask[b, ys[b] * W + xs[b]] = 1.0
        mask = np.maximum(mask, (rng.rand(B, H * W) < 0.7).astype(np.float32))
        windows.append((torch.from_numpy(ev), torch.from_numpy(pol), torch.from_numpy(mask).view(B, 1, H, W)))
        flows.append([torch.from_numpy((m / 512.0).astype(np.float32))])
    return Case(cid, B, H, W, windows, flows, exact=True, flow_scaling=flow_scaling, **opts)


def none_case(cid, B, H, W, T, seed, **opts):
    """No events at all (M = 0), masks of ones; loss_scaling must be off (nz = 0)."""
    rng = np.random.RandomState(seed)
    windows = [(torch.zeros(B, 0, 4), torch.zeros(B, 0, 2), torch.ones(B, 1, H, W)) for _ in range(T)]
    flows = [[torch.from_numpy(((rng.rand(B, 2, H, W) * 2 - 1) * 0.05).astype(np.float32))] for _ in range(T)]
    return Case(cid, B, H, W, windows, flows, loss_scaling=False, **opts)


# ---------------------------------------------------------------------------
# the case lists (one builder per id: built on demand, in the CPU file and the GPU file alike)
# ---------------------------------------------------------------------------
RAGGED = (2, 23, 47)
RAGGED_COUNTS = {"uneven": (300, 0, 2100), "equal": (256, 256, 256)}


def _shape_builders(w):
    kw = {"weight": w}
    return {
        "tiny": lambda c: safe_case(c, 1, 5, 7, (9,), 102, **kw),
        "band": lambda c: exact_case(c, 2, 16, 64, 3, 400, 111, 64, "dense", **kw),
        "ragged-uneven": lambda c: safe_case(c, *RAGGED, RAGGED_COUNTS["uneven"], 103, **kw),
        "ragged-equal": lambda c: safe_case(c, *RAGGED, RAGGED_COUNTS["equal"], 104, **kw),
        "batch17": lambda c: safe_case(c, 17, 6, 10, (40, 40), 105, **kw),
        "batch64": lambda c: safe_case(c, 64, 5, 7, (9,), 106, **kw),
        "windows": lambda c: safe_case(c, 1, 64, 68, (30,) * 64, 107, **kw),
        "windows-overwrite": lambda c: safe_case(c, 1, 64, 68, (30,) * 64, 107, overwrite=True, **kw),
        "wide1791": lambda c: safe_case(c, 2, 3, 1791, (400, 400), 108, **kw),
        "wide600": lambda c: safe_case(c, 2, 3, 600, (200, 200), 109, **kw),
        "none": lambda c: none_case(c, *RAGGED, 3, 110, **kw),
    }


BUILDERS = {}
for _w in (0.001, 1.0):
    for _n, _b in _shape_builders(_w).items():
        BUILDERS[f"{_n}-w{_w:g}"] = _b
TERM_CASES = list(BUILDERS)

OPTION_CASES = []
for _sm in (True, False):
    for _ls in (True, False):
        for _ow in (False, True):
            for _w in (0.001, 1.0):
                for _fs in (None, 20.0):
                    _cid = (f"opt-mask{int(_sm)}-scale{int(_ls)}-over{int(_ow)}-w{_w:g}-fs{'def' if _fs is None else '20'}")
                    BUILDERS[_cid] = (lambda c, sm=_sm, ls=_ls, ow=_ow, w=_w, fs=_fs: safe_case(
                        c, *RAGGED, RAGGED_COUNTS["uneven"], 120, smoothing_mask=sm, loss_scaling=ls, overwrite=ow,
                        weight=w, flow_scaling=fs))
                    OPTION_CASES.append(_cid)

TIE_CASES = []
for _shape, _args in (("band", (2, 16, 64, 3)), ("tiny", (1, 5, 7, 1))):
    for _v, _n in (("sparse", 9), ("dense", None), ("zero", None)):
        _cid = f"ties-{_shape}-{_v}"
        _nn = _n if _n is not None else (400 if _shape == "band" else 60)
        BUILDERS[_cid] = (lambda c, a=_args, n=_nn, v=_v, fs=(64 if _shape == "band" else 8): exact_case(
            c, *a, n, 130, fs, v))
        TIE_CASES.append(_cid)

BUILDERS.update({
    "content-padding": lambda c: safe_case(c, *RAGGED, RAGGED_COUNTS["uneven"], 140, pad=0.3),
    "content-patch": lambda c: safe_case(c, *RAGGED, RAGGED_COUNTS["uneven"], 141, place="patch", amp_px=1.0),
    "content-far": lambda c: safe_case(c, *RAGGED, RAGGED_COUNTS["uneven"], 142, amp_px=2 * 47 / 3.0),
    "content-border": lambda c: safe_case(c, *RAGGED, RAGGED_COUNTS["uneven"], 143, place="border", amp_px=3.0),
    "call-upstream": lambda c: safe_case(c, *RAGGED, RAGGED_COUNTS["equal"], 150, g=-2.5, weight=1.0),
    "call-two-maps": lambda c: safe_case(c, *RAGGED, RAGGED_COUNTS["equal"], 151, nmaps=2, weight=1.0),
    "call-noncontig": lambda c: safe_case(c, *RAGGED, RAGGED_COUNTS["equal"], 152, noncontig=True, weight=1.0),
})
CONTENT_CASES = ["content-padding", "content-patch", "content-far", "content-border"]
CALL_CASES = ["call-upstream", "call-two-maps", "call-noncontig"]
ALL_CASES = TERM_CASES + OPTION_CASES + TIE_CASES + CONTENT_CASES + CALL_CASES
REUSE_CASES = ["tiny-w0.001", "ragged-uneven-w0.001", "batch17-w0.001", "tiny-w0.001"]

_CACHE, _WANT = {}, {}


def get_case(cid):
    if cid not in _CACHE:
        _CACHE[cid] = BUILDERS[cid](cid)
    return _CACHE[cid]


def oracle64(cid):
    """The fp64 oracle's result at case ``cid``, computed once per process and left unchanged."""
    if cid not in _WANT:
        _WANT[cid] = run_oracle(get_case(cid), torch.float64)
    return _WANT[cid]


# ---------------------------------------------------------------------------
# runners: every result is {"loss", "grads" [T][nmaps] (None: no gradient), and for one flow map
# "images" [2,4,B,HW], "persample" [2,B,4], "smooth" [5]} as float64 numpy
# ---------------------------------------------------------------------------
def run_oracle(case, dtype):
    """EventWarpingRef in ``dtype`` on the case's fp32 values; one reference object per flow map, the
    losses averaged (loss/flow.py: loss /= len(flow_list))."""
    flows = [[f.detach().clone().to(dtype).requires_grad_(True) for f in maps] for maps in case.flows]
    losses, terms = [], None
    for i in range(case.nmaps):
        ref = iwe_ref.EventWarpingRef([case.H, case.W], flow_scaling=case.flow_scaling, weight=case.weight,
                                      smoothing_mask=case.smoothing_mask, overwrite_intermediate=case.overwrite,
                                      loss_scaling=case.loss_scaling)
        for (ev, pol, mask), maps in zip(case.windows, flows):
            ref.event_flow_association([maps[i]], ev.to(dtype), pol.to(dtype), mask.to(dtype))
        if case.overwrite:
            ref.overwrite_intermediate_flow([flows[-1][i]])
        terms = ref.terms()
        losses.append(terms["loss"])
    loss = losses[0] if case.nmaps == 1 else sum(losses) / case.nmaps
    (loss * case.g).backward()
    out = {"loss": float(loss.detach()), "grads": [[None if f.grad is None else f.grad.double().numpy() for f in maps]
                                          for maps in flows]}
    if case.nmaps == 1:
        out.update({k: terms[k].double().numpy() for k in ("images", "persample", "smooth")})
    return out


def run_ours(case, dev, ew=None):
    """snnflow.EventWarping on the device; with ``ew`` an existing object is reused (after reset())."""
    import snnflow

    if ew is None:
        ew = snnflow.EventWarping(case.cfg(), dev, flow_scaling=case.flow_scaling, loss_scaling=case.loss_scaling)
    else:
        ew.reset()
        ew.res, ew.flow_scaling = [case.H, case.W], case.s
        ew.weight, ew.smoothing_mask, ew.overwrite_intermediate = case.weight, case.smoothing_mask, case.overwrite
        ew.loss_scaling = case.loss_scaling
    leaves, flows = [], []
    for maps in case.flows:
        if case.noncontig:  # [B, H, W, 2] leaves handed over as permuted views
            lv = [f.permute(0, 2, 3, 1).contiguous().to(dev).requires_grad_(True) for f in maps]
            flows.append([x.permute(0, 3, 1, 2) for x in lv])
            assert not flows[-1][0].is_contiguous()
        else:
            lv = [f.to(dev).requires_grad_(True) for f in maps]
            flows.append(lv)
        leaves.append(lv)
    for (ev, pol, mask), maps in zip(case.windows, flows):
        ew.event_flow_association(maps, ev.to(dev), pol.to(dev), mask.to(dev))
    if case.overwrite:
        ew.overwrite_intermediate_flow(flows[-1])
    loss = ew()
    out = {}
    if case.nmaps == 1:
        images, persample, smooth = loss.grad_fn.saved_tensors[:3]
        n = 8 * case.B * case.H * case.W
        out["images"] = images[:n].double().cpu().numpy().reshape(2, 4, case.B, case.H * case.W)
        out["persample"] = persample.double().cpu().numpy().reshape(2, case.B, 4)
        out["smooth"] = smooth[:5].double().cpu().numpy()
        out["smooth_comb"] = float(smooth[5])
    (loss * case.g).backward()
    out["loss"] = float(loss.detach())
    out["loss_f32"] = loss.detach().cpu().numpy()

    def grad(x):
        if x.grad is None:
            return None
        g = x.grad.permute(0, 3, 1, 2) if case.noncontig else x.grad
        if case.noncontig:
            assert x.grad.shape == x.shape and x.grad.is_contiguous()
        return g.double().cpu().numpy()

    out["grads"] = [[grad(x) for x in lv] for lv in leaves]
    return out


# ---------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------
def _split(res):
    p = res["persample"]
    return {"images": res["images"], "Sp": p[:, :, 0], "Sn": p[:, :, 1], "lb": p[:, :, 3], "smooth": res["smooth"]}


def _gfree(case, res):
    free = case.free()
    vals = []
    for t, maps in enumerate(res["grads"]):
        m = free[t].numpy()[:, None].repeat(2, 1)
        for g in maps:
            vals.append(np.zeros(int(m.sum())) if g is None else g[m])
    return np.concatenate(vals)


def compare(case, ours, want, tag=None):
    """Errors of ``ours`` against ``want`` (the fp64 oracle): absolute worst for the elementwise quantities,
    relative for loss and grad; "mag": the largest magnitude of each elementwise quantity in ``want``."""
    r, mag = {}, {}
    if case.nmaps == 1:
        a, b = _split(ours), _split(want)
        for q in ("images", "Sp", "Sn", "lb", "smooth"):
            r[q] = float(np.abs(a[q] - b[q]).max())
            mag[q] = float(np.abs(b[q]).max())
        r["nz_equal"] = bool(np.array_equal(ours["persample"][:, :, 2], want["persample"][:, :, 2]))
        r["cnt_equal"] = bool(np.array_equal(ours["images"][:, :2], want["images"][:, :2]))
        r["finite"] = all(bool(np.isfinite(ours[k]).all()) for k in ("images", "persample", "smooth"))
    else:
        r["finite"] = True
    ga, gb = _gfree(case, ours), _gfree(case, want)
    r["gfree"], mag["gfree"] = float(np.abs(ga - gb).max()) if ga.size else 0.0, float(np.abs(gb).max()) if gb.size else 0.0
    r["loss"] = abs(ours["loss"] - want["loss"]) / max(abs(want["loss"]), 1e-300)
    r["finite"] = r["finite"] and bool(np.isfinite(ours["loss"]))
    worst, zero_ok = 0.0, True
    for mo, mw in zip(ours["grads"], want["grads"]):
        for go, gw in zip(mo, mw):
            if go is not None:
                r["finite"] = r["finite"] and bool(np.isfinite(go).all())
            if gw is None or not np.abs(gw).max() > 0:
                zero_ok = zero_ok and (go is None or float(np.abs(go).max()) == 0.0)
                continue
            if go is None:
                zero_ok = False
                continue
            worst = max(worst, float(np.linalg.norm(go - gw) / np.linalg.norm(gw)))
    r["grad"], r["grad_zero_ok"], r["mag"] = worst, zero_ok, mag
    if tag:
        print(f"\n[{tag} {case.cid}] loss {r['loss']:.3e} grad {r['grad']:.3e} | " +
              " ".join(f"{q} {r[q]:.3e}/{mag[q]:.3e}" for q in QUANTS if q in r))
    return r


def limits(cid, mag, widen=()):
    """The limit of every quantity at case ``cid``; ``widen``: which of ("loss", "grad") take 4 x REF_LOSS."""
    ref = REF_LOSS[cid]
    lim = {"loss": 4 * ref["loss"] if "loss" in widen else LOSS_RTOL,
           "grad": 4 * ref["grad"] if "grad" in widen else GRAD_TOL}
    for q in QUANTS:
        if q in mag:
            lim[q] = max(4 * ref[q], 2 * EPS32 * mag[q])
    return lim


def assert_case(case, r, lim):
    cid = case.cid
    assert r["finite"], cid
    if case.nmaps == 1:
        assert r["nz_equal"], (cid, "nz")
        if case.exact:
            assert r["cnt_equal"], (cid, "count images")
    assert r["grad_zero_ok"], (cid, "gradient of a window the oracle leaves at 0")
    for q in QUANTS + ("loss", "grad"):
        if q in r:
            assert r[q] <= lim[q], (cid, q, r[q], lim[q])


def ref_wide(cid, base_loss=LOSS_RTOL, base_grad=GRAD_TOL):
    """The fp32 oracle's own widening (test_loss_edges_cpu.py): the quantities whose committed figure
    exceeds the project's limit."""
    ref = REF_LOSS[cid]
    return tuple(q for q, b in (("loss", base_loss), ("grad", base_grad)) if ref[q] > b)


# ---------------------------------------------------------------------------
# refusals of the C entry points (no launch: the buffers may live on the host)
# ---------------------------------------------------------------------------
def refusal_calls(device):
    """(name, thunk -> return code, buffers that must stay untouched) per refused call.  Every buffer has
    the size its shape asks for and is pre-filled with 7."""
    import ctypes

    from snnflow import _lib

    lib = _lib.lib

    def make(B, H, W, offs, tf=None, bwd=False, misalign=False, M=None):
        T = len(offs) - 1
        tf = T if tf is None else tf
        M = offs[-1] if M is None else M
        Ta, tfa = min(T, _lib.MAX_WINDOWS), min(max(tf, 1), _lib.MAX_WINDOWS)
        Mb = max(M, offs[-1], 1)
        n_img = max(int(lib.snnflow_iwe_scratch_floats(min(B, 64), Mb, Ta, tfa, H, W)), 8) + 4
        n_acc = max(int(lib.snnflow_iwe_acc_doubles(min(B, 64), H, W, tfa)), 1)
        f32 = dict(dtype=torch.float32, device=device)
        bufs = {"images": torch.full((n_img,), 7.0, **f32), "acc": torch.full((n_acc,), 7.0, dtype=torch.float64, device=device),
                "persample": torch.full((2 * B * 4,), 7.0, **f32), "smooth": torch.full((8,), 7.0, **f32),
                "loss": torch.full((1,), 7.0, **f32), "g_flows": torch.full((B * tfa * 2 * H * W,), 7.0, **f32)}
        keep = {"ev": torch.zeros(B * Mb * 4, **f32), "pol": torch.zeros(B * Mb * 2, **f32),
                "flow": torch.zeros(B * 2 * H * W, **f32), "mask": torch.ones(B * H * W, **f32), "g": torch.ones(1, **f32)}
        a = _lib.IweLossArgs()
        a.B, a.M, a.T, a.H, a.W, a.tf = B, M, T, H, W, tf
        for k in range(Ta):
            a.events[k], a.pol[k] = keep["ev"].data_ptr(), keep["pol"].data_ptr()
        for t in range(tfa):
            a.flows[t], a.masks[t] = keep["flow"].data_ptr(), keep["mask"].data_ptr()
        for i, o in enumerate(offs[:_lib.MAX_WINDOWS + 1]):
            a.off[i] = o
        a.flow_scaling, a.weight, a.smoothing_mask, a.loss_scaling = float(max(H, W)), 0.001, 1, 1
        a.images = bufs["images"].data_ptr() + (4 if misalign else 0)
        a.acc, a.persample = bufs["acc"].data_ptr(), bufs["persample"].data_ptr()
        a.smooth, a.loss = bufs["smooth"].data_ptr(), bufs["loss"].data_ptr()

        def thunk():
            if bwd:
                return lib.snnflow_iwe_loss_bwd(ctypes.byref(a), keep["g"].data_ptr(), bufs["g_flows"].data_ptr(), None)
            return lib.snnflow_iwe_loss_fwd(ctypes.byref(a), None)

        return thunk, bufs, (a, keep)

    yield ("W=1792 backward",) + make(1, 1, 1792, [0, 4], bwd=True)
    yield ("HW=2^21+1 forward",) + make(1, 1, (1 << 21) + 1, [0, 4])
    yield ("HW=2^21+1 backward",) + make(1, (1 << 21) + 1, 1, [0, 4], bwd=True)
    yield ("B=65",) + make(65, 4, 4, [0, 4])
    yield ("T=65",) + make(1, 4, 4, list(range(66)))
    yield ("tf=2 of T=3",) + make(1, 4, 4, [0, 2, 4, 6], tf=2)
    yield ("tf=2 of T=3 backward",) + make(1, 4, 4, [0, 2, 4, 6], tf=2, bwd=True)
    yield ("misaligned images",) + make(1, 4, 4, [0, 4], misalign=True)
    yield ("offsets end before M",) + make(1, 4, 4, [0, 2, 3], M=4)


def assert_refusals(device):
    n = 0
    for name, thunk, bufs, _keep in refusal_calls(device):
        rc = thunk()
        assert rc == -1, (name, rc)  # SNNFLOW_E_ARG
        for k, v in bufs.items():
            assert bool((v == 7.0).all()), (name, k)
        n += 1
    return n


# ---------------------------------------------------------------------------
# Reference against reference: the fp32 CPU oracle against the fp64 oracle through compare(), per case
# (test_loss_edges_cpu.py recomputes and checks them; printed by ``python tests/loss_harness.py``).
# loss: relative; grad: worst relative L2; the others: worst absolute elementwise error.
# ---------------------------------------------------------------------------
REF_LOSS = {
    "tiny-w0.001": {"loss": 3.177e-08, "grad": 9.919e-07, "images": 1.762e-07, "Sp": 2.528e-07, "Sn": 1.614e-08, "lb": 2.488e-08, "smooth": 3.450e-07, "gfree": 1.355e-10},
    "band-w0.001": {"loss": 9.882e-08, "grad": 1.770e-07, "images": 0.000e+00, "Sp": 3.094e-05, "Sn": 2.217e-05, "lb": 6.823e-08, "smooth": 1.046e-05, "gfree": 1.571e-10},
    "ragged-uneven-w0.001": {"loss": 5.360e-08, "grad": 4.720e-04, "images": 1.464e-05, "Sp": 1.250e-04, "Sn": 7.604e-05, "lb": 8.916e-08, "smooth": 1.074e-05, "gfree": 2.254e-10},
    "ragged-equal-w0.001": {"loss": 6.262e-08, "grad": 3.693e-05, "images": 1.187e-05, "Sp": 3.858e-05, "Sn": 1.790e-05, "lb": 5.184e-08, "smooth": 1.165e-05, "gfree": 4.790e-10},
    "batch17-w0.001": {"loss": 1.841e-08, "grad": 2.632e-05, "images": 1.527e-06, "Sp": 8.033e-06, "Sn": 7.950e-06, "lb": 2.694e-07, "smooth": 7.097e-06, "gfree": 5.360e-10},
    "batch64-w0.001": {"loss": 3.836e-08, "grad": 2.010e-06, "images": 4.534e-07, "Sp": 1.475e-06, "Sn": 1.116e-06, "lb": 1.112e-07, "smooth": 1.036e-05, "gfree": 2.874e-09},
    "windows-w0.001": {"loss": 3.847e-09, "grad": 1.246e-04, "images": 3.241e-04, "Sp": 3.487e-05, "Sn": 8.493e-05, "lb": 1.460e-08, "smooth": 7.308e-05, "gfree": 5.873e-12},
    "windows-overwrite-w0.001": {"loss": 1.731e-09, "grad": 3.250e-05, "images": 3.058e-04, "Sp": 6.133e-05, "Sn": 5.886e-05, "lb": 2.831e-08, "smooth": 1.630e-06, "gfree": 3.317e-10},
    "wide1791-w0.001": {"loss": 7.140e-08, "grad": 2.041e-03, "images": 1.382e-04, "Sp": 5.847e-04, "Sn": 1.626e-04, "lb": 3.050e-07, "smooth": 7.312e-07, "gfree": 1.138e-10},
    "wide600-w0.001": {"loss": 1.027e-07, "grad": 4.308e-05, "images": 4.682e-05, "Sp": 1.912e-05, "Sn": 3.622e-05, "lb": 9.301e-08, "smooth": 6.807e-07, "gfree": 1.432e-10},
    "none-w0.001": {"loss": 1.820e-09, "grad": 1.502e-07, "images": 0.000e+00, "Sp": 0.000e+00, "Sn": 0.000e+00, "lb": 0.000e+00, "smooth": 7.111e-06, "gfree": 3.444e-10},
    "tiny-w1": {"loss": 4.959e-08, "grad": 1.147e-07, "images": 1.762e-07, "Sp": 2.528e-07, "Sn": 1.614e-08, "lb": 2.488e-08, "smooth": 3.450e-07, "gfree": 5.580e-08},
    "band-w1": {"loss": 2.402e-08, "grad": 1.130e-07, "images": 0.000e+00, "Sp": 3.094e-05, "Sn": 2.217e-05, "lb": 6.823e-08, "smooth": 1.046e-05, "gfree": 1.221e-07},
    "ragged-uneven-w1": {"loss": 8.013e-08, "grad": 2.189e-04, "images": 1.464e-05, "Sp": 1.250e-04, "Sn": 7.604e-05, "lb": 8.916e-08, "smooth": 1.074e-05, "gfree": 2.089e-07},
    "ragged-equal-w1": {"loss": 3.084e-08, "grad": 1.981e-05, "images": 1.187e-05, "Sp": 3.858e-05, "Sn": 1.790e-05, "lb": 5.184e-08, "smooth": 1.165e-05, "gfree": 4.931e-07},
    "batch17-w1": {"loss": 1.001e-08, "grad": 1.434e-05, "images": 1.527e-06, "Sp": 8.033e-06, "Sn": 7.950e-06, "lb": 2.694e-07, "smooth": 7.097e-06, "gfree": 5.217e-07},
    "batch64-w1": {"loss": 8.621e-08, "grad": 3.180e-07, "images": 4.534e-07, "Sp": 1.475e-06, "Sn": 1.116e-06, "lb": 1.112e-07, "smooth": 1.036e-05, "gfree": 2.892e-06},
    "windows-w1": {"loss": 1.721e-08, "grad": 1.228e-04, "images": 3.241e-04, "Sp": 3.487e-05, "Sn": 8.493e-05, "lb": 1.460e-08, "smooth": 7.308e-05, "gfree": 5.145e-09},
    "windows-overwrite-w1": {"loss": 3.041e-08, "grad": 1.423e-05, "images": 3.058e-04, "Sp": 6.133e-05, "Sn": 5.886e-05, "lb": 2.831e-08, "smooth": 1.630e-06, "gfree": 2.431e-07},
    "wide1791-w1": {"loss": 1.796e-08, "grad": 1.522e-03, "images": 1.382e-04, "Sp": 5.847e-04, "Sn": 1.626e-04, "lb": 3.050e-07, "smooth": 7.312e-07, "gfree": 1.147e-07},
    "wide600-w1": {"loss": 7.805e-08, "grad": 2.077e-05, "images": 4.682e-05, "Sp": 1.912e-05, "Sn": 3.622e-05, "lb": 9.301e-08, "smooth": 6.807e-07, "gfree": 1.153e-07},
    "none-w1": {"loss": 1.904e-08, "grad": 1.022e-07, "images": 0.000e+00, "Sp": 0.000e+00, "Sn": 0.000e+00, "lb": 0.000e+00, "smooth": 7.111e-06, "gfree": 3.301e-07},
    "opt-mask1-scale1-over0-w0.001-fsdef": {"loss": 6.067e-08, "grad": 5.114e-05, "images": 1.618e-05, "Sp": 4.622e-05, "Sn": 5.808e-05, "lb": 4.602e-08, "smooth": 8.053e-06, "gfree": 2.960e-10},
    "opt-mask1-scale1-over0-w0.001-fs20": {"loss": 5.409e-08, "grad": 3.231e-05, "images": 1.625e-05, "Sp": 6.693e-05, "Sn": 3.827e-05, "lb": 1.391e-07, "smooth": 8.053e-06, "gfree": 2.960e-10},
    "opt-mask1-scale1-over0-w1-fsdef": {"loss": 1.133e-08, "grad": 8.304e-06, "images": 1.618e-05, "Sp": 4.622e-05, "Sn": 5.808e-05, "lb": 4.602e-08, "smooth": 8.053e-06, "gfree": 3.009e-07},
    "opt-mask1-scale1-over0-w1-fs20": {"loss": 2.074e-08, "grad": 2.296e-06, "images": 1.625e-05, "Sp": 6.693e-05, "Sn": 3.827e-05, "lb": 1.391e-07, "smooth": 8.053e-06, "gfree": 3.009e-07},
    "opt-mask1-scale1-over1-w0.001-fsdef": {"loss": 3.997e-08, "grad": 8.942e-05, "images": 1.618e-05, "Sp": 4.771e-05, "Sn": 2.647e-05, "lb": 1.250e-07, "smooth": 6.958e-06, "gfree": 1.042e-09},
    "opt-mask1-scale1-over1-w0.001-fs20": {"loss": 7.974e-08, "grad": 1.272e-05, "images": 1.577e-05, "Sp": 8.526e-05, "Sn": 1.014e-04, "lb": 1.509e-07, "smooth": 6.958e-06, "gfree": 1.042e-09},
    "opt-mask1-scale1-over1-w1-fsdef": {"loss": 4.170e-08, "grad": 8.855e-06, "images": 1.618e-05, "Sp": 4.771e-05, "Sn": 2.647e-05, "lb": 1.250e-07, "smooth": 6.958e-06, "gfree": 1.093e-06},
    "opt-mask1-scale1-over1-w1-fs20": {"loss": 3.858e-08, "grad": 3.385e-07, "images": 1.577e-05, "Sp": 8.526e-05, "Sn": 1.014e-04, "lb": 1.509e-07, "smooth": 6.958e-06, "gfree": 1.093e-06},
    "opt-mask1-scale0-over0-w0.001-fsdef": {"loss": 8.431e-09, "grad": 5.115e-05, "images": 1.618e-05, "Sp": 4.622e-05, "Sn": 5.808e-05, "lb": 7.081e-05, "smooth": 8.053e-06, "gfree": 2.960e-10},
    "opt-mask1-scale0-over0-w0.001-fs20": {"loss": 5.399e-08, "grad": 3.241e-05, "images": 1.625e-05, "Sp": 6.693e-05, "Sn": 3.827e-05, "lb": 1.052e-04, "smooth": 8.053e-06, "gfree": 2.960e-10},
    "opt-mask1-scale0-over0-w1-fsdef": {"loss": 3.089e-08, "grad": 5.114e-05, "images": 1.618e-05, "Sp": 4.622e-05, "Sn": 5.808e-05, "lb": 7.081e-05, "smooth": 8.053e-06, "gfree": 3.009e-07},
    "opt-mask1-scale0-over0-w1-fs20": {"loss": 2.955e-08, "grad": 3.242e-05, "images": 1.625e-05, "Sp": 6.693e-05, "Sn": 3.827e-05, "lb": 1.052e-04, "smooth": 8.053e-06, "gfree": 3.009e-07},
    "opt-mask1-scale0-over1-w0.001-fsdef": {"loss": 1.085e-07, "grad": 8.996e-05, "images": 1.618e-05, "Sp": 4.771e-05, "Sn": 2.647e-05, "lb": 1.250e-04, "smooth": 6.958e-06, "gfree": 1.042e-09},
    "opt-mask1-scale0-over1-w0.001-fs20": {"loss": 3.171e-08, "grad": 1.275e-05, "images": 1.577e-05, "Sp": 8.526e-05, "Sn": 1.014e-04, "lb": 1.418e-04, "smooth": 6.958e-06, "gfree": 1.042e-09},
    "opt-mask1-scale0-over1-w1-fsdef": {"loss": 3.262e-08, "grad": 8.994e-05, "images": 1.618e-05, "Sp": 4.771e-05, "Sn": 2.647e-05, "lb": 1.250e-04, "smooth": 6.958e-06, "gfree": 1.093e-06},
    "opt-mask1-scale0-over1-w1-fs20": {"loss": 4.419e-08, "grad": 1.274e-05, "images": 1.577e-05, "Sp": 8.526e-05, "Sn": 1.014e-04, "lb": 1.418e-04, "smooth": 6.958e-06, "gfree": 1.093e-06},
    "opt-mask0-scale1-over0-w0.001-fsdef": {"loss": 7.258e-08, "grad": 5.113e-05, "images": 1.618e-05, "Sp": 4.622e-05, "Sn": 5.808e-05, "lb": 4.602e-08, "smooth": 1.421e-05, "gfree": 3.102e-10},
    "opt-mask0-scale1-over0-w0.001-fs20": {"loss": 6.669e-08, "grad": 3.230e-05, "images": 1.625e-05, "Sp": 6.693e-05, "Sn": 3.827e-05, "lb": 1.391e-07, "smooth": 1.421e-05, "gfree": 3.102e-10},
    "opt-mask0-scale1-over0-w1-fsdef": {"loss": 1.336e-09, "grad": 7.054e-06, "images": 1.618e-05, "Sp": 4.622e-05, "Sn": 5.808e-05, "lb": 4.602e-08, "smooth": 1.421e-05, "gfree": 2.936e-07},
    "opt-mask0-scale1-over0-w1-fs20": {"loss": 4.971e-08, "grad": 1.941e-06, "images": 1.625e-05, "Sp": 6.693e-05, "Sn": 3.827e-05, "lb": 1.391e-07, "smooth": 1.421e-05, "gfree": 2.936e-07},
    "opt-mask0-scale1-over1-w0.001-fsdef": {"loss": 1.896e-08, "grad": 8.942e-05, "images": 1.618e-05, "Sp": 4.771e-05, "Sn": 2.647e-05, "lb": 1.250e-07, "smooth": 5.440e-06, "gfree": 1.042e-09},
    "opt-mask0-scale1-over1-w0.001-fs20": {"loss": 1.015e-07, "grad": 1.272e-05, "images": 1.577e-05, "Sp": 8.526e-05, "Sn": 1.014e-04, "lb": 1.509e-07, "smooth": 5.440e-06, "gfree": 1.042e-09},
    "opt-mask0-scale1-over1-w1-fsdef": {"loss": 1.944e-08, "grad": 8.726e-06, "images": 1.618e-05, "Sp": 4.771e-05, "Sn": 2.647e-05, "lb": 1.250e-07, "smooth": 5.440e-06, "gfree": 1.093e-06},
    "opt-mask0-scale1-over1-w1-fs20": {"loss": 2.255e-08, "grad": 3.340e-07, "images": 1.577e-05, "Sp": 8.526e-05, "Sn": 1.014e-04, "lb": 1.509e-07, "smooth": 5.440e-06, "gfree": 1.093e-06},
    "opt-mask0-scale0-over0-w0.001-fsdef": {"loss": 5.981e-08, "grad": 5.115e-05, "images": 1.618e-05, "Sp": 4.622e-05, "Sn": 5.808e-05, "lb": 7.081e-05, "smooth": 1.421e-05, "gfree": 3.102e-10},
    "opt-mask0-scale0-over0-w0.001-fs20": {"loss": 3.827e-10, "grad": 3.240e-05, "images": 1.625e-05, "Sp": 6.693e-05, "Sn": 3.827e-05, "lb": 1.052e-04, "smooth": 1.421e-05, "gfree": 3.102e-10},
    "opt-mask0-scale0-over0-w1-fsdef": {"loss": 7.375e-08, "grad": 5.113e-05, "images": 1.618e-05, "Sp": 4.622e-05, "Sn": 5.808e-05, "lb": 7.081e-05, "smooth": 1.421e-05, "gfree": 2.936e-07},
    "opt-mask0-scale0-over0-w1-fs20": {"loss": 1.642e-08, "grad": 3.241e-05, "images": 1.625e-05, "Sp": 6.693e-05, "Sn": 3.827e-05, "lb": 1.052e-04, "smooth": 1.421e-05, "gfree": 2.936e-07},
    "opt-mask0-scale0-over1-w0.001-fsdef": {"loss": 9.010e-08, "grad": 8.996e-05, "images": 1.618e-05, "Sp": 4.771e-05, "Sn": 2.647e-05, "lb": 1.250e-04, "smooth": 5.440e-06, "gfree": 1.042e-09},
    "opt-mask0-scale0-over1-w0.001-fs20": {"loss": 1.258e-08, "grad": 1.275e-05, "images": 1.577e-05, "Sp": 8.526e-05, "Sn": 1.014e-04, "lb": 1.418e-04, "smooth": 5.440e-06, "gfree": 1.042e-09},
    "opt-mask0-scale0-over1-w1-fsdef": {"loss": 4.710e-08, "grad": 8.994e-05, "images": 1.618e-05, "Sp": 4.771e-05, "Sn": 2.647e-05, "lb": 1.250e-04, "smooth": 5.440e-06, "gfree": 1.093e-06},
    "opt-mask0-scale0-over1-w1-fs20": {"loss": 2.907e-08, "grad": 1.273e-05, "images": 1.577e-05, "Sp": 8.526e-05, "Sn": 1.014e-04, "lb": 1.418e-04, "smooth": 5.440e-06, "gfree": 1.093e-06},
    "ties-band-sparse": {"loss": 3.485e-08, "grad": 3.115e-06, "images": 0.000e+00, "Sp": 8.493e-07, "Sn": 6.090e-07, "lb": 1.807e-08, "smooth": 6.102e-06, "gfree": 1.577e-10},
    "ties-band-dense": {"loss": 2.861e-08, "grad": 1.372e-07, "images": 0.000e+00, "Sp": 1.338e-05, "Sn": 1.757e-05, "lb": 2.842e-08, "smooth": 9.634e-06, "gfree": 1.591e-10},
    "ties-band-zero": {"loss": 4.563e-08, "grad": 9.673e-08, "images": 0.000e+00, "Sp": 5.016e-06, "Sn": 7.991e-06, "lb": 4.130e-08, "smooth": 6.123e-07, "gfree": 0.000e+00},
    "ties-tiny-sparse": {"loss": 2.546e-08, "grad": 1.052e-07, "images": 0.000e+00, "Sp": 1.105e-07, "Sn": 8.000e-09, "lb": 3.926e-09, "smooth": 3.709e-07, "gfree": 9.625e-11},
    "ties-tiny-dense": {"loss": 3.912e-08, "grad": 1.235e-07, "images": 0.000e+00, "Sp": 1.137e-07, "Sn": 1.245e-06, "lb": 5.535e-08, "smooth": 3.126e-07, "gfree": 6.380e-11},
    "ties-tiny-zero": {"loss": 1.243e-07, "grad": 4.482e-08, "images": 0.000e+00, "Sp": 1.498e-08, "Sn": 4.078e-07, "lb": 2.050e-08, "smooth": 2.891e-09, "gfree": 0.000e+00},
    "content-padding": {"loss": 3.869e-08, "grad": 7.293e-05, "images": 1.125e-05, "Sp": 2.376e-05, "Sn": 4.405e-05, "lb": 4.483e-08, "smooth": 1.168e-05, "gfree": 5.058e-10},
    "content-patch": {"loss": 1.809e-08, "grad": 4.155e-06, "images": 2.004e-04, "Sp": 3.079e-06, "Sn": 4.015e-06, "lb": 1.750e-07, "smooth": 4.345e-06, "gfree": 1.835e-10},
    "content-far": {"loss": 7.494e-08, "grad": 6.641e-05, "images": 2.920e-05, "Sp": 3.933e-05, "Sn": 1.490e-05, "lb": 6.705e-08, "smooth": 1.325e-04, "gfree": 5.085e-10},
    "content-border": {"loss": 1.513e-08, "grad": 3.516e-05, "images": 3.387e-05, "Sp": 2.783e-05, "Sn": 1.754e-05, "lb": 1.208e-07, "smooth": 2.103e-05, "gfree": 2.171e-10},
    "call-upstream": {"loss": 8.391e-08, "grad": 3.220e-05, "images": 7.580e-06, "Sp": 2.910e-05, "Sn": 1.504e-05, "lb": 8.950e-08, "smooth": 1.381e-05, "gfree": 1.148e-06},
    "call-two-maps": {"loss": 8.154e-09, "grad": 7.834e-06, "gfree": 1.848e-07},
    "call-noncontig": {"loss": 1.639e-08, "grad": 7.952e-06, "images": 8.144e-06, "Sp": 3.199e-05, "Sn": 3.566e-05, "lb": 4.996e-08, "smooth": 6.226e-06, "gfree": 3.803e-07},
}


def ref_figures(cid):
    case = get_case(cid)
    r = compare(case, run_oracle(case, torch.float32), oracle64(cid))
    return {q: r[q] for q in ("loss", "grad") + QUANTS if q in r}, r


if __name__ == "__main__":
    print("REF_LOSS = {")
    for c in ALL_CASES:
        fig, _ = ref_figures(c)
        print(f'    "{c}": {{' + ", ".join(f'"{q}": {v:.3e}' for q, v in fig.items()) + "},")
    print("}")
