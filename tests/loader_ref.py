"""Numpy restatement of the batch-preparation semantics (test support, no GPU, no torch).

One slot at a time, in fp32 throughout, in the order the reference loader works
(dataloader/h5.py:285-333, 373-437; dataloader/base.py:71-127, 144-159, 237-256):
formatting, augmentation, full-resolution encodings, hot-pixel filter, average pooling,
scaled and clamped event list, zero rows for padding.  tests/golden/loader_case.npz (written
by tests/golden/make_golden_loader.py from the reference's own code) pins it down.
"""
import numpy as np

F32 = np.float32
MECH = ("Horizontal", "Vertical", "Polarity")
TENSORS = ("event_cnt", "event_voxel", "event_mask", "event_list", "event_list_pol_mask")


def config(g, mode, pooled, batch_size, keep=False, hot=False, prob=(0.5, 0.5, 0.5)):
    """The config make_golden_loader.py built the case with."""
    return {"data": {"mode": mode},
            "loader": {"resolution": [int(v) for v in (g["res_pooled"] if pooled else g["res_full"])],
                       "std_resolution": [int(v) for v in g["res_full"]], "batch_size": batch_size,
                       "augment": list(MECH), "augment_prob": list(prob), "keep_gt_full_res": keep},
            "hot_filter": {"enabled": hot, "max_px": 3, "min_obvs": 2, "max_rate": 0.8}}


CASES = {"A": ("A", "events", False, False), "Bk": ("B", "gtflow_dt1", True, True),
         "Bp": ("B", "gtflow_dt1", True, False), "D": ("D", "events", False, False)}


def case_inputs(g, case):
    src = CASES[case][0]
    gt = g[f"{src}_gtflow_in"] if f"{src}_gtflow_in" in g else None
    return g[f"{src}_xs"], g[f"{src}_ys"], g[f"{src}_ts"], g[f"{src}_ps"], g[f"{src}_counts"], gt


def geometry(config):
    """(H0, W0), (Ht, Wt) of the outputs, pooled."""
    ld = config["loader"]
    events_mode = config["data"]["mode"] == "events"
    H0, W0 = ld["resolution"] if events_mode else ld["std_resolution"]
    Ht, Wt = ld["resolution"]
    pooled = (not events_mode) and (Ht < H0 or Wt < W0)
    if not pooled:
        Ht, Wt = H0, W0
    return (H0, W0), (Ht, Wt), pooled


def _scatter_add(img, pix, val):
    np.add.at(img.reshape(-1), pix, val.astype(F32))  # sequential fp32 adds in event order


def _pool(x, ph, pw):
    """F.avg_pool2d(kernel = stride = (ph, pw)): row-major fp32 sum of the window, then one division."""
    s = np.zeros(x.shape[:-2] + (x.shape[-2] // ph, x.shape[-1] // pw), F32)
    for dy in range(ph):
        for dx in range(pw):
            s = (s + x[..., dy::ph, dx::pw]).astype(F32)
    return (s / F32(ph * pw)).astype(F32)


def hot_mask(rate, idx, max_px, min_obvs, max_rate):
    """get_hot_event_mask (encodings.py:88-103): max_px rounds of argmax (first maximum = lowest
    flat index) while the maximum exceeds max_rate (compared in fp32)."""
    rate = rate.copy()
    mask = np.ones(rate.shape, F32)
    if idx > min_obvs:
        flat, m = rate.reshape(-1), mask.reshape(-1)
        for _ in range(max_px):
            i = int(np.argmax(flat))
            if flat[i] > F32(max_rate):
                flat[i] = 0
                m[i] = 0
            else:
                break
    return mask


class RefPreparer:
    """The semantics of snnflow.BatchPreparer on numpy arrays.  `flags`: [B][3] bools (H, V, P)."""

    def __init__(self, config, num_bins, round_encoding=False, flags=None):
        self.config, self.num_bins, self.round_encoding = config, num_bins, round_encoding
        self.full, self.out, self.pooled = geometry(config)
        self.keep = bool(config["loader"].get("keep_gt_full_res", False)) and self.pooled
        B = config["loader"]["batch_size"]
        self.flags = np.zeros((B, 3), bool) if flags is None else np.array(flags, bool)
        self.hot = dict(config["hot_filter"])
        self.hot_events = np.zeros((B,) + tuple(self.full), F32)
        self.hot_idx = np.zeros(B, np.int32)

    def reset_sequence(self, slot):
        self.hot_events[slot] = 0
        self.hot_idx[slot] = 0

    def _slot(self, b, xs, ys, ts, ps, flow):
        (H0, W0), (Ht, Wt) = self.full, self.out
        n, bins = len(xs), self.num_bins
        fh, fv, fp = self.flags[b]
        xs, ys, ts = xs.astype(F32), ys.astype(F32), ts.astype(F32)
        p = (ps.astype(F32) * F32(2) - F32(1)).astype(F32)
        if n > 0:  # base.py:89-98
            rng = F32(ts.max() - ts.min())
            ts = ((ts - ts.min()) / rng).astype(F32) if rng > 0 else np.zeros_like(ts)
        if fh:
            xs = (F32(W0 - 1) - xs).astype(F32)
        if fv:
            ys = (F32(H0 - 1) - ys).astype(F32)
        if fp:
            p = (p * F32(-1)).astype(F32)
        pix = ys.astype(np.int64) * W0 + xs.astype(np.int64)  # .long(): truncation
        cnt = np.zeros((2, H0, W0), F32)
        _scatter_add(cnt[0], pix, p * np.maximum(p, 0))
        _scatter_add(cnt[1], pix, p * np.minimum(p, 0))
        mask = np.zeros((1, H0, W0), F32)
        mask.reshape(-1)[pix] = np.abs(p)
        tb = (ts * F32(bins - 1)).astype(F32)
        if self.round_encoding:
            tb = np.rint(tb).astype(F32)  # half to even
        vox = np.zeros((bins, H0, W0), F32)
        k_ev = np.zeros((H0, W0), np.int64)      # events per pixel        } for the voxel bound of
        s_abs = np.zeros((bins, H0, W0))         # sum |p*w| per element   } the GPU tests (float64)
        np.add.at(k_ev.reshape(-1), pix, 1)
        for k in range(bins):
            w = np.maximum(F32(0), F32(1) - np.abs(tb - F32(k))).astype(F32)
            _scatter_add(vox[k], pix, p * w)
            np.add.at(s_abs[k].reshape(-1), pix, np.abs((p * w).astype(np.float64)))
        if self.hot["enabled"]:  # base.py:245-256
            self.hot_events[b] += (cnt[0] + cnt[1] > 0).astype(F32)
            self.hot_idx[b] += 1
            rate = (self.hot_events[b] / F32(self.hot_idx[b])).astype(F32)
            hm = hot_mask(rate, int(self.hot_idx[b]), self.hot["max_px"], self.hot["min_obvs"], self.hot["max_rate"])
            cnt, vox, mask = cnt * hm, vox * hm, mask * hm
            k_ev, s_abs = k_ev * (hm != 0), s_abs * hm
        ly, lx = ys, xs
        if flow is not None:  # base.py:151-158
            flow = flow.astype(F32).copy()
            if fh:
                flow = flow[:, :, ::-1].copy()
                flow[0] *= F32(-1)
            if fv:
                flow = flow[:, ::-1, :].copy()
                flow[1] *= F32(-1)
        if self.pooled:
            ph, pw = H0 // Ht, W0 // Wt
            cnt, vox = _pool(cnt, ph, pw), _pool(vox, ph, pw)
            k_ev = k_ev.reshape(Ht, ph, Wt, pw).sum((1, 3))
            s_abs = s_abs.reshape(bins, Ht, ph, Wt, pw).sum((2, 4)) / (ph * pw)
            if not self.keep:
                mask = _pool(mask, ph, pw)
                if flow is not None:
                    flow = _pool(flow, ph, pw)
            ly = np.clip((ys * F32(Ht / H0)).astype(F32), F32(0), F32(Ht - 1))  # h5.py:404-408
            lx = np.clip((xs * F32(Wt / W0)).astype(F32), F32(0), F32(Wt - 1))
        lst = np.stack([ts, ly, lx, p], 1).astype(F32)
        pol = np.stack([np.maximum(p, 0), -np.minimum(p, 0)], 1).astype(F32)
        return cnt, vox, mask, lst, pol, flow, k_ev, s_abs

    def prepare(self, xs, ys, ts, ps, counts=None, gtflow=None):
        """[B, N] arrays -> dict of fp32 arrays in the collate layout, plus voxel_K [B, Ht, Wt] (events
        in the element's pool window) and voxel_S [B, bins, Ht, Wt] (sum of their |p*w|, over the
        window size: the scale of the element's terms)."""
        B, N = xs.shape
        counts = np.full(B, N) if counts is None else counts
        out = {k: [] for k in ("event_cnt", "event_voxel", "event_mask", "event_list", "event_list_pol_mask",
                               "gtflow", "voxel_K", "voxel_S")}
        for b in range(B):
            c = int(counts[b])
            cnt, vox, mask, lst, pol, flow, k_ev, s_abs = self._slot(
                b, xs[b, :c], ys[b, :c], ts[b, :c], ps[b, :c], None if gtflow is None else gtflow[b])
            pad = np.zeros((N - c, 4), F32)
            for k, v in (("event_cnt", cnt), ("event_voxel", vox), ("event_mask", mask),
                         ("event_list", np.concatenate([lst.reshape(c, 4), pad])),
                         ("event_list_pol_mask", np.concatenate([pol.reshape(c, 2), pad[:, :2]])),
                         ("gtflow", flow), ("voxel_K", k_ev), ("voxel_S", s_abs)):
                out[k].append(v)
        if gtflow is None:
            del out["gtflow"]
        return {k: np.stack(v) for k, v in out.items()}


def voxel_bound(ref):
    """|got - want| <= 2 K 2^-24 S: the worst-case difference between two fp32 summation orders of the
    same K terms of total magnitude S (each order is within (K - 1) 2^-24 S of the exact sum)."""
    return 2.0 * ref["voxel_K"][:, None] * 2.0 ** -24 * ref["voxel_S"]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def assert_bit_equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = bits(got) != bits(want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at " \
                          f"{np.argwhere(bad)[0].tolist()}: {got[bad][0]!r} vs {want[bad][0]!r}"
