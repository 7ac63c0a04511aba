"""Writes tests/golden/loader_case.npz: what the reference's loader makes of raw event windows.

    python tests/golden/make_golden_loader.py REFERENCE_ROOT

Runs on the CPU.  Everything up to the hot-pixel removal is the reference's own code
(dataloader/base.py event_formatting, augment_events, augment_flowmap, create_*_encoding,
create_polarity_mask, create_hot_mask; dataloader/encodings.py); only the part of
H5Loader.__getitem__ that sits behind the H5 reader is restated here, line by line:
h5.py:327-333 (hot-mask multiply) and h5.py:373-437 (avg_pool2d / scaled list tail).

Cases (prefix of the keys):
  A   events mode, 18x16, no pooling, flags (none, H+P, V), counts (101, 37, 1), dyadic timestamps
  Bk  gtflow_dt1 mode, 18x16 -> 6x8 (window 3x2), random gtflow, keep_gt_full_res True
  Bp  the same with keep_gt_full_res False
  C   hot-filter sequence: B's geometry, B = 2, 8 windows, slot 1 reset after window 5
  D   A with generic float64 timestamps
  F   augmentation flags under a numpy seed: after construction and after reset_sequence(slot)
The script asserts the coverage conditions each case exists for.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
MECH = ["Horizontal", "Vertical", "Polarity"]
H0, W0 = 18, 16
N = 101
BINS = 3


def import_dataloader(ref_root):
    """dataloader/__init__.py imports h5py (absent): register the package without running it."""
    pkg = types.ModuleType("dataloader")
    pkg.__path__ = [os.path.join(ref_root, "dataloader")]
    sys.modules["dataloader"] = pkg
    import dataloader.base as ref_base
    import dataloader.encodings as ref_enc
    return ref_enc, ref_base


def config(mode, resolution, batch_size, keep=False, hot=False, prob=(0.5, 0.5, 0.5)):
    return {"data": {"mode": mode},
            "loader": {"resolution": list(resolution), "std_resolution": [H0, W0], "batch_size": batch_size,
                       "augment": list(MECH), "augment_prob": list(prob), "keep_gt_full_res": keep},
            "hot_filter": {"enabled": hot, "max_px": 3, "min_obvs": 2, "max_rate": 0.8}}


def make_loader_class(ref_base):
    class Loader(ref_base.BaseDataLoader):
        def __getitem__(self, index):
            raise NotImplementedError

        def get_events(self, history):
            raise NotImplementedError

    return Loader


def reference_item(ld, xs, ys, ts, ps, flow, slot):
    """H5Loader.__getitem__ from "arrays read from the file" on, for one slot."""
    cfg = ld.config
    xs, ys, ts, ps = ld.event_formatting(xs, ys, ts, ps)                      # h5.py:289
    target_height, target_width = cfg["loader"]["resolution"]                 # h5.py:293
    if cfg["data"]["mode"] == "events":                                       # h5.py:308-314
        original_height, original_width = cfg["loader"]["resolution"]
    else:                                                                     # h5.py:298-307: the flow map's size
        original_height, original_width = cfg["loader"]["std_resolution"]
    xs, ys, ps = ld.augment_events(xs, ys, ps, slot)                          # h5.py:317
    event_cnt = ld.create_cnt_encoding(xs, ys, ps)                            # h5.py:320-324
    event_mask = ld.create_mask_encoding(xs, ys, ps)
    event_voxel = ld.create_voxel_encoding(xs, ys, ts, ps)
    event_list = ld.create_list_encoding(xs, ys, ts, ps)
    event_list_pol_mask = ld.create_polarity_mask(ps)
    hot_mask = None
    if cfg["hot_filter"]["enabled"]:                                          # h5.py:327-333
        hot_mask = ld.create_hot_mask(event_cnt, slot)
        hot_mask_voxel = torch.stack([hot_mask] * ld.num_bins, axis=2).permute(2, 0, 1)
        hot_mask_cnt = torch.stack([hot_mask] * 2, axis=2).permute(2, 0, 1)
        event_voxel = event_voxel * hot_mask_voxel
        event_cnt = event_cnt * hot_mask_cnt
        event_mask *= hot_mask.view((1, hot_mask.shape[0], hot_mask.shape[1]))
    flowmap = None
    if flow is not None:                                                      # h5.py:358-359
        flowmap = ld.augment_flowmap(flow.copy(), slot)
        flowmap = torch.from_numpy(flowmap.copy())
    output = {}
    keep_gt_full_res = cfg["loader"].get("keep_gt_full_res", False)           # h5.py:374
    if target_height < original_height or target_width < original_width:     # h5.py:376-377
        pool_h = original_height // target_height                             # h5.py:380-381
        pool_w = original_width // target_width
        k = (pool_h, pool_w)
        output["event_cnt"] = F.avg_pool2d(event_cnt.unsqueeze(0), kernel_size=k, stride=k).squeeze(0)    # :390
        output["event_voxel"] = F.avg_pool2d(event_voxel.unsqueeze(0), kernel_size=k, stride=k).squeeze(0)  # :391
        if keep_gt_full_res:                                                  # h5.py:394-399
            output["event_mask"] = event_mask
        else:
            output["event_mask"] = F.avg_pool2d(event_mask.unsqueeze(0), kernel_size=k, stride=k).squeeze(0)
        scaled_event_list = event_list.clone()                                # h5.py:402-410
        scaled_event_list[1, :] = scaled_event_list[1, :] * (target_height / original_height)
        scaled_event_list[2, :] = scaled_event_list[2, :] * (target_width / original_width)
        scaled_event_list[1, :] = torch.clamp(scaled_event_list[1, :], 0, target_height - 1)
        scaled_event_list[2, :] = torch.clamp(scaled_event_list[2, :], 0, target_width - 1)
        output["event_list"] = scaled_event_list
        output["event_list_pol_mask"] = event_list_pol_mask
        if flowmap is not None:                                               # h5.py:423-430
            if keep_gt_full_res:
                output["gtflow"] = flowmap
            else:
                output["gtflow"] = F.avg_pool2d(flowmap.unsqueeze(0), kernel_size=k, stride=k).squeeze(0)
    else:                                                                     # h5.py:431-442
        output["event_cnt"] = event_cnt
        output["event_voxel"] = event_voxel
        output["event_mask"] = event_mask
        output["event_list"] = event_list
        output["event_list_pol_mask"] = event_list_pol_mask
        if flowmap is not None:
            output["gtflow"] = flowmap
    output["_hot_mask"] = hot_mask
    output["_unclamped_y"] = event_list[1] * (target_height / original_height)
    output["_unclamped_x"] = event_list[2] * (target_width / original_width)
    return output


def reference_batch(ld, xs, ys, ts, ps, counts, flow):
    """All slots of one window, collated (base.py:261-278) with zero rows behind counts[b]."""
    B, n = xs.shape
    items = [reference_item(ld, xs[b, :counts[b]], ys[b, :counts[b]], ts[b, :counts[b]], ps[b, :counts[b]],
                            None if flow is None else flow[b], b) for b in range(B)]
    out = {}
    for key in ("event_cnt", "event_voxel", "event_mask") + (("gtflow",) if flow is not None else ()):
        out[key] = torch.stack([it[key] for it in items]).numpy().astype(np.float32)
    lst = np.zeros((B, n, 4), np.float32)
    pol = np.zeros((B, n, 2), np.float32)
    for b, it in enumerate(items):
        lst[b, :counts[b]] = it["event_list"].numpy().T
        pol[b, :counts[b]] = it["event_list_pol_mask"].numpy().T
    out["event_list"], out["event_list_pol_mask"] = lst, pol
    return out, items


def set_flags(ld, per_slot):
    """per_slot: one string of H / V / P letters per slot."""
    for m in MECH:
        ld.batch_augmentation[m] = [m[0] in s for s in per_slot]


def flags_array(ld):
    return np.array([[bool(ld.batch_augmentation[m][b]) for m in MECH] for b in range(len(ld.batch_augmentation[MECH[0]]))])


def raw_events(rng, counts, dyadic=True):
    """Integer pixel coordinates, half of them drawn from 12 pixels so that several share one;
    timestamps: integers whose valid part spans exactly 64 (dyadic once normalised and scaled
    by num_bins - 1), or generic float64 seconds."""
    B = len(counts)
    xs = rng.integers(0, W0, (B, N))
    ys = rng.integers(0, H0, (B, N))
    px = rng.integers(0, H0 * W0, 12)
    pick = rng.integers(0, 12, (B, N))
    use = rng.random((B, N)) < 0.5
    xs = np.where(use, px[pick] % W0, xs)
    ys = np.where(use, px[pick] // W0, ys)
    ps = rng.integers(0, 2, (B, N))
    if dyadic:
        ts = np.sort(rng.integers(0, 65, (B, N)), axis=1).astype(np.float64)
        for b, c in enumerate(counts):
            ts[b, 0], ts[b, c - 1] = 0, 64
            assert c == 1 or ts[b, :c].max() - ts[b, :c].min() == 64
        ts = ts + 1000.0
    else:
        ts = np.sort(12.3 + 0.05 * rng.random((B, N)), axis=1)
    return xs.astype(np.int16), ys.astype(np.int16), ts, ps.astype(np.int8)


def store(rec, prefix, out):
    for k, v in out.items():
        rec[f"{prefix}_{k}"] = v


def main():
    if len(sys.argv) != 2:
        sys.exit("usage: make_golden_loader.py REFERENCE_ROOT  (a checkout of the reference project)")
    ref_root = sys.argv[1]
    sys.path.insert(0, ref_root)
    _, ref_base = import_dataloader(ref_root)
    Loader = make_loader_class(ref_base)
    torch.set_num_threads(1)
    rng = np.random.default_rng(20240611)
    rec = {"res_full": np.array([H0, W0]), "res_pooled": np.array([6, 8]), "num_bins": np.array(BINS)}
    flags3 = ["", "HP", "V"]
    counts3 = np.array([101, 37, 1], np.int32)

    # ---- A: events mode, no pooling
    xs, ys, ts, ps = raw_events(rng, counts3)
    ld = Loader(config("events", [H0, W0], 3), BINS)
    set_flags(ld, flags3)
    out, items = reference_batch(ld, xs, ys, ts, ps, counts3, None)
    assert out["event_cnt"].sum(1).max() >= 3, "A: no pixel with 3 or more events"
    for b in range(2):
        assert set(np.unique(out["event_list"][b, :counts3[b], 3])) == {-1.0, 1.0}, "A: a polarity is missing"
    assert (out["event_list"][2, 0, 0] == 0) and out["event_voxel"][2].sum() != 0, "A: zero-range slot"
    rec.update(A_xs=xs, A_ys=ys, A_ts=ts, A_ps=ps, A_counts=counts3, A_flags=flags_array(ld))
    store(rec, "A", out)

    # ---- B: gtflow_dt1 mode, pooled 3x2, keep_gt_full_res True / False
    xs, ys, ts, ps = raw_events(rng, counts3)
    flow = rng.standard_normal((3, 2, H0, W0)).astype(np.float32)
    rec.update(B_xs=xs, B_ys=ys, B_ts=ts, B_ps=ps, B_counts=counts3, B_gtflow_in=flow)
    for prefix, keep in (("Bk", True), ("Bp", False)):
        ld = Loader(config("gtflow_dt1", [6, 8], 3, keep=keep), BINS)
        set_flags(ld, flags3)
        out, items = reference_batch(ld, xs, ys, ts, ps, counts3, flow)
        assert any((it["_unclamped_y"] > 5).any() for it in items), "B: y clamp not hit"
        assert any((it["_unclamped_x"] > 7).any() for it in items), "B: x clamp not hit"
        assert out["event_cnt"].shape == (3, 2, 6, 8)
        assert out["event_mask"].shape == ((3, 1, H0, W0) if keep else (3, 1, 6, 8))
        assert out["gtflow"].shape == ((3, 2, H0, W0) if keep else (3, 2, 6, 8))
        rec[f"{prefix}_flags"] = flags_array(ld)
        store(rec, prefix, out)

    # ---- C: hot-filter sequence.  Slot 0: five pixels fire in every window (rate 1: more than
    # max_px candidates, tied across the cut) and pixel q fires in windows 0-3 only (4 hits at
    # idx 5: rate == fp32(0.8), kept).  Slot 1: two pixels fire in every window (1..max_px
    # candidates); it is reset after window 5, so its windows 6, 7 are unfiltered again.
    T, Bc, Nc = 8, 2, 32
    hot0 = np.array([40, 41, 100, 101, 200]); q = 150; hot1 = np.array([7, 250])
    special = set(hot0.tolist() + [q] + hot1.tolist())
    free = np.array([p for p in range(H0 * W0) if p not in special])
    np.random.seed(7)
    ld = Loader(config("gtflow_dt1", [6, 8], Bc, keep=True, hot=True), BINS)
    set_flags(ld, ["", ""])
    cxs = np.zeros((T, Bc, Nc), np.int16); cys = np.zeros((T, Bc, Nc), np.int16)
    cts = np.zeros((T, Bc, Nc)); cps = np.zeros((T, Bc, Nc), np.int8)
    ccounts = np.full((T, Bc), Nc, np.int32)
    cflags = np.zeros((T, Bc, 3), bool)
    seen = {"cut_tie": False, "few": False, "exact_rate": False}
    seq = {}
    for t in range(T):
        for b in range(Bc):
            fixed = list(hot0) + ([q] if t < 4 else []) if b == 0 else list(hot1)
            fixed = fixed + fixed[:2]   # twice on some of them: hits count once per window
            bg = rng.choice(free, Nc - len(fixed), replace=True)
            pix = rng.permutation(np.concatenate([np.array(fixed), bg]))
            cxs[t, b], cys[t, b] = pix % W0, pix // W0
            k = np.sort(rng.integers(0, 65, Nc)); k[0], k[-1] = 0, 64
            cts[t, b] = 2000.0 + 100 * t + k
            cps[t, b] = rng.integers(0, 2, Nc)
        if t == 6:
            ld.reset_sequence(1)   # after window 5 (0-based: windows 0..5 done)
        cflags[t] = flags_array(ld)
        out, items = reference_batch(ld, cxs[t], cys[t], cts[t], cps[t], ccounts[t], None)
        for b in range(Bc):
            idx = ld.hot_idx[b]
            rate = (ld.hot_events[b] / idx).numpy()
            ncand = int((rate > np.float32(0.8)).sum())
            removed = int((items[b]["_hot_mask"] == 0).sum())
            if idx <= 2:
                assert removed == 0, "C: filtered before min_obvs"
            else:
                assert removed == min(ncand, 3)
                if ncand > 3:
                    cand = np.sort(rate[rate > np.float32(0.8)])[::-1]
                    seen["cut_tie"] |= bool(cand[2] == cand[3])
                if 1 <= ncand <= 3:
                    seen["few"] = True
            if b == 0 and idx == 5:
                r = rate.reshape(-1)[q]
                assert ld.hot_events[0].reshape(-1)[q] == 4
                seen["exact_rate"] = bool(r == np.float32(0.8)) and bool(items[0]["_hot_mask"].reshape(-1)[q] == 1)
        out["hot_events"] = torch.stack(ld.hot_events).numpy().astype(np.float32)
        out["hot_idx"] = np.array(ld.hot_idx, np.int32)
        for k_, v in out.items():
            seq.setdefault(k_, []).append(v)
    assert all(seen.values()), seen
    assert ld.hot_idx == [8, 2]
    store(rec, "C", {k_: np.stack(v) for k_, v in seq.items()})   # [T, ...] each
    rec.update(C_xs=cxs, C_ys=cys, C_ts=cts, C_ps=cps, C_counts=ccounts, C_flags=cflags,
               C_reset_before=np.array(6), C_reset_slot=np.array(1))

    # ---- D: A with generic timestamps
    xs, ys, ts, ps = raw_events(rng, counts3, dyadic=False)
    ld = Loader(config("events", [H0, W0], 3), BINS)
    set_flags(ld, flags3)
    out, _ = reference_batch(ld, xs, ys, ts, ps, counts3, None)
    rec.update(D_xs=xs, D_ys=ys, D_ts=ts, D_ps=ps, D_counts=counts3, D_flags=flags_array(ld))
    store(rec, "D", out)

    # ---- F: flags under a numpy seed
    seed, Bf, prob = 1234, 4, (0.5, 0.3, 0.7)
    np.random.seed(seed)
    ld = Loader(config("events", [H0, W0], Bf, prob=prob), BINS)
    f = [flags_array(ld)]
    for slot in range(Bf):
        ld.reset_sequence(slot)
        f.append(flags_array(ld))
    f = np.stack(f)
    assert f.any() and not f.all()
    rec.update(F_seed=np.array(seed), F_prob=np.array(prob), F_flags=f)

    path = os.path.join(HERE, "loader_case.npz")
    np.savez_compressed(path, **rec)
    print(f"loader fixture written: {os.path.getsize(path)} bytes, {len(rec)} arrays")


if __name__ == "__main__":
    main()
