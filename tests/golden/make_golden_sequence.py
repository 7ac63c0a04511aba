"""Writes tests/golden/sequence_case.npz: what the reference's H5Loader cuts out of recordings.

    python tests/golden/make_golden_sequence.py REFERENCE_ROOT

Runs on the CPU.  The windows, rows, sequence indices, dt_input / dt_gt and (case L) the final
item dicts are the reference's own code (dataloader/h5.py H5Loader, dataloader/base.py,
dataloader/encodings.py).  h5py, hdf5plugin, torchvision.transforms and progress.bar are not
installed: in-memory stand-ins take their place (H5Loader uses File, __getitem__, attrs,
visititems and close of h5py only), and os.walk inside h5.py is patched to a fixed, sorted file
list before construction (the reference takes the directory order).  The synthetic recordings come
from tests/sequence_ref.py make_sequences(); they are stored too.

Cases (prefix of the keys; geometry 20x24, crop 12x16, pooled 10x12, window 101):
  E    events, no crop, B = 3, sequences (a, s90, b, c)
  Ec   events, crop 12x16, B = 3, sequences (a, s, b, c)
  T    time, window 0.125, B = 2
  G1 / G05 / G04   gtflow_dt1, B = 1, windows 1, 0.5, 0.4
  L    events + crop, three augmentations at 0.5 under a numpy seed, hot filter on, B = 3:
       the collated item dicts
The script asserts the conditions each case exists for.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import sequence_ref as sr  # noqa: E402

SEED = 20240917


class Attrs(dict):
    pass


class Dataset:
    def __init__(self, arr, attrs=None):
        self.arr = np.asarray(arr)
        self.attrs = Attrs(attrs or {})
        self.dtype = self.arr.dtype

    def __getitem__(self, k):
        v = self.arr[k]
        return v.copy() if isinstance(v, np.ndarray) else v

    def __len__(self):
        return len(self.arr)


class Group:
    def __init__(self, items):
        self.items = items

    def __getitem__(self, k):
        return self.items[k]

    def visititems(self, fn):
        for k in sorted(self.items):
            fn(k, self.items[k])


class File:
    registry = {}

    def __init__(self, path, mode="r"):
        self.d = File.registry[os.path.basename(path)]
        self.attrs = Attrs(self.d["attrs"])

    def __getitem__(self, k):
        return self.d[k]

    def close(self):
        pass


def install_stand_ins(ref_root):
    h5py = types.ModuleType("h5py")
    h5py.File = File
    sys.modules["h5py"] = h5py
    sys.modules["hdf5plugin"] = types.ModuleType("hdf5plugin")
    tv, tvt = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
    tv.transforms = tvt
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("torchvision.transforms", tvt)
    pg, pgb = types.ModuleType("progress"), types.ModuleType("progress.bar")
    pgb.Bar = object
    sys.modules["progress"], sys.modules["progress.bar"] = pg, pgb
    pkg = types.ModuleType("dataloader")   # dataloader/__init__.py is not run
    pkg.__path__ = [os.path.join(ref_root, "dataloader")]
    sys.modules["dataloader"] = pkg
    import dataloader.h5 as h5
    return h5


def as_file(s):
    flows = {f"{i:06d}": Dataset(m, {"timestamp": float(t)}) for i, (t, m) in enumerate(zip(s["flow_ts"], s["flow_maps"]))}
    return {"attrs": {"t0": s["t0"], "duration": s["duration"]}, "events/xs": Dataset(s["xs"]),
            "events/ys": Dataset(s["ys"]), "events/ts": Dataset(s["ts"]), "events/ps": Dataset(s["ps"].astype(bool)),
            "flow_dt1": Group(flows)}


def make_loader(h5, seqs, case, num_bins=2, augment=False, hot=False):
    mode, window, res, B, order, _, calls = case
    names = [f"{i}_{n}.h5" for i, n in enumerate(order)]
    File.registry = {f: as_file(seqs[n]) for f, n in zip(names, order)}
    real_walk = h5.os.walk
    h5.os.walk = lambda path: [(path, [], sorted(names))]   # the file order, fixed before construction
    try:
        ld = h5.H5Loader(sr.config(mode, window, res, B, augment, hot), num_bins=num_bins)
    finally:
        h5.os.walk = real_walk
    assert [os.path.basename(f) for f in ld.files] == names
    return ld, calls


def run_case(h5, seqs, name, rec, log):
    case = sr.CASES[name]
    mode, window, res, B, order, _, _ = case
    ld, calls = make_loader(h5, seqs, case)
    raw, resets, crops = [], [0] * B, []
    fmt, reset, crop = ld.event_formatting, ld.reset_sequence, ld.get_events_spatially_filtered

    def event_formatting(xs, ys, ts, ps):
        raw.append((np.asarray(xs).astype(np.int16), np.asarray(ys).astype(np.int16),
                    np.asarray(ts).astype(np.float64), np.asarray(ps).astype(np.uint8)))
        return fmt(xs, ys, ts, ps)

    def reset_sequence(batch):
        resets[batch] += 1
        return reset(batch)

    def spatially_filtered(file, batch, target):
        before = ld.batch_row[batch]
        r = crop(file, batch, target)
        crops.append((before, len(r[0]), ld.batch_row[batch], len(file["events/xs"])))
        return r

    ld.event_formatting, ld.reset_sequence, ld.get_events_spatially_filtered = event_formatting, reset_sequence, spatially_filtered
    R = {k: [] for k in ("counts", "rows", "idx", "new_seq", "restarts", "dt_input", "dt_gt", "flow_idx")}
    gt = mode.startswith("gtflow")
    for it in range(calls):
        ld.new_seq = False
        resets[:] = [0] * B
        n0 = len(raw)
        rows_before, idx_before = list(ld.batch_row), list(ld.batch_idx)
        dts, dgs, fl = [], [], []
        for b in range(B):      # per slot: custom_collate cannot stack unequal counts
            out = ld[b]
            dts.append(float(out["dt_input"]))
            dgs.append(float(out["dt_gt"]))
            f = -1
            if gt:
                f = int(np.ceil(ld.batch_row[b]))   # row + window, the value h5.py:352 rounds
                s = seqs[order[ld.batch_idx[b] % len(order)]]
                want = F.avg_pool2d(torch.from_numpy(s["flow_maps"][f]).unsqueeze(0), kernel_size=2, stride=2).squeeze(0)
                assert torch.equal(out["gtflow"], want), (name, it)
            fl.append(f)
        assert len(raw) - n0 == B
        R["counts"].append([len(r[0]) for r in raw[n0:]])
        R["rows"].append(list(ld.batch_row)); R["idx"].append(list(ld.batch_idx)); R["new_seq"].append(ld.new_seq)
        R["restarts"].append(list(resets)); R["dt_input"].append(dts); R["dt_gt"].append(dgs); R["flow_idx"].append(fl)
        log.append((name, it, rows_before, idx_before, list(resets)))
    for i, k in enumerate(("xs", "ys", "ts", "ps")):
        rec[f"{name}_raw_{k}"] = np.concatenate([r[i] for r in raw])
    rec[f"{name}_counts"] = np.array(R["counts"], np.int32)
    rec[f"{name}_rows"] = np.array(R["rows"], np.float64)
    rec[f"{name}_idx"] = np.array(R["idx"], np.int64)
    rec[f"{name}_new_seq"] = np.array(R["new_seq"], bool)
    rec[f"{name}_restarts"] = np.array(R["restarts"], np.int32)
    rec[f"{name}_dt_input"] = np.array(R["dt_input"], np.float64)
    rec[f"{name}_dt_gt"] = np.array(R["dt_gt"], np.float64)
    rec[f"{name}_flow_idx"] = np.array(R["flow_idx"], np.int64)
    return R, crops, order


def main():
    if len(sys.argv) != 2:
        sys.exit("usage: make_golden_sequence.py REFERENCE_ROOT  (a checkout of the reference project)")
    ref_root = sys.argv[1]
    sys.path.insert(0, ref_root)
    sys.dont_write_bytecode = True
    h5 = install_stand_ins(ref_root)
    torch.set_num_threads(1)
    seqs = sr.make_sequences(SEED)
    rec, log = {}, []
    for n, s in seqs.items():
        for k, v in s.items():
            rec[f"seq_{n}_{k}"] = np.asarray(v)
    W = sr.WINDOW

    # ---- E
    R, _, order = run_case(h5, seqs, "E", rec, log)
    rs, idx = np.array(R["restarts"]), np.array(R["idx"])
    assert rs[0, 1] >= 1, "E: slot 1 does not restart in the first call"
    assert ((rs > 0).sum(1) >= 2).any(), "E: no call in which two slots restart"
    assert (rs >= 2).any(), "E: no slot restarts twice in one call"
    assert (idx >= len(order)).any(), "E: batch_idx never wraps"
    assert (np.array(R["counts"]) == W).all()

    # ---- Ec
    R, crops, order = run_case(h5, seqs, "Ec", rec, log)
    sums = (2 * W, 6 * W, 11 * W)
    assert any(c < W and after - before >= 10 * W and after < n for before, c, after, n in crops), "Ec: 10x limit"
    assert any(c == W and after - before >= 6 * W for before, c, after, n in crops), "Ec: chunk doubling"
    assert any(after == n and (n - before) not in sums for before, c, after, n in crops), "Ec: end inside a chunk"
    assert any(c == W and after - before > W for before, c, after, n in crops), "Ec: row jump"
    assert np.array(R["restarts"]).sum() >= 3

    # ---- T
    R, _, order = run_case(h5, seqs, "T", rec, log)
    mode, window, _, B, _, nmax, _ = sr.CASES["T"]
    rows, idx, cnt, rs = np.array(R["rows"]), np.array(R["idx"]), np.array(R["counts"]), np.array(R["restarts"])
    seen = {"exact": False, "dup_edge": False, "empty": False, "restart": bool(rs.any())}
    for it in range(len(rows)):
        for b in range(B):
            s = seqs[order[idx[it, b] % len(order)]]
            r0 = rows[it, b] - window
            for x in (r0 + s["t0"], r0 + s["t0"] + window):
                i = sr.binary_search_array(s["ts"], x)
                seen["exact"] |= bool(0 <= i < len(s["ts"]) and s["ts"][i] == x)
                seen["dup_edge"] |= bool(0 < i < len(s["ts"]) and s["ts"][i - 1] == s["ts"][i])
            seen["empty"] |= bool(cnt[it, b] == 0 and rs[it, b] == 0)
    assert all(seen.values()), seen
    assert cnt.max() <= nmax, cnt.max()

    # ---- G
    for name in ("G1", "G05", "G04"):
        R, _, order = run_case(h5, seqs, name, rec, log)
        window = sr.CASES[name][1]
        rows, rs = np.array(R["rows"]), np.array(R["restarts"])
        assert rs.any(), f"{name}: no restart"
        assert (np.array(R["dt_gt"]) > 0).any() and (np.array(R["flow_idx"]) > 0).all()
        assert np.array(R["counts"]).max() <= sr.CASES[name][5]
        assert (np.array(R["counts"]) > 10).any()
        if name == "G04":
            r0 = rows[:, 0] - window
            assert (np.ceil(r0 + window) - np.floor(r0) > 1).any(), "G04: the idx1 - idx0 > 1 adjustment is not reached"

    # ---- L
    mode, window, res, B, order, _, calls = sr.L_CASE
    np.random.seed(sr.L_SEED)
    ld, calls = make_loader(h5, seqs, sr.L_CASE, num_bins=sr.L_BINS, augment=True, hot=True)
    resets = [0] * B
    reset = ld.reset_sequence

    def reset_sequence(batch):
        resets[batch] += 1
        return reset(batch)

    ld.reset_sequence = reset_sequence
    keys = ("event_cnt", "event_voxel", "event_mask", "event_list", "event_list_pol_mask", "dt_gt", "dt_input")
    L = {k: [] for k in keys + ("flags", "hot_events", "hot_idx", "restarts", "rows", "idx")}
    L["flags0"] = np.array([[bool(ld.batch_augmentation[m][b]) for m in sr.MECH] for b in range(B)])
    for it in range(calls):
        resets[:] = [0] * B
        out = ld.custom_collate([ld[b] for b in range(B)])
        for k in keys:
            L[k].append(out[k].numpy())
        L["flags"].append([[bool(ld.batch_augmentation[m][b]) for m in sr.MECH] for b in range(B)])
        L["hot_events"].append(torch.stack(ld.hot_events).numpy().astype(np.float32))
        L["hot_idx"].append(list(ld.hot_idx)); L["restarts"].append(list(resets))
        L["rows"].append(list(ld.batch_row)); L["idx"].append(list(ld.batch_idx))
    rs = np.array(L["restarts"])
    assert rs.sum() >= 2 and rs[1:].any(), "L: no restart after the first call"
    assert (rs >= 2).any()
    flags = np.array(L["flags"])
    assert flags.any() and not flags.all()
    assert any((np.abs(L["event_cnt"][i]).sum((1, 2, 3)) < W).any() for i in range(calls)), "L: the hot filter never acts"
    for k, v in L.items():
        rec[f"L_{k}"] = np.asarray(v)

    path = os.path.join(HERE, "sequence_case.npz")
    np.savez_compressed(path, **rec)
    size = os.path.getsize(path)
    print(f"sequence fixture written: {size} bytes, {len(rec)} arrays")
    assert size <= 200 * 1000, size


if __name__ == "__main__":
    main()
