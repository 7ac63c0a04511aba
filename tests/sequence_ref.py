"""Numpy restatement of the sequence reader's semantics (test support, no GPU, no torch): the
file side of the reference's H5Loader (dataloader/h5.py:138-283, 350-365, 449-545;
dataloader/encodings.py:9-27), one slot at a time in the reference's order, on plain arrays.
tests/golden/sequence_case.npz (written by tests/golden/make_golden_sequence.py from the
reference's own H5Loader over in-memory stand-ins for h5py) pins it down; the synthetic
recordings of that fixture and of the GPU tests' second seed come from make_sequences() below.
"""
import numpy as np

H0, W0 = 20, 24            # std_resolution
CROP = (12, 16)
POOLED = (10, 12)
WINDOW = 101               # not a multiple of 64; crop chunks 202 -> 404 -> 505
MECH = ("Horizontal", "Vertical", "Polarity")


def config(mode, window, resolution, B, augment=False, hot=False):
    return {"data": {"path": "data", "mode": mode, "window": window},
            "loader": {"batch_size": B, "resolution": list(resolution), "std_resolution": [H0, W0],
                       "augment": list(MECH) if augment else [], "augment_prob": [0.5, 0.5, 0.5] if augment else [],
                       "keep_gt_full_res": False},
            "hot_filter": {"enabled": hot, "max_px": 3, "min_obvs": 2, "max_rate": 0.8}, "vis": {"bars": False}}


# case -> (mode, window, resolution, B, sequence order, max_events, calls)
CASES = {
    "E": ("events", WINDOW, (H0, W0), 3, ("a", "s90", "b", "c"), None, 27),
    "Ec": ("events", WINDOW, CROP, 3, ("a", "s", "b", "c"), None, 14),
    "T": ("time", 0.125, (H0, W0), 2, ("a", "s", "b", "c"), 640, 12),
    "G1": ("gtflow_dt1", 1, POOLED, 1, ("a", "s", "b", "c"), 640, 8),
    "G05": ("gtflow_dt1", 0.5, POOLED, 1, ("a", "s", "b", "c"), 640, 14),
    "G04": ("gtflow_dt1", 0.4, POOLED, 1, ("a", "s", "b", "c"), 640, 16),
}
L_CASE = ("events", WINDOW, CROP, 3, ("s", "a", "s", "b"), None, 5)
L_SEED, L_BINS = 11, 2


def _inside(n, rng):
    return rng.integers(4, 20, n), rng.integers(4, 16, n)          # x, y inside the 12 x 16 centre crop


def _outside(n, rng):
    x, y = rng.integers(0, W0, n), rng.integers(0, H0, n)
    bad = (x >= 4) & (x < 20) & (y >= 4) & (y < 16)
    x[bad] = rng.integers(0, 4, int(bad.sum()))                     # left margin
    return x, y


def make_sequences(seed, dyadic=True):
    """{name: dict(xs, ys, ts, ps, t0, duration, flow_ts, flow_maps)}.  a (2600 events) and c (2540)
    are uniform over the frame but for a stretch of ~20 % crop density in c, b (2530) has a
    stretch of 1100 events outside the crop, s has 150 events and s90 (case E only: a sequence that cannot
    yield a single window of 101) 90.  Timestamps: dyadic (multiples of 2^-12 from a dyadic t0, with
    runs of duplicates and a silent gap in a) or generic float64."""
    rng = np.random.default_rng(seed)
    out = {}
    spec = {"a": (2600, 1000.25, 1.0, 5), "s": (150, 3.5, 0.25, 2), "s90": (90, 3.5, 0.25, 2),
            "b": (2530, 50.5, 1.0, 4), "c": (2540, 7.125, 1.0, 4)}
    for name, (n, t0, dur, nflow) in spec.items():
        if not dyadic:
            t0 = t0 + float(rng.random()) * 0.1
        x, y = rng.integers(0, W0, n), rng.integers(0, H0, n)
        if name == "b":
            x[300:1400], y[300:1400] = _outside(1100, rng)           # the 10x search limit ends the search
        if name == "c":
            lo = slice(600, 1500)                                    # under 50 % density: chunk doubling
            xi, yi = _inside(900, rng)
            xo, yo = _outside(900, rng)
            pick = rng.random(900) < 0.2
            x[lo], y[lo] = np.where(pick, xi, xo), np.where(pick, yi, yo)
        if dyadic:
            k = np.sort(rng.integers(1, int(dur * 4096), n))
            k[k % 7 == 0] += 1                                       # more duplicates
            k = np.sort(k)
            if name == "a":                                          # a gap: [0.5, 0.625) keeps 8 events
                gap = (k >= 2048) & (k < 2560)
                keep = np.flatnonzero(gap)[:8]
                k[gap] = 2047
                k[keep] = 2048 + 40 * np.arange(len(keep))
                k = np.sort(k)
                k[np.searchsorted(k, 1024):np.searchsorted(k, 1024) + 3] = 1024   # a run across row + t0 = 0.25
            ts = t0 + k / 4096.0
        else:
            ts = np.sort(t0 + dur * rng.random(n))
        first = 0.3 * dur                                            # flow maps close together: short windows
        flow_ts = t0 + first + 0.04 * dur * (np.arange(nflow) + (0 if dyadic else rng.random(nflow) * 0.5))
        flow_maps = (rng.integers(-8, 9, (nflow, 2, H0, W0)) * 0.25).astype(np.float32)
        out[name] = dict(xs=x.astype(np.int16), ys=y.astype(np.int16), ts=ts.astype(np.float64),
                         ps=rng.integers(0, 2, n).astype(np.uint8), t0=float(t0), duration=float(dur),
                         flow_ts=flow_ts.astype(np.float64), flow_maps=flow_maps)
    return out


def sequences_from_fixture(g):
    return {n: {k: (float(g[f"seq_{n}_{k}"]) if k in ("t0", "duration") else g[f"seq_{n}_{k}"])
                for k in ("xs", "ys", "ts", "ps", "t0", "duration", "flow_ts", "flow_maps")}
            for n in ("a", "s", "s90", "b", "c")}


def binary_search_array(array, x):
    """encodings.py:9-27, iteratively: the first probe that hits an equal value, else the insertion point."""
    left, right = 0, len(array) - 1
    while left <= right:
        mid = left + (right - left) // 2
        if array[mid] == x:
            return mid
        if x < array[mid]:
            right = mid - 1
        else:
            left = mid + 1
    return left


class StuckError(RuntimeError):
    pass


class RefSequenceReader:
    """The semantics of snnflow.SequenceReader on numpy arrays.  next() -> dict of xs, ys, ts, ps
    [B, N] float32 (zero tails), counts, dt_input, dt_gt, restarts, flow_idx (-1: none) and gtflow."""

    def __init__(self, config, sequences, max_events=None):
        self.config, self.seqs = config, list(sequences)
        self.mode = config["data"]["mode"]
        self.window = config["data"]["window"]
        self.B = config["loader"]["batch_size"]
        self.N = int(self.window) if self.mode == "events" else int(max_events)
        self.batch_idx = list(range(self.B))
        self.batch_row = [0 for _ in range(self.B)]
        self.status = [0] * self.B
        res, std = config["loader"]["resolution"], config["loader"]["std_resolution"]
        self.cropped = self.mode == "events" and (res[0] < std[0] or res[1] < std[1])

    def _crop(self, s, b):                                                       # h5.py:449-545
        (sh, sw), (th, tw) = self.config["loader"]["std_resolution"], self.config["loader"]["resolution"]
        y0, x0 = (sh - th) // 2, (sw - tw) // 2
        y1, x1 = y0 + th, x0 + tw
        target = self.window
        cur, collected, chunk, searched = self.batch_row[b], 0, target * 2, 0
        take = []
        n = len(s["xs"])
        while collected < target and searched < target * 10:
            end = min(cur + chunk, n)
            if cur >= end:
                break
            xs, ys = s["xs"][cur:end], s["ys"][cur:end]
            m = (ys >= y0) & (ys < y1) & (xs >= x0) & (xs < x1)
            k = min(int(m.sum()), target - collected)
            if k > 0:
                take.extend((cur + np.where(m)[0][:k]).tolist())
                collected += k
            cur = end
            searched += chunk
            if collected < target * 0.5:
                chunk = min(chunk * 2, target * 5)
        if take:
            self.batch_row[b] = cur
        return np.array(take, np.int64), y0, x0

    def _slot(self, b):
        """One pass of H5Loader.__getitem__'s loop body -> (restart, event indices, y0, x0, flow index, dt_gt)."""
        s = self.seqs[self.batch_idx[b] % len(self.seqs)]
        row, window, n = self.batch_row[b], self.window, len(s["xs"])
        gt = self.mode in ("gtflow_dt1", "gtflow_dt4")
        y0 = x0 = 0
        flow, dt_gt = -1, 0.0
        sel = np.zeros(0, np.int64)
        restart = False
        if gt and int(np.ceil(row + window)) >= len(s["flow_ts"]):               # :195-200
            restart = True
        if not restart:
            if self.cropped:
                sel, y0, x0 = self._crop(s, b)
            else:
                if self.mode == "events":                                        # :149-150
                    i0, i1 = row, row + window
                elif self.mode == "time":                                        # :152-157
                    i0 = binary_search_array(s["ts"], row + s["t0"])
                    i1 = binary_search_array(s["ts"], row + s["t0"] + window)
                else:                                                            # :166-171
                    f0, f1 = int(np.floor(row)), int(np.ceil(row + window))
                    if window < 1.0 and f1 - f0 > 1:
                        f0 += f1 - f0 - 1
                    i0 = binary_search_array(s["ts"], s["flow_ts"][f0])
                    i1 = binary_search_array(s["ts"], s["flow_ts"][f1])
                    if window < 1.0:                                             # :221-236
                        c0, c1 = row - f0, row + window - f0
                        delta = i1 - i0
                        i1 = int(i0 + c1 * delta)
                        i0 = int(i0 + c0 * delta)
                sel = np.arange(n, dtype=np.int64)[i0:i1]
        if (self.mode == "events" and len(sel) < window) or (
                self.mode == "time" and row + window >= s["ts"][-1] - s["t0"]):  # :241-245
            restart = True
        if len(sel) <= 10:                                                       # :248-252
            sel = sel[:0]
        if not restart and gt:                                                   # :350-361
            flow = int(np.ceil(row + window))
            if flow > 0:
                dt_gt = s["flow_ts"][flow] - s["flow_ts"][flow - 1]
        return restart, s, sel, y0, x0, flow, dt_gt

    def next(self):
        B, N = self.B, self.N
        out = {k: np.zeros((B, N), np.float32) for k in ("xs", "ys", "ts", "ps")}
        out.update(counts=np.zeros(B, np.int32), dt_input=np.zeros(B), dt_gt=np.zeros(B),
                   restarts=np.zeros(B, np.int32), flow_idx=np.full(B, -1, np.int64))
        if self.mode in ("gtflow_dt1", "gtflow_dt4"):
            out["gtflow"] = np.zeros((B, 2) + tuple(self.config["loader"]["std_resolution"]), np.float32)
        for b in range(B):
            while True:
                restart, s, sel, y0, x0, flow, dt_gt = self._slot(b)
                if not restart:
                    break
                if out["restarts"][b] == len(self.seqs):
                    self.status[b] |= 2
                    raise StuckError(f"slot {b} found no usable sequence")
                out["restarts"][b] += 1                                          # :255-263
                self.batch_row[b] = 0
                self.batch_idx[b] = max(self.batch_idx) + 1
            ts = s["ts"][sel] - s["t0"]                                          # :133 (float64)
            if len(sel) > 0:
                out["dt_input"][b] = ts[-1] - ts[0]                              # :286-288
            c = min(len(sel), N)
            if len(sel) > N:
                self.status[b] |= 1
            out["xs"][b, :c] = (s["xs"][sel] - x0)[:c]
            out["ys"][b, :c] = (s["ys"][sel] - y0)[:c]
            out["ts"][b, :c] = ts.astype(np.float32)[:c]                         # base.py:87
            out["ps"][b, :c] = s["ps"][sel][:c]
            out["counts"][b] = c
            out["dt_gt"][b], out["flow_idx"][b] = dt_gt, flow
            if flow >= 0:
                out["gtflow"][b] = s["flow_maps"][flow]
            self.batch_row[b] += self.window                                     # :365
        return out


def case_reader_args(g_or_seqs, name):
    """(config, ordered sequence dicts, max_events, calls) of a fixture case (or of L)."""
    mode, window, res, B, order, nmax, calls = L_CASE if name == "L" else CASES[name]
    seqs = g_or_seqs if "a" in g_or_seqs else sequences_from_fixture(g_or_seqs)
    cfg = config(mode, window, res, B, augment=name == "L", hot=name == "L")
    return cfg, [seqs[n] for n in order], nmax, calls


def fixture_windows(g, name):
    """The recorded windows of a case, one dict per call, in the reader's layout."""
    _, window, _, B, _, nmax, calls = CASES[name]
    N = int(window) if nmax is None else nmax
    counts = g[f"{name}_counts"]
    at = 0
    for it in range(calls):
        out = {k: np.zeros((B, N), np.float32) for k in ("xs", "ys", "ts", "ps")}
        for b in range(B):
            c = int(counts[it, b])
            for k in ("xs", "ys", "ts", "ps"):
                out[k][b, :c] = g[f"{name}_raw_{k}"][at:at + c].astype(np.float32)
            at += c
        out.update(counts=counts[it], dt_input=g[f"{name}_dt_input"][it], dt_gt=g[f"{name}_dt_gt"][it],
                   restarts=g[f"{name}_restarts"][it], flow_idx=g[f"{name}_flow_idx"][it],
                   rows=g[f"{name}_rows"][it], idx=g[f"{name}_idx"][it], new_seq=bool(g[f"{name}_new_seq"][it]))
        yield out
    assert at == len(g[f"{name}_raw_xs"])


def assert_window_equal(got, want, what, rows=None, idx=None):
    """Bit for bit: fp32 rows, counts, restarts and the float64 dt_input / dt_gt (and rows, indices)."""
    for k in ("xs", "ys", "ts", "ps"):
        a, b = np.ascontiguousarray(got[k], np.float32), np.ascontiguousarray(want[k], np.float32)
        assert a.shape == b.shape and (a.view(np.int32) == b.view(np.int32)).all(), (what, k)
    for k in ("counts", "restarts"):
        assert (np.asarray(got[k]) == np.asarray(want[k])).all(), (what, k, got[k], want[k])
    for k in ("dt_input", "dt_gt"):
        a, b = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
        assert (a.view(np.int64) == b.view(np.int64)).all(), (what, k, a, b)
    if rows is not None:
        a, b = np.asarray(rows, np.float64), np.asarray(want["rows"], np.float64)
        assert (a.view(np.int64) == b.view(np.int64)).all(), (what, "rows", a, b)
    if idx is not None:
        assert (np.asarray(idx) == np.asarray(want["idx"])).all(), (what, "idx", idx, want["idx"])


class RefLoader:
    """RefSequenceReader + RefPreparer: the restatements chained as SequenceLoader chains the kernels."""

    def __init__(self, cfg, seqs, bins):
        import loader_ref

        self.rd = RefSequenceReader(cfg, seqs)
        self.prep = loader_ref.RefPreparer(cfg, bins)
        self.B = cfg["loader"]["batch_size"]

    def next(self, flags):
        raw = self.rd.next()
        for b in range(self.B):
            for _ in range(int(raw["restarts"][b])):
                self.prep.reset_sequence(b)
        self.prep.flags = flags
        return self.prep.prepare(raw["xs"], raw["ys"], raw["ts"], raw["ps"], raw["counts"])
