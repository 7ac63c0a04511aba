"""On-device sequence reading: the file side of the reference's ``H5Loader``
(``dataloader/h5.py:47-70, 138-283, 350-365, 449-545``) over recordings that live in device memory,
running on the HIP sequence reader (csrc/sequence.hip).

``EventSequence`` is one recording (13 bytes an event) resident on the device, ``SequenceReader``
keeps the per-slot state of ``H5Loader`` (row, running sequence counter) on the device and cuts the
next window of every batch slot in one C-ABI call (2 kernel launches, no host synchronisation,
capturable into a HIP graph), and ``SequenceLoader`` chains it to a ``BatchPreparer``: the drop-in
for ``H5Loader`` + ``DataLoader(collate_fn=custom_collate)``.  APS frames (``frames`` mode) and the
HDF5 format itself (beyond the few lines of ``EventSequence.from_h5``) stay with the caller.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import SnnflowError, lib, ptr
from .loader import BatchPreparer

_MODES = {"events": _lib.SEQ_EVENTS, "time": _lib.SEQ_TIME, "gtflow_dt1": _lib.SEQ_GTFLOW,
          "gtflow_dt4": _lib.SEQ_GTFLOW}


def _host(a, name):
    if a is None:
        return None
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.dtype == object:
        raise SnnflowError(f"{name} must be a numeric array")
    return a


def _default_device(device):
    if device is None:
        if not torch.cuda.is_available():
            return None
        return torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise SnnflowError(f"sequences live on a HIP device (got {device}); there is no CPU fallback")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


class EventSequence:
    """One recording: ``xs``, ``ys`` (int16 pixels), ``ts`` (float64, absolute), ``ps`` (uint8 in
    {0, 1}), ``t0`` and optionally the ground-truth maps of one ``flow_dt*`` group (``flow_ts`` [F]
    float64, ``flow_maps`` [F, 2, H0, W0] float32, in the order ``visititems`` yields them).
    Numpy arrays or tensors; validated on the host, then uploaded (at once when a HIP device is
    given or visible, otherwise when a reader binds the sequence to one)."""

    def __init__(self, xs, ys, ts, ps, t0, duration=None, flow_ts=None, flow_maps=None, device=None):
        xs, ys, ts, ps = (_host(a, n) for a, n in ((xs, "xs"), (ys, "ys"), (ts, "ts"), (ps, "ps")))
        for a, n in ((xs, "xs"), (ys, "ys"), (ts, "ts"), (ps, "ps")):
            if a.ndim != 1:
                raise SnnflowError(f"{n} must be one-dimensional (got shape {a.shape})")
        if not (len(xs) == len(ys) == len(ts) == len(ps)):
            raise SnnflowError(f"xs, ys, ts, ps differ in length: {len(xs)}, {len(ys)}, {len(ts)}, {len(ps)}")
        self.n = len(xs)
        for a, n in ((xs, "xs"), (ys, "ys")):
            if a.dtype.kind not in "iu":
                raise SnnflowError(f"{n} must hold integer pixel coordinates (got {a.dtype})")
            if self.n and (int(a.min()) < 0 or int(a.max()) > 32767):
                raise SnnflowError(f"{n} must be non-negative and fit int16")
        if self.n and not np.isin(ps, (0, 1)).all():
            raise SnnflowError("ps must be 0 or 1")
        ts = ts.astype(np.float64)
        if self.n > 1 and not (np.diff(ts) >= 0).all():
            raise SnnflowError("ts must be non-decreasing")
        self.t0 = float(t0)
        self.duration = None if duration is None else float(duration)
        self.last_ts = float(ts[-1]) if self.n else self.t0
        self.x_max = int(xs.max()) if self.n else -1
        self.y_max = int(ys.max()) if self.n else -1
        flow_ts, flow_maps = _host(flow_ts, "flow_ts"), _host(flow_maps, "flow_maps")
        if (flow_ts is None) != (flow_maps is None):
            raise SnnflowError("flow_ts and flow_maps go together")
        self.nflow, self.flow_shape = 0, None
        if flow_ts is not None:
            if flow_ts.ndim != 1 or flow_maps.ndim != 4 or flow_maps.shape[1] != 2 or len(flow_ts) != len(flow_maps):
                raise SnnflowError(f"flow_ts [F] and flow_maps [F, 2, H0, W0] expected (got {flow_ts.shape}, "
                                   f"{flow_maps.shape})")
            self.nflow, self.flow_shape = len(flow_ts), tuple(flow_maps.shape[2:])
            flow_ts, flow_maps = flow_ts.astype(np.float64), flow_maps.astype(np.float32)
        self._host = (xs.astype(np.int16), ys.astype(np.int16), ts, ps.astype(np.uint8), flow_ts, flow_maps)
        self._dev = None
        self.device = None
        device = _default_device(device)
        if device is not None:
            self.to(device)

    def to(self, device):
        """Upload to ``device`` (once; the host copies are dropped)."""
        device = _default_device(device)
        if device is None:
            raise SnnflowError("EventSequence needs a HIP device (none visible); there is no CPU fallback")
        if self._dev is None:
            self._dev = tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)
                              for a in self._host)
            self._host = None
            self.device = device
        elif device != self.device:
            raise SnnflowError(f"sequence on {self.device}, asked for {device}")
        return self

    def __len__(self):
        return self.n

    def _desc(self):
        xs, ys, ts, ps, flow_ts, flow_maps = self._dev
        d = _lib.SeqDesc()
        d.xs, d.ys, d.ts, d.ps = ptr(xs), ptr(ys), ptr(ts), ptr(ps)
        d.n, d.t0, d.last_ts, d.nflow = self.n, self.t0, self.last_ts, self.nflow
        d.flow_ts, d.flow_maps = ptr(flow_ts), ptr(flow_maps)
        return d

    @classmethod
    def from_npz(cls, path, device=None):
        """Keys ``xs, ys, ts, ps, t0`` and optionally ``duration, flow_ts, flow_maps``."""
        with np.load(path, allow_pickle=False) as f:
            opt = {k: f[k] for k in ("flow_ts", "flow_maps") if k in f}
            duration = float(f["duration"]) if "duration" in f else None
            return cls(f["xs"], f["ys"], f["ts"], f["ps"], float(f["t0"]), duration, device=device, **opt)

    @classmethod
    def from_h5(cls, path, flow_group=None, device=None):
        """The datasets ``H5Loader`` reads (``h5.py:129-133``: ``events/xs, ys, ts, ps``, ``attrs["t0"]``;
        ``:82-89``: the maps of ``flow_group`` = ``"flow_dt1"`` / ``"flow_dt4"`` in ``visititems`` order with
        their ``timestamp`` attributes).  Needs ``h5py``.  It is not installed where this project is
        developed, so this constructor has never been run against a real file: it is kept to the few lines
        that name the datasets."""
        try:
            import h5py
        except ImportError as e:
            raise ImportError("EventSequence.from_h5 needs h5py, which is not installed; convert the recording "
                              "to npz (xs, ys, ts, ps, t0[, flow_ts, flow_maps]) and use from_npz") from e
        with h5py.File(path, "r") as f:
            flow_ts = flow_maps = None
            if flow_group is not None:
                names, flow_ts = [], []

                def visit(name, obj):
                    if hasattr(obj, "dtype") and name not in names:
                        names.append(name)
                        flow_ts.append(obj.attrs["timestamp"])

                f[flow_group].visititems(visit)
                flow_maps = np.stack([f[flow_group][n][:] for n in names])
                flow_ts = np.asarray(flow_ts, np.float64)
            return cls(f["events/xs"][:], f["events/ys"][:], f["events/ts"][:], f["events/ps"][:], f.attrs["t0"],
                       f.attrs.get("duration"), flow_ts, flow_maps, device=device)


class SequenceReader:
    """The file-side state of ``H5Loader`` with ``sequences`` in place of ``self.files``: slot ``b``
    starts on ``sequences[b]`` at row 0 and moves to sequence ``max(batch_idx) + 1`` when its window
    cannot be cut (``h5.py:195-200, 241-263``).  ``next()`` returns ``xs, ys, ts, ps`` [B, N] fp32
    (zeros behind ``counts[b]``), ``counts`` [B] int32, ``dt_input``, ``dt_gt`` [B] float64,
    ``restarts`` [B] int32 and, in the gtflow modes, ``gtflow`` [B, 2, H0, W0]: what
    ``BatchPreparer.prepare`` takes.  N is ``data.window`` in ``events`` mode and ``max_events``
    otherwise."""

    def __init__(self, config, sequences, max_events=None, device=None):
        self.config = config
        mode = config["data"]["mode"]
        if mode == "frames":
            raise NotImplementedError("data.mode 'frames': APS frames are not read on the device")
        if mode not in _MODES:
            raise SnnflowError(f"unknown data.mode {mode!r}")
        self.mode = _MODES[mode]
        ld = config["loader"]
        self.batch_size = int(ld["batch_size"])
        self.std_resolution = [int(v) for v in ld["std_resolution"]]
        self.crop = list(self.std_resolution)
        window = config["data"]["window"]
        if not window > 0:
            raise SnnflowError(f"data.window must be positive (got {window})")
        if self.mode == _lib.SEQ_EVENTS:
            if int(window) != window:
                raise SnnflowError(f"data.window counts events in 'events' mode (got {window})")
            self.crop = [int(v) for v in ld["resolution"]]
            if self.crop[0] > self.std_resolution[0] or self.crop[1] > self.std_resolution[1]:
                raise SnnflowError(f"loader.resolution {self.crop} is larger than std_resolution {self.std_resolution}")
            self.max_events = int(window)
        else:
            if max_events is None:
                raise SnnflowError(f"max_events is required in {mode!r} mode (the padded window length)")
            self.max_events = int(max_events)
        if self.max_events <= 0:
            raise SnnflowError("max_events must be positive")
        self.window = float(window)
        self.sequences = list(sequences)
        if len(self.sequences) < self.batch_size:
            raise SnnflowError(f"{len(self.sequences)} sequences for {self.batch_size} batch slots")
        H0, W0 = self.std_resolution
        for i, s in enumerate(self.sequences):
            if not isinstance(s, EventSequence):
                raise SnnflowError(f"sequences[{i}] is not an EventSequence")
            # the kernels downstream scatter by these values: nothing outside the frame may reach them
            if s.x_max >= W0 or s.y_max >= H0:
                raise SnnflowError(f"sequences[{i}] has events outside std_resolution {self.std_resolution} "
                                   f"(max x {s.x_max}, max y {s.y_max})")
            if self.mode == _lib.SEQ_GTFLOW and s.nflow and s.flow_shape != (H0, W0):
                raise SnnflowError(f"sequences[{i}]: flow maps of {s.flow_shape}, std_resolution {self.std_resolution}")
        device = _default_device(device)
        if device is None:
            raise SnnflowError("SequenceReader needs a HIP device (none visible); there is no CPU fallback")
        self.device = device
        for s in self.sequences:
            s.to(device)
        B, N = self.batch_size, self.max_events
        descs = (_lib.SeqDesc * len(self.sequences))(*[s._desc() for s in self.sequences])
        self._descs = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(device)
        self._row = torch.zeros(B, dtype=torch.float64, device=device)                 # h5.py:54-56
        self._batch_idx = torch.arange(B, dtype=torch.int64, device=device)            # h5.py:53
        self.status = torch.zeros(B, dtype=torch.int32, device=device)
        self._scratch = torch.zeros(_lib.seq_scratch_words(B, N), dtype=torch.int64, device=device)

    def buffers(self):
        """A set of output tensors for ``next(out=...)``."""
        B, N, dev = self.batch_size, self.max_events, self.device
        out = {k: torch.empty(B, N, device=dev) for k in ("xs", "ys", "ts", "ps")}
        out["counts"] = torch.empty(B, dtype=torch.int32, device=dev)
        out["dt_input"] = torch.empty(B, dtype=torch.float64, device=dev)
        out["dt_gt"] = torch.empty(B, dtype=torch.float64, device=dev)
        out["restarts"] = torch.empty(B, dtype=torch.int32, device=dev)
        if self.mode == _lib.SEQ_GTFLOW:
            out["gtflow"] = torch.empty(B, 2, *self.std_resolution, device=dev)
        return out

    def next(self, out=None):
        """Cut the next window of every slot on the current stream; ``out``: tensors of ``buffers()``
        to write into (a fresh set otherwise)."""
        if out is None:
            out = self.buffers()
        a = _lib.SeqArgs()
        a.B, a.N, a.mode, a.nseq = self.batch_size, self.max_events, self.mode, len(self.sequences)
        a.H0, a.W0 = self.std_resolution
        a.Hc, a.Wc = self.crop
        a.window = self.window
        a.seqs, a.row, a.batch_idx, a.status = ptr(self._descs), ptr(self._row), ptr(self._batch_idx), ptr(self.status)
        a.scratch, a.scratch_words = ptr(self._scratch), self._scratch.numel()
        a.xs, a.ys, a.ts, a.ps = ptr(out["xs"]), ptr(out["ys"]), ptr(out["ts"]), ptr(out["ps"])
        a.counts, a.dt_input, a.dt_gt = ptr(out["counts"]), ptr(out["dt_input"]), ptr(out["dt_gt"])
        a.gtflow, a.restarts = ptr(out.get("gtflow")), ptr(out["restarts"])
        _lib.call("seq_next", lib.snnflow_seq_next, ctypes.byref(a), _lib.stream_ptr(self.device))
        return out

    def check(self):
        """Read the status words (synchronises) and raise if a window overflowed N or a slot found no
        usable sequence; the bits are cleared."""
        st = self.status.cpu().numpy()
        self.status.zero_()
        over = [b for b in range(len(st)) if st[b] & _lib.SEQ_OVERFLOW]
        stuck = [b for b in range(len(st)) if st[b] & _lib.SEQ_STUCK]
        if stuck:
            raise SnnflowError(f"slots {stuck} restarted {len(self.sequences)} times in one call without finding a "
                               "sequence that yields a window (the reference would loop forever)")
        if over:
            raise SnnflowError(f"slots {over}: a window held more than max_events = {self.max_events} events; "
                               "only the first were delivered")

    @property
    def batch_row(self):
        """``H5Loader.batch_row`` (read on demand, synchronises)."""
        return self._row.cpu().tolist()

    @property
    def batch_idx(self):
        """``H5Loader.batch_idx`` (read on demand, synchronises)."""
        return self._batch_idx.cpu().tolist()


class SequenceLoader:
    """``H5Loader(config, num_bins, round_encoding)`` + ``DataLoader(collate_fn=custom_collate)`` over
    resident sequences: an endless iterator of the collate-layout dict of ``BatchPreparer.prepare``
    plus ``dt_input`` and ``dt_gt`` [B] float64.  ``new_seq`` is set (never cleared here, as in the
    reference) when a slot changed sequence, ``seq_num`` counts the changes.  After every window the
    slots' restart counts (4 B bytes) are read and ``reset_sequence(slot)`` is called that often for
    ``slot in range(B)``: the order in which the reference draws from ``np.random``
    (``base.py:54-69``).  With ``prefetch`` the selection of window k+1 runs on a side stream
    while window k is prepared and consumed, and ``__next__`` waits on an event, not the device."""

    def __init__(self, config, sequences, num_bins, round_encoding=False, prefetch=True, device=None, max_events=None):
        self.config = config
        if max_events is None:
            max_events = config["data"].get("max_events")
        self.reader = SequenceReader(config, sequences, max_events=max_events, device=device)
        self.device = self.reader.device
        self.prep = BatchPreparer(config, num_bins, round_encoding, device=self.device)
        self.new_seq = False
        self.seq_num = 0
        self.epoch = 0      # base.py:17-19: counters the train loop keeps on its loader
        self.samples = 0
        self.files = self.reader.sequences  # the loop only takes len(data.files)
        self.prefetch = bool(prefetch)
        self._k = 0
        nbuf = 2 if self.prefetch else 1
        self._bufs = [self.reader.buffers() for _ in range(nbuf)]
        if self.prefetch:
            B = self.reader.batch_size
            self._pinned = [torch.empty(B, dtype=torch.int32).pin_memory() for _ in range(nbuf)]
            self._ready = [torch.cuda.Event() for _ in range(nbuf)]
            self._consumed = [None] * nbuf
            self._side = torch.cuda.Stream(self.device)
            self._side.wait_stream(torch.cuda.current_stream(self.device))  # uploads and state
            self._issued = -1

    @property
    def batch_augmentation(self):
        return self.prep.batch_augmentation

    @property
    def batch_row(self):
        return self.reader.batch_row

    @property
    def batch_idx(self):
        return self.reader.batch_idx

    def __iter__(self):
        return self

    def _issue(self, k):
        i = k % 2
        with torch.cuda.stream(self._side):
            if self._consumed[i] is not None:  # the prepare that last read this buffer
                self._side.wait_event(self._consumed[i])
            self.reader.next(self._bufs[i])
            self._pinned[i].copy_(self._bufs[i]["restarts"], non_blocking=True)
            self._ready[i].record(self._side)
        self._issued = k

    def _resets(self, restarts):
        nseq = len(self.reader.sequences)
        for slot, n in enumerate(restarts):
            for _ in range(min(n, nseq)):
                self.new_seq = True                                                    # h5.py:256-257
                self.seq_num += 1
                self.prep.reset_sequence(slot)
        if max(restarts) >= nseq:
            self.reader.check()

    def __next__(self):
        k, cur = self._k, torch.cuda.current_stream(self.device)
        if self.prefetch:
            i = k % 2
            if self._issued < k:
                self._issue(k)
            self._ready[i].synchronize()
            restarts = self._pinned[i].tolist()
            cur.wait_event(self._ready[i])
            self._issue(k + 1)
        else:
            i = 0
            self.reader.next(self._bufs[0])
            restarts = self._bufs[0]["restarts"].cpu().tolist()
        self._resets(restarts)
        buf = self._bufs[i]
        out = self.prep.prepare(buf["xs"], buf["ys"], buf["ts"], buf["ps"], buf["counts"], buf.get("gtflow"))
        out["dt_input"], out["dt_gt"] = buf["dt_input"].clone(), buf["dt_gt"].clone()
        if self.prefetch:
            ev = torch.cuda.Event()
            ev.record(cur)
            self._consumed[i] = ev
        self._k = k + 1
        return out
