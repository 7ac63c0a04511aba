"""On-device batch preparation: the reference loader's stages between "raw events of a window,
as read from the file" and the dict the loop consumes (``dataloader/h5.py:285-333, 373-437``,
``dataloader/base.py:71-127, 144-159, 237-256``), running on the HIP loader (csrc/loader.hip).

``BatchPreparer`` takes ``BaseDataLoader``'s constructor arguments and config keys, draws the
augmentation flags in its order, keeps the hot-pixel state on the device and turns the raw
``[B, N]`` event arrays of one window per batch slot into the collate-layout dict in one C-ABI
call (2-5 kernel launches, no host synchronisation, capturable into a HIP graph).  Reading the
file, ``dt_input`` / ``dt_gt`` and APS frames stay with the caller.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import SnnflowError, lib, ptr

_AUG_BITS = {"Horizontal": _lib.AUG_H, "Vertical": _lib.AUG_V, "Polarity": _lib.AUG_P}


class BatchPreparer:
    """``BaseDataLoader(config, num_bins, round_encoding)`` without the file reader.

    ``batch_augmentation[mechanism][slot]`` (bools) is drawn with ``np.random.random()`` exactly as
    ``base.py:31-37`` (constructor) and ``base.py:65-69`` (``reset_sequence``) draw it, so the same
    numpy seed gives the reference's flags.  ``hot_events`` [B, H0, W0] fp32 and ``hot_idx`` [B]
    int32 are device tensors (``None`` until a device is known); both, and the flags, are plain
    attributes the caller may overwrite."""

    def __init__(self, config, num_bins, round_encoding=False, device=None):
        self.config = config
        self.num_bins = int(num_bins)
        self.round_encoding = bool(round_encoding)
        ld = config["loader"]
        self.batch_size = int(ld["batch_size"])
        # base.py:24-27
        self.resolution = list(ld["resolution"] if config["data"]["mode"] == "events" else ld["std_resolution"])
        self.target_resolution = list(ld["resolution"])
        self.keep_gt_full_res = bool(ld.get("keep_gt_full_res", False))
        H0, W0 = self.resolution
        Ht, Wt = self.target_resolution
        # h5.py:291-314, 376-377: only the non-events modes pool, and only down
        self.pooled = config["data"]["mode"] != "events" and (Ht < H0 or Wt < W0)
        if self.pooled:
            if Ht > H0 or Wt > W0 or H0 % Ht or W0 % Wt:
                # the reference pools with (H0 // Ht, W0 // Wt) and silently returns another size
                raise SnnflowError(f"loader.resolution {self.target_resolution} must divide the full resolution "
                                   f"{self.resolution}")
        else:
            Ht, Wt = H0, W0
        self.out_resolution = [Ht, Wt]

        self.batch_augmentation = {}
        for mechanism in ld["augment"]:
            self.batch_augmentation[mechanism] = [False for _ in range(self.batch_size)]
        for i, mechanism in enumerate(ld["augment"]):
            for slot in range(self.batch_size):
                if np.random.random() < ld["augment_prob"][i]:
                    self.batch_augmentation[mechanism][slot] = True

        hf = config["hot_filter"]
        self.hot_enabled = bool(hf["enabled"])
        self.hot_max_px = int(hf["max_px"]) if self.hot_enabled else 0
        self.hot_min_obvs = int(hf["min_obvs"]) if self.hot_enabled else 0
        self.hot_max_rate = float(hf["max_rate"]) if self.hot_enabled else 0.0
        self.hot_events = None
        self.hot_idx = None
        self.device = None
        self._flags_host = None
        self._flags_dev = None
        self._scratch = None
        if device is None and torch.cuda.is_available():
            device = torch.device("cuda", torch.cuda.current_device())
        if device is not None:
            self._bind(torch.device(device))

    def _bind(self, device):
        if device.type != "cuda":
            raise SnnflowError(f"BatchPreparer needs a HIP device (got {device}); there is no CPU fallback")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        if self.hot_enabled:
            self.hot_events = torch.zeros(self.batch_size, *self.resolution, device=device)
            self.hot_idx = torch.zeros(self.batch_size, dtype=torch.int32, device=device)
        self._sync_flags()

    def _flag_words(self):
        words = [0] * self.batch_size
        for mechanism, flags in self.batch_augmentation.items():
            bit = _AUG_BITS.get(mechanism, 0)  # augment_events ignores any other mechanism (base.py:113-125)
            for slot in range(self.batch_size):
                if flags[slot]:
                    words[slot] |= bit
        return tuple(words)

    def _sync_flags(self):
        words = self._flag_words()
        if words != self._flags_host:
            t = torch.tensor(words, dtype=torch.int32)
            if self._flags_dev is None:
                self._flags_dev = t.to(self.device)
            else:
                self._flags_dev.copy_(t)
            self._flags_host = words

    def reset_sequence(self, slot):
        """``base.py:54-69``: zero the slot's hot-pixel state and redraw its augmentation flags."""
        if self.hot_enabled and self.hot_events is not None:
            self.hot_events[slot].zero_()
            self.hot_idx[slot].zero_()
        ld = self.config["loader"]
        for i, mechanism in enumerate(ld["augment"]):
            self.batch_augmentation[mechanism][slot] = bool(np.random.random() < ld["augment_prob"][i])

    def _field(self, t, name, shape):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            where = t.device if isinstance(t, torch.Tensor) else type(t).__name__
            raise SnnflowError(f"{name} must be a HIP device tensor (got {where}); there is no CPU fallback")
        if tuple(t.shape) != tuple(shape):
            raise SnnflowError(f"{name} must have shape {tuple(shape)} (got {tuple(t.shape)})")
        return t.to(torch.float32).contiguous()  # ts.astype(np.float32) of event_formatting (base.py:85-88)

    def prepare(self, xs, ys, ts, ps, counts=None, gtflow=None):
        """Raw events ``[B, N]`` of one window per slot (``ps`` in {0, 1}, ``ts`` in seconds), the
        valid events per slot ``counts`` [B] int32 (None: all N) and optionally ``gtflow``
        [B, 2, H0, W0] -> dict of event_cnt, event_voxel, event_mask, event_list (ts, y, x, p),
        event_list_pol_mask (and gtflow) in the collate layout (``base.py:261-278``)."""
        if not isinstance(ps, torch.Tensor) or ps.dim() != 2:
            raise SnnflowError("events must be [B, N] tensors")
        B, N = ps.shape
        if B != self.batch_size:
            raise SnnflowError(f"batch of {B} slots, loader.batch_size is {self.batch_size}")
        xs, ys, ts, ps = (self._field(t, n, (B, N)) for t, n in ((xs, "xs"), (ys, "ys"), (ts, "ts"), (ps, "ps")))
        dev = ps.device
        if self.device is None:
            self._bind(dev)
        elif dev != self.device:
            raise SnnflowError(f"events on {dev}, BatchPreparer on {self.device}")
        self._sync_flags()
        H0, W0 = self.resolution
        Ht, Wt = self.out_resolution
        keep = self.pooled and self.keep_gt_full_res
        a = _lib.LoaderArgs()
        a.B, a.N, a.H0, a.W0, a.Ht, a.Wt = B, N, H0, W0, Ht, Wt
        a.num_bins, a.round_ts, a.keep_gt_full_res = self.num_bins, 1 if self.round_encoding else 0, 1 if keep else 0
        a.hot_enabled, a.hot_max_px, a.hot_min_obvs = 1 if self.hot_enabled else 0, self.hot_max_px, self.hot_min_obvs
        a.hot_max_rate = self.hot_max_rate  # c_float rounds to fp32
        a.scale_y, a.scale_x = Ht / H0, Wt / W0  # h5.py:404-405: python ratio, rounded to fp32 by the multiply
        a.xs, a.ys, a.ts, a.ps = ptr(xs), ptr(ys), ptr(ts), ptr(ps)
        if counts is not None:
            if not counts.is_cuda or counts.dtype != torch.int32 or tuple(counts.shape) != (B,):
                raise SnnflowError("counts must be a [B] int32 HIP device tensor")
            counts = counts.contiguous()
            a.counts = ptr(counts)
        a.flags = ptr(self._flags_dev)
        out = {"event_cnt": torch.empty(B, 2, Ht, Wt, device=dev),
               "event_voxel": torch.empty(B, self.num_bins, Ht, Wt, device=dev),
               "event_mask": torch.empty(B, 1, *((H0, W0) if keep else (Ht, Wt)), device=dev),
               "event_list": torch.empty(B, N, 4, device=dev),
               "event_list_pol_mask": torch.empty(B, N, 2, device=dev)}
        if gtflow is not None:
            gtflow = self._field(gtflow, "gtflow", (B, 2, H0, W0))
            out["gtflow"] = torch.empty(B, 2, *((H0, W0) if keep else (Ht, Wt)), device=dev)
            a.gtflow_in, a.gtflow = ptr(gtflow), ptr(out["gtflow"])
        if self.hot_enabled:
            for t, name, shape, dt in ((self.hot_events, "hot_events", (B, H0, W0), torch.float32),
                                       (self.hot_idx, "hot_idx", (B,), torch.int32)):
                if not t.is_cuda or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
                    raise SnnflowError(f"{name} must be a contiguous {shape} {dt} HIP device tensor")
            a.hot_events, a.hot_idx = ptr(self.hot_events), ptr(self.hot_idx)
        n = lib.snnflow_loader_scratch_floats(B, N, H0, W0, Ht, Wt, self.num_bins, a.hot_enabled, a.keep_gt_full_res)
        if n < 0:
            _lib.check(int(n), "loader_scratch_floats")
        if self._scratch is None or self._scratch.numel() < n:
            self._scratch = torch.empty(int(n), device=dev)
        a.scratch = ptr(self._scratch)
        a.event_cnt, a.event_voxel, a.event_mask = ptr(out["event_cnt"]), ptr(out["event_voxel"]), ptr(out["event_mask"])
        a.event_list, a.pol_mask = ptr(out["event_list"]), ptr(out["event_list_pol_mask"])
        _lib.call("loader_prepare", lib.snnflow_loader_prepare, ctypes.byref(a), _lib.stream_ptr(dev))
        return out
