"""On-device visual evaluation: the static renderers of the reference's ``Visualization``
(``utils/visualization.py``: ``flow_to_image`` :649-709, ``events_to_image`` :1037-1084,
``error_to_image`` :618-645, ``minmax_norm`` :1025-1034) and the exact ``np.percentile`` they
rest on, as HIP kernels (csrc/vis.hip).

Every function takes device tensors and returns device tensors on the caller's current
stream: the raw flow, IWE and count tensors never cross to the host, only finished frames do
(``.cpu()`` on the result).  Statistics are per image, never across the batch.  Inputs must be
finite.

Not covered (host drawing, left to the caller): ``flow_to_vector`` (cv2 arrows), the
``Visualization`` window / video class itself and its ``_upsample_frame`` (cv2's
nearest-neighbour resize).
"""
import ctypes

import torch

from . import _lib
from ._lib import lib, ptr


def _f32(t, name):
    _lib.require_device(t, name)
    return t.detach().contiguous()


def percentile(x, qs, fp64=False):
    """``np.percentile(plane, q)`` (method "linear") for every plane of ``x`` [N, ...] (planes
    flattened over the trailing dims) and every q of ``qs`` (at most 4), exact: [N, len(qs)],
    float32 -- numpy's result for a float32 plane -- or, with ``fp64``, float64 -- numpy's result
    for ``plane.astype(float64)``."""
    x = _f32(x, "x")
    qs = [float(q) for q in qs]
    if x.dim() < 1 or x.shape[0] == 0 or not 1 <= len(qs) <= _lib.VIS_MAX_Q:
        raise _lib.SnnflowError(f"percentile: x [N, ...] with N >= 1 and 1..{_lib.VIS_MAX_Q} percentages")
    N = x.shape[0]
    out = torch.empty(N, len(qs), dtype=torch.float64 if fp64 else torch.float32, device=x.device)
    a = _lib.PercentilesArgs()
    a.nplanes, a.n, a.nq, a.fp64 = N, x.numel() // N, len(qs), int(bool(fp64))
    a.x, a.out = ptr(x), ptr(out)
    for k, q in enumerate(qs):
        a.q[k] = q
    _lib.call("percentiles", lib.snnflow_percentiles, ctypes.byref(a), _lib.stream_ptr(x.device))
    return out


def flow_to_image(flow, uniform_v=None):
    """``Visualization.flow_to_image(flow[b, 0], flow[b, 1], uniform_v)`` for every image of
    ``flow`` [B, 2, H, W] (channel 0 = x): uint8 [B, H, W, 3]."""
    flow = _f32(flow, "flow")
    if flow.dim() != 4 or flow.shape[1] != 2:
        raise _lib.SnnflowError("flow_to_image: flow [B, 2, H, W]")
    B, _, H, W = flow.shape
    stats = torch.empty(B, 4, dtype=torch.float64, device=flow.device)
    out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=flow.device)
    a = _lib.FlowToImageArgs()
    a.B, a.H, a.W = B, H, W
    a.flow, a.stats, a.out = ptr(flow), ptr(stats), ptr(out)
    a.has_uniform_v, a.uniform_v = int(uniform_v is not None), float(uniform_v or 0.0)
    _lib.call("flow_to_image", lib.snnflow_flow_to_image, ctypes.byref(a), _lib.stream_ptr(flow.device))
    return out


def events_to_image(cnt, color_scheme="green_red"):
    """``Visualization.events_to_image`` for every image of ``cnt`` [B, 2, H, W] (per-pixel,
    per-polarity counts or IWE): float32 [B, H, W, 3] ("green_red") or [B, H, W] ("gray"), the
    reference's float64 values rounded to float32."""
    if color_scheme not in ("green_red", "gray"):
        raise ValueError(f"events_to_image: unknown color_scheme {color_scheme!r}")
    cnt = _f32(cnt, "cnt")
    if cnt.dim() != 4 or cnt.shape[1] != 2:
        raise _lib.SnnflowError("events_to_image: cnt [B, 2, H, W]")
    B, _, H, W = cnt.shape
    gray = color_scheme == "gray"
    stats = torch.empty(B, 2, 2, device=cnt.device)
    out = torch.empty((B, H, W) if gray else (B, H, W, 3), device=cnt.device)
    a = _lib.EventsToImageArgs()
    a.B, a.H, a.W, a.gray = B, H, W, int(gray)
    a.cnt, a.stats, a.out = ptr(cnt), ptr(stats), ptr(out)
    _lib.call("events_to_image", lib.snnflow_events_to_image, ctypes.byref(a), _lib.stream_ptr(cnt.device))
    return out


def error_to_image(err):
    """``Visualization.error_to_image`` (radians -> red gradient over [0, 180] degrees) of ``err``
    [B, H, W] or [H, W]: uint8 with a trailing 3.  The reference renders sample 0 of a batch;
    every sample is rendered here and ``[0]`` is the reference's image."""
    err = _f32(err, "err")
    if err.dim() not in (2, 3) or err.numel() == 0:
        raise _lib.SnnflowError("error_to_image: err [B, H, W] or [H, W]")
    out = torch.empty(tuple(err.shape) + (3,), dtype=torch.uint8, device=err.device)
    _lib.call("error_to_image", lib.snnflow_error_to_image, ptr(err), err.numel(), ptr(out),
              _lib.stream_ptr(err.device))
    return out


def minmax_norm(x):
    """``Visualization.minmax_norm`` (robust 1st / 99th percentile normalisation) of every plane
    of ``x`` [B, H, W]: float32 [B, H, W]."""
    x = _f32(x, "x")
    if x.dim() != 3 or x.numel() == 0:
        raise _lib.SnnflowError("minmax_norm: x [B, H, W]")
    B = x.shape[0]
    stats = torch.empty(B, 2, device=x.device)
    out = torch.empty_like(x)
    a = _lib.MinmaxNormArgs()
    a.B, a.n = B, x.numel() // B
    a.x, a.stats, a.out = ptr(x), ptr(stats), ptr(out)
    _lib.call("minmax_norm", lib.snnflow_minmax_norm, ctypes.byref(a), _lib.stream_ptr(x.device))
    return out
