"""Contrast-maximisation landscape for global flows: the reference's brute-force demo
(``tools/demo_iwe.py:46-102``) on ``snnflow_iwe_landscape`` (csrc/landscape.hip).

The demo fills a constant flow map per candidate ``(u, v)`` and runs ``EventWarping`` on it, 2500
times for its 50 x 50 heatmap.  A uniform flow needs no map and no gather, and its smoothness term
is the same constant for every candidate, so one call evaluates the loss' data term for all
candidates: ``loss_landscape`` returns it per sample, ``flow_heatmap`` the demo's heatmap and
``best_global_flow`` the learning-free global-motion estimate with its image of warped events.
Nothing here synchronises with the host.  One event window only (``max_ts = 1``), no gradients.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import lib, ptr
from .iwe import compute_pol_iwe


def _res(res):
    if len(res) != 2 or int(res[0]) < 1 or int(res[1]) < 1:
        raise _lib.SnnflowError(f"resolution {tuple(res)}, expected (H, W)")
    H, W = int(res[0]), int(res[1])
    if H * W > _lib.LANDSCAPE_MAX_PIXELS:
        raise _lib.SnnflowError(f"resolution {H} x {W}: H * W above 2^21 pixels")
    return H, W


def loss_landscape(event_list, pol_mask, res, candidates, flow_scaling=1.0, loss_scaling=True):
    """Data term of ``EventWarping`` (``loss/flow.py:197-261``: ``fw_loss + bw_loss``, no smoothness) per
    sample for K global flows: ``[B, K]`` float32 on the events' device.

    ``event_list`` [B, N, 4] = (ts, y, x, p) with ts in [0, 1] (one window), ``pol_mask`` [B, N, 2], both
    float32 device tensors; ``candidates`` any [K, 2] tensor or array of (u, v) = (horizontal, vertical)
    flow, not tied to a grid.  ``out[b, k]`` is what ``EventWarping(flow_scaling=flow_scaling)`` with weight
    0 gives for sample ``b`` alone on the constant map ``flow[:, 0] = u, flow[:, 1] = v``; it is
    bit-reproducible and does not depend on the other candidates of the call.  Events whose two polarity
    masks are 0 (padding) contribute nothing; a sample without a non-zero pixel in the forward or the
    backward image gives NaN (the reference's 0/0)."""
    H, W = _res(res)
    if not torch.is_tensor(event_list) or not torch.is_tensor(pol_mask):
        raise _lib.SnnflowError("loss_landscape: event_list and pol_mask must be tensors")
    if event_list.dim() != 3 or event_list.shape[2] != 4 or event_list.shape[0] < 1 or event_list.shape[1] < 1:
        raise _lib.SnnflowError(f"loss_landscape: events {tuple(event_list.shape)}, expected [B, N, 4] with B, N >= 1")
    B, N = event_list.shape[0], event_list.shape[1]
    if tuple(pol_mask.shape) != (B, N, 2):
        raise _lib.SnnflowError(f"loss_landscape: polarity masks {tuple(pol_mask.shape)}, expected {(B, N, 2)}")
    cand = candidates if torch.is_tensor(candidates) else torch.as_tensor(np.asarray(candidates))
    if cand.dim() != 2 or cand.shape[1] != 2 or cand.shape[0] < 1:
        raise _lib.SnnflowError(f"loss_landscape: candidates {tuple(cand.shape)}, expected [K, 2] with K >= 1")
    K = cand.shape[0]
    for name, t in (("event_list", event_list), ("pol_mask", pol_mask)):
        if t.dtype != torch.float32:
            raise _lib.SnnflowError(f"loss_landscape: {name} must be float32 (got {t.dtype})")
    _lib.require_device(event_list, "event_list")
    _lib.require_device(pol_mask, "pol_mask")
    dev = event_list.device
    s = _lib.stream_ptr(dev)
    ev, pol = event_list.detach().contiguous(), pol_mask.detach().contiguous()
    cand = cand.detach().to(device=dev, dtype=torch.float32).contiguous()
    need = lib.snnflow_iwe_landscape_scratch_floats(B, N, K, H, W)
    if need < 0:
        raise _lib.SnnflowError(f"loss_landscape: unsupported shape B, N, K, H, W = {(B, N, K, H, W)}")
    scratch = torch.empty(need, device=dev)
    out = torch.empty(B, K, device=dev)
    a = _lib.LandscapeArgs()
    a.B, a.N, a.K, a.H, a.W = B, N, K, H, W
    a.loss_scaling, a.flow_scaling = 1 if loss_scaling else 0, float(flow_scaling)
    a.events, a.pol, a.cand, a.out = ptr(ev), ptr(pol), ptr(cand), ptr(out)
    a.scratch, a.scratch_floats = ptr(scratch), need
    _lib.call("iwe_landscape", lib.snnflow_iwe_landscape, ctypes.byref(a), s)
    return out


def grid_candidates(x_maxdisp=64, y_maxdisp=64, heatmap_res=50):
    """The demo's candidates (``demo_iwe.py:47-48``) as ``(x_scale, y_scale, cand)``: ``cand[j * R + i] =
    (x_scale[i], y_scale[j])``, the flow of ``heatmap[j, i]``; float32."""
    R = int(heatmap_res)
    x_scale = np.linspace(-x_maxdisp, x_maxdisp, num=R).astype(np.float32)
    y_scale = np.linspace(-y_maxdisp, y_maxdisp, num=R).astype(np.float32)
    cand = np.stack([np.tile(x_scale, R), np.repeat(y_scale, R)], axis=1)
    return x_scale, y_scale, cand


def smoothness_constant(event_mask, config):
    """The smoothness term of ``EventWarping`` (``loss/flow.py:264-296``) on ANY constant flow map, before
    the weight: every flow difference is exactly 0, so each Charbonnier term is ``sqrt(1e-6)``, times the
    event-mask products with ``model.mask_output``; summed over the four spatial difference maps and
    divided by 5 components (``flow_dt`` is empty with one window, but counted) and 1 window.  A 0-dim
    tensor on the mask's device; runs on any device."""
    em = event_mask.float()
    c = torch.sqrt(torch.zeros((), device=em.device) ** 2 + 1e-6)
    pairs = ((em[:, :, :, :-1], em[:, :, :, 1:]), (em[:, :, :-1, :], em[:, :, 1:, :]),
             (em[:, :, :-1, :-1], em[:, :, 1:, 1:]), (em[:, :, 1:, :-1], em[:, :, :-1, 1:]))
    total = torch.zeros((), device=em.device)
    for a, b in pairs:
        d = c.expand(a.shape)
        if config["model"].get("mask_output", False):
            d = (a * b) * d
        total = total + d.sum()
    return total / 5 / 1


def _grid_call(event_list, pol_mask, event_mask, config, x_maxdisp, y_maxdisp, heatmap_res):
    if config["loss"].get("overwrite_intermediate", False):
        raise NotImplementedError("the landscape evaluates one event window: overwrite_intermediate is not supported")
    H, W = _res(config["loader"]["resolution"])
    if not torch.is_tensor(event_list) or event_list.dim() != 3:
        raise _lib.SnnflowError("event_list must be a [B, N, 4] tensor")
    B = event_list.shape[0]
    if not torch.is_tensor(event_mask) or tuple(event_mask.shape) != (B, 1, H, W):
        got = tuple(event_mask.shape) if torch.is_tensor(event_mask) else type(event_mask).__name__
        raise _lib.SnnflowError(f"event_mask {got}, expected {(B, 1, H, W)} (loader.resolution = {[H, W]})")
    x_scale, y_scale, cand = grid_candidates(x_maxdisp, y_maxdisp, heatmap_res)
    data = loss_landscape(event_list, pol_mask, (H, W), cand, flow_scaling=1.0)
    return (H, W), cand, data


def flow_heatmap(event_list, pol_mask, event_mask, config, x_maxdisp=64, y_maxdisp=64, heatmap_res=50):
    """The demo's heatmap (``demo_iwe.py:69-85``), ``[R, R]`` on the device: ``heatmap[j, i]`` is the full
    ``EventWarping(config, flow_scaling=1)`` loss of the constant flow ``(x_scale[i], y_scale[j])`` with
    ``x_scale = float32(linspace(-x_maxdisp, x_maxdisp, R))`` and likewise ``y_scale`` -- the data terms
    summed over the batch plus ``loss.flow_regul_weight`` times ``smoothness_constant``.  Honours
    ``loss.flow_regul_weight``, ``model.mask_output`` and ``loader.resolution``."""
    _, _, data = _grid_call(event_list, pol_mask, event_mask, config, x_maxdisp, y_maxdisp, heatmap_res)
    R = int(heatmap_res)
    heat = data.sum(dim=0)
    weight = float(config["loss"]["flow_regul_weight"])
    if weight != 0.0:
        heat = heat + weight * smoothness_constant(event_mask.to(heat.device), config)
    return heat.reshape(R, R)


def best_global_flow(event_list, pol_mask, event_mask, config, x_maxdisp=64, y_maxdisp=64, heatmap_res=50):
    """Per-sample minimum of the landscape over the demo's grid: ``(flow [B, 2] = (u, v), loss [B], iwe
    [B, 2, H, W])``, all on the device.  ``loss`` is the sample's data term at its best candidate (the
    smoothness constant does not move the minimum); NaN counts as +inf and ties go to the lowest flat
    index ``j * R + i``, like ``np.argmin``.  ``iwe`` is ``compute_pol_iwe`` on the winning constant map
    with ``flow_scaling=1, round_idx=True`` (``demo_iwe.py:94-102``).

    The reference indexes ``x_scale`` with the ROW of the argmin and ``y_scale`` with its column
    (``demo_iwe.py:88-91``) although ``heatmap[j, i]`` holds ``(x_scale[i], y_scale[j])``: off the
    diagonal it shows the transposed flow.  This function pairs them correctly: ``u = x_scale[i]``,
    ``v = y_scale[j]``."""
    (H, W), cand, data = _grid_call(event_list, pol_mask, event_mask, config, x_maxdisp, y_maxdisp, heatmap_res)
    dev = data.device
    K = data.shape[1]
    vals = torch.where(torch.isnan(data), torch.full_like(data, float("inf")), data)
    low = vals.min(dim=1, keepdim=True).values
    order = torch.arange(K, device=dev).expand_as(vals)
    best = torch.where(vals == low, order, torch.full_like(order, K)).min(dim=1).values
    flow = torch.as_tensor(cand, device=dev)[best]
    loss = data.gather(1, best[:, None])[:, 0]
    flowmap = flow[:, :, None, None].expand(-1, 2, H, W).contiguous()
    iwe = compute_pol_iwe(flowmap, event_list, (H, W), pol_mask[:, :, 0:1], pol_mask[:, :, 1:2], flow_scaling=1,
                          round_idx=True)
    return flow, loss, iwe
