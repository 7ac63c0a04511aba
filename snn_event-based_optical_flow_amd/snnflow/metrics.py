"""Validation metrics with the reference's API (``loss/flow.py:306-937``: BaseValidationLoss,
AEE, NEE, AAE, NAAE, AE_ofMeans, AAE_Weighted, AAE_Filtered), the evaluation counterpart of
the training loss.

``AEE.forward`` runs the HIP kernels of csrc/eval.hip (per-pixel endpoint error,
validity, outliers, per-sample reduction); the other metrics share one pass
(``snnflow_flow_metrics``: every per-pixel term of every metric, per-block rows, a
fixed-order reduction), each class returning its own columns with the reference's
formulas and quirks (AAE's inverted cosine, batch-total outlier counts of AEE/NEE,
the unmasked numerator of AAE_Weighted).  The association bookkeeping is the
reference's (last flow map, event masks, ground truth, time scaling).

Error maps for visualisation (``loss/flow.py:443-594``) are opt-in: with ``error_maps`` set
(by ``metrics.heat_map`` / ``vis.enabled`` / ``vis.store`` in the config, or by assignment)
``AEE`` / ``AAE`` / ``NAAE.forward()`` also launch ``snnflow_error_maps`` (csrc/vis.hip), which
writes the metric's unmasked per-pixel error and adds the masked error and the mask into
device accumulators owned by the metric object (``get_final_error_heatmap``); ``AAE`` keeps
the map for ``get_error_map``.  The metric values are the same tensors either way, and with
the flag off nothing extra is launched.  ``save_error_heatmap`` is the reference's host-side
matplotlib figure; ``compute_window_events`` / ``compute_masked_window_flow`` are the images
the visual branch of ``eval_flow.py`` (:313-315) draws, to be rendered with ``snnflow.vis``.

Difference, documented: the reference multiplies the flow by ``dt_gt / dt_input`` with
plain broadcasting, which is only per-sample for a batch of one; here the ratio is applied
per sample for any batch size (identical for B = 1 and for scalar dt).
"""
import collections
import ctypes

import torch

from . import _lib
from ._lib import lib, ptr
from .iwe import compute_pol_iwe, interpolate

_AEE_SCRATCH_STREAMS = 8  # AEE scratch buffers kept per metric object (one per stream, LRU)


class BaseValidationLoss(torch.nn.Module):
    """``loss/flow.py:306-475`` bookkeeping."""

    def __init__(self, config, device, flow_scaling=128):
        super().__init__()
        self.res = config["loader"]["resolution"]
        self.flow_scaling = flow_scaling
        self.overwrite_intermediate = config["loss"].get("overwrite_intermediate", False)
        self.device = device
        vis_cfg = config.get("vis") or {}
        self.error_maps = bool((config.get("metrics") or {}).get("heat_map") or vis_cfg.get("enabled")
                               or vis_cfg.get("store"))
        self._aggregated_error_map = None  # device [H, W]: sum of error * mask (reset() keeps these, as
        self._aggregated_mask_map = None   # the reference's does; reset_error_heatmap() clears them)
        self._last_error_map = None
        self._error_map_dev = None
        self.reset()

    def reset(self):
        self._passes = 0
        self._event_list = None
        self._pol_mask_list = None
        self._flow_map = None
        self._event_mask = None
        self._gtflow = None

    @property
    def num_events(self):
        return 0 if self._event_list is None else self._event_list.shape[1]

    def event_flow_association(self, flow_list, inputs):
        event_list = inputs["event_list"].to(self.device)
        pol_mask = inputs["event_list_pol_mask"].to(self.device)
        event_mask = inputs["event_mask"].to(self.device)
        gtflow = inputs["gtflow"].to(self.device) if "gtflow" in inputs else None
        flow = flow_list[-1]
        if self._event_list is None:
            self._event_list = event_list
            self._pol_mask_list = pol_mask
            self._event_mask = event_mask
            self._flow_map = []
        else:
            event_list = event_list.clone()
            event_list[:, :, 0:1] += self._passes
            self._event_list = torch.cat([self._event_list, event_list], dim=1)
            self._pol_mask_list = torch.cat([self._pol_mask_list, pol_mask], dim=1)
            self._event_mask = torch.cat([self._event_mask, event_mask], dim=1)
        self._flow_map.append(flow.reshape(flow.shape[0], 2, self.res[0], self.res[1]))
        self._gtflow = gtflow
        self._dt_input = inputs["dt_input"]
        self._dt_gt = inputs["dt_gt"]
        self._passes += 1

    def overwrite_intermediate_flow(self, flow_list):
        flow = flow_list[-1]
        self._flow_map = [flow.reshape(flow.shape[0], 2, self.res[0], self.res[1])]
        m = torch.sum(self._event_mask, dim=1, keepdim=True)
        m[m > 1] = 1
        self._event_mask = m

    def get_error_map(self):
        """``:443-452``: the last unmasked per-pixel error [B, H, W] as a numpy array (AAE with
        ``error_maps`` set), else None."""
        if self._last_error_map is not None:
            return self._last_error_map.detach().cpu().numpy()
        return None

    def last_error_map(self):
        """The unmasked per-pixel error [B, H, W] of the last ``forward()`` as a device tensor (AEE,
        AAE and NAAE with ``error_maps`` set; feeds ``snnflow.vis.error_to_image`` without a host
        round trip), else None."""
        return self._error_map_dev

    def _error_maps(self, metric):
        """The metric's unmasked error map [B, H, W] of the current association state, its masked
        sum and the mask added into the aggregate (one launch)."""
        flow = self._flow_map[-1].float().contiguous()
        B, _, H, W = flow.shape
        gt = self._gtflow.float().contiguous()
        mask = self._event_mask[:, -1, :, :].float().contiguous()
        ratio = _dt_ratio(self, B, flow.device)
        if self._aggregated_error_map is None:
            self._aggregated_error_map = torch.zeros(H, W, device=flow.device)
            self._aggregated_mask_map = torch.zeros(H, W, device=flow.device)
        err = torch.empty(B, H, W, device=flow.device)
        a = _lib.ErrorMapsArgs()
        a.B, a.H, a.W, a.metric = B, H, W, metric
        a.flow, a.gtflow, a.event_mask, a.dt_ratio = ptr(flow), ptr(gt), ptr(mask), ptr(ratio)
        a.flow_scaling = float(self.flow_scaling)
        a.err, a.sum, a.count = ptr(err), ptr(self._aggregated_error_map), ptr(self._aggregated_mask_map)
        _lib.call("error_maps", lib.snnflow_error_maps, ctypes.byref(a), _lib.stream_ptr(flow.device))
        self._error_map_dev = err
        return err

    def accumulate_error_heatmap(self, error_map, mask_map):
        """``:489-511`` on device tensors [B, H, W]: adds sum_b error * mask and sum_b mask into
        the aggregate (the metrics' own ``forward`` does this in its kernel)."""
        error_map = error_map.detach().float()
        mask_map = mask_map.detach().float().to(error_map.device)
        batch_error_sum = (error_map * mask_map).sum(dim=0)
        batch_sample_count = mask_map.sum(dim=0)
        if self._aggregated_error_map is None:
            self._aggregated_error_map = batch_error_sum
            self._aggregated_mask_map = batch_sample_count
        else:
            self._aggregated_error_map += batch_error_sum
            self._aggregated_mask_map += batch_sample_count

    def get_final_error_heatmap(self):
        """``:513-525``: (sum / (count + 1e-9), count) as CPU tensors [H, W], or (None, None)."""
        if self._aggregated_error_map is None or self._aggregated_mask_map is None:
            return None, None
        count = self._aggregated_mask_map.cpu()
        return self._aggregated_error_map.cpu() / (count + 1e-9), count

    def reset_error_heatmap(self):
        """``:589-594``."""
        self._aggregated_error_map = None
        self._aggregated_mask_map = None

    def save_error_heatmap(self, save_path, title="Error Heatmap", cmap="jet", **kwargs):
        """``:527-587`` on the host (matplotlib, Agg): the averaged error clipped to its 95th
        percentile, pixels without samples blank.  Extra keywords (``eval_flow.py:381-388`` passes
        ``mag_threshold``, ``show_magnitude_overlay``, ...) are accepted and ignored.  False
        without data."""
        averaged_error, pixel_count = self.get_final_error_heatmap()
        if averaged_error is None:
            print("No error heatmap available")
            return False
        import matplotlib

        matplotlib.use("Agg")
        import matplotlib.pyplot as plt

        error_vis = averaged_error.clone().float()
        error_vis[pixel_count == 0] = float("nan")
        valid_errors = error_vis[pixel_count > 0]
        if valid_errors.numel() > 0:
            p95 = torch.quantile(valid_errors, 0.95)
            error_vis = torch.clamp(error_vis, max=p95)
        fig, ax = plt.subplots(figsize=(12, 10))
        im = ax.imshow(error_vis.numpy(), cmap=cmap, aspect="auto")
        ax.set_title(title, fontsize=14)
        ax.set_xlabel("Width (pixels)")
        ax.set_ylabel("Height (pixels)")
        plt.colorbar(im, ax=ax, label="Average Error (clipped to 95th percentile)")
        ax.grid(True, alpha=0.3)
        plt.savefig(save_path, dpi=150, bbox_inches="tight")
        plt.close(fig)
        print(f"Heatmap saved to {save_path}")
        if valid_errors.numel() > 0:
            print(f"  Error range: {valid_errors.min():.4f} - {valid_errors.max():.4f} (95th %ile: {p95:.4f})")
        return True

    def compute_window_events(self):
        """``:454-463``: per-polarity count image [B, 2, H, W] of the window's events at their own
        pixels."""
        ev = self._event_list
        idx = (ev[:, :, 1:2] * self.res[1] + ev[:, :, 2:3]).long()
        weights = torch.ones(idx.shape, device=ev.device)
        pol = self._pol_mask_list
        return torch.cat([interpolate(idx, weights, self.res, polarity_mask=pol[:, :, 0:1]),
                          interpolate(idx, weights, self.res, polarity_mask=pol[:, :, 1:2])], dim=1)

    def compute_masked_window_flow(self):
        """``:465-474``: the last flow map times the event mask (``overwrite_intermediate``), or
        the mask-weighted average of the window's flow maps."""
        if self.overwrite_intermediate:
            return self._flow_map[-1] * self._event_mask
        avg_flow = self._flow_map[0] * self._event_mask[:, 0:1, :, :]
        for i in range(1, self._event_mask.shape[1]):
            avg_flow += self._flow_map[i] * self._event_mask[:, i:i + 1, :, :]
        avg_flow /= torch.sum(self._event_mask, dim=1, keepdim=True) + 1e-9
        return avg_flow

    def compute_window_iwe(self, round_idx=True):
        """Per-polarity image of all window events warped with their window's flow (``:476-487``);
        uses the last flow map for every event (the reference's per-event flow list)."""
        pol = self._pol_mask_list
        return compute_pol_iwe(self._flow_map[-1], self._event_list, self.res, pol[:, :, 0:1], pol[:, :, 1:2],
                               flow_scaling=self.flow_scaling, round_idx=round_idx)


class AEE(BaseValidationLoss):
    """``loss/flow.py:597-649``: average endpoint error and outlier percentage per sample."""

    @property
    def num_events(self):
        return float("inf")

    def forward(self):
        flow = self._flow_map[-1].float().contiguous()
        B, _, H, W = flow.shape
        gt = self._gtflow.float().contiguous()
        mask = self._event_mask[:, -1, :, :].float().contiguous()
        # dt_gt / dt_input (one value for the batch, or B) divided in the kernel
        dtg = torch.as_tensor(self._dt_gt, dtype=torch.float32, device=flow.device).reshape(-1).contiguous()
        dti = torch.as_tensor(self._dt_input, dtype=torch.float32, device=flow.device).reshape(-1).contiguous()
        n = lib.snnflow_aee_acc_doubles(B, H, W)
        # the scratch carries the kernel's completion counter acc[0] (zero between calls: the last
        # block resets it), so it must never be shared by launches that can overlap: one scratch per
        # stream (a graph replays on the stream it was captured on, in order with eager calls there)
        # (a stream handle may be reused after its stream is destroyed: harmless, the counter is zero
        # between calls).  At most _AEE_SCRATCH_STREAMS streams are kept, least recently used dropped.
        stream = _lib.stream_ptr(flow.device)
        scratch = self.__dict__.setdefault("_aee_acc", collections.OrderedDict())
        key = (flow.device, stream)
        acc = scratch.pop(key, None)
        if acc is None or acc.numel() < n:
            acc = torch.zeros(n, dtype=torch.float64, device=flow.device)  # counter acc[0]: zero, kept zero
        scratch[key] = acc  # most recently used last
        while len(scratch) > _AEE_SCRATCH_STREAMS:
            scratch.popitem(last=False)
        aee = torch.empty(B, device=flow.device)
        pct = torch.empty(B, device=flow.device)
        a = _lib.AeeArgs()
        a.B, a.H, a.W = B, H, W
        a.flow, a.gtflow, a.event_mask, a.dt_ratio = ptr(flow), ptr(gt), ptr(mask), None
        a.dt_gt, a.dt_input, a.dt_gt_n, a.dt_input_n = ptr(dtg), ptr(dti), dtg.numel(), dti.numel()
        a.flow_scaling = float(self.flow_scaling)
        a.acc, a.aee, a.percent = ptr(acc), ptr(aee), ptr(pct)
        try:
            _lib.call("aee", lib.snnflow_aee, ctypes.byref(a), stream)
        except Exception:
            scratch.pop(key, None)  # a refused or failed launch may leave the counter nonzero: fresh scratch next time
            raise
        if self.error_maps:
            self._error_maps(_lib.EM_AEE)
        return aee, pct


def _dt_ratio(m, B, device):
    """dt_gt / dt_input per sample [B] (one value for the batch, or B)."""
    ratio = torch.as_tensor(m._dt_gt, dtype=torch.float32, device=device) / torch.as_tensor(
        m._dt_input, dtype=torch.float32, device=device)
    return ratio.reshape(-1).expand(B).contiguous() if ratio.numel() == 1 else ratio.reshape(B).contiguous()


def _flow_metrics(m, mag_threshold=0.5):
    """All SNNFLOW_M_* columns for the current association state of metric object m."""
    flow = m._flow_map[-1].float().contiguous()
    B, _, H, W = flow.shape
    gt = m._gtflow.float().contiguous()
    mask = m._event_mask[:, -1, :, :].float().contiguous()
    ratio = _dt_ratio(m, B, flow.device)
    rows = torch.empty(lib.snnflow_flow_metrics_rows(B, H, W), dtype=torch.float64, device=flow.device)
    out = torch.empty(B, len(_lib.METRICS), device=flow.device)
    a = _lib.FlowMetricsArgs()
    a.B, a.H, a.W = B, H, W
    a.flow, a.gtflow, a.event_mask, a.dt_ratio = ptr(flow), ptr(gt), ptr(mask), ptr(ratio)
    a.flow_scaling, a.mag_threshold = float(m.flow_scaling), float(mag_threshold)
    a.rows, a.out = ptr(rows), ptr(out)
    _lib.call("flow_metrics", lib.snnflow_flow_metrics, ctypes.byref(a), _lib.stream_ptr(flow.device))
    return {k: out[:, i] for i, k in enumerate(_lib.METRICS)}


class NEE(BaseValidationLoss):
    """``loss/flow.py:651-701``: normalised endpoint error |f-g| / (min(|f|,|g|) + 0.01) and
    the share of outliers (> 0.5), the latter counted over the whole batch as the reference does."""

    @property
    def num_events(self):
        return float("inf")

    def forward(self):
        r = _flow_metrics(self)
        return r["nee"], r["nee_pct"]


class AAE(BaseValidationLoss):
    """``loss/flow.py:703-762``: angular error with the reference's cosine
    (|f||g| / (f.g + 0.01), clamped) and the per-sample share of errors above pi/6."""

    @property
    def num_events(self):
        return float("inf")

    def forward(self):
        r = _flow_metrics(self)
        if self.error_maps:
            self._last_error_map = self._error_maps(_lib.EM_AAE)
        return r["aae"], r["aae_pct"]


class NAAE(BaseValidationLoss):
    """``loss/flow.py:764-820``: angular error divided by the predicted flow magnitude."""

    @property
    def num_events(self):
        return float("inf")

    def forward(self):
        naae = _flow_metrics(self)["naae"]
        if self.error_maps:
            self._error_maps(_lib.EM_NAAE)
        return naae


class AE_ofMeans(BaseValidationLoss):
    """``loss/flow.py:822-883``: angle between the masked mean flow and mean ground truth."""

    @property
    def num_events(self):
        return float("inf")

    def forward(self):
        return _flow_metrics(self)["ae_of_means"]


class AAE_Weighted(BaseValidationLoss):
    """``loss/flow.py:885-909``: magnitude-weighted angular error (numerator over all pixels,
    as in the reference)."""

    def forward(self):
        return _flow_metrics(self)["aae_weighted"]


class AAE_Filtered(BaseValidationLoss):
    """``loss/flow.py:911-937``: angular error over valid pixels with |f| >= mag_threshold."""

    def __init__(self, config, device, flow_scaling=128, mag_threshold=0.5):
        super().__init__(config, device, flow_scaling)
        self.mag_threshold = mag_threshold

    def forward(self):
        return _flow_metrics(self, self.mag_threshold)["aae_filtered"]
