"""Writes tests/golden/landscape_case.npz: the reference's brute-force contrast-maximisation heatmap.

    python tests/golden/make_golden_landscape.py REFERENCE_ROOT

Runs the reference's own loop (``tools/demo_iwe.py:71-85``: a constant flow map per candidate,
``loss.flow.EventWarping(config, "cpu", flow_scaling=1)`` ``event_flow_association`` + ``forward`` +
``reset``, ``heatmap[j, i]`` at ``(x_scale[i], y_scale[j])``) on two windows and stores, per case,

    {case}_events [B, N, 4]   {case}_pol [B, N, 2]   {case}_mask [B, 1, H, W]
    {case}_x_scale [R]        {case}_y_scale [R]     {case}_cand [R*R, 2]   (cand[j*R+i] = (x[i], y[j]))
    {case}_heatmap [R, R]     float32, the reference's losses
    {case}_meta               (H, W, maxdisp, R, flow_regul_weight, mask_output) as float64

Cases:
    a   12 x 20 (one partial band), B = 2, N = 300 uniform events (make_golden.synth_events, seed 21),
        9 x 9 candidates over +-4, flow_regul_weight 0.001, mask_output on: the batch sum and the
        regulariser constant.  Events at ts = 0 and ts = 1 and the integer candidates warp to exact
        integers (corner weights of exactly 0).
    b   40 x 72 (three bands, the last partial), B = 1, N = 1500: 24 points of random polarity that
        translate with the true flow (u, v) = (6, -4) px per window, pos = floor(p0 + (u, v) ts), events
        that leave the frame masked out (pol = 0); ts sorted and normalised to [0, 1]; seed 21; 9 x 9
        candidates over +-8, no regulariser.  The known answer: the reference's argmin is (6, -4).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (synth_events, install_stubs)

TRUE_FLOW = (6.0, -4.0)


def moving_points(gen, B, N, H, W, npts=24):
    u, v = TRUE_FLOW
    ts = torch.sort(torch.rand(B, N, generator=gen), dim=1).values
    ts = (ts - ts[:, :1]) / (ts[:, -1:] - ts[:, :1])
    y0 = torch.rand(B, npts, generator=gen) * H
    x0 = torch.rand(B, npts, generator=gen) * W
    pp = torch.randint(0, 2, (B, npts), generator=gen).float() * 2 - 1
    which = torch.randint(0, npts, (B, N), generator=gen)
    ys = torch.floor(torch.gather(y0, 1, which) + v * ts)
    xs = torch.floor(torch.gather(x0, 1, which) + u * ts)
    ps = torch.gather(pp, 1, which)
    inside = ((ys >= 0) & (ys < H) & (xs >= 0) & (xs < W)).float()
    ys, xs = ys * inside, xs * inside           # masked events sit at pixel (0, 0), as padding does
    ev = torch.stack([ts, ys, xs, ps], dim=2)
    pol = torch.stack([(ps > 0).float() * inside, (ps < 0).float() * inside], dim=2)
    mask = torch.zeros(B, 1, H, W)
    for b in range(B):
        keep = inside[b] > 0
        mask[b, 0, ys[b][keep].long(), xs[b][keep].long()] = 1
    return ev, pol, mask


def reference_heatmap(ref_flow, config, ev, pol, mask, maxdisp, R):
    loss_function = ref_flow.EventWarping(config, "cpu", flow_scaling=1)
    x_scale = np.linspace(-maxdisp, maxdisp, num=R)
    y_scale = np.linspace(-maxdisp, maxdisp, num=R)
    H, W = config["loader"]["resolution"]
    flowmap = torch.ones((ev.shape[0], 2, H, W))
    heatmap = np.zeros((R, R))
    with torch.no_grad():
        for i, u in enumerate(x_scale):
            for j, v in enumerate(y_scale):
                flow = flowmap.clone()
                flow[:, 0, :, :] *= u
                flow[:, 1, :, :] *= v
                loss_function.event_flow_association([flow], ev.clone(), pol.clone(), mask.clone())
                loss = loss_function()
                loss_function.reset()
                heatmap[j, i] = loss.cpu().numpy()
    return x_scale, y_scale, heatmap


def record(out, case, ref_flow, ev, pol, mask, H, W, maxdisp, R, weight, mask_output):
    config = {"loader": {"resolution": [H, W]}, "loss": {"flow_regul_weight": weight},
              "model": {"mask_output": mask_output}}
    x_scale, y_scale, heatmap = reference_heatmap(ref_flow, config, ev, pol, mask, maxdisp, R)
    xs, ys = x_scale.astype(np.float32), y_scale.astype(np.float32)
    out[f"{case}_events"], out[f"{case}_pol"], out[f"{case}_mask"] = ev.numpy(), pol.numpy(), mask.numpy()
    out[f"{case}_x_scale"], out[f"{case}_y_scale"] = xs, ys
    out[f"{case}_cand"] = np.stack([np.tile(xs, R), np.repeat(ys, R)], axis=1)
    out[f"{case}_heatmap"] = heatmap.astype(np.float32)
    out[f"{case}_meta"] = np.array([H, W, maxdisp, R, weight, float(mask_output)], dtype=np.float64)
    return x_scale, y_scale, heatmap


def main(root):
    make_golden.install_stubs()
    sys.path.insert(0, root)
    import loss.flow as ref_flow
    torch.set_num_threads(1)
    out = {}

    gen = torch.Generator().manual_seed(21)
    ev, pol, _, mask = make_golden.synth_events(gen, 2, 300, 12, 20)
    assert (ev[:, 0, 0] == 0).all() and (ev[:, -1, 0] == 1).all()
    _, _, heat = record(out, "a", ref_flow, ev, pol, mask, 12, 20, 4, 9, 0.001, True)
    assert np.isfinite(heat).all()

    gen = torch.Generator().manual_seed(21)
    ev, pol, mask = moving_points(gen, 1, 1500, 40, 72)
    assert (ev[:, 0, 0] == 0).all() and (ev[:, -1, 0] == 1).all()
    masked = int((pol.sum(dim=2) == 0).sum())
    assert 0 < masked < 1500 // 2, masked
    x_scale, y_scale, heat = record(out, "b", ref_flow, ev, pol, mask, 40, 72, 8, 9, 0.0, False)
    j, i = np.unravel_index(np.argmin(heat), heat.shape)
    best = np.sort(heat.ravel())[:2]
    assert (x_scale[i], y_scale[j]) == TRUE_FLOW, (x_scale[i], y_scale[j])
    print(f"case b: argmin ({x_scale[i]}, {y_scale[j]}), minimum {best[0]:.4f}, runner-up {best[1]:.4f}, "
          f"{masked} events masked out")

    path = os.path.join(HERE, "landscape_case.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1])
