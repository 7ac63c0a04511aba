"""Shared harness (a plain helper module, like firenet_harness.py): the implicit-GEMM U-Net kernels
(csrc/unet.hip: standalone ConvLIF / ConvLIFRecurrent cells outside the fixed one-kernel path, and the
whole SpikingRecEVFlowNet) at ragged shapes against the fp64 CPU oracle (oracle/unet_ref.py).

Case tables (``CELL_CASES`` / ``MODEL_CASES``), their ids and data seeds; fp32 data builders on the CPU
(``cell_data`` / ``model_data``); oracle runners in fp32 or fp64 (``cell_oracle`` / ``model_oracle``) that can
follow "ours": where an oracle spike differs from ours the oracle adopts ours straight-through (value
ours, the oracle's graph and surrogate kept); a differing spike whose oracle membrane is not within
``EPS`` of the threshold is counted as ``hard`` and fails the caller's test.  The membrane of this neuron
flavour is stored before the reset, so an adopted spike changes no stored membrane of its own step.
``cell_hip`` / ``model_hip`` run the HIP path; ``cell_compare`` / ``assert_cell`` and ``model_compare`` /
``assert_model`` are used identically by test_unet_ragged_cpu.py (the fp32 oracle in the role of "ours")
and test_gpu_unet_ragged.py.

The last part restates the host-side kernel selection of csrc/unet.hip in Python (``conv_ksplit``,
``conv_label``, ``wgrad_plan``, ``wgrad_partial_floats``) and enumerates the GEMM launches of a case in the
order snnflow.unet logs them (``cell_launches`` / ``model_launches``).  It only labels launches with the
instantiation they run; test_unet_ragged_cpu.py pins it to the library's own host functions for every
launch of every case, and test_gpu_unet_ragged.py compares the predicted plans with snnflow.unet.PLAN_LOG.
"""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

from firenet_harness import EPS, _cast, rel

ACTS = ("arctanspike", "superspike", "mgspike", "trianglespike")
S1, S2, T2 = 0, 1, 2  # segment modes (include/snnflow.h SNNFLOW_UNET_MODE_*)


def pad32(c):
    return (c + 31) // 32 * 32


def mpad(m):
    return (m + 127) // 128 * 128


# ---------------------------------------------------------------------------
# standalone cells: 2 chained steps, loss sum(z w) + 0.3 sum(v)
# ---------------------------------------------------------------------------
_CELL_ROWS = [  # (tag, recurrent, stride, k, cin, C, (B, H, W), options)
    ("tile1", False, 1, 3, 3, 12, (1, 5, 7), {}),          # one partial tile, odd W, partial channel quad in dgrad (M=3)
    ("res", False, 1, 3, 24, 24, (3, 9, 33), {"res": True}),
    ("recfrac", True, 1, 3, 12, 24, (3, 9, 33), {"detach": False, "frac": True}),
    ("m160", False, 1, 3, 40, 160, (2, 17, 65), {}),       # two 128-row tiles, 18 pixel tiles with a partial last
    ("rec64", True, 1, 3, 64, 64, (2, 15, 31), {}),
    ("s2m2", False, 2, 3, 2, 16, (3, 10, 34), {}),         # parity-class input gradient with M=2
    ("s2wo33", False, 2, 3, 20, 40, (3, 18, 66), {}),
    ("s2r3x65", False, 2, 3, 48, 96, (2, 6, 130), {}),
    ("s2rows", False, 2, 3, 40, 64, (2, 16, 32), {}),      # stride-2 row strips (Wo=16, Ho=8)
    ("s2rowsout", False, 2, 3, 40, 64, (2, 12, 32), {}),   # Ho=6, no multiple of 4: just outside eligibility
    ("rowsm32", True, 1, 3, 8, 24, (2, 16, 8), {}),
    ("rowsm64", False, 1, 3, 8, 48, (2, 4, 64), {}),
    ("rows2strip", False, 1, 3, 54, 24, (1, 12, 128), {}),
    ("k5", False, 1, 5, 6, 12, (2, 9, 33), {}),
    ("k5rec", True, 1, 5, 20, 20, (2, 12, 58), {}),
    ("k7", False, 1, 7, 3, 8, (2, 9, 33), {}),             # 49 taps: register-staged forward and input gradient
    ("k7wide", False, 1, 7, 40, 8, (1, 5, 9), {}),         # 49 taps with M=40: the register-staged 64-row input gradient
    ("k5s2", False, 2, 5, 8, 36, (2, 10, 34), {}),         # 3 or 2 taps per parity class
    ("k1", False, 1, 1, 16, 8, (3, 9, 33), {}),
    ("splitk", False, 1, 3, 100, 320, (1, 8, 24), {}),     # split-K > 1, 2.5 m-tiles; dgrad M=100 (128 tile)
    ("dg96", False, 1, 3, 80, 24, (1, 8, 24), {}),
    ("dg160", False, 1, 3, 150, 24, (1, 8, 24), {}),
    ("dg2x96", False, 1, 3, 180, 24, (1, 8, 24), {}),
    ("twopass", False, 1, 3, 2, 8, (2, 72, 72), {}),       # nsplit > 16 on the generic weight gradient
    ("twopassrows", False, 1, 3, 2, 8, (2, 72, 64), {}),   # ... and on the row strips
]
# weight-gradient tile sweep: channel pitch 32 / 64 / 96 / 128 / 160 x tm 32 / 64 / 128 without (160, 128)
_CELL_ROWS += [(f"wg{pad32(3 * cin)}x{tm}", False, 1, 3, cin, C, (2, 9, 33), {})
               for cin in (4, 16, 28, 36, 48) for C, tm in ((20, 32), (48, 64), (96, 128)) if (cin, C) != (48, 96)]
_CELL_ROWS += [
    # row strips whose split plan differs from the generic kernel's at the same shape (channel pitch 160 with
    # M > 64: the generic 96 x 128 tile pads it to 192, the 32-channel strip tiles do not), so that the logged
    # plan tells the two apart (test_unet_ragged_cpu.py::test_row_strip_plans_differ_from_generic)
    ("s2rowspad", False, 2, 3, 48, 96, (2, 16, 32), {}),
    ("rowspad", False, 1, 3, 48, 96, (2, 4, 64), {}),
    # 49 taps at M = 24 / 48 / 96: the 32-, 64- and 128-row register-staged forward (k7 and k7wide run the 16-row one)
    ("k7m32", False, 1, 7, 3, 24, (1, 5, 9), {}),
    ("k7m64", False, 1, 7, 3, 48, (1, 5, 9), {}),
    ("k7m128", False, 1, 7, 3, 96, (1, 5, 9), {}),
]


def _would_be_fixed(k, stride, cin, C, act, detach):
    """snnflow.convlif._fixed_kernel's condition (asserted against it by both test files)."""
    return k == 3 and stride == 1 and C in (4, 8, 16, 32) and act == "arctanspike" and detach and (1 <= cin <= 5 or cin == C)


def _cell_cases():
    """The rows with the four surrogates, hard / soft reset and detach rotated over them; a rotation
    that would land on the fixed one-kernel path moves on to the next surrogate."""
    cases = []
    for i, (tag, rec, stride, k, cin, C, shape, opt) in enumerate(_CELL_ROWS):
        act, hard, detach = ACTS[i % 4], (i // 2) % 2 == 0, opt.get("detach", i % 3 != 1)
        if _would_be_fixed(k, stride, cin, C, act, detach):
            act = ACTS[(i + 1) % 4]
        cases.append({"tag": tag, "rec": rec, "stride": stride, "k": k, "cin": cin, "C": C, "shape": shape, "act": act,
                      "hard": hard, "detach": detach, "res": bool(opt.get("res")), "frac": bool(opt.get("frac"))})
    return cases


CELL_CASES = _cell_cases()
CELL_T = 2


def cell_id(c):
    B, H, W = c["shape"]
    return f"{c['tag']}-{'rec' if c['rec'] else 'ff'}-s{c['stride']}-k{c['k']}-{c['cin']}to{c['C']}-{B}x{H}x{W}"


# Data seed of a cell case where the default (100) leaves more neurons of the fp64 oracle within EPS of
# the threshold than cell_cap allows (test_unet_ragged_cpu.py::test_cell_near_threshold_cap holds the
# rule: seeds are chosen on the CPU, from the oracle alone).
CELL_SEED = {"rec64-rec-s1-k3-64to64-2x15x31": 102, "s2rows-ff-s2-k3-40to64-2x16x32": 102,
             "rows2strip-ff-s1-k3-54to24-1x12x128": 101, "k5-ff-s1-k5-6to12-2x9x33": 103, "k7-ff-s1-k7-3to8-2x9x33": 101,
             "dg96-ff-s1-k3-80to24-1x8x24": 101, "dg160-ff-s1-k3-150to24-1x8x24": 102,
             "dg2x96-ff-s1-k3-180to24-1x8x24": 102, "wg32x128-ff-s1-k3-4to96-2x9x33": 101,
             "wg96x64-ff-s1-k3-28to48-2x9x33": 101}


def cell_out_hw(c):
    B, H, W = c["shape"]
    return (H // c["stride"], W // c["stride"])


def cell_neuron_steps(c):
    Ho, Wo = cell_out_hw(c)
    return CELL_T * c["shape"][0] * c["C"] * Ho * Wo


def cell_cap(c):
    """0.01 % of the case's neuron-steps, rounded down (firenet_harness.cell_cap's rule)."""
    return cell_neuron_steps(c) // 10000


def _ramp(shape, gen):
    n = int(np.prod(shape))
    return (torch.linspace(-1, 1, n) + 0.5 * torch.randn(n, generator=gen)).view(*shape)


def _new_cell_ref(c):
    from oracle.unet_ref import _Cell

    return _Cell(c["cin"], c["C"], c["k"], stride=c["stride"], recurrent=c["rec"], activation=c["act"],
                 leak=(0.0, 1.0), thresh=(0.5, 0.2), hard_reset=c["hard"], detach=c["detach"])


def cell_data(c):
    """fp32 CPU data of a case: parameters (the oracle's / the HIP cell's common state dict), CELL_T
    inputs (randn masked at 50 %: not exact in bf16, so the mid and lo planes of the split operand
    carry data), the previous state (binary spikes, or fractional ones for ``frac``), per-step upstream
    weights (firenet_harness.cell_data's asymmetric ramp plus noise) and residuals."""
    seed = CELL_SEED.get(cell_id(c), 100)
    B, H, W = c["shape"]
    Ho, Wo = cell_out_hw(c)
    torch.manual_seed(1000 + seed)
    sd = {k: v.clone() for k, v in _new_cell_ref(c).state_dict().items()}
    gen = torch.Generator().manual_seed(seed)
    xs = [torch.randn(B, c["cin"], H, W, generator=gen) * (torch.rand(B, c["cin"], H, W, generator=gen) < 0.5).float()
          for _ in range(CELL_T)]
    v0 = torch.randn(B, c["C"], Ho, Wo, generator=gen) * 0.5
    z0 = torch.rand(B, c["C"], Ho, Wo, generator=gen)
    s0 = torch.stack([v0, z0 if c["frac"] else (z0 < 0.3).float()])
    wz = [_ramp((B, c["C"], Ho, Wo), gen) for _ in range(CELL_T)]
    res = [torch.randn(B, c["C"], Ho, Wo, generator=gen) * 0.5 for _ in range(CELL_T)] if c["res"] else None
    return {"sd": sd, "xs": xs, "s0": s0, "wz": wz, "res": res}


def _adopt(v, s, th, target, eps, counters):
    """Counts the neurons within eps of the threshold; with ``target`` (our spikes) counts the
    differing spikes (all / away from the threshold) and returns the oracle's spikes with ours adopted
    straight-through."""
    near = (v.detach() - th).abs() <= eps
    counters["near"] += int(near.sum())
    if target is None:
        return s
    o = target.to(s.dtype)
    diff = s.detach() != o
    n = int(diff.sum())
    if n:
        counters["flips"] += n
        counters["hard"] += int((diff & ~near).sum())
        s = s + ((o - s.detach()) * diff).detach()
    return s


def _new_counters():
    return {"flips": 0, "hard": 0, "near": 0}


def cell_oracle(c, data, dtype, ours=None, eps=EPS):
    """The oracle cell's CELL_T chained steps and backward in ``dtype``; ``ours``: a result dict whose
    spikes to follow.  Returns spikes and membranes per step, the loss, the gradients of inputs,
    previous state, residuals and parameters, and the near / flips / hard counters."""
    ref = _new_cell_ref(c)
    ref.load_state_dict(data["sd"])
    ref = ref.to(dtype)
    xs = [x.to(dtype).clone().requires_grad_(True) for x in data["xs"]]
    s0 = data["s0"].to(dtype).clone().requires_grad_(True)
    res = [r.to(dtype).clone().requires_grad_(True) for r in data["res"]] if c["res"] else None
    cnt = _new_counters()
    st, loss, spk, mem = s0, 0, [], []
    for t in range(CELL_T):
        r = res[t] if res else 0
        _, st = ref(xs[t], st, r)
        v = st[0]
        s = _adopt(v, st[1], ref.thresh.detach().clamp_min(0.01), None if ours is None else ours["spk"][t].detach().cpu(),
                   eps, cnt)
        st = torch.stack([v, s])
        loss = loss + ((s + r) * data["wz"][t].to(dtype)).sum() + 0.3 * v.sum()
        spk.append(s.detach())
        mem.append(v.detach())
    loss.backward()
    grads = {f"x{t}": xs[t].grad for t in range(CELL_T)}
    grads["state0"] = s0.grad
    if res:
        grads.update({f"res{t}": res[t].grad for t in range(CELL_T)})
    grads.update({n: p.grad for n, p in ref.named_parameters()})
    return {"spk": spk, "mem": mem, "loss": float(loss.detach()), "grads": grads, **cnt}


def new_hip_cell(c, dev="cpu"):
    import snnflow

    kw = dict(activation=c["act"], leak=(0.0, 1.0), thresh=(0.5, 0.2), hard_reset=c["hard"], detach=c["detach"])
    if c["rec"]:
        return snnflow.ConvLIFRecurrent(c["cin"], c["C"], c["k"], **kw).to(dev)
    return snnflow.ConvLIF(c["cin"], c["C"], c["k"], stride=c["stride"], **kw).to(dev)


def cell_hip(c, data, dev):
    """The same steps through the HIP cell (snnflow.unet.ConvLIFCellFn); ``plans``: snnflow.unet.PLAN_LOG."""
    import snnflow.unet as un
    from snnflow import convlif

    cell = new_hip_cell(c, dev)
    assert not convlif._fixed_kernel(cell), cell_id(c)
    cell.load_state_dict({k: v.to(dev) for k, v in data["sd"].items()})
    xs = [x.to(dev).requires_grad_(True) for x in data["xs"]]
    s0 = data["s0"].to(dev).requires_grad_(True)
    res = [r.to(dev).requires_grad_(True) for r in data["res"]] if c["res"] else None
    un.PLAN_LOG = []
    try:
        st, loss, spk, mem = s0, 0, [], []
        for t in range(CELL_T):
            if c["rec"]:
                z, st = cell(xs[t], st)
            else:
                z, st = cell(xs[t], st, residual=res[t] if res else 0)
            loss = loss + (z * data["wz"][t].to(dev)).sum() + 0.3 * st[0].sum()
            spk.append(st[1].detach().cpu())
            mem.append(st[0].detach().cpu())
            if res:  # the output is the spikes plus the residual
                assert torch.equal(z.detach(), st[1].detach() + res[t].detach()), cell_id(c)
        loss.backward()
        plans = list(un.PLAN_LOG)
    finally:
        un.PLAN_LOG = None
    grads = {f"x{t}": xs[t].grad.cpu() for t in range(CELL_T)}
    grads["state0"] = s0.grad.cpu()
    if res:
        grads.update({f"res{t}": res[t].grad.cpu() for t in range(CELL_T)})
    grads.update({n: p.grad.cpu() for n, p in cell.named_parameters()})
    return {"spk": spk, "mem": mem, "loss": float(loss.detach()), "grads": grads, "plans": plans}


# Limits, all the project's own (tests/test_gpu_unet.py)
CELL_STATE_TOL = 1e-5    # rtol = atol on membranes (test_convlif_general_cell_vs_oracle)
MODEL_STATE_TOL = 1e-4   # rtol = atol on the model's states (test_unet_vs_oracle)
FLOW_RTOL, FLOW_ATOL = 1e-4, 1e-6
LOSS_RTOL = 1e-5
GRAD_FLOOR = 2e-5        # gradients: rel-L2 against fp64 <= max(2 x the fp32 oracle's, GRAD_FLOOR)
                         # (test_unet_cfg5_shapes_vs_oracle)
MODEL_CAP = 3e-4         # near-threshold neurons of a model case: 0.03 % of its neuron-steps

# Measured on the MI355X (test_gpu_unet_ragged.py prints them): worst rel-L2 against fp64 over a case's
# gradients.  Figures only; the limit is max(2 x the fp32 oracle's error, GRAD_FLOOR) for every case.
REF_CELL_GRAD = {"tile1-ff-s1-k3-3to12-1x5x7": 2.18e-07, "res-ff-s1-k3-24to24-3x9x33": 7.55e-07,
                 "recfrac-rec-s1-k3-12to24-3x9x33": 3.59e-07, "m160-ff-s1-k3-40to160-2x17x65": 9.68e-07,
                 "rec64-rec-s1-k3-64to64-2x15x31": 4.65e-07, "s2m2-ff-s2-k3-2to16-3x10x34": 4.18e-07,
                 "s2wo33-ff-s2-k3-20to40-3x18x66": 2.43e-07, "s2r3x65-ff-s2-k3-48to96-2x6x130": 1.10e-06,
                 "s2rows-ff-s2-k3-40to64-2x16x32": 3.00e-07, "s2rowsout-ff-s2-k3-40to64-2x12x32": 7.21e-07,
                 "rowsm32-rec-s1-k3-8to24-2x16x8": 2.37e-07, "rowsm64-ff-s1-k3-8to48-2x4x64": 5.26e-07,
                 "rows2strip-ff-s1-k3-54to24-1x12x128": 3.86e-07, "k5-ff-s1-k5-6to12-2x9x33": 8.54e-07,
                 "k5rec-rec-s1-k5-20to20-2x12x58": 3.25e-07, "k7-ff-s1-k7-3to8-2x9x33": 1.31e-06,
                 "k7wide-ff-s1-k7-40to8-1x5x9": 4.21e-07, "k5s2-ff-s2-k5-8to36-2x10x34": 8.78e-07,
                 "k1-ff-s1-k1-16to8-3x9x33": 2.89e-07, "splitk-ff-s1-k3-100to320-1x8x24": 1.09e-06,
                 "dg96-ff-s1-k3-80to24-1x8x24": 3.03e-07, "dg160-ff-s1-k3-150to24-1x8x24": 8.63e-07,
                 "dg2x96-ff-s1-k3-180to24-1x8x24": 3.06e-07, "twopass-ff-s1-k3-2to8-2x72x72": 9.60e-07,
                 "twopassrows-ff-s1-k3-2to8-2x72x64": 8.56e-07, "wg32x32-ff-s1-k3-4to20-2x9x33": 5.52e-07,
                 "wg32x64-ff-s1-k3-4to48-2x9x33": 3.17e-07, "wg32x128-ff-s1-k3-4to96-2x9x33": 6.23e-07,
                 "wg64x32-ff-s1-k3-16to20-2x9x33": 2.52e-07, "wg64x64-ff-s1-k3-16to48-2x9x33": 7.72e-07,
                 "wg64x128-ff-s1-k3-16to96-2x9x33": 3.91e-07, "wg96x32-ff-s1-k3-28to20-2x9x33": 1.00e-06,
                 "wg96x64-ff-s1-k3-28to48-2x9x33": 3.92e-07, "wg96x128-ff-s1-k3-28to96-2x9x33": 9.71e-07,
                 "wg128x32-ff-s1-k3-36to20-2x9x33": 2.49e-07, "wg128x64-ff-s1-k3-36to48-2x9x33": 1.03e-06,
                 "wg128x128-ff-s1-k3-36to96-2x9x33": 4.74e-07, "wg160x32-ff-s1-k3-48to20-2x9x33": 8.30e-07,
                 "wg160x64-ff-s1-k3-48to48-2x9x33": 3.08e-07, "s2rowspad-ff-s2-k3-48to96-2x16x32": 1.13e-06,
                 "rowspad-ff-s1-k3-48to96-2x4x64": 4.73e-07, "k7m32-ff-s1-k7-3to24-1x5x9": 7.58e-07,
                 "k7m64-ff-s1-k7-3to48-1x5x9": 3.59e-07, "k7m128-ff-s1-k7-3to96-1x5x9": 1.40e-06}
REF_MODEL_GRAD = {"norows-base12-3x48x80": 1.57e-06, "m160-base20-1x80x48": 4.47e-06,
                  "wide-base8-3x16x176": 5.06e-07, "tall-base4-2x112x16": 9.75e-06,
                  "mixed-base12-2x48x128": 1.83e-06, "voxel5-base8-2x32x48": 4.85e-06,
                  "given-base8-2x48x64": 5.85e-07, "crop-base8-2x37x51": 6.59e-06, "crop-base8-2x20x44": 8.26e-07}
# Reference against reference: the fp32 CPU oracle's loss against the fp64 oracle's (relative), listed where
# it exceeds LOSS_RTOL; such a case's limit is 4 x its figure (``wide``).  At 1 x 80 x 48 every flow of the
# two oracles agrees within FLOW_RTOL / FLOW_ATOL as in the other cases and the loss still differs: the contrast loss divides per-pixel sums of bilinear weights by
# (count + 1e-9), and a pixel that only a far corner of a barely-moved event touches has a count of the
# order of the fp32 rounding of the warped coordinate (firenet_harness.REF_STEP_GRAD tells the same of its
# gradient; here dL/dflow of the two oracles differs by 0.8 relative L2).  The HIP loss reproduces the fp32
# arithmetic, which is why the network backward of every run is seeded with ours' dL/dflow.
REF_MODEL_LOSS = {"m160-base20-1x80x48": 2.59e-5}


def wide(figure, base):
    """The limit where the fp32 oracle's own committed figure exceeds the project's: 4 x the figure."""
    return 4 * figure if figure is not None and figure > base else base


def _excess(a, b, tol):
    """max(|a - b| - tol |b|): <= tol is allclose(rtol=tol, atol=tol)."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float(((a - b).abs() - tol * b.abs()).max())


def _grad_figures(ours, w64, w32):
    e_ours = {n: rel(ours["grads"][n].detach().cpu().numpy(), g.numpy()) for n, g in w64["grads"].items()}
    e_32 = {n: rel(w32["grads"][n].detach().cpu().numpy(), g.numpy()) for n, g in w64["grads"].items()}
    return e_ours, e_32


def _finite(ts):
    return all(bool(torch.isfinite(t).all()) for t in ts)


def cell_compare(tag, ours, w64, w32):
    """Figures of a cell result against the fp64 oracle that followed it (``w32``: the fp32 oracle
    that followed it, for the gradient limit): printed, then returned for ``assert_cell``.
    ``spk_diff`` is a self-check of the adoption, not a measurement: the oracle's spikes are returned
    after ours were adopted, so it is 0 unless the adoption itself is broken; what holds the spikes is
    ``hard`` == 0 and ``adopted`` <= min(``near``, cap).  On the CPU side ``w32`` is ``ours`` itself (the fp32
    oracle plays ours), so the gradient limit holds trivially there: that run shows that the harness can pass
    and prints the reference-against-reference figures, it does not test the limit."""
    e_ours, e_32 = _grad_figures(ours, w64, w32)
    r = {"finite": _finite(ours["spk"] + ours["mem"] + list(ours["grads"].values())),
         "binary": all(bool(((s == 0) | (s == 1)).all()) for s in ours["spk"]),
         "spk_diff": sum(int((a.double() != b.double()).sum()) for a, b in zip(ours["spk"], w64["spk"])),
         "mem_excess": max(_excess(a, b, CELL_STATE_TOL) for a, b in zip(ours["mem"], w64["mem"])),
         "loss": (ours["loss"], w64["loss"]), "e_ours": e_ours, "e_32": e_32,
         "near": w64["near"], "adopted": w64["flips"] - w64["hard"], "hard": w64["hard"] + w32["hard"]}
    worst = max(e_ours.items(), key=lambda kv: kv[1])
    r["worst"] = worst[1]
    print(f"\n[{tag}] near {r['near']} adopted {r['adopted']} hard {r['hard']} spk_diff {r['spk_diff']} "
          f"mem excess {r['mem_excess']:.2e} loss {r['loss'][0]:.9g} / {r['loss'][1]:.9g} "
          f"(rel {abs(r['loss'][0] - r['loss'][1]) / abs(r['loss'][1]):.2e}); grad rel-L2 vs fp64: worst "
          f"{worst[0]} {worst[1]:.2e} (fp32 oracle there {e_32[worst[0]]:.2e}; fp32 oracle worst {max(e_32.values()):.2e}): "
          + ", ".join(f"{k}={v:.1e}" for k, v in e_ours.items()))
    return r


def _assert_common(cid, r, cap, state_tol):
    assert r["finite"] and r["binary"], cid
    assert r["hard"] == 0, f"{cid}: {r['hard']} spikes differ away from the threshold"
    assert r["adopted"] <= min(r["near"], cap), f"{cid}: {r['adopted']} spikes adopted, near {r['near']}, cap {cap}"
    assert r["spk_diff"] == 0, (cid, r["spk_diff"])
    assert r["mem_excess"] <= state_tol, (cid, r["mem_excess"])
    for n, e in r["e_ours"].items():
        assert np.isfinite(e) and e <= max(2 * r["e_32"][n], GRAD_FLOOR), (cid, n, e, r["e_32"][n])


def assert_cell(cid, r, cap):
    _assert_common(cid, r, cap, CELL_STATE_TOL)
    assert abs(r["loss"][0] - r["loss"][1]) <= LOSS_RTOL * abs(r["loss"][1]), (cid, r["loss"])


# ---------------------------------------------------------------------------
# whole model: T = 3 windows of 1000 events, EventWarping over the 4 flows
# ---------------------------------------------------------------------------
MODEL_T, MODEL_N, MODEL_WSEED, MODEL_DSEED = 3, 1000, 5, 3
_MODEL_ROWS = [  # (tag, base, (B, H, W), options)
    ("norows", 12, (3, 48, 80), {}),      # no layer row-strip-eligible; deepest level 3x5; M 24..192
    ("m160", 20, (1, 80, 48), {}),        # M 40..320; 160-row input-gradient tile
    ("wide", 8, (3, 16, 176), {}),        # deepest level 1x11
    ("tall", 4, (2, 112, 16), {}),        # deepest level 7x1
    ("mixed", 12, (2, 48, 128), {}),      # row-strip and generic layers in one model
    ("voxel5", 8, (2, 32, 48), {"voxel": 5}),
    ("given", 8, (2, 48, 64), {"given": True}),
    ("crop", 8, (2, 37, 51), {"crop": True}),
    ("crop", 8, (2, 20, 44), {"crop": True}),
]
_ACT_PAIRS = [("arctanspike", "arctanspike"), ("superspike", "trianglespike"), ("mgspike", "arctanspike"),
              ("trianglespike", "superspike")]
MODEL_CASES = [{"tag": tag, "base": base, "shape": shape, "acts": _ACT_PAIRS[i % 4], "hard": i % 2 == 0,
                "voxel": opt.get("voxel", 0), "given": bool(opt.get("given")), "crop": bool(opt.get("crop"))}
               for i, (tag, base, shape, opt) in enumerate(_MODEL_ROWS)]


def model_id(c):
    B, H, W = c["shape"]
    return f"{c['tag']}-base{c['base']}-{B}x{H}x{W}"


def unet_kw(base, activations=("arctanspike", "arctanspike"), hard=True, encoding="cnt", num_bins=2):
    return {"name": "SpikingRecEVFlowNet", "encoding": encoding, "round_encoding": False, "norm_input": False,
            "num_bins": num_bins, "base_num_channels": base, "kernel_size": 3, "activations": list(activations),
            "mask_output": True,
            "spiking_neuron": {"leak": [0.0, 1.0], "thresh": [0.0, 0.8], "learn_leak": True, "learn_thresh": True,
                               "hard_reset": hard}}


def loss_cfg(H, W):
    return {"loader": {"resolution": [H, W]}, "loss": {"flow_regul_weight": 0.001, "overwrite_intermediate": False},
            "model": {"mask_output": True}}


def model_kw(c):
    return unet_kw(c["base"], c["acts"], c["hard"], "voxel" if c["voxel"] else "cnt", c["voxel"] or 2)


def crop_geometry(H, W):
    """Zero padding to the next multiple of 16, the extra row / column at the top / left when the
    padding is odd: (padded H, padded W, top, left)."""
    Hc, Wc = (H + 15) // 16 * 16, (W + 15) // 16 * 16
    return Hc, Wc, (Hc - H + 1) // 2, (Wc - W + 1) // 2


def padded_hw(c):
    B, H, W = c["shape"]
    return crop_geometry(H, W)[:2] if c["crop"] else (H, W)


def model_cell_shapes(c):
    """(C, h, w) of the 16 cells in the order of ``_ref_cells``."""
    H, W = padded_hw(c)
    base, out = c["base"], []
    for i in range(4):
        out += [(base << (i + 1), H >> (i + 1), W >> (i + 1))] * 2
    out += [(base << 4, H >> 4, W >> 4)] * 4
    for i in range(4):
        out.append((base << (3 - i), H >> (3 - i), W >> (3 - i)))
    return out


def model_neuron_steps(c):
    return MODEL_T * c["shape"][0] * sum(C * h * w for C, h, w in model_cell_shapes(c))


def model_cap(c):
    return int(MODEL_CAP * model_neuron_steps(c))


def voxel_of(win, nb, H, W):
    """Real-valued [B, nb, H, W] input of a window: every event's polarity spread over the two
    bins next to ts (nb - 1) with bilinear weights."""
    ev = win["event_list"]
    B, N, _ = ev.shape
    pos = ev[..., 0] * (nb - 1)
    lo = pos.floor().clamp(0, nb - 1)
    pix = (ev[..., 1] * W + ev[..., 2]).long()
    vox = torch.zeros(B, nb * H * W)
    for b, wgt in ((lo, 1 - (pos - lo)), ((lo + 1).clamp(max=nb - 1), pos - lo)):
        vox.scatter_add_(1, b.long() * (H * W) + pix, ev[..., 3] * wgt)
    return vox.view(B, nb, H, W)


def model_data(c):
    """fp32 CPU data of a model case: initial parameters (weight seed 5), MODEL_T windows (data seed
    3; ``x``: the network input) and, for ``given``, the 10 initial states (random membranes, binary spikes)."""
    from oracle.unet_ref import SpikingRecEVFlowNetRef
    from snnflow.synthetic import make_window

    B, H, W = c["shape"]
    torch.manual_seed(MODEL_WSEED)
    init = {k: v.clone() for k, v in SpikingRecEVFlowNetRef(model_kw(c)).state_dict().items()}
    gen = torch.Generator().manual_seed(MODEL_DSEED)
    wins = [make_window(B, MODEL_N, H, W, gen, "cpu") for _ in range(MODEL_T)]
    for w in wins:
        w["x"] = voxel_of(w, c["voxel"], H, W) if c["voxel"] else w["event_cnt"]
    states0 = None
    if c["given"]:
        g = torch.Generator().manual_seed(4)
        shapes = model_cell_shapes(c)

        def one(C, h, w):
            return torch.stack([torch.randn(B, C, h, w, generator=g) * 0.5, (torch.rand(B, C, h, w, generator=g) < 0.2).float()])
        states0 = [torch.stack([one(*shapes[2 * i]), one(*shapes[2 * i + 1])]) for i in range(6)]
        states0 += [one(*shapes[12 + i]) for i in range(4)]
    return {"init": init, "wins": wins, "states0": states0}


def _ref_cells(ref):
    """The oracle U-Net's cells in the order of the model's 10 states, as (cell, state index,
    sub-index or None) (encoders: ff + recurrent cell, resblocks: conv1 + conv2, decoders)."""
    u = ref.multires_unetrec
    out = []
    for i, e in enumerate(u.encoders):
        out += [(e.conv, i, 0), (e.recurrent_block, i, 1)]
    for j, r in enumerate(u.resblocks):
        out += [(r.conv1, 4 + j, 0), (r.conv2, 4 + j, 1)]
    for i, d in enumerate(u.decoders):
        out.append((d.conv2d, 6 + i, None))
    return out


def _patch_flips(ref, ours_states, eps, counters):
    """Flip correction of the oracle U-Net (see test_unet_cfg5_shapes_vs_oracle): every cell adopts
    our spike straight-through where its own differs; the ones whose membrane is not within eps of
    the threshold are counted as hard, and every neuron within eps of the threshold as near.
    ``ours_states`` None: the oracle runs free and only ``near`` is counted.  Returns the per-step
    target setter."""
    counters.setdefault("near", 0)
    cells = _ref_cells(ref)
    targets = []
    for cell, i, j in cells:
        tgt = {}
        orig = type(cell).forward

        def fwd(x, prev, residual=0, cell=cell, tgt=tgt, orig=orig):
            out, st = orig(cell, x, prev, residual)
            v, s0 = st[0], st[1]
            s = _adopt(v, s0, cell.thresh.detach().clamp_min(0.01), tgt.get("state"), eps, counters)
            if s is not s0:
                st = torch.stack([v, s])
                out = s + residual
            return out, st
        cell.forward = fwd
        targets.append((tgt, i, j))

    def set_step(t):
        if ours_states is None:
            return
        for tgt, i, j in targets:
            st = ours_states[t][i]
            tgt["state"] = (st[j] if j is not None else st)[1]
    return set_step


def _spikes(st):
    return st[:, 1] if st.dim() == 6 else st[1]


def _membranes(st):
    return st[:, 0] if st.dim() == 6 else st[0]


def model_oracle(c, data, dtype, ours=None, eps=EPS):
    """The oracle model's MODEL_T steps, EventWarping loss over the 4 flows and backward in ``dtype``.
    ``ours``: a result dict; the oracle follows its spikes and its backward through the network is
    seeded with ITS dL/dflow (test_unet_cfg5_shapes_vs_oracle: the contrast loss is ill-conditioned in
    the flows, so equal flows can give dL/dflow that differ by 1e-4; the loss gradient has its own
    tests); without, the oracle runs free and back-propagates its own loss.  ``init_cropping`` cases:
    the input zero-padded to the next multiple of 16, the flows cropped back, the loss at the original
    resolution."""
    from oracle import iwe_ref
    from oracle.unet_ref import SpikingRecEVFlowNetRef

    B, H, W = c["shape"]
    ref = SpikingRecEVFlowNetRef(model_kw(c))
    ref.load_state_dict(data["init"])
    ref = ref.to(dtype)
    cnt = _new_counters()
    step = _patch_flips(ref, None if ours is None else ours["states"], eps, cnt)
    states0 = None
    if data["states0"] is not None:
        states0 = [s.to(dtype).clone().requires_grad_(True) for s in data["states0"]]
        ref.states = states0
    Hc, Wc, top, left = crop_geometry(H, W)
    flows, states = [], []
    for t, w in enumerate(data["wins"]):
        x = w["x"].to(dtype)
        if c["crop"]:
            x = F.pad(x, (left, Wc - W - left, top, Hc - H - top))
        step(t)
        fl = ref(x, x)["flow"]
        if c["crop"]:
            fl = [f[:, :, top:top + H, left:left + W] for f in fl]
        flows.append(fl)
        states.append([s.detach() for s in ref.states])
    loss = 0
    for i in range(4):
        lf = iwe_ref.EventWarpingRef([H, W], weight=0.001)
        for t, w in enumerate(data["wins"]):
            w = _cast(w, dtype)
            lf.event_flow_association([flows[t][i]], w["event_list"], w["event_list_pol_mask"], w["event_mask"])
        loss = loss + lf()
    loss = loss / 4
    allf = [f for fs in flows for f in fs]
    seeds = [g.detach() for g in torch.autograd.grad(loss, allf, retain_graph=True)]
    torch.autograd.backward(allf, seeds if ours is None else [g.detach().cpu().to(dtype) for g in ours["seeds"]])
    grads = {n: p.grad for n, p in ref.named_parameters()}
    if states0 is not None:
        grads.update({f"state{k}": s.grad for k, s in enumerate(states0)})
    return {"flows": [[f.detach() for f in fs] for fs in flows], "states": states, "loss": float(loss.detach()), "seeds": seeds,
            "grads": grads, **cnt}


def model_hip(c, data, dev):
    """The same train step through snnflow.SpikingRecEVFlowNet and snnflow.EventWarping; ``plans``:
    snnflow.unet.PLAN_LOG over forward and backward."""
    import snnflow
    import snnflow.unet as un

    B, H, W = c["shape"]
    model = snnflow.SpikingRecEVFlowNet(model_kw(c)).to(dev)
    model.load_state_dict({k: v.to(dev) for k, v in data["init"].items()})
    if c["crop"]:
        model.init_cropping(W, H)
    states0 = None
    if data["states0"] is not None:
        states0 = [s.to(dev).requires_grad_(True) for s in data["states0"]]
        model.states = states0
    ew = snnflow.EventWarping(loss_cfg(H, W), dev)
    un.PLAN_LOG = []
    try:
        flows, states = [], []
        for w in data["wins"]:
            x = w["x"].to(dev)
            fl = model(x, x)["flow"]
            for f in fl:
                f.retain_grad()
            flows.append(fl)
            states.append([s.detach().cpu() for s in model.states])
            ew.event_flow_association(fl, w["event_list"].to(dev), w["event_list_pol_mask"].to(dev), w["event_mask"].to(dev))
        loss = ew()
        loss.backward()
        plans = list(un.PLAN_LOG)
    finally:
        un.PLAN_LOG = None
    grads = {n: p.grad.cpu() for n, p in model.named_parameters()}
    if states0 is not None:
        grads.update({f"state{k}": s.grad.cpu() for k, s in enumerate(states0)})
    return {"flows": [[f.detach().cpu() for f in fs] for fs in flows], "states": states, "loss": float(loss.detach()),
            "seeds": [f.grad.cpu() for fs in flows for f in fs], "grads": grads, "plans": plans, "model": model}


def model_compare(tag, ours, w64, w32):
    """Figures of a model result against the fp64 oracle that followed it (``w32``: the fp32 oracle
    that followed it): printed, then returned for ``assert_model``.  ``spk_diff`` is a self-check of the
    adoption, as in ``cell_compare``."""
    e_ours, e_32 = _grad_figures(ours, w64, w32)
    T = len(w64["flows"])
    fo = [f for fs in ours["flows"] for f in fs]
    fr = [f for fs in w64["flows"] for f in fs]
    so = [s for sts in ours["states"] for s in sts]
    sr = [s for sts in w64["states"] for s in sts]
    r = {"finite": _finite(fo + so + list(ours["grads"].values())),
         "binary": all(bool(((_spikes(s) == 0) | (_spikes(s) == 1)).all()) for s in so),
         "spk_diff": sum(int((_spikes(a).double() != _spikes(b).double()).sum()) for a, b in zip(so, sr)),
         "mem_excess": max(_excess(_membranes(a), _membranes(b), MODEL_STATE_TOL) for a, b in zip(so, sr)),
         "flow_excess": max(float(((a.double() - b.double()).abs() - FLOW_RTOL * b.double().abs()).max()) for a, b in zip(fo, fr)),
         "flow_shapes": [tuple(f.shape) for f in fo], "loss": (ours["loss"], w64["loss"]),
         "seed_rel": rel(torch.cat([g.reshape(-1) for g in ours["seeds"]]).numpy(),
                         torch.cat([g.reshape(-1) for g in w64["seeds"]]).numpy()),
         "e_ours": e_ours, "e_32": e_32, "near": w64["near"], "adopted": w64["flips"] - w64["hard"],
         "hard": w64["hard"] + w32["hard"], "T": T}
    worst = max(e_ours.items(), key=lambda kv: kv[1])
    r["worst"] = worst[1]
    print(f"\n[{tag}] near {r['near']} adopted {r['adopted']} hard {r['hard']} spk_diff {r['spk_diff']} "
          f"state excess {r['mem_excess']:.2e} flow excess over rtol {r['flow_excess']:.2e} loss {r['loss'][0]:.9g} / "
          f"{r['loss'][1]:.9g} (rel {abs(r['loss'][0] - r['loss'][1]) / abs(r['loss'][1]):.2e}) dL/dflow rel-L2 {r['seed_rel']:.2e}; grad rel-L2 vs fp64 over {len(e_ours)} tensors: worst "
          f"{worst[0]} {worst[1]:.2e} (fp32 oracle there {e_32[worst[0]]:.2e}; fp32 oracle worst {max(e_32.values()):.2e})")
    return r


def assert_model(cid, c, r):
    B, H, W = c["shape"]
    _assert_common(cid, r, model_cap(c), MODEL_STATE_TOL)
    assert r["flow_shapes"] == [(B, 2, H, W)] * (4 * r["T"]), (cid, r["flow_shapes"])
    assert r["flow_excess"] <= FLOW_ATOL, (cid, r["flow_excess"])
    assert abs(r["loss"][0] - r["loss"][1]) <= wide(REF_MODEL_LOSS.get(cid), LOSS_RTOL) * abs(r["loss"][1]), (cid, r["loss"])


# ---------------------------------------------------------------------------
# the host-side selection of csrc/unet.hip, restated (labels only; pinned to the library on the CPU)
# ---------------------------------------------------------------------------
MAX_KSPLIT, WG_PS, WG_RCHUNK = 16, 64, 16


def _conv(kind, B, Ho, Wo, M, k, segs, kct, mp, pclass=-1, xpart=0):
    """A conv (xparts 1) or input-gradient (xparts 3) launch; segs: (H, W, cpitch, mode)."""
    return {"kind": kind, "B": B, "Ho": Ho, "Wo": Wo, "M": M, "k": k, "segs": segs, "kct": kct, "mpad": mp,
            "xparts": 3 if kind == "dgrad" else 1, "pclass": pclass, "xpart": xpart}


def _wgrad(B, Ho, Wo, M, k, seg):
    return {"kind": "wgrad", "B": B, "Ho": Ho, "Wo": Wo, "M": M, "k": k, "segs": [seg]}


def dom_pixels(l):
    if l.get("pclass", -1) >= 0:
        return l["B"] * ((l["Ho"] - (l["pclass"] >> 1) + 1) // 2) * ((l["Wo"] - (l["pclass"] & 1) + 1) // 2)
    return l["B"] * l["Ho"] * l["Wo"]


def dgrad_bm96(M):
    return (M + 95) // 96 * 96 < (M + 127) // 128 * 128


def conv_tile(l):
    M = l["M"]
    if l["xparts"] == 3:
        bm = 160 if 128 < M <= 160 else ((96 if dgrad_bm96(M) else 128) if M > 64 else (64 if M > 32 else 32))
        return bm, (128 if M > 32 else 256)
    if M > 64:
        return 128, 128
    if M > 32:
        return 64, 128
    return (32, 256) if M > 16 else (16, 256)


def conv_ksplit(l):
    bm, bn = conv_tile(l)
    tiles = ((l["M"] + bm - 1) // bm) * ((dom_pixels(l) + bn - 1) // bn)
    taps = l["k"] * l["k"]
    if l["pclass"] >= 0:
        pad = l["k"] // 2
        ky0, kx0 = ((l["pclass"] >> 1) + pad) & 1, ((l["pclass"] & 1) + pad) & 1
        taps = ((l["k"] - ky0 + 1) // 2) * ((l["k"] - kx0 + 1) // 2)
    steps = sum(taps * (s[2] // 32) for s in l["segs"])
    ks = 1
    while ks < MAX_KSPLIT and tiles * ks < 512 and steps // (2 * ks) >= 16:
        ks *= 2
    return ks


def _w_offsets_32bit(l):
    return 3 * l["k"] * l["k"] * l["kct"] * l["mpad"] * 32 < 2 ** 31


def conv_label(l):
    """The instantiation snnflow_unet_conv dispatches: tile rows and the LDS-DMA (``dma``) or the
    register-staged (``reg``) kernel; ``-pc``: one parity class of a transposed stride-2 segment."""
    bm, _ = conv_tile(l)
    taps32 = l["k"] * l["k"] <= 32
    if l["xparts"] == 3:
        H, W, cp, mode = l["segs"][0]
        ok = (len(l["segs"]) == 1 and taps32 and _w_offsets_32bit(l) and (2 * l["xpart"] + l["B"] * H * W * cp) * 2 < 2 ** 31
              and (mode == T2) == (l["pclass"] >= 0) and mode != S2)
        return f"dgrad{bm}-{'dma' if ok and l['M'] > 32 else 'reg'}" + ("-pc" if l["pclass"] >= 0 else "")
    ok = (l["pclass"] < 0 and taps32 and _w_offsets_32bit(l)
          and all(l["B"] * H * W * cp * 2 < 2 ** 31 and mode in (S1, S2) for H, W, cp, mode in l["segs"]))
    return f"fwd{bm}-{'dma' if ok else 'reg'}"


def wrows_eligible(l):
    H, W, cp, mode = l["segs"][0]
    Ho, Wo = l["Ho"], l["Wo"]
    if l["k"] != 3 or Wo < 8 or (Wo % 64 != 0 and 64 % Wo != 0):
        return False
    if Ho % (64 // min(Wo, 64)) != 0:
        return False
    if mode == S1:
        return H == Ho and W == Wo
    return mode == S2 and l["M"] > 32 and (H + 1) // 2 == Ho and (W + 1) // 2 == Wo


def wgrad_tile(cp, M):
    tm = 32 if M <= 32 else (64 if M <= 64 else 128)
    best, tbest, tk = 1 << 30, 32, 0
    for c in (128, 160, 96, 64, 32):
        if c == 160 and tm > 64:
            continue
        padded = (cp + c - 1) // c * c
        if tk == 0 and 5 * (padded - cp) <= cp:
            tk = c
        if padded < best:
            best, tbest = padded, c
    return tk or tbest, tm


def wgrad_plan(l, rows=None):
    """(label, tk, tm, ktiles, mtiles, taps in the partial tiles, nsplit) of a weight-gradient launch.
    ``rows`` False: the generic kernel's plan even where the row strips are eligible."""
    H, W, cp, mode = l["segs"][0]
    M, P = l["M"], l["B"] * l["Ho"] * l["Wo"]
    if wrows_eligible(l) if rows is None else rows:
        label, (tk, tm) = ("rows-s2", (32, 64)) if mode == S2 else (("rows-m32", (64, 32)) if M <= 32 else ("rows-m64", (32, 64)))
        ktiles, mtiles = (cp + tk - 1) // tk, (M + tm - 1) // tm
        nstrips = P // 64
        ns = max(1, min((1024 + ktiles * mtiles - 1) // (ktiles * mtiles), nstrips // 8))
        steps = (nstrips + ns - 1) // ns
        return label, tk, tm, ktiles, mtiles, 9, (nstrips + steps - 1) // steps
    tk, tm = wgrad_tile(cp, M)
    ktiles, mtiles = (cp + tk - 1) // tk, (M + tm - 1) // tm
    tiles = l["k"] * l["k"] * ktiles * mtiles
    total_steps = (P + WG_PS - 1) // WG_PS
    nsplit = max(1, min((1024 + tiles - 1) // tiles, total_steps // 8))
    return f"wg{tk}x{tm}", tk, tm, ktiles, mtiles, l["k"] * l["k"], nsplit


def wgrad_partial_floats(l, rows=None):
    _, tk, tm, ktiles, mtiles, taps, nsplit = wgrad_plan(l, rows)
    n = nsplit * taps * ktiles * tk * mtiles * tm
    if nsplit > WG_RCHUNK:  # the chunk sums of the two-pass split reduction
        n += (nsplit + WG_RCHUNK - 1) // WG_RCHUNK * l["k"] * l["k"] * l["segs"][0][2] * l["M"]
    return n


def _nsplit_class(n):
    return "1" if n == 1 else ("2-16" if n <= WG_RCHUNK else ">16")


def launch_labels(l):
    """The coverage labels of a launch."""
    if l["kind"] == "wgrad":
        label, *_, nsplit = wgrad_plan(l)
        return [label, f"{'rows' if label.startswith('rows') else 'wg'}-nsplit{_nsplit_class(nsplit)}"]
    return [conv_label(l), "splitk1" if conv_ksplit(l) == 1 else "splitk>1"]


def predicted_plan(l):
    """The launch as snnflow.unet logs it in PLAN_LOG: (kind, M, K, P, plan)."""
    K = sum(s[2] for s in l["segs"])
    if l["kind"] == "wgrad":
        return ("wgrad", l["M"], K, l["B"] * l["Ho"] * l["Wo"], wgrad_partial_floats(l))
    return (l["kind"], l["M"], K, dom_pixels(l), conv_ksplit(l))


REQUIRED_LABELS = (["fwd16-dma", "fwd32-dma", "fwd64-dma", "fwd128-dma", "fwd16-reg", "fwd32-reg", "fwd64-reg", "fwd128-reg",
                    "dgrad32-reg", "dgrad64-dma",
                    "dgrad96-dma", "dgrad128-dma", "dgrad160-dma", "dgrad>32-reg", "*-pc", "splitk1", "splitk>1"]
                   + [f"wg{tk}x{tm}" for tk in (32, 64, 96, 128, 160) for tm in (32, 64, 128) if (tk, tm) != (160, 128)]
                   + ["rows-s2", "rows-m32", "rows-m64", "wg-nsplit1", "wg-nsplit2-16", "wg-nsplit>16", "rows-nsplit>16"])


def label_reached(req, labels):
    if req == "dgrad>32-reg":
        return any(x.startswith("dgrad") and "-reg" in x and not x.startswith("dgrad32") for x in labels)
    if req == "*-pc":
        return any(x.endswith("-pc") for x in labels)
    return req in labels


def lib_conv_ksplit(l):
    """snnflow_unet_conv_ksplit of the launch (host only)."""
    from snnflow import _lib

    a = _lib.UNetConvArgs()
    a.B, a.Ho, a.Wo, a.M, a.ksize, a.nseg = l["B"], l["Ho"], l["Wo"], l["M"], l["k"], len(l["segs"])
    for n, (H, W, cp, mode) in enumerate(l["segs"]):
        a.seg[n] = _lib.UNetSeg(None, H, W, cp, mode, 0, 3)
    a.kct, a.mpad, a.xparts, a.xpart, a.pclass = l["kct"], l["mpad"], l["xparts"], l["xpart"], l["pclass"]
    return int(_lib.lib.snnflow_unet_conv_ksplit(ctypes.byref(a)))


def lib_wgrad_partial_floats(l):
    """snnflow_unet_wgrad_partial_floats of the launch (host only)."""
    from snnflow import _lib

    a = _lib.UNetWgradArgs()
    a.B, a.Ho, a.Wo, a.M, a.ksize = l["B"], l["Ho"], l["Wo"], l["M"], l["k"]
    H, W, cp, mode = l["segs"][0]
    a.seg = _lib.UNetSeg(None, H, W, cp, mode, 0, 3)
    return int(_lib.lib.snnflow_unet_wgrad_partial_floats(ctypes.byref(a)))


def _dgrad_launches(B, Hi, Wi, Hg, Wg, M, k, C, stride2):
    """Input gradient into a [B, Hi, Wi] activation with M channels from the gradient planes
    [3][B, Hg, Wg][pad32(C)]: one launch, or one per parity class of a stride-2 conv."""
    gp = pad32(C)
    seg = [(Hg, Wg, gp, T2 if stride2 else S1)]
    xpart = B * Hg * Wg * gp
    return [_conv("dgrad", B, Hi, Wi, M, k, seg, gp // 32, mpad(M), cls, xpart) for cls in (range(4) if stride2 else (-1,))]


def cell_launches(c):
    """The GEMM launches of a standalone-cell case in PLAN_LOG order (snnflow.unet.ConvLIFCellFn): the
    forward convs of the CELL_T steps, then per step, last first: the weight gradient(s), the input
    gradient and the previous-spike gradient."""
    B, H, W = c["shape"]
    Ho, Wo = cell_out_hw(c)
    cin, C, k = c["cin"], c["C"], c["k"]
    px, pz = pad32(3 * cin), pad32(3 * C)
    sx, sz = (H, W, px, S2 if c["stride"] == 2 else S1), (Ho, Wo, pz, S1)
    segs = [sx, sz] if c["rec"] else [sx]
    kct = sum(s[2] for s in segs) // 32
    fwd = [_conv("conv", B, Ho, Wo, C, k, segs, kct, mpad(C))]
    bwd = [_wgrad(B, Ho, Wo, C, k, s) for s in segs] + _dgrad_launches(B, H, W, Ho, Wo, cin, k, C, c["stride"] == 2)
    if c["rec"]:
        bwd += _dgrad_launches(B, Ho, Wo, Ho, Wo, C, k, C, False)
    return fwd * CELL_T + bwd * CELL_T


def model_launches(c):
    """The GEMM launches of a model case in PLAN_LOG order (snnflow.unet.UNetStep forward and
    backward): MODEL_T forward steps, then the backward steps, last first.  The recurrent cells' second
    segment (the previous spikes) takes part from the second step on, or from the first with given states."""
    B = c["shape"][0]
    H, W = padded_hw(c)
    base, k = c["base"], 3
    Cs = [base << (i + 1) for i in range(4)]
    cm = Cs[-1]
    dec = []  # (C, input pitch, h2, w2)
    for i in range(4):
        cx = Cs[3 - i]
        dec.append((cx // 2, pad32(2 * cx + (6 if i else 0)), H >> (3 - i), W >> (3 - i)))

    def one(seg, B, h, w, M):
        return _conv("conv", B, h, w, M, k, seg, sum(s[2] for s in seg) // 32, mpad(M))

    def forward(rec):
        out, h, w, pitch = [], H, W, 32
        for C in Cs:
            h2, w2, cp = h // 2, w // 2, pad32(C)
            out.append(one([(h, w, pitch, S2)], B, h2, w2, C))
            out.append(one([(h2, w2, cp, S1)] * (2 if rec else 1), B, h2, w2, C))
            h, w, pitch = h2, w2, cp
        out += [one([(h, w, pad32(cm), S1)], B, h, w, cm)] * 4
        for C, p, h2, w2 in dec:
            out.append(one([(h2, w2, p, S1)], B, h2, w2, C))
        return out

    def backward(rec):
        out = []
        for C, p, h2, w2 in reversed(dec):
            out.append(_wgrad(B, h2, w2, C, k, (h2, w2, p, S1)))
            out += _dgrad_launches(B, h2, w2, h2, w2, p, k, C, False)
        h, w = H // 16, W // 16
        for _ in range(4):
            out.append(_wgrad(B, h, w, cm, k, (h, w, pad32(cm), S1)))
            out += _dgrad_launches(B, h, w, h, w, pad32(cm), k, cm, False)
        for i in range(3, -1, -1):
            C, h, w = Cs[i], H >> (i + 1), W >> (i + 1)
            cp = pad32(C)
            out.append(_wgrad(B, h, w, C, k, (h, w, cp, S1)))
            if rec:
                out.append(_wgrad(B, h, w, C, k, (h, w, cp, S1)))
                out += _dgrad_launches(B, h, w, h, w, C, k, C, False)
            out += _dgrad_launches(B, h, w, h, w, cp, k, C, False)
            pin = pad32(Cs[i - 1]) if i else 32
            out.append(_wgrad(B, h, w, C, k, (2 * h, 2 * w, pin, S2)))
            if i:
                out += _dgrad_launches(B, 2 * h, 2 * w, h, w, pin, k, C, True)
        return out

    recs = [c["given"] or t > 0 for t in range(MODEL_T)]
    return [l for r in recs for l in forward(r)] + [l for r in reversed(recs) for l in backward(r)]
