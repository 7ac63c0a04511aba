"""Cases, data and oracle of the K x K cell tests (model.kernel_size 1, 5, 7; csrc/convk.hip):
``firenet_harness``'s cell recipe with ``k`` in place of its hard-coded 3, and its compare / assert
functions as they are.  test_convk_cpu.py holds the oracle alone to the rules here; test_gpu_convk.py
runs the HIP cells against it."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import firenet_harness as fh  # noqa: E402

# (K, B, H, W, C, cin, recurrent, train), data seed.  5x7 is smaller than the K = 7 footprint (every pixel
# sees zero padding on both sides), 9x33 is one pixel past the tile in both directions, 12x58 has two
# partial tile rows and a ragged last column.  Seeds: chosen on the CPU from the fp64 oracle alone
# (test_convk_cpu.py::test_cell_near_threshold_cap).
_CASES = [
    ((5, 1, 5, 7, 8, 2, False, True), 100),
    ((5, 3, 9, 33, 8, 8, False, True), 100),
    ((5, 3, 9, 33, 8, 8, True, True), 100),
    ((5, 3, 9, 33, 8, 2, True, True), 101),
    ((5, 3, 9, 33, 8, 8, True, False), 100),
    ((5, 3, 9, 33, 4, 4, True, True), 100),
    ((5, 3, 9, 33, 16, 16, True, True), 102),
    ((5, 2, 12, 58, 32, 32, False, True), 102),
    ((5, 2, 12, 58, 32, 32, True, True), 100),
    ((7, 1, 5, 7, 8, 8, True, True), 100),
    ((7, 3, 9, 33, 8, 2, False, True), 100),
    ((7, 3, 9, 33, 32, 32, True, True), 100),
    ((1, 3, 9, 33, 8, 2, False, True), 101),
    ((1, 3, 9, 33, 8, 8, True, True), 101),
    ((1, 2, 12, 58, 32, 32, False, True), 100),
]
CELL_CASES = [c for c, _ in _CASES]


def cell_id(case):
    return f"K{case[0]}-{fh.cell_id(case[1:])}"


CELL_SEED = {cell_id(c): s for c, s in _CASES}

# The float-input case (test_gpu_convk.py::test_cell_convk_float_input): K = 5, C = cin = 8, feed-forward,
# 3x9x33, input 0.7 * randn instead of spikes; its seed by the same rule.
FLOAT_CASE = (5, 3, 9, 33, 8, 8, False, True)
FLOAT_SEED = 105  # (100 .. 104 leave 1 to 3 neurons of the fp64 oracle within 1e-4 of the threshold; cap 0)
FLOAT_ID = cell_id(FLOAT_CASE) + "-float"


def cell_cap(case):
    return fh.cell_cap(case[1:])


def cell_data(case, seed=None, float_input=False):
    """``firenet_harness.cell_data`` with a K x K oracle cell (same draws in the same order).
    ``float_input``: the input is 0.7 * randn (drawn in the input's place), not spikes or counts."""
    from oracle import lif_ref

    K, B, H, W, C, cin, rec, train = case
    seed = CELL_SEED[cell_id(case)] if seed is None else seed
    torch.manual_seed(1000 + seed)
    ref = lif_ref.SnnTorchCellRef(cin, C, K, recurrent=rec)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        ref.bn.weight.copy_(0.5 + torch.rand(C, generator=gen))
        ref.bn.bias.copy_(0.2 * torch.randn(C, generator=gen))
        ref.bn.running_mean.copy_(0.2 * torch.randn(C, generator=gen))
        ref.bn.running_var.copy_(0.5 + torch.rand(C, generator=gen))
    if float_input:
        x = 0.7 * torch.randn(B, cin, H, W, generator=gen)
    elif cin == 2:  # event counts
        x = torch.floor(torch.rand(B, cin, H, W, generator=gen) * 4) * (torch.rand(B, cin, H, W, generator=gen) < 0.4).float()
    else:           # spikes of the layer below
        x = (torch.rand(B, cin, H, W, generator=gen) < 0.3).float()
    prev = torch.stack([torch.randn(B, C, H, W, generator=gen) * 0.5,
                        (torch.rand(B, C, H, W, generator=gen) < 0.2).float()])
    n = B * C * H * W
    wgt = (torch.linspace(-1, 1, n) + 0.5 * torch.randn(n, generator=gen)).view(B, C, H, W)
    return {k: v.clone() for k, v in ref.state_dict().items()}, x, prev, wgt


def cell_oracle(case, sd, x, prev, wgt, dtype, ours=None, eps=fh.EPS):
    """``firenet_harness.cell_oracle`` with a K x K oracle cell: same adoption rule, same result dict."""
    from oracle import lif_ref

    K, B, H, W, C, cin, rec, train = case
    ref = lif_ref.SnnTorchCellRef(cin, C, K, recurrent=rec)
    ref.load_state_dict(sd)
    ref = ref.to(dtype).train(train)
    xi = x.to(dtype).clone().requires_grad_(True)
    pi = prev.to(dtype).clone().requires_grad_(True)
    spk, st = ref(xi, pi)
    near = (ref.lif.last_v - ref.lif.threshold.detach()).abs() < eps
    out = {"near": int(near.sum()), "adopted": 0, "hard": 0, "adopt_mask": torch.zeros_like(near)}
    mem = st[0].detach()
    if ours is not None:
        ospk, ostate = ours[0].detach().cpu().to(dtype), ours[1].detach().cpu().to(dtype)
        diff = spk.detach() != ospk
        adopt = diff & near
        out["hard"], out["adopted"], out["adopt_mask"] = int((diff & ~near).sum()), int(adopt.sum()), adopt
        spk = spk + torch.where(adopt, ospk - spk.detach(), torch.zeros_like(ospk))
        mem = torch.where(adopt, ostate[0], mem)
    (spk * wgt.to(dtype)).sum().backward()
    out.update(spk=spk.detach(), mem=mem, run_mean=ref.bn.running_mean.clone(), run_var=ref.bn.running_var.clone(),
               nbt=int(ref.bn.num_batches_tracked),
               grads={**{n: p.grad.detach() for n, p in ref.named_parameters()}, "input": xi.grad,
                      **({"prev_state": pi.grad} if rec else {})})
    return out


# Reference against reference: worst membrane excess over rtol 1e-5 of the fp32 CPU oracle against the fp64
# oracle per case (test_convk_cpu.py::test_cell_fp32_oracle_vs_fp64 prints them; every case: 0 spike
# differences, worst gradient relative L2 -- the previous-state gradient included -- <= 1.7e-6).  A
# case's GPU limit may be set to 4 x its figure where the GPU exceeds CELL_ATOL and stays within that.
REF_CELL_MEM = {"K5-1x5x7-C8-cin2-ff-train": 0.0, "K5-3x9x33-C8-cin8-ff-train": 3.27e-7,
                "K5-3x9x33-C8-cin8-rec-train": 6.97e-7, "K5-3x9x33-C8-cin2-rec-train": 2.51e-7,
                "K5-3x9x33-C8-cin8-rec-eval": 1.01e-6, "K5-3x9x33-C4-cin4-rec-train": 1.38e-7,
                "K5-3x9x33-C16-cin16-rec-train": 1.18e-6, "K5-2x12x58-C32-cin32-ff-train": 2.21e-6,
                "K5-2x12x58-C32-cin32-rec-train": 1.85e-6, "K7-1x5x7-C8-cin8-rec-train": 4.24e-8,
                "K7-3x9x33-C8-cin2-ff-train": 1.74e-7, "K7-3x9x33-C32-cin32-rec-train": 1.83e-6,
                "K1-3x9x33-C8-cin2-ff-train": 1.90e-8, "K1-3x9x33-C8-cin8-rec-train": 7.79e-8,
                "K1-2x12x58-C32-cin32-ff-train": 4.65e-7, "K5-3x9x33-C8-cin8-ff-train-float": 5.66e-7}

# Whole model, LIFFireNet C = 8 at (3, 9, 33), T = 3 windows of 300 events: worst parameter-gradient
# relative L2 of the fp32 CPU oracle against the fp64 oracle (oracle_as_ours through oracle_run / compare,
# test_convk_cpu.py::test_train_step_fp32_oracle_vs_fp64 prints it).  The figure is the loss's, as
# firenet_harness.REF_STEP_GRAD explains; the fp64 leg of the GPU step may be held to 4 x it.
REF_STEP_GRAD = {5: 7.058e-5, 1: 3.298e-5}
STEP_SHAPE = (3, 9, 33)


def step_id(K):
    return f"LIFFireNet-K{K}-C8-3x9x33"


def patch_kernel_size(monkeypatch, K):
    """``lif_ref.make_unet_kwargs`` returning ``"kernel_size": K``: ``fh.new_model``, ``fh.oracle_run``,
    ``fh.oracle_as_ours`` and ``fh.oracle_eval`` then build K x K models unchanged."""
    from oracle import lif_ref

    real = lif_ref.make_unet_kwargs

    def make(*args, **kw):
        d = real(*args, **kw)
        d["kernel_size"] = K
        return d

    monkeypatch.setattr(lif_ref, "make_unet_kwargs", make)
