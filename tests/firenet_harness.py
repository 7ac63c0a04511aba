"""Shared harness (a plain helper module, imported like loader_ref.py / vis_ref.py): the LIFFireNet
family's train step and its cells against the CPU oracle (oracle/lif_ref.py + oracle/iwe_ref.py).

Whole train step (``gpu_run`` / ``oracle_run`` / ``compare`` / ``report``; test_gpu_fullsize.py and
test_gpu_ragged.py): "ours" runs forward + EventWarping + backward and hands over every step's states;
the oracle then runs the same windows from the same initial weights layer by layer (``oracle_step``),
counts the spikes that differ from ours and -- with ``eps`` -- adopts ours (straight-through: value
ours, the oracle's graph and surrogate kept, with our reset membrane) wherever its own pre-reset
membrane lies within eps of the threshold.  A differing spike anywhere else is counted as ``hard`` and
fails the caller's test.  ``oracle_as_ours`` runs the fp32 CPU oracle free in the role of "ours", so a
machine without a GPU can drive the same compare functions (test_ragged_cpu.py) and measure the
reference-against-reference error the tolerances rest on.

One cell, one step (``CELL_CASES`` / ``cell_data`` / ``cell_oracle`` / ``cell_compare``): random
previous state, non-uniform upstream gradient; the same adoption rule with a counted cap.

``dtype``: the oracle's precision.  With torch.float64 the cells (``ref.double()``: convolutions,
BatchNorm and its running statistics, LIF, surrogate), the prediction layer and the whole of
EventWarpingRef (gather, warp, bilinear splat, loss, smoothing) run in fp64 on fp64 inputs and states;
nothing the harness calls in oracle/lif_ref.py or oracle/iwe_ref.py hard-codes fp32 (the numpy
bit-exact corner restatement ``warp_corners_np`` does, and is not part of the train step).  The AEE of
``compare`` goes through oracle/metrics_ref.py on fp32 copies of the flows, as before."""
import numpy as np
import torch

EPS = 1e-4  # |v - theta| below which a spike is fp32-ill-conditioned (SURVEY finding 4)

# (B, H, W): the smallest image sizes at which each boundary of the 8 x 32-pixel tiles exists
RAGGED_SHAPES = [(1, 5, 7),     # one partial tile in both directions; odd W < 32; 35 pixels per BatchNorm channel
                 (3, 9, 33),    # 2 x 2 tiles, last row / column one pixel thick; padding starts at row 9; odd B
                 (2, 15, 31),   # one short of the tile multiples
                 (2, 12, 58),   # MVSEC's residues (260 x 346: 4 rows, 26 columns); W no multiple of 4
                 (3, 17, 65)]   # 3 x 3 tiles: a full interior tile surrounded by ragged ones


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def cfg(H, W):
    return {"loader": {"resolution": [H, W]}, "loss": {"flow_regul_weight": 0.001, "overwrite_intermediate": False},
            "model": {"mask_output": True}}


def aee_pair(flow_ours, flow_ref, gt, mask, dev):
    """AEE of our flow through snnflow.AEE (HIP) and of the oracle's flow through the oracle's
    metric restatement (oracle/metrics_ref.py, pinned by eval_case.npz)."""
    import snnflow
    from oracle.metrics_ref import flow_metrics_ref

    B, _, H, W = flow_ours.shape
    m = snnflow.AEE(cfg(H, W), dev, flow_scaling=128)
    ev = torch.zeros(B, 1, 4, device=dev)
    one = torch.ones(1)
    m.event_flow_association([flow_ours], {"event_list": ev, "event_list_pol_mask": torch.zeros(B, 1, 2, device=dev),
                                           "event_mask": mask.to(dev), "gtflow": gt.to(dev),
                                           "dt_input": one, "dt_gt": one})
    aee, _ = m()
    ref = flow_metrics_ref(flow_ref.float(), gt, mask, one, one, 128)["aee"]
    return aee.cpu().numpy().astype(np.float64), ref.numpy().astype(np.float64)


def oracle_step(ref, x, ours, eps):
    """One oracle time step, layer by layer (oracle/lif_ref.py LIFFireNetRef.forward).  Every
    oracle spike that differs from ours (``ours``: our [2,B,C,H,W] states of this step) is
    counted; if ``eps`` is set, a differing spike whose pre-reset membrane lies within eps of the
    threshold (fp32-ill-conditioned) is replaced by ours, straight-through (value ours, the
    oracle's graph and surrogate kept), with our reset membrane.  Returns (flow, flips per layer,
    flips NOT within eps of the threshold)."""
    h, flips, hard = x, [], 0
    for i, (name, _) in enumerate(ref.spec):
        cell = getattr(ref, name)
        spk, st = cell(h, ref._states[i])
        mine = ours[i].to(spk.dtype)
        diff = spk.detach() != mine[1]
        n = int(diff.sum())
        flips.append(n)
        if n:
            near = (cell.lif.last_v - cell.lif.threshold.detach()).abs() <= (eps or 0.0)
            hard += int((diff & ~near).sum())
            if eps:
                spk = spk + (mine[1] - spk).detach()
                st = torch.stack([torch.where(diff, mine[0], st[0]), spk])
        ref._states[i] = st
        h = spk
    return ref.pred(h), flips, hard


def new_model(C, name="LIFFireNet"):
    import snnflow
    from oracle import lif_ref

    torch.manual_seed(0)
    return getattr(snnflow, name)(lif_ref.make_unet_kwargs(base_num_channels=C))


def gpu_run(dev, path, wins, C, name="LIFFireNet", model=None):
    """The train step's forward + loss + backward on the GPU; returns (model, initial state dict,
    flows, loss, per-step CPU copies of the L states).  ``model``: a prepared model in place of a
    fresh ``new_model(C, name)`` (engine switches set, states given)."""
    import snnflow

    if model is None:
        model = new_model(C, name).to(dev).train()
    init = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    B, _, H, W = wins[0]["event_cnt"].shape
    ew = snnflow.EventWarping(cfg(H, W), dev)
    states = []
    if path == "sequence":
        model.engine.capture_states = True
        try:
            outs = model.forward_sequence([w["event_voxel"] for w in wins], [w["event_cnt"] for w in wins])
        finally:
            model.engine.capture_states = False
        flows = [o["flow"][0] for o in outs]
        states = [[s.detach().cpu() for s in sts] for sts in model.engine.seq_states]
        model.engine.seq_states = None
    else:
        flows = []
        for w in wins:
            flows.append(model(w["event_voxel"], w["event_cnt"])["flow"][0])
            states.append([s.detach().cpu() for s in model._states])
    for t, w in enumerate(wins):
        ew.event_flow_association([flows[t]], w["event_list"], w["event_list_pol_mask"], w["event_mask"])
    loss = ew()
    loss.backward()
    return model, init, flows, loss.item(), states


def _new_ref(init, C, name, dtype, train=True):
    from oracle import lif_ref

    ref = lif_ref.LIFFireNetRef(lif_ref.make_unet_kwargs(base_num_channels=C), name).train(train)
    ref.load_state_dict(init)
    return ref.to(dtype) if dtype is not None else ref


def _cast(w, dtype):
    return w if dtype is None else {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in w.items()}


def oracle_run(init, C, cpu_wins, ours_states, eps, name="LIFFireNet", dtype=None):
    """The oracle's train step on the same windows and initial weights, following our spikes as
    ``oracle_step`` describes.  ``dtype``: the oracle's precision (None: fp32 as loaded).  Returns
    (oracle, flows, loss, flips [T, L], hard)."""
    from oracle import iwe_ref

    B, _, H, W = cpu_wins[0]["event_cnt"].shape
    ref = _new_ref(init, C, name, dtype)
    rew = iwe_ref.EventWarpingRef([H, W], weight=0.001)
    flows, flips, hard = [], [], 0
    for t, w in enumerate(cpu_wins):
        w = _cast(w, dtype)
        f, fl, hd = oracle_step(ref, w["event_cnt"], ours_states[t], eps)
        flows.append(f)
        flips.append(fl)
        hard += hd
        rew.event_flow_association([f], w["event_list"], w["event_list_pol_mask"], w["event_mask"])
    loss = rew()
    loss.backward()
    return ref, flows, loss.item(), np.array(flips), hard


def oracle_as_ours(cpu_wins, C, name="LIFFireNet", dtype=None):
    """The oracle, free-running, in the role of "ours" (what ``gpu_run`` returns): the fp32 CPU
    oracle against the fp64 oracle goes through ``oracle_run`` / ``compare`` like a GPU run."""
    from oracle import iwe_ref

    init = {k: v.detach().clone() for k, v in new_ref_init(C, name).items()}
    B, _, H, W = cpu_wins[0]["event_cnt"].shape
    ref = _new_ref(init, C, name, dtype)
    rew = iwe_ref.EventWarpingRef([H, W], weight=0.001)
    flows, states = [], []
    for w in cpu_wins:
        w = _cast(w, dtype)
        f = ref(w["event_voxel"], w["event_cnt"])["flow"][0]
        flows.append(f)
        states.append([s.detach().clone() for s in ref._states])
        rew.event_flow_association([f], w["event_list"], w["event_list_pol_mask"], w["event_mask"])
    loss = rew()
    loss.backward()
    return ref, init, flows, loss.item(), states


def new_ref_init(C, name="LIFFireNet"):
    """Initial parameters and buffers of ``new_model(C, name)`` without building the HIP model: the
    oracle draws from the torch RNG in the same order (oracle/lif_ref.py)."""
    from oracle import lif_ref

    torch.manual_seed(0)
    return lif_ref.LIFFireNetRef(lif_ref.make_unet_kwargs(base_num_channels=C), name).state_dict()


def compare(tag, model, flows, loss, ref, rflows, rloss, flips, cpu_wins, C=None, aee=True):
    """Differences of ours (model, flows, loss) from the oracle's: flips, loss, per-step flow
    relative L2 and max-abs, every parameter gradient's relative L2, and (``aee``, needs the GPU)
    the AEE of a synthetic ground truth through both metrics.  Printed by ``report``."""
    B, _, H, W = cpu_wins[0]["event_cnt"].shape
    r = {"flips": flips, "loss": (loss, rloss),
         "flow_rel": [rel(f.detach().cpu().numpy(), q.detach().numpy()) for f, q in zip(flows, rflows)],
         "flow_maxabs": max(float((f.detach().cpu() - q.detach()).abs().max()) for f, q in zip(flows, rflows)),
         "grad_rel": {n: rel(a.grad.cpu().numpy(), b.grad.numpy())
                      for (n, a), (_, b) in zip(model.named_parameters(), ref.named_parameters())}}
    # BatchNorm running statistics after the T steps (their pixel count is B H W, not the tile-padded one):
    # worst |ours - oracle| - 1e-5 |oracle| (held to atol 1e-6 by assert_step), num_batches_tracked equal
    so, sr = model.state_dict(), ref.state_dict()
    run = [k for k in sr if k.endswith(("running_mean", "running_var"))]
    r["stats_excess"] = max(float(((so[k].detach().cpu().double() - sr[k].double()).abs()
                                   - 1e-5 * sr[k].double().abs()).max()) for k in run)
    r["nbt_equal"] = all(int(so[k]) == int(sr[k]) for k in sr if k.endswith("num_batches_tracked"))
    if aee:
        gtg = torch.Generator().manual_seed(2)
        gt = (torch.rand(B, 2, H, W, generator=gtg) - 0.5) * 8.0
        r["aee"] = aee_pair(flows[-1].detach(), rflows[-1].detach(), gt, cpu_wins[-1]["event_mask"],
                            flows[-1].device)
    report(tag, r, B * (C if C is not None else model.engine.C) * H * W)
    return r


def report(tag, r, per_layer):
    print(f"\n[{tag}] spike flips per step x layer (of {per_layer} each):\n{r['flips']}")
    print(f"[{tag}] loss ours {r['loss'][0]:.9g} oracle {r['loss'][1]:.9g} "
          f"rel {abs(r['loss'][0] - r['loss'][1]) / abs(r['loss'][1]):.3e}")
    print(f"[{tag}] flow rel-L2 per step {['%.2e' % v for v in r['flow_rel']]} max|d| {r['flow_maxabs']:.3e}")
    if "aee" in r:
        print(f"[{tag}] AEE ours {np.round(r['aee'][0], 6).tolist()} oracle {np.round(r['aee'][1], 6).tolist()} "
              f"max|dAEE| {np.abs(r['aee'][0] - r['aee'][1]).max():.3e}")
    if "stats_excess" in r:
        print(f"[{tag}] running statistics: excess over rtol 1e-5 {r['stats_excess']:.2e}, "
              f"num_batches_tracked equal {r['nbt_equal']}")
    worst = max(r["grad_rel"].items(), key=lambda kv: kv[1])
    print(f"[{tag}] grad rel-L2 worst {worst[0]} {worst[1]:.3e}; all: "
          + ", ".join(f"{k}={v:.1e}" for k, v in r["grad_rel"].items()))


def cpu_windows(B, H, W, T, N, seed):
    """T synthetic windows drawn on the CPU (the same on every machine; a GPU test moves them)."""
    from snnflow.synthetic import make_window

    gen = torch.Generator().manual_seed(seed)
    return [make_window(B, N, H, W, gen, "cpu") for _ in range(T)]


# ---------------------------------------------------------------------------
# one cell, one step, teacher-forced
# ---------------------------------------------------------------------------
def _cell_cases():
    """(B, H, W, C, cin, recurrent, train): every (C, recurrent) pair at 9x33 and 12x58, every shape
    at C = 8 and C = 32; feed-forward cin in {2, C}, recurrent cin = C plus (2, 8), the narrow-input
    recurrent kernel; one eval-mode case (running statistics away from (0, 1)) per C."""
    cases = []
    for C in (4, 8, 16, 32):
        shapes = RAGGED_SHAPES if C in (8, 32) else [(3, 9, 33), (2, 12, 58)]
        kinds = [(2, False), (C, False), (C, True)] + ([(2, True)] if C == 8 else [])
        for B, H, W in shapes:
            for cin, rec in kinds:
                cases.append((B, H, W, C, cin, rec, True))
        cases.append((3, 9, 33, C, C, True, False))
    return cases


CELL_CASES = _cell_cases()

# Data seed of a cell case where the default (the case's index) leaves a neuron of the fp64 oracle within
# EPS of the threshold beyond the cap (test_ragged_cpu.py::test_cell_near_threshold_cap holds the rule:
# seeds are chosen on the CPU, from the oracle alone).
CELL_SEED = {"3x9x33-C4-cin4-rec-train": 100, "1x5x7-C8-cin2-ff-train": 100, "3x9x33-C8-cin8-ff-train": 100,
             "3x9x33-C8-cin8-rec-train": 100, "3x9x33-C8-cin2-rec-train": 101, "2x15x31-C8-cin2-ff-train": 100,
             "2x15x31-C8-cin8-ff-train": 100, "3x9x33-C8-cin8-rec-eval": 100, "3x9x33-C16-cin16-rec-train": 100,
             "1x5x7-C32-cin32-rec-train": 100, "3x9x33-C32-cin2-ff-train": 100, "3x9x33-C32-cin32-ff-train": 102,
             "3x9x33-C32-cin32-rec-train": 100, "2x15x31-C32-cin2-ff-train": 100, "2x15x31-C32-cin32-rec-train": 101,
             "2x12x58-C32-cin32-ff-train": 100, "3x17x65-C32-cin2-ff-train": 100, "3x9x33-C32-cin32-rec-eval": 100}


def cell_id(case):
    B, H, W, C, cin, rec, train = case
    return f"{B}x{H}x{W}-C{C}-cin{cin}-{'rec' if rec else 'ff'}-{'train' if train else 'eval'}"


def cell_cap(case):
    """The most near-threshold neurons a case may hold (and so the most spikes it may adopt):
    0.01 % of its neurons, rounded down -- 0 for 5x7 (35 C neurons) and for every case below 10^4."""
    B, H, W, C = case[:4]
    return (B * H * W * C) // 10000


def cell_data(case):
    """Parameters (a state dict in the oracle's / the HIP cell's common layout), input, previous
    state and upstream-gradient weight of a case, all fp32 on the CPU.  The weight is a ramp over
    the flattened [B,C,H,W] index plus noise: non-uniform, and not symmetric under a flip of the
    image in either direction (a mirrored or transposed halo changes every gradient)."""
    from oracle import lif_ref

    B, H, W, C, cin, rec, train = case
    seed = CELL_SEED.get(cell_id(case), CELL_CASES.index(case))
    torch.manual_seed(1000 + seed)
    ref = lif_ref.SnnTorchCellRef(cin, C, 3, recurrent=rec)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        ref.bn.weight.copy_(0.5 + torch.rand(C, generator=gen))
        ref.bn.bias.copy_(0.2 * torch.randn(C, generator=gen))
        ref.bn.running_mean.copy_(0.2 * torch.randn(C, generator=gen))
        ref.bn.running_var.copy_(0.5 + torch.rand(C, generator=gen))
    if cin == 2:  # event counts
        x = torch.floor(torch.rand(B, cin, H, W, generator=gen) * 4) * (torch.rand(B, cin, H, W, generator=gen) < 0.4).float()
    else:         # spikes of the layer below
        x = (torch.rand(B, cin, H, W, generator=gen) < 0.3).float()
    prev = torch.stack([torch.randn(B, C, H, W, generator=gen) * 0.5,
                        (torch.rand(B, C, H, W, generator=gen) < 0.2).float()])
    n = B * C * H * W
    wgt = (torch.linspace(-1, 1, n) + 0.5 * torch.randn(n, generator=gen)).view(B, C, H, W)
    return {k: v.clone() for k, v in ref.state_dict().items()}, x, prev, wgt


def cell_oracle(case, sd, x, prev, wgt, dtype, ours=None, eps=EPS):
    """The oracle cell's step and backward in ``dtype``.  ``ours``: (spikes, state) to follow -- the
    oracle adopts our spike (straight-through, with our reset membrane) where it differs and the
    oracle's pre-reset membrane lies within eps of the threshold.  Returns a dict of results; ``near``
    counts the neurons within eps of the threshold, ``adopted`` / ``hard`` the differing spikes within /
    away from it."""
    from oracle import lif_ref

    B, H, W, C, cin, rec, train = case
    ref = lif_ref.SnnTorchCellRef(cin, C, 3, recurrent=rec)
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


def cell_compare(tag, ours, want):
    """Figures of one cell result against the oracle's (both dicts as ``cell_oracle`` returns, ours
    with tensors on any device): printed, then returned for the caller's assertions.  Membranes are
    compared where no spike was adopted (an adopted spike carries our reset membrane)."""
    def t(v):
        return v.detach().cpu().double()

    keep = ~want["adopt_mask"]
    mo, mw = t(ours["mem"])[keep], t(want["mem"])[keep]
    r = {"finite": all(bool(torch.isfinite(t(v)).all()) for v in
                       [ours["spk"], ours["mem"], ours["run_mean"], ours["run_var"], *ours["grads"].values()]),
         "binary": bool(((t(ours["spk"]) == 0) | (t(ours["spk"]) == 1)).all()),
         "spk_diff": int((t(ours["spk"]) != t(want["spk"])).sum()),
         "mem_excess": float(((mo - mw).abs() - 1e-5 * mw.abs()).max()),      # <= atol 1e-6 asserted
         "mem_rel": rel(mo.numpy(), mw.numpy()),
         "mean_excess": float(((t(ours["run_mean"]) - t(want["run_mean"])).abs() - 1e-5 * t(want["run_mean"]).abs()).max()),
         "var_excess": float(((t(ours["run_var"]) - t(want["run_var"])).abs() - 1e-5 * t(want["run_var"]).abs()).max()),
         "nbt": (int(ours["nbt"]), int(want["nbt"])),
         "grad_rel": {n: rel(t(ours["grads"][n]).numpy(), t(g).numpy()) for n, g in want["grads"].items()}}
    worst = max(r["grad_rel"].items(), key=lambda kv: kv[1])
    print(f"\n[{tag}] near {want['near']} adopted {want['adopted']} hard {want['hard']} spk_diff {r['spk_diff']} "
          f"mem rel {r['mem_rel']:.2e} excess {r['mem_excess']:.2e} mean excess {r['mean_excess']:.2e} "
          f"var excess {r['var_excess']:.2e} grad worst {worst[0]} {worst[1]:.2e}: "
          + ", ".join(f"{k}={v:.1e}" for k, v in r["grad_rel"].items()))
    return r


# ---------------------------------------------------------------------------
# limits
# ---------------------------------------------------------------------------
# One cell: the project's own numbers (test_gpu_parity.py): ORACLE_GRAD_TOL on every gradient's relative
# L2 (recorded worst 4.4e-6), rtol 1e-5 / atol 1e-6 on membranes and running statistics.
CELL_GRAD_TOL = 1e-5
CELL_ATOL = 1e-6

# Whole train step: test_cfg2_train_step_vs_oracle's limits -- loss 1e-5 relative, flows 1e-4 relative
# L2 and max-abs, gradients GRAD_TOL of the matching width (C = 8: cfg2's 6e-6; C = 32: cfg2-C32's
# 5e-5; C = 16 has no headline configuration: ORACLE_GRAD_TOL 1e-5, the bound test_cell_teacher_forced
# and the fused-Adam step hold C = 16 to).
STEP_LOSS_RTOL = 1e-5
STEP_FLOW_TOL = 1e-4
STEP_GRAD_TOL = {8: 6e-6, 16: 1e-5, 32: 5e-5}

# (model, C, (B, H, W)): widths 8 / 16 / 32 at 9x33, 12x58 and 17x65; the short and the feed-forward
# family members at C = 8, 9x33
STEP_CASES = ([("LIFFireNet", C, s) for C in (8, 16, 32) for s in ((3, 9, 33), (2, 12, 58), (3, 17, 65))]
              + [("LIFFireNet_short", 8, (3, 9, 33)), ("LIFFireFlowNet", 8, (3, 9, 33))])
STEP_T, STEP_N = 3, 300
T33_ID = "LIFFireNet-C8-1x9x33-T33"

# Reference against reference: figures of the fp32 CPU oracle against the fp64 oracle through this
# harness (test_ragged_cpu.py prints them), listed where they exceed the limits above.  A case's limit
# may be set to 4 x its figure here where the GPU exceeds the limit above and stays within that.
# cell id: worst membrane excess over rtol 1e-5 (limit 1e-6; C >= 16: 9 C-term convolution sums in fp32)
REF_CELL_MEM = {"3x9x33-C16-cin16-rec-train": 1.07e-6, "2x12x58-C32-cin32-ff-train": 1.20e-6,
                "3x17x65-C32-cin32-ff-train": 1.16e-6, "3x17x65-C32-cin32-rec-train": 7.14e-7}
# step id: worst relative L2 over the parameter gradients.  The loss divides per-pixel sums of bilinear
# weights by (count + 1e-9); a pixel that only a far corner of a barely-moved event touches has a count of
# the order of the fp32 rounding of the warped coordinate, so dL/dflow of the fp32 reference arithmetic
# (which the HIP loss reproduces) is 1e-5 .. 6e-3 away from the fp64 value whatever the image size, and
# the cells' gradients inherit that figure as a common factor (all parameters of a case show the same
# error).  Against the fp32 oracle the same arithmetic cancels: test_gpu_ragged.py holds that leg to
# STEP_GRAD_TOL unwidened.
REF_STEP_GRAD = {"LIFFireNet-C8-3x9x33": 1.989e-5, "LIFFireNet-C8-2x12x58": 1.394e-3, "LIFFireNet-C8-3x17x65": 2.273e-3,
                 "LIFFireNet-C16-3x9x33": 7.738e-6, "LIFFireNet-C16-2x12x58": 4.614e-5,
                 "LIFFireNet-C16-3x17x65": 1.528e-4, "LIFFireNet-C32-3x9x33": 1.757e-5,
                 "LIFFireNet-C32-2x12x58": 1.490e-4, "LIFFireNet-C32-3x17x65": 4.506e-4,
                 "LIFFireNet_short-C8-3x9x33": 6.138e-5, "LIFFireFlowNet-C8-3x9x33": 8.939e-5,
                 "LIFFireNet-C8-1x9x33-T33": 2.616e-6}


def step_id(case):
    name, C, (B, H, W) = case
    return f"{name}-C{C}-{B}x{H}x{W}"


def assert_cell(cid, r, want, cap, wide=None):
    """The assertions of one cell case on ``cell_compare``'s figures.  ``wide``: {"mem" / "grad": limit}
    replacing CELL_ATOL (membrane) / CELL_GRAD_TOL for this case."""
    wide = wide or {}
    assert r["finite"], cid
    assert r["binary"], cid
    assert want["hard"] == 0, f"{cid}: {want['hard']} spikes differ away from the threshold"
    assert want["adopted"] <= cap, f"{cid}: {want['adopted']} spikes adopted, cap {cap}"
    assert r["spk_diff"] == 0, cid
    assert r["mem_excess"] <= wide.get("mem", CELL_ATOL), (cid, r["mem_excess"])
    assert r["mean_excess"] <= CELL_ATOL and r["var_excess"] <= CELL_ATOL, (cid, r["mean_excess"], r["var_excess"])
    assert r["nbt"][0] == r["nbt"][1], (cid, r["nbt"])
    for n, v in r["grad_rel"].items():
        assert v <= wide.get("grad", CELL_GRAD_TOL), (cid, n, v)


def assert_states_sane(cid, states):
    """Every state of every step finite, every spike exactly 0 or 1."""
    for t, sts in enumerate(states):
        for l, st in enumerate(sts):
            assert bool(torch.isfinite(st).all()), (cid, t, l)
            assert bool(((st[1] == 0) | (st[1] == 1)).all()), (cid, t, l)


def assert_step(cid, r, hard, C, wide=None):
    """The flip-corrected leg's assertions (those of test_cfg2_train_step_vs_oracle, plus the running
    statistics) on ``compare``'s figures.  ``wide``: {"grad": limit} replacing STEP_GRAD_TOL[C] for
    this case."""
    wide = wide or {}
    assert hard == 0, f"{cid}: {hard} spikes differ away from the threshold"
    assert np.isfinite(r["loss"][0]) and np.isfinite(r["flow_maxabs"]), cid
    assert abs(r["loss"][0] - r["loss"][1]) <= STEP_LOSS_RTOL * abs(r["loss"][1]), (cid, r["loss"])
    assert max(r["flow_rel"]) <= STEP_FLOW_TOL and r["flow_maxabs"] <= STEP_FLOW_TOL, (cid, r["flow_rel"], r["flow_maxabs"])
    if "aee" in r:
        assert np.abs(r["aee"][0] - r["aee"][1]).max() <= 1e-4, (cid, r["aee"])
    assert r["stats_excess"] <= CELL_ATOL and r["nbt_equal"], (cid, r["stats_excess"], r["nbt_equal"])
    for n, v in r["grad_rel"].items():
        assert np.isfinite(v) and v <= wide.get("grad", STEP_GRAD_TOL[C]), (cid, n, v)


def oracle_eval(init, C, cpu_wins, ours_states, eps, name="LIFFireNet", dtype=None, states0=None):
    """The oracle in eval mode under no_grad over the windows, following our spikes (``oracle_step``).
    Returns (flows, final states, flips, hard)."""
    ref = _new_ref(init, C, name, dtype, train=False)
    if states0 is not None:
        ref._states = [s.to(dtype or s.dtype) for s in states0]
    flows, flips, hard = [], 0, 0
    with torch.no_grad():
        for t, w in enumerate(cpu_wins):
            f, fl, hd = oracle_step(ref, _cast(w, dtype)["event_cnt"], ours_states[t], eps)
            flows.append(f)
            flips += sum(fl)
            hard += hd
    return flows, list(ref._states), flips, hard


def eval_compare(tag, flows, final, rflows, rfinal, flips, hard):
    """Figures of an eval-mode run against ``oracle_eval``'s: worst |dflow|, final spikes differing,
    worst membrane excess over rtol 1e-5 (the oracle's adopted spikes carry our membrane)."""
    r = {"flips": flips, "hard": hard,
         "flow_maxabs": max(float((f.detach().cpu().double() - q.double()).abs().max()) for f, q in zip(flows, rflows)),
         "spk_diff": sum(int((a[1].detach().cpu().double() != b[1].double()).sum()) for a, b in zip(final, rfinal)),
         "mem_excess": max(float(((a[0].detach().cpu().double() - b[0].double()).abs() - 1e-5 * b[0].double().abs()).max())
                           for a, b in zip(final, rfinal)),
         "finite": all(bool(torch.isfinite(f).all()) for f in flows)}
    print(f"\n[{tag}] spike flips {flips} (away from the threshold: {hard}); max|dflow| {r['flow_maxabs']:.2e}; "
          f"final spikes differing {r['spk_diff']}; final membrane excess over rtol 1e-5 {r['mem_excess']:.2e}")
    return r


def assert_eval(cid, r, wide=None):
    """test_cfg2_eval_vs_oracle's flow limit; final states as one cell step's (spikes equal, membranes
    rtol 1e-5 / atol CELL_ATOL or ``wide["mem"]``)."""
    assert r["finite"], cid
    assert r["hard"] == 0, f"{cid}: {r['hard']} spikes differ away from the threshold"
    assert r["flow_maxabs"] <= 1e-4, (cid, r["flow_maxabs"])
    assert r["spk_diff"] == 0, cid
    assert r["mem_excess"] <= (wide or {}).get("mem", CELL_ATOL), (cid, r["mem_excess"])


def trained_looking_stats(model_or_sd_owner, seed=3):
    """Running statistics away from (0, 1), so that the eval-mode BatchNorm is not the identity."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model_or_sd_owner.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.running_mean.copy_(0.2 * torch.randn(m.running_mean.shape, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))


def given_states(B, C, H, W, L, seed=4):
    """Caller-given initial states: random membranes, binary spikes."""
    g = torch.Generator().manual_seed(seed)
    return [torch.stack([torch.randn(B, C, H, W, generator=g) * 0.5, (torch.rand(B, C, H, W, generator=g) < 0.2).float()])
            for _ in range(L)]
