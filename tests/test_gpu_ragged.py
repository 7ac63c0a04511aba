"""The LIFFireNet kernels (csrc/lif_layers.hip, csrc/wgrad.hip, csrc/snnflow_tile.h: Conv3x3 + BatchNorm
+ LIF on 8 x 32-pixel tiles with a one-pixel halo) at image sizes that are no tile multiples, against
the CPU oracle in fp64 (tests/firenet_harness.py).  Every test has the oracle on the other side; none
compares two GPU paths.

a. one cell, one step, teacher-forced (test_cell_ragged): C in {4, 8, 16, 32}, feed-forward and
   recurrent, train and eval mode -- spikes, membrane, running statistics, every gradient.
b. the whole train step (test_train_step_ragged): T = 3 windows of 300 events, both paths, C in
   {8, 16, 32}, LIFFireNet / LIFFireNet_short / LIFFireFlowNet.
c. the launch variants of forward_sequence (test_launch_variants_c8 / _c16_c32), each asserted to have
   run: the entry points the engine called and the planners it asked are recorded.
d. the fused evaluation launches (test_eval_fused_ragged).
e. T = 33, one more step than one deferred weight-gradient call takes (test_step_count_boundary).
f. in every case: outputs finite, spikes exactly 0 or 1, BatchNorm running statistics equal to the
   oracle's (their pixel count is B H W, not the tile-padded count).

Spikes: the oracle adopts ours where it differs and its fp64 membrane lies within 1e-4 of the threshold
(counted; for the cells capped by firenet_harness.cell_cap, which test_ragged_cpu.py holds the oracle
alone to); any other differing spike fails.  Gradients are then always compared.

The train-step legs: (1) free-running fp64 oracle, reported; (2) flip-corrected fp64 oracle, asserted at
test_cfg2_train_step_vs_oracle's limits -- the gradient limit of a case is 4 x the error of the fp32 CPU
oracle against the fp64 oracle at that case (firenet_harness.REF_STEP_GRAD; WIDENED_STEP below) where the
case exceeded its limit and stayed within that; (3) flip-corrected fp32 oracle, the arithmetic the HIP
loss reproduces, asserted at the unwidened limits."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import firenet_harness as fh  # noqa: E402

pytestmark = pytest.mark.gpu

# Cases whose limit against the fp64 oracle is 4 x the reference-against-reference figure
# (firenet_harness.REF_CELL_MEM / REF_STEP_GRAD): the case exceeded the project's limit on the GPU and
# stayed within 4 x the figure.  Measured GPU value next to each.
# cell id: membrane excess over rtol 1e-5 (limit 1e-6) measured on MI355X; reference figures 1.20e-6,
# 1.16e-6, 7.14e-7 -> limits 4.8e-6, 4.6e-6, 2.9e-6.  C = 32 only: 288-term convolution sums in fp32.
WIDENED_CELL_MEM = {"2x12x58-C32-cin32-ff-train": 1.89e-6, "3x17x65-C32-cin32-ff-train": 1.96e-6,
                    "3x17x65-C32-cin32-rec-train": 1.57e-6}
# step id: worst gradient relative L2 against the fp64 oracle measured on MI355X (over both paths and all
# launch variants); every one equals the reference figure to 2-3 digits -- the HIP loss reproduces the
# fp32 reference arithmetic, whose dL/dflow is what is off from fp64 (firenet_harness.REF_STEP_GRAD).
# The same runs against the fp32 oracle: at most 3.4e-6 (limits 6e-6 / 1e-5 / 5e-5, unwidened).
WIDENED_STEP = {"LIFFireNet-C8-3x9x33": 2.060e-5, "LIFFireNet-C8-2x12x58": 1.394e-3, "LIFFireNet-C8-3x17x65": 2.273e-3,
                "LIFFireNet-C16-2x12x58": 4.630e-5, "LIFFireNet-C16-3x17x65": 1.527e-4,
                "LIFFireNet-C32-2x12x58": 1.493e-4, "LIFFireNet-C32-3x17x65": 4.506e-4,
                "LIFFireNet_short-C8-3x9x33": 6.143e-5, "LIFFireFlowNet-C8-3x9x33": 8.943e-5}

PER_STEP_ENTRIES = {"snnflow_firenet_fwd", "snnflow_conv_fwd", "snnflow_lif_fwd", "snnflow_firenet_bwd",
                    "snnflow_firenet_bwd_seq", "snnflow_layer_bwd", "snnflow_lif_bwd"}


class _Spy:
    """What the engine launched: C-ABI entry points and call names in order (snnflow._lib.call), and how
    often it asked each launch planner."""

    def __init__(self, monkeypatch):
        from snnflow import _lib, engine

        self.entries, self.names, self.planners = [], [], {}
        real = _lib.call

        def call(name, fn, *args, **kw):
            self.entries.append(getattr(fn, "__name__", "?"))
            self.names.append(name)
            return real(name, fn, *args, **kw)

        monkeypatch.setattr(_lib, "call", call)
        for p in ("chained_fwd_slots", "chained_bwd_slots", "wavefront_slots"):
            self.planners[p] = 0
            monkeypatch.setattr(engine, p, self._count(p, getattr(engine, p)))

    def _count(self, p, real):
        def wrapped(*args, **kw):
            self.planners[p] += 1
            return real(*args, **kw)
        return wrapped

    def count(self, entry):
        return self.entries.count(entry)


def _to(dev, wins):
    return [{k: v.to(dev) for k, v in w.items()} for w in wins]


# ---------------------------------------------------------------------------
# a. one cell, one step
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", fh.CELL_CASES, ids=fh.cell_id)
def test_cell_ragged(dev, case):
    import snnflow

    B, H, W, C, cin, rec, train = case
    cid = fh.cell_id(case)
    sd, x, prev, wgt = fh.cell_data(case)
    cls = snnflow.SNNtorch_ConvLIFRecurrent if rec else snnflow.SNNtorch_ConvLIF
    cell = cls(cin, C, 3).to(dev)
    cell.load_state_dict({k: v.to(dev) for k, v in sd.items()})
    cell.train(train)
    xd = x.to(dev).requires_grad_(True)
    pd = prev.to(dev).requires_grad_(True)
    spk, st = cell(xd, pd)
    (spk * wgt.to(dev)).sum().backward()
    want = fh.cell_oracle(case, sd, x, prev, wgt, torch.float64, ours=(spk, st))
    names = [n for n, _ in cell.named_parameters()]
    assert set(names) == set(want["grads"]) - {"input", "prev_state"}
    grads = {n: p.grad for n, p in cell.named_parameters()}
    grads["input"] = xd.grad
    if rec:
        grads["prev_state"] = pd.grad
    assert all(g is not None for g in grads.values()), {n for n, g in grads.items() if g is None}
    ours = {"spk": spk.detach(), "mem": st[0].detach(), "run_mean": cell.bn.running_mean, "run_var": cell.bn.running_var,
            "nbt": int(cell.bn.num_batches_tracked), "grads": grads}
    r = fh.cell_compare(f"hip {cid}", ours, want)
    wide = {"mem": 4 * fh.REF_CELL_MEM[cid]} if cid in WIDENED_CELL_MEM else None
    fh.assert_cell(cid, r, want, fh.cell_cap(case), wide)


# ---------------------------------------------------------------------------
# b, c, e. the whole train step
# ---------------------------------------------------------------------------
def _train_step(dev, cid, tag, name, C, B, H, W, T, path, model=None):
    """gpu_run on CPU-drawn windows, then the three oracle legs of the module docstring."""
    cpu_wins = fh.cpu_windows(B, H, W, T, fh.STEP_N, seed=1)
    model, init, flows, loss, states = fh.gpu_run(dev, path, _to(dev, cpu_wins), C, name, model)
    fh.assert_states_sane(cid, states)
    assert all(bool(torch.isfinite(f).all()) for f in flows), cid
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters()), cid
    f64 = torch.float64
    ref, rflows, rloss, flips, _ = fh.oracle_run(init, C, cpu_wins, states, None, name, f64)
    fh.compare(f"{tag} free-running fp64", model, flows, loss, ref, rflows, rloss, flips, cpu_wins)
    ref, rflows, rloss, flips, hard = fh.oracle_run(init, C, cpu_wins, states, fh.EPS, name, f64)
    r = fh.compare(f"{tag} flip-corrected fp64", model, flows, loss, ref, rflows, rloss, flips, cpu_wins)
    print(f"[{tag}] adopted near-threshold spikes: {int(flips.sum())}")
    ref, rflows, rloss, flips, hard32 = fh.oracle_run(init, C, cpu_wins, states, fh.EPS, name)
    r32 = fh.compare(f"{tag} flip-corrected fp32", model, flows, loss, ref, rflows, rloss, flips, cpu_wins)
    fh.assert_step(cid, r, hard, C, {"grad": 4 * fh.REF_STEP_GRAD[cid]} if cid in WIDENED_STEP else None)
    fh.assert_step(cid, r32, hard32, C)
    return model, flows


@pytest.mark.parametrize("path", ["sequence", "per_step"])
@pytest.mark.parametrize("case", fh.STEP_CASES, ids=fh.step_id)
def test_train_step_ragged(dev, monkeypatch, case, path):
    name, C, (B, H, W) = case
    spy = _Spy(monkeypatch)
    model, _ = _train_step(dev, fh.step_id(case), f"{fh.step_id(case)} {path}", name, C, B, H, W, fh.STEP_T, path)
    assert model.engine.sequence_ok(2)
    if path == "sequence":  # the wavefront launches, not a fallback to the per-step kernels
        assert not PER_STEP_ENTRIES & set(spy.entries), spy.entries
    else:
        assert spy.count("snnflow_firenet_fwd") == fh.STEP_T, spy.entries


@pytest.mark.parametrize("path", ["sequence", "per_step"])
def test_step_count_boundary(dev, monkeypatch, path):
    """T = 33 at B = 1, 9x33, C = 8: the head's deferred weight gradients take two calls (32 steps, then
    one accumulated on top); the other layers' are fused into the backward at C = 8."""
    from snnflow import _lib

    T = _lib.MAX_WGRAD_STEPS + 1
    spy = _Spy(monkeypatch)
    _train_step(dev, fh.T33_ID, f"{fh.T33_ID} {path}", "LIFFireNet", 8, 1, 9, 33, T, path)
    assert spy.names.count("wgrad[0]") == 2, spy.names
    if path == "sequence":
        assert not PER_STEP_ENTRIES & set(spy.entries), spy.entries


@pytest.mark.parametrize("pipe", [0, 1, 2, 5])
@pytest.mark.parametrize("chain", [False, True], ids=["wavefront", "chained"])
@pytest.mark.parametrize("B,H,W", [(3, 9, 33), (3, 17, 65)])
def test_launch_variants_c8(dev, monkeypatch, B, H, W, chain, pipe):
    """C = 8, sequence path: fwd_chain / bwd_chain on and off; 0, 1, 2 and 5 tiles per block of the forward
    tile pipeline (3 x 9 x 33: 12 tiles, so 5 leaves a short last block)."""
    from snnflow import _lib

    T, L = fh.STEP_T, 7
    cid = f"LIFFireNet-C8-{B}x{H}x{W}"
    model = fh.new_model(8).to(dev).train()
    model.engine.fwd_chain = model.engine.bwd_chain = chain
    spy = _Spy(monkeypatch)
    old = _lib.lib.snnflow_get_pipe(0)
    assert _lib.lib.snnflow_set_pipe(pipe, 0) == 0
    try:
        _train_step(dev, cid, f"{cid} chain={chain} pipe={pipe}", "LIFFireNet", 8, B, H, W, T, "sequence", model)
        assert _lib.lib.snnflow_get_pipe(0) == pipe
    finally:
        _lib.lib.snnflow_set_pipe(old, 0)
    assert model.engine.sequence_ok(2)
    assert not PER_STEP_ENTRIES & set(spy.entries), spy.entries
    fwd_chained = chain and pipe > 0  # the chained forward hands spikes over inside the tile pipeline
    wave = 2 * (T - 1) + L + 1
    assert spy.count("snnflow_fwd_chain") == (T + L if fwd_chained else 0), spy.entries
    assert spy.count("snnflow_fwd_slot") == (0 if fwd_chained else wave), spy.entries
    assert spy.count("snnflow_bwd_chain") == (T + L if chain else 0), spy.entries
    assert spy.count("snnflow_bwd_slot") == (0 if chain else wave), spy.entries
    assert spy.planners == {"chained_fwd_slots": int(fwd_chained), "chained_bwd_slots": int(chain),
                            "wavefront_slots": int(not fwd_chained) + int(not chain)}, spy.planners


@pytest.mark.parametrize("fuse_head", [False, True], ids=["head-deferred", "head-fused"])
@pytest.mark.parametrize("bits", [False, True], ids=["fp32-spikes", "bit-planes"])
@pytest.mark.parametrize("B,H,W", [(3, 9, 33), (2, 12, 58)])
@pytest.mark.parametrize("C", [16, 32])
def test_launch_variants_c16_c32(dev, monkeypatch, C, B, H, W, bits, fuse_head):
    """C = 16 / 32, sequence path: the spike bit planes on and off (at W = 33 the uint16 rows of the C = 16
    planes are not 4-byte aligned) and the head's weight gradient fused into its backward task or deferred."""
    T, L = fh.STEP_T, 7
    cid = f"LIFFireNet-C{C}-{B}x{H}x{W}"
    model = fh.new_model(C).to(dev).train()
    model.engine.spk_bits, model.engine.fuse_head = bits, fuse_head
    spy = _Spy(monkeypatch)
    _, flows = _train_step(dev, cid, f"{cid} bits={bits} fuse_head={fuse_head}", "LIFFireNet", C, B, H, W, T,
                           "sequence", model)
    assert model.engine.sequence_ok(2)
    assert not PER_STEP_ENTRIES & set(spy.entries), spy.entries
    wave = 2 * (T - 1) + L + 1
    assert spy.count("snnflow_fwd_slot") == wave and spy.count("snnflow_bwd_slot") == wave, spy.entries
    node = flows[0].grad_fn  # the FireNetSequence node: the bit planes its forward wrote, if any
    assert (node.bits is not None) == bits
    assert any(p is not None for row in node.bptr for p in row) == bits
    # every layer's weight gradient is deferred at these widths, the head's unless fused into its backward
    assert [n for n in spy.names if n.startswith("wgrad[")] == [f"wgrad[{l}]" for l in range(int(fuse_head), L)], spy.names


# ---------------------------------------------------------------------------
# d. fused evaluation
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("given", [False, True], ids=["zero-states", "given-states"])
@pytest.mark.parametrize("B,H,W", [(3, 9, 33), (2, 12, 58)])
def test_eval_fused_ragged(dev, monkeypatch, B, H, W, given):
    """model.eval() under no_grad through forward_sequence at C = 8 (snnflow_eval_slot: conv + BatchNorm +
    LIF per task) with running statistics away from (0, 1), from zero and from caller-given states:
    flows and final states against the fp64 oracle in eval mode."""
    from snnflow.engine import eval_fused_ok

    C, T, L = 8, fh.STEP_T, 7
    cid = f"eval-C8-{B}x{H}x{W}-{'given' if given else 'zero'}"
    cpu_wins = fh.cpu_windows(B, H, W, T, fh.STEP_N, seed=7)
    wins = _to(dev, cpu_wins)
    model = fh.new_model(C)
    fh.trained_looking_stats(model)
    init = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    model = model.to(dev).eval()
    st0 = fh.given_states(B, C, H, W, L) if given else None
    if given:
        model.states = [s.to(dev) for s in st0]
    spy = _Spy(monkeypatch)
    model.engine.capture_states = True
    try:
        with torch.no_grad():
            assert eval_fused_ok(model.engine, [w["event_cnt"] for w in wins], model._states)
            outs = model.forward_sequence([w["event_voxel"] for w in wins], [w["event_cnt"] for w in wins])
    finally:
        model.engine.capture_states = False
    flows = [o["flow"][0] for o in outs]
    states = [[s.detach().cpu() for s in sts] for sts in model.engine.seq_states]
    model.engine.seq_states = None
    # T + L - 1 wavefront launches of the fused evaluation kernels and nothing of the train path
    launched = [e for e in spy.entries if e != "snnflow_prep_weights_batch"]
    assert launched == ["snnflow_eval_slot"] * (T + L - 1), spy.entries
    fh.assert_states_sane(cid, states)
    rflows, rfinal, flips, hard = fh.oracle_eval(init, C, cpu_wins, states, fh.EPS, dtype=torch.float64, states0=st0)
    r = fh.eval_compare(cid, flows, model._states, rflows, rfinal, flips, hard)
    fh.assert_eval(cid, r)
