"""The K x K cells (model.kernel_size 1, 5, 7; csrc/convk.hip: snnflow_convk_fwd, snnflow_layerk_bwd,
snnflow_wgradk on 8 x 32-pixel tiles with a K / 2-pixel halo) against the CPU oracle in fp64
(tests/convk_harness.py, tests/firenet_harness.py).

a. one cell, one step, teacher-forced (test_cell_convk): spikes, membrane, running statistics, every
   gradient, at shapes below the K = 7 footprint, one pixel past the tile and with two partial tile rows.
b. the same with an input that is not spikes (test_cell_convk_float_input).
c. weight gradients bit-identical run to run (test_convk_weight_grads_bit_reproducible).
d. the whole train step of LIFFireNet C = 8 with K = 5 and K = 1 (test_liffirenet_convk_train_step): the
   three oracle legs of test_gpu_ragged._train_step, and the entry points that ran.
e. forward_sequence == T forward calls, exactly (its documented fall-back; the one comparison of two GPU runs).
f. eval mode under no_grad against the oracle in eval mode (test_liffirenet_convk_eval).
g. the entry points refuse what belongs to the 3x3 calls (test_convk_refuses).

Spikes: the oracle adopts ours where it differs and its fp64 membrane lies within 1e-4 of the threshold,
at most cell_cap(case) of them (test_convk_cpu.py holds the oracle alone to that); any other differing
spike fails."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convk_harness as ch  # noqa: E402
import firenet_harness as fh  # noqa: E402

pytestmark = pytest.mark.gpu

# Cases whose membrane limit against the fp64 oracle is 4 x the reference-against-reference figure
# (convk_harness.REF_CELL_MEM; the rule of test_gpu_ragged.py): the case exceeded CELL_ATOL 1e-6 over
# rtol 1e-5 on the GPU and stayed within 4 x the figure.  cell id: the excess measured on MI355X
# (reference figure 1.83e-6 -> limit 7.3e-6; 1568-term convolution sums in fp32, twice).  Every other case
# measured 1.4e-8 .. 7.4e-7 and keeps CELL_ATOL.
WIDENED_CELL_MEM = {"K7-3x9x33-C32-cin32-rec-train": 1.01e-6}
# step K: worst gradient relative L2 against the fp64 oracle measured on MI355X, where it exceeded
# STEP_GRAD_TOL[8] = 6e-6 and stayed within 4 x convk_harness.REF_STEP_GRAD[K] (the fp32 reference loss
# arithmetic, which the HIP loss reproduces, is that far from fp64; the fp32 leg is held unwidened and
# measured 1.98e-6 / 1.40e-6).  Reference figures 7.058e-5 / 3.298e-5 -> limits 2.8e-4 / 1.3e-4.
WIDENED_STEP = {5: 6.931e-5, 1: 3.279e-5}

CONVK_ENTRIES = ("snnflow_convk_fwd", "snnflow_layerk_bwd", "snnflow_wgradk")
NOT_3X3 = ("snnflow_conv_fwd", "snnflow_fwd_slot", "snnflow_firenet_fwd")


def _to(dev, wins):
    return [{k: v.to(dev) for k, v in w.items()} for w in wins]


def _spy(monkeypatch):
    """The C-ABI entry points the package launched, in order (snnflow._lib.call)."""
    from snnflow import _lib

    entries, real = [], _lib.call

    def call(name, fn, *args, **kw):
        entries.append(getattr(fn, "__name__", "?"))
        return real(name, fn, *args, **kw)

    monkeypatch.setattr(_lib, "call", call)
    return entries


def _run_cell(dev, case, data):
    """One HIP cell step and backward on the case's data; returns (cell, spk, state, gradients)."""
    import snnflow

    K, B, H, W, C, cin, rec, train = case
    sd, x, prev, wgt = data
    cls = snnflow.SNNtorch_ConvLIFRecurrent if rec else snnflow.SNNtorch_ConvLIF
    cell = cls(cin, C, K).to(dev)
    cell.load_state_dict({k: v.to(dev) for k, v in sd.items()})
    cell.train(train)
    xd = x.to(dev).requires_grad_(True)
    pd = prev.to(dev).requires_grad_(True)
    spk, st = cell(xd, pd)
    (spk * wgt.to(dev)).sum().backward()
    grads = {n: p.grad for n, p in cell.named_parameters()}
    grads["input"] = xd.grad
    if rec:
        grads["prev_state"] = pd.grad
    return cell, spk, st, grads


def _check_cell(dev, cid, case, data):
    cell, spk, st, grads = _run_cell(dev, case, data)
    want = ch.cell_oracle(case, *data, torch.float64, ours=(spk, st))
    assert set(n for n, _ in cell.named_parameters()) == set(want["grads"]) - {"input", "prev_state"}
    assert set(grads) == set(want["grads"])
    assert all(g is not None for g in grads.values()), {n for n, g in grads.items() if g is None}
    assert tuple(grads["ff.weight"].shape) == (case[4], case[5], case[0], case[0])
    ours = {"spk": spk.detach(), "mem": st[0].detach(), "run_mean": cell.bn.running_mean, "run_var": cell.bn.running_var,
            "nbt": int(cell.bn.num_batches_tracked), "grads": grads}
    r = fh.cell_compare(f"hip {cid}", ours, want)
    wide = {"mem": 4 * ch.REF_CELL_MEM[cid]} if cid in WIDENED_CELL_MEM else None
    fh.assert_cell(cid, r, want, ch.cell_cap(case), wide)


# ---------------------------------------------------------------------------
# a, b, c. one cell, one step
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ch.CELL_CASES, ids=ch.cell_id)
def test_cell_convk(dev, monkeypatch, case):
    entries = _spy(monkeypatch)
    _check_cell(dev, ch.cell_id(case), case, ch.cell_data(case))
    assert all(entries.count(e) == 1 for e in CONVK_ENTRIES), entries
    assert not set(entries) & {"snnflow_conv_fwd", "snnflow_layer_bwd", "snnflow_wgrad"}, entries


def test_cell_convk_float_input(dev):
    """The input is 0.7 * randn, not spikes: a kernel that assumed bf16-exact inputs would be ~1e-3 off."""
    _check_cell(dev, ch.FLOAT_ID, ch.FLOAT_CASE, ch.cell_data(ch.FLOAT_CASE, ch.FLOAT_SEED, True))


def test_convk_weight_grads_bit_reproducible(dev):
    case = (5, 3, 9, 33, 8, 8, True, True)
    data = ch.cell_data(case)
    runs = [_run_cell(dev, case, data)[3] for _ in range(2)]
    for n in ("ff.weight", "rec.weight"):
        assert torch.equal(runs[0][n], runs[1][n]), n


# ---------------------------------------------------------------------------
# d, e, f. the whole model
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", [5, 1])
def test_liffirenet_convk_train_step(dev, monkeypatch, K):
    ch.patch_kernel_size(monkeypatch, K)
    entries = _spy(monkeypatch)
    B, H, W = ch.STEP_SHAPE
    C, cid, name = 8, ch.step_id(K), "LIFFireNet"
    cpu_wins = fh.cpu_windows(B, H, W, fh.STEP_T, fh.STEP_N, seed=1)
    model, init, flows, loss, states = fh.gpu_run(dev, "per_step", _to(dev, cpu_wins), C, name)
    assert tuple(model.head.ff.weight.shape) == (C, 2, K, K) and tuple(model.G1.rec.weight.shape) == (C, C, K, K)
    ran = list(entries)
    fh.assert_states_sane(cid, states)
    assert all(bool(torch.isfinite(f).all()) for f in flows), cid
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters()), cid
    f64 = torch.float64
    ref, rflows, rloss, flips, _ = fh.oracle_run(init, C, cpu_wins, states, None, name, f64)
    fh.compare(f"{cid} free-running fp64", model, flows, loss, ref, rflows, rloss, flips, cpu_wins)
    ref, rflows, rloss, flips, hard = fh.oracle_run(init, C, cpu_wins, states, fh.EPS, name, f64)
    r = fh.compare(f"{cid} flip-corrected fp64", model, flows, loss, ref, rflows, rloss, flips, cpu_wins)
    print(f"[{cid}] adopted near-threshold spikes: {int(flips.sum())}")
    ref, rflows, rloss, flips, hard32 = fh.oracle_run(init, C, cpu_wins, states, fh.EPS, name)
    r32 = fh.compare(f"{cid} flip-corrected fp32", model, flows, loss, ref, rflows, rloss, flips, cpu_wins)
    fh.assert_step(cid, r, hard, C, {"grad": 4 * ch.REF_STEP_GRAD[K]} if K in WIDENED_STEP else None)
    fh.assert_step(cid, r32, hard32, C)
    L, T = 7, fh.STEP_T
    for e in CONVK_ENTRIES:
        assert ran.count(e) == L * T, (e, ran.count(e))
    assert not set(ran) & set(NOT_3X3), ran


def test_liffirenet_convk_forward_sequence_equals_steps(dev, monkeypatch):
    ch.patch_kernel_size(monkeypatch, 5)
    B, H, W = ch.STEP_SHAPE
    wins = _to(dev, fh.cpu_windows(B, H, W, fh.STEP_T, fh.STEP_N, seed=1))
    a = fh.new_model(8).to(dev).train()
    b = fh.new_model(8).to(dev).train()
    assert all(torch.equal(p, q) for p, q in zip(a.state_dict().values(), b.state_dict().values()))
    outs = a.forward_sequence([w["event_voxel"] for w in wins], [w["event_cnt"] for w in wins])
    steps = [b(w["event_voxel"], w["event_cnt"]) for w in wins]
    assert len(outs) == len(steps) == fh.STEP_T
    for o, s in zip(outs, steps):
        assert torch.equal(o["flow"][0], s["flow"][0])
    for sa, sb in zip(a._states, b._states):
        assert torch.equal(sa, sb)


def test_liffirenet_convk_eval(dev, monkeypatch):
    """K = 5, model.eval() under no_grad, running statistics away from (0, 1), caller-given states."""
    ch.patch_kernel_size(monkeypatch, 5)
    B, H, W = ch.STEP_SHAPE
    C, T, L, cid = 8, fh.STEP_T, 7, "eval-K5-C8-3x9x33-given"
    cpu_wins = fh.cpu_windows(B, H, W, T, fh.STEP_N, seed=7)
    wins = _to(dev, cpu_wins)
    model = fh.new_model(C)
    fh.trained_looking_stats(model)
    init = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    model = model.to(dev).eval()
    st0 = fh.given_states(B, C, H, W, L)
    model.states = [s.to(dev) for s in st0]
    entries = _spy(monkeypatch)
    flows, states = [], []
    with torch.no_grad():
        for w in wins:
            flows.append(model(w["event_voxel"], w["event_cnt"])["flow"][0])
            states.append([s.detach().cpu() for s in model._states])
    assert entries.count("snnflow_convk_fwd") == L * T and "snnflow_eval_slot" not in entries, entries
    fh.assert_states_sane(cid, states)
    rflows, rfinal, flips, hard = fh.oracle_eval(init, C, cpu_wins, states, fh.EPS, dtype=torch.float64, states0=st0)
    r = fh.eval_compare(cid, flows, model._states, rflows, rfinal, flips, hard)
    fh.assert_eval(cid, r)


# ---------------------------------------------------------------------------
# g. refusals
# ---------------------------------------------------------------------------
def test_convk_refuses(dev):
    """Bad calls return their error code before anything is launched; the device stays clean."""
    import snnflow
    from snnflow import _lib

    E_ARG, E_CHANNELS = -1, -2
    B, H, W, C, cin = 1, 9, 33, 8, 8
    s = _lib.stream_ptr(dev)
    x = torch.zeros(B, cin, H, W, device=dev)
    y = torch.full((B, H, W, C), 7.0, device=dev)
    wt = torch.zeros(25 * cin * C, device=dev)

    def args(**kw):
        a = _lib.ConvFwdArgs()
        a.B, a.H, a.W, a.cin, a.c, a.lif_in = B, H, W, cin, C, 0
        a.x = x.data_ptr()
        a.xs_b, a.xs_c, a.xs_h, a.xs_w = x.stride()
        a.wt_ff = a.wt_ff_t = wt.data_ptr()
        a.y = y.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    fwd = _lib.lib.snnflow_convk_fwd
    assert fwd(ctypes.byref(args()), 3, s) == E_ARG          # 3 belongs to snnflow_conv_fwd
    assert fwd(ctypes.byref(args()), 4, s) == E_ARG
    assert fwd(ctypes.byref(args(lif_in=1)), 5, s) == E_ARG
    assert fwd(ctypes.byref(args(wf_ff=wt.data_ptr())), 5, s) == E_ARG
    assert fwd(ctypes.byref(args(state_spk_skip=1)), 5, s) == E_ARG
    assert _lib.lib.snnflow_convk_supported(5, 8, 3, 0) == 0
    assert fwd(ctypes.byref(args(cin=3)), 5, s) == E_CHANNELS
    assert _lib.lib.snnflow_convk_supported(5, 12, 12, 0) == 0
    assert fwd(ctypes.byref(args(c=12, cin=12)), 5, s) == E_CHANNELS
    assert b"convk_fwd" in _lib.lib.snnflow_last_error()
    assert _lib.lib.snnflow_prep_weights_k(wt.data_ptr(), C, cin, 3, wt.data_ptr(), wt.data_ptr(), s) == E_ARG
    wa = _lib.WgradArgs()
    assert _lib.lib.snnflow_wgradk(ctypes.byref(wa), 5, s) == E_ARG
    la = _lib.LayerBwdArgs()
    assert _lib.lib.snnflow_layerk_bwd(ctypes.byref(la), 5, s) == E_ARG
    torch.cuda.synchronize()
    snnflow.check_device_errors()
    assert bool((y == 7.0).all())  # nothing ran
