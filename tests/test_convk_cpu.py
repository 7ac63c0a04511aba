"""CPU side of the K x K cells (model.kernel_size 1, 5, 7; no GPU): the C ABI's new entry points and
the constructors, and the oracle alone held to the rules test_gpu_convk.py rests on -- the near-threshold
cap of every data seed, and the fp32 CPU oracle in the role of "ours" against the fp64 oracle through the
same compare / assert functions (tests/convk_harness.py, tests/firenet_harness.py), which prints the
reference-against-reference figures a widened GPU limit may be derived from."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convk_harness as ch  # noqa: E402
import firenet_harness as fh  # noqa: E402

NEW_SYMBOLS = ("snnflow_convk_supported", "snnflow_prep_weights_k", "snnflow_convk_fwd", "snnflow_layerk_bwd",
               "snnflow_wgradk")


# ---------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------
def test_abi_symbols_and_version():
    from snnflow import _lib

    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTS, name
        assert getattr(_lib.lib, name).argtypes is not None
    assert _lib.lib.snnflow_abi_version() == 41


def test_convk_supported():
    from snnflow import _lib

    sup = _lib.lib.snnflow_convk_supported
    for K, B, H, W, C, cin, rec, train in ch.CELL_CASES:
        assert sup(K, C, cin, int(rec)) == 1, (K, C, cin, rec)
    for k in (2, 3, 4, 9):
        for C, cin in ((8, 8), (8, 2), (32, 32)):
            for rec in (0, 1):
                assert sup(k, C, cin, rec) == 0, (k, C, cin, rec)
    # the widths the 3x3 cells take: C in {4, 8, 16, 32}, cin in {1, 2, 4, 5, C}
    for k in (1, 5, 7):
        for C in (4, 8, 16, 32):
            for cin in (1, 2, 4, 5, C):
                assert sup(k, C, cin, 0) == 1 and sup(k, C, cin, 1) == 1, (k, C, cin)
        assert sup(k, 8, 3, 0) == 0 and sup(k, 12, 12, 0) == 0 and sup(k, 16, 8, 1) == 0


# ---------------------------------------------------------------------------
# constructors
# ---------------------------------------------------------------------------
def test_cell_constructors():
    import snnflow

    ff = snnflow.SNNtorch_ConvLIF(2, 8, 5)
    assert tuple(ff.ff.weight.shape) == (8, 2, 5, 5) and ff.kernel_size == 5
    rc = snnflow.SNNtorch_ConvLIFRecurrent(8, 8, 7)
    assert tuple(rc.ff.weight.shape) == (8, 8, 7, 7) and tuple(rc.rec.weight.shape) == (8, 8, 7, 7)
    assert rc.ff.padding == (3, 3) and rc.kernel_size == 7
    assert snnflow.SNNtorch_ConvLIF(8, 8, 1).ff.padding == (0, 0)
    for cls in (snnflow.SNNtorch_ConvLIF, snnflow.SNNtorch_ConvLIFRecurrent):
        for k in (4, 9):
            with pytest.raises(NotImplementedError, match="1, 3, 5, 7"):
                cls(8, 8, k)


@pytest.mark.parametrize("name", ["LIFFireNet", "LIFFireNet_short", "LIFFireFlowNet", "LIFFireFlowNet_short"])
def test_model_kernel_size_5(name):
    import snnflow
    from oracle import lif_ref

    kw = lif_ref.make_unet_kwargs(base_num_channels=8)
    kw["kernel_size"] = 5
    torch.manual_seed(0)
    model = getattr(snnflow, name)(kw)
    assert tuple(model.head.ff.weight.shape) == (8, 2, 5, 5)
    assert tuple(model.G1.ff.weight.shape) == (8, 8, 5, 5)
    assert model._cellwise()
    assert not model.engine.sequence_ok(2)
    ref = lif_ref.LIFFireNetRef(kw, name)
    model.load_state_dict(ref.state_dict(), strict=True)
    for (n, a), (m, b) in zip(model.state_dict().items(), ref.state_dict().items()):
        assert n == m and torch.equal(a, b), (n, m)
    kw["kernel_size"] = 4
    with pytest.raises(NotImplementedError):
        getattr(snnflow, name)(kw)
    kw["kernel_size"] = 3
    assert not getattr(snnflow, name)(kw)._cellwise()


# ---------------------------------------------------------------------------
# the oracle alone: seeds and reference-against-reference figures
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cell64():
    """The fp64 oracle's result of every cell case (and the float-input case), computed once."""
    cache = {}

    def get(case, float_input=False):
        cid = ch.FLOAT_ID if float_input else ch.cell_id(case)
        if cid not in cache:
            data = ch.cell_data(case, ch.FLOAT_SEED, True) if float_input else ch.cell_data(case)
            cache[cid] = (data, ch.cell_oracle(case, *data, torch.float64))
        return cache[cid]

    return get


@pytest.mark.parametrize("case", ch.CELL_CASES, ids=ch.cell_id)
def test_cell_near_threshold_cap(cell64, case):
    """A condition on the committed seeds, not a measurement (test_ragged_cpu.py's rule): neurons of the
    fp64 oracle within 1e-4 of the threshold <= 0.01 % of the case's neurons, 0 below 10^4 neurons."""
    _, want = cell64(case)
    assert want["near"] <= ch.cell_cap(case), (ch.cell_id(case), want["near"], ch.cell_cap(case))


def test_float_input_near_threshold_cap(cell64):
    _, want = cell64(ch.FLOAT_CASE, True)
    assert want["near"] <= ch.cell_cap(ch.FLOAT_CASE), (ch.FLOAT_ID, want["near"])


def _wide(figure, base):
    """The fp32 oracle's own limit where its committed figure exceeds the project's: 4 x the figure
    (thread counts change the CPU convolutions' summation order)."""
    return 4 * figure if figure is not None and figure > base else base


def _cell32(cid, case, data):
    ours = ch.cell_oracle(case, *data, torch.float32)
    state = torch.stack([ours["mem"], ours["spk"]])
    want = ch.cell_oracle(case, *data, torch.float64, ours=(ours["spk"], state))
    r = fh.cell_compare(f"cpu32 {cid}", ours, want)
    print(f"[cpu32 {cid}] membrane excess {r['mem_excess']:.2e} worst gradient rel-L2 {max(r['grad_rel'].values()):.2e}")
    fh.assert_cell(cid, r, want, ch.cell_cap(case), {"mem": _wide(ch.REF_CELL_MEM.get(cid), fh.CELL_ATOL)})


@pytest.mark.parametrize("case", ch.CELL_CASES, ids=ch.cell_id)
def test_cell_fp32_oracle_vs_fp64(cell64, case):
    data, _ = cell64(case)
    _cell32(ch.cell_id(case), case, data)


def test_float_input_fp32_oracle_vs_fp64(cell64):
    data, _ = cell64(ch.FLOAT_CASE, True)
    _cell32(ch.FLOAT_ID, ch.FLOAT_CASE, data)


@pytest.mark.parametrize("K", [5, 1])
def test_train_step_fp32_oracle_vs_fp64(monkeypatch, K):
    """The fp32 oracle, free-running, against the fp64 oracle following it: LIFFireNet C = 8 with K x K
    cells at (3, 9, 33), T = 3 windows of 300 events.  Prints the figure convk_harness.REF_STEP_GRAD holds."""
    ch.patch_kernel_size(monkeypatch, K)
    B, H, W = ch.STEP_SHAPE
    cid, C = ch.step_id(K), 8
    wins = fh.cpu_windows(B, H, W, fh.STEP_T, fh.STEP_N, seed=1)
    model, init, flows, loss, states = fh.oracle_as_ours(wins, C)
    assert tuple(init["head.ff.weight"].shape) == (C, 2, K, K)
    fh.assert_states_sane(cid, states)
    ref, rflows, rloss, flips, hard = fh.oracle_run(init, C, wins, states, fh.EPS, "LIFFireNet", torch.float64)
    r = fh.compare(f"cpu32 {cid} flip-corrected", model, flows, loss, ref, rflows, rloss, flips, wins, C=C, aee=False)
    print(f"[cpu32 {cid}] worst gradient rel-L2 {max(r['grad_rel'].values()):.3e}")
    fh.assert_step(cid, r, hard, C, {"grad": _wide(ch.REF_STEP_GRAD[K], fh.STEP_GRAD_TOL[C])})


def test_eval_fp32_oracle_vs_fp64(monkeypatch):
    """Eval mode, K = 5, running statistics away from (0, 1), given states: fp32 oracle free-running
    against the fp64 oracle following it (the CPU side of test_liffirenet_convk_eval)."""
    from oracle import lif_ref

    ch.patch_kernel_size(monkeypatch, 5)
    B, H, W = ch.STEP_SHAPE
    C, cid = 8, "eval-K5-C8-3x9x33-given"
    wins = fh.cpu_windows(B, H, W, fh.STEP_T, fh.STEP_N, seed=7)
    torch.manual_seed(0)
    ours = lif_ref.LIFFireNetRef(lif_ref.make_unet_kwargs(base_num_channels=C), "LIFFireNet").eval()
    fh.trained_looking_stats(ours)
    init = {k: v.detach().clone() for k, v in ours.state_dict().items()}
    st0 = fh.given_states(B, C, H, W, 7)
    ours._states = [s.clone() for s in st0]
    flows, states = [], []
    with torch.no_grad():
        for w in wins:
            flows.append(ours(w["event_voxel"], w["event_cnt"])["flow"][0])
            states.append([s.clone() for s in ours._states])
    rflows, rfinal, flips, hard = fh.oracle_eval(init, C, wins, states, fh.EPS, dtype=torch.float64, states0=st0)
    r = fh.eval_compare(cid, flows, states[-1], rflows, rfinal, flips, hard)
    fh.assert_eval(cid, r)
