"""CPU-side validation of the ragged-shape harness (tests/firenet_harness.py; no GPU): the fp32 CPU
oracle in the role of "ours" against the fp64 oracle, through the compare and assert functions
test_gpu_ragged.py uses, for every shape, width and model of that file.  This proves that the harness
can pass and prints the reference-against-reference error the tolerances rest on; and it holds the
condition on the cell cases' data seeds: the fp64 oracle alone keeps at most cell_cap(case) neurons
within 1e-4 of the threshold, which caps what the GPU test may adopt."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import firenet_harness as fh  # noqa: E402


@pytest.fixture(scope="module")
def cell64():
    """The fp64 oracle's result of every cell case, computed once."""
    cache = {}

    def get(case):
        cid = fh.cell_id(case)
        if cid not in cache:
            data = fh.cell_data(case)
            cache[cid] = (data, fh.cell_oracle(case, *data, torch.float64))
        return cache[cid]

    return get


@pytest.mark.parametrize("case", fh.CELL_CASES, ids=fh.cell_id)
def test_cell_near_threshold_cap(cell64, case):
    """A condition on the committed seeds, not a measurement: neurons of the fp64 oracle within 1e-4
    of the threshold <= 0.01 % of the case's neurons (0 of 35 C at 5x7)."""
    _, want = cell64(case)
    assert want["near"] <= fh.cell_cap(case), (fh.cell_id(case), want["near"], fh.cell_cap(case))


def _wide(figure, base):
    """The fp32 oracle's own limit where its committed figure (firenet_harness.REF_*) exceeds the project's:
    4 x the figure (thread counts change the CPU convolutions' summation order)."""
    return 4 * figure if figure is not None and figure > base else base


@pytest.mark.parametrize("case", fh.CELL_CASES, ids=fh.cell_id)
def test_cell_fp32_oracle_vs_fp64(cell64, case):
    data, _ = cell64(case)
    ours = fh.cell_oracle(case, *data, torch.float32)
    state = torch.stack([ours["mem"], ours["spk"]])
    want = fh.cell_oracle(case, *data, torch.float64, ours=(ours["spk"], state))
    cid = fh.cell_id(case)
    r = fh.cell_compare(f"cpu32 {cid}", ours, want)
    fh.assert_cell(cid, r, want, fh.cell_cap(case), {"mem": _wide(fh.REF_CELL_MEM.get(cid), fh.CELL_ATOL)})


def _step(cid, name, C, B, H, W, T):
    wins = fh.cpu_windows(B, H, W, T, fh.STEP_N, seed=1)
    model, init, flows, loss, states = fh.oracle_as_ours(wins, C, name)
    fh.assert_states_sane(cid, states)
    ref, rflows, rloss, flips, hard = fh.oracle_run(init, C, wins, states, fh.EPS, name, torch.float64)
    r = fh.compare(f"cpu32 {cid} flip-corrected", model, flows, loss, ref, rflows, rloss, flips, wins, C=C, aee=False)
    fh.assert_step(cid, r, hard, C, {"grad": _wide(fh.REF_STEP_GRAD.get(cid), fh.STEP_GRAD_TOL[C])})


@pytest.mark.parametrize("case", fh.STEP_CASES, ids=fh.step_id)
def test_train_step_fp32_oracle_vs_fp64(case):
    name, C, (B, H, W) = case
    _step(fh.step_id(case), name, C, B, H, W, fh.STEP_T)


def test_step_count_boundary_fp32_oracle_vs_fp64():
    """T = 33 (one more than the deferred weight-gradient drivers take per call) at B = 1, 9x33, C = 8."""
    _step(fh.T33_ID, "LIFFireNet", 8, 1, 9, 33, 33)


@pytest.mark.parametrize("given", [False, True], ids=["zero-states", "given-states"])
@pytest.mark.parametrize("B,H,W", [(3, 9, 33), (2, 12, 58)])
def test_eval_fp32_oracle_vs_fp64(B, H, W, given):
    """Eval mode, running statistics away from (0, 1), C = 8: fp32 oracle free-running against the fp64
    oracle following it."""
    from oracle import lif_ref

    C, cid = 8, f"eval-C8-{B}x{H}x{W}-{'given' if given else 'zero'}"
    wins = fh.cpu_windows(B, H, W, fh.STEP_T, fh.STEP_N, seed=7)
    torch.manual_seed(0)
    ours = lif_ref.LIFFireNetRef(lif_ref.make_unet_kwargs(base_num_channels=C), "LIFFireNet").eval()
    fh.trained_looking_stats(ours)
    init = {k: v.detach().clone() for k, v in ours.state_dict().items()}
    st0 = fh.given_states(B, C, H, W, 7) if given else None
    if given:
        ours._states = [s.clone() for s in st0]
    flows, states = [], []
    with torch.no_grad():
        for w in wins:
            flows.append(ours(w["event_voxel"], w["event_cnt"])["flow"][0])
            states.append([s.clone() for s in ours._states])
    rflows, rfinal, flips, hard = fh.oracle_eval(init, C, wins, states, fh.EPS, dtype=torch.float64, states0=st0)
    r = fh.eval_compare(cid, flows, states[-1], rflows, rfinal, flips, hard)
    fh.assert_eval(cid, r)
