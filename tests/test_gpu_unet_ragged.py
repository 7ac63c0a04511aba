"""The implicit-GEMM U-Net kernels (csrc/unet.hip) at ragged shapes against the fp64 CPU oracle
(tests/unet_harness.py holds the cases, the oracle runners, the limits and the restated kernel selection;
test_unet_ragged_cpu.py drives the same compare / assert functions with the fp32 oracle as "ours", holds
the near-threshold caps on the committed seeds and proves that the cases reach every instantiation).

Standalone cells outside the fixed one-kernel path: non-square, odd and sub-tile image sizes, inputs
that are not exact in bf16 (the mid and lo planes of the split operand carry data), kernel sizes 1, 5 and
7, stride 2 with odd output widths, a residual, fractional previous spikes, every generic
weight-gradient tile, the three row-strip variants and both sides of their eligibility boundary,
split-K, one- and two-pass split reductions.  Whole models: non-square sizes down to a 1 x 11 and a 7 x 1
deepest level, base widths 12 and 20, a 5-bin real-valued voxel input, given initial states that require
grad, and init_cropping at sizes that are no multiple of 16.

Every case: spikes equal to the fp64 oracle's that follows ours (adopted near-threshold spikes counted
and capped, none away from the threshold), membranes / states, flows (models) and loss (cells and models,
rtol 1e-5) within the limits of test_gpu_unet.py, every gradient's relative L2 against fp64 within
max(2 x the fp32 oracle's, 2e-5); and the split plans snnflow.unet logged equal the ones the restated selection predicts, launch by launch, so the
kernels the coverage table names did run."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unet_harness as uh  # noqa: E402

pytestmark = pytest.mark.gpu


def _check_plans(cid, launches, plans):
    want = [uh.predicted_plan(l) for l in launches]
    assert len(plans) == len(want), (cid, len(plans), len(want))
    for n, (got, exp) in enumerate(zip(plans, want)):
        assert tuple(got) == exp, (cid, n, got, exp)
    print(f"[{cid}] {len(plans)} GEMM launches as predicted: "
          + " ".join(sorted({x for l in launches for x in uh.launch_labels(l)})))


@pytest.mark.parametrize("c", uh.CELL_CASES, ids=uh.cell_id)
def test_cell_vs_fp64_oracle(dev, c):
    cid = uh.cell_id(c)
    data = uh.cell_data(c)
    ours = uh.cell_hip(c, data, dev)
    w64 = uh.cell_oracle(c, data, torch.float64, ours=ours)
    w32 = uh.cell_oracle(c, data, torch.float32, ours=ours)
    r = uh.cell_compare(cid, ours, w64, w32)
    _check_plans(cid, uh.cell_launches(c), ours["plans"])
    uh.assert_cell(cid, r, uh.cell_cap(c))


@pytest.mark.parametrize("c", uh.MODEL_CASES, ids=uh.model_id)
def test_model_vs_fp64_oracle(dev, c):
    cid = uh.model_id(c)
    data = uh.model_data(c)
    ours = uh.model_hip(c, data, dev)
    if c["crop"]:
        B, H, W = c["shape"]
        Hc, Wc, top, left = uh.crop_geometry(H, W)
        crop = ours["model"].crop
        assert (crop.height_crop_size, crop.width_crop_size, crop.iy0, crop.ix0) == (Hc, Wc, top, left)
        assert tuple(ours["states"][0][9].shape[-2:]) == (Hc, Wc)
    w64 = uh.model_oracle(c, data, torch.float64, ours=ours)
    w32 = uh.model_oracle(c, data, torch.float32, ours=ours)
    r = uh.model_compare(cid, ours, w64, w32)
    _check_plans(cid, uh.model_launches(c), ours["plans"])
    uh.assert_model(cid, c, r)
