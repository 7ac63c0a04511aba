"""CPU-side validation of the U-Net ragged-shape harness (tests/unet_harness.py; no GPU).

The fp32 CPU oracle plays "ours" against the fp64 oracle through the compare and assert functions
test_gpu_unet_ragged.py uses, for every cell and model case of that file: the harness can pass, and the
reference-against-reference figures the limits rest on are printed.  The conditions on the committed
seeds are held here: the fp64 oracle alone keeps at most 0.01 % (cells) / 0.03 % (models) of a case's
neuron-steps within 1e-4 of the threshold, which caps what the GPU test may adopt.

Dispatch coverage: the harness's restatement of the host-side kernel selection of csrc/unet.hip must
reproduce the library's snnflow_unet_conv_ksplit and snnflow_unet_wgrad_partial_floats for every GEMM
launch of every case, and the union of the launches' labels must reach every instantiation that
snnflow_unet_conv and snnflow_unet_wgrad can dispatch.

What this file does not test: with the fp32 oracle as "ours", the fp32 oracle that follows ours is ours
itself, so the gradient limit max(2 x the fp32 oracle's error, 2e-5) holds trivially here; the figures
printed are the reference-against-reference errors the GPU file's limit rests on."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unet_harness as uh  # noqa: E402


@pytest.fixture(scope="module")
def cell64():
    """The data and the free-running fp64 oracle's result of every cell case, computed once."""
    cache = {}

    def get(c):
        cid = uh.cell_id(c)
        if cid not in cache:
            data = uh.cell_data(c)
            cache[cid] = (data, uh.cell_oracle(c, data, torch.float64))
        return cache[cid]

    return get


@pytest.mark.parametrize("c", uh.CELL_CASES, ids=uh.cell_id)
def test_cell_takes_the_gemm_path(c):
    from snnflow import convlif

    assert not convlif._fixed_kernel(uh.new_hip_cell(c)), uh.cell_id(c)


@pytest.mark.parametrize("c", uh.CELL_CASES, ids=uh.cell_id)
def test_cell_near_threshold_cap(cell64, c):
    """A condition on the committed seeds, not a measurement."""
    _, want = cell64(c)
    print(f"\n[{uh.cell_id(c)}] fp64 oracle: {want['near']} of {uh.cell_neuron_steps(c)} neuron-steps within "
          f"{uh.EPS} of the threshold, cap {uh.cell_cap(c)}")
    assert want["near"] <= uh.cell_cap(c), (uh.cell_id(c), want["near"], uh.cell_cap(c))


@pytest.mark.parametrize("c", uh.CELL_CASES, ids=uh.cell_id)
def test_cell_fp32_oracle_vs_fp64(cell64, c):
    data, _ = cell64(c)
    ours = uh.cell_oracle(c, data, torch.float32)
    want = uh.cell_oracle(c, data, torch.float64, ours=ours)
    cid = uh.cell_id(c)
    r = uh.cell_compare(f"cpu32 {cid}", ours, want, ours)
    uh.assert_cell(cid, r, uh.cell_cap(c))


@pytest.mark.parametrize("c", uh.MODEL_CASES, ids=uh.model_id)
def test_model_fp32_oracle_vs_fp64(c):
    """The free-running fp64 oracle's near-threshold count under the 0.03 % cap, then the fp32 oracle
    as "ours" against the fp64 oracle following it."""
    cid = uh.model_id(c)
    data = uh.model_data(c)
    free = uh.model_oracle(c, data, torch.float64)
    print(f"\n[{cid}] fp64 oracle: {free['near']} of {uh.model_neuron_steps(c)} neuron-steps within {uh.EPS} of the "
          f"threshold, cap {uh.model_cap(c)}")
    assert free["near"] <= uh.model_cap(c), (cid, free["near"], uh.model_cap(c))
    ours = uh.model_oracle(c, data, torch.float32)
    want = uh.model_oracle(c, data, torch.float64, ours=ours)
    r = uh.model_compare(f"cpu32 {cid}", ours, want, ours)
    uh.assert_model(cid, c, r)


@pytest.mark.parametrize("H,W", [(37, 51), (20, 44), (16, 32), (1, 17)])
def test_crop_parameters(H, W):
    """CropParameters pads to the smallest multiple of 16 (the extra row / column at the top / left),
    and crop(pad(x)) = x."""
    from snnflow.unet import CropParameters

    cp = CropParameters(W, H, 4)
    Hc, Wc, top, left = uh.crop_geometry(H, W)
    assert Hc % 16 == 0 and Wc % 16 == 0 and 0 <= Hc - H < 16 and 0 <= Wc - W < 16
    assert (cp.height_crop_size, cp.width_crop_size) == (Hc, Wc)
    assert (cp.padding_top, cp.padding_left) == (top, left) == (cp.iy0, cp.ix0)
    assert (cp.padding_bottom, cp.padding_right) == (Hc - H - top, Wc - W - left)
    assert top >= Hc - H - top and left >= Wc - W - left
    x = torch.arange(2 * 3 * H * W, dtype=torch.float32).view(2, 3, H, W) + 1
    p = cp.pad(x)
    assert p.shape == (2, 3, Hc, Wc) and float(p.sum()) == float(x.sum())
    assert torch.equal(cp.crop(p), x)
    assert torch.equal(p[:, :, cp.iy0:cp.iy1, cp.ix0:cp.ix1], x)


def _all_launches():
    return ([(uh.cell_id(c), uh.cell_launches(c)) for c in uh.CELL_CASES]
            + [(uh.model_id(c), uh.model_launches(c)) for c in uh.MODEL_CASES])


def test_selection_restatement_equals_library():
    """Every launch of every case: the restated split-K factor and weight-gradient partial-float
    count equal the library's host functions."""
    n = 0
    for cid, launches in _all_launches():
        for l in launches:
            if l["kind"] == "wgrad":
                assert uh.wgrad_partial_floats(l) == uh.lib_wgrad_partial_floats(l), (cid, l, uh.wgrad_plan(l))
            else:
                assert uh.conv_ksplit(l) == uh.lib_conv_ksplit(l), (cid, l)
            n += 1
    print(f"\n{n} launches: restated selection equal to the library")


def test_row_strip_plans_differ_from_generic():
    """The logged plan of a weight gradient is its partial-float count.  A row-strip launch and the
    generic launch of the same shape can have equal counts (same padded tile, same split), and then
    neither the library pin above nor the GPU test's PLAN_LOG comparison can tell which kernel ran.  So
    every row-strip variant must have a launch whose count differs from the generic kernel's at that shape."""
    told = {}
    for cid, launches in _all_launches():
        for l in launches:
            if l["kind"] == "wgrad" and uh.wrows_eligible(l):
                if uh.wgrad_partial_floats(l) != uh.wgrad_partial_floats(l, rows=False):
                    told.setdefault(uh.wgrad_plan(l)[0], set()).add(cid)
    for label in ("rows-s2", "rows-m32", "rows-m64"):
        print(f"{label}: plan differs from the generic kernel's in {sorted(told.get(label, []))}")
        assert told.get(label), label


def test_dispatch_coverage():
    """The union over all cases reaches every instantiation; the table is printed."""
    reached = {}
    for cid, launches in _all_launches():
        labels = sorted({x for l in launches for x in uh.launch_labels(l)})
        print(f"{cid}: {' '.join(labels)}")
        for x in labels:
            reached.setdefault(x, []).append(cid)
    print()
    missing = []
    for req in uh.REQUIRED_LABELS:
        by = sorted({cid for x, cids in reached.items() if uh.label_reached(req, [x]) for cid in cids})
        print(f"{req}: {len(by)} cases ({', '.join(by[:4])}{', ...' if len(by) > 4 else ''})")
        if not by:
            missing.append(req)
    assert not missing, f"unreached: {missing}"
    known = [x for x in reached if not any(uh.label_reached(req, [x]) for req in uh.REQUIRED_LABELS)]
    print("labels outside the required list: " + ", ".join(sorted(known)))
