"""The forward tile pipeline's halo refill order (fwd_lif8_pipe, fwd_chain8_pipe: every wave drains its
own 1-KB chunks of the raw y / membrane halo into registers and refills them by LDS-DMA for the next
tile or half before the LIF phase, with no block barrier in between) against the one-tile-per-block
bodies (snnflow_set_pipe(0, 0) on the wavefront schedule: conv_fwd_body, which uses no LDS-DMA), on
identical copies of LIFFireNet at C = 8 in train mode.

Code under test: fwd_chain in {False, True} x 1, 2, 3 tiles per block.  Every case runs two consecutive
windows of T = 3: the first from reset states (no membrane: no membrane chunk is issued) or from
caller-supplied non-binary states, the second from the first's final states (non-zero membranes and
recurrent spikes).

Both sides run the same arithmetic per (layer, step); only the arrival order of the fp64 batch-sum
atomics may differ.  Everything is held to the bound the suite uses for two launch orders of the same
arithmetic (relative L2 < 1e-5, as test_gpu_fwd_chain.py), and where the pre-BN currents and the batch
statistics are both bit-equal the states must be equal.  (Equal currents alone do not settle the
membranes: a block of two or three tiles adds its tiles' batch sums in fp32 before its fp64 atomics, the
one-tile bodies add one tile's, so the statistics, and with them the membranes, may differ in the last
bit while every spike and every current is the same.  This is so before and after the refill change.)
Each comparison prints whether it came out bit-identical."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-5
L, C, T = 7, 8, 3

# name: (B, H, W, non-binary initial states)
CASES = {
    # 8 tiles per image, partial in both directions, 24 tiles: at 2 tiles per block 16 blocks, eight with
    # two tiles and eight with one (the exit without a refill); at 3, 8 blocks of three tiles (a refill
    # lands on a refilled region)
    "ragged": (3, 30, 50, False),
    "full": (3, 32, 64, False),      # full tiles only
    "one_tile": (2, 8, 32, False),   # 2 tiles in 8 blocks: padding blocks return at once
    # step 0's recurrent tasks take the exact vector path for their s_prev (rec_bf == false)
    "ragged_nonbinary": (3, 30, 50, True),
}


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def _np(ts):
    return [None if t is None else t.detach().cpu().numpy() for t in ts]


def _window(m, xs, states=None):
    """One window through the sequence node itself: flows, final states, captured (ys, stats)."""
    from snnflow.engine import FireNetSequence

    eng = m.engine
    eng.capture_states, eng.keep_seq_states, eng.final_state_out = True, False, None
    try:
        res = FireNetSequence.apply(eng, len(xs), *xs, *(states if states is not None else m._states), *eng.param_list())
    finally:
        eng.capture_states = eng.keep_seq_states = False
    ys, stats, _ = eng.seq_debug
    eng.seq_states, eng.seq_debug = None, None
    n = len(xs)
    return list(res[:n]), list(res[n:]), (ys.clone(), stats.clone())


_BASE, _REF = {}, {}


def _base(dev, case):
    """One model and one set of inputs per case; every run takes a deep copy of the model."""
    if case not in _BASE:
        import snnflow
        from oracle import lif_ref

        B, H, W, nonbin = CASES[case]
        torch.manual_seed(31)
        model = snnflow.LIFFireNet(lif_ref.make_unet_kwargs(base_num_channels=C)).to(dev).train()
        gen = torch.Generator(device=dev).manual_seed(11)
        xs = [(torch.rand(B, 2, H, W, generator=gen, device=dev) < 0.2).float() * 3 for _ in range(2 * T)]
        wts = [torch.randn(B, 2, H, W, generator=gen, device=dev) for _ in range(2 * T)]
        st0 = None
        if nonbin:  # spike halves in (0, 0.8)
            st0 = [torch.rand(2, B, C, H, W, generator=gen, device=dev) * 0.8 for _ in range(L)]
        _BASE[case] = (model, xs, wts, st0)
    return _BASE[case]


def _run(dev, case, chain, tiles):
    """Two consecutive windows and one backward pass with `tiles` tiles per block (0: one-tile bodies)."""
    from snnflow import _lib

    base, xs, wts, st0 = _base(dev, case)
    m = copy.deepcopy(base)
    m.engine.fwd_chain = chain
    old = _lib.lib.snnflow_get_pipe(0)
    assert _lib.lib.snnflow_set_pipe(tiles, 0) == 0
    try:
        f1, s1, (y1, t1) = _window(m, xs[:T], states=None if st0 is None else [s.clone() for s in st0])
        f2, s2, (y2, t2) = _window(m, xs[T:], states=s1)
        flows = f1 + f2
        loss = sum((f * w).sum() for f, w in zip(flows, wts))
        loss.backward()
        torch.cuda.synchronize()
    finally:
        _lib.lib.snnflow_set_pipe(old, 0)
    return {"ys": _np([y1, y2]), "stats": _np([t1, t2]), "flows": _np(flows), "states between": _np(s1),
            "final states": _np(s2), "loss": loss.item(), "parameter gradients": _np([p.grad for p in m.parameters()])}


def _reference(dev, case):
    """The wavefront schedule on the one-tile-per-block bodies: computed once per case, never changed."""
    if case not in _REF:
        _REF[case] = _run(dev, case, False, 0)
    return _REF[case]


def _compare(tag, ga, gb):
    """ga: reference, gb: under test; lists of arrays (None allowed on both sides alike)."""
    assert len(ga) == len(gb)
    worst, same = 0.0, True
    for i, (a, b) in enumerate(zip(ga, gb)):
        assert (a is None) == (b is None), (tag, i)
        if a is not None:
            assert np.isfinite(b).all(), (tag, i)
            e = _rel(b, a)
            worst = max(worst, e)
            same = same and np.array_equal(a, b)
            assert e < TOL, (tag, i, e)
    print(f"[{tag}] worst rel-L2 {worst:.2e} bit-identical {same}")
    return same


@pytest.mark.parametrize("tiles", [1, 2, 3])
@pytest.mark.parametrize("chain", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_refill_order_matches_one_tile_bodies(dev, case, chain, tiles):
    ref = _reference(dev, case)
    got = _run(dev, case, chain, tiles)
    tag = f"{case} chain={chain} tiles={tiles}"
    ys_same = _compare(f"{tag} ys", ref["ys"], got["ys"])
    stats_same = _compare(f"{tag} stats", ref["stats"], got["stats"])
    _compare(f"{tag} flows", ref["flows"], got["flows"])
    st_same = _compare(f"{tag} states between", ref["states between"], got["states between"])
    st_same = _compare(f"{tag} final states", ref["final states"], got["final states"]) and st_same
    if ys_same and stats_same:  # equal currents and statistics: equal membranes and spikes
        assert st_same, tag
    la, lb = ref["loss"], got["loss"]
    print(f"[{tag}] loss {la!r} / {lb!r} bit-identical {la == lb}")
    assert abs(lb - la) <= TOL * max(abs(la), 1e-30), (tag, la, lb)
    _compare(f"{tag} parameter gradients", ref["parameter gradients"], got["parameter gradients"])
