"""The chained forward schedule of forward_sequence (snnflow_fwd_chain: the task that computes a
recurrent layer's spikes and that layer's task of the next step in one block, T + L launches) against
today's wavefront launches (snnflow_fwd_slot, 2(T-1) + L + 1) on identical copies of LIFFireNet at
C = 8 in train mode.

Both schedules run the same arithmetic per (layer, step) over the same tiles per block; only the
arrival order of the fp64 batch-sum atomics may differ.  Everything is held to the bound the suite uses
for two launch orders of the same arithmetic (relative L2 < 1e-5: _check_sequence_vs_per_step in
test_gpu_parity.py, test_gpu_bwd_chain.py), and where both schedules' pre-BN currents are bit-equal the
states (membranes and spikes) must be equal.  Each comparison prints whether it came out bit-identical."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-5
L = 7


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def _models(dev, seed):
    import snnflow
    from oracle import lif_ref

    torch.manual_seed(seed)
    ma = snnflow.LIFFireNet(lif_ref.make_unet_kwargs(base_num_channels=8)).to(dev).train()
    mb = copy.deepcopy(ma)
    ma.engine.fwd_chain = False
    mb.engine.fwd_chain = True
    return ma, mb


def _inputs(dev, seed, n, B, H, W):
    gen = torch.Generator(device=dev).manual_seed(seed)
    xs = [(torch.rand(B, 2, H, W, generator=gen, device=dev) < 0.2).float() * 3 for _ in range(n)]
    wts = [torch.randn(B, 2, H, W, generator=gen, device=dev) for _ in range(n)]
    return gen, xs, wts


def _spy(monkeypatch):
    """Records the schedules the chained path asks for: [(launches, pairs)]."""
    from snnflow import engine

    seen = []
    real = engine.chained_fwd_slots

    def wrapped(T, rec, chain=(), **kw):
        out = real(T, rec, chain, **kw)
        seen.append((len(out), sum(len(n) == 2 for la in out for n in la)))
        return out

    monkeypatch.setattr(engine, "chained_fwd_slots", wrapped)
    return seen


def _window(m, xs, states=None, keep=False, fin=None):
    """One window through the sequence node itself (forward_sequence hands T = 1 to the per-step path and
    ties keep_seq_states to capture_states): flows, final states, captured (ys, stats), per-step states."""
    from snnflow.engine import FireNetSequence

    eng = m.engine
    eng.capture_states, eng.keep_seq_states, eng.final_state_out = True, keep, fin
    try:
        res = FireNetSequence.apply(eng, len(xs), *xs, *(states if states is not None else m._states), *eng.param_list())
    finally:
        eng.capture_states = eng.keep_seq_states = False
    ys, stats, _ = eng.seq_debug
    seq, eng.seq_states, eng.seq_debug = eng.seq_states, None, None
    T = len(xs)
    return list(res[:T]), list(res[T:]), (ys.clone(), stats.clone()), seq


def _np(ts):
    return [None if t is None else t.detach().cpu().numpy() for t in ts]


def _compare(tag, ga, gb):
    """ga: wavefront, gb: chained; lists of arrays (None allowed on both sides alike)."""
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


def _compare_runs(tag, ra, rb, wts):
    """Flows, loss, final states, captured ys / stats and the parameter gradients of two windows."""
    (fa, sa, (ya, ta), _, ma), (fb, sb, (yb, tb), _, mb) = ra, rb
    ys_same = _compare(f"{tag} ys", _np([ya]), _np([yb]))
    _compare(f"{tag} stats", _np([ta]), _np([tb]))
    _compare(f"{tag} flows", _np(fa), _np(fb))
    st_same = _compare(f"{tag} final states", _np(sa), _np(sb))
    if ys_same:  # equal currents: equal membranes and spikes
        assert st_same, tag
    grads = []
    for m, flows in ((ma, fa), (mb, fb)):
        loss = sum((f * w).sum() for f, w in zip(flows, wts))
        loss.backward()
        grads.append((loss.item(), _np([p.grad for p in m.parameters()])))
    (la, pa), (lb, pb) = grads
    print(f"[{tag}] loss {la!r} / {lb!r} bit-identical {la == lb}")
    assert abs(lb - la) <= TOL * max(abs(la), 1e-30), (tag, la, lb)
    _compare(f"{tag} parameter gradients", pa, pb)


@pytest.mark.parametrize("B,H,W,T", [(1, 8, 32, 2),     # one tile; one pair per loop plus the unchained edge tasks
                                     (2, 40, 72, 3),    # partial tiles; 30 tiles in 16 blocks: one or two tiles per block
                                     (1, 16, 32, 1)])   # T = 1: no pair, today's launches
def test_chained_forward_matches_wavefront(dev, monkeypatch, B, H, W, T):
    seen = _spy(monkeypatch)
    ma, mb = _models(dev, 21)
    _, xs, wts = _inputs(dev, 6, T, B, H, W)
    runs = [_window(m, xs) + (m,) for m in (ma, mb)]
    assert seen == [(T + L, 2 * (T - 1))]  # only the second model took the chained schedule
    _compare_runs(f"{B}x{H}x{W} T={T}", runs[0], runs[1], wts)


def test_chained_forward_non_binary_initial_spikes(dev, monkeypatch):
    """Caller-supplied initial states whose spike halves are not 0/1: step 0's recurrent tasks stay
    unchained and take the exact vector path for their s_prev."""
    seen = _spy(monkeypatch)
    B, H, W, T, C = 2, 32, 32, 3, 8
    ma, mb = _models(dev, 22)
    gen, xs, wts = _inputs(dev, 7, T, B, H, W)
    st0 = [torch.rand(2, B, C, H, W, generator=gen, device=dev) * 0.8 for _ in range(L)]  # spike halves in (0, 0.8)
    runs = [_window(m, xs, states=[s.clone() for s in st0]) + (m,) for m in (ma, mb)]
    assert seen == [(T + L, 2 * (T - 1))]
    _compare_runs("non-binary s_prev", runs[0], runs[1], wts)


def test_chained_forward_two_windows_without_detach(dev, monkeypatch):
    """Two windows of T = 5 chained without detach (forward_sequence: the state_spk_skip rules of the
    feed-forward layers apply, the second window's step 0 reads the first's final states)."""
    seen = _spy(monkeypatch)
    B, H, W, T = 2, 64, 64, 5
    ma, mb = _models(dev, 23)
    _, xs, wts = _inputs(dev, 8, 2 * T, B, H, W)
    res = []
    for m in (ma, mb):
        o1 = m.forward_sequence(None, xs[:T])
        mid = [s.detach().clone() for s in m.states]
        o2 = m.forward_sequence(None, xs[T:])
        flows = [o["flow"][0] for o in o1 + o2]
        loss = sum((f * w).sum() for f, w in zip(flows, wts))
        loss.backward()
        res.append((flows, loss.item(), _np([p.grad for p in m.parameters()]), mid, list(m.states)))
    (fa, la, pa, mida, sa), (fb, lb, pb, midb, sb) = res
    assert seen == [(T + L, 2 * (T - 1))] * 2
    _compare("two windows: states between", _np(mida), _np(midb))
    _compare("two windows: flows", _np(fa), _np(fb))
    _compare("two windows: final states", _np(sa), _np(sb))
    print(f"[two windows] loss {la!r} / {lb!r} bit-identical {la == lb}")
    assert abs(lb - la) <= TOL * max(abs(la), 1e-30)
    _compare("two windows: parameter gradients", pa, pb)


def test_chained_forward_keeps_every_step_state(dev, monkeypatch):
    """keep_seq_states with a final_state_out buffer: every step's states (spike halves included) and the
    handed-over buffer are equal between the schedules."""
    seen = _spy(monkeypatch)
    B, H, W, T, C = 2, 32, 32, 3, 8
    ma, mb = _models(dev, 24)
    _, xs, wts = _inputs(dev, 9, T, B, H, W)
    runs, fins = [], []
    for m in (ma, mb):
        fin = torch.full((L * 2 * B * H * W * C,), float("nan"), device=dev)
        runs.append(_window(m, xs, keep=True, fin=fin) + (m,))
        fins.append(fin)
    assert seen == [(T + L, 2 * (T - 1))]
    seqa, seqb = runs[0][3], runs[1][3]
    assert len(seqa) == len(seqb) == T
    for t in range(T):
        assert len(seqa[t]) == len(seqb[t]) == L
        for l in range(L):
            assert torch.equal(seqa[t][l], seqb[t][l]), (t, l)
    assert torch.isfinite(fins[1]).all() and torch.equal(fins[0], fins[1])
    _compare_runs("keep_seq_states", runs[0], runs[1], wts)
