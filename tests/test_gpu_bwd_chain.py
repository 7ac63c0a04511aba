"""The chained backward schedule of forward_sequence (snnflow_bwd_chain: the backward task of a
recurrent layer and its consumer's in one block, T + L launches) against today's wavefront launches
(snnflow_bwd_slot, 2(T-1) + L + 1) on identical copies of LIFFireNet at C = 8.

The forward is the same code on both sides: flows, loss and states must be equal.  The backward is
the same arithmetic per (layer, step) in another launch order, so only the fp64 batch-sum atomics may
add in another order: every gradient is held to the bound the suite uses for two launch orders of the
same arithmetic (relative L2 < 1e-5: _check_sequence_vs_per_step and
test_forward_sequence_input_and_state_grads in test_gpu_parity.py)."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def _models(dev, seed):
    import snnflow
    from oracle import lif_ref

    torch.manual_seed(seed)
    ma = snnflow.LIFFireNet(lif_ref.make_unet_kwargs(base_num_channels=8)).to(dev).train()
    mb = copy.deepcopy(ma)
    ma.engine.bwd_chain = False
    mb.engine.bwd_chain = True
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
    real = engine.chained_bwd_slots

    def wrapped(T, rec, chain=(), **kw):
        out = real(T, rec, chain, **kw)
        seen.append((len(out), sum(len(n) == 2 for la in out for n in la)))
        return out

    monkeypatch.setattr(engine, "chained_bwd_slots", wrapped)
    return seen


def _sequence(m, xs):
    """Flows and final states of one window.  forward_sequence hands a single step to the per-step
    path, so T = 1 goes to the sequence node itself."""
    if len(xs) > 1:
        flows = [o["flow"][0] for o in m.forward_sequence(None, xs)]
        return flows, m.states
    from snnflow.engine import FireNetSequence

    eng = m.engine
    res = FireNetSequence.apply(eng, 1, *xs, *m._states, *eng.param_list())
    return [res[0]], list(res[1:])


def _compare(tag, ga, gb):
    assert len(ga) == len(gb)
    worst = 0.0
    for i, (a, b) in enumerate(zip(ga, gb)):
        assert (a is None) == (b is None), (tag, i)
        if a is not None:
            assert np.isfinite(b).all(), (tag, i)
            e = _rel(b, a)
            worst = max(worst, e)
            assert e < TOL, (tag, i, e)
    print(f"[{tag}] worst rel-L2 {worst:.2e}")


def _np(ts):
    return [None if t is None else t.detach().cpu().numpy() for t in ts]


@pytest.mark.parametrize("B,H,W,T", [(1, 8, 32, 2),     # one tile; one pair per loop plus the edge tasks
                                     (2, 40, 72, 3),    # partial tiles; 30 tiles in 32 blocks: idle blocks skip both halves
                                     (1, 16, 32, 1)])   # T = 1: no pair
def test_chained_backward_matches_wavefront(dev, monkeypatch, B, H, W, T):
    seen = _spy(monkeypatch)
    ma, mb = _models(dev, 11)
    _, xs, wts = _inputs(dev, 3, T, B, H, W)
    res = []
    for m in (ma, mb):
        flows, states = _sequence(m, xs)
        loss = sum((f * w).sum() for f, w in zip(flows, wts))
        loss.backward()
        res.append((flows, loss, _np([p.grad for p in m.parameters()]), states))
    (fa, la, pa, sa), (fb, lb, pb, sb) = res
    assert seen == [(T + 7, 2 * (T - 1))]  # only the second model took the chained schedule
    for a, b in zip(fa, fb):
        assert torch.equal(a, b)
    assert la.item() == lb.item()
    for a, b in zip(sa, sb):
        assert torch.equal(a, b)
    _compare(f"params {B}x{H}x{W} T={T}", pa, pb)


def test_chained_backward_two_windows_without_detach(dev, monkeypatch):
    """Two windows of T = 5 chained without detach: the second window's backward hands a state gradient
    to the last step of the first (the unchained task (r+1, T-1) reads it from memory)."""
    seen = _spy(monkeypatch)
    B, H, W, T = 2, 64, 64, 5
    ma, mb = _models(dev, 12)
    _, xs, wts = _inputs(dev, 4, 2 * T, B, H, W)
    res = []
    for m in (ma, mb):
        o1 = m.forward_sequence(None, xs[:T])
        mid = [s.detach().clone() for s in m.states]
        o2 = m.forward_sequence(None, xs[T:])
        flows = [o["flow"][0] for o in o1 + o2]
        loss = sum((f * w).sum() for f, w in zip(flows, wts))
        loss.backward()
        res.append((flows, loss, _np([p.grad for p in m.parameters()]), mid, m.states))
    (fa, la, pa, ma_mid, sa), (fb, lb, pb, mb_mid, sb) = res
    assert seen == [(T + 7, 2 * (T - 1))] * 2
    for a, b in zip(ma_mid, mb_mid):  # the second window starts from equal states
        assert torch.equal(a, b)
    for a, b in zip(fa, fb):
        assert torch.equal(a, b)
    assert la.item() == lb.item()
    for a, b in zip(sa, sb):
        assert torch.equal(a, b)
    _compare("params two windows", pa, pb)


def test_chained_backward_input_and_state_grads(dev, monkeypatch):
    """Inputs and initial states that require grad: the g_x path of the head and the g0 path of step 0
    (whose state gradient leaves the chain: step 0's recurrent tasks stay unchained and store it)."""
    seen = _spy(monkeypatch)
    B, H, W, T, C = 2, 32, 32, 3, 8
    ma, mb = _models(dev, 13)
    gen, xs, wts = _inputs(dev, 5, T, B, H, W)
    st0 = [(torch.rand(2, B, C, H, W, generator=gen, device=dev) * 0.8) for _ in range(7)]
    for s in st0:
        s[1] = (s[1] > 0.5).float()
    res = []
    for m in (ma, mb):
        xg = [x.clone().requires_grad_(True) for x in xs]
        sg = [s.clone().requires_grad_(True) for s in st0]
        m.states = sg
        flows = [o["flow"][0] for o in m.forward_sequence(None, xg)]
        loss = sum((f * w).sum() for f, w in zip(flows, wts))
        loss.backward()
        res.append((flows, loss, _np([p.grad for p in m.parameters()]), _np([x.grad for x in xg]),
                    _np([s.grad for s in sg])))
    (fa, la, pa, xa, ga), (fb, lb, pb, xb, gb) = res
    assert seen == [(T + 7, 2 * (T - 1))]
    for a, b in zip(fa, fb):
        assert torch.equal(a, b)
    assert la.item() == lb.item()
    assert all(g is not None for g in xa) and any(g is not None for g in ga)
    _compare("params", pa, pb)
    _compare("input grads", xa, xb)
    _compare("initial-state grads", ga, gb)
