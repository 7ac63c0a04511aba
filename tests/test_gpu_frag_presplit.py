"""The C = 8 input-gradient weight fragments split once per step (k_prep_weights' fragb images, copied
into LDS by the backward kernels) against the split inside every block (engine.frag8 = False: the kernels
get NULL fragment pointers) on identical copies of LIFFireNet at C = 8 in train mode.  The forward kernels
split in the block on both sides (their share of the change measured no gain and was not kept), so the
forward results also show that the preparation of the images disturbs nothing.

Both sides feed the matrix cores the same bf16 hi / mid / lo bits, so only the arrival order of the fp64
batch-sum atomics may differ: everything is held to the suite's bound for one arithmetic under two
arrival orders (relative L2 <= 1e-5: test_gpu_fwd_chain.py, test_gpu_bwd_chain.py).  Each comparison
prints whether it came out bit-identical.

Shapes: B = 2, 20 x 40 (8 x 32 tiles: a 3 x 2 tile grid with a ragged bottom row and a ragged right column,
forward blocks own two tiles), T = 3 (chained pairs in both directions) and T = 1 (no pair)."""
import copy

import numpy as np
import pytest
import torch

import firenet_harness as fh

pytestmark = pytest.mark.gpu

TOL = 1e-5
L = 7
B, H, W, N = 2, 20, 40, 64


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def _np(ts):
    return [None if t is None else t.detach().cpu().numpy() for t in ts]


def _compare(tag, ga, gb):
    """ga: split in every block, gb: split once; lists of arrays (None allowed on both sides alike)."""
    assert len(ga) == len(gb)
    worst, same = 0.0, True
    for i, (a, b) in enumerate(zip(ga, gb)):
        assert (a is None) == (b is None), (tag, i)
        if a is not None:
            assert np.isfinite(b).all(), (tag, i)
            e = _rel(b, a)
            worst = max(worst, e)
            same = same and np.array_equal(a, b)
            assert e <= TOL, (tag, i, e)
    print(f"[{tag}] worst rel-L2 {worst:.2e} bit-identical {same}")
    return same


def _models(dev, seed, chain=True):
    import snnflow
    from oracle import lif_ref

    torch.manual_seed(seed)
    ma = snnflow.LIFFireNet(lif_ref.make_unet_kwargs(base_num_channels=8)).to(dev).train()
    mb = copy.deepcopy(ma)
    ma.engine.frag8 = False
    mb.engine.frag8 = True
    for m in (ma, mb):
        m.engine.fwd_chain = m.engine.bwd_chain = chain
    return ma, mb


def _windows(dev, T, seed):
    return [{k: v.to(dev) for k, v in w.items()} for w in fh.cpu_windows(B, H, W, T, N, seed)]


def _sequence(m, wins):
    """One window through the sequence node itself (forward_sequence hands T = 1 to the per-step path):
    flows, final states, captured (ys, stats)."""
    from snnflow.engine import FireNetSequence

    eng = m.engine
    xs = [w["event_cnt"] for w in wins]
    eng.capture_states = True
    try:
        res = FireNetSequence.apply(eng, len(xs), *xs, *m._states, *eng.param_list())
    finally:
        eng.capture_states = False
    ys, stats, _ = eng.seq_debug
    eng.seq_states, eng.seq_debug = None, None
    T = len(xs)
    return list(res[:T]), list(res[T:]), [ys.clone(), stats.clone()]


def _per_step(m, wins):
    flows = [m(w["event_voxel"], w["event_cnt"])["flow"][0] for w in wins]
    return flows, list(m._states), []


def _loss_backward(dev, m, flows, wins):
    import snnflow

    ew = snnflow.EventWarping(fh.cfg(H, W), dev)
    for f, w in zip(flows, wins):
        ew.event_flow_association([f], w["event_list"], w["event_list_pol_mask"], w["event_mask"])
    loss = ew()
    loss.backward()
    return loss.item(), _np([p.grad for p in m.parameters()])


def _compare_windows(tag, ra, rb):
    (fa, sa, da, la, pa), (fb, sb, db, lb, pb) = ra, rb
    _compare(f"{tag} ys / stats", _np(da), _np(db))
    _compare(f"{tag} flows", _np(fa), _np(fb))
    _compare(f"{tag} final states", _np(sa), _np(sb))
    print(f"[{tag}] loss {la!r} / {lb!r} bit-identical {la == lb}")
    assert np.isfinite(lb) and abs(lb - la) <= TOL * max(abs(la), 1e-30), (tag, la, lb)
    assert all(p is not None for p in pb), tag
    _compare(f"{tag} parameter gradients", pa, pb)


# ---------------------------------------------------------------------------
# 1. the images
# ---------------------------------------------------------------------------
def _host_image(w, fwd):
    """prep_frag's layout for an 8 x 8 conv: int16 [chunk 0..2][part hi / mid / lo][lane 16 g + n][j] with
    tap = 4 chunk + g; forward n = co, j = ci; input gradient n = ci, j = co; columns n >= 8 and taps >= 9
    zero.  The split is the kernels' three-part round-to-nearest one."""
    w = w.detach().cpu().float().contiguous()
    h = w.bfloat16()
    r1 = w - h.float()
    m = r1.bfloat16()
    lo = (r1 - m.float()).bfloat16()
    img = torch.zeros(3, 3, 64, 8, dtype=torch.int16)
    for q, p in enumerate((h, m, lo)):
        bits = p.contiguous().view(torch.int16).reshape(8, 8, 9)  # [co][ci][tap]
        for tap in range(9):
            ch, g = divmod(tap, 4)
            blk = bits[:, :, tap]
            img[ch, q, 16 * g:16 * g + 8, :] = blk if fwd else blk.t()
    return img.reshape(-1)


def test_prepared_images_match_host_split(dev):
    from snnflow import _lib

    m, _ = _models(dev, 31)
    eng = m.engine
    half = 1.0 + 2.0 ** -8  # exactly between the bf16 neighbours 1 and 1 + 2^-7
    special = torch.tensor([0.0, -0.0, 2.0 ** -120, -(2.0 ** -120), half, -half, 1024.0 + 2.0 ** -3 + 2.0 ** -11,
                            -(2.0 ** 10) * (1.0 + 2.0 ** -8)], device=dev)
    eng.param_list()
    eng.prep_weights(_lib.stream_ptr(dev))  # buffers exist; the edit below must refresh them
    convs = [(i, w) for i, w in enumerate(eng._prep_ws) if w.shape[0] == w.shape[1]]
    assert len(convs) == 8  # six feed-forward and two recurrent 8 x 8 convs
    with torch.no_grad():
        for k, (_, w) in enumerate(convs):
            idx = (torch.arange(special.numel(), device=dev) * 67 + 5 * k) % w.numel()
            w.view(-1)[idx] = special
    eng.prep_weights(_lib.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    assert eng.prep.frag.get(0) is None and eng.prep.fragb.get(0) is None  # the head (2 -> 8) has no fragments
    for i, w in convs:
        assert eng.prep.frag[i] is None  # C = 8: no forward image (the forward kernels split in the block)
        for name, img, fwd in (("fragb", eng.prep.fragb[i], False),):
            assert img is not None and img.numel() == _lib.lib.snnflow_frag_halfs(8, 8) == 4608
            want = _host_image(w, fwd)
            got = img.cpu()
            bad = int((got != want).sum())
            print(f"[images] conv {i} {name}: {bad} of {want.numel()} halves differ")
            assert bad == 0, (i, name, bad)


# ---------------------------------------------------------------------------
# 2. on against off, one window
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("T,path", [(3, "chained"), (3, "wavefront"), (3, "per_step"), (1, "chained")],
                         ids=["T3-chained", "T3-wavefront", "T3-per-step", "T1-sequence-node"])
def test_presplit_matches_in_block_split(dev, T, path):
    ma, mb = _models(dev, 32, chain=path == "chained")
    wins = _windows(dev, T, seed=2)
    runs = []
    for m in (ma, mb):
        flows, states, dbg = (_per_step if path == "per_step" else _sequence)(m, wins)
        runs.append((flows, states, dbg) + _loss_backward(dev, m, flows, wins))
    _compare_windows(f"T={T} {path}", runs[0], runs[1])


# ---------------------------------------------------------------------------
# 3. weights that change between windows
# ---------------------------------------------------------------------------
def _train_window(dev, m, lf, wins, seed=None):
    lf.reset()
    outs = m.forward_sequence([w["event_voxel"] for w in wins], [w["event_cnt"] for w in wins])
    for o, w in zip(outs, wins):
        lf.event_flow_association(o["flow"], w["event_list"], w["event_list_pol_mask"], w["event_mask"])
    loss = lf()
    if seed is None:
        loss.backward()
    else:
        loss.backward(seed)
    return loss, [o["flow"][0] for o in outs]


def test_two_windows_with_optimizer_step(dev):
    """The second window runs on weights ClipAdam has just changed: a stale image would show here."""
    import snnflow

    T = 3
    ma, mb = _models(dev, 33)
    pool = [_windows(dev, T, seed=3), _windows(dev, T, seed=4)]
    res = []
    for m in (ma, mb):
        lf = snnflow.EventWarping(fh.cfg(H, W), dev)
        opt = snnflow.ClipAdam(list(m.parameters()), lr=1e-2, max_norm=1.0)
        per = []
        for wins in pool:
            opt.zero_grad(set_to_none=True)
            loss, flows = _train_window(dev, m, lf, wins)
            per.append((loss.item(), _np(flows), _np([p.grad for p in m.parameters()])))
            opt.step()
            m.detach_states()
        res.append((per, _np(list(m.parameters()))))
    (pa, wa), (pb, wb) = res
    for j, ((la, fa, ga), (lb, fb, gb)) in enumerate(zip(pa, pb)):
        print(f"[window {j}] loss {la!r} / {lb!r} bit-identical {la == lb}")
        assert np.isfinite(lb) and abs(lb - la) <= TOL * max(abs(la), 1e-30), (j, la, lb)
        _compare(f"window {j} flows", fa, fb)
        _compare(f"window {j} parameter gradients", ga, gb)
    assert pb[0][0] != pb[1][0]
    _compare("parameters after two steps", wa, wb)


def test_two_steps_graph_replay_matches_eager(dev):
    """The bench's timed step at a small size (test_bench_graph_pingpong_matches_eager's procedure): one
    graph per resident batch holding forward_sequence + EventWarping + backward + ClipAdam, replayed once
    each, against the same two steps run eagerly; the replay must use the image of the weights the replay
    itself has just written.  Loss and parameters."""
    import bench
    import snnflow
    from oracle import lif_ref
    from snnflow.synthetic import make_window

    T = 3
    gen = torch.Generator(device=dev).manual_seed(12)
    pool = [bench._pack([make_window(B, N, H, W, gen, dev) for _ in range(T)]) for _ in range(2)]
    seed = torch.ones((), device=dev)

    def build():
        torch.manual_seed(34)
        m = snnflow.LIFFireNet(lif_ref.make_unet_kwargs(base_num_channels=8)).to(dev).train()
        assert m.engine.frag8
        return m, snnflow.EventWarping(fh.cfg(H, W), dev), snnflow.ClipAdam(list(m.parameters()), lr=1e-2, max_norm=1.0)

    me, lfe, oe = build()
    want = []
    for j in range(2):
        oe.zero_grad(set_to_none=True)
        loss, _ = _train_window(dev, me, lfe, pool[j][1], seed)
        oe.step()
        want.append((loss.item(), _np(list(me.parameters()))))
        me.detach_states()

    mg, lfg, og = build()
    init = {k: v.detach().clone() for k, v in mg.state_dict().items()}
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for j in range(3):
            og.zero_grad(set_to_none=True)
            _train_window(dev, mg, lfg, pool[j % 2][1], seed)
            og.step()
            mg.detach_states()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    pingpong = bench.StatePingPong(dev, mg._states)
    graphs, losses = [], []
    for j in range(pingpong.cycle(len(pool))):
        og.zero_grad(set_to_none=True)
        pingpong.arm(mg, j)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            losses.append(_train_window(dev, mg, lfg, pool[j % len(pool)][1], seed)[0])
            og.step()
        graphs.append(g)
    with torch.no_grad():
        for k, v in mg.state_dict().items():
            v.copy_(init[k])
        for t in og._moments[1:4]:
            t.zero_()
        for b in pingpong.bufs:
            b.zero_()
    torch.cuda.synchronize(dev)
    for j in range(2):
        graphs[j].replay()
        torch.cuda.synchronize(dev)
        wl, wp = want[j]
        gl = losses[j].item()
        print(f"[graph step {j}] loss {gl!r} / eager {wl!r} bit-identical {gl == wl}")
        assert np.isfinite(gl) and abs(gl - wl) <= TOL * max(abs(wl), 1e-30), (j, gl, wl)
        _compare(f"graph step {j} parameters", wp, _np(list(mg.parameters())))
    assert want[0][0] != want[1][0]


# ---------------------------------------------------------------------------
# 4. the switch reaches the kernels
# ---------------------------------------------------------------------------
def _spy(monkeypatch):
    """Records the fragment pointers the argument builders hand to the kernels: {(direction, layer,
    ff set, rec set)} per engine."""
    from snnflow import engine

    seen = {}

    def wrap(name, fields, direction):
        real = getattr(engine, name)

        def wrapped(eng, l, *args, **kw):
            a = real(eng, l, *args, **kw)
            seen.setdefault(id(eng), set()).add((direction, l) + tuple(bool(getattr(a, f)) for f in fields))
            return a

        monkeypatch.setattr(engine, name, wrapped)

    wrap("_fwd_conv_args", ("wf_ff", "wf_rec"), "fwd")
    wrap("_bwd_layer_args", ("wd_ff", "wd_rec"), "bwd")
    return seen


@pytest.mark.parametrize("on", [False, True], ids=["off", "on"])
def test_switch_reaches_the_kernels(dev, monkeypatch, on):
    seen = _spy(monkeypatch)
    _, m = _models(dev, 35)
    eng = m.engine
    assert eng.frag8  # the default
    eng.frag8 = on
    wins = _windows(dev, 2, seed=5)
    flows, _, _ = _sequence(m, wins)
    _loss_backward(dev, m, flows, wins)
    rec = list(eng.rec)
    assert sum(rec) == 2 and not rec[0]
    want = set()
    for l in range(L):
        b = l > 0 and on
        want.add(("fwd", l, False, False))  # C = 8: the forward kernels take no image
        want.add(("bwd", l, b, b and rec[l]))
    assert seen[id(eng)] == want, sorted(seen[id(eng)] ^ want)
    # the C step driver's plan (the per-step path) carries the same pointers
    m.detach_states()
    m(wins[0]["event_voxel"], wins[0]["event_cnt"])
    plan = eng._plan[1]
    for l in range(L):
        assert not plan.wf_ff[l] and not plan.wf_rec[l], l
        assert bool(plan.wd_ff[l]) == (l > 0 and on) and bool(plan.wd_rec[l]) == (rec[l] and on), l
