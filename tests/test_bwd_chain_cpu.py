"""The chained backward schedule (snnflow.engine.chained_bwd_slots) and the validation of
snnflow_bwd_chain, without a GPU.

A schedule is checked against the dependencies of the backward tasks written out here on their own
(not taken from the scheduler): task (k, t) -- layer k at step t, k = L the top task -- follows
(k+1, t), (k, t+1) and, where layer k-1 is recurrent, (k-1, t+1)."""
import ctypes

import pytest

from snnflow import _lib
from snnflow.engine import chainable_layers, chained_bwd_slots, wavefront_slots

F, R = False, True
SPECS = {
    "no_recurrent": [F, F, F, F, F, F, F],          # LIFFireFlowNet
    "liffirenet": [F, R, F, F, R, F, F],            # head, G1, R1a, R1b, G2, R2a, R2b
    "adjacent_recurrent": [F, R, R, F, F, F, F],
    "recurrent_last": [F, F, F, F, F, F, R],
}
TS = (1, 2, 3, 10)


def _deps(k, t, T, rec):
    L = len(rec)
    d = []
    if k < L:
        d.append((k + 1, t))
    if t + 1 < T:
        d.append((k, t + 1))
        if k >= 1 and rec[k - 1]:
            d.append((k - 1, t + 1))
    return d


def _check(T, rec, chain):
    L = len(rec)
    launches = chained_bwd_slots(T, rec, chain)
    where, node_of = {}, {}
    for i, la in enumerate(launches):
        assert la, "empty launch"
        assert sum(1 for n in la for k, _ in n if k < L) <= _lib.MAX_CHAIN_TASKS
        assert sum(1 for n in la for k, _ in n if k == L) <= 1  # one top task per launch
        for n in la:
            assert len(n) in (1, 2)
            if len(n) == 2:  # (recurrent (r, t+1), feed-forward (r+1, t)), r chained
                (r, t1), (k2, t) = n
                assert r in chain and k2 == r + 1 and t1 == t + 1 and rec[r] and not rec[r + 1] and 1 <= r < L - 1
            for task in n:
                assert task not in where, task
                where[task] = i
                node_of[task] = n
    assert sorted(where) == [(k, t) for k in range(L + 1) for t in range(T)]  # every task once
    for (k, t), i in where.items():
        for dep in _deps(k, t, T, rec):
            if node_of[dep] is node_of[(k, t)]:
                # the only dependency a pair keeps inside: the spike gradient handed from (r, t+1) to (r+1, t)
                assert dep == (k - 1, t + 1) and node_of[dep] == (dep, (k, t))
            else:
                assert where[dep] < i, (T, rec, (k, t), dep)
    for k in range(L + 1):  # one layer's tasks: distinct launches, descending t
        order = [where[(k, t)] for t in range(T - 1, -1, -1)]
        assert all(a < b for a, b in zip(order, order[1:])), (k, order)
    for r in chain:  # every step that can be chained is
        for t in range(T - 1):
            assert node_of[(r, t + 1)] == ((r, t + 1), (r + 1, t))
    return launches


@pytest.mark.parametrize("name", sorted(SPECS))
@pytest.mark.parametrize("T", TS)
def test_schedule_respects_dependencies(name, T):
    rec = SPECS[name]
    _check(T, rec, chainable_layers(rec))
    _check(T, rec, [])


def test_chainable_layers():
    assert chainable_layers(SPECS["liffirenet"]) == [1, 4]
    assert chainable_layers(SPECS["no_recurrent"]) == []
    assert chainable_layers(SPECS["adjacent_recurrent"]) == [2]     # layer 1's consumer is recurrent itself
    assert chainable_layers(SPECS["recurrent_last"]) == []          # its consumer is the top task
    assert chainable_layers([R, F, F]) == []                        # a recurrent head is not LIF-fed
    with pytest.raises(ValueError):
        chained_bwd_slots(3, SPECS["adjacent_recurrent"], [1])
    with pytest.raises(ValueError):
        chained_bwd_slots(3, SPECS["recurrent_last"], [6])


def test_launch_counts():
    L = 7
    for T in TS:
        legacy = len(wavefront_slots(T, L + 1))
        assert legacy == 2 * (T - 1) + L + 1
        # LIFFireNet: both loops chained -> one launch per step
        assert len(_check(T, SPECS["liffirenet"], [1, 4])) == T + L
        # no recurrent layer: the shorter schedule, no pairs
        la = _check(T, SPECS["no_recurrent"], [])
        assert len(la) == T + L and all(len(n) == 1 for launch in la for n in launch)
        # an unchained loop keeps two launches per step: today's count
        assert len(_check(T, SPECS["recurrent_last"], [])) == legacy
        assert len(_check(T, SPECS["liffirenet"], [])) == legacy
        assert len(_check(T, SPECS["liffirenet"], [4])) == legacy
        assert len(_check(T, SPECS["adjacent_recurrent"], chainable_layers(SPECS["adjacent_recurrent"]))) == legacy
    assert len(chained_bwd_slots(10, SPECS["liffirenet"], [1, 4])) == 17
    # steady state: top, B(6), pair(4, 5), B(3), pair(1, 2), head = eight layer-steps
    mid = chained_bwd_slots(10, SPECS["liffirenet"], [1, 4])[8]
    assert [tuple(k for k, _ in n) for n in mid] == [(7,), (6,), (4, 5), (3,), (1, 2), (0,)]


def test_task_cap_is_honoured():
    rec = [F] * 8  # eight layers: a launch of the uncapped wavefront would hold eight layer tasks
    launches = chained_bwd_slots(10, rec, [])
    assert max(sum(1 for n in la for k, _ in n if k < 8) for la in launches) <= _lib.MAX_CHAIN_TASKS
    _check(10, rec, [])


def _pair():
    """A well-formed chained pair as far as snnflow_bwd_chain's pair validation goes (fake pointers:
    nothing is launched by the calls below, every one is refused first)."""
    arr = (_lib.LayerBwdArgs * 3)()
    for a in arr:
        a.B, a.H, a.W, a.c, a.cin, a.lif_in = 1, 8, 32, 8, 8, 1
        a.wslab_ff = 0x1000
    r, f = arr[0], arr[1]
    r.wt_bwd_rec = r.wt_fwd_rec = r.wslab_rec = r.s_prev = 0x1000
    r.n.bn_weight = f.prev.bn_weight = 0x2000
    r.n.threshold = f.prev.threshold = 0x3000
    return arr


def _refused(arr, n, pair, what):
    flags = (ctypes.c_ubyte * len(pair))(*pair)
    rc = _lib.lib.snnflow_bwd_chain(arr, n, flags, None, None)
    msg = _lib.lib.snnflow_last_error()
    assert rc in (-1, -2) and b"bwd_chain" in msg and what in msg, (rc, msg)


def test_bwd_chain_refuses_malformed_pairs():
    lib = _lib.lib
    arr = _pair()
    assert lib.snnflow_bwd_chain(arr, 0, None, None, None) == -1                       # no task
    big = (_lib.LayerBwdArgs * (_lib.MAX_CHAIN_TASKS + 1))()
    assert lib.snnflow_bwd_chain(big, _lib.MAX_CHAIN_TASKS + 1, None, None, None) == -1
    assert b"task count" in lib.snnflow_last_error()
    _refused(arr, 1, [1], b"consecutive")                  # first half without a second
    _refused(arr, 3, [1, 1, 0], b"consecutive")            # overlapping pairs
    a = _pair(); a[1].c = a[1].cin = 16
    _refused(a, 2, [1, 0], b"c = cin = 8")
    a = _pair(); a[0].lif_in = 0
    _refused(a, 2, [1, 0], b"c = cin = 8")
    a = _pair(); a[1].H = 16
    _refused(a, 2, [1, 0], b"shapes")
    a = _pair(); a[0].wt_bwd_rec = None                    # first half not recurrent
    _refused(a, 2, [1, 0], b"recurrent")
    a = _pair(); a[1].wt_bwd_rec = 0x1000                  # second half recurrent
    _refused(a, 2, [1, 0], b"recurrent")
    a = _pair(); a[1].wslab_ff = None                      # second half without the fused weight gradients
    _refused(a, 2, [1, 0], b"fused weight gradients")
    a = _pair(); a[0].s_prev = None
    _refused(a, 2, [1, 0], b"fused weight gradients")
    a = _pair(); a[0].g_state_prev = 0x1000                # hand-over and a buffer at once
    _refused(a, 2, [1, 0], b"handed")
    a = _pair(); a[1].prev_g_state = 0x1000
    _refused(a, 2, [1, 0], b"handed")
    a = _pair(); a[1].prev.bn_weight = 0x4000              # second half's layer l-1 is another layer
    _refused(a, 2, [1, 0], b"handed")
    # the four-task limit of snnflow_bwd_slot stands beside the new entry point
    assert lib.snnflow_bwd_slot(big, 5, None, None) == -1
