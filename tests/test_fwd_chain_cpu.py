"""The chained forward schedule (snnflow.engine.chained_fwd_slots) and the validation of
snnflow_fwd_chain, without a GPU.

A schedule is checked against the dependencies of the forward tasks written out here on their own
(not taken from the scheduler): task (k, t) -- layer k at step t, k = L the top task -- follows
(k-1, t), (k, t-1) and, where layer k is recurrent, (k+1, t-1)."""
import ctypes

import pytest

from snnflow import _lib
from snnflow.engine import chainable_layers, chained_fwd_slots, wavefront_slots

F, R = False, True
SPECS = {
    "no_recurrent": [F, F, F, F, F, F, F],          # LIFFireFlowNet
    "liffirenet": [F, R, F, F, R, F, F],            # head, G1, R1a, R1b, G2, R2a, R2b
    "adjacent_recurrent": [F, R, R, F, F, F, F],
    "recurrent_last": [F, F, F, F, F, F, R],
}
TS = (1, 2, 3, 10)


def _deps(k, t, rec):
    L = len(rec)
    d = []
    if k >= 1:
        d.append((k - 1, t))
    if t >= 1:
        d.append((k, t - 1))
        if k < L and rec[k]:
            d.append((k + 1, t - 1))
    return d


def _check(T, rec, chain, **kw):
    L = len(rec)
    cap = kw.get("max_tasks", _lib.MAX_CHAIN_TASKS)
    launches = chained_fwd_slots(T, rec, chain, **kw)
    where, node_of = {}, {}
    for i, la in enumerate(launches):
        assert la, "empty launch"
        assert sum(1 for n in la for k, _ in n if k < L) <= cap
        assert sum(1 for n in la for k, _ in n if k == L) <= 1  # one top task per launch
        for n in la:
            assert len(n) in (1, 2)
            if len(n) == 2:  # (feed-forward (r+1, t-1), recurrent (r, t)), r chained
                (k1, t1), (r, t) = n
                assert r in chain and k1 == r + 1 and t1 == t - 1 and rec[r] and not rec[r + 1] and 1 <= r < L - 1
            for task in n:
                assert task not in where, task
                where[task] = i
                node_of[task] = n
    assert sorted(where) == [(k, t) for k in range(L + 1) for t in range(T)]  # every task once
    for (k, t), i in where.items():
        for dep in _deps(k, t, rec):
            if node_of[dep] is node_of[(k, t)]:
                # the only dependency a pair keeps inside: the spikes handed from (r+1, t-1) to (r, t)
                assert dep == (k + 1, t - 1) and node_of[dep] == (dep, (k, t))
            else:
                assert where[dep] < i, (T, rec, (k, t), dep)
    for k in range(L + 1):  # one layer's tasks: distinct launches, ascending t
        order = [where[(k, t)] for t in range(T)]
        assert all(a < b for a, b in zip(order, order[1:])), (k, order)
    for r in chain:  # every step that can be chained is; step 0 of r and (r+1, T-1) stay single
        for t in range(1, T):
            assert node_of[(r, t)] == ((r + 1, t - 1), (r, t))
        assert node_of[(r, 0)] == ((r, 0),) and node_of[(r + 1, T - 1)] == ((r + 1, T - 1),)
    return launches


@pytest.mark.parametrize("name", sorted(SPECS))
@pytest.mark.parametrize("T", TS)
def test_schedule_respects_dependencies(name, T):
    rec = SPECS[name]
    _check(T, rec, chainable_layers(rec))
    _check(T, rec, [])


def test_ineligible_chain_entries_raise():
    for rec, r in ((SPECS["adjacent_recurrent"], 1),   # its spikes come from a recurrent layer's task
                   (SPECS["recurrent_last"], 6),       # its spikes come from the top task
                   (SPECS["liffirenet"], 2),           # not recurrent
                   ([R, F, F], 0),                     # a recurrent head is not LIF-fed
                   (SPECS["liffirenet"], 7)):          # no such layer
        with pytest.raises(ValueError):
            chained_fwd_slots(3, rec, [r])


def test_launch_counts():
    L = 7
    for T in TS:
        legacy = len(wavefront_slots(T, L + 1))
        assert legacy == 2 * (T - 1) + L + 1
        # LIFFireNet: both loops chained -> one launch per step, 2 (T - 1) pairs
        la = _check(T, SPECS["liffirenet"], [1, 4])
        assert len(la) == T + L and sum(len(n) == 2 for launch in la for n in launch) == 2 * (T - 1)
        # no recurrent layer: the shorter schedule, no pairs
        la = _check(T, SPECS["no_recurrent"], [])
        assert len(la) == T + L and all(len(n) == 1 for launch in la for n in launch)
        # an unchained loop keeps two launches per step: today's count
        assert len(_check(T, SPECS["liffirenet"], [])) == legacy
        assert len(_check(T, SPECS["recurrent_last"], [])) == legacy
        assert len(_check(T, SPECS["liffirenet"], [4])) == legacy
        assert len(_check(T, SPECS["adjacent_recurrent"], chainable_layers(SPECS["adjacent_recurrent"]))) == legacy
    # T = 1 with chain=(): today's launches, task for task
    assert [[n[0] for n in la] for la in chained_fwd_slots(1, SPECS["liffirenet"], [])] == wavefront_slots(1, L + 1)
    assert len(chained_fwd_slots(10, SPECS["liffirenet"], [1, 4])) == 17
    # steady state: head, pair(2, 1), F(3), pair(5, 4), F(6), top = eight tasks, the steps skewed by one
    mid = chained_fwd_slots(10, SPECS["liffirenet"], [1, 4])[8]
    assert [tuple(k for k, _ in n) for n in mid] == [(0,), (2, 1), (3,), (5, 4), (6,), (7,)]
    assert sorted(t for n in mid for _, t in n) == [1, 2, 3, 4, 5, 6, 7, 8]


def test_task_cap_is_honoured():
    rec = [F] * 8  # eight layers: a launch of the uncapped wavefront would hold eight conv tasks
    launches = chained_fwd_slots(10, rec, [])
    assert max(sum(1 for n in la for k, _ in n if k < 8) for la in launches) <= _lib.MAX_CHAIN_TASKS
    _check(10, rec, [])
    _check(10, SPECS["liffirenet"], [1, 4], max_tasks=4)  # pairs never split over the cap


def _pair():
    """A well-formed chained pair as far as snnflow_fwd_chain's pair validation goes (fake pointers:
    nothing is launched by the calls below, every one is refused first)."""
    arr = (_lib.ConvFwdArgs * 3)()
    for i, a in enumerate(arr):
        a.B, a.H, a.W, a.c, a.cin, a.lif_in = 1, 8, 32, 8, 8, 1
        a.wt_ff = a.wt_ff_t = 0x1000
        a.prev_y, a.prev_state, a.y = 0x10000 * (i + 1), 0x10000 * (i + 1) + 0x100, 0x10000 * (i + 1) + 0x200
    arr[1].wt_rec = arr[1].wt_rec_t = 0x2000
    return arr


def _refused(arr, n, pair, what):
    flags = (ctypes.c_ubyte * len(pair))(*pair)
    rc = _lib.lib.snnflow_fwd_chain(arr, n, flags, None, None)
    msg = _lib.lib.snnflow_last_error()
    assert rc in (-1, -2) and b"fwd_chain" in msg and what in msg, (rc, msg)


def test_fwd_chain_refuses_malformed_pairs():
    lib = _lib.lib
    arr = _pair()
    assert lib.snnflow_fwd_chain(arr, 0, None, None, None) == -1                       # no task
    big = (_lib.ConvFwdArgs * (_lib.MAX_CHAIN_TASKS + 1))()
    assert lib.snnflow_fwd_chain(big, _lib.MAX_CHAIN_TASKS + 1, None, None, None) == -1
    assert b"task count" in lib.snnflow_last_error()
    _refused(arr, 1, [1], b"consecutive")                  # first half without a second
    _refused(arr, 3, [1, 1, 0], b"consecutive")            # overlapping pairs
    a = _pair(); a[1].c = a[1].cin = 16
    _refused(a, 2, [1, 0], b"c = cin = 8")
    a = _pair(); a[0].lif_in = 0
    _refused(a, 2, [1, 0], b"c = cin = 8")
    a = _pair(); a[1].H = 16
    _refused(a, 2, [1, 0], b"shapes")
    a = _pair(); a[0].wt_rec = a[0].wt_rec_t = 0x2000      # first half recurrent
    _refused(a, 2, [1, 0], b"recurrent")
    a = _pair(); a[1].wt_rec = a[1].wt_rec_t = None        # second half feed-forward
    _refused(a, 2, [1, 0], b"recurrent")
    a = _pair(); a[0].prev_spk_bits = 0x3000               # spike bit planes: not the tile pipeline
    _refused(a, 2, [1, 0], b"tile pipeline")
    a = _pair(); a[0].B = a[1].B = 1 << 20; a[0].H = a[1].H = 64   # 2^31 bytes: past the pipeline's offsets
    _refused(a, 2, [1, 0], b"tile pipeline")
    a = _pair(); a[1].s_prev = 0x4000                      # hand-over and a buffer at once
    _refused(a, 2, [1, 0], b"handed")
    a = _pair(); a[0].prev_state = a[1].prev_state         # the first half's LIF is not of the second's own layer
    _refused(a, 2, [1, 0], b"one step earlier")
    # the four-task limit of snnflow_fwd_slot stands beside the new entry point
    assert lib.snnflow_fwd_slot(big, 5, None, None) == -1
