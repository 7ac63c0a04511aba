"""Launch schedules of a truncated-BPTT window (engine.FireNetSequence): which (layer, step) tasks
share a launch.  Pure Python, no device work; the docstrings are the specification."""
from . import _lib


def wavefront_slots(T, K):
    """Launch order of a (kernel k < K, step t < T) grid whose task (k, t) reads the outputs of
    (k-1, t), (k, t-1) and (k+1, t-1) (the spikes of a recurrent layer come out of the next
    kernel of the previous step): task (k, t) runs in launch k + 2t, so every launch holds
    mutually independent tasks and follows all of its inputs' launches.
    Returns [[(k, t), ...] per launch]."""
    slots = [[] for _ in range(K + 2 * (T - 1))]
    for t in range(T):
        for k in range(K):
            slots[k + 2 * t].append((k, t))
    return slots


def chainable_layers(rec):
    """Recurrent layers r whose backward task (r, t+1) can run chained to task (r+1, t): r is LIF-fed
    (not the head), layer r+1 is a feed-forward layer below the top (its task consumes the gradient of
    r's spikes; for the last layer the top task does, and an adjacent recurrent layer r+1 would close a
    second loop through the same block)."""
    L = len(rec)
    return [r for r in range(1, L - 1) if rec[r] and not rec[r + 1]]


def _list_schedule(T, rec, chain, max_tasks, pair, task_deps, node_key, launch_key, error):
    """The list scheduler behind both chained schedules.  Tasks (k, t), k <= L (L: the top task), t < T.
    pair(r, t): the node of a chained layer r's tasks around step t >= 1, a tuple of two tasks;
    task_deps(k, t): the tasks (k, t) follows; node_key(n): order of the nodes within one longest-path
    level; launch_key(n): order of the nodes within one launch.  Returns [[node, ...] per launch]."""
    L = len(rec)
    chain = set(chain)
    if not all(1 <= r < L - 1 and rec[r] and not rec[r + 1] for r in chain):
        raise ValueError(error)
    node_of = {(k, t): ((k, t),) for k in range(L + 1) for t in range(T)}
    for r in chain:
        for t in range(1, T):
            node = pair(r, t)
            for task in node:
                node_of[task] = node

    def deps(node):
        return {node_of[d] for task in node for d in task_deps(*task) if d not in node}

    level = {}

    def lvl(node):  # longest path from a source (depth <= T + L nodes)
        if node not in level:
            level[node] = 1 + max((lvl(d) for d in deps(node)), default=-1)
        return level[node]

    nodes = sorted(set(node_of.values()), key=lambda n: (lvl(n), *node_key(n)))
    slot, fill, launches = {}, [], []
    for n in nodes:
        s = 1 + max((slot[d] for d in deps(n)), default=-1)
        nl = sum(1 for k, _ in n if k < L)
        while s < len(fill) and fill[s] + nl > max_tasks:
            s += 1
        while len(launches) <= s:
            launches.append([])
            fill.append(0)
        slot[n] = s
        fill[s] += nl
        launches[s].append(n)
    for la in launches:
        la.sort(key=launch_key)
    return launches


def chained_bwd_slots(T, rec, chain=(), max_tasks=_lib.MAX_CHAIN_TASKS):
    """Launches of the backward of a T-step window over layers 0..L-1 (rec[l]: recurrent); task (k, t)
    is the backward task of layer k at step t, (L, t) the top task.  Task (k, t) follows
      (k+1, t)    g_cur and the BatchNorm-backward sums of layer k,
      (k, t+1)    the same layer's later step (parameter gradients and slab rows are read-modify-write
                  in descending t, so one layer's tasks sit in distinct launches in that order),
      (k-1, t+1)  where layer k-1 is recurrent: the gradient of its spikes at step t.
    For r in `chain` the tasks (r, t+1) and (r+1, t) form one node, a chained pair run by one block per
    tile (snnflow_bwd_chain): the third dependency stays inside the node, so the loop around layer r
    costs one launch per step, not two.  A node goes into the launch after its latest dependency (its
    longest-path level: the same-layer order skews the steps into a wavefront, so the launches fill
    evenly), or the next one with room for its tasks (max_tasks layer tasks per launch).
    Returns [[node, ...] per launch], node = ((k, t),) or ((r, t+1), (r+1, t)), layers descending."""
    L = len(rec)

    def task_deps(k, t):
        if k < L:
            yield k + 1, t
        if t + 1 < T:
            yield k, t + 1
            if k >= 1 and rec[k - 1]:
                yield k - 1, t + 1

    return _list_schedule(
        T, rec, chain, max_tasks, lambda r, t: ((r, t), (r + 1, t - 1)), task_deps,
        node_key=lambda n: (-n[0][0], -n[0][1]), launch_key=lambda n: -n[0][0],
        error="chained_bwd_slots: a chained layer is recurrent, LIF-fed and followed by a feed-forward layer")


def chained_fwd_slots(T, rec, chain=(), max_tasks=_lib.MAX_CHAIN_TASKS):
    """Launches of the forward of a T-step window over layers 0..L-1 (rec[l]: recurrent); task (k, t)
    is the forward task of layer k at step t (the LIF of layer k-1 on the halo + the convs of layer k),
    (L, t) the top task.  Task (k, t) follows
      (k-1, t)    the pre-BN current of layer k-1 and its batch statistics,
      (k, t-1)    the same layer's earlier step (membrane of layer k-1, running statistics; kept for the
                  head too, so that the steps skew into an even wavefront),
      (k+1, t-1)  where layer k is recurrent: its spikes of step t-1, computed by the next layer's task.
    For r in `chain` the tasks (r+1, t-1) and (r, t) form one node, a chained pair run by one block per
    tile (snnflow_fwd_chain): the third dependency stays inside the node, so the loop around layer r
    costs one launch per step, not two.  Step 0's task of layer r and task (r+1, T-1) stay single.  A
    node goes into the launch after its latest dependency (its longest-path level), or the next one
    with room for its tasks (max_tasks conv tasks per launch).
    Returns [[node, ...] per launch], node = ((k, t),) or ((r+1, t-1), (r, t)), layers ascending."""
    L = len(rec)

    def task_deps(k, t):
        if k >= 1:
            yield k - 1, t
        if t >= 1:
            yield k, t - 1
            if k < L and rec[k]:
                yield k + 1, t - 1

    def lowest(n):
        return min(k for k, _ in n)

    return _list_schedule(
        T, rec, chain, max_tasks, lambda r, t: ((r + 1, t - 1), (r, t)), task_deps,
        node_key=lambda n: (lowest(n), n[0][1]), launch_key=lowest,
        error="chained_fwd_slots: a chained layer is recurrent, LIF-fed and followed by a feed-forward "
              "layer below the top")
