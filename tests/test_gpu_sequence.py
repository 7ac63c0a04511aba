"""On-device sequence reading (snnflow.SequenceReader / SequenceLoader -> snnflow_seq_next) against
the reference H5Loader's recorded windows (tests/golden/sequence_case.npz) and the numpy
restatement (tests/sequence_ref.py).  Nothing is toleranced: window selection is integer, float64
or single-rounding arithmetic in a fixed order.  The one exception is the loader's event_voxel,
whose sums follow the atomic arrival order of the batch preparation and are held to its existing
bound (loader_ref.voxel_bound)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loader_ref  # noqa: E402
import sequence_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

SECOND_SEED = 77


@pytest.fixture(scope="module")
def g(golden):
    return golden("sequence_case.npz")


@pytest.fixture(scope="module")
def second():
    return sr.make_sequences(SECOND_SEED, dyadic=False)


def upload(seqs, dev):
    import snnflow

    return [snnflow.EventSequence(s["xs"], s["ys"], s["ts"], s["ps"], s["t0"], s["duration"], s["flow_ts"],
                                  s["flow_maps"], device=dev) for s in seqs]


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("case", list(sr.CASES))
def test_reader_equals_fixture_bitwise(g, dev, case):
    import snnflow

    cfg, seqs, nmax, calls = sr.case_reader_args(g, case)
    rd = snnflow.SequenceReader(cfg, upload(seqs, dev), max_events=nmax, device=dev)
    assert rd.batch_idx == list(range(cfg["loader"]["batch_size"])) and not any(rd.batch_row)
    for it, want in enumerate(sr.fixture_windows(g, case)):
        out = host(rd.next())
        sr.assert_window_equal(out, want, f"{case} call {it}", rows=rd.batch_row, idx=rd.batch_idx)
        if "gtflow" in out:
            for b, f in enumerate(want["flow_idx"]):
                s = seqs[want["idx"][b] % len(seqs)]
                assert np.array_equal(out["gtflow"][b], s["flow_maps"][f]), (case, it, b)
        else:
            assert case[0] != "G"
    assert it == calls - 1
    rd.check()  # a clean run: no overflow, no stuck slot
    assert not rd.status.any()


@pytest.mark.parametrize("case", list(sr.CASES))
def test_reader_equals_restatement_on_a_second_seed(second, dev, case):
    """Generic float64 timestamps and t0: the rounding of ts - t0 and of the row sums is exercised."""
    import snnflow

    cfg, seqs, nmax, calls = sr.case_reader_args(second, case)
    rd = snnflow.SequenceReader(cfg, upload(seqs, dev), max_events=nmax, device=dev)
    ref = sr.RefSequenceReader(cfg, seqs, nmax)
    restarts = 0
    for it in range(calls + 4):
        out, want = host(rd.next()), ref.next()
        want["rows"], want["idx"] = ref.batch_row, ref.batch_idx
        sr.assert_window_equal(out, want, f"{case} call {it}", rows=rd.batch_row, idx=rd.batch_idx)
        if "gtflow" in want:
            assert np.array_equal(out["gtflow"], want["gtflow"]), (case, it)
        restarts += int(want["restarts"].sum())
    assert restarts > 0 and ref.status == [0] * ref.B
    rd.check()


def test_overflow_delivers_the_first_events_and_raises(g, dev):
    import snnflow

    cfg, seqs, _, _ = sr.case_reader_args(g, "T")
    most = int(g["T_counts"].max())
    nmax = 64
    assert most > nmax
    rd = snnflow.SequenceReader(cfg, upload(seqs, dev), max_events=nmax, device=dev)
    ref = sr.RefSequenceReader(cfg, seqs, nmax)
    for it in range(3):
        out, want = host(rd.next()), ref.next()
        sr.assert_window_equal(out, want, f"overflow call {it}")
    assert (out["counts"] == nmax).any() and any(s & 1 for s in ref.status)
    assert rd.status.cpu().tolist() == ref.status
    with pytest.raises(snnflow.SnnflowError, match="max_events"):
        rd.check()
    rd.check()  # the bits were cleared


def test_no_usable_sequence_is_reported_not_looped_on(g, dev):
    """Every sequence is shorter than a window: the reference would restart forever."""
    import snnflow

    seqs = sr.sequences_from_fixture(g)
    cfg = sr.config("events", sr.WINDOW, (sr.H0, sr.W0), 2)
    rd = snnflow.SequenceReader(cfg, upload([seqs["s90"], seqs["a"], seqs["s90"], seqs["a"]], dev), device=dev)
    out = host(rd.next())       # slot 0: s90 -> index 2 = s90 -> index 3 = a: usable after two restarts of four
    assert out["restarts"].tolist() == [2, 0] and out["counts"].tolist() == [sr.WINDOW, sr.WINDOW]
    assert rd.batch_idx == [3, 1]
    rd.check()
    rd = snnflow.SequenceReader(cfg, upload([seqs["s90"], seqs["s90"]], dev), device=dev)
    out = host(rd.next())
    assert out["restarts"].tolist() == [2, 2] and out["counts"].tolist() == [0, 0] and not out["xs"].any()
    with pytest.raises(snnflow.SnnflowError, match="without finding"):
        rd.check()


def _loader(cfg, seqs, dev, prefetch, seed=sr.L_SEED, bins=sr.L_BINS):
    import snnflow

    np.random.seed(seed)
    return snnflow.SequenceLoader(cfg, upload(seqs, dev), bins, prefetch=prefetch, device=dev)


def _flags(ld, B):
    return np.array([[bool(ld.batch_augmentation.get(m, [False] * B)[b]) for m in sr.MECH] for b in range(B)])


def check_voxel_bound(got, want, r, what):
    """got and want sum the same fp32 terms in two orders: loader_ref.voxel_bound (K, S from r)."""
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bound = loader_ref.voxel_bound(r)
    print(f"{what}: max voxel error {err.max():.3e}, smallest slack {np.min(bound - err):.3e}")
    assert (err <= bound).all(), (what, float(err.max()))


@pytest.mark.parametrize("prefetch", [False, True])
def test_loader_equals_the_reference_item_dicts(g, dev, prefetch):
    cfg, seqs, _, calls = sr.case_reader_args(g, "L")
    B = cfg["loader"]["batch_size"]
    ld = _loader(cfg, seqs, dev, prefetch)
    assert (_flags(ld, B) == g["L_flags0"]).all()
    ref = sr.RefLoader(cfg, seqs, sr.L_BINS)
    seq_num = 0
    for it in range(calls):
        out = host(next(ld))
        r = ref.next(g["L_flags"][it])
        assert (_flags(ld, B) == g["L_flags"][it]).all(), it   # the reference's flags after every restart
        for k in ("event_cnt", "event_mask", "event_list", "event_list_pol_mask"):
            loader_ref.assert_bit_equal(out[k], g[f"L_{k}"][it], f"L call {it} {k}")
        for k in ("dt_input", "dt_gt"):
            assert out[k].dtype == np.float64 and np.array_equal(out[k], g[f"L_{k}"][it]), (it, k)
        check_voxel_bound(out["event_voxel"], g["L_event_voxel"][it], r, f"L call {it}")
        loader_ref.assert_bit_equal(ld.prep.hot_events.cpu().numpy(), g["L_hot_events"][it], f"L call {it} hot_events")
        assert (ld.prep.hot_idx.cpu().numpy() == g["L_hot_idx"][it]).all(), it
        seq_num += int(g["L_restarts"][it].sum())
        assert ld.seq_num == seq_num and ld.new_seq == (seq_num > 0)
    torch.cuda.synchronize(dev)
    if not prefetch:  # with prefetch the reader already stands one window further
        assert ld.batch_row == g["L_rows"][-1].tolist() and ld.batch_idx == g["L_idx"][-1].tolist()
    ld.reader.check()


@pytest.mark.parametrize("case", ["L", "E"])
def test_prefetch_changes_nothing(g, dev, case):
    """Both paths over the whole case give identical tensors; event_voxel, whose sums follow the atomic
    arrival order of the batch preparation in either path, is held to that order's bound."""
    cfg, seqs, _, calls = sr.case_reader_args(g, case)
    bins = sr.L_BINS
    loaders, states = [], []   # the loaders draw from the global np.random: each gets a stream of its own
    for prefetch in (False, True):
        loaders.append(_loader(cfg, seqs, dev, prefetch))
        states.append(np.random.get_state())

    def step(i):
        np.random.set_state(states[i])
        out = host(next(loaders[i]))
        states[i] = np.random.get_state()
        return out

    a, b = loaders
    ref = sr.RefLoader(cfg, seqs, bins)
    B = a.reader.batch_size
    for it in range(calls):
        x, y = step(0), step(1)
        assert set(x) == set(y) and (_flags(a, B) == _flags(b, B)).all()
        flags = _flags(a, B) if cfg["loader"]["augment"] else np.zeros((B, 3), bool)
        r = ref.next(flags)
        for k in x:
            if k == "event_voxel":
                check_voxel_bound(x[k], y[k], r, f"{case} call {it}")
            else:
                assert np.array_equal(x[k], y[k]), (case, it, k)
        assert a.seq_num == b.seq_num and a.new_seq == b.new_seq
    assert a.seq_num > 0
    assert torch.equal(a.prep.hot_events, b.prep.hot_events) if a.prep.hot_enabled else a.prep.hot_events is None


@pytest.mark.parametrize("case", ["Ec", "T", "G04"])
def test_graph_capture_matches_eager(g, dev, case):
    """next() captured once and replayed k times (state carried on the device, the completion counter
    left at zero by every call) cuts the same windows as k eager calls of a twin."""
    import snnflow

    cfg, seqs, nmax, calls = sr.case_reader_args(g, case)
    up = upload(seqs, dev)
    rd = snnflow.SequenceReader(cfg, up, max_events=nmax, device=dev)
    twin = snnflow.SequenceReader(cfg, up, max_events=nmax, device=dev)
    bufs = rd.buffers()
    snnflow.SequenceReader(cfg, up, max_events=nmax, device=dev).next()   # the kernels are loaded before the capture
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rd.next(bufs)
    torch.cuda.synchronize(dev)
    assert not any(rd.batch_row), "capture must not run the kernels"
    for it, want in enumerate(sr.fixture_windows(g, case)):
        graph.replay()
        eager = twin.next()
        torch.cuda.synchronize(dev)
        for k in eager:
            assert torch.equal(bufs[k], eager[k]), (case, it, k)
        sr.assert_window_equal(host(bufs), want, f"{case} replay {it}", rows=rd.batch_row, idx=rd.batch_idx)
    rd.check()


def test_long_sequences_three_search_rounds(dev):
    """70 000 events: the k-ary search takes three rounds (256 probes each), with timestamps on a
    coarse grid so that the probes land inside long runs of equal values."""
    import snnflow

    rng = np.random.default_rng(5)
    seqs = []
    for n, t0 in ((70000, 12.5), (66000, 3.25), (70001, 100.0)):
        ts = t0 + np.sort(rng.integers(0, 5000, n)) / 4096.0
        seqs.append(dict(xs=rng.integers(0, sr.W0, n).astype(np.int16), ys=rng.integers(0, sr.H0, n).astype(np.int16),
                         ts=ts, ps=rng.integers(0, 2, n).astype(np.uint8), t0=t0, duration=5000 / 4096.0,
                         flow_ts=None, flow_maps=None))
    cfg = sr.config("time", 0.125, (sr.H0, sr.W0), 2)
    rd = snnflow.SequenceReader(cfg, upload(seqs, dev), max_events=8192, device=dev)
    ref = sr.RefSequenceReader(cfg, seqs, 8192)
    restarts = 0
    for it in range(13):
        out, want = host(rd.next()), ref.next()
        want["rows"], want["idx"] = ref.batch_row, ref.batch_idx
        sr.assert_window_equal(out, want, f"long call {it}", rows=rd.batch_row, idx=rd.batch_idx)
        restarts += int(want["restarts"].sum())
    assert restarts >= 2 and int(want["counts"].max()) > 5000 and ref.status == [0, 0]
    rd.check()
