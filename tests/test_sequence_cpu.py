"""CPU-side checks of the sequence reader (no GPU compute): the numpy restatement
(tests/sequence_ref.py) reproduces the reference's H5Loader as recorded in
tests/golden/sequence_case.npz, the new C-ABI structs have the declared layout,
snnflow_seq_next validates its arguments before any device work, and the Python classes refuse
bad recordings on the host."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sequence_ref as sr  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "snnflow.h")


@pytest.fixture(scope="module")
def g(golden):
    return golden("sequence_case.npz")


@pytest.mark.parametrize("case", list(sr.CASES))
def test_restatement_reproduces_reference_bitwise(g, case):
    cfg, seqs, nmax, calls = sr.case_reader_args(g, case)
    ref = sr.RefSequenceReader(cfg, seqs, nmax)
    restarted = False
    for it, want in enumerate(sr.fixture_windows(g, case)):
        out = ref.next()
        sr.assert_window_equal(out, want, f"{case} call {it}", rows=ref.batch_row, idx=ref.batch_idx)
        assert (out["flow_idx"] == want["flow_idx"]).all(), (case, it)
        assert bool(out["restarts"].any()) == want["new_seq"], (case, it)
        restarted |= want["new_seq"]
    assert it == calls - 1 and restarted and ref.status == [0] * len(ref.status)


def test_chained_restatements_reproduce_the_reference_item_dicts(g):
    """Case L: RefSequenceReader -> RefPreparer, reset in slot order as often as a slot restarted."""
    import loader_ref

    cfg, seqs, _, calls = sr.case_reader_args(g, "L")
    ref = sr.RefLoader(cfg, seqs, sr.L_BINS)
    for it in range(calls):
        r = ref.next(g["L_flags"][it])
        for k in ("event_cnt", "event_mask", "event_list", "event_list_pol_mask"):
            loader_ref.assert_bit_equal(r[k], g[f"L_{k}"][it], f"L call {it} {k}")
        err = np.abs(r["event_voxel"].astype(np.float64) - g["L_event_voxel"][it])
        assert (err <= loader_ref.voxel_bound(r)).all(), (it, err.max())
        loader_ref.assert_bit_equal(ref.prep.hot_events, g["L_hot_events"][it], f"L call {it} hot_events")
        assert (ref.prep.hot_idx == g["L_hot_idx"][it]).all()
        assert (ref.rd.batch_row == g["L_rows"][it]).all() and (ref.rd.batch_idx == g["L_idx"][it]).all()


def test_fixture_holds_the_generated_sequences(g):
    """make_sequences() is what the fixture's recordings were made with (the GPU tests build their
    second seed with it)."""
    import zlib

    got = sr.sequences_from_fixture(g)
    assert set(got) == {"a", "s", "s90", "b", "c"}
    assert [len(got[n]["xs"]) for n in ("a", "s", "s90", "b", "c")] == [2600, 150, 90, 2530, 2540]
    for s in got.values():
        assert (np.diff(s["ts"]) >= 0).all() and s["xs"].max() < sr.W0 and s["ys"].max() < sr.H0
        assert s["flow_maps"].shape[1:] == (2, sr.H0, sr.W0)
    assert zlib.crc32(got["a"]["xs"].tobytes()) == zlib.crc32(sr.make_sequences(20240917)["a"]["xs"].tobytes())


def _layout(tmp_path, struct, py):
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
             f'printf("size %zu\\n", sizeof({struct}));']
    for fname, _ in py._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof({struct}, {fname}));')
    lines += ['printf("abi %d\\n", SNNFLOW_ABI_VERSION);',
              'printf("consts %d %d %d %d %d\\n", SNNFLOW_SEQ_EVENTS, SNNFLOW_SEQ_TIME, SNNFLOW_SEQ_GTFLOW, '
              'SNNFLOW_SEQ_OVERFLOW, SNNFLOW_SEQ_STUCK);',
              'printf("words %lld\\n", (long long)SNNFLOW_SEQ_SCRATCH_WORDS(3, 101));', "return 0;}"]
    c = tmp_path / f"{struct}.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / struct
    subprocess.run(["gcc", "-std=c11", str(c), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    return dict(line.split(" ", 1) for line in out if line)


@pytest.mark.parametrize("struct,cls", [("snnflow_seq_desc", "SeqDesc"), ("snnflow_seq_args", "SeqArgs")])
def test_seq_structs_layout_matches_c(tmp_path, struct, cls):
    from snnflow import _lib

    py = getattr(_lib, cls)
    got = _layout(tmp_path, struct, py)
    assert int(got["size"]) == ctypes.sizeof(py)
    for fname, _ in py._fields_:
        assert int(got[fname]) == getattr(py, fname).offset, fname
    assert int(got["abi"]) == 41 == _lib.ABI_VERSION == _lib.lib.snnflow_abi_version()
    assert got["consts"] == f"{_lib.SEQ_EVENTS} {_lib.SEQ_TIME} {_lib.SEQ_GTFLOW} {_lib.SEQ_OVERFLOW} {_lib.SEQ_STUCK}"
    assert int(got["words"]) == _lib.seq_scratch_words(3, 101)


def _valid_args(_lib):
    a = _lib.SeqArgs()
    a.B, a.N, a.mode, a.nseq, a.H0, a.W0, a.Hc, a.Wc, a.window = 3, 101, _lib.SEQ_EVENTS, 4, 20, 24, 12, 16, 101.0
    for f in ("seqs", "row", "batch_idx", "status", "scratch", "xs", "ys", "ts", "ps", "counts", "dt_input", "dt_gt",
              "restarts"):
        setattr(a, f, 64)
    a.scratch_words = _lib.seq_scratch_words(3, 101)
    return a


@pytest.mark.parametrize("field,value,message", [
    ("B", 0, b"B must"), ("N", 0, b"B must"), ("N", -5, b"B must"), ("mode", 3, b"mode"), ("mode", -1, b"mode"),
    ("nseq", 0, b"sequences"), ("window", 0.0, b"window"), ("window", -1.0, b"window"), ("window", float("nan"), b"window"),
    ("window", 100.5, b"whole number"), ("window", 102.0, b"whole number"),
    ("Hc", 21, b"crop"), ("Wc", 25, b"crop"), ("H0", 0, b"resolution"),
    ("seqs", None, b"NULL"), ("row", None, b"NULL"), ("batch_idx", None, b"NULL"), ("status", None, b"NULL"),
    ("scratch", None, b"NULL"), ("xs", None, b"NULL"), ("ys", None, b"NULL"), ("ts", None, b"NULL"),
    ("ps", None, b"NULL"), ("counts", None, b"NULL"), ("dt_input", None, b"NULL"), ("dt_gt", None, b"NULL"),
    ("restarts", None, b"NULL"), ("scratch_words", 100, b"scratch")])
def test_seq_next_validates_before_any_launch(field, value, message):
    """Every refusal comes back as -1 with a message and before any device work: the pointers of the
    otherwise valid argument block are not device memory, and no GPU is needed to get here."""
    from snnflow import _lib

    lib = _lib.lib
    assert "snnflow_seq_next" in _lib.EXPORTS
    a = _valid_args(_lib)
    setattr(a, field, value)
    assert lib.snnflow_seq_next(ctypes.byref(a), None) == -1
    err = lib.snnflow_last_error()
    assert b"seq_next" in err and message in err, err


def test_seq_next_refuses_null_args_and_gtflow_without_output():
    from snnflow import _lib

    lib = _lib.lib
    assert lib.snnflow_seq_next(None, None) == -1 and b"seq_next" in lib.snnflow_last_error()
    a = _valid_args(_lib)
    a.mode, a.window, a.Hc, a.Wc = _lib.SEQ_GTFLOW, 0.5, 20, 24
    assert lib.snnflow_seq_next(ctypes.byref(a), None) == -1 and b"NULL" in lib.snnflow_last_error()


def _arrays(n=50, xmax=sr.W0, ymax=sr.H0):
    rng = np.random.default_rng(0)
    return (rng.integers(0, xmax, n).astype(np.int16), rng.integers(0, ymax, n).astype(np.int16),
            np.sort(5.0 + rng.random(n)), rng.integers(0, 2, n).astype(np.uint8))


def test_event_sequence_validates_on_the_host():
    import snnflow

    xs, ys, ts, ps = _arrays()
    with pytest.raises(snnflow.SnnflowError, match="length"):
        snnflow.EventSequence(xs, ys[:-1], ts, ps, 5.0)
    with pytest.raises(snnflow.SnnflowError, match="0 or 1"):
        snnflow.EventSequence(xs, ys, ts, ps + 1, 5.0)
    with pytest.raises(snnflow.SnnflowError, match="int16"):
        snnflow.EventSequence(xs.astype(np.int64) - 1, ys, ts, ps, 5.0)
    with pytest.raises(snnflow.SnnflowError, match="int16"):
        snnflow.EventSequence(xs.astype(np.int64) + 40000, ys, ts, ps, 5.0)
    with pytest.raises(snnflow.SnnflowError, match="non-decreasing"):
        snnflow.EventSequence(xs, ys, ts[::-1], ps, 5.0)
    with pytest.raises(snnflow.SnnflowError, match="go together"):
        snnflow.EventSequence(xs, ys, ts, ps, 5.0, flow_ts=np.zeros(2))


def test_reader_refuses_out_of_frame_coordinates_and_frames_mode():
    """Checked on the host against std_resolution when the sequences are bound, before anything
    else: it raises with or without a device."""
    import torch

    import snnflow

    def seq(*a, **k):
        try:
            return snnflow.EventSequence(*a, **k)
        except snnflow.SnnflowError:
            raise
        except Exception as e:  # a visible but unusable device is not this test's subject
            pytest.skip(f"upload failed: {e}")

    cfg = sr.config("events", sr.WINDOW, (sr.H0, sr.W0), 1)
    for kw in ({"xmax": sr.W0 + 1}, {"ymax": sr.H0 + 1}):
        xs, ys, ts, ps = _arrays(400, **kw)
        xs[0], ys[0] = kw.get("xmax", 1) - 1, kw.get("ymax", 1) - 1
        with pytest.raises(snnflow.SnnflowError, match="outside std_resolution"):
            snnflow.SequenceReader(cfg, [seq(xs, ys, ts, ps, 5.0)])
    good = seq(*_arrays(400), 5.0)
    with pytest.raises(NotImplementedError):
        snnflow.SequenceReader(sr.config("frames", 1, (sr.H0, sr.W0), 1), [good])
    with pytest.raises(snnflow.SnnflowError, match="max_events"):
        snnflow.SequenceReader(sr.config("time", 0.1, (sr.H0, sr.W0), 1), [good])
    with pytest.raises(snnflow.SnnflowError, match="batch slots"):
        snnflow.SequenceReader(sr.config("events", sr.WINDOW, (sr.H0, sr.W0), 2), [good])
    with pytest.raises(snnflow.SnnflowError, match="larger than"):
        snnflow.SequenceReader(sr.config("events", sr.WINDOW, (sr.H0 + 2, sr.W0), 1), [good])
    if not torch.cuda.is_available():
        with pytest.raises(snnflow.SnnflowError, match="HIP device"):
            snnflow.SequenceReader(cfg, [good])


def test_from_npz_round_trip(tmp_path):
    import snnflow

    xs, ys, ts, ps = _arrays()
    path = tmp_path / "rec.npz"
    np.savez(path, xs=xs, ys=ys, ts=ts, ps=ps, t0=np.float64(5.0))
    s = snnflow.EventSequence.from_npz(str(path))
    assert len(s) == 50 and s.t0 == 5.0 and s.last_ts == ts[-1] and s.nflow == 0


def test_from_h5_without_h5py_raises_import_error(tmp_path):
    import snnflow

    try:
        import h5py  # noqa: F401
    except ImportError:
        pass
    else:
        pytest.skip("h5py is installed")
    with pytest.raises(ImportError, match="h5py"):
        snnflow.EventSequence.from_h5(str(tmp_path / "rec.h5"))
