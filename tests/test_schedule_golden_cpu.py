"""The window schedulers against launch lists recorded before they moved into snnflow/schedule.py
(tests/golden/schedules.json.gz, written by tests/golden/make_golden_schedules.py): every case must
give the recorded launches exactly, in order.  Without a GPU."""
import gzip
import importlib.util
import json
import os

from snnflow import engine, schedule

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load():
    with gzip.open(os.path.join(GOLDEN, "schedules.json.gz"), "rb") as f:
        return json.loads(f.read().decode())


def _maker():
    spec = importlib.util.spec_from_file_location("make_golden_schedules",
                                                  os.path.join(GOLDEN, "make_golden_schedules.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_engine_reexports_the_schedulers():
    for name in ("wavefront_slots", "chainable_layers", "chained_fwd_slots", "chained_bwd_slots"):
        assert getattr(engine, name) is getattr(schedule, name), name


def test_chained_schedules_match_the_recorded_launches():
    mk = _maker()
    gold = _load()["chained"]
    cases = list(mk.chained_cases(schedule.chainable_layers))
    assert len(cases) == len(gold) == 4284  # a forward and a backward schedule each: 8,568 launch lists
    for (T, rec, chain, mt), g in zip(cases, gold):
        case = f"T={T} rec={g['rec']} chain={g['chain']} max_tasks={mt}"
        # the fixture's own case list is the recorded one, in the recorded order
        assert (T, "".join("1" if r else "0" for r in rec), list(chain), mt) == \
            (g["T"], g["rec"], g["chain"], g["max_tasks"]), case
        fwd = mk.as_lists(schedule.chained_fwd_slots(T, list(rec), chain, mt))
        assert fwd == g["fwd"], f"chained_fwd_slots differs first at {case}"
        bwd = mk.as_lists(schedule.chained_bwd_slots(T, list(rec), chain, mt))
        assert bwd == g["bwd"], f"chained_bwd_slots differs first at {case}"


def test_wavefront_slots_match_the_recorded_launches():
    mk = _maker()
    gold = _load()["wavefront"]
    assert [(g["T"], g["K"]) for g in gold] == [(T, K) for T in mk.WAVEFRONT_T for K in mk.WAVEFRONT_K]
    for g in gold:
        got = mk.as_lists(schedule.wavefront_slots(g["T"], g["K"]))
        assert got == g["slots"], f"wavefront_slots differs first at T={g['T']} K={g['K']}"
