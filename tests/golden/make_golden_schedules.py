"""Writes tests/golden/schedules.json.gz: the full launch lists of the window schedulers
(snnflow.engine.chained_fwd_slots / chained_bwd_slots / wavefront_slots) over a fixed set of cases.

The file was generated once, before the schedulers moved into snnflow/schedule.py, and pins them:
tests/test_schedule_golden_cpu.py compares today's launch lists with it case by case.  Regenerate
only when a schedule is meant to change:

    python tests/golden/make_golden_schedules.py
"""
import gzip
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "schedules.json.gz")

LAYERS = range(1, 7)
STEPS = (1, 2, 3, 4, 5, 10)
MAX_TASKS = (2, 4, 7)
WAVEFRONT_T = range(1, 11)
WAVEFRONT_K = range(1, 9)


def chained_cases(chainable_layers):
    """(T, rec, chain, max_tasks) of every chained case, in the file's order."""
    for L in LAYERS:
        for rec in itertools.product((False, True), repeat=L):
            able = chainable_layers(list(rec))
            for n in range(len(able) + 1):
                for chain in itertools.combinations(able, n):
                    for T in STEPS:
                        for mt in MAX_TASKS:
                            yield T, rec, chain, mt


def as_lists(launches):
    """Launch lists as JSON stores them (tuples become lists)."""
    return json.loads(json.dumps(launches))


def build(engine):
    chained = []
    for T, rec, chain, mt in chained_cases(engine.chainable_layers):
        chained.append({"T": T, "rec": "".join("1" if r else "0" for r in rec), "chain": list(chain), "max_tasks": mt,
                        "fwd": engine.chained_fwd_slots(T, list(rec), chain, mt),
                        "bwd": engine.chained_bwd_slots(T, list(rec), chain, mt)})
    wave = [{"T": T, "K": K, "slots": engine.wavefront_slots(T, K)} for T in WAVEFRONT_T for K in WAVEFRONT_K]
    return {"chained": chained, "wavefront": wave}


def main():
    for p in (REPO, os.path.join(REPO, "snn_event-based_optical_flow_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from snnflow import engine
    data = json.dumps(build(engine), separators=(",", ":")).encode()
    with open(OUT, "wb") as f:
        with gzip.GzipFile(fileobj=f, mode="wb", mtime=0, compresslevel=9) as g:
            g.write(data)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
