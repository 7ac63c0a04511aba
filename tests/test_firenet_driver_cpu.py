"""The host-side step driver (csrc/firenet_step.hip) against recorded argument bytes, without a GPU.

tests/firenet_driver.cpp links the driver's object against recording stubs of the launch functions
and calls snnflow_firenet_fwd / _bwd / _bwd_seq / _wgrad with synthetic plans.  Everything is built
with the host address and undefined-behaviour sanitizers (a plain executable).  Every argument struct
the stubs receive must match tests/golden/firenet_driver_case.npz byte for byte, and so must every
call's return code; the golden file was recorded before the argument builders of the two backward
drivers were merged.  Regenerate (only when the driver's launches are meant to change):

    python tests/test_firenet_driver_cpu.py
"""
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "snn_event-based_optical_flow_amd", "csrc")
GOLDEN = os.path.join(REPO, "tests", "golden", "firenet_driver_case.npz")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN = "-fsanitize=address,undefined"


def run_driver(tmp):
    """Builds and runs the program in directory `tmp`; returns (log bytes, return codes)."""
    tmp = str(tmp)
    inc = ["-I" + os.path.join(REPO, "include"), "-I" + CSRC]
    obj, stub, exe, log = (os.path.join(tmp, n) for n in ("firenet_step.o", "driver.o", "driver", "log.bin"))
    subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-Xarch_host", SAN,
                    "-fno-sanitize-recover=undefined", *inc, "-c", os.path.join(CSRC, "firenet_step.hip"), "-o", obj],
                   check=True)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", SAN, "-fno-sanitize-recover=undefined", *inc, "-c",
                    os.path.join(REPO, "tests", "firenet_driver.cpp"), "-o", stub], check=True)
    # (the sanitizer runtimes linked statically: the executable then carries them itself)
    subprocess.run(["g++", SAN, "-static-libasan", "-static-libubsan", stub, obj, "-o", exe], check=True)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    r = subprocess.run([exe, log], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), f"driver exit {r.returncode}\n{r.stderr[-4000:]}"
    rcs = np.array([int(v) for v in r.stdout.split()], dtype=np.int32)
    return np.fromfile(log, dtype=np.uint8), rcs


def _records(log):
    """[(tag, payload bytes)] of a log."""
    out, i, raw = [], 0, log.tobytes()
    while i < len(raw):
        n = int.from_bytes(raw[i + 4:i + 8], "little")
        out.append((raw[i:i + 4].decode(), raw[i + 8:i + 8 + n]))
        i += 8 + n
    return out


def test_driver_arguments_match_the_recorded_bytes(tmp_path):
    log, rcs = run_driver(tmp_path)
    gold = np.load(GOLDEN, allow_pickle=False)
    assert len(rcs) == len(gold["rc"]) and (rcs != 0).sum() >= 4 and (rcs == 0).sum() > 100
    np.testing.assert_array_equal(rcs, gold["rc"])
    if not np.array_equal(log, gold["log"]):  # name the first differing record
        case = None
        for k, (a, b) in enumerate(zip(_records(log), _records(gold["log"]))):
            if a[0] == "CASE":
                case = int.from_bytes(a[1], "little")
            assert a == b, f"record {k} ({a[0]} / recorded {b[0]}) of driver call {case} differs"
        raise AssertionError(f"log lengths differ: {len(log)} / recorded {len(gold['log'])}")


if __name__ == "__main__":
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        log, rcs = run_driver(d)
    np.savez_compressed(GOLDEN, log=log, rc=rcs)
    print(f"{GOLDEN}: {os.path.getsize(GOLDEN)} bytes, {len(log)} log bytes, {len(rcs)} calls, "
          f"{int((rcs != 0).sum())} refused", file=sys.stderr)
