"""Every C-ABI launch of the LIFFireNet host engine over a fixed set of cases, in a canonical text form:
one line per snnflow._lib.call with the entry point's name and its arguments.  Two checkouts that
print the same trace hand the library the same arguments up to addresses -- the check of a host-side
refactor (profiles/r12/).

Canonical form: integer and float fields by value, pointer fields as P (non-NULL; NULL fields, zero
integers and zero floats are left out), nested structs and arrays recursively; positional c_void_p
arguments as P / 0, integers by value; the trailing stream argument is skipped.  A struct is written
out once, as @n{...} where it first occurs in the run, and as @n wherever the same text recurs (the
neuron structs and most tasks repeat across launches; the full text would be seven times as long).

Cases (fixed seeds; B=1 H=8 W=32, one tile, and B=2 H=40 W=72, partial tiles; T = 3):
  seq_c8_chain / seq_c8_nochain / seq_c16   a forward_sequence train window, forward + backward
  steps_defer / steps_nodefer               T model() calls + one backward()
  seq_c8_timer                              seq_c8_chain under a KernelTimer (the per-kernel branch)
  eval                                      eval_sequence
  seq_continue                              two windows, the second continuing from the first one's
                                            states, one backward (a chain that is not fresh, root false)

    python tools/launch_trace.py [out.txt]"""
import ctypes
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "snn_event-based_optical_flow_amd")]
import torch  # noqa: E402

import snnflow  # noqa: E402
from oracle import lif_ref  # noqa: E402
from snnflow import _lib  # noqa: E402

SHAPES = ((1, 8, 32), (2, 40, 72))
T = 3
LINES = []
STRUCTS = {}  # canonical text of a struct -> its number (first occurrence order over the whole run)
_INTS = (ctypes.c_int8, ctypes.c_uint8, ctypes.c_int16, ctypes.c_uint16, ctypes.c_int32, ctypes.c_uint32,
         ctypes.c_int64, ctypes.c_uint64)


def canon(v):
    """Canonical text of one ctypes value (struct, array, byref, simple) or Python scalar."""
    if hasattr(v, "_obj"):  # ctypes.byref(x)
        return canon(v._obj)
    if isinstance(v, ctypes.Structure):
        parts = []
        for name, typ in v._fields_:
            if typ is ctypes.c_void_p:
                txt = "P" if getattr(v, name) else ""
            else:
                txt = canon(getattr(v, name))
            if txt not in ("", "0", "0.0", "{}", "[]"):
                parts.append(f"{name}={txt}")
        if not parts:
            return "{}"
        txt = "{" + ",".join(parts) + "}"
        if txt in STRUCTS:  # printed before: its number stands for it
            return f"@{STRUCTS[txt]}"
        STRUCTS[txt] = len(STRUCTS)
        return f"@{STRUCTS[txt]}{txt}"
    if isinstance(v, ctypes.Array):
        if v._type_ is ctypes.c_void_p:
            items = ["P" if x else "0" for x in v]
        else:
            items = [canon(x) for x in v]
        while items and items[-1] in ("0", "0.0", "{}", "[]"):  # trailing zeros of a fixed-size array
            items.pop()
        return "[" + ",".join(items) + "]"
    if isinstance(v, ctypes.c_void_p):
        return "P" if v.value else "0"
    if isinstance(v, _INTS + (ctypes.c_float, ctypes.c_double)):
        return repr(v.value)
    if v is None:
        return "0"
    if isinstance(v, (bool, int, float)):
        return repr(v)
    raise TypeError(f"launch_trace: no canonical form for {type(v)}")


def traced_call(real):
    def call(name, fn, *args, work=None):
        types = fn.argtypes
        assert types is not None and len(types) == len(args), name
        n = len(args) - 1 if types[-1] is ctypes.c_void_p else len(args)  # the stream comes last
        out = []
        for a, t in zip(args[:n], types[:n]):
            if t is ctypes.c_void_p and (a is None or isinstance(a, int)):
                out.append("P" if a else "0")
            else:
                out.append(canon(a))
        LINES.append(f"{fn.__name__} {name} " + " ".join(out))
        return real(name, fn, *args, work=work)
    return call


def model_for(dev, C, seed=11):
    torch.manual_seed(seed)
    return snnflow.LIFFireNet(lif_ref.make_unet_kwargs(base_num_channels=C)).to(dev).train()


def inputs(dev, n, B, H, W, seed=3):
    gen = torch.Generator(device=dev).manual_seed(seed)
    xs = [(torch.rand(B, 2, H, W, generator=gen, device=dev) < 0.2).float() * 3 for _ in range(n)]
    wts = [torch.randn(B, 2, H, W, generator=gen, device=dev) for _ in range(n)]
    return xs, wts


def window(m, xs, wts):
    flows = [o["flow"][0] for o in m.forward_sequence(None, xs)]
    return sum((f * w).sum() for f, w in zip(flows, wts))


def case_seq(dev, shape, C, chain=True, timer=False):
    m = model_for(dev, C)
    m.engine.fwd_chain = m.engine.bwd_chain = chain
    xs, wts = inputs(dev, T, *shape)
    _lib.TIMER = _lib.KernelTimer() if timer else None
    try:
        window(m, xs, wts).backward()
    finally:
        _lib.TIMER = None


def case_steps(dev, shape, defer):
    m = model_for(dev, 8)
    m.engine.defer_backward = defer
    xs, wts = inputs(dev, T, *shape)
    flows = [m(None, x)["flow"][0] for x in xs]
    sum((f * w).sum() for f, w in zip(flows, wts)).backward()


def case_eval(dev, shape):
    m = model_for(dev, 8).eval()
    xs, _ = inputs(dev, T, *shape)
    with torch.no_grad():
        m.forward_sequence(None, xs)


def case_continue(dev, shape):
    m = model_for(dev, 8)
    xs, wts = inputs(dev, 2 * T, *shape)
    loss = window(m, xs[:T], wts[:T]) + window(m, xs[T:], wts[T:])  # (no detach in between)
    loss.backward()


CASES = (
    ("seq_c8_chain", lambda d, s: case_seq(d, s, 8, True)),
    ("seq_c8_nochain", lambda d, s: case_seq(d, s, 8, False)),
    ("seq_c16", lambda d, s: case_seq(d, s, 16)),
    ("steps_defer", lambda d, s: case_steps(d, s, True)),
    ("steps_nodefer", lambda d, s: case_steps(d, s, False)),
    ("seq_c8_timer", lambda d, s: case_seq(d, s, 8, True, timer=True)),
    ("eval", case_eval),
    ("seq_continue", case_continue),
)


def main(out=None):
    dev = torch.device("cuda:0")
    _lib.call = traced_call(_lib.call)
    for name, fn in CASES:
        for shape in SHAPES:
            LINES.append(f"# case {name} B={shape[0]} H={shape[1]} W={shape[2]}")
            n0 = len(LINES)
            fn(dev, shape)
            torch.cuda.synchronize()
            assert len(LINES) > n0, name
    text = "\n".join(LINES) + "\n"
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)
        print(f"{out}: {len(LINES)} lines, {len(text)} bytes")
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
