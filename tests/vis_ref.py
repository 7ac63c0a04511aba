"""numpy restatement of the visual-evaluation path (test infrastructure): the frame renderers
snnflow.vis reproduces, the interpolation arithmetic of the percentile kernel, and the per-pixel
error maps in float32 (the kernels' expressions) and float64 (for the tolerances).

Images follow the reference's conventions: one image per call, flow components [H, W],
event counts [H, W, 2]."""
import numpy as np

F32 = np.float32


def assert_bit_equal(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert a.tobytes() == b.tobytes(), f"{what}: {int((a != b).sum())} of {a.size} values differ"


def percentile_model(x, q, fp64):
    """The select kernel's arithmetic on a sorted copy: virtual index, the two neighbours and the
    two-sided lerp, every step in float64 (x widened) or in float32.  Equals np.percentile(x64, q)
    / np.percentile(x32, q) bit for bit (tests/test_vis_cpu.py)."""
    s = np.sort(np.asarray(x, dtype=F32).ravel())
    n = s.size
    if fp64:
        s = s.astype(np.float64)
        vi = np.float64(n - 1) * (np.float64(q) / np.float64(100))
        one, half = np.float64(1), np.float64(0.5)
    else:
        vi = F32(n - 1) * (F32(q) / F32(100))
        one, half = F32(1), F32(0.5)
    lo = np.floor(vi)
    g = vi - lo
    if vi >= n - 1:
        a = b = s[n - 1]
    else:
        a, b = s[int(lo)], s[int(lo) + 1]
    d = b - a
    return b - d * (one - g) if g >= half else a + d * g


def hsv_to_rgb(h, s, v):
    """matplotlib's hsv_to_rgb on float64 planes."""
    h6 = h * 6.0
    i = h6.astype(int)
    f = h6 - i
    p = v * (1.0 - s)
    q = v * (1.0 - s * f)
    t = v * (1.0 - s * (1.0 - f))
    k = i % 6
    r = np.select([k == 0, k == 1, k == 2, k == 3, k == 4], [v, q, p, p, t], v)
    g = np.select([k == 0, k == 1, k == 2, k == 3, k == 4], [t, v, v, q, p], p)
    b = np.select([k == 0, k == 1, k == 2, k == 3, k == 4], [p, p, t, v, v], q)
    return np.stack([r, g, b], axis=-1)


def flow_to_image(flow_x, flow_y, uniform_v=None):
    """uint8 [H, W, 3] colour coding of a flow field: hue = direction (float32), value = magnitude
    between its 5th and 95th percentile under a square-root curve with a brightness floor (float64),
    true zeros black; a field of one magnitude is drawn at that brightness (times uniform_v)."""
    fx, fy = np.asarray(flow_x, dtype=F32), np.asarray(flow_y, dtype=F32)
    mag = np.sqrt(fx * fx + fy * fy).astype(np.float64)
    lo, hi = float(mag.min()), float(mag.max())
    hue = (np.arctan2(fy, fx) + F32(np.pi)) * F32(1.0 / np.pi / 2.0)
    assert hue.dtype == F32
    if hi - lo > 0.0:
        p5, p95 = float(np.percentile(mag, 5)), float(np.percentile(mag, 95))
        v = np.power(np.clip((mag - p5) / (p95 - p5 + 1e-8), 0.0, 1.0), 0.5)
        val = np.where(mag > 0, np.clip(v * 1.3 + 0.15, 0.15, 1.0), 0.0)
    elif hi > 0.0:
        v = mag / hi
        if uniform_v is not None:
            v = v * float(uniform_v)
        val = np.where(mag > 0, np.clip(np.power(v, 0.5) * 1.3 + 0.15, 0.15, 1.0), 0.0)
    else:
        val = np.zeros_like(mag)
    rgb = hsv_to_rgb(hue.astype(np.float64), np.ones_like(mag), val)
    return (255 * rgb).astype(np.uint8)


def events_to_image(event_cnt, color_scheme="green_red"):
    """float64 image of per-polarity counts [H, W, 2]: both planes scaled from their own 1st
    percentile to the larger 99th, clipped; (neg, pos, 0) or the gray mix 0.5 + 0.5 pos - 0.5 neg."""
    cnt = np.asarray(event_cnt, dtype=F32)
    pos, neg = cnt[:, :, 0], cnt[:, :, 1]
    p_lo, p_hi = np.percentile(pos, 1), np.percentile(pos, 99)
    n_lo, n_hi = np.percentile(neg, 1), np.percentile(neg, 99)
    top = p_hi if p_hi > n_hi else n_hi
    if p_lo != top:
        pos = (pos - p_lo) / (top - p_lo)
    if n_lo != top:
        neg = (neg - n_lo) / (top - n_lo)
    pos, neg = np.clip(pos, 0, 1), np.clip(neg, 0, 1)
    assert pos.dtype == F32 and neg.dtype == F32
    if color_scheme == "gray":
        return 0.5 + (pos * F32(0.5) + neg * F32(-0.5)).astype(np.float64)
    img = np.zeros(pos.shape + (3,))
    img[:, :, 0] = np.where(neg > 0, neg, 0)
    img[:, :, 1] = np.where(pos > 0, pos, 0)
    return img


def error_to_image(error_map):
    """uint8 [H, W, 3]: radians -> degrees / 180, clipped, in the red channel (sample 0 of a batch)."""
    e = np.asarray(error_map, dtype=F32)
    if e.ndim == 3:
        e = e[0]
    v = np.clip(np.degrees(e) / 180.0, 0.0, 1.0)
    assert v.dtype == F32
    img = np.zeros(e.shape + (3,), dtype=np.uint8)
    img[:, :, 0] = (v * 255).astype(np.uint8)
    return img


def minmax_norm(x):
    x = np.asarray(x, dtype=F32)
    den = np.percentile(x, 99) - np.percentile(x, 1)
    if den != 0:
        x = (x - np.percentile(x, 1)) / den
    return np.clip(x, 0, 1)


# ---- error maps ----
CLAMP_LO, CLAMP_HI = F32(-1.0) + F32(1e-5), F32(1.0) - F32(1e-5)
METRICS = ("AEE", "AAE", "NAAE")


def error_maps(flow, gt, event_mask, ratio, flow_scaling, metric, dtype=F32):
    """Unmasked per-pixel error [B, H, W] of the metric and the validity mask, in `dtype`; for AAE /
    NAAE also the clamped cosine and |flow'| (the tolerance of the acos is set by them)."""
    t = dtype
    f = (np.asarray(flow, dtype=F32).astype(t) * t(flow_scaling)) * np.asarray(ratio, dtype=F32).astype(t).reshape(-1, 1, 1, 1)
    g = np.asarray(gt, dtype=F32).astype(t)
    valid = (np.asarray(event_mask) != 0) & ~((g[:, 0] == 0) & (g[:, 1] == 0))
    if metric == "AEE":
        d = f - g
        return np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]), valid, None, None
    fn = np.sqrt(f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1])
    gn = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1])
    dot = f[:, 0] * g[:, 0] + f[:, 1] * g[:, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        c = (fn * gn) / (dot + t(0.01)) if metric == "AAE" else dot / (fn * gn + t(1e-9))
    c = np.clip(c, t(CLAMP_LO), t(CLAMP_HI))
    e = np.arccos(c)
    if metric == "NAAE":
        e = e / (fn + t(1e-9))
    return e, valid, c, fn


EPS32 = float(np.finfo(F32).eps)


def error_map_bound(ref, flow, gt, event_mask, ratio, flow_scaling, metric):
    """Per-pixel bound on |map - ref| (derivation: tests/test_gpu_vis.py).  AEE: one float32 ulp of
    the reference.  AAE / NAAE: 1e-5 |ref| + 8 eps32 (1 + 1/sqrt(max(1 - c^2, 2e-5))), the second term
    over (|flow'| + 1e-9) for NAAE, with the clamped cosine c recomputed in float64."""
    ref = np.asarray(ref, dtype=np.float64)
    if metric == "AEE":
        return np.spacing(np.abs(ref).astype(F32)).astype(np.float64)
    _, _, c, fn = error_maps(flow, gt, event_mask, ratio, flow_scaling, metric, dtype=np.float64)
    cond = 8.0 * EPS32 * (1.0 + 1.0 / np.sqrt(np.maximum(1.0 - c * c, 2e-5)))
    if metric == "NAAE":
        cond = cond / (fn + 1e-9)
    return 1e-5 * np.abs(ref) + cond
