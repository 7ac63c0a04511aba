// On-device batch preparation for gfx950: the loader stages between "raw events of a window"
// and the dict the train / evaluation loop consumes (reference dataloader/h5.py:285-333 and
// 373-437, dataloader/base.py:71-127, 144-159, 237-256, dataloader/encodings.py:88-103),
// batched over the slots of a batch.  Up to five kernels, all on one stream, no host round trip:
//   k_loader_minmax    per-slot partial min/max of the timestamps (one block per 2048 events)
//                      and the zeroing of the scatter targets
//   k_loader_events    one thread per event: format, flip, list + polarity mask, scatter
//   k_loader_hot_update  one thread per pixel: hot-pixel state update, candidate list
//   k_loader_hot_select  one block per slot: the ordered top-max_px selection among the candidates
//                      (radix select on the fp32 rate bits, then on the pixel index among ties)
//   k_loader_finalize  hot-mask multiply, row-major average pool, ground-truth flow flip / pool
// Counts, masks, lists, hot state and gtflow are exact; voxel sums follow the atomic arrival
// order (as k_encode's do).
#include <cmath>

#include "snnflow_dev.h"
#include "snnflow_host.h"

using namespace snnflow;

namespace {

constexpr int LCHUNK = 2048;  // events per min/max block (8 per thread)
constexpr int HNT = 1024;     // threads of the hot-pixel block (one block per slot)

struct Layout {  // offsets (floats) into the caller's scratch
    int nchunk;
    int64_t part, fcnt, fvox, fmask, hotmask, cand_n, cand_bits, cand_px, total;
};

inline Layout layout(int B, int N, int H0, int W0, int Ht, int Wt, int bins, int hot, int keep) {
    Layout l;
    const int64_t hw = (int64_t)B * H0 * W0;
    const bool pooled = Ht < H0 || Wt < W0;
    l.nchunk = N > 0 ? (N + LCHUNK - 1) / LCHUNK : 1;
    int64_t o = 0;
    l.part = o; o += ((int64_t)2 * B * l.nchunk + 3) / 4 * 4;
    l.fcnt = l.fvox = l.fmask = l.hotmask = l.cand_n = l.cand_bits = l.cand_px = -1;
    if (pooled) {
        l.fcnt = o; o += 2 * hw;
        l.fvox = o; o += (int64_t)bins * hw;
        if (!keep) { l.fmask = o; o += hw; }
    }
    if (hot) {  // the mask and the candidate lists (32-bit words in the float scratch)
        l.hotmask = o; o += hw;
        l.cand_bits = o; o += hw;
        l.cand_px = o; o += hw;
        l.cand_n = o; o += ((int64_t)B + 3) / 4 * 4;
    }
    l.total = o;
    return l;
}

struct ZeroList { float* p[4]; int64_t n[4]; };

__device__ inline int slot_count(const snnflow_loader_args& a, int b) {
    if (!a.counts) return a.N;
    const int c = a.counts[b];
    return c < 0 ? 0 : (c > a.N ? a.N : c);
}

// (a) partial min/max of slot blockIdx.y's valid timestamps in chunk blockIdx.x -> part[b][chunk][2]
// (an empty chunk leaves (+inf, -inf); a NaN makes both NaN, as torch's min / max propagate it);
// every block also zeroes its share of the scatter targets.
__global__ __launch_bounds__(NT) void k_loader_minmax(snnflow_loader_args a, float* part, int nchunk, ZeroList z) {
    const int64_t nb = (int64_t)gridDim.x * gridDim.y, id = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    for (int r = 0; r < 4; ++r)
        if (z.p[r])
            for (int64_t i = id * NT + threadIdx.x; i < z.n[r]; i += nb * NT) z.p[r][i] = 0.0f;
    if ((int)blockIdx.x >= nchunk) return;
    __shared__ float s_mn[NT / 64], s_mx[NT / 64];
    __shared__ int s_nan[NT / 64];
    const int b = blockIdx.y, cnt = slot_count(a, b);
    const float* ts = a.ts + (int64_t)b * a.N;
    float mn = INFINITY, mx = -INFINITY;
    int nan = 0;
    for (int k = 0; k < LCHUNK / NT; ++k) {
        const int i = blockIdx.x * LCHUNK + k * NT + threadIdx.x;
        if (i < cnt) {
            const float t = ts[i];
            nan |= (t != t);
            mn = fminf(mn, t);
            mx = fmaxf(mx, t);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        nan |= __shfl_xor(nan, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        s_mn[threadIdx.x >> 6] = mn;
        s_mx[threadIdx.x >> 6] = mx;
        s_nan[threadIdx.x >> 6] = nan;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < NT / 64; ++w) {
            mn = fminf(mn, s_mn[w]);
            mx = fmaxf(mx, s_mx[w]);
            nan |= s_nan[w];
        }
        float* o = part + ((int64_t)b * nchunk + blockIdx.x) * 2;
        o[0] = nan ? NAN : mn;
        o[1] = nan ? NAN : mx;
    }
}

// (b) one thread per event of slot blockIdx.y: event_formatting (base.py:85-99), augment_events
// (base.py:113-127), the list (scaled and clamped when pooled, h5.py:402-409) and polarity mask,
// and the full-resolution scatter of counts, mask and voxel (k_encode's definitions).
__global__ __launch_bounds__(NT) void k_loader_events(snnflow_loader_args a, const float* part, int nchunk, int pooled,
                                                      float* fcnt, float* fvox, float* fmask) {
    const int b = blockIdx.y, i = blockIdx.x * NT + threadIdx.x;
    if (i >= a.N) return;
    const int64_t e = (int64_t)b * a.N + i;
    float4* lst = reinterpret_cast<float4*>(a.event_list) + e;
    float2* pm = reinterpret_cast<float2*>(a.pol_mask) + e;
    if (i >= slot_count(a, b)) {  // padding
        *lst = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        *pm = make_float2(0.0f, 0.0f);
        return;
    }
    float mn = INFINITY, mx = -INFINITY;
    bool nan = false;
    for (int c = 0; c < nchunk; ++c) {
        const float m0 = part[((int64_t)b * nchunk + c) * 2], m1 = part[((int64_t)b * nchunk + c) * 2 + 1];
        nan |= (m0 != m0);
        mn = fminf(mn, m0);
        mx = fmaxf(mx, m1);
    }
    const float range = nan ? NAN : mx - mn;
    const float t = range > 0.0f ? (a.ts[e] - mn) / range : 0.0f;
    float p = a.ps[e] * 2.0f - 1.0f, x = a.xs[e], y = a.ys[e];
    const int fl = a.flags ? a.flags[b] : 0;
    if (fl & SNNFLOW_AUG_H) x = (float)(a.W0 - 1) - x;
    if (fl & SNNFLOW_AUG_V) y = (float)(a.H0 - 1) - y;
    if (fl & SNNFLOW_AUG_P) p = p * -1.0f;
    float ly = y, lx = x;
    if (pooled) {
        ly = fminf(fmaxf(y * a.scale_y, 0.0f), (float)(a.Ht - 1));
        lx = fminf(fmaxf(x * a.scale_x, 0.0f), (float)(a.Wt - 1));
    }
    *lst = make_float4(t, ly, lx, p);
    *pm = make_float2(p < 0.0f ? 0.0f : p, (p > 0.0f ? 0.0f : p) * -1.0f);
    const int64_t yi = (int64_t)y, xi = (int64_t)x;  // .long(): truncation toward zero
    if (yi < 0 || yi >= a.H0 || xi < 0 || xi >= a.W0) return;
    const int64_t HWp = (int64_t)a.H0 * a.W0, pix = yi * a.W0 + xi;
    float* c = fcnt + (int64_t)b * 2 * HWp + pix;
    const float pos = p * (p < 0.0f ? 0.0f : p), neg = p * (p > 0.0f ? 0.0f : p);
    if (pos != 0.0f) atomicAdd(c, pos);
    if (neg != 0.0f) atomicAdd(c + HWp, neg);
    fmask[(int64_t)b * HWp + pix] = fabsf(p);
    float tb = t * (float)(a.num_bins - 1);
    if (a.round_ts) tb = rintf(tb);  // torch.round: half to even
    float* v = fvox + (int64_t)b * a.num_bins * HWp + pix;
    for (int k = 0; k < a.num_bins; ++k) {
        const float w = fmaxf(0.0f, 1.0f - fabsf(tb - (float)k));
        if (w != 0.0f) atomicAdd(v + k * HWp, p * w);
    }
}

// (c1) one thread per pixel of slot blockIdx.y: create_hot_mask's state update (base.py:245-249)
// and the candidates of get_hot_event_mask (encodings.py:93-103), the pixels with rate > max_rate
// once hot_idx > min_obvs.  The mask is written as if every candidate were removed (true whenever
// there are at most max_px of them); the candidates' (rate bits, pixel) pairs are appended to the
// slot's list, one atomic per wave, for k_loader_hot_select to choose among.  hot_idx is only read
// here; k_loader_hot_select advances it.
__global__ __launch_bounds__(NT) void k_loader_hot_update(snnflow_loader_args a, const float* fcnt, float* hotmask,
                                                          unsigned* cand_n, unsigned* cand_bits, int* cand_px) {
    const int b = blockIdx.y, px = blockIdx.x * NT + threadIdx.x, lane = threadIdx.x & 63;
    const int HWp = a.H0 * a.W0;
    const bool valid = px < HWp;
    const int idx = a.hot_idx[b] + 1;
    const bool active = idx > a.hot_min_obvs && a.hot_max_px > 0;
    bool cand = false;
    float r = 0.0f;
    if (valid) {
        float* he = a.hot_events + (int64_t)b * HWp + px;
        const float* c = fcnt + (int64_t)b * 2 * HWp + px;
        const float h = *he + ((c[0] + c[HWp]) > 0.0f ? 1.0f : 0.0f);
        *he = h;
        r = h / (float)idx;
        cand = active && r > a.hot_max_rate;
        hotmask[(int64_t)b * HWp + px] = cand ? 0.0f : 1.0f;
    }
    const unsigned long long m = __ballot(cand);
    if (m == 0) return;  // wave-uniform
    const int leader = __ffsll((long long)m) - 1;
    unsigned base = 0;
    if (lane == leader) base = atomicAdd(&cand_n[b], (unsigned)__popcll(m));
    base = __shfl(base, leader, 64);
    if (cand) {
        const unsigned at = base + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
        cand_bits[(int64_t)b * HWp + at] = __float_as_uint(r);
        cand_px[(int64_t)b * HWp + at] = px;
    }
}

// The k-th key (k >= 1) in descending (DESC) or ascending order among the n list entries that
// key(i, kv) accepts: four 8-bit radix passes over LDS histograms, most significant digit first;
// the bin holding the k-th key is found by one wave (4 bins per lane, suffix sums by shuffles).
// Returns the key; sel[1] = how many entries equal to it are still inside the first k, sel[2] =
// how many entries equal it.  All HNT threads call it; at least k entries must be accepted.
template <bool DESC, class KeyFn>
__device__ inline unsigned radix_select(int n, unsigned k, KeyFn key, unsigned* hist, unsigned* sel) {
    const int tid = threadIdx.x;
    unsigned prefix = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        const unsigned hi = shift == 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
        for (int i = tid; i < n; i += HNT) {
            unsigned kv;
            if (key(i, kv) && (kv & hi) == prefix) {
                const unsigned dig = (kv >> shift) & 255u;
                atomicAdd(&hist[DESC ? dig : 255u - dig], 1u);  // bin 255 = first in the order
            }
        }
        __syncthreads();
        if (tid < 64) {
            const unsigned h0 = hist[4 * tid], h1 = hist[4 * tid + 1], h2 = hist[4 * tid + 2], h3 = hist[4 * tid + 3];
            const unsigned s = h0 + h1 + h2 + h3;
            unsigned incl = s;  // this lane's bins and every bin above them
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned u = __shfl_down(incl, o, 64);
                if (tid + o < 64) incl += u;
            }
            unsigned above = incl - s;
            if (above < k && k <= incl) {  // exactly one lane
                const unsigned h[4] = {h0, h1, h2, h3};
                int j = 3;
                for (; j > 0; --j) {
                    if (above + h[j] >= k) break;
                    above += h[j];
                }
                const unsigned bin = 4u * tid + j;
                sel[0] = DESC ? bin : 255u - bin;
                sel[1] = k - above;
                sel[2] = h[j];
            }
        }
        __syncthreads();
        prefix |= sel[0] << shift;
        k = sel[1];
    }
    return prefix;
}

// (c2) one block per slot: get_hot_event_mask's max_px sequential argmax rounds (encodings.py:95-102)
// as a selection.  The rounds remove the candidates in order of decreasing rate, lowest flat index
// first among equal rates (argmax returns the first maximum), and stop after max_px: the max_px
// largest (rate, -index) pairs.  Rates are positive, so their fp32 bit patterns order like the
// values: a descending radix select finds the cut rate T and how many pixels of rate T are still
// removed; if not all of them are, an ascending radix select on the pixel index among them finds
// the last index removed.  Every other candidate gets its mask value back.
__global__ __launch_bounds__(HNT) void k_loader_hot_select(snnflow_loader_args a, float* hotmask, const unsigned* cand_n,
                                                           const unsigned* cand_bits, const int* cand_px) {
    __shared__ unsigned hist[256];
    __shared__ unsigned sel[3];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int HWp = a.H0 * a.W0;
    if (tid == 0) a.hot_idx[b] += 1;
    const unsigned nc = cand_n[b];
    const int n = nc < (unsigned)HWp ? (int)nc : HWp;
    if (n <= a.hot_max_px) return;  // every candidate is removed (block-uniform)
    const unsigned* bits = cand_bits + (int64_t)b * HWp;
    const int* pxs = cand_px + (int64_t)b * HWp;
    float* hm = hotmask + (int64_t)b * HWp;
    const unsigned T = radix_select<true>(n, (unsigned)a.hot_max_px,
                                          [&](int i, unsigned& kv) { kv = bits[i]; return true; }, hist, sel);
    const unsigned k_eq = sel[1], n_eq = sel[2];
    unsigned last = 0xFFFFFFFFu;  // highest pixel index of rate T that is removed
    if (k_eq < n_eq)
        last = radix_select<false>(n, k_eq, [&](int i, unsigned& kv) { kv = (unsigned)pxs[i]; return bits[i] == T; },
                                   hist, sel);
    for (int i = tid; i < n; i += HNT) {
        const unsigned v = bits[i];
        const bool take = v > T || (v == T && (unsigned)pxs[i] <= last);
        if (!take) hm[pxs[i]] = 1.0f;
    }
}

// Row-major fp32 sum of one pool window of src (times the hot mask, when given), then the
// division by the window size: F.avg_pool2d(kernel = stride = (ph, pw)), h5.py:390-399.
__device__ inline float pool_window(const float* src, const float* hm, int W0, int y0, int x0, int ph, int pw) {
    float s = 0.0f;
    for (int dy = 0; dy < ph; ++dy)
        for (int dx = 0; dx < pw; ++dx) {
            const int px = (y0 + dy) * W0 + x0 + dx;
            float v = src[px];
            if (hm) v = v * hm[px];
            s += v;
        }
    return s / (float)(ph * pw);
}

// augment_flowmap (base.py:151-158) at output pixel (y, x) of component ch.
__device__ inline float flow_at(const float* g, int ch, int y, int x, int H0, int W0, int fl) {
    const int sy = (fl & SNNFLOW_AUG_V) ? H0 - 1 - y : y, sx = (fl & SNNFLOW_AUG_H) ? W0 - 1 - x : x;
    float v = g[((int64_t)ch * H0 + sy) * W0 + sx];
    if ((fl & SNNFLOW_AUG_H) && ch == 0) v = v * -1.0f;
    if ((fl & SNNFLOW_AUG_V) && ch == 1) v = v * -1.0f;
    return v;
}

// (d) items [0, n_pool): one pooled output pixel each (all its channels); items [n_pool,
// n_pool + n_full): one full-resolution pixel each -- the in-place hot-mask multiply of what
// stays at full resolution (h5.py:327-333) and the flipped copy of the ground-truth flow.
__global__ __launch_bounds__(NT) void k_loader_finalize(snnflow_loader_args a, int pooled, const float* fcnt,
                                                        const float* fvox, float* fmask, const float* hotmask,
                                                        int64_t n_pool, int64_t n_full) {
    const int HWp = a.H0 * a.W0, HWt = a.Ht * a.Wt;
    const int ph = a.H0 / a.Ht, pw = a.W0 / a.Wt;
    for (int64_t it = (int64_t)blockIdx.x * NT + threadIdx.x; it < n_pool + n_full; it += (int64_t)gridDim.x * NT) {
        if (it < n_pool) {
            const int b = (int)(it / HWt), o = (int)(it - (int64_t)b * HWt);
            const int y0 = (o / a.Wt) * ph, x0 = (o % a.Wt) * pw;
            const float* hm = hotmask ? hotmask + (int64_t)b * HWp : nullptr;
            for (int ch = 0; ch < 2; ++ch)
                a.event_cnt[((int64_t)b * 2 + ch) * HWt + o] =
                    pool_window(fcnt + ((int64_t)b * 2 + ch) * HWp, hm, a.W0, y0, x0, ph, pw);
            for (int ch = 0; ch < a.num_bins; ++ch)
                a.event_voxel[((int64_t)b * a.num_bins + ch) * HWt + o] =
                    pool_window(fvox + ((int64_t)b * a.num_bins + ch) * HWp, hm, a.W0, y0, x0, ph, pw);
            if (a.keep_gt_full_res) continue;
            a.event_mask[(int64_t)b * HWt + o] = pool_window(fmask + (int64_t)b * HWp, hm, a.W0, y0, x0, ph, pw);
            if (a.gtflow) {
                const int fl = a.flags ? a.flags[b] : 0;
                const float* g = a.gtflow_in + (int64_t)b * 2 * HWp;
                for (int ch = 0; ch < 2; ++ch) {
                    float s = 0.0f;
                    for (int dy = 0; dy < ph; ++dy)
                        for (int dx = 0; dx < pw; ++dx) s += flow_at(g, ch, y0 + dy, x0 + dx, a.H0, a.W0, fl);
                    a.gtflow[((int64_t)b * 2 + ch) * HWt + o] = s / (float)(ph * pw);
                }
            }
        } else {
            const int64_t f = it - n_pool;
            const int b = (int)(f / HWp), px = (int)(f - (int64_t)b * HWp);
            if (hotmask) {
                const float m = hotmask[(int64_t)b * HWp + px];
                if (!pooled) {
                    for (int ch = 0; ch < 2; ++ch) a.event_cnt[((int64_t)b * 2 + ch) * HWp + px] *= m;
                    for (int ch = 0; ch < a.num_bins; ++ch)
                        a.event_voxel[((int64_t)b * a.num_bins + ch) * HWp + px] *= m;
                }
                fmask[(int64_t)b * HWp + px] *= m;
            }
            if (a.gtflow) {
                const int fl = a.flags ? a.flags[b] : 0;
                const float* g = a.gtflow_in + (int64_t)b * 2 * HWp;
                for (int ch = 0; ch < 2; ++ch)
                    a.gtflow[((int64_t)b * 2 + ch) * HWp + px] = flow_at(g, ch, px / a.W0, px % a.W0, a.H0, a.W0, fl);
            }
        }
    }
}

}  // namespace

extern "C" int64_t snnflow_loader_scratch_floats(int B, int N, int H0, int W0, int Ht, int Wt, int num_bins,
                                                 int hot_enabled, int keep_gt_full_res) {
    if (B <= 0 || N < 0 || H0 <= 0 || W0 <= 0 || Ht <= 0 || Wt <= 0 || num_bins < 1)
        SNN_FAIL(SNNFLOW_E_ARG, "loader_scratch_floats: bad args");
    return layout(B, N, H0, W0, Ht, Wt, num_bins, hot_enabled, keep_gt_full_res).total;
}

extern "C" int snnflow_loader_prepare(const snnflow_loader_args* a, void* stream) {
    if (!a || a->B <= 0 || a->B > 65535 || a->N < 0 || a->H0 <= 0 || a->W0 <= 0 || a->Ht <= 0 || a->Wt <= 0 ||
        a->num_bins < 1 || !a->event_cnt || !a->event_voxel || !a->event_mask || !a->scratch ||
        (a->N > 0 && (!a->xs || !a->ys || !a->ts || !a->ps || !a->event_list || !a->pol_mask)))
        SNN_FAIL(SNNFLOW_E_ARG, "loader_prepare: bad args");
    if (a->Ht > a->H0 || a->Wt > a->W0 || a->H0 % a->Ht || a->W0 % a->Wt)
        SNN_FAIL(SNNFLOW_E_ARG, "loader_prepare: the target resolution must divide the full resolution");
    if ((int64_t)a->H0 * a->W0 > (1 << 30) || (int64_t)a->B * a->N > (int64_t)1 << 40)
        SNN_FAIL(SNNFLOW_E_ARG, "loader_prepare: shape too large");
    if (((uintptr_t)a->event_list & 15) || ((uintptr_t)a->pol_mask & 7))
        SNN_FAIL(SNNFLOW_E_ARG, "loader_prepare: event_list must be 16-byte and pol_mask 8-byte aligned");
    if (a->hot_enabled && (!a->hot_events || !a->hot_idx || a->hot_max_px < 0))
        SNN_FAIL(SNNFLOW_E_ARG, "loader_prepare: hot filter without state or with a negative max_px");
    if ((a->gtflow_in == nullptr) != (a->gtflow == nullptr))
        SNN_FAIL(SNNFLOW_E_ARG, "loader_prepare: gtflow_in and gtflow go together");
    const hipStream_t s = (hipStream_t)stream;
    const bool pooled = a->Ht < a->H0 || a->Wt < a->W0;
    const bool keep = pooled && a->keep_gt_full_res;
    snnflow_loader_args q = *a;
    q.keep_gt_full_res = keep ? 1 : 0;
    const Layout l = layout(q.B, q.N, q.H0, q.W0, q.Ht, q.Wt, q.num_bins, q.hot_enabled, q.keep_gt_full_res);
    const int64_t hw = (int64_t)q.B * q.H0 * q.W0;
    float* part = q.scratch + l.part;
    float* fcnt = pooled ? q.scratch + l.fcnt : q.event_cnt;
    float* fvox = pooled ? q.scratch + l.fvox : q.event_voxel;
    float* fmask = (pooled && !keep) ? q.scratch + l.fmask : q.event_mask;
    float* hotmask = q.hot_enabled ? q.scratch + l.hotmask : nullptr;

    ZeroList z;
    z.p[0] = fcnt; z.n[0] = 2 * hw;
    z.p[1] = fvox; z.n[1] = (int64_t)q.num_bins * hw;
    z.p[2] = fmask; z.n[2] = hw;
    z.p[3] = q.hot_enabled ? q.scratch + l.cand_n : nullptr; z.n[3] = q.B;  // candidate counters (0.0f = 0u)
    int64_t gz = ((2 + q.num_bins + 1) * hw / q.B + NT * 16 - 1) / (NT * 16);
    if (gz > 256) gz = 256;
    const unsigned gx = (unsigned)(gz > l.nchunk ? gz : l.nchunk);
    hipLaunchKernelGGL(k_loader_minmax, dim3(gx, (unsigned)q.B), dim3(NT), 0, s, q, part, l.nchunk, z);
    SNN_CHECK_LAUNCH();
    if (q.N > 0) {
        hipLaunchKernelGGL(k_loader_events, dim3((unsigned)((q.N + NT - 1) / NT), (unsigned)q.B), dim3(NT), 0, s, q,
                           (const float*)part, l.nchunk, pooled ? 1 : 0, fcnt, fvox, fmask);
        SNN_CHECK_LAUNCH();
    }
    if (q.hot_enabled) {
        unsigned* cand_n = reinterpret_cast<unsigned*>(q.scratch + l.cand_n);
        unsigned* cand_bits = reinterpret_cast<unsigned*>(q.scratch + l.cand_bits);
        int* cand_px = reinterpret_cast<int*>(q.scratch + l.cand_px);
        const unsigned gp = (unsigned)(((int64_t)q.H0 * q.W0 + NT - 1) / NT);
        hipLaunchKernelGGL(k_loader_hot_update, dim3(gp, (unsigned)q.B), dim3(NT), 0, s, q, (const float*)fcnt, hotmask,
                           cand_n, cand_bits, cand_px);
        SNN_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_loader_hot_select, dim3((unsigned)q.B), dim3(HNT), 0, s, q, hotmask,
                           (const unsigned*)cand_n, (const unsigned*)cand_bits, (const int*)cand_px);
        SNN_CHECK_LAUNCH();
    }
    const int64_t n_pool = pooled ? (int64_t)q.B * q.Ht * q.Wt : 0;
    const int64_t n_full = ((!pooled && (q.hot_enabled || q.gtflow)) || (keep && (q.hot_enabled || q.gtflow))) ? hw : 0;
    if (n_pool + n_full > 0) {
        int64_t g = (n_pool + n_full + NT - 1) / NT;
        if (g > 8192) g = 8192;
        hipLaunchKernelGGL(k_loader_finalize, dim3((unsigned)g), dim3(NT), 0, s, q, pooled ? 1 : 0, (const float*)fcnt,
                           (const float*)fvox, fmask, (const float*)hotmask, n_pool, n_full);
        SNN_CHECK_LAUNCH();
    }
    return 0;
}
