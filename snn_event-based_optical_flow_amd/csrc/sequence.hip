// On-device sequence reading for gfx950: the file side of the reference's H5Loader
// (dataloader/h5.py:47-70, 138-283, 350-365, 449-545; dataloader/encodings.py:9-27) over
// recordings resident in device memory.  Two kernels on one stream, no host round trip:
//   k_seq_select  one block per batch slot: the slot's window bounds in its mode (or the
//                 centre-crop search), the restart test and the row advance.  Restarts depend on
//                 each other in slot order (h5.py:259: max(batch_idx) + 1), so the last block to
//                 finish (completion counter, as k_aee's) walks the restarting slots in order and
//                 repeats the selection on their new sequences, as often as a slot needs.
//   k_seq_gather  one thread per output event: int16 / float64 / uint8 -> the fp32 [B][N] rows
//                 snnflow_loader_prepare reads (zero tails), dt_input, and the slot's flow map.
// Everything is integer, float64 or one rounding to fp32 in the reference's order
// (-ffp-contract=off keeps `idx0 + change * delta` a multiply and an add): bit-reproducible.
#include <cmath>

#include "snnflow_dev.h"
#include "snnflow_host.h"

using namespace snnflow;

namespace {

constexpr int kFewEvents = 10;   // h5.py:248: a window of at most 10 events is delivered empty
constexpr int kNW = NT / 64;

struct Scratch {  // views into snnflow_seq_args::scratch (int64 words)
    unsigned long long* done;   // [1] completion counter, left at zero by every call
    int64_t* i0;                // [B] first event of the window (plain ranges)
    int64_t* cnt;               // [B] events of the window before the cut to N; -1 = restart pending
    int64_t* flow;              // [B] flow map delivered, -1 = none
    int64_t* idx;               // [B][N] event indices of a crop window
};

__host__ __device__ inline Scratch scratch_of(const snnflow_seq_args& a) {
    Scratch s;
    s.done = reinterpret_cast<unsigned long long*>(a.scratch);
    s.i0 = a.scratch + 2;
    s.cnt = s.i0 + a.B;
    s.flow = s.cnt + a.B;
    s.idx = s.flow + a.B;
    return s;
}

// Exclusive prefix of `f` over the block's threads (ballot + popcount per wave, wave totals
// through LDS) and the block total.  Every thread calls it; `total` is block-uniform.
__device__ inline int block_scan(bool f, int* s_w, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long m = __ballot(f);
    if (lane == 0) s_w[w] = __popcll(m);
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < kNW; ++k) {
        const int c = s_w[k];
        if (k < w) before += c;
        total += c;
    }
    __syncthreads();
    return before + __popcll(m & ((1ull << lane) - 1ull));
}

// First index of the sorted a[0, n) with a >= x (STRICT: a > x), n if none: a block-wide k-ary
// search, NT probes a round (three rounds cover 16 M events), every round one independent
// load per thread instead of a chain of dependent ones.  Block-uniform result.
template <bool STRICT>
__device__ inline int64_t block_bound(const double* __restrict__ a, int64_t n, double x, int* s_w) {
    int64_t lo = 0, hi = n;  // the answer lies in [lo, hi]
    while (lo < hi) {
        const int64_t step = (hi - lo + NT - 1) / NT;
        const int64_t q = lo + (int64_t)threadIdx.x * step;
        bool below = false;
        if (q < hi) {
            const double v = a[q];
            below = STRICT ? (v <= x) : (v < x);
        }
        int c;
        block_scan(below, s_w, c);  // sorted: the probes below x are the first c
        if (c == 0) {
            hi = lo;
        } else {
            const int64_t nhi = lo + (int64_t)c * step;
            lo = lo + (int64_t)(c - 1) * step + 1;
            hi = nhi < hi ? nhi : hi;
        }
    }
    return lo;
}

// binary_search_array (encodings.py:9-27) replayed without memory: the recursion returns the
// first probe that hits an equal timestamp (not the leftmost one), else the insertion point.
// With L = first a >= x and U = first a > x:  a[mid] == x <=> L <= mid < U,  x < a[mid] <=> mid >= U.
__device__ inline int64_t ref_bisect(int64_t n, int64_t L, int64_t U) {
    int64_t left = 0, right = n - 1;
    while (left <= right) {                              // :18
        const int64_t mid = left + (right - left) / 2;  // :16
        if (mid >= L && mid < U) return mid;             // :21
        if (mid >= U) right = mid - 1;                   // :24
        else left = mid + 1;                             // :27
    }
    return left;
}

__device__ inline int64_t find_ts_index(const snnflow_seq_desc& d, double x, int* s_w) {  // h5.py:177-182
    const int64_t L = block_bound<false>(d.ts, d.n, x, s_w);
    const int64_t U = block_bound<true>(d.ts, d.n, x, s_w);
    return ref_bisect(d.n, L, U);
}

// One bound of a Python slice a[i:j] over n elements.
__device__ inline int64_t slice_bound(int64_t i, int64_t n) {
    if (i < 0) {
        i += n;
        if (i < 0) i = 0;
    }
    return i > n ? n : i;
}

struct Window {
    int64_t i0, cnt, flow;
    double dt_gt, row;   // row: where the slot stands after a delivered window
    bool restart;
};

// One pass of H5Loader.__getitem__'s loop body (h5.py:186-263, 350-365) for slot b on sequence d
// at `row`.  Every thread of the block calls it; the result is block-uniform.
__device__ inline Window select_window(const snnflow_seq_args& a, const snnflow_seq_desc& d, double row,
                                       int64_t* __restrict__ idx, int* s_w) {
    Window w;
    w.i0 = 0; w.cnt = 0; w.flow = -1; w.dt_gt = 0.0; w.restart = false;
    int64_t i0 = 0, i1 = 0;
    if (a.mode == SNNFLOW_SEQ_EVENTS) {
        const int64_t W = (int64_t)a.window;
        if (a.Hc < a.H0 || a.Wc < a.W0) {  // get_events_spatially_filtered, h5.py:449-545
            const int cy0 = (a.H0 - a.Hc) / 2, cy1 = cy0 + a.Hc, cx0 = (a.W0 - a.Wc) / 2, cx1 = cx0 + a.Wc;  // :458-461
            int64_t cur = (int64_t)row, chunk = W * 2, searched = 0, collected = 0;                           // :464-474
            while (collected < W && searched < W * 10) {                                                      // :476
                const int64_t end = cur + chunk < d.n ? cur + chunk : d.n;                                    // :478
                if (cur >= end) break;                                                                        // :480
                // the first (W - collected) events of the chunk inside the crop, in order (:491-507);
                // once the window is full the rest of the chunk changes nothing
                for (int64_t base = cur; base < end && collected < W; base += NT) {
                    const int64_t i = base + threadIdx.x;
                    bool in = false;
                    if (i < end) {
                        const int x = d.xs[i], y = d.ys[i];
                        in = y >= cy0 && y < cy1 && x >= cx0 && x < cx1;
                    }
                    int tot;
                    const int64_t at = collected + block_scan(in, s_w, tot);
                    if (in && at < W) idx[at] = i;
                    collected = collected + tot < W ? collected + tot : W;
                }
                cur = end;                                                                                    // :509
                searched += chunk;                                                                            // :510
                if (2 * collected < W) chunk = chunk * 2 < W * 5 ? chunk * 2 : W * 5;                         // :513-514
            }
            if (collected > 0) row = (double)cur;                                                             // :543
            w.i0 = -1;
            w.cnt = collected;
        } else {                                                                                              // :149-150
            i0 = slice_bound((int64_t)row, d.n);
            i1 = slice_bound((int64_t)row + W, d.n);
            w.i0 = i0;
            w.cnt = i1 > i0 ? i1 - i0 : 0;
        }
        w.restart = w.cnt < W;                                                                                // :241
    } else if (a.mode == SNNFLOW_SEQ_TIME) {                                                                  // :152-157
        const double x0 = row + d.t0;
        i0 = slice_bound(find_ts_index(d, x0, s_w), d.n);
        i1 = slice_bound(find_ts_index(d, x0 + a.window, s_w), d.n);
        w.i0 = i0;
        w.cnt = i1 > i0 ? i1 - i0 : 0;
        w.restart = row + a.window >= d.last_ts - d.t0;                                                       // :242-243, :70
    } else {
        const int64_t ic = (int64_t)ceil(row + a.window);
        if (ic >= d.nflow) {                                                                                  // :195-200
            w.restart = true;
        } else {
            int64_t f0 = (int64_t)floor(row);                                                                 // :166-169
            if (a.window < 1.0 && ic - f0 > 1) f0 += ic - f0 - 1;
            int64_t e0 = find_ts_index(d, d.flow_ts[f0], s_w);                                                // :170-171
            int64_t e1 = find_ts_index(d, d.flow_ts[ic], s_w);
            if (a.window < 1.0) {                                                                             // :221-236
                const double c0 = row - (double)f0, c1 = row + a.window - (double)f0;
                const double delta = (double)(e1 - e0), base = (double)e0;
                e1 = (int64_t)(base + c1 * delta);
                e0 = (int64_t)(base + c0 * delta);
            }
            i0 = slice_bound(e0, d.n);
            i1 = slice_bound(e1, d.n);
            w.i0 = i0;
            w.cnt = i1 > i0 ? i1 - i0 : 0;
            w.flow = ic;                                                                                      // :352
            if (ic > 0) w.dt_gt = d.flow_ts[ic] - d.flow_ts[ic - 1];                                          // :360-361
        }
    }
    if (w.cnt <= kFewEvents) w.cnt = 0;                                                                       // :248-252
    w.row = row + a.window;                                                                                   // :365
    return w;
}

__device__ inline void commit(const snnflow_seq_args& a, const Scratch& s, int b, const Window& w, int restarts,
                              int stuck) {
    a.row[b] = w.row;
    s.i0[b] = w.i0;
    s.cnt[b] = w.cnt;
    s.flow[b] = w.flow;
    a.counts[b] = (int)(w.cnt < a.N ? w.cnt : a.N);
    a.dt_gt[b] = w.dt_gt;
    a.restarts[b] = restarts;
    const int bits = (w.cnt > a.N ? SNNFLOW_SEQ_OVERFLOW : 0) | (stuck ? SNNFLOW_SEQ_STUCK : 0);
    if (bits) a.status[b] |= bits;
}

__global__ __launch_bounds__(NT) void k_seq_select(snnflow_seq_args a) {
    __shared__ int s_w[kNW];
    __shared__ int s_last;
    const Scratch s = scratch_of(a);
    const int b = blockIdx.x, tid = threadIdx.x;
    {
        const snnflow_seq_desc d = a.seqs[a.batch_idx[b] % a.nseq];
        const Window w = select_window(a, d, a.row[b], s.idx + (int64_t)b * a.N, s_w);
        if (tid == 0) {
            if (w.restart) s.cnt[b] = -1;
            else commit(a, s, b, w, 0, 0);
        }
    }
    // every wave's stores have completed; thread 0 publishes the block's results device-wide
    // (one fence per block) and counts the block as done
    __syncthreads();
    if (tid == 0) {
        __threadfence();
        const unsigned long long done = atomicAdd(s.done, 1ull);
        const int last = done == (unsigned long long)gridDim.x - 1;
        if (last) {
            __threadfence();
            *s.done = 0ull;  // ready for the next call (and for a graph replay)
        }
        s_last = last;
    }
    __syncthreads();
    if (!s_last) return;
    // the last block: restarts in slot order (h5.py:255-263); rare, so one block takes them all
    for (int r = 0; r < a.B; ++r) {
        const int64_t pending = (int64_t)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(s.cnt + r),
                                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (pending != -1) continue;  // block-uniform
        int n = 0;
        for (;;) {
            if (n == a.nseq) {  // the reference would loop forever: an empty window and a status bit
                Window w;
                w.i0 = 0; w.cnt = 0; w.flow = -1; w.dt_gt = 0.0; w.row = 0.0; w.restart = false;
                if (tid == 0) commit(a, s, r, w, n, 1);
                break;
            }
            int64_t mx = a.batch_idx[0];
            for (int k = 1; k < a.B; ++k) mx = a.batch_idx[k] > mx ? a.batch_idx[k] : mx;
            __syncthreads();  // every thread has read the old indices
            if (tid == 0) a.batch_idx[r] = mx + 1;                                                            // :259
            ++n;
            const snnflow_seq_desc d = a.seqs[(mx + 1) % a.nseq];                                             // :262
            const Window w = select_window(a, d, 0.0, s.idx + (int64_t)r * a.N, s_w);                         // :258
            __syncthreads();  // the new index is visible to the next round's maximum
            if (!w.restart) {
                if (tid == 0) commit(a, s, r, w, n, 0);
                break;
            }
        }
    }
}

// grid (nev + nfl, B): blocks [0, nev) of a slot move its events, blocks [nev, nev + nfl) its flow map.
__global__ __launch_bounds__(NT) void k_seq_gather(snnflow_seq_args a, int nev) {
    const Scratch s = scratch_of(a);
    const int b = blockIdx.y;
    const int64_t cnt_all = s.cnt[b], cnt = cnt_all < a.N ? cnt_all : a.N;
    if ((int)blockIdx.x >= nev) {
        if (!a.gtflow) return;
        const int64_t HW2 = (int64_t)2 * a.H0 * a.W0, f = s.flow[b];
        float* dst = a.gtflow + (int64_t)b * HW2;
        const float* src = nullptr;
        if (f >= 0) src = a.seqs[a.batch_idx[b] % a.nseq].flow_maps + f * HW2;                                // :354
        for (int64_t i = (int64_t)(blockIdx.x - nev) * NT + threadIdx.x; i < HW2; i += (int64_t)(gridDim.x - nev) * NT)
            dst[i] = src ? src[i] : 0.0f;
        return;
    }
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= a.N) return;
    const int64_t e = (int64_t)b * a.N + i;
    if (i >= cnt) {  // padding
        a.xs[e] = 0.0f; a.ys[e] = 0.0f; a.ts[e] = 0.0f; a.ps[e] = 0.0f;
        if (i == 0) a.dt_input[b] = 0.0;                                                                      // :286
        return;
    }
    const snnflow_seq_desc d = a.seqs[a.batch_idx[b] % a.nseq];
    const int64_t i0 = s.i0[b];
    const bool crop = i0 < 0;
    const int cy0 = crop ? (a.H0 - a.Hc) / 2 : 0, cx0 = crop ? (a.W0 - a.Wc) / 2 : 0;
    const int64_t src = crop ? s.idx[e] : i0 + i;
    a.xs[e] = (float)(d.xs[src] - cx0);                                                                       // :524-525
    a.ys[e] = (float)(d.ys[src] - cy0);
    a.ts[e] = (float)(d.ts[src] - d.t0);                                                                      // :133, base.py:87
    a.ps[e] = (float)d.ps[src];
    if (i == 0) {
        const int64_t last = crop ? s.idx[(int64_t)b * a.N + cnt_all - 1] : i0 + cnt_all - 1;
        a.dt_input[b] = (d.ts[last] - d.t0) - (d.ts[src] - d.t0);                                             // :288
    }
}

}  // namespace

extern "C" int snnflow_seq_next(const snnflow_seq_args* a, void* stream) {
    if (!a) SNN_FAIL(SNNFLOW_E_ARG, "seq_next: NULL args");
    if (a->B <= 0 || a->B > 65535 || a->N <= 0) SNN_FAIL(SNNFLOW_E_ARG, "seq_next: B must be in [1, 65535] and N positive");
    if (a->mode != SNNFLOW_SEQ_EVENTS && a->mode != SNNFLOW_SEQ_TIME && a->mode != SNNFLOW_SEQ_GTFLOW)
        SNN_FAIL(SNNFLOW_E_ARG, "seq_next: unknown mode");
    if (a->nseq <= 0) SNN_FAIL(SNNFLOW_E_ARG, "seq_next: no sequences");
    if (!(a->window > 0.0) || a->window > 1e15) SNN_FAIL(SNNFLOW_E_ARG, "seq_next: window must be positive");
    if (a->H0 <= 0 || a->W0 <= 0 || a->Hc <= 0 || a->Wc <= 0 || a->H0 > 32767 || a->W0 > 32767)
        SNN_FAIL(SNNFLOW_E_ARG, "seq_next: bad resolution");
    if (a->Hc > a->H0 || a->Wc > a->W0) SNN_FAIL(SNNFLOW_E_ARG, "seq_next: the crop is larger than the frame");
    if (a->mode == SNNFLOW_SEQ_EVENTS && (a->window != floor(a->window) || a->window > (double)a->N))
        SNN_FAIL(SNNFLOW_E_ARG, "seq_next: an event window is a whole number of at most N events");
    if (!a->seqs || !a->row || !a->batch_idx || !a->status || !a->scratch || !a->xs || !a->ys || !a->ts || !a->ps ||
        !a->counts || !a->dt_input || !a->dt_gt || !a->restarts || (a->mode == SNNFLOW_SEQ_GTFLOW && !a->gtflow))
        SNN_FAIL(SNNFLOW_E_ARG, "seq_next: NULL pointer");
    if (a->scratch_words < SNNFLOW_SEQ_SCRATCH_WORDS(a->B, a->N)) SNN_FAIL(SNNFLOW_E_ARG, "seq_next: scratch too small");
    const hipStream_t s = (hipStream_t)stream;
    snnflow_seq_args q = *a;
    if (q.mode != SNNFLOW_SEQ_GTFLOW) q.gtflow = nullptr;
    hipLaunchKernelGGL(k_seq_select, dim3((unsigned)q.B), dim3(NT), 0, s, q);
    SNN_CHECK_LAUNCH();
    const int nev = (q.N + NT - 1) / NT;
    int nfl = 0;
    if (q.gtflow) {
        const int64_t want = ((int64_t)2 * q.H0 * q.W0 + NT * 4 - 1) / (NT * 4);
        nfl = (int)(want < 64 ? want : 64);
    }
    hipLaunchKernelGGL(k_seq_gather, dim3((unsigned)(nev + nfl), (unsigned)q.B), dim3(NT), 0, s, q, nev);
    SNN_CHECK_LAUNCH();
    return 0;
}
