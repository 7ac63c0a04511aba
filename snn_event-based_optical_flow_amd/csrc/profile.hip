// Membrane profiling for gfx950: the statistics the reference's two membrane-dynamics tools collect
// through forward hooks and host copies (analyze_voltage_dynamics.py:33-241 VoltageProfiler,
// eval_flow_quant.py:186-463 profile_membrane_ranges), as one streaming pass over cell states that are
// already in HBM.  A call folds up to SNNFLOW_VSTATS_MAX_TENSORS states [2][B][C][H][W] (membrane half,
// spike half) into persistent per-slot accumulators (a slot is a layer): exact integer counts, exact
// extrema, fp64 sums and a 65536-bin histogram of every finite membrane value.
//
// k_vstats: one thread owns (slot, pixel, 4 channels) items, loops over the slot's tensors of the call
// (ascending) and over the batch, and keeps its per-channel partials in registers.  The neuron spike
// counters of its item are then a plain read-modify-write (no atomics).  The block reduces the partials
// of the threads that share a channel quad (wave shuffles over the lane bits above the quad index, then
// the four waves through LDS, both in a fixed order) and writes one record per (slot, block) to scratch.
// k_vstats_fold: one wave per slot adds the records in ascending block order and updates the
// accumulators -- no float atomics anywhere, so the fp64 sums are bit-reproducible for the same sequence
// of calls.  The histogram is integer counts (any order gives the same table): exact zeros (every neuron
// that just spiked) are counted in a register and added once per block; other values go to the table by
// integer atomics: through an LDS sub-table of the 2048 bins of 2^-6 <= |v| < 4 that the block flushes at
// its end (the default), or all directly to global memory (snnflow_vstats_hist_mode(0)).
#include <cstdlib>

#include "snnflow_dev.h"
#include "snnflow_host.h"

using namespace snnflow;

namespace {

typedef unsigned long long u64;
constexpr int kMaxT = SNNFLOW_VSTATS_MAX_TENSORS;
constexpr int kMaxBlocks = 256;  // records per slot (items beyond are grid-strided)
constexpr int kWaves = NT / 64;
constexpr int kLdsBins = 2048;   // sign x 8 exponents (2^-6 .. 2^1) x 128 bf16 mantissas
constexpr unsigned kLdsE0 = 121u << 7, kLdsE1 = 129u << 7;

struct KArgs {
    const float* t[kMaxT];      // grouped by slot (the order of slots[]), call order within a slot
    int start[kMaxT + 1];       // tensors of slots[i]: t[start[i] .. start[i + 1])
    int slots[kMaxT];           // distinct slots of the call, ascending
    int n, nact, B, C, HW, nchw, nblk;
    double* scratch;
    u64* count; u64* nonfinite;
    double* chan_sum; double* chan_sumsq;
    float* chan_min; float* chan_max;
    u64* chan_spikes;
    unsigned* neuron;           // [slot][HW][C]
    u64* hist;                  // [slot][65536] or NULL
};

// Scratch record of one (slot, block): 8-byte entries sum[C], sumsq[C], (min, max)[C], spikes[C],
// count[Q], nonfinite[Q]  (Q = C / 4 channel quads; NCHW blocks hold one quad each: blockIdx.y).
__host__ __device__ inline int rec_len(int C) { return 4 * C + 2 * (C / 4); }

__device__ inline unsigned canon_bits(float v) {
    const unsigned b = __float_as_uint(v);
    return b == 0x80000000u ? 0u : b;   // v + 0.0f: -0.0 counts as +0.0
}
__device__ inline unsigned key16(unsigned b) { return ((b >> 31) ? ~b : (b | 0x80000000u)) >> 16; }

struct Part {
    double sum[4], sq[4];
    float mn[4], mx[4];
    unsigned spk[4];
    unsigned cnt, nonf, zeros;
};

template <bool HIST, bool LDSH>
__device__ inline void take(Part& p, int j, float vraw, float s, u64* __restrict__ hist, unsigned* lh) {
    const unsigned b = canon_bits(vraw);
    const bool fin = (b & 0x7F800000u) != 0x7F800000u;
    const float v = __uint_as_float(b);
    const double dv = fin ? (double)v : 0.0;
    p.sum[j] += dv;
    p.sq[j] += dv * dv;
    p.mn[j] = fin ? fminf(p.mn[j], v) : p.mn[j];
    p.mx[j] = fin ? fmaxf(p.mx[j], v) : p.mx[j];
    p.cnt += fin ? 1u : 0u;
    p.nonf += fin ? 0u : 1u;
    p.spk[j] += (s != 0.0f) ? 1u : 0u;
    if constexpr (HIST) {
        if (fin) {
            if (b == 0u) {
                p.zeros += 1u;
            } else {
                const unsigned e7 = (b >> 16) & 0x7FFFu;
                if (LDSH && e7 >= kLdsE0 && e7 < kLdsE1)
                    atomicAdd(lh + ((b >> 31) * (kLdsBins / 2) + (e7 - kLdsE0)), 1u);
                else
                    atomicAdd(hist + key16(b), (u64)1);
            }
        }
    }
}

template <typename T>
__device__ inline T shx(T v, int o) { return __shfl_xor(v, o, 64); }

template <bool HIST, bool LDSH>
__global__ __launch_bounds__(NT) void k_vstats(KArgs a) {
    __shared__ double sh[kWaves][16][16];   // per wave, per quad lane: 16 8-byte entries of the record
    __shared__ unsigned lh[LDSH ? kLdsBins : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ai = blockIdx.z, slot = a.slots[ai];
    const int C = a.C, Q = C >> 2, HW = a.HW, B = a.B;
    const int qmod = a.nchw ? 1 : Q;                  // threads of a block that share a quad: tid % qmod
    const int64_t nitems = a.nchw ? (int64_t)HW : (int64_t)HW * Q;
    const int64_t half = (int64_t)B * C * HW;         // floats of a state half
    u64* __restrict__ hist = HIST ? a.hist + (size_t)slot * 65536 : nullptr;
    if constexpr (LDSH) {
        for (int i = tid; i < kLdsBins; i += NT) lh[i] = 0u;
        __syncthreads();
    }
    Part p;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        p.sum[j] = 0.0; p.sq[j] = 0.0; p.mn[j] = INFINITY; p.mx[j] = -INFINITY; p.spk[j] = 0u;
    }
    p.cnt = p.nonf = p.zeros = 0u;
    const int qn = a.nchw ? (int)blockIdx.y : 0;      // NCHW: the block's quad
    const int k0 = a.start[ai], total = (a.start[ai + 1] - k0) * B;   // the slot's tensors: t[k0 ..), call order
    for (int64_t item = (int64_t)blockIdx.x * NT + tid; item < nitems; item += (int64_t)gridDim.x * NT) {
        // NHWC: item = pixel * Q + quad (consecutive lanes read consecutive 16-B words);
        // NCHW: item = pixel, four channel planes (consecutive lanes read consecutive floats of each)
        const int64_t px = a.nchw ? item : item / Q;
        const int q = a.nchw ? qn : (int)(item - px * Q);
        unsigned ns[4] = {0u, 0u, 0u, 0u};
        // (tensor k, batch entry b) of the slot in call order; the next pair's loads are issued before this
        // pair's values are used
        auto load = [&](int k, int b, float (&m)[4], float (&s)[4]) {
            const float* __restrict__ t = a.t[k];
            if (a.nchw) {
                const int64_t o = ((int64_t)b * C + 4 * q) * HW + px;
#pragma unroll
                for (int j = 0; j < 4; ++j) { m[j] = t[o + (int64_t)j * HW]; s[j] = t[half + o + (int64_t)j * HW]; }
            } else {
                const int64_t o = ((int64_t)b * HW + px) * C + 4 * q;
                const float4 mv = *reinterpret_cast<const float4*>(t + o);
                const float4 sv = *reinterpret_cast<const float4*>(t + half + o);
                m[0] = mv.x; m[1] = mv.y; m[2] = mv.z; m[3] = mv.w;
                s[0] = sv.x; s[1] = sv.y; s[2] = sv.z; s[3] = sv.w;
            }
        };
        float m[4], s[4];
        int k = k0, b = 0;
        load(k, b, m, s);
        for (int it = 0; it < total; ++it) {
            float mn[4], sn[4];
            if (it + 1 < total) {                      // block-uniform
                if (++b == B) { b = 0; ++k; }
            }
            load(k, b, mn, sn);                        // (the last pair again at the end: in bounds, unused)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned before = p.spk[j];
                take<HIST, LDSH>(p, j, m[j], s[j], hist, lh);
                ns[j] += p.spk[j] - before;
                m[j] = mn[j]; s[j] = sn[j];
            }
        }
        uint4* nc = reinterpret_cast<uint4*>(a.neuron + ((size_t)slot * HW + px) * C + 4 * q);
        uint4 o = *nc;
        o.x += ns[0]; o.y += ns[1]; o.z += ns[2]; o.w += ns[3];
        *nc = o;
    }
    // the wave's threads of one quad: lanes equal in lane % qmod (xor offsets >= qmod keep it), fixed order
    for (int o = 32; o >= qmod; o >>= 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            p.sum[j] += shx(p.sum[j], o);
            p.sq[j] += shx(p.sq[j], o);
            p.mn[j] = fminf(p.mn[j], shx(p.mn[j], o));
            p.mx[j] = fmaxf(p.mx[j], shx(p.mx[j], o));
            p.spk[j] += shx(p.spk[j], o);
        }
        p.cnt += shx(p.cnt, o);
        p.nonf += shx(p.nonf, o);
        p.zeros += shx(p.zeros, o);
    }
    if (lane < qmod) {
        double* r = sh[wave][lane];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            r[j] = p.sum[j];
            r[4 + j] = p.sq[j];
            r[8 + j] = __hiloint2double(__float_as_int(p.mx[j]), __float_as_int(p.mn[j]));
            r[12 + j] = __longlong_as_double((long long)p.spk[j]);
        }
    }
    __shared__ unsigned cn[kWaves][16][3];
    if (lane < qmod) { cn[wave][lane][0] = p.cnt; cn[wave][lane][1] = p.nonf; cn[wave][lane][2] = p.zeros; }
    __syncthreads();
    if (tid < qmod) {
        const int q = a.nchw ? qn : tid;
        double sum[4], sq[4];
        float mn[4], mx[4];
        u64 spk[4];
        u64 cnt = 0, nonf = 0, zeros = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) { sum[j] = 0.0; sq[j] = 0.0; mn[j] = INFINITY; mx[j] = -INFINITY; spk[j] = 0; }
        for (int w = 0; w < kWaves; ++w) {
            const double* r = sh[w][tid];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sum[j] += r[j];
                sq[j] += r[4 + j];
                mn[j] = fminf(mn[j], __int_as_float(__double2loint(r[8 + j])));
                mx[j] = fmaxf(mx[j], __int_as_float(__double2hiint(r[8 + j])));
                spk[j] += (u64)__double_as_longlong(r[12 + j]);
            }
            cnt += cn[w][tid][0]; nonf += cn[w][tid][1]; zeros += cn[w][tid][2];
        }
        double* rec = a.scratch + ((size_t)ai * a.nblk + blockIdx.x) * rec_len(C);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = 4 * q + j;
            rec[c] = sum[j];
            rec[C + c] = sq[j];
            rec[2 * C + c] = __hiloint2double(__float_as_int(mx[j]), __float_as_int(mn[j]));
            rec[3 * C + c] = __longlong_as_double((long long)spk[j]);
        }
        rec[4 * C + q] = __longlong_as_double((long long)cnt);
        rec[4 * C + Q + q] = __longlong_as_double((long long)nonf);
        if (HIST && zeros) atomicAdd(hist + 0x8000, zeros);   // key16(+0.0)
    }
    if constexpr (HIST && LDSH) {
        for (int i = tid; i < kLdsBins; i += NT) {           // (lh is complete: the barrier above)
            const unsigned v = lh[i];
            if (v) {
                const unsigned e7 = kLdsE0 + (i & (kLdsBins / 2 - 1));
                const unsigned bin = (i >= kLdsBins / 2) ? 0x7FFFu - e7 : 0x8000u | e7;
                atomicAdd(hist + bin, (u64)v);
            }
        }
    }
}

__global__ __launch_bounds__(64) void k_vstats_fold(KArgs a) {
    const int ai = blockIdx.x, slot = a.slots[ai], C = a.C, Q = C >> 2, c = threadIdx.x;
    const int L = rec_len(C);
    const double* base = a.scratch + (size_t)ai * a.nblk * L;
    if (c < C) {
        double sum = 0.0, sq = 0.0;
        float mn = INFINITY, mx = -INFINITY;
        u64 spk = 0;
        for (int bx = 0; bx < a.nblk; ++bx) {   // ascending block order
            const double* rec = base + (size_t)bx * L;
            sum += rec[c];
            sq += rec[C + c];
            mn = fminf(mn, __int_as_float(__double2loint(rec[2 * C + c])));
            mx = fmaxf(mx, __int_as_float(__double2hiint(rec[2 * C + c])));
            spk += (u64)__double_as_longlong(rec[3 * C + c]);
        }
        const size_t k = (size_t)slot * C + c;
        a.chan_sum[k] += sum;
        a.chan_sumsq[k] += sq;
        a.chan_min[k] = fminf(a.chan_min[k], mn);
        a.chan_max[k] = fmaxf(a.chan_max[k], mx);
        a.chan_spikes[k] += spk;
    }
    if (c == 0) {
        u64 cnt = 0, nonf = 0;
        for (int bx = 0; bx < a.nblk; ++bx) {
            const double* rec = base + (size_t)bx * L + 4 * C;
            for (int q = 0; q < Q; ++q) {
                cnt += (u64)__double_as_longlong(rec[q]);
                nonf += (u64)__double_as_longlong(rec[Q + q]);
            }
        }
        a.count[slot] += cnt;
        a.nonfinite[slot] += nonf;
    }
}

int blocks_per_slot(int C, int H, int W, int layout) {
    const int64_t items = layout == SNNFLOW_LAYOUT_NCHW ? (int64_t)H * W : (int64_t)H * W * (C / 4);
    int64_t g = (items + NT - 1) / NT;
    if (g > kMaxBlocks) g = kMaxBlocks;
    return (int)g;
}

bool width_ok(int C) { return C == 4 || C == 8 || C == 16 || C == 32 || C == 64; }

// process-wide tuning (as snnflow_set_pipe): 0 = global integer atomics, 1 = the LDS sub-table (measured
// faster at every shape of tools/profile_time.py: DESIGN.md section 4)
int g_hist_lds = [] { const char* e = std::getenv("SNNFLOW_VSTATS_HIST_LDS"); return e && e[0] == '0' ? 0 : 1; }();

}  // namespace

extern "C" int snnflow_vstats_hist_mode(int mode) {
    if (mode == 0 || mode == 1) g_hist_lds = mode;
    return g_hist_lds;
}

extern "C" int64_t snnflow_vstats_scratch_bytes(int n, int B, int C, int H, int W, int layout) {
    if (n < 1 || n > kMaxT || B < 1 || H < 1 || W < 1 || !width_ok(C) ||
        (layout != SNNFLOW_LAYOUT_NHWC && layout != SNNFLOW_LAYOUT_NCHW))
        return -1;
    return (int64_t)n * blocks_per_slot(C, H, W, layout) * rec_len(C) * (int64_t)sizeof(double);
}

extern "C" int snnflow_vstats_update(const snnflow_vstats_args* g, void* stream) {
    if (!g) SNN_FAIL(SNNFLOW_E_ARG, "vstats: NULL args");
    if (g->n < 1 || g->n > kMaxT) SNN_FAIL(SNNFLOW_E_ARG, "vstats: n outside 1..SNNFLOW_VSTATS_MAX_TENSORS");
    if (g->layout != SNNFLOW_LAYOUT_NHWC && g->layout != SNNFLOW_LAYOUT_NCHW) SNN_FAIL(SNNFLOW_E_ARG, "vstats: unknown layout");
    if (g->B < 1 || g->H < 1 || g->W < 1) SNN_FAIL(SNNFLOW_E_ARG, "vstats: non-positive B, H or W");
    if (!width_ok(g->C)) SNN_FAIL(SNNFLOW_E_CHANNELS, "vstats: C must be 4, 8, 16, 32 or 64");
    if ((int64_t)g->H * g->W > (int64_t)1 << 26 || (int64_t)g->B * g->C * g->H * g->W > (int64_t)1 << 40)
        SNN_FAIL(SNNFLOW_E_ARG, "vstats: tensor too large");
    if (g->nslots < 1) SNN_FAIL(SNNFLOW_E_ARG, "vstats: nslots < 1");
    if (!g->count || !g->nonfinite || !g->chan_sum || !g->chan_sumsq || !g->chan_min || !g->chan_max ||
        !g->chan_spikes || !g->neuron_spikes || !g->scratch)
        SNN_FAIL(SNNFLOW_E_ARG, "vstats: NULL accumulator or scratch");
    KArgs a = {};
    for (int i = 0; i < g->n; ++i) {
        if (!g->state[i]) SNN_FAIL(SNNFLOW_E_ARG, "vstats: NULL state tensor");
        if (reinterpret_cast<uintptr_t>(g->state[i]) & (g->layout == SNNFLOW_LAYOUT_NHWC ? 15 : 3))
            SNN_FAIL(SNNFLOW_E_ARG, "vstats: misaligned state tensor (NHWC: 16 bytes)");
        if (g->slot[i] < 0 || g->slot[i] >= g->nslots) SNN_FAIL(SNNFLOW_E_ARG, "vstats: slot outside [0, nslots)");
    }
    // distinct slots, ascending; then the tensors grouped by slot, call order within a slot
    int nact = 0;
    for (int i = 0; i < g->n; ++i) {
        int k = 0;
        while (k < nact && a.slots[k] < g->slot[i]) ++k;
        if (k < nact && a.slots[k] == g->slot[i]) continue;
        for (int j = nact; j > k; --j) a.slots[j] = a.slots[j - 1];
        a.slots[k] = g->slot[i];
        ++nact;
    }
    for (int k = 0, pos = 0; k < nact; ++k) {
        a.start[k] = pos;
        for (int i = 0; i < g->n; ++i)
            if (g->slot[i] == a.slots[k]) a.t[pos++] = g->state[i];
        a.start[k + 1] = pos;
    }
    const int nblk = blocks_per_slot(g->C, g->H, g->W, g->layout);
    {   // a block's counts (finite values, zeros, LDS bins) are 32-bit until the fold
        int most = 0;
        for (int k = 0; k < nact; ++k) most = a.start[k + 1] - a.start[k] > most ? a.start[k + 1] - a.start[k] : most;
        const int64_t items = g->layout == SNNFLOW_LAYOUT_NCHW ? (int64_t)g->H * g->W : (int64_t)g->H * g->W * (g->C / 4);
        const int64_t per_thread = (items + (int64_t)nblk * NT - 1) / ((int64_t)nblk * NT);
        if (per_thread * NT * 4 * g->B * most >= (int64_t)1 << 32)
            SNN_FAIL(SNNFLOW_E_ARG, "vstats: too many values per block for one call (pass fewer states per call)");
    }
    if (g->scratch_bytes < (int64_t)nact * nblk * rec_len(g->C) * (int64_t)sizeof(double))
        SNN_FAIL(SNNFLOW_E_ARG, "vstats: scratch too small (snnflow_vstats_scratch_bytes)");
    a.n = g->n; a.nact = nact; a.B = g->B; a.C = g->C; a.HW = g->H * g->W;
    a.nchw = g->layout == SNNFLOW_LAYOUT_NCHW;
    a.nblk = nblk;
    a.scratch = static_cast<double*>(g->scratch);
    a.count = reinterpret_cast<u64*>(g->count);
    a.nonfinite = reinterpret_cast<u64*>(g->nonfinite);
    a.chan_sum = g->chan_sum; a.chan_sumsq = g->chan_sumsq;
    a.chan_min = g->chan_min; a.chan_max = g->chan_max;
    a.chan_spikes = reinterpret_cast<u64*>(g->chan_spikes);
    a.neuron = g->neuron_spikes;
    a.hist = reinterpret_cast<u64*>(g->hist);
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)nblk, a.nchw ? (unsigned)(g->C / 4) : 1u, (unsigned)nact);
    if (!a.hist) hipLaunchKernelGGL((k_vstats<false, false>), grid, dim3(NT), 0, s, a);
    else if (g_hist_lds) hipLaunchKernelGGL((k_vstats<true, true>), grid, dim3(NT), 0, s, a);
    else hipLaunchKernelGGL((k_vstats<true, false>), grid, dim3(NT), 0, s, a);
    SNN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_vstats_fold, dim3((unsigned)nact), dim3(64), 0, s, a);
    SNN_CHECK_LAUNCH();
    return 0;
}
