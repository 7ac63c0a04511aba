// Visual evaluation for gfx950: exact np.percentile by radix selection, the frame renderers of
// utils/visualization.py (flow_to_image :649-709, events_to_image :1037-1084, error_to_image
// :618-645, minmax_norm :1025-1034) and the per-pixel error maps of loss/flow.py:618-631, 729-747,
// 790-808 with their aggregation (:489-511).  Finite inputs only (snnflow.h).
#include <cmath>

#include "snnflow_dev.h"
#include "snnflow_host.h"

using namespace snnflow;

namespace {

// ---- radix select ----
// One block per plane.  A target is one order statistic (a rank in the sorted plane); a quantile has
// two, floor(vi) and the next.  Pass k (k = 0..3) fixes bits 31-8k .. 24-8k of every target's key:
// the block histograms that digit over the elements whose higher bits equal the target's prefix,
// and the target walks the 256 counts to the digit that holds its remaining rank.  Targets with
// the same prefix share one histogram (all of them in pass 0, the two of a quantile until their
// keys part), so a pass costs one LDS atomic per element and distinct prefix.
constexpr int SEL_NT = 1024, SEL_MAXT = 2 * SNNFLOW_VIS_MAX_Q, SEL_MAX_N = 1 << 24;

struct SelPlan {
    int nq, fp64;
    int rank[SEL_MAXT];               // targets 2k, 2k+1: the ranks around quantile k
    double g64[SNNFLOW_VIS_MAX_Q];    // numpy's gamma (fp64 mode)
    float g32[SNNFLOW_VIS_MAX_Q];     // (fp32 mode)
};

// order-preserving key of a finite float (-0 as +0)
__device__ inline unsigned f2key(float v) {
    const unsigned u = __float_as_uint(v + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float key2f(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// h[bin] += 1 for every lane with `on`; lanes of the wave that share a bin (event counts are mostly
// zeros, a uniform field is one value) are counted with ballots and added once, for the bins of the
// first two distinct leaders; whatever is left adds by itself.  Called by whole waves.
__device__ inline void hist_add(unsigned* h, int bin, bool on) {
    unsigned long long todo = __ballot(on);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        if (!todo) break;
        const int leader = __ffsll((long long)todo) - 1;
        const int lb = __shfl(bin, leader, 64);
        const unsigned long long same = __ballot(on && bin == lb);
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&h[lb], (unsigned)__popcll(same));
        if (bin == lb) on = false;
        todo &= ~same;
    }
    if (on) atomicAdd(&h[bin], 1u);
}

// MAG: the plane is the fp32 magnitude of a flow image (x at src[i], y at src[n + i])
template <bool MAG>
__device__ inline float sel_load(const float* __restrict__ src, int n, int i) {
    if constexpr (MAG) {
        const float x = src[i], y = src[n + i];
        return sqrtf(x * x + y * y);
    } else {
        return src[i];
    }
}

template <bool MAG>
__global__ __launch_bounds__(SEL_NT) void k_select(const float* __restrict__ x, int n, SelPlan p, void* out) {
    __shared__ unsigned hist[SEL_MAXT][256];
    __shared__ unsigned prefix[SEL_MAXT], rem[SEL_MAXT], gpre[SEL_MAXT];
    __shared__ int tgrp[SEL_MAXT], ngrp;
    const int tid = threadIdx.x, nt = 2 * p.nq;
    const float* src = x + (int64_t)blockIdx.x * (MAG ? 2 : 1) * n;
    if (tid < nt) {
        prefix[tid] = 0u;
        rem[tid] = (unsigned)p.rank[tid];
        tgrp[tid] = 0;
    }
    if (tid == 0) {
        ngrp = 1;
        gpre[0] = 0u;
    }
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        for (int j = tid; j < SEL_MAXT * 256; j += SEL_NT) (&hist[0][0])[j] = 0u;
        __syncthreads();
        const int ng = ngrp;
        unsigned gp[SEL_MAXT];
#pragma unroll
        for (int g = 0; g < SEL_MAXT; ++g) gp[g] = g < ng ? gpre[g] : 0u;
        // whole waves stay in the loop (ballots in hist_add).  One block walks the plane and the loop is
        // bound by instruction issue on its CU, not by load latency: four loads in flight per thread
        // measured 0.3185 -> 0.3143 ms per 260x346 flow image, not kept
        for (int base = 0; base < n; base += SEL_NT) {
            const int i = base + tid;
            const bool valid = i < n;
            const unsigned key = valid ? f2key(sel_load<MAG>(src, n, i)) : 0u;
            const int bin = (int)((key >> shift) & 255u);
#pragma unroll
            for (int g = 0; g < SEL_MAXT; ++g) {
                if (g >= ng) break;
                const bool on = valid && (pass == 0 || ((key ^ gp[g]) >> (shift + 8)) == 0u);
                hist_add(hist[g], bin, on);
            }
        }
        __syncthreads();
        if (tid < nt) {
            const unsigned* h = hist[tgrp[tid]];
            unsigned r = rem[tid], cum = 0u;
            int d = 0;
            for (; d < 255; ++d) {  // the counts of the target's prefix sum to more than its rank
                const unsigned c = h[d];
                if (r < cum + c) break;
                cum += c;
            }
            prefix[tid] |= (unsigned)d << shift;
            rem[tid] = r - cum;
        }
        __syncthreads();
        if (tid == 0) {  // distinct prefixes -> histogram rows of the next pass
            int ngn = 0;
            for (int t = 0; t < nt; ++t) {
                int g = 0;
                while (g < ngn && gpre[g] != prefix[t]) ++g;
                if (g == ngn) gpre[ngn++] = prefix[t];
                tgrp[t] = g;
            }
            ngrp = ngn;
        }
        __syncthreads();
    }
    if (tid < p.nq) {  // numpy's _lerp
        const float a = key2f(prefix[2 * tid]), b = key2f(prefix[2 * tid + 1]);
        if (p.fp64) {
            const double g = p.g64[tid], d = (double)b - (double)a;
            double r = (double)a + d * g;
            if (g >= 0.5) r = (double)b - d * (1.0 - g);
            static_cast<double*>(out)[(int64_t)blockIdx.x * p.nq + tid] = r;
        } else {
            const float g = p.g32[tid], d = b - a;
            float r = a + d * g;
            if (g >= 0.5f) r = b - d * (1.0f - g);
            static_cast<float*>(out)[(int64_t)blockIdx.x * p.nq + tid] = r;
        }
    }
}

// numpy's virtual index, neighbours and gamma (lib/_function_base_impl.py _quantile, _get_indexes,
// _get_gamma) on the host: plain IEEE arithmetic (-ffp-contract=off).
bool make_plan(int n, int nq, const double* q, int fp64, SelPlan& p) {
    if (n < 1 || n > SEL_MAX_N || nq < 1 || nq > SNNFLOW_VIS_MAX_Q) return false;
    p.nq = nq;
    p.fp64 = fp64;
    for (int k = 0; k < nq; ++k) {
        if (!(q[k] >= 0.0 && q[k] <= 100.0)) return false;
        double lo;
        bool above;
        if (fp64) {
            const double vi = (double)(n - 1) * (q[k] / 100.0);
            lo = std::floor(vi);
            above = vi >= (double)(n - 1);
            p.g64[k] = vi - lo;
            p.g32[k] = 0.0f;
        } else {
            const float q32 = (float)q[k] / 100.0f;
            const float vi = (float)(n - 1) * q32;
            const float fl = std::floor(vi);
            lo = (double)fl;
            above = vi >= (float)(n - 1);
            p.g32[k] = vi - fl;
            p.g64[k] = 0.0;
        }
        const int l = above ? n - 1 : (int)lo;
        p.rank[2 * k] = l;
        p.rank[2 * k + 1] = above ? n - 1 : l + 1;  // (l + 1 <= n - 1 below the bound)
        if (p.rank[2 * k + 1] > n - 1) p.rank[2 * k + 1] = n - 1;
    }
    for (int k = 2 * nq; k < SEL_MAXT; ++k) p.rank[k] = 0;
    return true;
}

// ---- renderers: one thread per pixel ----

__device__ inline double clipd(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }
__device__ inline float clipf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

__global__ __launch_bounds__(NT) void k_flow_render(const float* __restrict__ flow, const double* __restrict__ stats,
                                                   int B, int HWp, int has_uv, double uv, uint8_t* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= (int64_t)B * HWp) return;
    const int b = (int)(idx / HWp), p = (int)(idx - (int64_t)b * HWp);
    const float x = flow[(int64_t)b * 2 * HWp + p], y = flow[(int64_t)b * 2 * HWp + HWp + p];
    const double mag = (double)sqrtf(x * x + y * y);
    const double mn = stats[4 * b], mx = stats[4 * b + 1], p5 = stats[4 * b + 2], p95 = stats[4 * b + 3];
    float ang = atan2f(y, x) + kPiF;  // numpy keeps the hue in fp32
    ang = ang * (float)(1.0 / 3.14159265358979323846 / 2.0);
    const double h = (double)ang;
    double v = 0.0;
    if (mx - mn > 0.0) {
        const double nm = sqrt(clipd((mag - p5) / (p95 - p5 + 1e-8), 0.0, 1.0));
        v = mag > 0.0 ? clipd(nm * 1.3 + 0.15, 0.15, 1.0) : 0.0;
    } else if (mx > 0.0) {
        double u = mag / mx;
        if (has_uv) u = u * uv;
        u = sqrt(u) * 1.3 + 0.15;
        v = mag > 0.0 ? clipd(u, 0.15, 1.0) : 0.0;
    }
    // matplotlib.colors.hsv_to_rgb with s = 1
    const double h6 = h * 6.0;
    const int i = (int)h6;
    const double f = h6 - (double)i;
    const double pp = v * (1.0 - 1.0), qq = v * (1.0 - 1.0 * f), tt = v * (1.0 - 1.0 * (1.0 - f));
    double r, g, bl;
    switch (i % 6) {
        case 0: r = v; g = tt; bl = pp; break;
        case 1: r = qq; g = v; bl = pp; break;
        case 2: r = pp; g = v; bl = tt; break;
        case 3: r = pp; g = qq; bl = v; break;
        case 4: r = tt; g = pp; bl = v; break;
        default: r = v; g = pp; bl = qq; break;
    }
    uint8_t* o = out + idx * 3;
    o[0] = (uint8_t)(int)(255.0 * r);
    o[1] = (uint8_t)(int)(255.0 * g);
    o[2] = (uint8_t)(int)(255.0 * bl);
}

__global__ __launch_bounds__(NT) void k_events_render(const float* __restrict__ cnt, const float* __restrict__ stats,
                                                     int B, int HWp, int gray, float* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= (int64_t)B * HWp) return;
    const int b = (int)(idx / HWp), p = (int)(idx - (int64_t)b * HWp);
    float pos = cnt[(int64_t)b * 2 * HWp + p], neg = cnt[(int64_t)b * 2 * HWp + HWp + p];
    const float pmin = stats[4 * b], pmax = stats[4 * b + 1], nmin = stats[4 * b + 2], nmax = stats[4 * b + 3];
    const float mx = pmax > nmax ? pmax : nmax;
    if (pmin != mx) pos = (pos - pmin) / (mx - pmin);
    if (nmin != mx) neg = (neg - nmin) / (mx - nmin);
    pos = clipf(pos, 0.0f, 1.0f);
    neg = clipf(neg, 0.0f, 1.0f);
    if (gray) {
        pos = pos * 0.5f;
        neg = neg * -0.5f;
        out[idx] = (float)(0.5 + (double)(pos + neg));  // the reference's image is fp64
    } else {
        float* o = out + idx * 3;
        o[0] = neg > 0.0f ? neg : 0.0f;
        o[1] = pos > 0.0f ? pos : 0.0f;
        o[2] = 0.0f;
    }
}

__global__ __launch_bounds__(NT) void k_minmax_render(const float* __restrict__ x, const float* __restrict__ stats,
                                                     int B, int n, float* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= (int64_t)B * n) return;
    const int b = (int)(idx / n);
    const float p1 = stats[2 * b], den = stats[2 * b + 1] - p1;
    float v = x[idx];
    if (den != 0.0f) v = (v - p1) / den;
    out[idx] = clipf(v, 0.0f, 1.0f);
}

__global__ __launch_bounds__(NT) void k_error_render(const float* __restrict__ err, int64_t n, uint8_t* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= n) return;
    const float deg = err[idx] * (180.0f / kPiF);  // np.degrees of a float32 array
    const float v = clipf(deg / 180.0f, 0.0f, 1.0f);
    uint8_t* o = out + idx * 3;
    o[0] = (uint8_t)(int)(v * 255.0f);
    o[1] = 0;
    o[2] = 0;
}

// ---- error maps: the per-pixel expressions of k_aee / k_flow_metrics (eval.hip) ----
constexpr float kClampLo = -1.0f + 1e-5f, kClampHi = 1.0f - 1e-5f;

__global__ __launch_bounds__(NT) void k_error_maps(snnflow_error_maps_args a) {
    const int64_t HWp = (int64_t)a.H * a.W;
    const int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (p >= HWp) return;
    float s = 0.0f, c = 0.0f;
    for (int b = 0; b < a.B; ++b) {
        const float r = a.dt_ratio[b];
        const float* f = a.flow + (int64_t)b * 2 * HWp + p;
        const float* g = a.gtflow + (int64_t)b * 2 * HWp + p;
        const float fx = (f[0] * a.flow_scaling) * r, fy = (f[HWp] * a.flow_scaling) * r;
        const float gx = g[0], gy = g[HWp];
        const bool valid = a.event_mask[(int64_t)b * HWp + p] != 0.0f && !(gx == 0.0f && gy == 0.0f);
        const float mk = valid ? 1.0f : 0.0f;
        float e;
        if (a.metric == SNNFLOW_EM_AEE) {
            const float dx = fx - gx, dy = fy - gy;
            e = sqrtf(dx * dx + dy * dy);
        } else {
            const float fn = sqrtf(fx * fx + fy * fy), gn = sqrtf(gx * gx + gy * gy);
            const float dot = fx * gx + fy * gy;
            if (a.metric == SNNFLOW_EM_AAE) {
                e = acosf(fminf(fmaxf((fn * gn) / (dot + 0.01f), kClampLo), kClampHi));
            } else {
                const float ang = acosf(fminf(fmaxf(dot / (fn * gn + 1e-9f), kClampLo), kClampHi));
                e = ang / (fn + 1e-9f);
            }
        }
        a.err[(int64_t)b * HWp + p] = e;
        s += e * mk;
        c += mk;
    }
    if (a.sum) {
        a.sum[p] += s;
        a.count[p] += c;
    }
}

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + NT - 1) / NT); }

}  // namespace

extern "C" {

int snnflow_percentiles(const snnflow_percentiles_args* a, void* stream) {
    SelPlan p;
    if (!a || a->nplanes <= 0 || !a->x || !a->out || !make_plan(a->n, a->nq, a->q, a->fp64 != 0, p))
        SNN_FAIL(SNNFLOW_E_ARG, "percentiles: bad args (1 <= n <= 2^24, 1 <= nq <= 4, 0 <= q <= 100)");
    hipLaunchKernelGGL(k_select<false>, dim3((unsigned)a->nplanes), dim3(SEL_NT), 0, (hipStream_t)stream, a->x, a->n, p,
                       a->out);
    SNN_CHECK_LAUNCH();
    return 0;
}

int snnflow_flow_to_image(const snnflow_flow_to_image_args* a, void* stream) {
    if (!a || a->B <= 0 || a->H <= 0 || a->W <= 0 || (int64_t)a->H * a->W > SEL_MAX_N || (int64_t)a->B * a->H * a->W > ((int64_t)1 << 36) || !a->flow || !a->stats ||
        !a->out)
        SNN_FAIL(SNNFLOW_E_ARG, "flow_to_image: bad args");
    const int n = a->H * a->W;
    const double q[4] = {0.0, 100.0, 5.0, 95.0};  // min, max, p5, p95
    SelPlan p;
    if (!make_plan(n, 4, q, 1, p)) SNN_FAIL(SNNFLOW_E_ARG, "flow_to_image: bad args");
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_select<true>, dim3((unsigned)a->B), dim3(SEL_NT), 0, s, a->flow, n, p, (void*)a->stats);
    hipLaunchKernelGGL(k_flow_render, dim3(blocks_for((int64_t)a->B * n)), dim3(NT), 0, s, a->flow, a->stats, a->B, n,
                       a->has_uniform_v, a->uniform_v, a->out);
    SNN_CHECK_LAUNCH();
    return 0;
}

int snnflow_events_to_image(const snnflow_events_to_image_args* a, void* stream) {
    if (!a || a->B <= 0 || a->H <= 0 || a->W <= 0 || (int64_t)a->H * a->W > SEL_MAX_N || (int64_t)a->B * a->H * a->W > ((int64_t)1 << 36) || !a->cnt || !a->stats ||
        !a->out)
        SNN_FAIL(SNNFLOW_E_ARG, "events_to_image: bad args");
    const int n = a->H * a->W;
    const double q[2] = {1.0, 99.0};
    SelPlan p;
    if (!make_plan(n, 2, q, 0, p)) SNN_FAIL(SNNFLOW_E_ARG, "events_to_image: bad args");
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_select<false>, dim3((unsigned)(2 * a->B)), dim3(SEL_NT), 0, s, a->cnt, n, p, (void*)a->stats);
    hipLaunchKernelGGL(k_events_render, dim3(blocks_for((int64_t)a->B * n)), dim3(NT), 0, s, a->cnt, a->stats, a->B, n,
                       a->gray, a->out);
    SNN_CHECK_LAUNCH();
    return 0;
}

int snnflow_minmax_norm(const snnflow_minmax_norm_args* a, void* stream) {
    if (!a || a->B <= 0 || a->n <= 0 || a->n > SEL_MAX_N || (int64_t)a->B * a->n > ((int64_t)1 << 36) || !a->x || !a->stats || !a->out)
        SNN_FAIL(SNNFLOW_E_ARG, "minmax_norm: bad args");
    const double q[2] = {1.0, 99.0};
    SelPlan p;
    if (!make_plan(a->n, 2, q, 0, p)) SNN_FAIL(SNNFLOW_E_ARG, "minmax_norm: bad args");
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_select<false>, dim3((unsigned)a->B), dim3(SEL_NT), 0, s, a->x, a->n, p, (void*)a->stats);
    hipLaunchKernelGGL(k_minmax_render, dim3(blocks_for((int64_t)a->B * a->n)), dim3(NT), 0, s, a->x, a->stats, a->B,
                       a->n, a->out);
    SNN_CHECK_LAUNCH();
    return 0;
}

int snnflow_error_to_image(const float* err, int64_t n, uint8_t* out, void* stream) {
    if (!err || !out || n <= 0 || n > ((int64_t)1 << 36)) SNN_FAIL(SNNFLOW_E_ARG, "error_to_image: bad args");
    hipLaunchKernelGGL(k_error_render, dim3(blocks_for(n)), dim3(NT), 0, (hipStream_t)stream, err, n, out);
    SNN_CHECK_LAUNCH();
    return 0;
}

int snnflow_error_maps(const snnflow_error_maps_args* a, void* stream) {
    if (!a || a->B <= 0 || a->H <= 0 || a->W <= 0 || !a->flow || !a->gtflow || !a->event_mask || !a->dt_ratio ||
        !a->err || (a->sum == nullptr) != (a->count == nullptr) || a->metric < SNNFLOW_EM_AEE ||
        a->metric > SNNFLOW_EM_NAAE)
        SNN_FAIL(SNNFLOW_E_ARG, "error_maps: bad args");
    hipLaunchKernelGGL(k_error_maps, dim3(blocks_for((int64_t)a->H * a->W)), dim3(NT), 0, (hipStream_t)stream, *a);
    SNN_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
