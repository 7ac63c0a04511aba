// Per-step utility kernels of the training loop for gfx950: weight preparation (transposed copies and
// matrix-core fragments), the subtract-reset threshold gradient, gradient clipping, clip + Adam, and
// the reference's LIF export op.
#include <algorithm>
#include <cmath>

#include "lif_common.h"
#include "snnflow_dev.h"
#include "snnflow_host.h"

namespace {

// Matrix-core operand geometry of a KIN x NOUT 3x3 conv at run time (Bf3Geo / bf3_k).
struct FragGeo {
    int gpt, tpi, ipt, ni, nnt;
    __host__ __device__ FragGeo(int kin, int nout) {
        gpt = kin / 8;
        tpi = gpt >= 4 ? 1 : 4 / gpt;
        ipt = gpt >= 4 ? gpt / 4 : 1;
        ni = ((9 + tpi - 1) / tpi) * ipt;
        nnt = (nout + 15) / 16;
    }
    __host__ __device__ int halfs() const { return ni * nnt * 3 * 512; }
    __device__ void k(int i, int g, int& tap, int& c0) const {
        if (gpt >= 4) {
            tap = i / ipt;
            c0 = ((i % ipt) * 4 + g) * 8;
        } else {
            tap = i * tpi + g / gpt;
            c0 = (g % gpt) * 8;
        }
    }
};

// Fragment element e (chunk, n-tile, lane, j) of a KIN x NOUT conv: the three bf16 parts of
// W(tap, n, k = c0 + j) at frag[((chunk * nnt + nt) * 3 + part) * 512 + lane * 8 + j]
// (FragStage's layout, in global memory).  fwd: n = co, k = ci; !fwd (input gradient): n = ci, k = co.
__device__ inline void prep_frag(const snnflow_prep_desc& d, int e, bool fwd) {
    const int c = d.c, cin = d.cin;
    const FragGeo G(fwd ? cin : c, fwd ? c : cin);
    if (e >= G.ni * G.nnt * 512) return;
    const int j = e & 7, lane = (e >> 3) & 63, rest = e >> 9;
    const int nt = rest % G.nnt, ch = rest / G.nnt, n = nt * 16 + (lane & 15);
    int tap, c0;
    G.k(ch, lane >> 4, tap, c0);
    const int kk = c0 + j, nout = fwd ? c : cin;
    float w = 0.0f;
    if (tap < 9 && n < nout) w = fwd ? d.w[(n * cin + kk) * 9 + tap] : d.w[(kk * cin + n) * 9 + tap];
    const __bf16 h = (__bf16)w;
    const float r1 = w - (float)h;
    const __bf16 md = (__bf16)r1;
    const __bf16 lo = (__bf16)(r1 - (float)md);
    uint16_t* f = (fwd ? d.frag_fwd : d.frag_bwd) + (rest * 3) * 512 + (e & 511);
    f[0] = __builtin_bit_cast(uint16_t, h);
    f[512] = __builtin_bit_cast(uint16_t, md);
    f[1024] = __builtin_bit_cast(uint16_t, lo);
}

__global__ void k_prep_weights(DescBatch<snnflow_prep_desc> batch) {
    const snnflow_prep_desc d = batch.pick(blockIdx.y);
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int c = d.c, cin = d.cin, n = c * cin * 9;
    if (d.w && e < n) {
        const int k = e % 9, ci = (e / 9) % cin, co = e / (9 * cin);
        const float v = d.w[e];
        d.wt_fwd[(k * cin + ci) * c + co] = v;
        d.wt_bwd[(k * c + co) * cin + ci] = v;
    }
    if (d.w && d.frag_fwd) prep_frag(d, e, true);
    if (d.w && d.frag_bwd) prep_frag(d, e, false);
    if (d.threshold && e < d.thr_n) {
        const float t = d.threshold[e];
        d.threshold[e] = (t < 0.01f) ? 0.01f : t;
    }
    if (d.zero) {
        for (int64_t i = e; i < d.zero_n; i += (int64_t)gridDim.x * blockDim.x) d.zero[i] = 0.0;
    }
}

// Subtract-reset threshold gradient (include/snnflow.h snnflow_lif_theta_subtract): thread per
// float4 of the NHWC tensors, grid-stride (the channel quad of a thread is fixed), per-block
// channel totals through LDS into part[block][C]; k_lif_theta_reduce then sums the blocks' totals
// in block order (fp64) -- no atomics, so the gradient is the same on every run.
template <int C>
__global__ __launch_bounds__(NT) void k_lif_theta_subtract(const float* __restrict__ g_cur, const float* __restrict__ mem,
                                                        const float* __restrict__ thr, int64_t npix, float* part) {
    constexpr int Q = C / 4;
    __shared__ float4 lds[NT];
    const int tid = threadIdx.x, q = tid % Q;
    const float t0 = thr[4 * q], t1 = thr[4 * q + 1], t2 = thr[4 * q + 2], t3 = thr[4 * q + 3];
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    const int64_t n4 = npix * Q, stride = (int64_t)gridDim.x * NT;  // stride % Q == 0 (Q | 256)
    for (int64_t e = (int64_t)blockIdx.x * NT + tid; e < n4; e += stride) {
        const float4 g = reinterpret_cast<const float4*>(g_cur)[e];
        const float4 m = reinterpret_cast<const float4*>(mem)[e];
        acc.x += (m.x - t0 > 0.0f) ? g.x : 0.0f;
        acc.y += (m.y - t1 > 0.0f) ? g.y : 0.0f;
        acc.z += (m.z - t2 > 0.0f) ? g.z : 0.0f;
        acc.w += (m.w - t3 > 0.0f) ? g.w : 0.0f;
    }
    lds[tid] = acc;
    __syncthreads();
    if (tid < C) {
        const int qq = tid / 4, j = tid & 3;
        float s = 0.0f;
        for (int k = qq; k < NT; k += Q) {
            const float4 v = lds[k];
            s += j == 0 ? v.x : (j == 1 ? v.y : (j == 2 ? v.z : v.w));
        }
        part[(int64_t)blockIdx.x * C + tid] = s;
    }
}

__global__ __launch_bounds__(64) void k_lif_theta_reduce(const float* __restrict__ part, int nblk, int c,
                                                      float* g_theta) {
    const int ch = threadIdx.x;
    if (ch >= c) return;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += (double)part[(int64_t)b * c + ch];
    g_theta[ch] -= (float)s;
}

// torch.nn.utils.clip_grad_norm_ over the engine's flat gradient buffer in one block:
// total = ||g||_2 (fp64 accumulation, fixed order), coef = min(max_norm / (total + eps), 1),
// g *= coef (train_flow.py:265-266).
constexpr int CLIP_NT = 1024;

__global__ __launch_bounds__(CLIP_NT) void k_clip_grad_norm(float* g, int64_t n, float max_norm, float eps,
                                                          float* total_out) {
    __shared__ double part[CLIP_NT / 64];
    __shared__ float coef_s;
    // 8 guarded loads in flight per thread and round (one block: the vector is small, ~5e3..1e5
    // floats; a serial tail loop waited one memory latency per element)
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 8 * CLIP_NT) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = i + k * CLIP_NT < n ? g[i + k * CLIP_NT] : 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) s += (double)v[k] * (double)v[k];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < CLIP_NT / 64; ++w) t += part[w];
        const float total = (float)sqrt(t);
        float c = max_norm / (total + eps);
        coef_s = c < 1.0f ? c : 1.0f;
        if (total_out) total_out[0] = total;
    }
    __syncthreads();
    const float c = coef_s;
    for (int64_t j = threadIdx.x; j < n; j += 8 * CLIP_NT) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = j + k * CLIP_NT < n ? g[j + k * CLIP_NT] : 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (j + k * CLIP_NT < n) g[j + k * CLIP_NT] = v[k] * c;
    }
}

// clip_grad_norm_ + Adam (snnflow_clip_adam).  Block b owns elements [b S, (b+1) S), S =
// CLIP_PER * CLIP_NT, one round with every load issued before any math.  One block (n <= S): the norm
// pass and the step increment in the same launch.  Several blocks: k_clip_adam_norm writes per-block
// norm partials and increments the step first; every block of k_clip_adam then sums all partials in
// block order (the same value everywhere, deterministic).  Elements find their parameter tensor by a
// binary search over the LDS copy of the table (offsets ascending, host-checked); Adam as the reference
// (torch _single_tensor_adam: lerp first moment, fp64 bias corrections).
constexpr int CLIP_PER = 8, CLIP_SLICE = CLIP_PER * CLIP_NT;
static_assert(CLIP_SLICE == SNNFLOW_CLIP_ADAM_ONE_BLOCK, "one-block size");

__device__ inline double clip_sq_slice(const float* g, int64_t n, int64_t i0, int64_t i1) {
    double s = 0.0;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += (int64_t)CLIP_SLICE) {
        float v[CLIP_PER];
#pragma unroll
        for (int k = 0; k < CLIP_PER; ++k) v[k] = i + k * CLIP_NT < i1 ? g[i + k * CLIP_NT] : 0.0f;
#pragma unroll
        for (int k = 0; k < CLIP_PER; ++k) s += (double)v[k] * (double)v[k];
    }
    return s;
}

// block total of a per-thread double (all threads; result valid in thread 0)
__device__ inline double clip_block_sum(double s, double* part) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < CLIP_NT / 64; ++w) t += part[w];
    return t;
}

__global__ __launch_bounds__(CLIP_NT) void k_clip_adam_norm(snnflow_clip_adam_args a) {
    __shared__ double part[CLIP_NT / 64];
    const int64_t i0 = (int64_t)blockIdx.x * CLIP_SLICE, i1 = i0 + CLIP_SLICE < a.n ? i0 + CLIP_SLICE : a.n;
    const double t = clip_block_sum(a.max_norm > 0.0f ? clip_sq_slice(a.grad, a.n, i0, i1) : 0.0, part);
    if (threadIdx.x == 0) {
        a.scratch[blockIdx.x] = t;
        if (blockIdx.x == 0) a.step[0] = a.step[0] + 1.0f;
    }
}

__global__ __launch_bounds__(CLIP_NT) void k_clip_adam(snnflow_clip_adam_args a, int nparts) {
    // Every load of the block (step counter, gradients, parameters, both moments) is issued in one
    // round ahead of the norm reduction: the update needs nothing from the norm but the clip factor,
    // so the kernel waits for one memory latency, not three (norm pass, step counter, update).
    __shared__ double part[CLIP_NT / 64];
    __shared__ float coef_s;
    __shared__ snnflow_adam_tensor tab[SNNFLOW_ADAM_MAX_TENSORS];  // the argument table, for lookups
    if (threadIdx.x < a.ntensors) tab[threadIdx.x] = a.t[threadIdx.x];
    const bool clip = a.max_norm > 0.0f;
    const float st_in = a.step[0];
    __syncthreads();
    const int64_t lo_i = nparts ? (int64_t)blockIdx.x * CLIP_SLICE : 0;
    const int64_t hi_i = lo_i + CLIP_SLICE < a.n ? lo_i + CLIP_SLICE : a.n;  // (one block: n <= CLIP_SLICE)
    float gv[CLIP_PER], pv[CLIP_PER], mv[CLIP_PER], vv[CLIP_PER];
    float *pp[CLIP_PER], *mp[CLIP_PER], *vp[CLIP_PER];
#pragma unroll
    for (int u = 0; u < CLIP_PER; ++u) {  // gradients first: the norm waits only for them
        const int64_t i = lo_i + threadIdx.x + (int64_t)u * CLIP_NT;
        gv[u] = i < hi_i ? a.grad[i] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < CLIP_PER; ++u) {
        const int64_t i = lo_i + threadIdx.x + (int64_t)u * CLIP_NT;
        pp[u] = nullptr;
        if (i >= hi_i) continue;
        int lo = 0, hi = a.ntensors - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (tab[mid].offset <= i) lo = mid;
            else hi = mid - 1;
        }
        const int64_t j = i - tab[lo].offset;
        if (j < 0 || j >= tab[lo].numel) continue;  // a gap between tensors (not written by the engine)
        pp[u] = tab[lo].param + j;
        mp[u] = a.exp_avg + tab[lo].state_offset + j;
        vp[u] = a.exp_avg_sq + tab[lo].state_offset + j;
        pv[u] = *pp[u];
        mv[u] = *mp[u];
        vv[u] = *vp[u];
    }
    double tot = 0.0;
    if (nparts == 0) {  // one block: the norm over all n here (the same squares, the same order)
        double sq = 0.0;
        if (clip) {
#pragma unroll
            for (int u = 0; u < CLIP_PER; ++u) sq += (double)gv[u] * (double)gv[u];
        }
        tot = clip_block_sum(sq, part);
    } else if (threadIdx.x == 0 && clip) {
        for (int j = 0; j < nparts; ++j) tot += a.scratch[j];
    }
    // the step counter: incremented here (one block) or by k_clip_adam_norm (several)
    const float st = nparts == 0 ? st_in + 1.0f : st_in;
    if (threadIdx.x == 0) {
        if (clip) {
            const float total = (float)sqrt(tot);
            const float cc = a.max_norm / (total + a.clip_eps);
            coef_s = cc < 1.0f ? cc : 1.0f;
            if (a.total_out && blockIdx.x == 0) a.total_out[0] = total;
        } else {
            coef_s = 1.0f;
        }
        if (nparts == 0) a.step[0] = st;
    }
    const double step = (double)st;
    const double bc1 = 1.0 - pow(a.beta1, step), bc2 = 1.0 - pow(a.beta2, step);  // (overlaps the barrier wait)
    __syncthreads();
    const float c = coef_s;
    const float neg_step_size = (float)(-(a.lr / bc1));
    const float bc2_sqrt = (float)sqrt(bc2);
    const float w1 = (float)(1.0 - a.beta1), b2 = (float)a.beta2, w2 = (float)(1.0 - a.beta2);
    const float eps = (float)a.eps, wd = (float)a.weight_decay;
#pragma unroll
    for (int u = 0; u < CLIP_PER; ++u) {
        if (!pp[u]) continue;
        float g = gv[u];
        if (clip) {
            g = g * c;
            a.grad[lo_i + threadIdx.x + (int64_t)u * CLIP_NT] = g;  // clip_grad_norm_ scales the gradients in place
        }
        float p = pv[u];
        if (wd != 0.0f) g = g + wd * p;
        const float m = mv[u] + w1 * (g - mv[u]);  // lerp, weight < 0.5
        const float v = vv[u] * b2 + w2 * g * g;
        const float denom = sqrtf(v) / bc2_sqrt + eps;
        p = p + neg_step_size * (m / denom);
        *mp[u] = m;
        *vp[u] = v;
        *pp[u] = p;
    }
}

__global__ void k_lif_export(const float* __restrict__ x, const float* __restrict__ mem, const float* __restrict__ beta,
                             const float* __restrict__ thr, int64_t total, int C, int HW, float* spk, float* mout) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)((i / HW) % C);
        const float m = beta[c] * mem[i] + x[i];
        const bool s = m >= thr[c];
        spk[i] = s ? 1.0f : 0.0f;
        mout[i] = s ? 0.0f : m;
    }
}

}  // namespace

extern "C" {

int snnflow_frag_halfs(int c, int cin) {
    if (cin != c || c <= 0 || c % 8 != 0 || c > 64) return 0;
    return FragGeo(c, c).halfs();
}

int snnflow_prep_weights_batch(const snnflow_prep_desc* d, int n, void* stream) {
    if (!d || n <= 0 || n > SNNFLOW_MAX_BATCH) SNN_FAIL(SNNFLOW_E_ARG, "prep_weights_batch: bad count");
    DescBatch<snnflow_prep_desc> batch = {};
    int maxe = 1;
    for (int i = 0; i < n; ++i) {
        const snnflow_prep_desc& x = d[i];
        if ((x.w && (x.c <= 0 || x.cin <= 0 || !x.wt_fwd || !x.wt_bwd)) || (!x.w && !x.threshold && !x.zero) ||
            (x.threshold && x.thr_n <= 0) || (x.zero && x.zero_n < 0))
            SNN_FAIL(SNNFLOW_E_ARG, "prep_weights_batch: bad descriptor");
        if ((x.frag_fwd || x.frag_bwd) && (!x.w || snnflow_frag_halfs(x.c, x.cin) == 0))
            SNN_FAIL(SNNFLOW_E_ARG, "prep_weights_batch: fragments need cin == c, c % 8 == 0");
        batch.d[i] = x;
        if (x.w && x.c * x.cin * 9 > maxe) maxe = x.c * x.cin * 9;
        if (x.frag_fwd || x.frag_bwd) {
            const int fe = snnflow_frag_halfs(x.c, x.cin) / 3;
            if (fe > maxe) maxe = fe;
        }
        if (x.threshold && x.thr_n > maxe) maxe = x.thr_n;
        if (x.zero) maxe = std::max(maxe, (int)std::min<int64_t>(x.zero_n, 65536));  // grid-stride beyond
    }
    hipLaunchKernelGGL(k_prep_weights, dim3((maxe + 255) / 256, n), dim3(256), 0, (hipStream_t)stream, batch);
    SNN_CHECK_LAUNCH();
    return 0;
}

int snnflow_prep_weights(const float* w, int c, int cin, float* wt_fwd, float* wt_bwd, float* threshold,
                         void* stream) {
    if (c <= 0 || cin <= 0 || (w && (!wt_fwd || !wt_bwd)) || (!w && !threshold))
        SNN_FAIL(SNNFLOW_E_ARG, "prep_weights: bad args");
    snnflow_prep_desc d = {w, c, cin, wt_fwd, wt_bwd, threshold, c, nullptr, nullptr, nullptr, 0};
    return snnflow_prep_weights_batch(&d, 1, stream);
}

int snnflow_lif_theta_subtract(const float* g_cur, const float* mem, const float* thr, int64_t npix, int c,
                               float* g_theta, float* scratch, void* stream) {
    if (!g_cur || !mem || !thr || !g_theta || !scratch || npix <= 0)
        SNN_FAIL(SNNFLOW_E_ARG, "lif_theta_subtract: bad args");
    const int64_t n4 = npix * (c / 4);
    int64_t g = (n4 + NT - 1) / NT;
    if (g > SNNFLOW_THETA_BLOCKS) g = SNNFLOW_THETA_BLOCKS;
    const dim3 grid((unsigned)g), block(NT);
    const hipStream_t s = (hipStream_t)stream;
    switch (c) {
        case 4: hipLaunchKernelGGL(k_lif_theta_subtract<4>, grid, block, 0, s, g_cur, mem, thr, npix, scratch); break;
        case 8: hipLaunchKernelGGL(k_lif_theta_subtract<8>, grid, block, 0, s, g_cur, mem, thr, npix, scratch); break;
        case 16: hipLaunchKernelGGL(k_lif_theta_subtract<16>, grid, block, 0, s, g_cur, mem, thr, npix, scratch); break;
        case 32: hipLaunchKernelGGL(k_lif_theta_subtract<32>, grid, block, 0, s, g_cur, mem, thr, npix, scratch); break;
        default: SNN_FAIL(SNNFLOW_E_CHANNELS, "lif_theta_subtract: c must be 4, 8, 16 or 32");
    }
    SNN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_lif_theta_reduce, dim3(1), dim3(64), 0, s, scratch, (int)g, c, g_theta);
    SNN_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"

namespace {
// Large-vector form (the U-Net's ~20 M parameters): per-block fp64 partial sums of squares in a
// fixed grid order, one block finishing the norm and the coefficient, a grid scaling the vector.
constexpr int CLIP2_NB = 512;

__global__ __launch_bounds__(256) void k_clip_partial(const float* __restrict__ g, int64_t n, double* partials) {
    __shared__ double part[4];
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double v = g[i];
        s += v * v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

__global__ void k_clip_coef(const double* partials, int nb, float max_norm, float eps, float* total_out, float* coef) {
    if (threadIdx.x != 0) return;
    double t = 0.0;
    for (int i = 0; i < nb; ++i) t += partials[i];
    const float total = (float)sqrt(t);
    const float c = max_norm / (total + eps);
    coef[0] = c < 1.0f ? c : 1.0f;
    if (total_out) total_out[0] = total;
}

__global__ __launch_bounds__(256) void k_clip_scale(float* __restrict__ g, int64_t n, const float* coef) {
    const float c = coef[0];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) g[i] = g[i] * c;
}
}  // namespace

extern "C" {

int snnflow_clip_grad_norm_large(float* g, int64_t n, float max_norm, float eps, float* total_out, double* scratch,
                                 void* stream) {
    if (!g || n < 0 || !scratch) SNN_FAIL(SNNFLOW_E_ARG, "clip_grad_norm_large: bad args");
    const hipStream_t s = (hipStream_t)stream;
    int64_t nb = (n + 255) / 256;
    if (nb > CLIP2_NB) nb = CLIP2_NB;
    if (nb < 1) nb = 1;
    float* coef = reinterpret_cast<float*>(scratch + CLIP2_NB);
    hipLaunchKernelGGL(k_clip_partial, dim3((unsigned)nb), dim3(256), 0, s, g, n, scratch);
    hipLaunchKernelGGL(k_clip_coef, dim3(1), dim3(64), 0, s, scratch, (int)nb, max_norm, eps, total_out, coef);
    int64_t gs = (n + 255) / 256;
    if (gs > 4096) gs = 4096;
    if (gs < 1) gs = 1;
    hipLaunchKernelGGL(k_clip_scale, dim3((unsigned)gs), dim3(256), 0, s, g, n, coef);
    SNN_CHECK_LAUNCH();
    return 0;
}

int snnflow_clip_adam(const snnflow_clip_adam_args* a, void* stream) {
    if (!a || !a->grad || !a->exp_avg || !a->exp_avg_sq || !a->step || a->n < 0 || a->n > SNNFLOW_CLIP_ADAM_MAX_N ||
        a->ntensors < 0 || a->ntensors > SNNFLOW_ADAM_MAX_TENSORS)
        SNN_FAIL(SNNFLOW_E_ARG, "clip_adam: bad args (n <= SNNFLOW_CLIP_ADAM_MAX_N, ntensors <= SNNFLOW_ADAM_MAX_TENSORS)");
    for (int k = 0; k < a->ntensors; ++k) {
        const snnflow_adam_tensor& t = a->t[k];
        if (!t.param || t.offset < 0 || t.state_offset < 0 || t.numel < 0 || t.offset + t.numel > a->n)
            SNN_FAIL(SNNFLOW_E_ARG, "clip_adam: tensor range outside the flat buffer");
        if (k > 0 && t.offset < a->t[k - 1].offset + a->t[k - 1].numel)
            SNN_FAIL(SNNFLOW_E_ARG, "clip_adam: tensors must be in ascending, non-overlapping gradient order");
    }
    const hipStream_t s = (hipStream_t)stream;
    if (a->n <= CLIP_SLICE) {
        hipLaunchKernelGGL(k_clip_adam, dim3(1), dim3(CLIP_NT), 0, s, *a, 0);
    } else {
        const int nb = (int)((a->n + CLIP_SLICE - 1) / CLIP_SLICE);
        if (!a->scratch || nb > SNNFLOW_CLIP_SCRATCH) SNN_FAIL(SNNFLOW_E_ARG, "clip_adam: scratch needed above SNNFLOW_CLIP_ADAM_ONE_BLOCK");
        hipLaunchKernelGGL(k_clip_adam_norm, dim3(nb), dim3(CLIP_NT), 0, s, *a);
        hipLaunchKernelGGL(k_clip_adam, dim3(nb), dim3(CLIP_NT), 0, s, *a, nb);
    }
    SNN_CHECK_LAUNCH();
    return 0;
}

int snnflow_clip_grad_norm(float* g, int64_t n, float max_norm, float eps, float* total_out, void* stream) {
    if (!g || n < 0) SNN_FAIL(SNNFLOW_E_ARG, "clip_grad_norm: bad args");
    hipLaunchKernelGGL(k_clip_grad_norm, dim3(1), dim3(CLIP_NT), 0, (hipStream_t)stream, g, n, max_norm, eps, total_out);
    SNN_CHECK_LAUNCH();
    return 0;
}

int snnflow_lif_export(const float* x, const float* mem, const float* beta, const float* thr, int N, int C, int HW,
                       float* spk, float* mem_out, void* stream) {
    if (!x || !mem || !beta || !thr || !spk || !mem_out || N < 0 || C <= 0 || HW <= 0)
        SNN_FAIL(SNNFLOW_E_ARG, "lif_export: bad args");
    const int64_t total = (int64_t)N * C * HW;
    if (total == 0) return 0;
    int g = elem_grid(total);
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(k_lif_export, dim3(g), dim3(NT), 0, (hipStream_t)stream, x, mem, beta, thr, total, C, HW, spk,
                       mem_out);
    SNN_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
