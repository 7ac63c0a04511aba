// K x K convolutions (K = 1, 5, 7; stride 1, pad K / 2) of the LIFFireNet cells for gfx950: the
// lif_in = 0 halves of snnflow_conv_fwd / snnflow_layer_bwd and the deferred weight gradient, for
// the cell-wise path of a model built with model.kernel_size != 3 (include/snnflow.h:
// snnflow_convk_fwd, snnflow_layerk_bwd, snnflow_wgradk, snnflow_prep_weights_k).
//
// One block of NT threads per 8 x 32 pixel tile, as in the 3 x 3 kernels, so snnflow_conv_blocks(),
// the slab rows and snnflow_slab_reduce serve unchanged; the halo is K / 2 pixels.  A halo tile of
// all channels does not fit in LDS at K = 7, C = 32 (14 x 38 pixels x 32 channels x 4 B = 68 KB, two
// of them for a recurrent cell), so every kernel walks the reduction channels in chunks of at most
// 16 and the two convolutions of a recurrent cell in turn over one staging tile (42.5 KB at K = 7).
//
// Arithmetic: exact f32 throughout, for arbitrary inputs (a standalone cell takes any values, not
// only spikes).  C x C convolutions at C >= 8 run on v_mfma_f32_16x16x4_f32 (f32 operands, f32
// accumulation); the narrow event inputs (cin 1, 2, 4, 5) and C = 4 run on vector FMAs with
// wave-uniform (scalar) weight loads.  The weight gradient reduces over the 256 pixels of the tile,
// which is long for every channel pair, so it runs on the matrix cores for all of them.
#include <type_traits>

#include "lif_common.h"
#include "snnflow_dev.h"
#include "snnflow_host.h"
#include "snnflow_tile.h"

namespace {

// Halo tile of a K x K convolution around the 8 x 32 pixel tile.
template <int K>
struct KGeo {
    static_assert(K % 2 == 1, "odd kernel sizes");
    static constexpr int R = K / 2, HH = TH + 2 * R, HW = TW + 2 * R, HN = HH * HW;
};

// Reduction channels staged at a time.
template <int C>
struct Chunk { static constexpr int v = C >= 16 ? 16 : C; };

constexpr int kVecPad = 5;  // pixel stride of the narrow-input tile (cin <= 5; odd: conflict-free scalar reads)

constexpr int cmax(int a, int b) { return a > b ? a : b; }

// LDS pool of the forward / backward kernels: the staging tile of one channel chunk, the narrow-input
// tile, or the matrix-core results [NT][Pad<C>] on their way back to one thread per pixel.
template <int K, int C>
struct PoolFloats {
    static constexpr int v = cmax(cmax(KGeo<K>::HN * Pad<Chunk<C>::v>::v, KGeo<K>::HN * kVecPad), C >= 8 ? NT * Pad<C>::v : 4);
};

// Strided input channels [c0, c0 + CH) of the halo -> tile[p * P + cl]; zero past cin and outside the image.
template <int K, int CH, int P>
__device__ void stage_x(const float* __restrict__ x, int64_t sb, int64_t sc, int64_t sh, int64_t sw, const Tile& tl,
                        int H, int W, int c0, int cin, float* tile) {
    using G = KGeo<K>;
    const float* xb = x + (int64_t)tl.b * sb;
    const bool cl_fast = sc == 1;  // channels-last: consecutive threads take consecutive channels
    for (int e = threadIdx.x; e < G::HN * CH; e += NT) {
        const int p = cl_fast ? e / CH : e % G::HN, cl = cl_fast ? e % CH : e / G::HN;
        const int r = p / G::HW, cc = p - r * G::HW;
        const int h = tl.h0 + r - G::R, w = tl.w0 + cc - G::R, ci = c0 + cl;
        tile[p * P + cl] = (ci < cin && in_image(h, w, H, W)) ? xb[ci * sc + h * sh + w * sw] : 0.0f;
    }
}

// Channels [c0, c0 + CH) of a dense NHWC tensor of C channels -> tile[p * Pad<CH> + cl].
template <int K, int CH>
__device__ void stage_nhwc_k(const float* __restrict__ s, const Tile& tl, int H, int W, int C, int c0, float* tile) {
    using G = KGeo<K>;
    static_assert(CH % 4 == 0, "vector staging");
    constexpr int P = Pad<CH>::v, Q = CH / 4;
    for (int e = threadIdx.x; e < G::HN * Q; e += NT) {
        const int p = e / Q, q = e - p * Q;
        const int r = p / G::HW, cc = p - r * G::HW;
        const int h = tl.h0 + r - G::R, w = tl.w0 + cc - G::R;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (in_image(h, w, H, W))
            v = *reinterpret_cast<const float4*>(s + (((int64_t)tl.b * H + h) * W + w) * C + c0 + 4 * q);
        *reinterpret_cast<float4*>(tile + p * P + 4 * q) = v;
    }
}

// K x K convolution of one output pixel from the narrow-input tile; wt: [K][K][CIN][C] (scalar loads).
template <int K, int CIN, int C, int P>
__device__ inline void vec_conv(const float* tile, const float* __restrict__ wt, int ty, int tx, float (&acc)[C]) {
    using G = KGeo<K>;
#pragma unroll 1
    for (int ky = 0; ky < K; ++ky) {
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
            const float* xp = tile + ((ty + ky) * G::HW + tx + kx) * P;
            const cfloat_ptr wk = as_const(wt) + (ky * K + kx) * CIN * C;
#pragma unroll
            for (int ci = 0; ci < CIN; ++ci) {
                const float xs = xp[ci];
#pragma unroll
                for (int co = 0; co < C; ++co) acc[co] = fmaf(wk[ci * C + co], xs, acc[co]);
            }
        }
    }
}

// Transposed K x K convolution (input gradient) of one pixel over the output channels [cb, cb + CH)
// held in the gradient tile gt[p * P + co - cb]; wd: [K][K][C][CIN] (scalar loads).
//   gx[ci] += sum_{ky,kx,co} w[co][ci][ky][kx] * G[h + R - ky][w + R - kx][co]
template <int K, int CIN, int C, int CH, int P>
__device__ inline void vec_dgrad(const float* gt, const float* __restrict__ wd, int cb, int ty, int tx, float (&gx)[kVecPad]) {
    using G = KGeo<K>;
    static_assert(CIN <= kVecPad && CH % 4 == 0, "narrow inputs");
#pragma unroll 1
    for (int ky = 0; ky < K; ++ky) {
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
            const float* gp = gt + ((ty + 2 * G::R - ky) * G::HW + tx + 2 * G::R - kx) * P;
            const cfloat_ptr wk = as_const(wd) + ((ky * K + kx) * C + cb) * CIN;
#pragma unroll
            for (int co = 0; co < CH; co += 4) {
                const float4 v = *reinterpret_cast<const float4*>(gp + co);
                const float gs[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int ci = 0; ci < CIN; ++ci) gx[ci] = fmaf(wk[(co + j) * CIN + ci], gs[j], gx[ci]);
            }
        }
    }
}

// Implicit-GEMM K x K convolution of the block's 256 pixels on v_mfma_f32_16x16x4_f32, one chunk of
// CH reduction channels [kb, kb + CH) of C:
//   acc[p][n] += sum_{tap, k} src[halo(p, tap)][k - kb] * wB[tap][n][k]
// M = 16 consecutive pixels of a tile row (16 M-tiles, four per wave), N = the C output channels in
// 16-wide tiles (C = 8 pads with zero weights).  In step j lane group g = lane >> 4 supplies channel
// E g + j of the chunk for both operands (a permutation of k, so each lane reads E consecutive
// channels with one vector load).  wB: global, [K * K][C][C], k fastest.  FLIP: the transposed
// convolution (halo offset K - 1 - ky, K - 1 - kx; wB then holds the forward-layout weights).
template <int C>
struct AccK {
    static constexpr int NNT = (C + 15) / 16;
    f32x4 v[4][NNT];
    __device__ inline void zero() {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < NNT; ++j) v[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
};

template <int K, int CH, int C, bool FLIP>
__device__ void mfma_chunk(const float* src, const float* __restrict__ wB, int kb, AccK<C>& acc) {
    using G = KGeo<K>;
    static_assert(CH == 8 || CH == 16, "matrix-core chunks of 8 or 16 channels");
    constexpr int E = CH / 4, P = Pad<CH>::v, NNT = AccK<C>::NNT;
    const int lane = threadIdx.x & 63, m = lane & 15, g = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
#pragma unroll 1
    for (int ky = 0; ky < K; ++ky) {
        // one kernel row of the chunk (K CH terms) in its own accumulators, added to the running sums after:
        // the rounding error of a K K C-term sum (1568 terms at K = 7, C = 32) grows with the length of
        // the longest chain, and a single chain measured three times the CPU reference's error at C = 16
        AccK<C> part;
        part.zero();
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
            const int tap = ky * K + kx;
            const int oy = FLIP ? K - 1 - ky : ky, ox = FLIP ? K - 1 - kx : kx;
            float b[NNT][E];
#pragma unroll
            for (int nt = 0; nt < NNT; ++nt) {
                const int n = nt * 16 + m;
                const bool ok = n < C;
                float v[E];
                ld_vec<E>(wB + (int64_t)(tap * C + (ok ? n : 0)) * C + kb + g * E, v);
#pragma unroll
                for (int j = 0; j < E; ++j) b[nt][j] = ok ? v[j] : 0.0f;
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const int T = wv * 4 + mt, row = T >> 1, c0 = (T & 1) * 16;
                float a[E];
                ld_vec<E>(src + ((row + oy) * G::HW + c0 + m + ox) * P + g * E, a);
#pragma unroll
                for (int j = 0; j < E; ++j)
#pragma unroll
                    for (int nt = 0; nt < NNT; ++nt)
                        part.v[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[nt][j], part.v[mt][nt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < NNT; ++nt) acc.v[mt][nt] = acc.v[mt][nt] + part.v[mt][nt];
    }
}

// Accumulators (lane: pixels 4g .. 4g + 3 of its M-tile, channel n = lane & 15) -> out[NT][Pad<C>].
template <int C>
__device__ void acc_store(const AccK<C>& acc, float* out) {
    constexpr int PO = Pad<C>::v;
    const int lane = threadIdx.x & 63, m = lane & 15, g = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const int T = wv * 4 + mt, row = T >> 1, c0 = (T & 1) * 16;
#pragma unroll
        for (int nt = 0; nt < AccK<C>::NNT; ++nt) {
            const int n = nt * 16 + m;
            if (n < C) {
#pragma unroll
                for (int r = 0; r < 4; ++r) out[(row * TW + c0 + g * 4 + r) * PO + n] = acc.v[mt][nt][r];
            }
        }
    }
}

// One C x C convolution of the block through the staging tile, chunk by chunk; the result comes
// back as this thread's pixel, all C channels.  load(cb): stages channels [cb, cb + CH) into pool.
template <int K, int C, bool FLIP, typename Load>
__device__ void mfma_conv(float* pool, const float* __restrict__ wB, float (&out)[C], Load&& load) {
    constexpr int CH = Chunk<C>::v, PC = Pad<C>::v;
    AccK<C> acc;
    acc.zero();
    for (int cb = 0; cb < C; cb += CH) {
        __syncthreads();  // the pool's previous readers
        load(cb);
        __syncthreads();
        mfma_chunk<K, CH, C, FLIP>(pool, wB, cb, acc);
    }
    __syncthreads();
    acc_store<C>(acc, pool);
    __syncthreads();
    const float* ol = pool + (int)threadIdx.x * PC;
#pragma unroll
    for (int c = 0; c < C; c += 4) {
        const float4 v = *reinterpret_cast<const float4*>(ol + c);
        out[c] = v.x; out[c + 1] = v.y; out[c + 2] = v.z; out[c + 3] = v.w;
    }
}

// ---------------------------------------------------------------------------
// Forward: y = ff(x) [+ rec(s_prev)] (pre-BN, NHWC) [+ the BatchNorm batch sums]
// FFM: cin == C >= 8 (the ff conv on the matrix cores); else cin in {1, 2, 4, 5} (or C = 4) on vector FMAs.
// ---------------------------------------------------------------------------
template <int K, int C, bool FFM, bool REC>
__global__ __launch_bounds__(NT) void k_convk_fwd(snnflow_conv_fwd_args a) {
    constexpr int CH = Chunk<C>::v, PCH = Pad<CH>::v;
    __shared__ __attribute__((aligned(16))) float pool[PoolFloats<K, C>::v];
    const int tid = threadIdx.x, ty = tid / TW, tx = tid - ty * TW;
    const int H = a.H, W = a.W;
    const Grid g = hw_grid();
    const Tile tl = block_tile(H, W, g);

    float y[C];
#pragma unroll
    for (int co = 0; co < C; ++co) y[co] = 0.0f;
    if constexpr (FFM) {
        mfma_conv<K, C, false>(pool, a.wt_ff_t, y, [&](int cb) {
            stage_x<K, CH, PCH>(a.x, a.xs_b, a.xs_c, a.xs_h, a.xs_w, tl, H, W, cb, C, pool);
        });
    } else {
        stage_x<K, kVecPad, kVecPad>(a.x, a.xs_b, a.xs_c, a.xs_h, a.xs_w, tl, H, W, 0, a.cin, pool);
        __syncthreads();
        switch (a.cin) {  // (block-uniform)
            case 1: vec_conv<K, 1, C, kVecPad>(pool, a.wt_ff, ty, tx, y); break;
            case 2: vec_conv<K, 2, C, kVecPad>(pool, a.wt_ff, ty, tx, y); break;
            case 4: vec_conv<K, 4, C, kVecPad>(pool, a.wt_ff, ty, tx, y); break;
            default: vec_conv<K, 5, C, kVecPad>(pool, a.wt_ff, ty, tx, y); break;
        }
    }
    if constexpr (REC) {
        if (a.s_prev != nullptr) {
            float r[C];
#pragma unroll
            for (int co = 0; co < C; ++co) r[co] = 0.0f;
            if constexpr (C >= 8) {
                mfma_conv<K, C, false>(pool, a.wt_rec_t, r,
                                       [&](int cb) { stage_nhwc_k<K, CH>(a.s_prev, tl, H, W, C, cb, pool); });
            } else {
                __syncthreads();
                stage_nhwc_k<K, C>(a.s_prev, tl, H, W, C, 0, pool);
                __syncthreads();
                vec_conv<K, C, C, Pad<C>::v>(pool, a.wt_rec, ty, tx, r);
            }
#pragma unroll
            for (int co = 0; co < C; ++co) y[co] = y[co] + r[co];  // ff + rec (SNNtorch_spiking_submodules.py:540)
        }
    }
    zero_consumed(a.zero0, a.zero1, a.zero_n, g);

    const int h = tl.h0 + ty, w = tl.w0 + tx;
    const bool in = (h < H) && (w < W);
    if (in) {
        float* yp = a.y + (((int64_t)tl.b * H + h) * W + w) * C;
#pragma unroll
        for (int co = 0; co < C; co += 4)
            *reinterpret_cast<float4*>(yp + co) = make_float4(y[co], y[co + 1], y[co + 2], y[co + 3]);
    }
    if (a.acc) {  // real pixels only: the tile padding adds zeros
        float v[2 * C];
#pragma unroll
        for (int co = 0; co < C; ++co) {
            const float yy = in ? y[co] : 0.0f;
            v[co] = yy;
            v[C + co] = yy * yy;
        }
        block_atomic_sum<2 * C>(v, acc_shard(a.acc, 2 * C, g.bid));
    }
}

// ---------------------------------------------------------------------------
// Backward: block 0 finishes the layer's neuron / BatchNorm parameter gradients and stores the
// BN-backward coefficients; every block forms G = BN-backward(g_cur, y) on its tile with the halo,
// chunk by chunk, and the transposed convolutions give g_x and the spike half of g_state_prev.
// ---------------------------------------------------------------------------
template <int K, int C, bool FFM, bool REC>
__global__ __launch_bounds__(NT) void k_layerk_bwd(snnflow_layer_bwd_args a) {
    using G = KGeo<K>;
    constexpr int CH = Chunk<C>::v, PCH = Pad<CH>::v;
    constexpr int NSUM = SNNFLOW_BWD_ACC(C), NBN = 2 * C, NL = NSUM - NBN;
    __shared__ __attribute__((aligned(16))) float pool[PoolFloats<K, C>::v];
    __shared__ BnBwdLds bnp[C];
    __shared__ double sums[NSUM];
    const int tid = threadIdx.x, ty = tid / TW, tx = tid - ty * TW;
    const int H = a.H, W = a.W;
    const Grid g = hw_grid();
    const Tile tl = block_tile(H, W, g);
    const bool lead = g.bid == 0;
    const double N = (double)a.B * H * W;
    const float nf = (float)N;

    // block 0's inputs of the parameter gradients, every load before any store
    float mean = 0.f, inv = 0.f, gamma = 0.f, be = 0.f, o0 = 0.f, o1 = 0.f, o2 = 0.f, o3 = 0.f;
    if (tid < C) {
        mean = a.stats[tid];
        inv = a.stats[C + tid];
        gamma = a.n.bn_weight[tid];
        if (lead) {
            be = a.n.beta[tid];
            if (a.accumulate) {
                o0 = a.ng.bn_weight[tid]; o1 = a.ng.bn_bias[tid]; o2 = a.ng.threshold[tid]; o3 = a.ng.beta[tid];
            }
        }
    }
    // every block needs the 2C BatchNorm sums; the other neuron-gradient sums only block 0
    acc_gather<NBN>(a.acc_in, NSUM, sums);
    if (lead) acc_gather<NL>(a.acc_in + NBN, NSUM, sums + NBN);  // (block-uniform: barriers inside)
    if (tid < C) {
        if (lead) {
            // gamma = dotp * invstd, bias = sum g, theta = (membrane-output part) - sum g, beta = sum g m'
            // on 0 <= beta <= 1 (torch batch_norm_cpu_backward; snntorch Leaky; clamp backward)
            const double gsum = sums[tid], dotp = sums[C + tid], gbm = sums[2 * C + tid];
            a.ng.bn_weight[tid] = o0 + (float)(dotp * (double)inv);
            a.ng.bn_bias[tid] = o1 + (float)gsum;
            a.ng.threshold[tid] = o2 + (float)(sums[3 * C + tid] - gsum);
            a.ng.beta[tid] = o3 + ((be >= 0.0f && be <= 1.0f) ? (float)gbm : 0.0f);
        }
        BnBwdLds c;
        c.mean = mean;
        c.inv = inv;
        c.w = gamma;
        if (a.n.bn_train) {
            // torch batch_norm_cpu_backward: k = dotp*invstd*invstd/n, grad_mean = sum/n
            c.k = (float)sums[C + tid] * inv * inv / nf;
            c.gm = (float)(sums[tid] / N);
        } else {
            c.k = 0.0f;
            c.gm = 0.0f;
        }
        bnp[tid] = c;
        if (lead && a.bnc_out) {
            a.bnc_out[tid] = c.gm;
            a.bnc_out[C + tid] = c.k;
        }
    }
    __syncthreads();
    zero_consumed(a.zero0, a.zero1, a.zero_n, g);

    const bool do_x = a.g_x != nullptr && a.wt_bwd_ff != nullptr;
    const bool do_r = REC && a.g_state_prev != nullptr;
    if (!do_x && !do_r) return;  // (block-uniform)
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    // G = dL/dy of channels [cb, cb + CH) on the halo tile, zero outside the image
    auto stage_g = [&](int cb) {
        constexpr int Q = CH / 4;
        for (int e = tid; e < G::HN * Q; e += NT) {
            const int p = e / Q, q = e - p * Q;
            const int r = p / G::HW, cc = p - r * G::HW;
            const int h = tl.h0 + r - G::R, w = tl.w0 + cc - G::R;
            float4 out = z4;
            if (in_image(h, w, H, W)) {
                const int64_t k = ((((int64_t)tl.b * H + h) * W + w) * C + cb) / 4 + q;
                out = bn_bwd4(reinterpret_cast<const float4*>(a.g_cur)[k], reinterpret_cast<const float4*>(a.y)[k],
                              bnp + cb + 4 * q);
            }
            *reinterpret_cast<float4*>(pool + p * PCH + 4 * q) = out;
        }
    };
    const int h = tl.h0 + ty, w = tl.w0 + tx;
    const bool in = (h < H) && (w < W);

    if (do_x) {
        float* gb = a.g_x + (int64_t)tl.b * a.gxs_b + h * a.gxs_h + w * a.gxs_w;
        if constexpr (FFM) {
            float gx[C];
            mfma_conv<K, C, true>(pool, a.wt_fwd_ff, gx, stage_g);
            if (in) {
#pragma unroll
                for (int ci = 0; ci < C; ++ci) gb[ci * a.gxs_c] = gx[ci];
            }
        } else {
            float gx[kVecPad] = {0.f, 0.f, 0.f, 0.f, 0.f};
            for (int cb = 0; cb < C; cb += CH) {
                __syncthreads();
                stage_g(cb);
                __syncthreads();
                switch (a.cin) {  // (block-uniform)
                    case 1: vec_dgrad<K, 1, C, CH, PCH>(pool, a.wt_bwd_ff, cb, ty, tx, gx); break;
                    case 2: vec_dgrad<K, 2, C, CH, PCH>(pool, a.wt_bwd_ff, cb, ty, tx, gx); break;
                    case 4: vec_dgrad<K, 4, C, CH, PCH>(pool, a.wt_bwd_ff, cb, ty, tx, gx); break;
                    default: vec_dgrad<K, 5, C, CH, PCH>(pool, a.wt_bwd_ff, cb, ty, tx, gx); break;
                }
            }
            if (in) {
#pragma unroll
                for (int ci = 0; ci < kVecPad; ++ci)
                    if (ci < a.cin) gb[ci * a.gxs_c] = gx[ci];
            }
        }
    }
    if constexpr (REC) {
        if (do_r) {
            float gr[C];
            if constexpr (C >= 8) {
                mfma_conv<K, C, true>(pool, a.wt_fwd_rec, gr, stage_g);
            } else {
                float g5[kVecPad] = {0.f, 0.f, 0.f, 0.f, 0.f};
                __syncthreads();
                stage_g(0);
                __syncthreads();
                vec_dgrad<K, C, C, CH, PCH>(pool, a.wt_bwd_rec, 0, ty, tx, g5);
#pragma unroll
                for (int c = 0; c < C; ++c) gr[c] = g5[c];
            }
            if (in) {
                const int64_t plane = (int64_t)a.B * H * W * C;
                float* gsp = a.g_state_prev + (((int64_t)tl.b * H + h) * W + w) * C;
#pragma unroll
                for (int c = 0; c < C; c += 4) {
                    if (a.zero_mem_half) *reinterpret_cast<float4*>(gsp + c) = z4;
                    *reinterpret_cast<float4*>(gsp + plane + c) = make_float4(gr[c], gr[c + 1], gr[c + 2], gr[c + 3]);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Weight gradients: dW[co][ci][tap] = sum_t sum_p G_t[p][co] src_t[p + tap][ci] with src = x (ff) or
// s_prev (rec), per tile into the block's slab row ([c * cin * K * K], the weight's own order).
// v_mfma_f32_16x16x4_f32 with M = 16 output channels (A = G^T from the interior tile), N = 16 input
// channels (B from the halo tile), K = 4 tile pixels per instruction (lane group g: pixel 4 s + g).
// One (conv, co-tile, ci-tile) at a time: its K * K taps are dealt to the four waves, the
// accumulators live across the time steps, and each slab element has one owner lane and one
// summation order: the gradients are the same bits on every run.
// Channel counts are run-time values here (zero-padded to the 16-wide tiles).
// ---------------------------------------------------------------------------
typedef const __attribute__((address_space(4))) snnflow_wgrad_args* cwgradk_ptr;

template <int K>
__global__ __launch_bounds__(NT) void k_wgradk(snnflow_wgrad_args) {
    using G = KGeo<K>;
    constexpr int KK = K * K, NTAP = (KK + 3) / 4, P = Pad<16>::v;
    __shared__ __attribute__((aligned(16))) float Gi[NT * P];
    __shared__ __attribute__((aligned(16))) float X[G::HN * P];
    __shared__ BnBwdLds coef[16];
    // the step table stays in the kernarg segment (scalar loads)
    const cwgradk_ptr ap = (cwgradk_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    const int tid = threadIdx.x, lane = tid & 63, m = lane & 15, g4 = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H = ap->H, W = ap->W, C = ap->c, CIN = ap->cin, nsteps = ap->nsteps, accumulate = ap->accumulate;
    const Tile tl = block_tile(H, W);
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const int nconv = ap->rec ? 2 : 1;
    for (int conv = 0; conv < nconv; ++conv) {
        const int SC = conv ? C : CIN;  // input channels of this convolution
        float* slab = (conv ? ap->slab_rec : ap->slab_ff) + (int64_t)blockIdx.x * ((int64_t)C * SC * KK);
        for (int cot = 0; cot * 16 < C; ++cot) {
            for (int cit = 0; cit * 16 < SC; ++cit) {
                f32x4 acc[NTAP];
#pragma unroll
                for (int i = 0; i < NTAP; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                for (int t = 0; t < nsteps; ++t) {
                    const float* src = conv ? ap->steps[t].s_prev : ap->steps[t].x;
                    if (src == nullptr) continue;  // zero previous state (block-uniform)
                    __syncthreads();  // the previous step's readers of coef, Gi, X
                    if (tid < 16) {
                        const int ch = cot * 16 + tid;
                        BnBwdLds k = {0.f, 1.f, 0.f, 0.f, 1.f};  // no BatchNorm: G = g_cur
                        const float* st = ap->steps[t].stats;
                        if (st && ch < C) {
                            const float* bc = ap->steps[t].bnc;
                            k.mean = st[ch];
                            k.inv = st[C + ch];
                            k.gm = bc[ch];
                            k.k = bc[C + ch];
                            k.w = ap->bn_weight[ch];
                        }
                        coef[tid] = k;
                    }
                    __syncthreads();
                    // G of output channels [16 cot, 16 cot + 16) on the tile interior (zero outside the image / past C)
                    const float* gc = ap->steps[t].g_cur;
                    const float* yy = ap->steps[t].y;
                    for (int e = tid; e < NT * 4; e += NT) {
                        const int p = e >> 2, q = e & 3, ch0 = cot * 16 + 4 * q;
                        const int h = tl.h0 + (p >> 5), w = tl.w0 + (p & 31);
                        float4 out = z4;
                        if (ch0 < C && h < H && w < W) {
                            const int64_t k = ((((int64_t)tl.b * H + h) * W + w) * C + ch0) / 4;
                            out = bn_bwd4(reinterpret_cast<const float4*>(gc)[k], reinterpret_cast<const float4*>(yy)[k],
                                          coef + 4 * q);
                        }
                        *reinterpret_cast<float4*>(Gi + p * P + 4 * q) = out;
                    }
                    // input channels [16 cit, 16 cit + 16) on the halo tile
                    if (conv) {
                        for (int e = tid; e < G::HN * 4; e += NT) {
                            const int p = e >> 2, q = e & 3, ch0 = cit * 16 + 4 * q;
                            const int r = p / G::HW, cc = p - r * G::HW;
                            const int h = tl.h0 + r - G::R, w = tl.w0 + cc - G::R;
                            float4 v = z4;
                            if (ch0 < C && in_image(h, w, H, W))
                                v = *reinterpret_cast<const float4*>(src + (((int64_t)tl.b * H + h) * W + w) * C + ch0);
                            *reinterpret_cast<float4*>(X + p * P + 4 * q) = v;
                        }
                    } else {
                        stage_x<K, 16, P>(src, ap->steps[t].xs_b, ap->steps[t].xs_c, ap->steps[t].xs_h, ap->steps[t].xs_w,
                                          tl, H, W, cit * 16, CIN, X);
                    }
                    __syncthreads();
#pragma unroll
                    for (int i = 0; i < NTAP; ++i) {
                        const int tap = wv + 4 * i;
                        if (tap < KK) {
                            const int ky = tap / K, kx = tap - ky * K;
                            const float* xb = X + (ky * G::HW + kx) * P + m;
                            f32x4 c = acc[i];
#pragma unroll 4
                            for (int s = 0; s < NT / 4; ++s) {
                                const int p = 4 * s + g4;
                                c = __builtin_amdgcn_mfma_f32_16x16x4f32(Gi[p * P + m], xb[((p >> 5) * G::HW + (p & 31)) * P], c,
                                                                         0, 0, 0);
                            }
                            acc[i] = c;
                        }
                    }
                }
                // lane: output channels 16 cot + 4 g4 .. + 3, input channel 16 cit + m
#pragma unroll
                for (int i = 0; i < NTAP; ++i) {
                    const int tap = wv + 4 * i;
                    if (tap < KK) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int co = cot * 16 + 4 * g4 + r, ci = cit * 16 + m;
                            if (co < C && ci < SC) {
                                float* d = slab + ((int64_t)co * SC + ci) * KK + tap;
                                *d = accumulate ? *d + acc[i][r] : acc[i][r];
                            }
                        }
                    }
                }
            }
        }
    }
}

__global__ void k_prep_weights_k(const float* __restrict__ w, int c, int cin, int kk, float* wt_fwd, float* wt_bwd) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= c * cin * kk) return;
    const int tap = e % kk, ci = (e / kk) % cin, co = e / (kk * cin);
    const float v = w[e];
    if (wt_fwd) wt_fwd[(tap * cin + ci) * c + co] = v;
    if (wt_bwd) wt_bwd[(tap * c + co) * cin + ci] = v;
}

bool k_ok(int k) { return k == 1 || k == 5 || k == 7; }
bool c_ok(int c) { return c == 4 || c == 8 || c == 16 || c == 32; }
bool cin_ok(int c, int cin) { return cin == c || cin == 1 || cin == 2 || cin == 4 || cin == 5; }

template <int K, int C>
int convk_fwd_kc(const snnflow_conv_fwd_args& a, hipStream_t s) {
    const dim3 grid(snnflow_conv_blocks(a.B, a.H, a.W)), block(NT);
    const bool rec = a.wt_rec != nullptr;
    if (C >= 8 && a.cin == C) {
        if constexpr (C >= 8) {
            if (rec) hipLaunchKernelGGL((k_convk_fwd<K, C, true, true>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((k_convk_fwd<K, C, true, false>), grid, block, 0, s, a);
        }
    } else if (rec) {
        hipLaunchKernelGGL((k_convk_fwd<K, C, false, true>), grid, block, 0, s, a);
    } else {
        hipLaunchKernelGGL((k_convk_fwd<K, C, false, false>), grid, block, 0, s, a);
    }
    SNN_CHECK_LAUNCH();
    return 0;
}

template <int K>
int convk_fwd_k(const snnflow_conv_fwd_args& a, hipStream_t s) {
    switch (a.c) {
        case 4: return convk_fwd_kc<K, 4>(a, s);
        case 8: return convk_fwd_kc<K, 8>(a, s);
        case 16: return convk_fwd_kc<K, 16>(a, s);
        default: return convk_fwd_kc<K, 32>(a, s);
    }
}

template <int K, int C>
int layerk_bwd_kc(const snnflow_layer_bwd_args& a, hipStream_t s) {
    // a layer without a per-pixel output only finishes its parameter gradients: block 0 alone
    const bool pixels = (a.g_x && a.wt_bwd_ff) || a.g_state_prev;
    const dim3 grid(pixels ? snnflow_conv_blocks(a.B, a.H, a.W) : 1), block(NT);
    const bool rec = a.wt_bwd_rec != nullptr || a.wt_fwd_rec != nullptr;
    if (C >= 8 && a.cin == C) {
        if constexpr (C >= 8) {
            if (rec) hipLaunchKernelGGL((k_layerk_bwd<K, C, true, true>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((k_layerk_bwd<K, C, true, false>), grid, block, 0, s, a);
        }
    } else if (rec) {
        hipLaunchKernelGGL((k_layerk_bwd<K, C, false, true>), grid, block, 0, s, a);
    } else {
        hipLaunchKernelGGL((k_layerk_bwd<K, C, false, false>), grid, block, 0, s, a);
    }
    SNN_CHECK_LAUNCH();
    return 0;
}

template <int K>
int layerk_bwd_k(const snnflow_layer_bwd_args& a, hipStream_t s) {
    switch (a.c) {
        case 4: return layerk_bwd_kc<K, 4>(a, s);
        case 8: return layerk_bwd_kc<K, 8>(a, s);
        case 16: return layerk_bwd_kc<K, 16>(a, s);
        default: return layerk_bwd_kc<K, 32>(a, s);
    }
}

}  // namespace

extern "C" {

int snnflow_convk_supported(int k, int c, int cin, int rec) {
    (void)rec;  // recurrent and feed-forward cells take the same input widths
    return (k_ok(k) && c_ok(c) && cin_ok(c, cin)) ? 1 : 0;
}

int snnflow_prep_weights_k(const float* w, int c, int cin, int k, float* wt_fwd, float* wt_bwd, void* stream) {
    if (!w || c <= 0 || cin <= 0 || (!wt_fwd && !wt_bwd)) SNN_FAIL(SNNFLOW_E_ARG, "prep_weights_k: bad args");
    if (!k_ok(k)) SNN_FAIL(SNNFLOW_E_ARG, "prep_weights_k: k must be 1, 5 or 7 (3: snnflow_prep_weights)");
    const int n = c * cin * k * k;
    hipLaunchKernelGGL(k_prep_weights_k, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, w, c, cin, k * k, wt_fwd,
                       wt_bwd);
    SNN_CHECK_LAUNCH();
    return 0;
}

int snnflow_convk_fwd(const snnflow_conv_fwd_args* a, int k, void* stream) {
    if (!a || a->B <= 0 || a->H <= 0 || a->W <= 0 || !a->wt_ff || !a->y || !a->x) SNN_FAIL(SNNFLOW_E_ARG, "convk_fwd: bad args");
    if (!k_ok(k)) SNN_FAIL(SNNFLOW_E_ARG, "convk_fwd: k must be 1, 5 or 7 (3: snnflow_conv_fwd)");
    if (a->lif_in) SNN_FAIL(SNNFLOW_E_ARG, "convk_fwd: lif_in must be 0");
    if (a->wf_ff || a->wf_rec || a->prev_spk_bits || a->s_prev_bits || a->prev_y || a->prev_mem || a->prev_acc ||
        a->prev_stats || a->prev_state || a->state_spk_skip)
        SNN_FAIL(SNNFLOW_E_ARG, "convk_fwd: a field of the 3x3 fast paths is set (wf_*, spike bit planes, prev_*, state_spk_skip)");
    if (!c_ok(a->c) || !cin_ok(a->c, a->cin)) SNN_FAIL(SNNFLOW_E_CHANNELS, "convk_fwd: c in {4, 8, 16, 32}, cin in {1, 2, 4, 5, c}");
    if (a->c >= 8 && ((a->cin == a->c && !a->wt_ff_t) || (a->wt_rec && !a->wt_rec_t)))
        SNN_FAIL(SNNFLOW_E_ARG, "convk_fwd: the matrix-core convs need the backward-layout weights wt_ff_t / wt_rec_t");
    const hipStream_t s = (hipStream_t)stream;
    switch (k) {
        case 1: return convk_fwd_k<1>(*a, s);
        case 5: return convk_fwd_k<5>(*a, s);
        default: return convk_fwd_k<7>(*a, s);
    }
}

int snnflow_layerk_bwd(const snnflow_layer_bwd_args* a, int k, void* stream) {
    if (!a || a->B <= 0 || a->H <= 0 || a->W <= 0 || !a->y || !a->stats || !a->g_cur || !a->acc_in)
        SNN_FAIL(SNNFLOW_E_ARG, "layerk_bwd: bad args");
    if (!a->ng.bn_weight || !a->ng.bn_bias || !a->ng.beta || !a->ng.threshold)
        SNN_FAIL(SNNFLOW_E_ARG, "layerk_bwd: missing parameter-gradient buffers");
    if (!k_ok(k)) SNN_FAIL(SNNFLOW_E_ARG, "layerk_bwd: k must be 1, 5 or 7 (3: snnflow_layer_bwd)");
    if (a->lif_in || a->has_pred) SNN_FAIL(SNNFLOW_E_ARG, "layerk_bwd: lif_in and has_pred must be 0");
    if (a->wd_ff || a->wd_rec || a->wslab_ff || a->wslab_rec || a->s_prev || a->x || a->prev_y || a->prev_mem ||
        a->prev_stats || a->prev_g_state || a->prev_g_cur || a->prev_g_mem || a->acc_out)
        SNN_FAIL(SNNFLOW_E_ARG, "layerk_bwd: a field of the 3x3 fast paths is set (wd_*, wslab_*, s_prev, x, prev_*)");
    if (!c_ok(a->c) || !cin_ok(a->c, a->cin)) SNN_FAIL(SNNFLOW_E_CHANNELS, "layerk_bwd: c in {4, 8, 16, 32}, cin in {1, 2, 4, 5, c}");
    if (a->c >= 8 ? ((a->cin == a->c && a->g_x && a->wt_bwd_ff && !a->wt_fwd_ff) || (a->g_state_prev && !a->wt_fwd_rec))
                  : (a->g_state_prev && !a->wt_bwd_rec))
        SNN_FAIL(SNNFLOW_E_ARG, "layerk_bwd: missing weights (matrix-core convs read wt_fwd_ff / wt_fwd_rec, vector ones wt_bwd_*)");
    const hipStream_t s = (hipStream_t)stream;
    switch (k) {
        case 1: return layerk_bwd_k<1>(*a, s);
        case 5: return layerk_bwd_k<5>(*a, s);
        default: return layerk_bwd_k<7>(*a, s);
    }
}

int snnflow_wgradk(const snnflow_wgrad_args* a, int k, void* stream) {
    if (!a || a->B <= 0 || a->H <= 0 || a->W <= 0 || a->nsteps <= 0 || a->nsteps > SNNFLOW_MAX_WGRAD_STEPS ||
        !a->slab_ff || (a->rec && !a->slab_rec))
        SNN_FAIL(SNNFLOW_E_ARG, "wgradk: bad args");
    if (!k_ok(k)) SNN_FAIL(SNNFLOW_E_ARG, "wgradk: k must be 1, 5 or 7 (3: snnflow_wgrad)");
    for (int t = 0; t < a->nsteps; ++t) {
        const snnflow_wgrad_step& st = a->steps[t];
        if (!st.g_cur || !st.y || !st.x || (st.stats && !st.bnc)) SNN_FAIL(SNNFLOW_E_ARG, "wgradk: incomplete step");
        if (st.x_bits || st.s_prev_bits) SNN_FAIL(SNNFLOW_E_ARG, "wgradk: spike bit planes belong to the 3x3 kernels");
        if (st.stats && !a->bn_weight) SNN_FAIL(SNNFLOW_E_ARG, "wgradk: BatchNorm step needs bn_weight");
    }
    if (!c_ok(a->c) || !cin_ok(a->c, a->cin)) SNN_FAIL(SNNFLOW_E_CHANNELS, "wgradk: c in {4, 8, 16, 32}, cin in {1, 2, 4, 5, c}");
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid(snnflow_conv_blocks(a->B, a->H, a->W)), block(NT);
    // (exact_inputs is not read: the f32 matrix cores are exact for any input)
    switch (k) {
        case 1: hipLaunchKernelGGL(k_wgradk<1>, grid, block, 0, s, *a); break;
        case 5: hipLaunchKernelGGL(k_wgradk<5>, grid, block, 0, s, *a); break;
        default: hipLaunchKernelGGL(k_wgradk<7>, grid, block, 0, s, *a); break;
    }
    SNN_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
