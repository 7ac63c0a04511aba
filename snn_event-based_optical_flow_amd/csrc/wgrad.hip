// Deferred weight gradients of the LIFFireNet layers for gfx950 (snnflow_wgrad) and the fixed-order
// reduction of their per-block slabs (snnflow_slab_reduce).
#include <cmath>
#include <type_traits>

#include "lif_common.h"
#include "snnflow_dev.h"
#include "snnflow_host.h"
#include "snnflow_tile.h"

namespace {

// ---------------------------------------------------------------------------
// Deferred weight gradients (snnflow_wgrad): one block per tile loops over the time
// steps of one layer; the next step's loads are issued before the current step's
// arithmetic (register double buffering); per-thread accumulators live across steps
// and the block writes its slab once.
// ---------------------------------------------------------------------------
typedef const __attribute__((address_space(4))) snnflow_wgrad_args* cwgrad_ptr;

// Matrix-core weight gradient of one block (C >= 16, CIN % 16 == 0): per tap,
//   dW_tap[co][ci] += sum_p G[p][co] * X[halo(p, tap)][ci]
// as v_mfma_f32_16x16x4_f32 with M = co (A = G^T from the interior tile), N = ci (B from the
// halo tile), K = 4 tile pixels per MFMA (lane group g takes pixel 4s + g).  The 9 x (C/16) x
// (CIN/16) output tiles of the ff conv [+ the 9 x (C/16)^2 of the recurrent conv] are dealt
// round-robin to the block's NW waves; accumulators live across all time steps.
template <int CIN, int C, bool REC, int NW>
struct WgradMfma {
    static constexpr int MTc = (C + 15) / 16, NTF = (CIN + 15) / 16, NTR = (C + 15) / 16;
    static constexpr int NFF = 9 * MTc * NTF, NREC = REC ? 9 * MTc * NTR : 0, NTOT = NFF + NREC;
    static constexpr int J = (NTOT + NW - 1) / NW;
    static_assert(C % 8 == 0 && CIN % 8 == 0, "MFMA wgrad: 8-channel multiples (C = 8 pads the 16-wide tiles)");
    f32x4 acc[J];
    // wave-uniform tile decode
    int off[J], mt[J], nt[J], tap[J];
    bool rec[J], live[J];
    __device__ void init() {
        const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
#pragma unroll
        for (int j = 0; j < J; ++j) {
            acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            const int i = wv + NW * j;
            live[j] = i < NTOT;
            rec[j] = i >= NFF;
            const int ii = rec[j] ? i - NFF : i, ntx = rec[j] ? NTR : NTF;
            tap[j] = live[j] ? ii / (MTc * ntx) : 0;
            const int rem = ii - tap[j] * (MTc * ntx);
            mt[j] = live[j] ? rem / ntx : 0;
            nt[j] = live[j] ? rem - mt[j] * ntx : 0;
            off[j] = (tap[j] / 3) * HWD + (tap[j] % 3);
        }
    }
    // Gi: interior G tile [NT][Pad<C>]; X: halo input [HN][Pad<CIN>]; S: halo s_prev [HN][Pad<C>]
    __device__ void step(const float* Gi, const float* X, const float* S, bool has_s) {
        constexpr int PC = Pad<C>::v, PX = Pad<CIN>::v;
        const int lane = threadIdx.x & 63, m = lane & 15, g = lane >> 4;
#pragma unroll 8
        for (int s = 0; s < NT / 4; ++s) {
            const int p = 4 * s + g, ty = p / TW, tx = p - ty * TW;
            const int hb = ty * HWD + tx;
            float a[MTc];
#pragma unroll
            for (int q = 0; q < MTc; ++q) a[q] = (q * 16 + m < C) ? Gi[p * PC + q * 16 + m] : 0.0f;
#pragma unroll
            for (int j = 0; j < J; ++j) {
                if (!live[j] || (rec[j] && !has_s)) continue;
                float av = a[0];
#pragma unroll
                for (int q = 1; q < MTc; ++q)
                    if (mt[j] == q) av = a[q];
                const int n = nt[j] * 16 + m;
                float b = 0.0f;  // padded columns: zero (their outputs are not stored)
                if (rec[j]) {
                    if (n < C) b = S[(hb + off[j]) * PC + n];
                } else if (n < CIN) {
                    b = X[(hb + off[j]) * PX + n];
                }
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b, acc[j], 0, 0, 0);
            }
        }
    }
    // C/D layout: rows co = 16 mt + 4 g + r, column ci = 16 nt + (lane & 15); slab [co][ci][tap]
    __device__ void flush(float* __restrict__ slab_ff, float* __restrict__ slab_rec, int accumulate) {
        const int lane = threadIdx.x & 63, m = lane & 15, g = lane >> 4;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            if (!live[j] || (rec[j] && !slab_rec)) continue;
            const int ci = nt[j] * 16 + m, cin = rec[j] ? C : CIN;
            if (ci >= cin) continue;
            float* base = rec[j] ? slab_rec : slab_ff;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = mt[j] * 16 + g * 4 + r;
                if (co >= C) continue;
                float* d = base + ((int64_t)co * cin + ci) * 9 + tap[j];
                *d = accumulate ? *d + acc[j][r] : acc[j][r];
            }
        }
    }
};

// own-pixel float4 elements of a C-channel NHWC tile, distributed over NTH threads
template <int CH, int NTH>
struct Own4 {
    static constexpr int Q = CH / 4, E = NT * Q, R = (E + NTH - 1) / NTH;
};

template <int CIN, int C, bool REC, int SPLIT>
__global__ __launch_bounds__(NT * SPLIT) void k_wgrad(snnflow_wgrad_args) {
    constexpr int NTB = NT * SPLIT;
    constexpr int PC = Pad<C>::v, PI_ = Pad<CIN>::v;
    constexpr bool XV = CIN % 4 == 0;  // x may be dense NHWC (register prefetch)
    // ff items on all threads; with a recurrent conv and SPLIT = 2 each conv gets one
    // half of the block (one accumulator set per thread)
    constexpr bool HALVES = REC && SPLIT == 2;
    using AF = WAcc<CIN, C, HALVES ? NT : NTB, 0>;
    using AR = WAcc<C, C, HALVES ? NT : NTB, HALVES ? NT : 0>;
    constexpr bool MF = C >= 16 && CIN % 16 == 0;  // matrix-core path (WgradMfma; at C = 8 the vector path is faster)
    using O = Own4<C, NTB>;
    constexpr int RX = XV ? Halo4<CIN, NTB>::R : 1, RS = REC ? Halo4<C, NTB>::R : 1;
    constexpr int SCR = MF ? 4 : ((REC && AR::SCRATCH > AF::SCRATCH) ? AR::SCRATCH : AF::SCRATCH);
    __shared__ __attribute__((aligned(16))) float Gi[NT * PC];
    __shared__ __attribute__((aligned(16))) float X[HN * PI_];
    __shared__ __attribute__((aligned(16))) float S[REC ? HN * PC : 4];
    __shared__ __attribute__((aligned(16))) float scratch[SCR];
    __shared__ BnBwdLds coef[SNNFLOW_MAX_WGRAD_STEPS][C];

    // the step table stays in the kernarg segment (scalar loads; a dynamically indexed
    // by-value copy would go to scratch)
    const cwgrad_ptr ap = (cwgrad_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    const int tid = threadIdx.x;
    const int H = ap->H, W = ap->W, nsteps = ap->nsteps;
    const Tile tl = block_tile(H, W);
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);

    // per-step BN backward coefficients of every channel (one round trip for all steps)
    for (int e = tid; e < nsteps * C; e += NTB) {
        const int t = e / C, c = e - t * C;
        const float* st = ap->steps[t].stats;
        const float* bc = ap->steps[t].bnc;
        BnBwdLds k = {0.f, 1.f, 0.f, 0.f, 1.f};  // no BatchNorm: G = g_cur
        if (st) {
            k.mean = st[c];
            k.inv = st[C + c];
            k.gm = bc[c];
            k.k = bc[C + c];
            k.w = ap->bn_weight[c];
        }
        coef[t][c] = k;
    }

    // narrow strided inputs (the head's NCHW event counts): element-wise register prefetch
    constexpr int RXS = XV ? 1 : (HN * CIN + NTB - 1) / NTB;
    // one step's loads in registers, D steps in flight.  D = 3 for the C = 8 feed-forward layers (the
    // deferred head of the wavefront path, 18 registers per step) measured 33.4-35.0 -> 36.2-36.8 us per
    // cfg2 step (profiles/r06/fuse_head_ab.txt): the head's per-step time is not load latency; D = 1.
    struct Pf {
        float4 rg[O::R], ry[O::R], rx[RX], rs[RS];
        float rxs[RXS];
        bool dense, has_s;
    };
    constexpr int D = 1;
    Pf pf[D];
    auto issue = [&](int t, Pf& f) {  // loads of step t into registers
        const float* g = ap->steps[t].g_cur;
        const float* y = ap->steps[t].y;
#pragma unroll
        for (int i = 0; i < O::R; ++i) {
            const int e = tid + i * NTB;
            const int p = e / O::Q, q = e - p * O::Q;
            const int ty = p / TW, tx = p - ty * TW;
            const int h = tl.h0 + ty, w = tl.w0 + tx;
            const bool ok = e < O::E && h < H && w < W;
            const int64_t k = ok ? (((int64_t)tl.b * H + h) * W + w) * O::Q + q : 0;
            f.rg[i] = ok ? reinterpret_cast<const float4*>(g)[k] : z4;
            f.ry[i] = ok ? reinterpret_cast<const float4*>(y)[k] : z4;
        }
        const float* sx = ap->steps[t].x;
        const float* sp = ap->steps[t].s_prev;
        f.dense = false;
        if constexpr (XV)
            f.dense = ap->steps[t].xs_c == 1 && ap->steps[t].xs_w == CIN && ap->steps[t].xs_h == (int64_t)W * CIN &&
                      ap->steps[t].xs_b == (int64_t)H * W * CIN;
        if constexpr (XV) {
            if (f.dense) halo_load<CIN, NTB>(sx, tl, H, W, f.rx);
        } else {
            const auto& st = ap->steps[t];
            const float* xb = sx + (int64_t)tl.b * st.xs_b;
#pragma unroll
            for (int i = 0; i < RXS; ++i) {
                const int e = tid + i * NTB;
                const int ci = e / HN, p = e - ci * HN;  // channel-major: plane reads coalesce
                const int r = p / HWD, cc = p - r * HWD;
                const int h = tl.h0 + r - 1, w = tl.w0 + cc - 1;
                f.rxs[i] = (e < HN * CIN && in_image(h, w, H, W)) ? xb[ci * st.xs_c + h * st.xs_h + w * st.xs_w] : 0.0f;
            }
        }
        f.has_s = REC && sp != nullptr;
        if constexpr (REC) {
            if (f.has_s) halo_load<C, NTB>(sp, tl, H, W, f.rs);
        }
    };
    // stage step t: G on the tile interior, x and s_prev halos
    auto stage = [&](int t, const Pf& f) {
#pragma unroll
        for (int i = 0; i < O::R; ++i) {
            const int e = tid + i * NTB;
            if (e < O::E) {
                const int p = e / O::Q, q = e - p * O::Q;
                const int ty = p / TW, tx = p - ty * TW;
                const bool img = tl.h0 + ty < H && tl.w0 + tx < W;  // G = 0 outside the image
                *reinterpret_cast<float4*>(Gi + p * PC + 4 * q) = img ? bn_bwd4(f.rg[i], f.ry[i], &coef[t][4 * q]) : z4;
            }
        }
        if constexpr (XV) {
            if (f.dense) halo_store<CIN, NTB>(X, f.rx);
        }
        if constexpr (!XV) {
#pragma unroll
            for (int i = 0; i < RXS; ++i) {
                const int e = tid + i * NTB;
                if (e < HN * CIN) {
                    const int ci = e / HN, p = e - ci * HN;
                    X[p * PI_ + ci] = f.rxs[i];
                }
            }
        } else if (!f.dense) {
            stage_strided<CIN, NTB>(ap->steps[t].x, ap->steps[t].xs_b, ap->steps[t].xs_c, ap->steps[t].xs_h,
                                    ap->steps[t].xs_w, tl, H, W, X);
        }
        if constexpr (REC) {
            if (f.has_s) halo_store<C, NTB>(S, f.rs);
        }
    };

    AF af;
    AR ar;
    WgradMfma<(MF ? CIN : 8), (MF ? C : 8), REC, NTB / 64> am;
    if constexpr (MF) {
        am.init();
    } else {
        af.zero();
        if constexpr (REC) ar.zero();
    }
#pragma unroll
    for (int k = 0; k < D; ++k)
        if (k < nsteps) issue(k, pf[k]);
    __syncthreads();  // coef
    for (int t0 = 0; t0 < nsteps; t0 += D) {
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const int t = t0 + k;
            if (t >= nsteps) break;
            stage(t, pf[k]);
            const bool has_s_t = pf[k].has_s;
            __syncthreads();
            if (t + D < nsteps) issue(t + D, pf[k]);  // step t+D's loads fly during the next D steps' math
            if constexpr (MF) {
                am.step(Gi, X, S, has_s_t);
            } else {
                af.step(Gi, X);
                if constexpr (REC) {
                    if (has_s_t) ar.step(Gi, S);
                }
            }
            __syncthreads();
        }
    }
    const int64_t blk = blockIdx.x;
    if constexpr (MF) {
        am.flush(ap->slab_ff + blk * (C * CIN * 9), REC ? ap->slab_rec + blk * (C * C * 9) : nullptr, ap->accumulate);
    } else {
        af.flush(ap->slab_ff + blk * (C * CIN * 9), ap->accumulate, scratch);
        if constexpr (REC) ar.flush(ap->slab_rec + blk * (C * C * 9), ap->accumulate, scratch);
    }
}

// ---------------------------------------------------------------------------
// Weight gradients of the C x C layers on the bf16 matrix cores (snnflow_wgrad with
// exact_inputs: the conv inputs -- spikes -- are exact in bf16).  Per tap,
//   dW_tap[co][ci] = sum_p G[p][co] * X[p + tap][ci]
// as v_mfma_f32_16x16x32_bf16 with M = co (A = G^T split into three bf16 parts, so the
// products are the exact f32 products), N = ci (B = X, exact), K = the 32 pixels of one tile
// row (lane group g: pixels 8g..8g+7).  LDS holds G^T [C][260] f32 and X^T / S^T
// [C][10][40] bf16 (channel-major, padded: conflict-free 16-B reads); one 12-element read
// of a halo row gives the B operands of all three kx taps by register shifts.  The output
// tiles (src, ci-tile, ky) x (kx, co-tile) are split over TG wave groups, the 8 tile rows
// over RG = 8 / TG row groups; row groups are summed through LDS in a fixed order at the
// end (deterministic), then one slab write per block.
// ---------------------------------------------------------------------------
template <int C, bool REC>
struct WbGeo {
    static constexpr int MTc = (C + 15) / 16, NTc = (C + 15) / 16;
    static constexpr int BROWS = (REC ? 2 : 1) * NTc * 3;  // (src, ci-tile, ky)
    static constexpr int TPB = 3 * MTc;                     // tiles per B-row: (kx, co-tile)
    static constexpr int NTOT = BROWS * TPB;
    // wave groups over the tiles: <= 9 accumulator tiles per wave up to C = 16, 18 at C = 32
    static constexpr int TG = C <= 16 ? (REC ? 2 : 1) : (REC ? 4 : 2);
    static constexpr int RG = 8 / TG;
    static constexpr int BRW = BROWS / TG;                  // B-rows per wave
    static constexpr int TPW = BRW * TPB;                   // accumulator tiles per wave
    static_assert(BROWS % TG == 0, "B-rows split evenly over the wave groups");
    static constexpr int GS = NT + 4;                       // G^T channel stride (floats)
    static constexpr int XS = 10 * 40 + 8;                  // X^T channel stride (bf16)
};

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// C = 32 feed-forward weight gradients without the register prefetch of the next step (A/B):
// <= 128 VGPRs, two blocks per CU (66 KB LDS), so the 512-tile grid of cfg2 is one round and the
// other block's math covers a block's loads.
#ifndef SNNFLOW_WG32_PF
#define SNNFLOW_WG32_PF 1
#endif
#ifndef SNNFLOW_WG32_SPLIT
#define SNNFLOW_WG32_SPLIT 1  // C = 32: k_wgrad_bf32 (two blocks per CU) for feed-forward layers (2: recurrent too)
#endif
template <int C, bool REC>
constexpr bool kWgPf = !(C == 32 && !REC && !SNNFLOW_WG32_PF);

template <int C, bool REC>
__global__ __launch_bounds__(NT * 2, (kWgPf<C, REC> ? 1 : 4)) void k_wgrad_bf(snnflow_wgrad_args) {
    using Gm = WbGeo<C, REC>;
    constexpr bool PF = kWgPf<C, REC>;
    constexpr int NTB = NT * 2, NW = NTB / 64, Q = C / 4;
    constexpr int RX = Halo4<C, NTB>::R;
    using O = Own4<C, NTB>;
    static_assert(NW == 8, "8 waves");
    // one pool for G^T, X^T, S^T: the row-group reduction at the end aliases all of it
    // (separate __shared__ arrays are not guaranteed to be contiguous)
    constexpr int GF = C * Gm::GS, XF = C * Gm::XS / 2, SF = REC ? C * Gm::XS / 2 : 4;
    constexpr int RF = Gm::TG * Gm::TPW * 256;
    __shared__ __attribute__((aligned(16))) float pool[(GF + XF + SF > RF ? GF + XF + SF : RF)];
    float* const Gt = pool;
    unsigned short* const Xt = reinterpret_cast<unsigned short*>(pool + GF);
    unsigned short* const St = reinterpret_cast<unsigned short*>(pool + GF + XF);
    __shared__ BnBwdLds coef[SNNFLOW_MAX_WGRAD_STEPS][C];

    const cwgrad_ptr ap = (cwgrad_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    const int tid = threadIdx.x, lane = tid & 63, m = lane & 15, g = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), tg = wv % Gm::TG, rg = wv / Gm::TG;
    const int H = ap->H, W = ap->W, nsteps = ap->nsteps;
    const Tile tl = block_tile(H, W);
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);

    for (int e = tid; e < nsteps * C; e += NTB) {
        const int t = e / C, c = e - t * C;
        const float* st = ap->steps[t].stats;
        const float* bc = ap->steps[t].bnc;
        BnBwdLds k = {0.f, 1.f, 0.f, 0.f, 1.f};
        if (st) {
            k.mean = st[c];
            k.inv = st[C + c];
            k.gm = bc[c];
            k.k = bc[C + c];
            k.w = ap->bn_weight[c];
        }
        coef[t][c] = k;
    }

    float4 rg4[O::R], ry4[O::R], rx[RX], rs[REC ? RX : 1];
    unsigned rxb[RX], rsb[REC ? RX : 1];  // x / s_prev as spike bit-plane words (ABI 39)
    bool dense = false, has_s = false, xbits = false, sbits = false;
    auto issue = [&](int t) {
        const float* gp = ap->steps[t].g_cur;
        const float* yp = ap->steps[t].y;
#pragma unroll
        for (int i = 0; i < O::R; ++i) {
            const int e = tid + i * NTB;
            const int p = e / Q, q = e - p * Q;
            const int ty = p / TW, tx = p - ty * TW;
            const int h = tl.h0 + ty, w = tl.w0 + tx;
            const bool ok = e < O::E && h < H && w < W;
            const int64_t k = ok ? (((int64_t)tl.b * H + h) * W + w) * Q + q : 0;
            rg4[i] = ok ? reinterpret_cast<const float4*>(gp)[k] : z4;
            ry4[i] = ok ? reinterpret_cast<const float4*>(yp)[k] : z4;
        }
        const auto& sp = ap->steps[t];
        xbits = sp.x_bits != nullptr;
        dense = xbits || (sp.xs_c == 1 && sp.xs_w == C && sp.xs_h == (int64_t)W * C && sp.xs_b == (int64_t)H * W * C);
        if (xbits) halo_load_bits<C, NTB>(sp.x_bits, tl, H, W, rxb);
        else if (dense) halo_load<C, NTB>(sp.x, tl, H, W, rx);
        sbits = REC && sp.s_prev_bits != nullptr;
        has_s = REC && (sp.s_prev != nullptr || sbits);
        if constexpr (REC) {
            if (sbits) halo_load_bits<C, NTB>(sp.s_prev_bits, tl, H, W, rsb);
            else if (has_s) halo_load<C, NTB>(sp.s_prev, tl, H, W, rs);
        }
    };
    // halo float4 element (pixel p, quad q) -> 4 bf16 of the channel-major tile
    auto put_halo = [&](unsigned short* T, int e, const float4& v) {
        const int p = e / Q, q = e - p * Q;
        const int hr = p / HWD, hc = p - hr * HWD;
        unsigned short* d = T + (4 * q) * Gm::XS + hr * 40 + hc;
        d[0] = __builtin_bit_cast(unsigned short, (__bf16)v.x);
        d[Gm::XS] = __builtin_bit_cast(unsigned short, (__bf16)v.y);
        d[2 * Gm::XS] = __builtin_bit_cast(unsigned short, (__bf16)v.z);
        d[3 * Gm::XS] = __builtin_bit_cast(unsigned short, (__bf16)v.w);
    };

    f32x4 acc[Gm::TPW];
#pragma unroll
    for (int j = 0; j < Gm::TPW; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

    if constexpr (PF) issue(0);
    __syncthreads();  // coef
    for (int t = 0; t < nsteps; ++t) {
        if constexpr (!PF) issue(t);
        // stage step t: G^T (BN backward of g_cur, zero outside the image), X^T, S^T
#pragma unroll
        for (int i = 0; i < O::R; ++i) {
            const int e = tid + i * NTB;
            if (e < O::E) {
                const int p = e / Q, q = e - p * Q;
                const int ty = p / TW, tx = p - ty * TW;
                const bool img = tl.h0 + ty < H && tl.w0 + tx < W;
                const float4 gv = img ? bn_bwd4(rg4[i], ry4[i], &coef[t][4 * q]) : z4;
                float* d = Gt + (4 * q) * Gm::GS + p;
                d[0] = gv.x;
                d[Gm::GS] = gv.y;
                d[2 * Gm::GS] = gv.z;
                d[3 * Gm::GS] = gv.w;
            }
        }
        const bool dense_t = dense, has_s_t = has_s, xbits_t = xbits, sbits_t = sbits;
        if (xbits_t) {
#pragma unroll
            for (int i = 0; i < RX; ++i) {
                const int e = tid + i * NTB;
                if (e < Halo4<C, NTB>::E) put_halo(Xt, e, spk_quad<C>(rxb[i], e % Q));
            }
        } else if (dense_t) {
#pragma unroll
            for (int i = 0; i < RX; ++i) {
                const int e = tid + i * NTB;
                if (e < Halo4<C, NTB>::E) put_halo(Xt, e, rx[i]);
            }
        } else {  // strided input: element-wise gather (not the engine's path)
            const auto& sp = ap->steps[t];
            for (int e = tid; e < HN * C; e += NTB) {
                const int p = e / C, c = e - p * C;
                const int hr = p / HWD, hc = p - hr * HWD;
                const int h = tl.h0 + hr - 1, w = tl.w0 + hc - 1;
                const float v = in_image(h, w, H, W) ? sp.x[tl.b * sp.xs_b + c * sp.xs_c + h * sp.xs_h + w * sp.xs_w] : 0.f;
                Xt[c * Gm::XS + hr * 40 + hc] = __builtin_bit_cast(unsigned short, (__bf16)v);
            }
        }
        if constexpr (REC) {
            if (sbits_t) {
#pragma unroll
                for (int i = 0; i < RX; ++i) {
                    const int e = tid + i * NTB;
                    if (e < Halo4<C, NTB>::E) put_halo(St, e, spk_quad<C>(rsb[i], e % Q));
                }
            } else if (has_s_t) {
#pragma unroll
                for (int i = 0; i < RX; ++i) {
                    const int e = tid + i * NTB;
                    if (e < Halo4<C, NTB>::E) put_halo(St, e, rs[i]);
                }
            }
        }
        __syncthreads();
        if constexpr (PF) {
            if (t + 1 < nsteps) issue(t + 1);  // next step's loads fly during this step's math
        }

        // compute: this wave's tile rows r = rg, rg + RG, ...
#pragma unroll
        for (int rr = 0; rr < Gm::TG; ++rr) {
            const int r = rg + rr * Gm::RG;
            bf16x8 ah[Gm::MTc], am[Gm::MTc], al[Gm::MTc];
#pragma unroll
            for (int mt = 0; mt < Gm::MTc; ++mt) {
                const int co = mt * 16 + m;
                float a8[8];
                if (co < C) {
                    const float* src = Gt + co * Gm::GS + r * TW + 8 * g;
                    const float4 u = *reinterpret_cast<const float4*>(src), v = *reinterpret_cast<const float4*>(src + 4);
                    a8[0] = u.x; a8[1] = u.y; a8[2] = u.z; a8[3] = u.w; a8[4] = v.x; a8[5] = v.y; a8[6] = v.z; a8[7] = v.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) a8[j] = 0.f;
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const __bf16 h = (__bf16)a8[j];
                    const float r1 = a8[j] - (float)h;
                    const __bf16 md = (__bf16)r1;
                    ah[mt][j] = h;
                    am[mt][j] = md;
                    al[mt][j] = (__bf16)(r1 - (float)md);
                }
            }
#pragma unroll
            for (int k = 0; k < Gm::BRW; ++k) {
                const int br = tg * Gm::BRW + k;  // (src, ci-tile, ky), ky fastest
                const int ky = br % 3, nt = (br / 3) % Gm::NTc, src = br / (3 * Gm::NTc);
                if (src == 1 && !has_s_t) continue;
                const int ci = nt * 16 + m;
                unsigned int w6[6] = {0u, 0u, 0u, 0u, 0u, 0u};
                if (ci < C) {
                    const unsigned short* T = (src == 0 ? Xt : St) + ci * Gm::XS + (r + ky) * 40 + 8 * g;
                    const u32x4 u = *reinterpret_cast<const u32x4*>(T);
                    const uint2 v = *reinterpret_cast<const uint2*>(T + 8);
                    w6[0] = u.x; w6[1] = u.y; w6[2] = u.z; w6[3] = u.w; w6[4] = v.x; w6[5] = v.y;
                }
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    u32x4 bw;
                    if (kx == 0) bw = u32x4{w6[0], w6[1], w6[2], w6[3]};
                    else if (kx == 2) bw = u32x4{w6[1], w6[2], w6[3], w6[4]};
                    else bw = u32x4{__builtin_amdgcn_alignbit(w6[1], w6[0], 16), __builtin_amdgcn_alignbit(w6[2], w6[1], 16),
                                    __builtin_amdgcn_alignbit(w6[3], w6[2], 16), __builtin_amdgcn_alignbit(w6[4], w6[3], 16)};
                    const bf16x8 b = __builtin_bit_cast(bf16x8, bw);
#pragma unroll
                    for (int mt = 0; mt < Gm::MTc; ++mt) {
                        f32x4& d = acc[k * Gm::TPB + kx * Gm::MTc + mt];
                        d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[mt], b, d, 0, 0, 0);
                        d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am[mt], b, d, 0, 0, 0);
                        d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[mt], b, d, 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();
    }

    // row groups 1..RG-1 add into row group 0 through LDS (fixed order), aliasing Gt/Xt/St
    float* red = pool;  // [TG][TPW][64][4] floats (RF)
#pragma unroll 1
    for (int q = 1; q < Gm::RG; ++q) {
        if (rg == q) {
#pragma unroll
            for (int j = 0; j < Gm::TPW; ++j)
                *reinterpret_cast<f32x4*>(red + ((tg * Gm::TPW + j) * 64 + lane) * 4) = acc[j];
        }
        __syncthreads();
        if (rg == 0) {
#pragma unroll
            for (int j = 0; j < Gm::TPW; ++j) acc[j] = acc[j] + *reinterpret_cast<const f32x4*>(red + ((tg * Gm::TPW + j) * 64 + lane) * 4);
        }
        __syncthreads();
    }
    if (rg != 0) return;
    const int64_t blk = blockIdx.x;
    const int accumulate = ap->accumulate;
#pragma unroll
    for (int k = 0; k < Gm::BRW; ++k) {
        const int br = tg * Gm::BRW + k;
        const int ky = br % 3, nt = (br / 3) % Gm::NTc, src = br / (3 * Gm::NTc);
        float* slab = (src == 0 ? ap->slab_ff : ap->slab_rec) + blk * (C * C * 9);
        const int ci = nt * 16 + m;
        if (ci >= C) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
            for (int mt = 0; mt < Gm::MTc; ++mt) {
                const f32x4 v = acc[k * Gm::TPB + kx * Gm::MTc + mt];
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    const int co = mt * 16 + 4 * g + r4;
                    if (co >= C) continue;
                    float* d = slab + ((int64_t)co * C + ci) * 9 + ky * 3 + kx;
                    *d = accumulate ? *d + v[r4] : v[r4];
                }
            }
    }
}

// C = 32 weight gradients at two blocks per CU (k_wgrad_bf<32> needs 212-244 VGPRs, one block per
// CU, so the 512-tile grid of cfg2 took two rounds).  Same arithmetic and slab layout as
// k_wgrad_bf; what changes is the split of the work and the staging:
//   * wave w: output tiles of (ci-tile nt = w & 1, co-tile mt = (w >> 1) & 1) -- all 3 x 3 taps,
//     per source 9 accumulator tiles (36 VGPRs) and ONE co-tile's A fragments (hi/mid/lo, 12
//     VGPRs) -- over the tile rows r = (w >> 2) + 2 i (two row groups, summed in LDS at the end);
//   * no next-step loads held in registers: each step's G / y / x loads are issued and stored to LDS
//     in batches (the other resident block's math covers them);
//   * recurrent cells stage S into the X buffer after the X pass (one X buffer: G^T 33 KB + X^T 26 KB
//     + BN coefficients 20 KB = 80 KB of LDS, two blocks per CU; <= 128 VGPRs).
// ---------------------------------------------------------------------------
// A lane's 36 slab elements of one C = 32 weight-gradient tile pair (rows co0 .. co0+3, column ci, the
// 9 taps; v(j) gives tap j's four values): written, or added to the old values -- every old value is
// loaded before the first add (a conditional load per element made the compiler wait 36 round trips).
template <typename F>
__device__ inline void slab_rmw_36(float* slab, int co0, int ci, int accumulate, F&& v) {
    constexpr int C = 32;
    float old[9][4];
    if (accumulate) {
#pragma unroll
        for (int j = 0; j < 9; ++j)
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) old[j][r4] = slab[((int64_t)(co0 + r4) * C + ci) * 9 + j];
    } else {
#pragma unroll
        for (int j = 0; j < 9; ++j)
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) old[j][r4] = 0.0f;
    }
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const f32x4 x = v(j);
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) slab[((int64_t)(co0 + r4) * C + ci) * 9 + j] = accumulate ? old[j][r4] + x[r4] : x[r4];
    }
}

template <bool REC>
__global__ __launch_bounds__(NT * 2, 4) void k_wgrad_bf32(snnflow_wgrad_args) {
    constexpr int C = 32, NTB = NT * 2, Q = C / 4;
    constexpr int GS = NT + 4, XS = 10 * 40 + 8;
    constexpr int RX = Halo4<C, NTB>::R;
    using O = Own4<C, NTB>;
    constexpr int NS = REC ? 2 : 1;      // sources: x (ff conv), s_prev (rec conv)
    constexpr int GF = C * GS, XF = C * XS / 2;
    constexpr int RF = 4 * 9 * 256;      // one source's row-group exchange [4 tg][9][64][4]
    static_assert(RF <= GF + XF, "exchange fits the staging pool");
    __shared__ __attribute__((aligned(16))) float pool[GF + XF];
    float* const Gt = pool;
    unsigned short* const Xt = reinterpret_cast<unsigned short*>(pool + GF);
    __shared__ BnBwdLds coef[SNNFLOW_MAX_WGRAD_STEPS][C];

    const cwgrad_ptr ap = (cwgrad_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    const int tid = threadIdx.x, lane = tid & 63, m = lane & 15, g = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nt = wv & 1, mt = (wv >> 1) & 1, rg = wv >> 2;
    const int H = ap->H, W = ap->W, nsteps = ap->nsteps;
    const Tile tl = block_tile(H, W);
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);

    for (int e = tid; e < nsteps * C; e += NTB) {
        const int t = e / C, c = e - t * C;
        const float* st = ap->steps[t].stats;
        const float* bc = ap->steps[t].bnc;
        BnBwdLds k = {0.f, 1.f, 0.f, 0.f, 1.f};
        if (st) {
            k.mean = st[c];
            k.inv = st[C + c];
            k.gm = bc[c];
            k.k = bc[C + c];
            k.w = ap->bn_weight[c];
        }
        coef[t][c] = k;
    }

    // halo float4 element (pixel p, quad q) -> 4 bf16 of the channel-major tile
    auto put_halo = [&](int e, const float4& v) {
        const int p = e / Q, q = e - p * Q;
        const int hr = p / HWD, hc = p - hr * HWD;
        unsigned short* d = Xt + (4 * q) * XS + hr * 40 + hc;
        d[0] = __builtin_bit_cast(unsigned short, (__bf16)v.x);
        d[XS] = __builtin_bit_cast(unsigned short, (__bf16)v.y);
        d[2 * XS] = __builtin_bit_cast(unsigned short, (__bf16)v.z);
        d[3 * XS] = __builtin_bit_cast(unsigned short, (__bf16)v.w);
    };
    // the conv input of step t (x or s_prev) into X^T: dense NHWC halo, or an element-wise gather
    auto stage_x = [&](const float* src, int64_t sb, int64_t sc, int64_t sh, int64_t sw, bool dense,
                       const uint8_t* bits) {
        if (bits) {  // spike bit plane (ABI 39): one word per element, all loads in flight at once
            unsigned rb[RX];
            halo_load_bits<C, NTB>(bits, tl, H, W, rb);
#pragma unroll
            for (int i = 0; i < RX; ++i) {
                const int e = tid + i * NTB;
                if (e < Halo4<C, NTB>::E) put_halo(e, spk_quad<C>(rb[i], e % Q));
            }
        } else if (dense) {  // two batches of loads (12 VGPRs each: the accumulators stay live)
            constexpr int RH = (RX + 1) / 2;
#pragma unroll
            for (int h2 = 0; h2 < RX; h2 += RH) {
                float4 rx[RH];
#pragma unroll
                for (int i = 0; i < RH; ++i) {
                    const int e = tid + (h2 + i) * NTB;
                    const int64_t k = (h2 + i) < RX && e < Halo4<C, NTB>::E ? halo_idx4<C>(e, tl, H, W) : -1;
                    rx[i] = k >= 0 ? reinterpret_cast<const float4*>(src)[k] : z4;
                }
#pragma unroll
                for (int i = 0; i < RH; ++i) {
                    const int e = tid + (h2 + i) * NTB;
                    if ((h2 + i) < RX && e < Halo4<C, NTB>::E) put_halo(e, rx[i]);
                }
            }
        } else {
            for (int e = tid; e < HN * C; e += NTB) {
                const int p = e / C, c = e - p * C;
                const int hr = p / HWD, hc = p - hr * HWD;
                const int h = tl.h0 + hr - 1, w = tl.w0 + hc - 1;
                const float v = in_image(h, w, H, W) ? src[tl.b * sb + c * sc + h * sh + w * sw] : 0.f;
                Xt[c * XS + hr * 40 + hc] = __builtin_bit_cast(unsigned short, (__bf16)v);
            }
        }
    };

    f32x4 acc[NS][9];
#pragma unroll
    for (int sidx = 0; sidx < NS; ++sidx)
#pragma unroll
        for (int j = 0; j < 9; ++j) acc[sidx][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // one source's MFMAs of the staged step: rows r = rg, rg + 2, ..., 9 taps of (nt, mt)
    auto compute = [&](f32x4 (&d)[9]) {
#pragma unroll 1
        for (int r = rg; r < TH; r += 2) {
            bf16x8 ah, am, al;
            {
                const int co = mt * 16 + m;
                const float* src = Gt + co * GS + r * TW + 8 * g;
                const float4 u = *reinterpret_cast<const float4*>(src), v = *reinterpret_cast<const float4*>(src + 4);
                const float a8[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const __bf16 h = (__bf16)a8[j];
                    const float r1 = a8[j] - (float)h;
                    const __bf16 md = (__bf16)r1;
                    ah[j] = h;
                    am[j] = md;
                    al[j] = (__bf16)(r1 - (float)md);
                }
            }
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const unsigned short* T = Xt + (nt * 16 + m) * XS + (r + ky) * 40 + 8 * g;
                const u32x4 u = *reinterpret_cast<const u32x4*>(T);
                const uint2 v = *reinterpret_cast<const uint2*>(T + 8);
                const unsigned int w6[5] = {u.x, u.y, u.z, u.w, v.x};
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    u32x4 bw;
                    if (kx == 0) bw = u32x4{w6[0], w6[1], w6[2], w6[3]};
                    else if (kx == 2) bw = u32x4{w6[1], w6[2], w6[3], w6[4]};
                    else bw = u32x4{__builtin_amdgcn_alignbit(w6[1], w6[0], 16), __builtin_amdgcn_alignbit(w6[2], w6[1], 16),
                                    __builtin_amdgcn_alignbit(w6[3], w6[2], 16), __builtin_amdgcn_alignbit(w6[4], w6[3], 16)};
                    const bf16x8 b = __builtin_bit_cast(bf16x8, bw);
                    f32x4& o = d[ky * 3 + kx];
                    o = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, b, o, 0, 0, 0);
                    o = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, b, o, 0, 0, 0);
                    o = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, b, o, 0, 0, 0);
                }
            }
        }
    };

    __syncthreads();  // coef
    for (int t = 0; t < nsteps; ++t) {
        const auto& sp = ap->steps[t];
        // G^T = BN backward of g_cur (zero outside the image), two batches of loads
#pragma unroll
        for (int h2 = 0; h2 < O::R; h2 += 2) {
            float4 rg4[2], ry4[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int e = tid + (h2 + i) * NTB;
                const int p = e / Q, q = e - p * Q;
                const int ty = p / TW, tx = p - ty * TW;
                const int h = tl.h0 + ty, w = tl.w0 + tx;
                const bool ok = e < O::E && h < H && w < W;
                const int64_t k = ok ? (((int64_t)tl.b * H + h) * W + w) * Q + q : 0;
                rg4[i] = ok ? reinterpret_cast<const float4*>(sp.g_cur)[k] : z4;
                ry4[i] = ok ? reinterpret_cast<const float4*>(sp.y)[k] : z4;
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int e = tid + (h2 + i) * NTB;
                if (e < O::E) {
                    const int p = e / Q, q = e - p * Q;
                    const int ty = p / TW, tx = p - ty * TW;
                    const bool img = tl.h0 + ty < H && tl.w0 + tx < W;
                    const float4 gv = img ? bn_bwd4(rg4[i], ry4[i], &coef[t][4 * q]) : z4;
                    float* d = Gt + (4 * q) * GS + p;
                    d[0] = gv.x;
                    d[GS] = gv.y;
                    d[2 * GS] = gv.z;
                    d[3 * GS] = gv.w;
                }
            }
        }
        const bool dense = sp.xs_c == 1 && sp.xs_w == C && sp.xs_h == (int64_t)W * C && sp.xs_b == (int64_t)H * W * C;
        stage_x(sp.x, sp.xs_b, sp.xs_c, sp.xs_h, sp.xs_w, dense, sp.x_bits);
        __syncthreads();
        compute(acc[0]);
        if constexpr (REC) {
            if (sp.s_prev != nullptr || sp.s_prev_bits != nullptr) {
                __syncthreads();  // X^T reads done
                stage_x(sp.s_prev, 0, 0, 0, 0, true, sp.s_prev_bits);
                __syncthreads();
                compute(acc[NS - 1]);
            }
        }
        __syncthreads();  // before the next step overwrites the tiles
    }

    // row group 1 adds into row group 0 through LDS (fixed order), one source at a time
    const int64_t blk = blockIdx.x;
    const int accumulate = ap->accumulate;
    float* red = pool;
    const int tg = wv & 3;
#pragma unroll
    for (int sidx = 0; sidx < NS; ++sidx) {
        if (rg == 1) {
#pragma unroll
            for (int j = 0; j < 9; ++j) *reinterpret_cast<f32x4*>(red + ((tg * 9 + j) * 64 + lane) * 4) = acc[sidx][j];
        }
        __syncthreads();
        if (rg == 0) {
            float* slab = (sidx == 0 ? ap->slab_ff : ap->slab_rec) + blk * (C * C * 9);
            const int ci = nt * 16 + m;
            slab_rmw_36(slab, mt * 16 + 4 * g, ci, accumulate, [&](int j) {
                return acc[sidx][j] + *reinterpret_cast<const f32x4*>(red + ((tg * 9 + j) * 64 + lane) * 4);
            });
        }
        __syncthreads();
    }
}

// C = 32 weight gradients from spike bit planes (ABI 39: the deferred weight gradients of the
// wavefront path).  k_wgrad_bf32's arithmetic, slab layout and wave split (wave w: ci-tile w & 1, co-tile
// (w >> 1) & 1, tile rows (w >> 2) + 2 i, all 9 taps), with
//   * the conv input of a step as one 32-bit word per halo pixel (1.4 KB per tile instead of 44 KB of
//     fp32 spikes), expanded to the channel-major bf16 X^T tile by the thread of that pixel;
//   * the next step's loads -- g_cur and y of the tile (8 float4 per thread) and the halo word -- issued
//     right after this step's tiles are staged, so they fly during this step's matrix-core work
//     (k_wgrad_bf32 loads each step after the previous one's MFMAs: its fp32 input halo would not fit
//     beside a prefetch in 128 registers);
//   * a recurrent layer's two convs as two block sets (source 0: x -> slab_ff; 1: s_prev -> slab_rec), each
//     block one source with 36 accumulator registers per wave like a feed-forward layer (k_wgrad_bf<32,
//     true> holds both: 256 registers, one block per CU).  Block b: XCD b % 8, source (b / 8) & 1, tile
//     (b % 8) + 8 (b / 16): the two sources of a tile run on one XCD at about the same time, so the second
//     read of G's inputs is an L2 hit.
// A step whose input has no bit plane (s_prev at t = 0: the caller's initial state) stages the fp32 plane;
// without either it adds nothing.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(NT * 2, 4) void k_wgrad_b32(snnflow_wgrad_args) {
    constexpr int C = 32, NTB = NT * 2, Q = C / 4;
    constexpr int GS = NT + 4, XS = 10 * 40 + 8;
    using O = Own4<C, NTB>;
    constexpr int GF = C * GS, XF = C * XS / 2;
    constexpr int RF = 4 * 9 * 256;  // one source's row-group exchange [4 tg][9][64][4]
    static_assert(RF <= GF + XF, "exchange fits the staging pool");
    static_assert(HN <= NTB, "one halo pixel per thread");
    __shared__ __attribute__((aligned(16))) float pool[GF + XF];
    float* const Gt = pool;
    unsigned short* const Xt = reinterpret_cast<unsigned short*>(pool + GF);
    __shared__ BnBwdLds coef[SNNFLOW_MAX_WGRAD_STEPS][C];

    const cwgrad_ptr ap = (cwgrad_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    const int tid = threadIdx.x, lane = tid & 63, m = lane & 15, g = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nt = wv & 1, mt = (wv >> 1) & 1, rg = wv >> 2;
    const int nsrc = ap->rec ? 2 : 1;
    const int b = blockIdx.x, src = nsrc == 2 ? (b >> 3) & 1 : 0;
    const int bt = nsrc == 2 ? (b & 7) + 8 * (b >> 4) : b;  // tile block index (block_tile's XCD order)
    const int H = ap->H, W = ap->W, nsteps = ap->nsteps;
    const int nbt = ap->B * tiles_per_image(H, W);
    if (bt >= nbt) return;  // padding block (recurrent grid: 2 x the tile count rounded up to 8)
    const Tile tl = block_tile(H, W, Grid{bt, nbt});
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);

    for (int e = tid; e < nsteps * C; e += NTB) {
        const int t = e / C, c = e - t * C;
        const float* st = ap->steps[t].stats;
        const float* bc = ap->steps[t].bnc;
        BnBwdLds k = {0.f, 1.f, 0.f, 0.f, 1.f};
        if (st) {
            k.mean = st[c];
            k.inv = st[C + c];
            k.gm = bc[c];
            k.k = bc[C + c];
            k.w = ap->bn_weight[c];
        }
        coef[t][c] = k;
    }

    // the halo pixel of this thread (tid < HN)
    const int hr = tid / HWD, hc = tid - hr * HWD;
    const int hh = tl.h0 + hr - 1, hw = tl.w0 + hc - 1;
    const bool hok = tid < HN && in_image(hh, hw, H, W);
    const int64_t hpix = hok ? ((int64_t)tl.b * H + hh) * W + hw : 0;
    auto in_bits = [&](int t) { return src == 0 ? ap->steps[t].x_bits : ap->steps[t].s_prev_bits; };

    float4 rg4[O::R], ry4[O::R];
    unsigned xw = 0u;
    // the loads are unconditional (an element outside the image reads element 0; the staging zeroes G
    // there): a conditional load made the compiler wait for each pair before issuing the next
    static_assert(O::E % NTB == 0, "every thread holds O::R elements");
    auto issue = [&](int t) {
        const auto& sp = ap->steps[t];
#pragma unroll
        for (int i = 0; i < O::R; ++i) {
            const int e = tid + i * NTB;
            const int p = e / Q, q = e - p * Q;
            const int ty = p / TW, tx = p - ty * TW;
            const int h = tl.h0 + ty, w = tl.w0 + tx;
            const bool ok = h < H && w < W;
            const int64_t k = ok ? (((int64_t)tl.b * H + h) * W + w) * Q + q : 0;
            rg4[i] = reinterpret_cast<const float4*>(sp.g_cur)[k];
            ry4[i] = reinterpret_cast<const float4*>(sp.y)[k];
        }
        const uint8_t* xb = in_bits(t);
        xw = (xb != nullptr && hok) ? spk_load_bits<C>(xb, hpix) : 0u;
    };

    f32x4 acc[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // this wave's MFMAs of the staged step: rows r = rg, rg + 2, ..., the 9 taps of (nt, mt)
    auto compute = [&]() {
#pragma unroll 1
        for (int r = rg; r < TH; r += 2) {
            bf16x8 ah, am, al;
            {
                const int co = mt * 16 + m;
                const float* srcg = Gt + co * GS + r * TW + 8 * g;
                const float4 u = *reinterpret_cast<const float4*>(srcg), v = *reinterpret_cast<const float4*>(srcg + 4);
                const float a8[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const __bf16 h = (__bf16)a8[j];
                    const float r1 = a8[j] - (float)h;
                    const __bf16 md = (__bf16)r1;
                    ah[j] = h;
                    am[j] = md;
                    al[j] = (__bf16)(r1 - (float)md);
                }
            }
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const unsigned short* T = Xt + (nt * 16 + m) * XS + (r + ky) * 40 + 8 * g;
                const u32x4 u = *reinterpret_cast<const u32x4*>(T);
                const uint2 v = *reinterpret_cast<const uint2*>(T + 8);
                const unsigned int w6[5] = {u.x, u.y, u.z, u.w, v.x};
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    u32x4 bw;
                    if (kx == 0) bw = u32x4{w6[0], w6[1], w6[2], w6[3]};
                    else if (kx == 2) bw = u32x4{w6[1], w6[2], w6[3], w6[4]};
                    else bw = u32x4{__builtin_amdgcn_alignbit(w6[1], w6[0], 16), __builtin_amdgcn_alignbit(w6[2], w6[1], 16),
                                    __builtin_amdgcn_alignbit(w6[3], w6[2], 16), __builtin_amdgcn_alignbit(w6[4], w6[3], 16)};
                    const bf16x8 bb = __builtin_bit_cast(bf16x8, bw);
                    f32x4& o = acc[ky * 3 + kx];
                    o = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bb, o, 0, 0, 0);
                    o = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, bb, o, 0, 0, 0);
                    o = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bb, o, 0, 0, 0);
                }
            }
        }
    };

    issue(0);
    __syncthreads();  // coef
    for (int t = 0; t < nsteps; ++t) {
        const auto& sp = ap->steps[t];
        // G^T = BN backward of g_cur (zero outside the image), from the prefetched registers
#pragma unroll
        for (int i = 0; i < O::R; ++i) {
            const int e = tid + i * NTB;
            if (e < O::E) {
                const int p = e / Q, q = e - p * Q;
                const int ty = p / TW, tx = p - ty * TW;
                const bool img = tl.h0 + ty < H && tl.w0 + tx < W;
                const float4 gv = img ? bn_bwd4(rg4[i], ry4[i], &coef[t][4 * q]) : z4;
                float* d = Gt + (4 * q) * GS + p;
                d[0] = gv.x;
                d[GS] = gv.y;
                d[2 * GS] = gv.z;
                d[3 * GS] = gv.w;
            }
        }
        // X^T: the conv input of step t (bit plane: the halo pixel's word -> 32 bf16 0 / 1)
        const uint8_t* xb = in_bits(t);
        const float* xf = src == 0 ? sp.x : sp.s_prev;
        const bool have = xb != nullptr || xf != nullptr;
        if (xb != nullptr) {
            if (tid < HN) {
                unsigned short* d = Xt + hr * 40 + hc;
#pragma unroll
                for (int c = 0; c < C; ++c)
                    d[c * XS] = ((xw >> SNNFLOW_SPK_BIT(C, c)) & 1u) ? (unsigned short)0x3F80 : (unsigned short)0;
            }
        } else if (xf != nullptr) {  // fp32 NHWC plane (s_prev at t = 0), element-wise
            for (int e = tid; e < HN * Q; e += NTB) {
                const int64_t k = halo_idx4<C>(e, tl, H, W);
                const float4 v = k >= 0 ? reinterpret_cast<const float4*>(xf)[k] : z4;
                const int p = e / Q, q = e - p * Q;
                const int r = p / HWD, cc = p - r * HWD;
                unsigned short* d = Xt + (4 * q) * XS + r * 40 + cc;
                d[0] = __builtin_bit_cast(unsigned short, (__bf16)v.x);
                d[XS] = __builtin_bit_cast(unsigned short, (__bf16)v.y);
                d[2 * XS] = __builtin_bit_cast(unsigned short, (__bf16)v.z);
                d[3 * XS] = __builtin_bit_cast(unsigned short, (__bf16)v.w);
            }
        }
        __syncthreads();
        if (t + 1 < nsteps) issue(t + 1);  // step t+1's loads fly during step t's MFMAs
        if (have) compute();
        __syncthreads();  // before the next step overwrites the tiles
    }

    // row group 1 adds into row group 0 through LDS (fixed order)
    const int64_t blk = bt;
    const int accumulate = ap->accumulate;
    float* red = pool;
    const int tg = wv & 3;
    if (rg == 1) {
#pragma unroll
        for (int j = 0; j < 9; ++j) *reinterpret_cast<f32x4*>(red + ((tg * 9 + j) * 64 + lane) * 4) = acc[j];
    }
    __syncthreads();
    if (rg == 0) {
        float* slab = (src == 0 ? ap->slab_ff : ap->slab_rec) + blk * (C * C * 9);
        const int ci = nt * 16 + m;
        slab_rmw_36(slab, mt * 16 + 4 * g, ci, accumulate, [&](int j) {
            return acc[j] + *reinterpret_cast<const f32x4*>(red + ((tg * 9 + j) * 64 + lane) * 4);
        });
    }
}

// Sum of per-block weight-gradient slabs in fp64, fixed order: 64 elements x 16 slab
// groups per 1024-thread block, 4 independent accumulators per thread.
constexpr int SR_E = 64, SR_G = 16;

__global__ __launch_bounds__(SR_E * SR_G) void k_slab_reduce(DescBatch<snnflow_slab_desc> batch, int nblk) {
    __shared__ double part[SR_G][SR_E];
    const snnflow_slab_desc d = batch.pick(blockIdx.y);
    const int le = threadIdx.x % SR_E, g = threadIdx.x / SR_E;
    const int e = blockIdx.x * SR_E + le;
    if (blockIdx.x * SR_E >= d.elems) return;  // uniform per block
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (e < d.elems) {
        const float* src = d.slab + e;
        const int64_t st = d.elems;
        int b = g;
        for (; b + 3 * SR_G < nblk; b += 4 * SR_G) {
            s0 += src[(int64_t)b * st];
            s1 += src[(int64_t)(b + SR_G) * st];
            s2 += src[(int64_t)(b + 2 * SR_G) * st];
            s3 += src[(int64_t)(b + 3 * SR_G) * st];
        }
        for (; b < nblk; b += SR_G) s0 += src[(int64_t)b * st];
    }
    part[g][le] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (g == 0 && e < d.elems) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < SR_G; ++k) s += part[k][le];
        d.out[e] = (float)s;
    }
}

bool valid_c(int c) { return c == 4 || c == 8 || c == 16 || c == 32; }

}  // namespace

extern "C" {

static int g_wg_bits = env_int("SNNFLOW_WG_BITS", 1);  // A/B: 0 = k_wgrad_bf32 / k_wgrad_bf on the bit planes
static int g_wg_head_sp2 = env_int("SNNFLOW_WG_HEAD_SP2", 1);
static bool wgrad_all_x_bits(const snnflow_wgrad_args* a) {
    for (int t = 0; t < a->nsteps; ++t)
        if (!a->steps[t].x_bits) return false;
    return true;
}

int snnflow_wgrad(const snnflow_wgrad_args* a, void* stream) {
    if (!a || a->B <= 0 || a->H <= 0 || a->W <= 0 || a->nsteps <= 0 || a->nsteps > SNNFLOW_MAX_WGRAD_STEPS ||
        !a->slab_ff || (a->rec && !a->slab_rec))
        SNN_FAIL(SNNFLOW_E_ARG, "wgrad: bad args");
    for (int t = 0; t < a->nsteps; ++t) {
        const snnflow_wgrad_step& st = a->steps[t];
        if (!st.g_cur || !st.y || !(st.x || st.x_bits) || (st.stats && !st.bnc)) SNN_FAIL(SNNFLOW_E_ARG, "wgrad: incomplete step");
        if ((st.x_bits || st.s_prev_bits) && !(a->exact_inputs && a->cin == a->c && (a->c == 8 || a->c == 16 || a->c == 32)))
            SNN_FAIL(SNNFLOW_E_ARG, "wgrad: spike bit planes need exact_inputs and cin == c in {8, 16, 32}");
        if (st.stats && !a->bn_weight) SNN_FAIL(SNNFLOW_E_ARG, "wgrad: BatchNorm step needs bn_weight");
    }
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid(snnflow_conv_blocks(a->B, a->H, a->W));
    const int c = a->c, cin = a->cin;
    if (!valid_c(c)) SNN_FAIL(SNNFLOW_E_CHANNELS, "wgrad: c must be 4, 8, 16 or 32");
#define WG_LAUNCH(CI_, CC_, REC_)                                                                          \
    do {                                                                                                   \
        constexpr int SP_ = (CC_ == 8 || CC_ == 16 || (CC_ == 32 && CI_ % 16 == 0)) ? 2 : 1;              \
        constexpr int SP2_ = (CC_ == 32 && CI_ == 2 && !REC_) ? 2 : SP_;                                  \
        if (SP2_ != SP_ && !g_wg_head_sp2)                                                                \
            hipLaunchKernelGGL((k_wgrad<CI_, CC_, REC_, SP_>), grid, dim3(NT * SP_), 0, s, *a);           \
        else                                                                                              \
            hipLaunchKernelGGL((k_wgrad<CI_, CC_, REC_, SP2_>), grid, dim3(NT * SP2_), 0, s, *a);         \
    } while (0)
#define WG_PICK(CI_, CC_)                                                                                  \
    do {                                                                                                   \
        if (a->rec) WG_LAUNCH(CI_, CC_, true);                                                             \
        else WG_LAUNCH(CI_, CC_, false);                                                                   \
    } while (0)
#define WG_CASE(CC_)                                                                                       \
    case CC_:                                                                                              \
        if (cin == CC_) WG_PICK(CC_, CC_);                                                                 \
        else if (cin == 1) WG_PICK(1, CC_);                                                                \
        else if (cin == 2) WG_PICK(2, CC_);                                                                \
        else if (cin == 3) WG_PICK(3, CC_);                                                                \
        else if (cin == 4) WG_PICK(4, CC_);                                                                \
        else if (cin == 5) WG_PICK(5, CC_);                                                                \
        else SNN_FAIL(SNNFLOW_E_CHANNELS, "wgrad: unsupported cin");                                       \
        break;
    if (a->exact_inputs && cin == c && (c == 8 || c == 16 || c == 32)) {
        const dim3 blk(NT * 2);
        if (c == 8) {
            if (a->rec) hipLaunchKernelGGL((k_wgrad_bf<8, true>), grid, blk, 0, s, *a);
            else hipLaunchKernelGGL((k_wgrad_bf<8, false>), grid, blk, 0, s, *a);
        } else if (c == 16) {
            if (a->rec) hipLaunchKernelGGL((k_wgrad_bf<16, true>), grid, blk, 0, s, *a);
            else hipLaunchKernelGGL((k_wgrad_bf<16, false>), grid, blk, 0, s, *a);
        } else if (g_wg_bits && wgrad_all_x_bits(a)) {
            // spike bit planes with the next step's loads in flight (k_wgrad_b32); recurrent layers as
            // two block sets (x and s_prev)
            hipLaunchKernelGGL(k_wgrad_b32, dim3(a->rec ? 2 * ((grid.x + 7) / 8 * 8) : grid.x), blk, 0, s, *a);
        } else {
            // feed-forward layers: k_wgrad_bf32 (two blocks per CU: 197 -> 164 us per cfg2 layer);
            // recurrent ones keep k_wgrad_bf (the split form's second staging pass measured 296 -> 315 us)
            if (a->rec) {
                if (SNNFLOW_WG32_SPLIT > 1) hipLaunchKernelGGL((k_wgrad_bf32<true>), grid, blk, 0, s, *a);
                else hipLaunchKernelGGL((k_wgrad_bf<32, true>), grid, blk, 0, s, *a);
            } else if (SNNFLOW_WG32_SPLIT) {
                hipLaunchKernelGGL((k_wgrad_bf32<false>), grid, blk, 0, s, *a);
            } else {
                hipLaunchKernelGGL((k_wgrad_bf<32, false>), grid, blk, 0, s, *a);
            }
        }
        SNN_CHECK_LAUNCH();
        return 0;
    }
    switch (c) {
        WG_CASE(4) WG_CASE(8) WG_CASE(16) WG_CASE(32)
        default: break;
    }
#undef WG_CASE
#undef WG_PICK
#undef WG_LAUNCH
    SNN_CHECK_LAUNCH();
    return 0;
}

int snnflow_slab_reduce(const snnflow_slab_desc* d, int n, int nblk, void* stream) {
    if (!d || n <= 0 || n > SNNFLOW_MAX_SLABS || nblk <= 0) SNN_FAIL(SNNFLOW_E_ARG, "slab_reduce: bad args");
    DescBatch<snnflow_slab_desc> batch = {};
    int maxe = 0;
    for (int i = 0; i < n; ++i) {
        batch.d[i] = d[i];
        if (!d[i].slab || !d[i].out || d[i].elems <= 0) SNN_FAIL(SNNFLOW_E_ARG, "slab_reduce: bad descriptor");
        maxe = d[i].elems > maxe ? d[i].elems : maxe;
    }
    hipLaunchKernelGGL(k_slab_reduce, dim3((maxe + SR_E - 1) / SR_E, n), dim3(SR_E * SR_G), 0, (hipStream_t)stream,
                       batch, nblk);
    SNN_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
