// Spiking U-Net (SpikingRecEVFlowNet) kernels for gfx950.
//
// Reference semantics:
//   models/model.py:723-858           SpikingRecEVFlowNet (input encoding, nearest upsample of the flows)
//   models/unet.py:310-461            SpikingMultiResUNetRecurrent (encoders, residual blocks,
//                                     decoders with concatenated skips and predictions)
//   models/spiking_submodules.py:29-151   ConvLIF (hard/soft reset, detached reset spikes, sigmoid leak,
//                                          clamp_min(thresh, 0.01), residual added to the spikes)
//   models/spiking_submodules.py:154-300  ConvLIFRecurrent (ff + rec conv of the previous spikes)
//   models/spiking_submodules.py:303-417  blocks; :415 F.interpolate(x2, bilinear, align_corners=False)
//   models/spiking_util.py:28-109         surrogate gradients
//   models/submodules.py:96-113           ConvLayer (prediction: 1x1 conv + bias + tanh)
//
// Every convolution (forward, input gradient, weight gradient) is an implicit GEMM on
// v_mfma_f32_16x16x32_bf16.  The pixel-side operand holds values that are exact in bf16 (spikes,
// small integer residual sums, their bilinear upsamples k/16, and fp32 tensors stored as hi/mid/lo
// bf16 planes or channels); the weight-side operand is split into three bf16 parts; so the
// products are exact fp32 products accumulated in fp32 (no reduced-precision arithmetic).
#include <cmath>

#include "snnflow_dev.h"
#include "snnflow_host.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float fx4 __attribute__((ext_vector_type(4)));

constexpr int UNT = 256;     // threads per block (4 waves)
constexpr int XP = 32;       // bf16 per LDS row of k_unet_conv: 32 k (64-B rows, 16-B pieces swizzled: xoff)

__device__ inline uint4 ld16(const uint16_t* p) { return *reinterpret_cast<const uint4*>(p); }

__device__ inline int swz(int n);
// bf16 offset of piece p (8 bf16) of LDS row n of a k_unet_conv tile: 64-B rows, pieces XOR-swizzled
__device__ inline int xoff(int n, int p) { return n * XP + ((p ^ swz(n)) << 3); }

__device__ inline float bf2f(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }
__device__ inline uint16_t f2bf(float f) {
    const __bf16 b = (__bf16)f;
    return *reinterpret_cast<const uint16_t*>(&b);
}

// hi / mid / lo bf16 parts of an fp32 value (round to nearest each; exact sum for fp32 inputs)
__device__ inline void split3(float x, uint16_t& h, uint16_t& m, uint16_t& l) {
    const __bf16 a = (__bf16)x;
    const float r1 = x - (float)a;
    const __bf16 b = (__bf16)r1;
    const __bf16 c = (__bf16)(r1 - (float)b);
    h = *reinterpret_cast<const uint16_t*>(&a);
    m = *reinterpret_cast<const uint16_t*>(&b);
    l = *reinterpret_cast<const uint16_t*>(&c);
}

// 16-bit element j of a 16-byte vector (constant j after unrolling)
__device__ inline uint16_t h16(const uint4& v, int j) {
    const uint32_t w = j < 2 ? v.x : (j < 4 ? v.y : (j < 6 ? v.z : v.w));
    return (uint16_t)((j & 1) ? (w >> 16) : (w & 0xffff));
}

// bijective XCD-aware remap (guide §5.5 T1): logical tiles t, t+1, ... land on one XCD
__device__ inline int xcd_remap(int bid, int nblk) {
    const int xcd = bid % 8, q = nblk / 8, r = nblk % 8;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + bid / 8;
}

// ---------------------------------------------------------------------------------------------
// Implicit-GEMM convolution: D[m][pix] = sum over (segment, tap, channel) of W[m][k] X[pix,tap][k]
// Block tile BM (m) x BN (pixels); 4 waves as WAVES_M x WAVES_N, each 16*WMT m x 64 pixels.
// One k-step = (segment, tap, 32-channel chunk): the X chunk (BN x 32 bf16, gathered with the
// tap offset / stride / transposed stride) and the W chunk (nparts x BM x 32 bf16) are staged
// through LDS; the next step's global loads are issued before this step's MFMAs.
// ---------------------------------------------------------------------------------------------
template <int WMT, int WAVES_M, int XPARTS>
struct ConvGeo {
    static constexpr int WAVES_N = 4 / WAVES_M;
    static constexpr int BM = 16 * WMT * WAVES_M;
    static constexpr int BN = 64 * WAVES_N;
    static constexpr int XR = BN / 64;              // 16-B X pieces per thread, plane and step
    static constexpr int WPIECES = 3 * BM * 4;      // 16-B W pieces per step (all parts)
    static constexpr int WR = (WPIECES + UNT - 1) / UNT;
};

// Output-pixel domain of a conv launch: all pixels (pclass < 0) or one parity class of a
// transposed stride-2 conv (output pixels (2yy + py, 2xx + px)), whose taps are then the
// (ky, kx) with ky = (py + pad) mod 2 (+2 ...) -- the only taps that reach such a pixel.
struct PixDom {
    int cls, py, px, Hd, Wd, P;   // Hd x Wd: the domain's grid per image
    int ky0, kx0, nty, ntx, kst;  // tap enumeration: ky = ky0 + kst * i (i < nty), likewise kx
};

__device__ inline PixDom pix_dom(const snnflow_unet_conv_args& a) {
    PixDom d;
    const int ks = a.ksize, pad = ks / 2;
    d.cls = a.pclass;
    if (d.cls < 0) {
        d.py = d.px = 0;
        d.Hd = a.Ho;
        d.Wd = a.Wo;
        d.ky0 = d.kx0 = 0;
        d.nty = d.ntx = ks;
        d.kst = 1;
    } else {
        d.py = d.cls >> 1;
        d.px = d.cls & 1;
        d.Hd = (a.Ho - d.py + 1) / 2;
        d.Wd = (a.Wo - d.px + 1) / 2;
        d.ky0 = (d.py + pad) & 1;
        d.kx0 = (d.px + pad) & 1;
        d.nty = (ks - d.ky0 + 1) / 2;
        d.ntx = (ks - d.kx0 + 1) / 2;
        d.kst = 2;
    }
    d.P = a.B * d.Hd * d.Wd;
    return d;
}

// domain pixel n -> image, output row, output column
__device__ inline void dom_pix(const PixDom& d, int n, int& b, int& y, int& x) {
    const int xx = n % d.Wd, rest = n / d.Wd;
    const int yy = rest % d.Hd;
    b = rest / d.Hd;
    y = d.cls < 0 ? yy : 2 * yy + d.py;
    x = d.cls < 0 ? xx : 2 * xx + d.px;
}

// Per-channel LIF constants of output channels m .. m+3: sigmoid(leak) and clamp_min(thresh, 0.01)
// (spiking_submodules.py:133-136), computed once per lane and channel quad, not per output element.
struct LifQuad { float lam[4], th[4]; };
__device__ inline LifQuad lif_quad(const snnflow_unet_conv_args& a, int m) {
    LifQuad q;
    if (a.epi != SNNFLOW_UNET_EPI_LIF) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            q.lam[r] = 0.0f;
            q.th[r] = 1.0f;
        }
        return q;
    }
    // the eight loads unconditional (channel clamped to the last one; unused there): one round trip
    float lk[4], t0[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int c = m + r < a.M ? m + r : a.M - 1;
        lk[r] = a.leak[c];
        t0[r] = a.thresh[c];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const bool ok = m + r < a.M;
        q.lam[r] = ok ? 1.0f / (1.0f + expf(-lk[r])) : 0.0f;
        const float th0 = ok ? t0[r] : 1.0f;
        q.th[r] = th0 < 0.01f ? 0.01f : th0;
    }
    return q;
}

// Epilogue of one output element quad (domain pixel nd, channels m .. m+3): EPI_STORE (optionally
// accumulating) or the ConvLIF update (spiking_submodules.py:121-151 / 265-300).
__device__ inline void conv_epilogue(const snnflow_unet_conv_args& a, const PixDom& dom, int nd, int m, float v0,
                                     float v1, float v2, float v3, const LifQuad& lq) {
    const float v[4] = {v0, v1, v2, v3};
    const int64_t Pfull = (int64_t)a.B * a.Ho * a.Wo;
    const int64_t plane = Pfull * a.M;
    int ob, oy, ox;
    dom_pix(dom, nd, ob, oy, ox);
    const int64_t n = ((int64_t)ob * a.Ho + oy) * a.Wo + ox;
    if (a.epi == SNNFLOW_UNET_EPI_STORE) {
        float* o = a.out + n * a.ld + m;
        if (m + 3 < a.M) {
            float4 val = make_float4(v[0], v[1], v[2], v[3]);
            if (a.accumulate) {
                const float4 old = *reinterpret_cast<const float4*>(o);
                val = make_float4(old.x + val.x, old.y + val.y, old.z + val.z, old.w + val.w);
            }
            *reinterpret_cast<float4*>(o) = val;
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (m + r < a.M) o[r] = a.accumulate ? o[r] + v[r] : v[r];
        }
        return;
    }
    // ConvLIF, M = hidden channels (multiple of 4)
    const int64_t e0 = n * a.M + m;
    float vp[4] = {0.f, 0.f, 0.f, 0.f}, zp[4] = {0.f, 0.f, 0.f, 0.f}, rs[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.prev_state) {
        const float4 tv = *reinterpret_cast<const float4*>(a.prev_state + e0);
        const float4 tz = *reinterpret_cast<const float4*>(a.prev_state + plane + e0);
        vp[0] = tv.x; vp[1] = tv.y; vp[2] = tv.z; vp[3] = tv.w;
        zp[0] = tz.x; zp[1] = tz.y; zp[2] = tz.z; zp[3] = tz.w;
    }
    if (a.residual) {
        const uint2 rr = *reinterpret_cast<const uint2*>(a.residual + n * a.res_pitch + m);
        rs[0] = bf2f(rr.x & 0xffff); rs[1] = bf2f(rr.x >> 16); rs[2] = bf2f(rr.y & 0xffff); rs[3] = bf2f(rr.y >> 16);
    }
    float vo[4], zo[4];
    uint16_t ob16[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float lam = lq.lam[r], th = lq.th[r];
        vo[r] = a.hard_reset ? ((vp[r] * lam) * (1.0f - zp[r])) + ((1.0f - lam) * v[r])
                             : ((vp[r] * lam) + ((1.0f - lam) * v[r])) - (zp[r] * th);
        zo[r] = (vo[r] - th > 0.0f) ? 1.0f : 0.0f;
        ob16[r] = f2bf(a.residual ? zo[r] + rs[r] : zo[r]);
    }
    *reinterpret_cast<float4*>(a.state + e0) = make_float4(vo[0], vo[1], vo[2], vo[3]);
    *reinterpret_cast<float4*>(a.state + plane + e0) = make_float4(zo[0], zo[1], zo[2], zo[3]);
    *reinterpret_cast<float4*>(a.current + e0) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<uint2*>(a.act + n * a.act_pitch + m) =
        make_uint2((uint32_t)ob16[0] | ((uint32_t)ob16[1] << 16), (uint32_t)ob16[2] | ((uint32_t)ob16[3] << 16));
}

// The epilogue of a lane's four output quads (channels m .. m+3 of domain pixels nd[j], j = 0..3; lanes
// whose m >= M or nd[j] >= P skip that quad): every load the four need (the old output values, the
// previous state, the residual) is issued before the first use -- one round trip instead of one per quad
// (a load inside conv_epilogue's conditionals made the compiler wait for it before the next quad).
// Loads of skipped quads read element 0 of the same tensor; the values are not used.
__device__ inline void conv_epilogue4(const snnflow_unet_conv_args& a, const PixDom& dom, int m, const int (&nd)[4],
                                      const fx4 (&v)[4], const LifQuad& lq) {
    const int64_t Pfull = (int64_t)a.B * a.Ho * a.Wo;
    const int64_t plane = Pfull * a.M;
    bool ok[4];
    int64_t n[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        ok[j] = m < a.M && nd[j] < dom.P;
        int ob, oy, ox;
        dom_pix(dom, ok[j] ? nd[j] : 0, ob, oy, ox);
        n[j] = ((int64_t)ob * a.Ho + oy) * a.Wo + ox;
    }
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.epi == SNNFLOW_UNET_EPI_STORE) {
        if (m + 3 >= a.M) {  // a partial channel quad (M not a multiple of 4): element-wise
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (ok[j]) conv_epilogue(a, dom, nd[j], m, v[j][0], v[j][1], v[j][2], v[j][3], lq);
            return;
        }
        float4 old[4] = {z4, z4, z4, z4};
        if (a.accumulate) {
#pragma unroll
            for (int j = 0; j < 4; ++j) old[j] = *reinterpret_cast<const float4*>(a.out + (ok[j] ? n[j] * a.ld + m : 0));
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!ok[j]) continue;
            float4 val = make_float4(v[j][0], v[j][1], v[j][2], v[j][3]);
            if (a.accumulate) val = make_float4(old[j].x + val.x, old[j].y + val.y, old[j].z + val.z, old[j].w + val.w);
            *reinterpret_cast<float4*>(a.out + n[j] * a.ld + m) = val;
        }
        return;
    }
    // ConvLIF (M = hidden channels, a multiple of 4): previous state and residual of all four quads first
    float4 tv[4] = {z4, z4, z4, z4}, tz[4] = {z4, z4, z4, z4};
    uint2 rr[4] = {make_uint2(0u, 0u), make_uint2(0u, 0u), make_uint2(0u, 0u), make_uint2(0u, 0u)};
    if (a.prev_state) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t e0 = ok[j] ? n[j] * a.M + m : 0;
            tv[j] = *reinterpret_cast<const float4*>(a.prev_state + e0);
            tz[j] = *reinterpret_cast<const float4*>(a.prev_state + plane + e0);
        }
    }
    if (a.residual) {
#pragma unroll
        for (int j = 0; j < 4; ++j) rr[j] = *reinterpret_cast<const uint2*>(a.residual + (ok[j] ? n[j] * a.res_pitch + m : 0));
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (!ok[j]) continue;
        const int64_t e0 = n[j] * a.M + m;
        const float vp[4] = {tv[j].x, tv[j].y, tv[j].z, tv[j].w}, zp[4] = {tz[j].x, tz[j].y, tz[j].z, tz[j].w};
        const float rs[4] = {bf2f(rr[j].x & 0xffff), bf2f(rr[j].x >> 16), bf2f(rr[j].y & 0xffff), bf2f(rr[j].y >> 16)};
        float vo[4], zo[4];
        uint16_t ob16[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float lam = lq.lam[r], th = lq.th[r];
            vo[r] = a.hard_reset ? ((vp[r] * lam) * (1.0f - zp[r])) + ((1.0f - lam) * v[j][r])
                                 : ((vp[r] * lam) + ((1.0f - lam) * v[j][r])) - (zp[r] * th);
            zo[r] = (vo[r] - th > 0.0f) ? 1.0f : 0.0f;
            ob16[r] = f2bf(a.residual ? zo[r] + rs[r] : zo[r]);
        }
        *reinterpret_cast<float4*>(a.state + e0) = make_float4(vo[0], vo[1], vo[2], vo[3]);
        *reinterpret_cast<float4*>(a.state + plane + e0) = make_float4(zo[0], zo[1], zo[2], zo[3]);
        *reinterpret_cast<float4*>(a.current + e0) = make_float4(v[j][0], v[j][1], v[j][2], v[j][3]);
        *reinterpret_cast<uint2*>(a.act + n[j] * a.act_pitch + m) =
            make_uint2((uint32_t)ob16[0] | ((uint32_t)ob16[1] << 16), (uint32_t)ob16[2] | ((uint32_t)ob16[3] << 16));
    }
}

// Segment k of the launch through constant kernarg indices (a dynamic index would copy the array to scratch).
__device__ inline snnflow_unet_seg seg_at(const snnflow_unet_conv_args& a, int k) {
    snnflow_unet_seg r = a.seg[0];
#pragma unroll
    for (int i = 1; i < SNNFLOW_UNET_MAX_SEGS; ++i)
        if (k == i) r = a.seg[i];
    return r;
}

// XPARTS == 1: X exact in bf16 (one plane), the weight parts of the segment (nparts) multiply it.
// XPARTS == 3: X is an fp32 tensor as hi / mid / lo planes (a.xpart apart); the products above
// 2^-24 relative are formed: X_hi x (W_hi, W_mid, W_lo), X_mid x (W_hi, W_mid), X_lo x W_hi.
template <int WMT, int WAVES_M, int XPARTS>
__global__ __launch_bounds__(UNT) void k_unet_conv(snnflow_unet_conv_args a) {
    using G = ConvGeo<WMT, WAVES_M, XPARTS>;
    constexpr int BM = G::BM, BN = G::BN;
    __shared__ __attribute__((aligned(16))) __bf16 Xs[XPARTS * BN * XP];
    // spike inputs stage the weight parts through LDS (shared by the block's WAVES_N waves); the
    // three-plane gradient inputs read each wave's weight fragments straight from global memory
    constexpr bool DW = XPARTS == 3;
    __shared__ __attribute__((aligned(16))) __bf16 Ws[DW ? 8 : 3 * BM * XP];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave % WAVES_M, wn = wave / WAVES_M;
    const PixDom dom = pix_dom(a);
    const int P = dom.P;
    const int mtiles = (a.M + BM - 1) / BM, ntiles = (P + BN - 1) / BN, ntc = mtiles * ntiles;
    const int ksplit = a.ksplit > 1 ? a.ksplit : 1;
    const int tl = xcd_remap(blockIdx.x, ntc * ksplit);
    const int split = tl / ntc, t = tl - split * ntc;
    const int m0 = (t % mtiles) * BM, n0 = (t / mtiles) * BN;
    const int ks = a.ksize, pad = ks / 2;
    const int taps = dom.nty * dom.ntx;
    const int64_t wpart = (int64_t)ks * ks * a.kct * a.mpad * 32;

    // this thread's X pieces: pixel (tid >> 2) + 64 r of the tile, 16-B piece q = tid & 3
    const int q = tid & 3;
    int pb[G::XR], py[G::XR], px[G::XR];
    bool pv[G::XR];
#pragma unroll
    for (int r = 0; r < G::XR; ++r) {
        const int n = n0 + (tid >> 2) + 64 * r;
        pv[r] = n < P;
        dom_pix(dom, pv[r] ? n : 0, pb[r], py[r], px[r]);
    }

    uint4 xr[XPARTS][G::XR], wr[DW ? 1 : G::WR];
    bf16x8 wf[DW ? WMT : 1][3];
    const uint4 z4 = make_uint4(0u, 0u, 0u, 0u);
    // global loads of one k-step (segment sg, tap index ti of the domain, chunk kc) into registers
    auto load = [&](const snnflow_unet_seg& sg, int ti, int kc) {
        const int ty_ = ti / dom.ntx;
        const int ky = dom.ky0 + dom.kst * ty_, kx = dom.kx0 + dom.kst * (ti - ty_ * dom.ntx);
        const int tap = ky * ks + kx;
        const int mode = sg.mode, H = sg.H, W = sg.W, cp = sg.cpitch;
#pragma unroll
        for (int r = 0; r < G::XR; ++r) {
            int iy, ix;
            bool ok = pv[r];
            if (mode == SNNFLOW_UNET_MODE_S1) {
                iy = py[r] + ky - pad;
                ix = px[r] + kx - pad;
            } else if (mode == SNNFLOW_UNET_MODE_S2) {
                iy = 2 * py[r] + ky - pad;
                ix = 2 * px[r] + kx - pad;
            } else {  // transposed stride 2: output pixel p receives input o with 2o + k - pad = p
                const int ty = py[r] + pad - ky, tx = px[r] + pad - kx;
                ok = ok && ty >= 0 && tx >= 0 && ((ty | tx) & 1) == 0;
                iy = ty >> 1;
                ix = tx >> 1;
            }
            ok = ok && iy >= 0 && iy < H && ix >= 0 && ix < W;
            const int64_t off = ok ? (((int64_t)pb[r] * H + iy) * W + ix) * cp + kc * 32 + q * 8 : 0;
#pragma unroll
            for (int xp = 0; xp < XPARTS; ++xp) {
                xr[xp][r] = ld16(sg.x + xp * a.xpart + off);
                if (!ok) xr[xp][r] = z4;
            }
        }
        if constexpr (DW) return;
        const int np = XPARTS == 3 ? 3 : sg.nparts;
        const int64_t wbase = ((int64_t)(tap * a.kct + sg.kc0 + kc) * a.mpad + m0) * 32;
#pragma unroll
        for (int r = 0; r < G::WR; ++r) {
            const int e = tid + r * UNT;
            const int part = e / (BM * 4), rem = e - part * (BM * 4);
            const bool ok = e < G::WPIECES && part < np;
            wr[r] = ld16(a.w + (ok ? part * wpart + wbase + (rem >> 2) * 32 + (rem & 3) * 8 : 0));
            if (!ok) wr[r] = z4;
        }
    };
    // this wave's weight fragments of one k-step (DW): the prepared layout [part][tap][kc][mpad][32]
    // makes a 16-row fragment one contiguous 1-KB read per wave
    auto load_w = [&](const snnflow_unet_seg& sg, int ti, int kc) {
        if constexpr (DW) {
            const int ty_ = ti / dom.ntx;
            const int ky = dom.ky0 + dom.kst * ty_, kx = dom.kx0 + dom.kst * (ti - ty_ * dom.ntx);
            const int tap = ky * ks + kx;
            const int64_t wbase =
                ((int64_t)(tap * a.kct + sg.kc0 + kc) * a.mpad + m0 + wm * 16 * WMT + (lane & 15)) * 32 + (lane >> 4) * 8;
#pragma unroll
            for (int i = 0; i < WMT; ++i)
#pragma unroll
                for (int p = 0; p < 3; ++p) wf[i][p] = __builtin_bit_cast(bf16x8, ld16(a.w + p * wpart + wbase + i * 16 * 32));
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int xp = 0; xp < XPARTS; ++xp)
#pragma unroll
            for (int r = 0; r < G::XR; ++r)
                *reinterpret_cast<uint4*>(&Xs[xoff(xp * BN + (tid >> 2) + 64 * r, q)]) = xr[xp][r];
#pragma unroll
        for (int r = 0; r < (DW ? 0 : G::WR); ++r) {
            const int e = tid + r * UNT;
            if (e < G::WPIECES) {
                const int part = e / (BM * 4), rem = e - part * (BM * 4);
                *reinterpret_cast<uint4*>(&Ws[xoff(part * BM + (rem >> 2), rem & 3)]) = wr[r];
            }
        }
    };

    fx4 acc[WMT][4];
#pragma unroll
    for (int i = 0; i < WMT; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fx4{0.f, 0.f, 0.f, 0.f};

    // k-steps: (segment, tap of the domain, 32-channel chunk) flattened; split-K blocks take a
    // contiguous range of them; each step's successor is loaded before the step's MFMAs
    int nits[SNNFLOW_UNET_MAX_SEGS];
    int ftot = 0;
#pragma unroll
    for (int k = 0; k < SNNFLOW_UNET_MAX_SEGS; ++k) {
        nits[k] = k < a.nseg ? taps * (a.seg[k].cpitch >> 5) : 0;
        ftot += nits[k];
    }
    const int f0 = (int)((int64_t)ftot * split / ksplit), f1 = (int)((int64_t)ftot * (split + 1) / ksplit);
    // flat step f -> segment k, tap index, chunk
    auto locate = [&](int f, int& k, int& ti, int& kc) {
        k = 0;
#pragma unroll
        for (int i = 0; i < SNNFLOW_UNET_MAX_SEGS - 1; ++i)
            if (k == i && f >= nits[i]) {
                f -= nits[i];
                k = i + 1;
            }
        const int nkc = seg_at(a, k).cpitch >> 5;
        ti = f / nkc;
        kc = f - ti * nkc;
    };
    if (f0 < f1) {
        int k, ti, kc;
        locate(f0, k, ti, kc);
        load(seg_at(a, k), ti, kc);
        load_w(seg_at(a, k), ti, kc);
    }
    for (int f = f0; f < f1; ++f) {
        int k, ti, kc;
        locate(f, k, ti, kc);
        const int np = seg_at(a, k).nparts;
        __syncthreads();  // the previous step's fragment reads are done
        store();
        __syncthreads();
        int k2 = 0, ti2 = 0, kc2 = 0;
        if (f + 1 < f1) {
            locate(f + 1, k2, ti2, kc2);
            load(seg_at(a, k2), ti2, kc2);
        }
        if constexpr (XPARTS == 1) {
            bf16x8 bx[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                bx[j] = *reinterpret_cast<const bf16x8*>(&Xs[xoff(wn * 64 + j * 16 + (lane & 15), lane >> 4)]);
#pragma unroll
            for (int i = 0; i < WMT; ++i) {
                const int row = wm * 16 * WMT + i * 16 + (lane & 15);
                for (int p = np - 1; p >= 0; --p) {  // lo, mid, hi: smallest products first
                    const bf16x8 aw = *reinterpret_cast<const bf16x8*>(&Ws[xoff(p * BM + row, lane >> 4)]);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aw, bx[j], acc[i][j], 0, 0, 0);
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < WMT; ++i) {
                const bf16x8* aw = wf[DW ? i : 0];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int col = xoff(wn * 64 + j * 16 + (lane & 15), lane >> 4);  // (BN * XP keeps the swizzle)
                    const bf16x8 xh = *reinterpret_cast<const bf16x8*>(&Xs[col]);
                    const bf16x8 xm = *reinterpret_cast<const bf16x8*>(&Xs[BN * XP + col]);
                    const bf16x8 xl = *reinterpret_cast<const bf16x8*>(&Xs[2 * BN * XP + col]);
                    // smallest first: lo*hi, mid*mid, hi*lo, mid*hi, hi*mid, hi*hi
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aw[0], xl, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aw[1], xm, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aw[2], xh, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aw[0], xm, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aw[1], xh, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aw[0], xh, acc[i][j], 0, 0, 0);
                }
            }
        }
        if (f + 1 < f1) load_w(seg_at(a, k2), ti2, kc2);  // after this step's MFMAs have read wf
    }

    // epilogue: lane holds rows m .. m+3 (4 consecutive output channels) of domain pixel nd
#pragma unroll
    for (int i = 0; i < WMT; ++i) {
        const int m = m0 + wm * 16 * WMT + i * 16 + 4 * (lane >> 4);
        if (ksplit > 1) {  // split-K: this split's partial sums, reduced by k_unet_conv_reduce
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int nd = n0 + wn * 64 + j * 16 + (lane & 15);
                if (nd >= P || m >= a.M) continue;
                const fx4 v = acc[i][j];
                float* o = a.partial + ((int64_t)split * P + nd) * a.M + m;
                if (m + 3 < a.M && (a.M & 3) == 0) {
                    *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (m + r < a.M) o[r] = v[r];
                }
            }
            continue;
        }
        const LifQuad lq = lif_quad(a, m);
        const int nd[4] = {n0 + wn * 64 + (lane & 15), n0 + wn * 64 + 16 + (lane & 15), n0 + wn * 64 + 32 + (lane & 15),
                           n0 + wn * 64 + 48 + (lane & 15)};
        const fx4 v[4] = {acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
        conv_epilogue4(a, dom, m, nd, v, lq);
    }
}

// ---------------------------------------------------------------------------------------------
// The same implicit GEMM for exact-in-bf16 inputs (XPARTS = 1) with its operands brought in by
// LDS-DMA (gfx950 global_load_lds_dwordx4 / buffer_load_dwordx4 ... lds): every k-step's X and W
// tiles go from global memory straight into one of NSTAGE LDS buffers, NSTAGE - 1 k-steps ahead of
// the MFMAs that read them -- no registers hold them in flight and there is no LDS store phase, so
// one barrier per k-step and a two-step lookahead replace the register-staged single-step pipeline.
// LDS rows are 64 B (32 bf16) with the four 16-B pieces of row n XOR-swizzled by (n >> 2) & 3, so the
// 16 lanes of a ds_read_b128 phase (16 consecutive rows, one piece) hit 16 distinct bank groups;
// the swizzle is applied on the load side (lane writes slot (n, s) with piece s ^ swz(n)).
// X pixels outside the input (padding, transposed-conv holes) come from a buffer load whose offset
// lies past the segment's extent: zeros.
// ---------------------------------------------------------------------------------------------
template <int N>
__device__ inline void wait_vm() {  // s_waitcnt vmcnt(N), the other counters untouched
    static_assert(N >= 0 && N < 64, "vmcnt");
    __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | (7 << 4) | (15 << 8));
}
// ds_read_b128 serves a wave in four 16-lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31} and the same
// +32 (MI355X_MICROARCH.md, LDS); a group of the operand reads (lane -> row base + (lane & 15), piece
// lane >> 4) holds rows r + 4q (q = 0..3) of each residue r = row mod 4 with pieces {g, g^1, g^1, g}
// (g = the group's lowest piece).  Row n's 16-B slot in its 256-B bank row is 4 (n mod 4) + piece';
// with piece' = piece ^ ((n >> 2) & 2) the four q of every residue land on four distinct slots:
// conflict-free.  (A (n >> 2) & 3 swizzle is 2-way on these groups.)
__device__ inline int swz(int n) { return (n >> 2) & 2; }

typedef __attribute__((address_space(3))) void lds_void;

template <int WMT, int WAVES_M, int NSTAGE>
__global__ __launch_bounds__(UNT) void k_unet_conv_dma(snnflow_unet_conv_args a) {
    using G = ConvGeo<WMT, WAVES_M, 1>;
    constexpr int BM = G::BM, BN = G::BN;
    constexpr int XB = BN * 64;                   // X tile bytes: BN rows x 32 bf16
    constexpr int WSL = 3 * BM * 4;               // W 16-B slots: 3 parts x BM rows x 4 pieces
    constexpr int LW = (WSL / 64 + 3) / 4;        // W wave-loads per wave (uniform; tail slots are dummies)
    constexpr int LX = BN / 64;                   // X wave-loads per wave (4 BN slots / 64 lanes / 4 waves)
    constexpr int LPS = LX + LW;                  // loads per wave and k-step
    constexpr int WB = 4 * LW * 1024;
    constexpr int SB = XB + WB;
    static_assert(4 * LW * 64 >= WSL, "W slots");
    __shared__ __attribute__((aligned(1024))) char lds[NSTAGE * SB];

    const int tid = threadIdx.x, lane = tid & 63, gq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave % WAVES_M, wn = wave / WAVES_M;
    const PixDom dom = pix_dom(a);
    const int P = dom.P;
    const int mtiles = (a.M + BM - 1) / BM, ntiles = (P + BN - 1) / BN, ntc = mtiles * ntiles;
    const int ksplit = a.ksplit > 1 ? a.ksplit : 1;
    const int tl = xcd_remap(blockIdx.x, ntc * ksplit);
    const int split = tl / ntc, t = tl - split * ntc;
    const int m0 = (t % mtiles) * BM, n0 = (t / mtiles) * BN;
    const int ks = a.ksize, pad = ks / 2;
    const int taps = dom.nty * dom.ntx;
    const int64_t wpart = (int64_t)ks * ks * a.kct * a.mpad * 32;

    // this lane's X slots: wave-load j = wave * LX + i, slot e = 64 j + lane -> tile row e >> 2, slot e & 3
    int pb[LX], py[LX], px[LX], xq[LX];
    bool pv[LX];
#pragma unroll
    for (int i = 0; i < LX; ++i) {
        const int e = (wave * LX + i) * 64 + lane, r = e >> 2;
        const int n = n0 + r;
        pv[i] = n < P;
        dom_pix(dom, pv[i] ? n : 0, pb[i], py[i], px[i]);
        xq[i] = (e & 3) ^ swz(r);
    }
    // W slots: wave-load j = wave * LW + i, slot e -> part, row, piece (dummy slots reload slot 0)
    int wofs[LW];
#pragma unroll
    for (int i = 0; i < LW; ++i) {
        int e = (wave * LW + i) * 64 + lane;
        if (e >= WSL) e = 0;
        const int part = e / (BM * 4), rem = e - part * (BM * 4), rr = rem >> 2;
        wofs[i] = (m0 + rr) * 32 + (((rem & 3) ^ swz(rr)) * 8);
        wofs[i] |= part << 28;  // part in the top bits (offsets < 2^28 elements per part row block)
    }

    int nits[SNNFLOW_UNET_MAX_SEGS];
    int ftot = 0;
#pragma unroll
    for (int k = 0; k < SNNFLOW_UNET_MAX_SEGS; ++k) {
        nits[k] = k < a.nseg ? taps * (a.seg[k].cpitch >> 5) : 0;
        ftot += nits[k];
    }
    const int f0 = (int)((int64_t)ftot * split / ksplit), f1 = (int)((int64_t)ftot * (split + 1) / ksplit);

    // k-step iterator (segment k, tap (ty, tx) of the domain, 32-channel chunk kc): wave-uniform, advanced
    // incrementally -- the flat-index divisions run once per block, not per k-step
    struct It { int k, ty, tx, kc; };
    auto start = [&](int f) {
        It it;
        it.k = 0;
#pragma unroll
        for (int i = 0; i < SNNFLOW_UNET_MAX_SEGS - 1; ++i)
            if (it.k == i && f >= nits[i]) {
                f -= nits[i];
                it.k = i + 1;
            }
        const int nkc = seg_at(a, it.k).cpitch >> 5;
        const int ti = f / nkc;
        it.kc = f - ti * nkc;
        it.ty = ti / dom.ntx;
        it.tx = ti - it.ty * dom.ntx;
        return it;
    };
    auto advance = [&](It& it) {
        if (++it.kc == (seg_at(a, it.k).cpitch >> 5)) {
            it.kc = 0;
            if (++it.tx == dom.ntx) {
                it.tx = 0;
                if (++it.ty == dom.nty) {
                    it.ty = 0;
                    ++it.k;
                }
            }
        }
    };

    // per segment, per lane: element offset of each X slot's pixel at tap (0, 0) (+ its piece), the
    // taps inside the input as a bit mask, and each W slot's element offset (part chosen for nparts):
    // a k-step's load address is then one add and one bit test
    int cur_k = -1, sW = 0, scp = 0, snp = 0, skc0 = 0;
    int xbase[LX], wsel[LW];
    uint32_t vmask[LX];
    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(a.seg[0].x), (short)0, 0, 0x00020000);
    auto load_seg = [&](int k) {
        const snnflow_unet_seg sg = seg_at(a, k);
        const int H = sg.H, W = sg.W, cp = sg.cpitch;
        const bool s2 = sg.mode == SNNFLOW_UNET_MODE_S2;
        rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(sg.x), (short)0,
                                               (int)((int64_t)a.B * H * W * cp * 2), 0x00020000);
        sW = W;
        scp = cp;
        snp = sg.nparts;
        skc0 = sg.kc0;
#pragma unroll
        for (int i = 0; i < LX; ++i) {
            const int iy0 = (s2 ? 2 * py[i] : py[i]) - pad, ix0 = (s2 ? 2 * px[i] : px[i]) - pad;
            xbase[i] = ((pb[i] * H + iy0) * W + ix0) * cp + xq[i] * 8;
            uint32_t m = 0u;
            if (pv[i])
                for (int ky = 0; ky < ks; ++ky)
                    for (int kx = 0; kx < ks; ++kx)
                        if (iy0 + ky >= 0 && iy0 + ky < H && ix0 + kx >= 0 && ix0 + kx < W) m |= 1u << (ky * ks + kx);
            vmask[i] = m;
        }
#pragma unroll
        for (int i = 0; i < LW; ++i) {
            int part = (int)((uint32_t)wofs[i] >> 28);
            if (part >= snp) part = 0;  // unused part of this segment: a harmless duplicate load
            wsel[i] = part * (int)wpart + (wofs[i] & 0x0fffffff);
        }
    };
    uint32_t npq = 0u;  // nparts of the issued, not yet computed k-steps: 2 bits per stage buffer
    // the LPS loads of k-step `it` into stage buffer b
    auto issue = [&](const It& it, int b) {
        if (it.k != cur_k) {
            load_seg(it.k);
            cur_k = it.k;
        }
        const int ky = dom.ky0 + dom.kst * it.ty, kx = dom.kx0 + dom.kst * it.tx;
        const int tap = ky * ks + kx;
        const int sdelta = (ky * sW + kx) * scp + it.kc * 32;
        char* const sb = lds + b * SB;
#pragma unroll
        for (int i = 0; i < LX; ++i) {
            const uint32_t off = ((vmask[i] >> tap) & 1u) ? (uint32_t)(xbase[i] + sdelta) * 2u : 0x80000000u;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void*)(sb + (wave * LX + i) * 1024), 16, off, 0, 0, 0);
        }
        const uint16_t* wb = a.w + ((int64_t)(tap * a.kct + skc0 + it.kc) * a.mpad) * 32;
#pragma unroll
        for (int i = 0; i < LW; ++i)
            __builtin_amdgcn_global_load_lds((const void*)(wb + wsel[i]), (lds_void*)(sb + XB + (wave * LW + i) * 1024), 16, 0, 0);
        npq |= (uint32_t)snp << (2 * b);
    };

    fx4 acc[WMT][4];
#pragma unroll
    for (int i = 0; i < WMT; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fx4{0.f, 0.f, 0.f, 0.f};

    It iss = start(f0);  // the next k-step to issue
#pragma unroll
    for (int i = 0; i < NSTAGE - 1; ++i)
        if (f0 + i < f1) {
            issue(iss, i);
            advance(iss);
        }
    for (int f = f0; f < f1; ++f) {
        const int ahead = f1 - 1 - f;  // k-steps issued after f (at most NSTAGE - 2)
        if constexpr (NSTAGE >= 3) {
            if (ahead >= 1) wait_vm<LPS>();
            else wait_vm<0>();
        } else {
            wait_vm<0>();
        }
        __syncthreads();  // stage f in LDS for every wave; every wave is done with stage f - 1
        const int bcur = (f - f0) % NSTAGE;  // (split-K blocks start at f0)
        const int np = (int)((npq >> (2 * bcur)) & 3u);
        npq &= ~(3u << (2 * bcur));
        if (f + NSTAGE - 1 < f1) {
            issue(iss, (f - f0 + NSTAGE - 1) % NSTAGE);
            advance(iss);
        }
        const char* sb = lds + bcur * SB;
        bf16x8 bx[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = wn * 64 + j * 16 + (lane & 15);
            bx[j] = *reinterpret_cast<const bf16x8*>(sb + (n * 4 + (gq ^ swz(n))) * 16);
        }
#pragma unroll
        for (int i = 0; i < WMT; ++i) {
            const int row = wm * 16 * WMT + i * 16 + (lane & 15);
            for (int p = np - 1; p >= 0; --p) {  // lo, mid, hi: smallest products first
                const bf16x8 aw = *reinterpret_cast<const bf16x8*>(sb + XB + ((p * BM + row) * 4 + (gq ^ swz(row))) * 16);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aw, bx[j], acc[i][j], 0, 0, 0);
            }
        }
    }

#pragma unroll
    for (int i = 0; i < WMT; ++i) {
        const int m = m0 + wm * 16 * WMT + i * 16 + 4 * (lane >> 4);
        if (ksplit > 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int nd = n0 + wn * 64 + j * 16 + (lane & 15);
                if (nd >= P || m >= a.M) continue;
                const fx4 v = acc[i][j];
                float* o = a.partial + ((int64_t)split * P + nd) * a.M + m;
                if (m + 3 < a.M && (a.M & 3) == 0) {
                    *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (m + r < a.M) o[r] = v[r];
                }
            }
            continue;
        }
        const LifQuad lq = lif_quad(a, m);
        const int nd[4] = {n0 + wn * 64 + (lane & 15), n0 + wn * 64 + 16 + (lane & 15), n0 + wn * 64 + 32 + (lane & 15),
                           n0 + wn * 64 + 48 + (lane & 15)};
        const fx4 v[4] = {acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
        conv_epilogue4(a, dom, m, nd, v, lq);
    }
}

// Input gradients (XPARTS = 3: the fp32 gradient as hi / mid / lo bf16 planes, one segment, stride 1
// or a parity class of the transposed stride-2 conv) with the three X planes brought in by LDS-DMA,
// double-buffered, and each wave's weight fragments (DW layout) as register loads issued for the next
// k-step right after the m-tile that used them.  Addresses as in k_unet_conv_dma: per-lane pixel bases
// and tap masks set once, an incremental k-step iterator; in a parity class the input pixel of domain
// tap (ty, tx) is (iy0 - ty, ix0 - tx), a stride-1 tap adds (ty, tx).
template <int WMT, int WAVES_M>
__global__ __launch_bounds__(UNT) void k_unet_dgrad_dma(snnflow_unet_conv_args a) {
    using G = ConvGeo<WMT, WAVES_M, 3>;
    constexpr int BM = G::BM, BN = G::BN, NSTAGE = 2;
    constexpr int XB = BN * 64;                   // one plane's tile bytes
    constexpr int LX = BN / 64;                   // wave-loads per wave and plane
    constexpr int SB = 3 * XB;
    __shared__ __attribute__((aligned(1024))) char lds[NSTAGE * SB];

    const int tid = threadIdx.x, lane = tid & 63, gq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave % WAVES_M, wn = wave / WAVES_M;
    const PixDom dom = pix_dom(a);
    const int P = dom.P;
    const int mtiles = (a.M + BM - 1) / BM, ntiles = (P + BN - 1) / BN, ntc = mtiles * ntiles;
    const int ksplit = a.ksplit > 1 ? a.ksplit : 1;
    const int tl = xcd_remap(blockIdx.x, ntc * ksplit);
    const int split = tl / ntc, t = tl - split * ntc;
    const int m0 = (t % mtiles) * BM, n0 = (t / mtiles) * BN;
    const int ks = a.ksize, pad = ks / 2;
    const int wpart = (int)((int64_t)ks * ks * a.kct * a.mpad * 32);
    const snnflow_unet_seg sg = a.seg[0];
    const int H = sg.H, W = sg.W, cp = sg.cpitch, nkc = cp >> 5;
    const bool t2 = sg.mode == SNNFLOW_UNET_MODE_T2;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint16_t*>(sg.x), (short)0, (int)(2 * a.xpart + (int64_t)a.B * H * W * cp) * 2, 0x00020000);

    // this lane's X slots (the same pixels in all three planes): pixel base at domain tap (0, 0), tap mask
    int xbase[LX];
    uint32_t vmask[LX];
#pragma unroll
    for (int i = 0; i < LX; ++i) {
        const int e = (wave * LX + i) * 64 + lane, r = e >> 2;
        const int n = n0 + r;
        int pb, py, px;
        dom_pix(dom, n < P ? n : 0, pb, py, px);
        const int q = (e & 3) ^ swz(r);
        // domain tap (ty, tx) reads input (iy0 + sy ty, ix0 + sy tx)
        const int iy0 = t2 ? (py + pad - dom.ky0) >> 1 : py - pad, ix0 = t2 ? (px + pad - dom.kx0) >> 1 : px - pad;
        const int sy = t2 ? -1 : 1;
        xbase[i] = ((pb * H + iy0) * W + ix0) * cp + q * 8;
        uint32_t m = 0u;
        if (n < P)
            for (int ty = 0; ty < dom.nty; ++ty)
                for (int tx = 0; tx < dom.ntx; ++tx) {
                    const int iy = iy0 + sy * ty, ix = ix0 + sy * tx;
                    // (t2: py + pad - ky >= 0 for the class's taps is iy >= 0)
                    if (iy >= 0 && iy < H && ix >= 0 && ix < W) m |= 1u << (ty * dom.ntx + tx);
                }
        vmask[i] = m;
    }
    const int sy = t2 ? -1 : 1;
    const int wlane = (m0 + wm * 16 * WMT + (lane & 15)) * 32 + gq * 8;  // this lane's fragment row / piece

    const int taps = dom.nty * dom.ntx, ftot = taps * nkc;
    const int f0 = (int)((int64_t)ftot * split / ksplit), f1 = (int)((int64_t)ftot * (split + 1) / ksplit);
    struct It { int ty, tx, kc; };
    It iss;
    {
        const int ti = f0 / nkc;
        iss.kc = f0 - ti * nkc;
        iss.ty = ti / dom.ntx;
        iss.tx = ti - iss.ty * dom.ntx;
    }
    auto advance = [&](It& it) {
        if (++it.kc == nkc) {
            it.kc = 0;
            if (++it.tx == dom.ntx) {
                it.tx = 0;
                ++it.ty;
            }
        }
    };
    auto wstep = [&](const It& it) {  // element offset of k-step it's weight rows (part 0)
        const int ky = dom.ky0 + dom.kst * it.ty, kx = dom.kx0 + dom.kst * it.tx;
        return ((ky * ks + kx) * a.kct + sg.kc0 + it.kc) * a.mpad * 32;
    };
    auto issue_x = [&](const It& it, int b) {
        const int tbit = it.ty * dom.ntx + it.tx;
        const int sdelta = sy * (it.ty * W + it.tx) * cp + it.kc * 32;
        char* const sb = lds + b * SB;
#pragma unroll
        for (int xp = 0; xp < 3; ++xp)
#pragma unroll
            for (int i = 0; i < LX; ++i) {
                const uint32_t off = ((vmask[i] >> tbit) & 1u) ? (uint32_t)(xp * (int)a.xpart + xbase[i] + sdelta) * 2u
                                                              : 0x80000000u;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void*)(sb + xp * XB + (wave * LX + i) * 1024), 16, off,
                                                         0, 0, 0);
            }
    };
    bf16x8 wf[WMT][3];
    auto load_wi = [&](int ws, int i) {
#pragma unroll
        for (int p = 0; p < 3; ++p)
            wf[i][p] = __builtin_bit_cast(bf16x8, ld16(a.w + p * wpart + ws + wlane + i * 16 * 32));
    };

    fx4 acc[WMT][4];
#pragma unroll
    for (int i = 0; i < WMT; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fx4{0.f, 0.f, 0.f, 0.f};

    if (f0 < f1) {
        issue_x(iss, 0);
        const int ws = wstep(iss);
#pragma unroll
        for (int i = 0; i < WMT; ++i) load_wi(ws, i);
        advance(iss);
    }
    for (int f = f0; f < f1; ++f) {
        wait_vm<0>();     // this k-step's planes (DMA) and weight fragments (registers) have landed
        __syncthreads();  // ... for every wave; every wave is done with the other buffer
        const bool more = f + 1 < f1;
        const int ws_next = more ? wstep(iss) : 0;
        if (more) issue_x(iss, (f - f0 + 1) & 1);
        const char* sb = lds + ((f - f0) & 1) * SB;
#pragma unroll
        for (int i = 0; i < WMT; ++i) {
            const bf16x8 w0 = wf[i][0], w1 = wf[i][1], w2 = wf[i][2];
            if (more) load_wi(ws_next, i);  // the next k-step's fragments of this m-tile, in flight from here
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = wn * 64 + j * 16 + (lane & 15);
                const int o = (n * 4 + (gq ^ swz(n))) * 16;
                const bf16x8 xh = *reinterpret_cast<const bf16x8*>(sb + o);
                const bf16x8 xm = *reinterpret_cast<const bf16x8*>(sb + XB + o);
                const bf16x8 xl = *reinterpret_cast<const bf16x8*>(sb + 2 * XB + o);
                // smallest first: lo*hi, mid*mid, hi*lo, mid*hi, hi*mid, hi*hi
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, xl, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, xm, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2, xh, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, xm, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, xh, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, xh, acc[i][j], 0, 0, 0);
            }
        }
        if (more) advance(iss);
    }

#pragma unroll
    for (int i = 0; i < WMT; ++i) {
        const int m = m0 + wm * 16 * WMT + i * 16 + 4 * (lane >> 4);
        if (ksplit > 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int nd = n0 + wn * 64 + j * 16 + (lane & 15);
                if (nd >= P || m >= a.M) continue;
                const fx4 v = acc[i][j];
                float* o = a.partial + ((int64_t)split * P + nd) * a.M + m;
                if (m + 3 < a.M && (a.M & 3) == 0) {
                    *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (m + r < a.M) o[r] = v[r];
                }
            }
            continue;
        }
        const LifQuad lq = lif_quad(a, m);
        const int nd[4] = {n0 + wn * 64 + (lane & 15), n0 + wn * 64 + 16 + (lane & 15), n0 + wn * 64 + 32 + (lane & 15),
                           n0 + wn * 64 + 48 + (lane & 15)};
        const fx4 v[4] = {acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
        conv_epilogue4(a, dom, m, nd, v, lq);
    }
}

// Split-K reduction: the partial tiles of the ksplit blocks of an output tile summed in split order
// (deterministic), then the launch's epilogue.  One thread per (domain pixel, 4 output channels).
__global__ __launch_bounds__(UNT) void k_unet_conv_reduce(snnflow_unet_conv_args a) {
    const PixDom dom = pix_dom(a);
    const int P = dom.P, mq = (a.M + 3) / 4;
    const int64_t e = (int64_t)blockIdx.x * UNT + threadIdx.x;
    if (e >= (int64_t)P * mq) return;
    const int nd = (int)(e / mq), m = (int)(e - (int64_t)nd * mq) * 4;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    for (int sp = 0; sp < a.ksplit; ++sp) {
        const float* o = a.partial + ((int64_t)sp * P + nd) * a.M + m;
        if (m + 3 < a.M && (a.M & 3) == 0) {
            const float4 u = *reinterpret_cast<const float4*>(o);
            v[0] += u.x; v[1] += u.y; v[2] += u.z; v[3] += u.w;
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (m + r < a.M) v[r] += o[r];
        }
    }
    conv_epilogue(a, dom, nd, m, v[0], v[1], v[2], v[3], lif_quad(a, m));
}

// ---------------------------------------------------------------------------------------------
// Weight gradient: D[k][m] = sum_pix X[gather(pix, tap)][k] * G[pix][m] with the pixel sum as the
// GEMM K dimension.  Both operands are NHWC (channel-contiguous), the MFMA wants 8 consecutive
// pixels per lane: each thread loads 8x8 (pixel x channel) blocks with 16-B loads, transposes them
// in registers (16-bit lane shuffles) and writes 16-B rows of [channel][pixel] LDS images.
// Block tile 64 k x 64 m, 128 pixels per step (4 MFMA k-steps), 4 waves of 32 x 32; the partial
// sums of a pixel range are added to dwk with fp32 atomics.
// ---------------------------------------------------------------------------------------------
constexpr int WG_PS = 64, WG_PP = WG_PS + 8;

// 8x8 transpose of 16-bit values: in[r] = channels 0..7 of pixel r -> out[c] = pixels 0..7 of channel c
__device__ inline void transpose8x8(const uint4 (&in)[8], uint4 (&out)[8]) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        uint32_t w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint4& a = in[2 * j];
            const uint4& b = in[2 * j + 1];
            const uint32_t wa = (c >> 1) == 0 ? a.x : ((c >> 1) == 1 ? a.y : ((c >> 1) == 2 ? a.z : a.w));
            const uint32_t wb = (c >> 1) == 0 ? b.x : ((c >> 1) == 1 ? b.y : ((c >> 1) == 2 ? b.z : b.w));
            w[j] = (c & 1) ? ((wa >> 16) | (wb & 0xffff0000u)) : ((wa & 0xffffu) | (wb << 16));
        }
        out[c] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// Block tile TK (input channels k) x TM (output channels m) of one tap, WG_PS pixels per step; 4 waves
// as 2 x 2, each (TK/2) x (TM/2): per 32-pixel MFMA k-step a wave reads TK/32 X and 3*TM/32 G fragments
// (16 B per lane) for (TK/32)*(TM/32)*3 MFMAs, so the larger tiles halve the LDS reads per MFMA of
// the 64 x 64 form.  Staging: 8x8 (pixel x channel) blocks loaded with 16-B loads, transposed in
// registers, written as 16-B rows of the [channel][pixel] LDS images; the next step's loads are
// issued before this step's MFMAs.
template <int TK, int TM>
struct WgGeo {
    static constexpr int XB = TK * WG_PS / 64;          // 8x8 X blocks per step
    static constexpr int GB = 3 * TM * WG_PS / 64;      // 8x8 G blocks (3 planes)
    static constexpr int U = (XB + GB + UNT - 1) / UNT; // blocks per thread
    static constexpr int NI = TK / 32, NJ = TM / 32;    // 16-row MFMA tiles per wave (k, m)
};

template <int TK, int TM>
__global__ __launch_bounds__(UNT) void k_unet_wgrad(snnflow_unet_wgrad_args a, int ktiles, int mtiles, int nsplit,
                                                    int steps) {
    using G = WgGeo<TK, TM>;
    constexpr int NI = G::NI, NJ = G::NJ, PGS = WG_PS / 8;  // pixel groups per step
    __shared__ __attribute__((aligned(16))) __bf16 Xt[TK * WG_PP];
    __shared__ __attribute__((aligned(16))) __bf16 Gt[3 * TM * WG_PP];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wk = wave & 1, wmv = wave >> 1;
    int b = xcd_remap(blockIdx.x, (int)gridDim.x);
    const int split = b % nsplit;
    b /= nsplit;
    const int mt = b % mtiles;
    b /= mtiles;
    const int kt = b % ktiles;
    const int tap = b / ktiles;
    const int ks = a.ksize, pad = ks / 2, ky = tap / ks, kx = tap - ky * ks;
    const int P = a.B * a.Ho * a.Wo;
    const snnflow_unet_seg& sg = a.seg;
    const uint4 z4 = make_uint4(0u, 0u, 0u, 0u);

    fx4 acc[NI][NJ];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = fx4{0.f, 0.f, 0.f, 0.f};

    uint4 rg[G::U][8];
    auto load = [&](int st) {
        const int pbase = (split * steps + st) * WG_PS;
#pragma unroll
        for (int u = 0; u < G::U; ++u) {
            const int blk = tid + u * UNT;
            if (blk < G::XB) {  // X block: pixel group, channel group
                const int pg = blk % PGS, cg = blk / PGS;
                const int kk = kt * TK + cg * 8;
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const int n = pbase + pg * 8 + r;
                    bool ok = n < P && kk < sg.cpitch;
                    const int nn = ok ? n : 0;
                    const int ox = nn % a.Wo, rest = nn / a.Wo, oy = rest % a.Ho, bb = rest / a.Ho;
                    const int iy = (sg.mode == SNNFLOW_UNET_MODE_S1 ? oy : 2 * oy) + ky - pad;
                    const int ix = (sg.mode == SNNFLOW_UNET_MODE_S1 ? ox : 2 * ox) + kx - pad;
                    ok = ok && iy >= 0 && iy < sg.H && ix >= 0 && ix < sg.W;
                    rg[u][r] = ld16(sg.x + (ok ? (((int64_t)bb * sg.H + iy) * sg.W + ix) * sg.cpitch + kk : 0));
                    if (!ok) rg[u][r] = z4;
                }
            } else if (blk < G::XB + G::GB) {  // G block: plane, channel group, pixel group
                const int gb = blk - G::XB;
                const int pg = gb % PGS, cg = (gb / PGS) % (TM / 8), part = gb / (PGS * (TM / 8));
                const int mm = mt * TM + cg * 8;
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const int n = pbase + pg * 8 + r;
                    const bool ok = n < P && mm < a.gpitch;
                    rg[u][r] = ld16(a.g3 + (ok ? part * a.gpart + (int64_t)n * a.gpitch + mm : 0));
                    if (!ok) rg[u][r] = z4;
                }
            }
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int u = 0; u < G::U; ++u) {
            const int blk = tid + u * UNT;
            if (blk >= G::XB + G::GB) continue;
            uint4 tr[8];
            transpose8x8(rg[u], tr);
            if (blk < G::XB) {
                const int pg = blk % PGS, cg = blk / PGS;
#pragma unroll
                for (int c = 0; c < 8; ++c) *reinterpret_cast<uint4*>(&Xt[(cg * 8 + c) * WG_PP + pg * 8]) = tr[c];
            } else {
                const int gb = blk - G::XB;
                const int pg = gb % PGS, cg = (gb / PGS) % (TM / 8), part = gb / (PGS * (TM / 8));
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    *reinterpret_cast<uint4*>(&Gt[(part * TM + cg * 8 + c) * WG_PP + pg * 8]) = tr[c];
            }
        }
    };

    const int total_steps = (P + WG_PS - 1) / WG_PS;
    const int st0 = split * steps;
    const int nst = st0 >= total_steps ? 0 : (total_steps - st0 < steps ? total_steps - st0 : steps);
    if (nst == 0 && !a.partial) return;
    if (nst > 0) load(0);
    for (int st = 0; st < nst; ++st) {
        __syncthreads();
        store();
        __syncthreads();
        if (st + 1 < nst) load(st + 1);
#pragma unroll
        for (int kk = 0; kk < WG_PS / 32; ++kk) {
            bf16x8 ax[NI];
#pragma unroll
            for (int i = 0; i < NI; ++i)
                ax[i] = *reinterpret_cast<const bf16x8*>(
                    &Xt[(wk * (TK / 2) + i * 16 + (lane & 15)) * WG_PP + kk * 32 + (lane >> 4) * 8]);
#pragma unroll
            for (int p = 2; p >= 0; --p)
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const bf16x8 bg = *reinterpret_cast<const bf16x8*>(
                        &Gt[(p * TM + wmv * (TM / 2) + j * 16 + (lane & 15)) * WG_PP + kk * 32 + (lane >> 4) * 8]);
#pragma unroll
                    for (int i = 0; i < NI; ++i)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ax[i], bg, acc[i][j], 0, 0, 0);
                }
        }
    }
    if (a.partial) {  // this split's tile, summed in split order by k_unet_wgrad_reduce (deterministic)
        const int KP = ktiles * TK, MP = mtiles * TM;
        float* part = a.partial + ((int64_t)split * (ks * ks) + tap) * KP * MP;
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int k = kt * TK + wk * (TK / 2) + i * 16 + 4 * (lane >> 4);
                const int m = mt * TM + wmv * (TM / 2) + j * 16 + (lane & 15);
#pragma unroll
                for (int r = 0; r < 4; ++r) part[(int64_t)(k + r) * MP + m] = acc[i][j][r];
            }
        return;
    }
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int k = kt * TK + wk * (TK / 2) + i * 16 + 4 * (lane >> 4);
            const int m = mt * TM + wmv * (TM / 2) + j * 16 + (lane & 15);
            if (m >= a.M) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (k + r < sg.cpitch) atomicAdd(a.dwk + ((int64_t)tap * a.ktot + a.k0 + k + r) * a.M + m, acc[i][j][r]);
        }
}

// First pass of a two-pass split reduction (many splits): chunk c of WG_RCHUNK consecutive splits
// summed in split order into tmp[c][tap][k][m] (the layout of the partial tiles with KP = K, MP = M).
constexpr int WG_RCHUNK = 16;
__global__ void k_unet_wgrad_reduce_chunks(snnflow_unet_wgrad_args a, int nsplit, int KP, int MP, float* tmp) {
    const int taps = a.ksize * a.ksize, K = a.seg.cpitch, M = a.M;
    const int64_t n = (int64_t)taps * K * M;
    const int nch = (nsplit + WG_RCHUNK - 1) / WG_RCHUNK;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n * nch; e += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(e / n);
        const int64_t o = e - (int64_t)c * n;
        const int m = (int)(o % M);
        const int64_t r = o / M;
        const int k = (int)(r % K), tap = (int)(r / K);
        const int sp1 = (c + 1) * WG_RCHUNK < nsplit ? (c + 1) * WG_RCHUNK : nsplit;
        float sum = 0.0f;
        for (int sp = c * WG_RCHUNK; sp < sp1; ++sp) sum += a.partial[(((int64_t)sp * taps + tap) * KP + k) * MP + m];
        tmp[e] = sum;
    }
}

// dwk[tap][k0 + k][m] += sum over the splits (fixed order) of the partial tiles.
__global__ void k_unet_wgrad_reduce(snnflow_unet_wgrad_args a, int nsplit, int KP, int MP) {
    const int taps = a.ksize * a.ksize, K = a.seg.cpitch, M = a.M;
    const int64_t n = (int64_t)taps * K * M;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int m = (int)(e % M);
        const int64_t r = e / M;
        const int k = (int)(r % K), tap = (int)(r / K);
        float sum = 0.0f;
        for (int sp = 0; sp < nsplit; ++sp) sum += a.partial[(((int64_t)sp * taps + tap) * KP + k) * MP + m];
        a.dwk[((int64_t)tap * a.ktot + a.k0 + k) * M + m] += sum;
    }
}

// ---------------------------------------------------------------------------------------------
// Tap-fused weight gradient of a 3x3 conv (stride S = 1 or 2) on strips of 64 output pixels: one
// block owns a TK x TM (k x m) tile of all nine taps, so X and G are read once per k/m tile instead
// of once per tap (k_unet_wgrad re-reads them nine times; at 256^2 and 128^2 that re-read is the HBM
// traffic).  A strip is R = 64 / TW rows of TW = min(Wo, 64) output pixels; the LDS holds its input
// halo (XH x XW pixels: (R + 2) x (TW + 2) at stride 1, (2R + 1) x (2TW + 1) at stride 2),
// pixel-major [pixel][k], and the three G planes [part][pixel][m], both copied with plain 16-B
// loads.  The MFMA operands (reduction = pixels) come out column-major through ds_read_b64_tr_b16,
// every lane addressing its own pixel row, so a tap is an offset of those rows.
// 4 waves as WK x WM, each NI x NJ 16x16 tiles of every tap (9 * NI * NJ accumulators).
// ---------------------------------------------------------------------------------------------
template <int NI, int NJ, int WK, int WM, int S>
struct WrGeo {
    static constexpr int TK = 16 * NI * WK, TM = 16 * NJ * WM;
    static constexpr int XS = TK + 8, GS = TM + 8;    // bf16 per LDS pixel row (16-B multiple)
    static constexpr int XPIX = S == 1 ? 198 : 387;   // halo pixels, largest strip shape (TW 64)
    static constexpr int XQ = TK / 8, GQ = TM / 8;     // 16-B pieces per pixel
    static constexpr int GPIECES = 3 * 64 * GQ;
    static constexpr int XR = (XPIX * XQ + UNT - 1) / UNT, GR = (GPIECES + UNT - 1) / UNT;
};

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// ds_read_b64_tr_b16 pair -> one 16x16x32 operand: lane (16 g + i) receives column i of 8 pixel rows
// (the rows lanes 4q+p of its group address in r0 (rows 0..3) and r1 (rows 4..7), 4p .. 4p+3
// already added), 8 consecutive reduction elements.
__device__ inline bf16x8 tr_pair(const __bf16* r0, const __bf16* r1) {
    const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(r0));
    const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(r1));
    const short __attribute__((ext_vector_type(8))) v = __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
}

template <int NI, int NJ, int WK, int WM, int S>
__global__ __launch_bounds__(UNT) void k_unet_wgrad_rows(snnflow_unet_wgrad_args a, int ktiles, int mtiles, int nsplit,
                                                         int spb) {
    using G = WrGeo<NI, NJ, WK, WM, S>;
    constexpr int TK = G::TK, TM = G::TM, XS = G::XS, GS = G::GS;
    __shared__ __attribute__((aligned(16))) __bf16 Xs[G::XPIX * XS];
    __shared__ __attribute__((aligned(16))) __bf16 Gs[3 * 64 * GS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wk = wave % WK, wm = wave / WK;
    int b = xcd_remap(blockIdx.x, (int)gridDim.x);
    const int split = b % nsplit;
    b /= nsplit;
    const int mt = b % mtiles, kt = b / mtiles;
    const int H = a.Ho, W = a.Wo;
    const snnflow_unet_seg& sg = a.seg;
    const int Hi = sg.H, Wi = sg.W, cp = sg.cpitch;
    // strip geometry: TW output columns x R rows (TW a power of two, 8..64)
    const int TW = W < 64 ? W : 64, lgw = 31 - __builtin_clz(TW), R = 64 >> lgw;
    const int XW = S == 1 ? TW + 2 : 2 * TW + 1, XH = S == 1 ? R + 2 : 2 * R + 1, xpieces = XH * XW * G::XQ;
    const int spr = W / TW, spi = (H / R) * spr;  // strips per strip-row, per image
    const int nstrips = a.B * spi;
    const int s0 = split * spb, s1 = s0 + spb < nstrips ? s0 + spb : nstrips;
    const int kbase = kt * TK, mbase = mt * TM;
    const uint4 z4 = make_uint4(0u, 0u, 0u, 0u);

    fx4 acc[9][NI][NJ];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[t][i][j] = fx4{0.f, 0.f, 0.f, 0.f};

    uint4 xr[G::XR], gr[G::GR];
    auto load = [&](int st) {
        const int bb = st / spi, rest = st - bb * spi, oy0 = (rest / spr) * R, x0 = (rest % spr) * TW;
        const int iy0 = S * oy0 - 1, ix0 = S * x0 - 1;
#pragma unroll
        for (int r = 0; r < G::XR; ++r) {
            const int e = tid + r * UNT;
            const int pix = e / G::XQ, c8 = e - pix * G::XQ, row = pix / XW, j = pix - row * XW;
            const int iy = iy0 + row, ix = ix0 + j, kk = kbase + 8 * c8;
            const bool ok = e < xpieces && iy >= 0 && iy < Hi && ix >= 0 && ix < Wi && kk < cp;
            xr[r] = ld16(sg.x + (ok ? (((int64_t)bb * Hi + iy) * Wi + ix) * cp + kk : 0));
            if (!ok) xr[r] = z4;
        }
#pragma unroll
        for (int r = 0; r < G::GR; ++r) {
            const int e = tid + r * UNT;
            const int part = e / (64 * G::GQ), rem = e - part * (64 * G::GQ), j = rem / G::GQ, c8 = rem - j * G::GQ;
            const int mm = mbase + 8 * c8;
            const bool ok = e < G::GPIECES && mm < a.gpitch;
            // the strip's 64 output pixels are consecutive in G (whole rows when TW < W is false)
            const int64_t n = ((int64_t)bb * H + oy0 + (j >> lgw)) * W + x0 + (j & (TW - 1));
            gr[r] = ld16(a.g3 + (ok ? part * a.gpart + n * a.gpitch + mm : 0));
            if (!ok) gr[r] = z4;
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int r = 0; r < G::XR; ++r) {
            const int e = tid + r * UNT;
            if (e < xpieces) {
                const int pix = e / G::XQ, c8 = e - pix * G::XQ;
                *reinterpret_cast<uint4*>(&Xs[pix * XS + 8 * c8]) = xr[r];
            }
        }
#pragma unroll
        for (int r = 0; r < G::GR; ++r) {
            const int e = tid + r * UNT;
            if (e < G::GPIECES) {
                const int part = e / (64 * G::GQ), rem = e - part * (64 * G::GQ), j = rem / G::GQ, c8 = rem - j * G::GQ;
                *reinterpret_cast<uint4*>(&Gs[(part * 64 + j) * GS + 8 * c8]) = gr[r];
            }
        }
    };

    // this lane's pixel rows of the transposed reads: output pixel n = 32 kk + 8 g + q (+ 4)
    const int g4 = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
    int xrow[2][2];  // [kk][half]: halo pixel of the tap (0, 0)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int n = kk * 32 + g4 * 8 + q + 4 * h, r = n >> lgw, c = n & (TW - 1);
            xrow[kk][h] = S * r * XW + S * c;
        }
    if (s0 < s1) load(s0);
    for (int st = s0; st < s1; ++st) {
        __syncthreads();
        store();
        __syncthreads();
        if (st + 1 < s1) load(st + 1);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int gp = kk * 32 + g4 * 8 + q;  // G pixel row of this lane (first half)
            bf16x8 bgf[3][NJ];
#pragma unroll
            for (int part = 0; part < 3; ++part)
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const __bf16* r0 = &Gs[(part * 64 + gp) * GS + wm * (TM / WM) + j * 16 + 4 * pp];
                    bgf[part][j] = tr_pair(r0, r0 + 4 * GS);
                }
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int toff = ky * XW + kx;
                    bf16x8 axf[NI];
#pragma unroll
                    for (int i = 0; i < NI; ++i) {
                        const int col = wk * (TK / WK) + i * 16 + 4 * pp;
                        axf[i] = tr_pair(&Xs[(xrow[kk][0] + toff) * XS + col], &Xs[(xrow[kk][1] + toff) * XS + col]);
                    }
#pragma unroll
                    for (int part = 2; part >= 0; --part)  // lo, mid, hi
#pragma unroll
                        for (int j = 0; j < NJ; ++j)
#pragma unroll
                            for (int i = 0; i < NI; ++i)
                                acc[ky * 3 + kx][i][j] =
                                    __builtin_amdgcn_mfma_f32_16x16x32_bf16(axf[i], bgf[part][j], acc[ky * 3 + kx][i][j], 0, 0, 0);
                }
        }
    }
    // lane holds k rows 4 (lane >> 4) .. +3 and m column (lane & 15) of each 16 x 16 tile
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int k = kbase + wk * (TK / WK) + i * 16 + 4 * (lane >> 4);
                const int m = mbase + wm * (TM / WM) + j * 16 + (lane & 15);
                if (a.partial) {  // split partial tiles, summed in split order by k_unet_wgrad_reduce
                    const int KP = ktiles * TK, MP = mtiles * TM;
                    float* part = a.partial + ((int64_t)split * 9 + t) * KP * MP;
#pragma unroll
                    for (int r = 0; r < 4; ++r) part[(int64_t)(k + r) * MP + m] = acc[t][i][j][r];
                } else if (m < a.M) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (k + r < cp) atomicAdd(a.dwk + ((int64_t)t * a.ktot + a.k0 + k + r) * a.M + m, acc[t][i][j][r]);
                }
            }
}

__global__ void k_unet_wgrad_finalize(const float* __restrict__ dwk, int ktot, const int* __restrict__ inv, int k0,
                                      int cout, int cin, int taps, int accumulate, float* __restrict__ dw) {
    const int64_t n = (int64_t)cout * cin * taps;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int tap = (int)(e % taps);
        const int64_t r = e / taps;
        const int c = (int)(r % cin), m = (int)(r / cin);
        float s = 0.0f;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int k = inv[c * 3 + j];
            if (k >= 0) s += dwk[((int64_t)tap * ktot + k0 + k) * cout + m];
        }
        dw[e] = accumulate ? dw[e] + s : s;
    }
}

// ---------------------------------------------------------------------------------------------
// Weight operand preparation (hi / mid / lo bf16 parts in the MFMA fragment order)
// ---------------------------------------------------------------------------------------------
__global__ void k_unet_prep_weights(const float* __restrict__ w, int cout, int cin, int ks, const int* __restrict__ kmap,
                                    int transpose, int flip, int mvalid, int kc0, int nkc, int kct, int mpad,
                                    uint16_t* __restrict__ dst) {
    const int taps = ks * ks;
    const int64_t per_part = (int64_t)taps * nkc * mpad * 32;
    const int64_t n = 3 * per_part;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int part = (int)(e / per_part);
        int64_t r = e - part * per_part;
        const int kk = (int)(r % 32);
        r /= 32;
        const int m = (int)(r % mpad);
        r /= mpad;
        const int kc = (int)(r % nkc);
        const int tap = (int)(r / nkc);
        float v = 0.0f;
        if (!transpose) {
            const int c = kmap[kc * 32 + kk];
            if (m < cout && c >= 0) v = w[((int64_t)m * cin + c) * taps + tap];
        } else {
            const int co = kc * 32 + kk;
            const int c = m < mvalid ? kmap[m] : -1;
            const int st = flip ? taps - 1 - tap : tap;
            if (co < cout && c >= 0) v = w[((int64_t)co * cin + c) * taps + st];
        }
        uint16_t h, md, l;
        split3(v, h, md, l);
        const uint16_t o = part == 0 ? h : (part == 1 ? md : l);
        dst[(int64_t)part * taps * kct * mpad * 32 + (((int64_t)tap * kct + kc0 + kc) * mpad + m) * 32 + kk] = o;
    }
}

// ---------------------------------------------------------------------------------------------
// ConvLIF backward (elementwise) with the surrogate gradients of spiking_util.py
// ---------------------------------------------------------------------------------------------
__device__ inline float gauss(float x, float mu, float sigma) {
    // spiking_util.py:6-10: exp(-((x - mu) * (x - mu)) / (2 * sigma * sigma)) / (sigma * sqrt(2 pi))
    const float d = x - mu;
    return expf(-(d * d) / ((2.0f * sigma) * sigma)) / (sigma * sqrtf(2.0f * 3.14159265358979323846f));
}

__device__ inline float surrogate(float x, float w, int kind) {
    switch (kind) {
        case SNNFLOW_SG_SUPERSPIKE: {  // 1 / (1 + width * |x|) ** 2
            const float d = 1.0f + w * fabsf(x);
            return 1.0f / (d * d);
        }
        case SNNFLOW_SG_MGSPIKE:  // 1.15 N(x; 0, w) - 0.15 N(x; w, 6w) - 0.15 N(x; -w, 6w)
            return (1.15f * gauss(x, 0.0f, w) - 0.15f * gauss(x, w, 6.0f * w)) - 0.15f * gauss(x, -w, 6.0f * w);
        case SNNFLOW_SG_TRIANGLE:  // relu(1 - width * |x|)
            return fmaxf(0.0f, 1.0f - w * fabsf(x));
        default:  // arctanspike: 1 / (1 + width * x * x)
            return 1.0f / (1.0f + (w * x) * x);
    }
}

// One pixel's loads of k_unet_lif_bwd (a channel quad): issued one iteration ahead.
struct LifBwdIn { float4 go, gsv, gsz, vp, zp, vo, I; };

__global__ __launch_bounds__(UNT) void k_unet_lif_bwd(snnflow_unet_lif_bwd_args a) {
    __shared__ float red[2 * UNT * 4];  // [pixel row][2C] thread sums (ppi * C <= UNT * 4)
    const int tid = threadIdx.x;
    const int C = a.C, PQ = a.gc_pitch / 4, CQ = C / 4;
    const int ppi = UNT / PQ;  // pixels per block iteration
    const int quad = tid % PQ, pr = tid / PQ;
    const int64_t plane = (int64_t)a.P * C;
    float st[4] = {0.f, 0.f, 0.f, 0.f}, sl[4] = {0.f, 0.f, 0.f, 0.f};
    const int c0 = quad * 4;
    float lam[4] = {0.f, 0.f, 0.f, 0.f}, th[4] = {0.f, 0.f, 0.f, 0.f};
    if (quad < CQ)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            lam[r] = 1.0f / (1.0f + expf(-a.leak[c0 + r]));
            const float t0 = a.thresh[c0 + r];
            th[r] = t0 < 0.01f ? 0.01f : t0;
        }
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    auto load = [&](int64_t p) {
        LifBwdIn v = {z4, z4, z4, z4, z4, z4, z4};
        const int64_t e0 = p * C + c0;
        if (a.g_out) v.go = *reinterpret_cast<const float4*>(a.g_out + p * a.g_pitch + c0);
        if (a.g_state) {
            v.gsv = *reinterpret_cast<const float4*>(a.g_state + e0);
            v.gsz = *reinterpret_cast<const float4*>(a.g_state + plane + e0);
        }
        if (a.prev_state) {
            v.vp = *reinterpret_cast<const float4*>(a.prev_state + e0);
            v.zp = *reinterpret_cast<const float4*>(a.prev_state + plane + e0);
        }
        v.vo = *reinterpret_cast<const float4*>(a.state + e0);
        v.I = *reinterpret_cast<const float4*>(a.current + e0);
        return v;
    };
    const int64_t stride = (int64_t)gridDim.x * ppi;
    int64_t p = (int64_t)blockIdx.x * ppi + pr;
    if (pr < ppi && quad >= CQ) {  // padding channels of the gradient planes
        for (; p < a.P; p += stride) {
            uint16_t* gh = a.g_cur3 + p * a.gc_pitch + c0;
#pragma unroll
            for (int k = 0; k < 3; ++k) *reinterpret_cast<uint2*>(gh + k * a.gc_part) = make_uint2(0u, 0u);
        }
    } else if (pr < ppi && p < a.P) {
        LifBwdIn cur = load(p);
        for (; p < a.P; p += stride) {
            // the next pixel's loads go out before this one's stores (no aliasing between them)
            LifBwdIn nxt = cur;
            if (p + stride < a.P) nxt = load(p + stride);
            const int64_t e0 = p * C + c0;
            const float go[4] = {cur.go.x, cur.go.y, cur.go.z, cur.go.w};
            const float gsv[4] = {cur.gsv.x, cur.gsv.y, cur.gsv.z, cur.gsv.w};
            const float gsz[4] = {cur.gsz.x, cur.gsz.y, cur.gsz.z, cur.gsz.w};
            const float vp[4] = {cur.vp.x, cur.vp.y, cur.vp.z, cur.vp.w};
            const float zp[4] = {cur.zp.x, cur.zp.y, cur.zp.z, cur.zp.w};
            const float vo[4] = {cur.vo.x, cur.vo.y, cur.vo.z, cur.vo.w};
            const float I[4] = {cur.I.x, cur.I.y, cur.I.z, cur.I.w};
            uint16_t hh[4], mm[4], ll[4];
            float gvp[4], gzp[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float x = vo[r] - th[r];
                const float gxs = (go[r] + gsz[r]) * surrogate(x, a.width, a.surrogate);
                const float gv = gsv[r] + gxs;
                split3(gv * (1.0f - lam[r]), hh[r], mm[r], ll[r]);
                if (a.hard_reset) {
                    gvp[r] = (gv * (1.0f - zp[r])) * lam[r];
                    gzp[r] = a.detach ? 0.0f : -(gv * (vp[r] * lam[r]));
                    sl[r] += gv * ((vp[r] * (1.0f - zp[r])) - I[r]);
                    st[r] += -gxs;
                } else {
                    gvp[r] = gv * lam[r];
                    gzp[r] = a.detach ? 0.0f : -(gv * th[r]);
                    sl[r] += gv * (vp[r] - I[r]);
                    st[r] += -gxs - gv * zp[r];
                }
            }
            uint16_t* gh = a.g_cur3 + p * a.gc_pitch + c0;
            *reinterpret_cast<uint2*>(gh) = make_uint2((uint32_t)hh[0] | ((uint32_t)hh[1] << 16), (uint32_t)hh[2] | ((uint32_t)hh[3] << 16));
            *reinterpret_cast<uint2*>(gh + a.gc_part) =
                make_uint2((uint32_t)mm[0] | ((uint32_t)mm[1] << 16), (uint32_t)mm[2] | ((uint32_t)mm[3] << 16));
            *reinterpret_cast<uint2*>(gh + 2 * a.gc_part) =
                make_uint2((uint32_t)ll[0] | ((uint32_t)ll[1] << 16), (uint32_t)ll[2] | ((uint32_t)ll[3] << 16));
            if (a.g_prev) {
                *reinterpret_cast<float4*>(a.g_prev + e0) = make_float4(gvp[0], gvp[1], gvp[2], gvp[3]);
                *reinterpret_cast<float4*>(a.g_prev + plane + e0) = make_float4(gzp[0], gzp[1], gzp[2], gzp[3]);
            }
            if (a.g_res) {
                float4* gr = reinterpret_cast<float4*>(a.g_res + p * a.gres_pitch + c0);
                if (a.res_assign) {
                    *gr = cur.go;
                } else {
                    const float4 o = *gr;
                    *gr = make_float4(o.x + go[0], o.y + go[1], o.z + go[2], o.w + go[3]);
                }
            }
            cur = nxt;
        }
    }
    if (pr < ppi && quad < CQ)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            red[pr * 2 * C + c0 + r] = st[r];
            red[pr * 2 * C + C + c0 + r] = sl[r];
        }
    __syncthreads();
    // the block's sums in a fixed order (pixel rows in sequence: bit-reproducible, unlike LDS atomics)
    for (int i = tid; i < 2 * C; i += UNT) {
        float v = 0.0f;
        for (int q = 0; q < ppi; ++q) v += red[q * 2 * C + i];
        if (a.partial) {  // this block's sums; k_unet_lif_bwd_reduce adds the blocks in column order
            // column: XCD-aware (the blocks of one XCD own consecutive columns, so each 64-B line of
            // the [2C][blocks] buffer is completed in one L2 -- no partial-line write-backs)
            a.partial[(int64_t)i * gridDim.x + xcd_remap(blockIdx.x, (int)gridDim.x)] = (double)v;
        } else {
            atomicAdd(a.acc + i, (double)v);
        }
    }
}

// acc[i] += sum over blocks b of partial[i][b], in a fixed order (per thread a strided run of blocks,
// coalesced, then a fixed LDS tree): one block per sum index i.
__global__ __launch_bounds__(UNT) void k_unet_lif_bwd_reduce(const double* __restrict__ part, int nblk, int n2,
                                                             double* acc) {
    __shared__ double red[UNT];
    const int i = blockIdx.x, tid = threadIdx.x;
    double v = 0.0;
    for (int b = tid; b < nblk; b += UNT) v += part[(int64_t)i * nblk + b];
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int o = UNT / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) acc[i] += red[0];
}

__global__ void k_unet_cell_param_grads(const double* acc, const float* leak, const float* thresh, int C, int accumulate,
                                        float* g_leak, float* g_thresh) {
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < C; j += gridDim.x * blockDim.x) {
        const float s = 1.0f / (1.0f + expf(-leak[j]));
        const float gth = thresh[j] >= 0.01f ? (float)acc[j] : 0.0f;
        const float glk = ((float)acc[C + j] * (1.0f - s)) * s;
        g_thresh[j] = accumulate ? g_thresh[j] + gth : gth;
        g_leak[j] = accumulate ? g_leak[j] + glk : glk;
    }
}

// ---------------------------------------------------------------------------------------------
// Packing, decoder input (upsample + concat), prediction layers
// ---------------------------------------------------------------------------------------------
// one thread per (pixel, 8 consecutive act channels): one 16-B store, source reads coalesced along
// x (NCHW) or along the channels (NHWC)
template <typename I>
__global__ void k_unet_pack(const float* __restrict__ src, int B, int H, int W, int C, int64_t sb, int64_t sc,
                            int64_t sh, int64_t sw, int split, uint16_t* __restrict__ dst, int cpitch) {
    const int G = cpitch / 8;
    const I n = (I)B * H * W * G;
    for (I e = (I)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (I)gridDim.x * blockDim.x) {
        const int g = (int)(e % (I)G);
        const I pix = e / (I)G;
        const I py = pix / (I)W;
        const int x = (int)(pix - py * (I)W), y = (int)(py % (I)H), b = (int)(py / (I)H);
        const float* sp = src + b * sb + y * sh + x * sw;
        uint16_t o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 8 * g + j;
            const int part = split ? k / C : (k < C ? 0 : 3);
            o[j] = 0;
            if (part < 3) {
                const float v = sp[(split ? k - part * C : k) * sc];
                uint16_t hh, mm, ll;
                split3(v, hh, mm, ll);
                o[j] = split ? (part == 0 ? hh : (part == 1 ? mm : ll)) : hh;
            }
        }
        *reinterpret_cast<uint4*>(dst + pix * cpitch + 8 * g) =
            make_uint4((uint32_t)o[0] | ((uint32_t)o[1] << 16), (uint32_t)o[2] | ((uint32_t)o[3] << 16),
                       (uint32_t)o[4] | ((uint32_t)o[5] << 16), (uint32_t)o[6] | ((uint32_t)o[7] << 16));
    }
}

// bilinear x2, align_corners=False (torch area_pixel_compute_source_index with scale 1/2):
// src = max(0, (dst + 0.5) * 0.5 - 0.5); i0 = floor(src); i1 = i0 + (i0 < n - 1); l1 = src - i0
struct Lin { int i0, i1; float l0, l1; };
__device__ inline Lin lin2(int d, int n) {
    float s = ((float)d + 0.5f) * 0.5f - 0.5f;
    s = s < 0.0f ? 0.0f : s;
    Lin r;
    r.i0 = (int)s;
    r.i1 = r.i0 + (r.i0 < n - 1 ? 1 : 0);
    r.l1 = s - (float)r.i0;
    r.l0 = 1.0f - r.l1;
    return r;
}

__device__ inline void ld4bf(const uint16_t* p, float (&v)[4]) {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    v[0] = bf2f(u.x & 0xffff); v[1] = bf2f(u.x >> 16); v[2] = bf2f(u.y & 0xffff); v[3] = bf2f(u.y >> 16);
}

// (I: the element index type -- 32-bit whenever the launch's element count allows: the index
// divisions are then 32-bit, a fraction of the 64-bit emulation's instructions)
// Row-oriented decoder input: block = (output row b*H + Y, chunk of DEC_CHUNK (X, channel quad)
// elements of it), the row's vertical interpolation uniform; blocks of one XCD take consecutive
// rows (their low-res rows shared in that XCD's L2).  (X, quad) from the in-row index by a float
// reciprocal with a +-1 correction (exact for in-row indices < 2^24).
constexpr int DEC_CHUNK = 1024;

__device__ inline void row_split(int e, int Q, float invQ, int& X, int& q) {
    X = (int)((float)e * invQ);
    q = e - X * Q;
    if (q < 0) { --X; q += Q; } else if (q >= Q) { ++X; q -= Q; }
}

__global__ __launch_bounds__(256) void k_unet_dec_in(const uint16_t* __restrict__ x, int cx, int pxp,
                                                     const uint16_t* __restrict__ blk, int cb, int pbp,
                                                     const float* __restrict__ pred, int B, int h, int w,
                                                     uint16_t* __restrict__ dst, int cpitch, int nchunk) {
    const int H = 2 * h, W = 2 * w, Q = cpitch / 4;
    const int lin = xcd_remap(blockIdx.x, (int)gridDim.x);
    const int row = lin / nchunk, chunk = lin - row * nchunk;
    const int b = row / H, Y = row - b * H;
    const Lin ly = lin2(Y, h);
    const int64_t r0 = ((int64_t)b * h + ly.i0) * w, r1 = ((int64_t)b * h + ly.i1) * w;
    const float invQ = 1.0f / (float)Q;
    const int e1 = min((chunk + 1) * DEC_CHUNK, W * Q);
    uint16_t* drow = dst + (int64_t)row * W * cpitch;
    for (int e = chunk * DEC_CHUNK + (int)threadIdx.x; e < e1; e += 256) {
        int X, q;
        row_split(e, Q, invQ, X, q);
        const int k = 4 * q;
        const Lin lx = lin2(X, w);
        uint16_t o[4] = {0, 0, 0, 0};
        const uint16_t* src = nullptr;
        int sp = 0, c = 0;
        if (k < cx) {
            src = x; sp = pxp; c = k;
        } else if (k < cx + cb) {
            src = blk; sp = pbp; c = k - cx;
        }
        if (src) {
            float a00[4], a01[4], a10[4], a11[4];
            ld4bf(src + (r0 + lx.i0) * sp + c, a00);
            ld4bf(src + (r0 + lx.i1) * sp + c, a01);
            ld4bf(src + (r1 + lx.i0) * sp + c, a10);
            ld4bf(src + (r1 + lx.i1) * sp + c, a11);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                o[r] = f2bf(ly.l0 * (lx.l0 * a00[r] + lx.l1 * a01[r]) + ly.l1 * (lx.l0 * a10[r] + lx.l1 * a11[r]));
        } else if (pred && k < cx + cb + 8) {
            float up[2];
#pragma unroll
            for (int ch = 0; ch < 2; ++ch) {
                const float* pp = pred + ((int64_t)b * 2 + ch) * h * w;
                const float v00 = pp[ly.i0 * w + lx.i0], v01 = pp[ly.i0 * w + lx.i1];
                const float v10 = pp[ly.i1 * w + lx.i0], v11 = pp[ly.i1 * w + lx.i1];
                up[ch] = ly.l0 * (lx.l0 * v00 + lx.l1 * v01) + ly.l1 * (lx.l0 * v10 + lx.l1 * v11);
            }
            uint16_t h0, m0, l0, h1, m1, l1;
            split3(up[0], h0, m0, l0);
            split3(up[1], h1, m1, l1);
            if (k == cx + cb) {
                o[0] = h0; o[1] = h1; o[2] = m0; o[3] = m1;
            } else {
                o[0] = l0; o[1] = l1;
            }
        }
        *reinterpret_cast<uint2*>(drow + (int64_t)X * cpitch + k) =
            make_uint2((uint32_t)o[0] | ((uint32_t)o[1] << 16), (uint32_t)o[2] | ((uint32_t)o[3] << 16));
    }
}

// weight of high-res coordinate D's interpolation on low-res index i
__device__ inline float lin_w(const Lin& l, int i) { return (l.i0 == i ? l.l0 : 0.0f) + (l.i1 == i ? l.l1 : 0.0f); }

template <typename I>
__global__ void k_unet_dec_in_bwd(const float* __restrict__ gup, int gpitch, int cx, int cb, int has_pred, int B, int h,
                                  int w, float* __restrict__ gx, int gxp, float* __restrict__ gb, int gbp,
                                  float* __restrict__ gpred, int assign) {
    const int H = 2 * h, W = 2 * w;
    const int Q = (cx + cb) / 4 + (has_pred ? 1 : 0);
    const I n = (I)B * h * w * Q;
    for (I e = (I)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (I)gridDim.x * blockDim.x) {
        const int k = (int)(e % (I)Q) * 4;
        const I pix = e / (I)Q;
        const I pyy = pix / (I)w;
        const int x = (int)(pix - pyy * (I)w), y = (int)(pyy % (I)h), b = (int)(pyy / (I)h);
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        for (int Y = 2 * y - 1; Y <= 2 * y + 2; ++Y) {
            if (Y < 0 || Y >= H) continue;
            const float wy = lin_w(lin2(Y, h), y);
            if (wy == 0.0f) continue;
            for (int X = 2 * x - 1; X <= 2 * x + 2; ++X) {
                if (X < 0 || X >= W) continue;
                const float wx = lin_w(lin2(X, w), x);
                if (wx == 0.0f) continue;
                const float4 g = *reinterpret_cast<const float4*>(gup + (((int64_t)b * H + Y) * W + X) * gpitch + k);
                const float ww = wy * wx;
                s[0] += ww * g.x; s[1] += ww * g.y; s[2] += ww * g.z; s[3] += ww * g.w;
            }
        }
        if (k < cx + cb) {
            const bool to_x = k < cx;
            float4* d = to_x ? reinterpret_cast<float4*>(gx + pix * gxp + k)
                             : reinterpret_cast<float4*>(gb + pix * gbp + (k - cx));
            if (assign & (to_x ? 1 : 2)) {  // first contribution: no read of a zeroed buffer
                *d = make_float4(s[0], s[1], s[2], s[3]);
            } else {
                const float4 o = *d;
                *d = make_float4(o.x + s[0], o.y + s[1], o.z + s[2], o.w + s[3]);
            }
        } else {  // pred channels: positions hi0, hi1 (mid / lo positions carry the same gradient)
            gpred[((int64_t)b * 2 + 0) * h * w + (int64_t)y * w + x] = s[0];
            gpred[((int64_t)b * 2 + 1) * h * w + (int64_t)y * w + x] = s[1];
        }
    }
}

__global__ void k_unet_pred_fwd(const uint16_t* __restrict__ x, int cpitch, int C, const float* __restrict__ wt,
                                const float* __restrict__ bias, int B, int h, int w, int up, float* __restrict__ flow,
                                float* __restrict__ flow_full) {
    const int64_t n = (int64_t)B * h * w;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const int xx = (int)(p % w), y = (int)((p / w) % h), b = (int)(p / ((int64_t)w * h));
        float s0 = 0.0f, s1 = 0.0f;
        const uint16_t* xp = x + p * cpitch;
        for (int c = 0; c < C; c += 4) {
            float v[4];
            ld4bf(xp + c, v);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s0 += v[r] * wt[c + r];
                s1 += v[r] * wt[C + c + r];
            }
        }
        const float f0 = tanhf(s0 + bias[0]), f1 = tanhf(s1 + bias[1]);
        flow[((int64_t)b * 2 + 0) * h * w + (int64_t)y * w + xx] = f0;
        flow[((int64_t)b * 2 + 1) * h * w + (int64_t)y * w + xx] = f1;
        const int Hf = h * up, Wf = w * up;
        for (int dy = 0; dy < up; ++dy)
            for (int dx = 0; dx < up; ++dx) {
                const int64_t o = (int64_t)(y * up + dy) * Wf + (xx * up + dx);
                flow_full[((int64_t)b * 2 + 0) * Hf * Wf + o] = f0;
                flow_full[((int64_t)b * 2 + 1) * Hf * Wf + o] = f1;
            }
    }
}

// g_pre[b][ch][y][x] = (1 - f^2) * (sum of g_full over the up x up block + g_extra); db sums
__global__ __launch_bounds__(256) void k_unet_pred_gpre(const float* __restrict__ flow, const float* __restrict__ g_full,
                                 const float* __restrict__ g_extra, int B, int h, int w, int up, float* __restrict__ gpre,
                                 double* acc, int C, double* partial) {
    __shared__ float sb[2][256];
    const int64_t n = (int64_t)B * h * w;
    float t0 = 0.0f, t1 = 0.0f;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const int xx = (int)(p % w), y = (int)((p / w) % h), b = (int)(p / ((int64_t)w * h));
        const int Hf = h * up, Wf = w * up;
        float gg[2];
#pragma unroll
        for (int ch = 0; ch < 2; ++ch) {
            float g = 0.0f;
            if (g_full) {
                const float* gf = g_full + ((int64_t)b * 2 + ch) * Hf * Wf;
                for (int dy = 0; dy < up; ++dy)
                    for (int dx = 0; dx < up; ++dx) g += gf[(int64_t)(y * up + dy) * Wf + (xx * up + dx)];
            }
            const int64_t lo = ((int64_t)b * 2 + ch) * h * w + (int64_t)y * w + xx;
            if (g_extra) g += g_extra[lo];
            const float f = flow[lo];
            gg[ch] = g * (1.0f - f * f);
            gpre[lo] = gg[ch];
        }
        t0 += gg[0];
        t1 += gg[1];
    }
    // db sums: a fixed-order LDS tree, then per-block partials (reduced in column order) or atomics
    const int tid = threadIdx.x;
    sb[0][tid] = t0;
    sb[1][tid] = t1;
    __syncthreads();
#pragma unroll
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            sb[0][tid] += sb[0][tid + o];
            sb[1][tid] += sb[1][tid + o];
        }
        __syncthreads();
    }
    if (tid < 2) {
        if (partial) partial[(int64_t)tid * gridDim.x + xcd_remap(blockIdx.x, (int)gridDim.x)] = (double)sb[tid][0];
        else atomicAdd(acc + 2 * C + tid, (double)sb[tid][0]);
    }
}

// g_x[pix][c] += W[0][c] g_pre0 + W[1][c] g_pre1; dW sums (2C)
__global__ __launch_bounds__(UNT) void k_unet_pred_bwd_x(const uint16_t* __restrict__ x, int cpitch, int C,
                                                         const float* __restrict__ wt, const float* __restrict__ gpre,
                                                         int B, int h, int w, float* __restrict__ gx, int gxp,
                                                         double* acc, int assign, double* partial) {
    __shared__ float red[2 * UNT * 4];  // [pixel row][2C] thread sums
    const int tid = threadIdx.x, CQ = C / 4;
    const int ppi = UNT / CQ, quad = tid % CQ, pr = tid / CQ, c0 = quad * 4;
    const int64_t n = (int64_t)B * h * w;
    float d0[4] = {0.f, 0.f, 0.f, 0.f}, d1[4] = {0.f, 0.f, 0.f, 0.f};
    if (pr < ppi) {
        float w0[4], w1[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            w0[r] = wt[c0 + r];
            w1[r] = wt[C + c0 + r];
        }
        const int hw = h * w;  // (< 2^31: checked by the host)
        for (int64_t p = (int64_t)blockIdx.x * ppi + pr; p < n; p += (int64_t)gridDim.x * ppi) {
            // 32-bit index math: image b and in-image offset (the 64-bit divisions cost ~4x)
            const uint32_t b = (uint32_t)p / (uint32_t)hw, r = (uint32_t)p - b * (uint32_t)hw;
            const float g0 = gpre[((int64_t)b * 2 + 0) * hw + r];
            const float g1 = gpre[((int64_t)b * 2 + 1) * hw + r];
            float v[4];
            ld4bf(x + p * cpitch + c0, v);
            float4* d = reinterpret_cast<float4*>(gx + p * gxp + c0);
            const float4 o = assign ? make_float4(0.f, 0.f, 0.f, 0.f) : *d;
            *d = make_float4(o.x + (w0[0] * g0 + w1[0] * g1), o.y + (w0[1] * g0 + w1[1] * g1),
                             o.z + (w0[2] * g0 + w1[2] * g1), o.w + (w0[3] * g0 + w1[3] * g1));
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                d0[r] += g0 * v[r];
                d1[r] += g1 * v[r];
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            red[pr * 2 * C + c0 + r] = d0[r];
            red[pr * 2 * C + C + c0 + r] = d1[r];
        }
    }
    __syncthreads();
    for (int i = tid; i < 2 * C; i += UNT) {  // fixed order over the block's pixel rows
        float v = 0.0f;
        for (int q = 0; q < ppi; ++q) v += red[q * 2 * C + i];
        if (partial) partial[(int64_t)i * gridDim.x + xcd_remap(blockIdx.x, (int)gridDim.x)] = (double)v;
        else atomicAdd(acc + i, (double)v);
    }
}

__global__ void k_unet_pred_param_grads(const double* acc, int C, int accumulate, float* g_w, float* g_b) {
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < 2 * C + 2; j += gridDim.x * blockDim.x) {
        const float v = (float)acc[j];
        if (j < 2 * C) g_w[j] = accumulate ? g_w[j] + v : v;
        else g_b[j - 2 * C] = accumulate ? g_b[j - 2 * C] + v : v;
    }
}

int grid1d(int64_t n, int per, int cap) {
    int64_t g = (n + per - 1) / per;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

inline int dom_pixels(const snnflow_unet_conv_args& a) {
    if (a.pclass >= 0) return a.B * ((a.Ho - (a.pclass >> 1) + 1) / 2) * ((a.Wo - (a.pclass & 1) + 1) / 2);
    return a.B * a.Ho * a.Wo;
}

template <int WMT, int WM, int XP_>
int launch_conv(const snnflow_unet_conv_args& a, hipStream_t s) {
    using G = ConvGeo<WMT, WM, XP_>;
    const int P = dom_pixels(a);
    const int ks = a.ksplit > 1 ? a.ksplit : 1;
    const int64_t nb = (int64_t)((a.M + G::BM - 1) / G::BM) * ((P + G::BN - 1) / G::BN) * ks;
    if (nb > 0x7fffffff) SNN_FAIL(SNNFLOW_E_ARG, "unet_conv: grid too large");
    if (nb == 0) return 0;
    hipLaunchKernelGGL((k_unet_conv<WMT, WM, XP_>), dim3((unsigned)nb), dim3(UNT), 0, s, a);
    if (ks > 1) {
        const int64_t n = (int64_t)P * ((a.M + 3) / 4);
        hipLaunchKernelGGL(k_unet_conv_reduce, dim3((unsigned)((n + UNT - 1) / UNT)), dim3(UNT), 0, s, a);
    }
    SNN_CHECK_LAUNCH();
    return 0;
}

#ifndef SNNFLOW_UNET_DMA
#define SNNFLOW_UNET_DMA 1     // forward convs (exact-in-bf16 inputs) through k_unet_conv_dma
#endif
#ifndef SNNFLOW_UNET_NSTAGE
#define SNNFLOW_UNET_NSTAGE 2  // LDS buffers of k_unet_conv_dma (cfg5: 2 -> 278.6 ms, 3 -> 308.2 ms: 72 KB of LDS, two blocks per CU;
                               // round 6, 3 or 4 for the M <= 64 tiles only: no change, 4 slower)
#endif
template <int WMT, int WM>
int launch_conv_dma(const snnflow_unet_conv_args& a, hipStream_t s) {
    using G = ConvGeo<WMT, WM, 1>;
    const int P = dom_pixels(a);
    const int ks = a.ksplit > 1 ? a.ksplit : 1;
    const int64_t nb = (int64_t)((a.M + G::BM - 1) / G::BM) * ((P + G::BN - 1) / G::BN) * ks;
    if (nb > 0x7fffffff) SNN_FAIL(SNNFLOW_E_ARG, "unet_conv: grid too large");
    if (nb == 0) return 0;
    // 32-bit buffer offsets (out-of-range offsets read zeros), stride-1 / stride-2 segments, taps as a
    // 32-bit mask, 32-bit W offsets; anything else runs the register-staged kernel
    if (a.pclass >= 0 || a.ksize * a.ksize > 32 || 3LL * a.ksize * a.ksize * a.kct * a.mpad * 32 >= 0x80000000LL)
        return launch_conv<WMT, WM, 1>(a, s);
    for (int k = 0; k < a.nseg; ++k)
        if ((int64_t)a.B * a.seg[k].H * a.seg[k].W * a.seg[k].cpitch * 2 >= 0x80000000LL ||
            (a.seg[k].mode != SNNFLOW_UNET_MODE_S1 && a.seg[k].mode != SNNFLOW_UNET_MODE_S2))
            return launch_conv<WMT, WM, 1>(a, s);
    hipLaunchKernelGGL((k_unet_conv_dma<WMT, WM, SNNFLOW_UNET_NSTAGE>), dim3((unsigned)nb), dim3(UNT), 0, s, a);
    if (ks > 1) {
        const int64_t n = (int64_t)P * ((a.M + 3) / 4);
        hipLaunchKernelGGL(k_unet_conv_reduce, dim3((unsigned)((n + UNT - 1) / UNT)), dim3(UNT), 0, s, a);
    }
    SNN_CHECK_LAUNCH();
    return 0;
}

#ifndef SNNFLOW_UNET_DGRAD_DMA
#define SNNFLOW_UNET_DGRAD_DMA 1  // input gradients through k_unet_dgrad_dma
#endif
// The LDS-DMA input-gradient kernels take one segment, 32-bit buffer offsets over the three planes, taps
// as a 32-bit mask, 32-bit W offsets; a transposed segment only as a parity class
inline bool dgrad_dma_ok(const snnflow_unet_conv_args& a) {
    const snnflow_unet_seg& g = a.seg[0];
    return !(a.nseg != 1 || a.ksize * a.ksize > 32 || 3LL * a.ksize * a.ksize * a.kct * a.mpad * 32 >= 0x80000000LL ||
             (2 * a.xpart + (int64_t)a.B * g.H * g.W * g.cpitch) * 2 >= 0x80000000LL ||
             (g.mode == SNNFLOW_UNET_MODE_T2) != (a.pclass >= 0) || g.mode == SNNFLOW_UNET_MODE_S2);
}

template <int WMT, int WM>
int launch_dgrad_dma(const snnflow_unet_conv_args& a, hipStream_t s) {
    using G = ConvGeo<WMT, WM, 3>;
    if (!dgrad_dma_ok(a)) return launch_conv<WMT, WM, 3>(a, s);
    const int P = dom_pixels(a);
    const int ks = a.ksplit > 1 ? a.ksplit : 1;
    const int64_t nb = (int64_t)((a.M + G::BM - 1) / G::BM) * ((P + G::BN - 1) / G::BN) * ks;
    if (nb > 0x7fffffff) SNN_FAIL(SNNFLOW_E_ARG, "unet_conv: grid too large");
    if (nb == 0) return 0;
    hipLaunchKernelGGL((k_unet_dgrad_dma<WMT, WM>), dim3((unsigned)nb), dim3(UNT), 0, s, a);
    if (ks > 1) {
        const int64_t n = (int64_t)P * ((a.M + 3) / 4);
        hipLaunchKernelGGL(k_unet_conv_reduce, dim3((unsigned)((n + UNT - 1) / UNT)), dim3(UNT), 0, s, a);
    }
    SNN_CHECK_LAUNCH();
    return 0;
}

// Input gradients with M > 64 (M = the forward conv's padded input channels): 96-row tiles where they
// pad M less than 128-row tiles (the decoders' 2 cx + 6 channels: M = 288 -> 3 x 96 instead of 3 x 128,
// 544 -> 6 x 96 instead of 5 x 128)
inline bool dgrad_bm96(int M) { return (M + 95) / 96 * 96 < (M + 127) / 128 * 128; }

// Output tiles of a launch for its tile configuration (the selection of snnflow_unet_conv).
inline void conv_tile(const snnflow_unet_conv_args& a, int& bm, int& bn) {
    if (a.xparts == 3) {
        bm = (a.M > 128 && a.M <= 160) ? 160 : (a.M > 64 ? (dgrad_bm96(a.M) ? 96 : 128) : (a.M > 32 ? 64 : 32));
        bn = a.M > 32 ? 128 : 256;
    } else if (a.M > 64) {
        bm = 128; bn = 128;
    } else if (a.M > 32) {
        bm = 64; bn = 128;
    } else if (a.M > 16) {
        bm = 32; bn = 256;
    } else {
        bm = 16; bn = 256;
    }
}

}  // namespace

extern "C" {

int snnflow_unet_conv_ksplit(const snnflow_unet_conv_args* a) {
    if (!a || a->B <= 0 || a->Ho <= 0 || a->Wo <= 0 || a->M <= 0 || a->nseg < 1 || a->nseg > SNNFLOW_UNET_MAX_SEGS ||
        a->ksize < 1)
        return 1;
    int bm, bn;
    conv_tile(*a, bm, bn);
    const int64_t tiles = (int64_t)((a->M + bm - 1) / bm) * ((dom_pixels(*a) + bn - 1) / bn);
    int taps = a->ksize * a->ksize;
    if (a->pclass >= 0) {
        const int pad = a->ksize / 2, ky0 = ((a->pclass >> 1) + pad) & 1, kx0 = ((a->pclass & 1) + pad) & 1;
        taps = ((a->ksize - ky0 + 1) / 2) * ((a->ksize - kx0 + 1) / 2);
    }
    int64_t steps = 0;
    for (int k = 0; k < a->nseg; ++k) steps += (int64_t)taps * (a->seg[k].cpitch / 32);
    // about two resident 4-wave blocks per CU (256 CUs) and at least 16 k-steps per split
    int ks = 1;
    while (ks < SNNFLOW_UNET_MAX_KSPLIT && tiles * ks < 512 && steps / (2 * ks) >= 16) ks *= 2;
    return ks;
}

int snnflow_unet_conv(const snnflow_unet_conv_args* a, void* stream) {
    if (!a || a->B <= 0 || a->Ho <= 0 || a->Wo <= 0 || a->M <= 0 || !a->w || a->nseg < 1 ||
        a->nseg > SNNFLOW_UNET_MAX_SEGS || a->ksize < 1 || (a->ksize & 1) == 0)
        SNN_FAIL(SNNFLOW_E_ARG, "unet_conv: bad args");
    if (a->mpad % 128 != 0 || a->mpad < a->M) SNN_FAIL(SNNFLOW_E_ARG, "unet_conv: mpad must cover M in multiples of 128");
    for (int s = 0; s < a->nseg; ++s) {
        const snnflow_unet_seg& g = a->seg[s];
        if (!g.x || g.cpitch <= 0 || g.cpitch % 32 != 0 || g.H <= 0 || g.W <= 0 || g.nparts < 1 || g.nparts > 3 ||
            g.mode < 0 || g.mode > 2 || g.kc0 < 0 || g.kc0 + g.cpitch / 32 > a->kct)
            SNN_FAIL(SNNFLOW_E_ARG, "unet_conv: bad segment");
        if (((uintptr_t)g.x & 15) != 0) SNN_FAIL(SNNFLOW_E_ARG, "unet_conv: segment not 16-B aligned");
    }
    if (a->epi == SNNFLOW_UNET_EPI_STORE) {
        if (!a->out || a->ld < a->M || (a->ld % 4) != 0) SNN_FAIL(SNNFLOW_E_ARG, "unet_conv: bad store output");
    } else if (a->epi == SNNFLOW_UNET_EPI_LIF) {
        if (!a->leak || !a->thresh || !a->state || !a->current || !a->act || a->M % 4 != 0 || a->act_pitch % 4 != 0 ||
            (a->residual && a->res_pitch % 4 != 0))
            SNN_FAIL(SNNFLOW_E_ARG, "unet_conv: bad LIF epilogue");
    } else {
        SNN_FAIL(SNNFLOW_E_ARG, "unet_conv: unknown epilogue");
    }
    if (a->xparts != 1 && a->xparts != 3) SNN_FAIL(SNNFLOW_E_ARG, "unet_conv: xparts must be 1 or 3");
    if (a->ksplit > 1 && (!a->partial || a->ksplit > SNNFLOW_UNET_MAX_KSPLIT))
        SNN_FAIL(SNNFLOW_E_ARG, "unet_conv: split-K needs the partial buffer (ksplit <= SNNFLOW_UNET_MAX_KSPLIT)");
    if (a->pclass >= 4 || (a->pclass >= 0 && (a->seg[0].mode != SNNFLOW_UNET_MODE_T2 || a->nseg != 1)))
        SNN_FAIL(SNNFLOW_E_ARG, "unet_conv: parity classes are for one transposed stride-2 segment");
    const hipStream_t s = (hipStream_t)stream;
    if (a->xparts == 3) {  // input gradients: the fp32 gradient as three bf16 planes
        if (SNNFLOW_UNET_DGRAD_DMA) {
            if (a->M > 128 && a->M <= 160) return launch_dgrad_dma<5, 2>(*a, s);
            if (a->M > 64 && dgrad_bm96(a->M)) return launch_dgrad_dma<3, 2>(*a, s);
            if (a->M > 64) return launch_dgrad_dma<4, 2>(*a, s);
            if (a->M > 32) return launch_dgrad_dma<2, 2>(*a, s);
            // M <= 32 keeps the register-staged kernel: its 256-pixel tiles would need 96 KB of LDS
            // and 257 VGPRs double-buffered
        }
        if (a->M > 128 && a->M <= 160) return launch_conv<5, 2, 3>(*a, s);
        if (a->M > 64 && dgrad_bm96(a->M)) return launch_conv<3, 2, 3>(*a, s);
        if (a->M > 64) return launch_conv<4, 2, 3>(*a, s);
        if (a->M > 32) return launch_conv<2, 2, 3>(*a, s);
        return launch_conv<2, 1, 3>(*a, s);
    }
    if (SNNFLOW_UNET_DMA) {  // LDS-DMA operands, NSTAGE-deep
        if (a->M > 64) return launch_conv_dma<4, 2>(*a, s);
        if (a->M > 32) return launch_conv_dma<2, 2>(*a, s);
        if (a->M > 16) return launch_conv_dma<2, 1>(*a, s);
        return launch_conv_dma<1, 1>(*a, s);
    }
    if (a->M > 64) return launch_conv<4, 2, 1>(*a, s);
    if (a->M > 32) return launch_conv<2, 2, 1>(*a, s);
    if (a->M > 16) return launch_conv<2, 1, 1>(*a, s);
    return launch_conv<1, 1, 1>(*a, s);
}

int snnflow_unet_prep_weights(const float* w, int cout, int cin, int ksize, const int* kmap, int transpose, int flip,
                              int mvalid, int kc0, int nkc, int kct, int mpad, uint16_t* dst, void* stream) {
    if (!w || !kmap || !dst || cout <= 0 || cin <= 0 || ksize <= 0 || nkc <= 0 || kc0 < 0 || kc0 + nkc > kct ||
        mpad <= 0 || mpad % 128 != 0)
        SNN_FAIL(SNNFLOW_E_ARG, "unet_prep_weights: bad args");
    if (!transpose && cout > mpad) SNN_FAIL(SNNFLOW_E_ARG, "unet_prep_weights: cout > mpad");
    if (transpose && (mvalid > mpad || nkc * 32 < cout)) SNN_FAIL(SNNFLOW_E_ARG, "unet_prep_weights: bad transpose dims");
    const int64_t n = 3LL * ksize * ksize * nkc * mpad * 32;
    hipLaunchKernelGGL(k_unet_prep_weights, dim3(grid1d(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream, w, cout, cin,
                       ksize, kmap, transpose, flip, mvalid, kc0, nkc, kct, mpad, dst);
    SNN_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"

namespace {
struct WgPlan { int ktiles, mtiles, nsplit, steps; int64_t tiles; };

// Floats of the split reduction's chunk sums behind the partial tiles (two passes above WG_RCHUNK splits).
int64_t wgrad_tmp_floats(const snnflow_unet_wgrad_args& a, int nsplit) {
    if (nsplit <= WG_RCHUNK) return 0;
    return (int64_t)((nsplit + WG_RCHUNK - 1) / WG_RCHUNK) * a.ksize * a.ksize * a.seg.cpitch * a.M;
}

// dwk += the split sums of the partial tiles ([nsplit][taps][KP][MP] at a.partial), in split order;
// above WG_RCHUNK splits through chunk sums (fixed association, so still deterministic).
void launch_wgrad_reduce(const snnflow_unet_wgrad_args& a, int nsplit, int KP, int MP, int64_t partial_floats,
                         hipStream_t s) {
    const int64_t n = (int64_t)a.ksize * a.ksize * a.seg.cpitch * a.M;
    if (nsplit <= WG_RCHUNK) {
        hipLaunchKernelGGL(k_unet_wgrad_reduce, dim3(grid1d(n, 256, 4096)), dim3(256), 0, s, a, nsplit, KP, MP);
        return;
    }
    const int nch = (nsplit + WG_RCHUNK - 1) / WG_RCHUNK;
    float* tmp = a.partial + partial_floats;
    hipLaunchKernelGGL(k_unet_wgrad_reduce_chunks, dim3(grid1d(n * nch, 256, 16384)), dim3(256), 0, s, a, nsplit, KP, MP,
                       tmp);
    snnflow_unet_wgrad_args b = a;
    b.partial = tmp;
    hipLaunchKernelGGL(k_unet_wgrad_reduce, dim3(grid1d(n, 256, 4096)), dim3(256), 0, s, b, nch, a.seg.cpitch, a.M);
}

template <int TK, int TM>
WgPlan wgrad_plan(const snnflow_unet_wgrad_args& a) {
    WgPlan p;
    const int P = a.B * a.Ho * a.Wo;
    p.ktiles = (a.seg.cpitch + TK - 1) / TK;
    p.mtiles = (a.M + TM - 1) / TM;
    p.tiles = (int64_t)a.ksize * a.ksize * p.ktiles * p.mtiles;
    const int total_steps = (P + WG_PS - 1) / WG_PS;
    p.nsplit = (int)((1024 + p.tiles - 1) / p.tiles);  // ~1024+ blocks
    if (p.nsplit > total_steps / 8) p.nsplit = total_steps / 8;  // >= 8 steps (512 pixels) per block
    if (p.nsplit < 1) p.nsplit = 1;
    p.steps = (total_steps + p.nsplit - 1) / p.nsplit;
    return p;
}

template <int TK, int TM>
int64_t wgrad_tiles_floats(const snnflow_unet_wgrad_args& a) {
    const WgPlan p = wgrad_plan<TK, TM>(a);
    return (int64_t)p.nsplit * a.ksize * a.ksize * p.ktiles * TK * p.mtiles * TM;
}

template <int TK, int TM>
int64_t wgrad_partial_floats(const snnflow_unet_wgrad_args& a) {
    return wgrad_tiles_floats<TK, TM>(a) + wgrad_tmp_floats(a, wgrad_plan<TK, TM>(a).nsplit);
}

template <int TK, int TM>
int launch_wgrad(const snnflow_unet_wgrad_args& a, hipStream_t s) {
    const WgPlan p = wgrad_plan<TK, TM>(a);
    hipLaunchKernelGGL((k_unet_wgrad<TK, TM>), dim3((unsigned)(p.tiles * p.nsplit)), dim3(UNT), 0, s, a, p.ktiles,
                       p.mtiles, p.nsplit, p.steps);
    if (a.partial) launch_wgrad_reduce(a, p.nsplit, p.ktiles * TK, p.mtiles * TM, wgrad_tiles_floats<TK, TM>(a), s);
    SNN_CHECK_LAUNCH();
    return 0;
}

// Tap-fused row-strip weight gradient (k_unet_wgrad_rows): stride-1 3x3 convs whose rows split
// into 64-pixel strips.  SNNFLOW_UNET_WROWS=0 turns it off (A/B), read once.
bool wrows_eligible(const snnflow_unet_wgrad_args& a) {
    static const int on = [] {
        const char* e = getenv("SNNFLOW_UNET_WROWS");
        return e ? atoi(e) : 1;
    }();
    if (!on || a.ksize != 3 || a.Wo < 8 || (a.Wo % 64 != 0 && 64 % a.Wo != 0)) return false;
    const int tw = a.Wo < 64 ? a.Wo : 64, r = 64 / tw;
    if (a.Ho % r != 0) return false;
    if (a.seg.mode == SNNFLOW_UNET_MODE_S1) return a.seg.H == a.Ho && a.seg.W == a.Wo;
    // stride 2 (pad 1): input (2Ho or 2Ho - 1) x ..., 32 x 64 tiles only (X staging registers)
    return a.seg.mode == SNNFLOW_UNET_MODE_S2 && a.M > 32 && (a.seg.H + 1) / 2 == a.Ho && (a.seg.W + 1) / 2 == a.Wo;
}

template <int NI, int NJ, int WK, int WM, int S>
WgPlan wrows_plan(const snnflow_unet_wgrad_args& a) {
    using G = WrGeo<NI, NJ, WK, WM, S>;
    WgPlan p;
    p.ktiles = (a.seg.cpitch + G::TK - 1) / G::TK;
    p.mtiles = (a.M + G::TM - 1) / G::TM;
    p.tiles = (int64_t)p.ktiles * p.mtiles;
    const int nstrips = a.B * a.Ho * a.Wo / 64;
    int ns = (int)((1024 + p.tiles - 1) / p.tiles);  // ~1024+ blocks, >= 8 strips each (the partial
    if (ns > nstrips / 8) ns = nstrips / 8;           // tile of a block is ~2 strips of input bytes)
    if (ns < 1) ns = 1;
    p.steps = (nstrips + ns - 1) / ns;                 // strips per block
    p.nsplit = (nstrips + p.steps - 1) / p.steps;
    return p;
}

template <int NI, int NJ, int WK, int WM, int S>
int64_t wrows_tiles_floats(const snnflow_unet_wgrad_args& a) {
    using G = WrGeo<NI, NJ, WK, WM, S>;
    const WgPlan p = wrows_plan<NI, NJ, WK, WM, S>(a);
    return (int64_t)p.nsplit * 9 * p.ktiles * G::TK * p.mtiles * G::TM;
}

template <int NI, int NJ, int WK, int WM, int S>
int64_t wrows_partial_floats(const snnflow_unet_wgrad_args& a) {
    return wrows_tiles_floats<NI, NJ, WK, WM, S>(a) + wgrad_tmp_floats(a, wrows_plan<NI, NJ, WK, WM, S>(a).nsplit);
}

template <int NI, int NJ, int WK, int WM, int S>
int launch_wrows(const snnflow_unet_wgrad_args& a, hipStream_t s) {
    using G = WrGeo<NI, NJ, WK, WM, S>;
    const WgPlan p = wrows_plan<NI, NJ, WK, WM, S>(a);
    hipLaunchKernelGGL((k_unet_wgrad_rows<NI, NJ, WK, WM, S>), dim3((unsigned)(p.tiles * p.nsplit)), dim3(UNT), 0, s, a,
                       p.ktiles, p.mtiles, p.nsplit, p.steps);
    if (a.partial)
        launch_wgrad_reduce(a, p.nsplit, p.ktiles * G::TK, p.mtiles * G::TM, wrows_tiles_floats<NI, NJ, WK, WM, S>(a), s);
    SNN_CHECK_LAUNCH();
    return 0;
}

// M <= 32: 4 waves along k (64 x 32 tile); else 2 x 2 waves (32 x 64)
#define WR_DISPATCH(FN, ARGS)                                                  \
    {                                                                          \
        if (a->seg.mode == SNNFLOW_UNET_MODE_S2) return FN<1, 2, 2, 2, 2> ARGS; \
        if (a->M <= 32) return FN<1, 2, 4, 1, 1> ARGS;                         \
        return FN<1, 2, 2, 2, 1> ARGS;                                         \
    }

// Tile of a launch: m 32 / 64 / 128; k the first of 128, 160 (m <= 64: registers), 96, 64, 32 whose
// padding of the segment's channel pitch stays within 1/5 (else the least padding) -- fewer wasted
// MFMAs and G loads on thin layers, wide tiles elsewhere.
void wgrad_tile(const snnflow_unet_wgrad_args& a, int& tk, int& tm) {
    tm = a.M <= 32 ? 32 : (a.M <= 64 ? 64 : 128);
    const int cp = a.seg.cpitch;
    int best = 1 << 30, tbest = 32;
    tk = 0;
    for (int c : {128, 160, 96, 64, 32}) {
        if (c == 160 && tm > 64) continue;
        const int padded = (cp + c - 1) / c * c;
        if (tk == 0 && 5 * (padded - cp) <= cp) tk = c;
        if (padded < best) {
            best = padded;
            tbest = c;
        }
    }
    if (tk == 0) tk = tbest;
}

#define WG_DISPATCH(FN, ARGS)                                                        \
    {                                                                               \
        int tk, tm;                                                                 \
        wgrad_tile(*a, tk, tm);                                                     \
        if (tk == 160 && tm == 32) return FN<160, 32> ARGS;                                 \
        if (tk == 160 && tm == 64) return FN<160, 64> ARGS;                                 \
        if (tk == 128 && tm == 32) return FN<128, 32> ARGS;                                 \
        if (tk == 128 && tm == 64) return FN<128, 64> ARGS;                                 \
        if (tk == 128 && tm == 128) return FN<128, 128> ARGS;                               \
        if (tk == 96 && tm == 32) return FN<96, 32> ARGS;                                   \
        if (tk == 96 && tm == 64) return FN<96, 64> ARGS;                                   \
        if (tk == 96 && tm == 128) return FN<96, 128> ARGS;                                 \
        if (tk == 64 && tm == 32) return FN<64, 32> ARGS;                                   \
        if (tk == 64 && tm == 64) return FN<64, 64> ARGS;                                   \
        if (tk == 64 && tm == 128) return FN<64, 128> ARGS;                                 \
        if (tk == 32 && tm == 32) return FN<32, 32> ARGS;                                   \
        if (tk == 32 && tm == 64) return FN<32, 64> ARGS;                                   \
        if (tk == 32 && tm == 128) return FN<32, 128> ARGS;                                 \
    }
}  // namespace

extern "C" {

int64_t snnflow_unet_wgrad_partial_floats(const snnflow_unet_wgrad_args* a) {
    if (!a || a->B <= 0 || a->Ho <= 0 || a->Wo <= 0 || a->M <= 0 || a->seg.cpitch <= 0 || a->ksize < 1) return 0;
    if (wrows_eligible(*a)) WR_DISPATCH(wrows_partial_floats, (*a))
    WG_DISPATCH(wgrad_partial_floats, (*a))
    return 0;
}

int snnflow_unet_wgrad(const snnflow_unet_wgrad_args* a, void* stream) {
    if (!a || !a->g3 || !a->dwk || !a->seg.x || a->B <= 0 || a->Ho <= 0 || a->Wo <= 0 || a->M <= 0 ||
        a->gpitch % 32 != 0 || a->seg.cpitch % 32 != 0 || a->seg.mode == SNNFLOW_UNET_MODE_T2 || a->ksize < 1)
        SNN_FAIL(SNNFLOW_E_ARG, "unet_wgrad: bad args");
    const hipStream_t s = (hipStream_t)stream;
    if (wrows_eligible(*a)) WR_DISPATCH(launch_wrows, (*a, s))
    WG_DISPATCH(launch_wgrad, (*a, s))
    SNN_FAIL(SNNFLOW_E_ARG, "unet_wgrad: no tile");
}

int snnflow_unet_wgrad_finalize(const float* dwk, int ktot, const int* kmap_inv, int k0, int nk, int cout, int cin,
                                int ksize, int accumulate, float* dw, void* stream) {
    (void)nk;
    if (!dwk || !kmap_inv || !dw || cout <= 0 || cin <= 0 || ksize <= 0) SNN_FAIL(SNNFLOW_E_ARG, "unet_wgrad_finalize: bad args");
    const int64_t n = (int64_t)cout * cin * ksize * ksize;
    hipLaunchKernelGGL(k_unet_wgrad_finalize, dim3(grid1d(n, 256, 4096)), dim3(256), 0, (hipStream_t)stream, dwk, ktot,
                       kmap_inv, k0, cout, cin, ksize * ksize, accumulate, dw);
    SNN_CHECK_LAUNCH();
    return 0;
}

// k_unet_lif_bwd's grid: at least LIF_BWD_ITERS pixel rounds per block (small deep levels: fewer,
// fuller blocks and fewer partial sums), at most 2048 blocks
constexpr int LIF_BWD_ITERS = 4;
static int lif_bwd_blocks(int64_t P, int gc_pitch) {
    const int ppi = UNT / (gc_pitch / 4);
    return grid1d((P + ppi - 1) / ppi, LIF_BWD_ITERS, 2048);
}

int snnflow_unet_lif_bwd(const snnflow_unet_lif_bwd_args* a, void* stream) {
    if (!a || a->P <= 0 || a->C <= 0 || a->C % 4 != 0 || a->C > 512 || !a->leak || !a->thresh || !a->state ||
        !a->current || !a->g_cur3 || !a->acc || a->gc_pitch % 32 != 0 || a->gc_pitch < a->C || a->gc_pitch > 1024 ||
        (a->g_out && a->g_pitch % 4 != 0) || (a->g_res && a->gres_pitch % 4 != 0) || a->surrogate < 0 ||
        a->surrogate > 3)
        SNN_FAIL(SNNFLOW_E_ARG, "unet_lif_bwd: bad args");
    const int nblk = lif_bwd_blocks(a->P, a->gc_pitch);
    hipLaunchKernelGGL(k_unet_lif_bwd, dim3(nblk), dim3(UNT), 0, (hipStream_t)stream, *a);
    if (a->partial)
        hipLaunchKernelGGL(k_unet_lif_bwd_reduce, dim3(2 * a->C), dim3(UNT), 0, (hipStream_t)stream, a->partial, nblk,
                           2 * a->C, a->acc);
    SNN_CHECK_LAUNCH();
    return 0;
}

int snnflow_unet_lif_bwd_partial_doubles(int P, int C, int gc_pitch) {
    if (P <= 0 || C <= 0 || gc_pitch < 4) return 0;
    return lif_bwd_blocks(P, gc_pitch) * 2 * C;
}

int snnflow_unet_cell_param_grads(const double* acc, const float* leak, const float* thresh, int C, int accumulate,
                                  float* g_leak, float* g_thresh, void* stream) {
    if (!acc || !leak || !thresh || !g_leak || !g_thresh || C <= 0) SNN_FAIL(SNNFLOW_E_ARG, "unet_cell_param_grads: bad args");
    hipLaunchKernelGGL(k_unet_cell_param_grads, dim3(grid1d(C, 256, 64)), dim3(256), 0, (hipStream_t)stream, acc, leak,
                       thresh, C, accumulate, g_leak, g_thresh);
    SNN_CHECK_LAUNCH();
    return 0;
}

int snnflow_unet_pack(const float* src, int B, int H, int W, int C, int64_t sb, int64_t sc, int64_t sh, int64_t sw,
                      int split, uint16_t* dst, int cpitch, void* stream) {
    if (!src || !dst || B <= 0 || H <= 0 || W <= 0 || C <= 0 || cpitch % 32 != 0 || (split ? 3 * C : C) > cpitch)
        SNN_FAIL(SNNFLOW_E_ARG, "unet_pack: bad args");
    const int64_t n = (int64_t)B * H * W * (cpitch / 8);
    if ((int64_t)B * H * W * cpitch < (1LL << 31))
        hipLaunchKernelGGL(k_unet_pack<uint32_t>, dim3(grid1d(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream, src, B, H, W,
                           C, sb, sc, sh, sw, split, dst, cpitch);
    else
        hipLaunchKernelGGL(k_unet_pack<int64_t>, dim3(grid1d(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream, src, B, H, W,
                           C, sb, sc, sh, sw, split, dst, cpitch);
    SNN_CHECK_LAUNCH();
    return 0;
}

int snnflow_unet_dec_in(const uint16_t* x, int cx, int px, const uint16_t* block, int cb, int pb, const float* pred, int B,
                        int h, int w, uint16_t* dst, int cpitch, void* stream) {
    if (!x || !block || !dst || B <= 0 || h <= 0 || w <= 0 || cx % 4 != 0 || cb % 4 != 0 || cpitch % 32 != 0 ||
        cx + cb + (pred ? 6 : 0) > cpitch || (int64_t)2 * w * (cpitch / 4) >= (1LL << 24))
        SNN_FAIL(SNNFLOW_E_ARG, "unet_dec_in: bad args");
    const int nchunk = (2 * w * (cpitch / 4) + DEC_CHUNK - 1) / DEC_CHUNK;
    const int64_t nblk = (int64_t)B * 2 * h * nchunk;
    if (nblk >= (1LL << 31)) SNN_FAIL(SNNFLOW_E_ARG, "unet_dec_in: too large");
    hipLaunchKernelGGL(k_unet_dec_in, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, x, cx, px, block, cb, pb,
                       pred, B, h, w, dst, cpitch, nchunk);
    SNN_CHECK_LAUNCH();
    return 0;
}

int snnflow_unet_dec_in_bwd(const float* g_up, int gpitch, int cx, int cb, int has_pred, int B, int h, int w, float* g_x,
                            int gx_pitch, float* g_block, int gb_pitch, float* g_pred, int assign, void* stream) {
    if (!g_up || !g_x || !g_block || (has_pred && !g_pred) || B <= 0 || h <= 0 || w <= 0 || cx % 4 != 0 ||
        cb % 4 != 0 || gpitch % 4 != 0 || gx_pitch % 4 != 0 || gb_pitch % 4 != 0)
        SNN_FAIL(SNNFLOW_E_ARG, "unet_dec_in_bwd: bad args");
    const int Q = (cx + cb) / 4 + (has_pred ? 1 : 0);
    const int64_t n = (int64_t)B * h * w * Q;
    const int64_t offs = (int64_t)B * h * w * (gx_pitch > gb_pitch ? gx_pitch : gb_pitch);
    if (n < (1LL << 30) && offs < (1LL << 31))
        hipLaunchKernelGGL(k_unet_dec_in_bwd<uint32_t>, dim3(grid1d(n, 256, 16384)), dim3(256), 0, (hipStream_t)stream, g_up,
                           gpitch, cx, cb, has_pred, B, h, w, g_x, gx_pitch, g_block, gb_pitch, g_pred, assign);
    else
        hipLaunchKernelGGL(k_unet_dec_in_bwd<int64_t>, dim3(grid1d(n, 256, 16384)), dim3(256), 0, (hipStream_t)stream, g_up,
                           gpitch, cx, cb, has_pred, B, h, w, g_x, gx_pitch, g_block, gb_pitch, g_pred, assign);
    SNN_CHECK_LAUNCH();
    return 0;
}

// grids of the prediction backward: g_pre (one pixel per thread) and the channel pass (>= 4 pixel
// rounds per block, as k_unet_lif_bwd)
static void pred_bwd_blocks(int64_t n, int C, int& ng, int& nx) {
    ng = grid1d(n, 256, 1024);
    const int ppi = UNT / (C / 4);
    nx = grid1d((n + ppi - 1) / ppi, 4, 2048);
}

int snnflow_unet_pred_fwd(const uint16_t* x, int cpitch, int C, const float* w, const float* b, int B, int h, int wd,
                          int up, float* flow, float* flow_full, void* stream) {
    if (!x || !w || !b || !flow || !flow_full || C <= 0 || C % 4 != 0 || C > cpitch || B <= 0 || h <= 0 || wd <= 0 ||
        up < 1)
        SNN_FAIL(SNNFLOW_E_ARG, "unet_pred_fwd: bad args");
    hipLaunchKernelGGL(k_unet_pred_fwd, dim3(grid1d((int64_t)B * h * wd, 256, 8192)), dim3(256), 0, (hipStream_t)stream, x,
                       cpitch, C, w, b, B, h, wd, up, flow, flow_full);
    SNN_CHECK_LAUNCH();
    return 0;
}

int snnflow_unet_pred_bwd(const uint16_t* x, int cpitch, int C, const float* w, const float* flow, const float* g_full,
                          const float* g_extra, int B, int h, int wd, int up, float* gpre, float* g_x, int gx_pitch,
                          double* acc, int assign, double* partial, void* stream) {
    if (!x || !w || !flow || !gpre || !g_x || !acc || C <= 0 || C % 4 != 0 || C > 512 || B <= 0 || h <= 0 || wd <= 0 ||
        up < 1 || gx_pitch % 4 != 0 || (int64_t)B * h * wd >= (1LL << 31))
        SNN_FAIL(SNNFLOW_E_ARG, "unet_pred_bwd: bad args");
    const hipStream_t s = (hipStream_t)stream;
    const int64_t n = (int64_t)B * h * wd;
    int ng, nx;
    pred_bwd_blocks(n, C, ng, nx);
    double* pg = partial;
    double* px = partial ? partial + 2 * ng : nullptr;
    hipLaunchKernelGGL(k_unet_pred_gpre, dim3(ng), dim3(256), 0, s, flow, g_full, g_extra, B, h, wd, up, gpre, acc, C, pg);
    hipLaunchKernelGGL(k_unet_pred_bwd_x, dim3(nx), dim3(UNT), 0, s, x, cpitch, C, w, gpre, B, h, wd, g_x, gx_pitch, acc,
                       assign, px);
    if (partial) {  // the blocks' sums added in column order (bit-reproducible parameter gradients)
        hipLaunchKernelGGL(k_unet_lif_bwd_reduce, dim3(2 * C), dim3(UNT), 0, s, px, nx, 2 * C, acc);
        hipLaunchKernelGGL(k_unet_lif_bwd_reduce, dim3(2), dim3(UNT), 0, s, pg, ng, 2, acc + 2 * C);
    }
    SNN_CHECK_LAUNCH();
    return 0;
}

int snnflow_unet_pred_bwd_partial_doubles(int B, int h, int wd, int C) {
    if (B <= 0 || h <= 0 || wd <= 0 || C <= 0 || C % 4 != 0 || C > 512) return 0;
    int ng, nx;
    pred_bwd_blocks((int64_t)B * h * wd, C, ng, nx);
    return 2 * ng + 2 * C * nx;
}

int snnflow_unet_pred_param_grads(const double* acc, int C, int accumulate, float* g_w, float* g_b, void* stream) {
    if (!acc || !g_w || !g_b || C <= 0) SNN_FAIL(SNNFLOW_E_ARG, "unet_pred_param_grads: bad args");
    hipLaunchKernelGGL(k_unet_pred_param_grads, dim3(grid1d(2 * C + 2, 256, 64)), dim3(256), 0, (hipStream_t)stream, acc,
                       C, accumulate, g_w, g_b);
    SNN_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
