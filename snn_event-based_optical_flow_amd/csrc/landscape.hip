// Contrast-maximisation landscape for global flows on gfx950: the data term of EventWarping.forward
// (loss/flow.py:197-261) of one event window for K candidate flows that all events of a sample share
// (the brute-force heatmap of tools/demo_iwe.py:46-102 in one launch sequence).
//
// A uniform flow needs no flow map and no gather: an event moves by (tref - ts) * (v, u) * s, the same
// warp4 on the same inputs as k_iwe_splat sees for a constant map, hence the same corners and weights.
//   k_land_bin    one block per sample, candidate-independent: drops the events whose two polarity
//                 masks are 0, files the others as records (ts, y, x, pol mask 0 | pol mask 1) by
//                 (timestamp slice of 1/16, group of rg source rows), slice-major (histogram in LDS,
//                 wave-0 prefix scan, placement), and takes the range [tmin, tmax] of their timestamps.
//   k_land_splat  one block per (sample, candidate): for both directions, band by band (SB_BAND
//                 pixels, the four images in LDS in the exact fixed point of SplatLds), reads per slice
//                 only the row groups whose events can reach the band under this candidate -- an event
//                 of a slice [tlo, thi] moves by a vertical displacement between (tref - thi) v s and
//                 (tref - tlo) v s, formed with warp4's own fp32 operations, which are monotone, so the
//                 bound holds exactly; one contiguous run of records per slice, the 16 runs walked as
//                 one flat range -- splats them, reduces (ts / (cnt + 1e-9))^2 and the non-zero-pixel
//                 count over the band in a fixed order and carries the sums in fp64 across its bands;
//                 then writes out[b][k].  No global atomics, no scratch per candidate: two launches
//                 whatever K.
// The sums over a band's pixels are exact integers of the events' contributions, and everything after
// them runs in a fixed order: out[b][k] is bit-reproducible and independent of the other candidates.
#include <cmath>

#include "snnflow_dev.h"
#include "snnflow_host.h"
#include "snnflow_splat.h"
#include "snnflow_warp.h"

using namespace snnflow;

namespace {

constexpr int LB_NT = 1024, kSlices = 16, kMaxRowBins = 256, kMaxBins = kSlices * kMaxRowBins;

__host__ __device__ inline int land_row_group(int H) { return (H + kMaxRowBins - 1) / kMaxRowBins; }

// The landscape scratch, float offsets, each region 16-B aligned: the records (rec4 = (ts, y, x, pol
// mask 0), rec1 = pol mask 1) of every sample by (timestamp slice, row group), the bin table
// [B][kSlices nrb + 1] (each bin's start, slice-major; the last entry: the events kept) and the
// timestamp range [B][2].
struct LandScratch {
    int64_t rec1, rows, trange, total;
    int rg, nrb;
    __host__ __device__ LandScratch(int B, int N, int H) {
        auto up4 = [](int64_t x) { return (x + 3) / 4 * 4; };
        rg = land_row_group(H);
        nrb = (H + rg - 1) / rg;
        rec1 = 4 * (int64_t)B * N;
        rows = up4(rec1 + (int64_t)B * N);
        trange = up4(rows + (int64_t)B * (kSlices * nrb + 1));
        total = up4(trange + 2 * (int64_t)B);
    }
};

// Slice sl holds the timestamps of [sl / kSlices, (sl + 1) / kSlices) -- ts * kSlices is exact in fp32 --
// and the first and the last slice whatever lies below 0 or from 1 on (NaN: slice 0, row 0).
__device__ inline int land_bin(float ts, float y, int H, int rg, int nrb) {
    const float t = ts * (float)kSlices;
    const int sl = t >= 0.0f ? (t < (float)kSlices ? (int)t : kSlices - 1) : 0;
    const int r = y >= 0.0f ? (y < (float)H ? (int)y : H - 1) : 0;
    return sl * nrb + r / rg;
}

__global__ __launch_bounds__(LB_NT) void k_land_bin(snnflow_landscape_args a, int rg, int nrb, float4* rec4, float* rec1,
                                                    int* rows, float* trange) {
    __shared__ int cnt[kMaxBins], cur[kMaxBins];
    __shared__ float tmn[LB_NT / 64], tmx[LB_NT / 64];
    const int tid = threadIdx.x, b = blockIdx.x, lane = tid & 63, wv = tid >> 6;
    const float4* ev = reinterpret_cast<const float4*>(a.events) + (int64_t)b * a.N;
    const float2* pol = reinterpret_cast<const float2*>(a.pol) + (int64_t)b * a.N;
    const int nbin = kSlices * nrb;
    for (int j = tid; j < nbin; j += LB_NT) cnt[j] = 0;
    __syncthreads();
    float lo = INFINITY, hi = -INFINITY;
    for (int i = tid; i < a.N; i += LB_NT) {
        const float2 pm = pol[i];
        if (pm.x == 0.0f && pm.y == 0.0f) continue;
        const float4 e = ev[i];
        atomicAdd(&cnt[land_bin(e.x, e.y, a.H, rg, nrb)], 1);
        lo = fminf(lo, e.x);
        hi = fmaxf(hi, e.x);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    if (lane == 0) {
        tmn[wv] = lo;
        tmx[wv] = hi;
    }
    __syncthreads();
    int* ro = rows + (int64_t)b * (nbin + 1);
    if (tid < 64) {  // exclusive prefix over the bins, 64 at a time
        int carry = 0;
        for (int j0 = 0; j0 < nbin; j0 += 64) {
            const int j = j0 + tid;
            const int c = j < nbin ? cnt[j] : 0;
            int x = c;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int y = __shfl_up(x, o, 64);
                if (tid >= o) x += y;
            }
            if (j < nbin) {
                cur[j] = carry + x - c;
                ro[j] = carry + x - c;
            }
            carry += __shfl(x, 63, 64);
        }
        if (tid == 0) ro[nbin] = carry;
    } else if (tid == 64) {
        float l2 = tmn[0], h2 = tmx[0];
        for (int w = 1; w < LB_NT / 64; ++w) {
            l2 = fminf(l2, tmn[w]);
            h2 = fmaxf(h2, tmx[w]);
        }
        trange[2 * b] = l2;
        trange[2 * b + 1] = h2;
    }
    __syncthreads();
    // (the order inside a bin follows the LDS atomics; it does not matter: the consumer sums in
    // exact fixed point)
    for (int i = tid; i < a.N; i += LB_NT) {
        const float2 pm = pol[i];
        if (pm.x == 0.0f && pm.y == 0.0f) continue;
        const float4 e = ev[i];
        const int slot = atomicAdd(&cur[land_bin(e.x, e.y, a.H, rg, nrb)], 1);
        rec4[(int64_t)b * a.N + slot] = make_float4(e.x, e.y, e.z, pm.x);
        rec1[(int64_t)b * a.N + slot] = pm.y;
    }
}

__global__ __launch_bounds__(SPLAT_NT) void k_land_splat(snnflow_landscape_args a, int rg, int nrb, int nbands,
                                                         const float4* __restrict__ rec4, const float* __restrict__ rec1,
                                                         const int* __restrict__ rows, const float* __restrict__ trange) {
    __shared__ SplatLds img;
    __shared__ float red[SPLAT_NT / 64][3];
    __shared__ double fin[6];
    __shared__ int seg0[2][kSlices], pre[2][kSlices + 1];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int k = blockIdx.x % a.K, b = blockIdx.x / a.K;  // a sample's candidates side by side: its records in one L2
    const float u = a.cand[2 * k], v = a.cand[2 * k + 1], s = a.flow_scaling;
    const float tmin = trange[2 * b], tmax = trange[2 * b + 1];
    const int nbin = kSlices * nrb;
    const int* rb = rows + (int64_t)b * (nbin + 1);
    const int kept = min(max(rb[nbin], 0), a.N);
    const int64_t HWp = (int64_t)a.H * a.W, base = (int64_t)b * a.N;
    // lanes 0 .. kSlices - 1 of wave 0 each look after one timestamp slice: the bounds of its timestamps
    const int sl = tid < kSlices ? tid : 0;
    const float tlo = sl == 0 ? fminf(tmin, 0.0f) : (float)sl / (float)kSlices;
    const float thi = sl == kSlices - 1 ? fmaxf(tmax, 1.0f) : (float)(sl + 1) / (float)kSlices;
    double run[2] = {0.0, 0.0};  // threads 0..2: S+, S-, nz of each direction over the bands so far
    int it = 0;
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const float tref = d == 0 ? 1.0f : 0.0f;
        // the vertical displacement of any event of the slice, with warp4's operations at the two ends of
        // its timestamp range (fp32 rounding is monotone: every event's value lies between them)
        const float da = ((tref - thi) * v) * s, db = ((tref - tlo) * v) * s;
        const float dmin = fminf(da, db), dmax = fmaxf(da, db);
        const bool bounded = isfinite(da) && isfinite(db);
        // y0 = floor(wy) <= r1 and y1 = floor(wy + 1) >= r0 with wy = fl(y + d): one row each side, one
        // more for the roundings, and the spacing of floats at the displacement's magnitude
        const double slack = 2.0 + fmax(fabs((double)dmin), fabs((double)dmax)) * 0x1p-21;
        for (int band = 0; band < nbands; ++band, ++it) {
            const int p0 = band * SB_BAND;
            const int np = (int)((HWp - p0) < SB_BAND ? (HWp - p0) : SB_BAND);
            // the band's records: per slice one contiguous run of row groups; their prefix (double-buffered:
            // a band without records is left before any further barrier)
            int* const sg = seg0[it & 1];
            int* const pr = pre[it & 1];
            if (tid < 64) {
                int len = 0;
                if (tid < kSlices) {
                    int g0 = 0, g1 = nrb - 1;
                    bool any = true;
                    if (bounded) {
                        const double ylo = (double)(p0 / a.W) - slack - (double)dmax;
                        const double yhi = (double)((p0 + np - 1) / a.W) + slack - (double)dmin;
                        if (yhi < 0.0 || ylo > (double)(a.H - 1)) {
                            any = false;
                        } else {
                            g0 = (int)fmax(ylo, 0.0) / rg;
                            g1 = (int)fmin(yhi, (double)(a.H - 1)) / rg;
                        }
                    }
                    int e0 = 0;
                    if (any) {
                        e0 = min(max(rb[sl * nrb + g0], 0), kept);
                        len = min(max(rb[sl * nrb + g1 + 1], e0), kept) - e0;
                    }
                    sg[tid] = e0;
                }
                int x = len;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int y = __shfl_up(x, o, 64);
                    if (tid >= o) x += y;
                }
                if (tid < kSlices) pr[tid + 1] = x;
                if (tid == 0) pr[0] = 0;
            }
            img.zero(tid);
            __syncthreads();
            const int total = pr[kSlices];
            if (total == 0) continue;  // (block-uniform) no event reaches the band: its pixels add zeros
            for (int f = tid; f < total; f += SPLAT_NT) {
                int lo = 0, hi = kSlices - 1;  // the slice holding flat record f: last sl with pr[sl] <= f
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (pr[mid] <= f) lo = mid;
                    else hi = mid - 1;
                }
                const int64_t ri = base + sg[lo] + (f - pr[lo]);
                const float4 r0 = rec4[ri];
                const float ts = r0.x, pm0 = r0.w, pm1 = rec1[ri];
                const float tsw = d == 0 ? ts : 1.0f - ts;
                Corner c[4];
                float wy, wx;
                warp4(ts, r0.y, r0.z, v, u, tref, s, a.H, a.W, c, wy, wx);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float w = c[q].wt;
                    const int li = c[q].idx - p0;
                    if (w == 0.0f || li < 0 || li >= np) continue;
                    const float wts = w * tsw;
                    if (pm0 != 0.0f) {
                        img.add(0, li, w * pm0);
                        img.add(2, li, wts * pm0);
                    }
                    if (pm1 != 0.0f) {
                        img.add(1, li, w * pm1);
                        img.add(3, li, wts * pm1);
                    }
                }
            }
            __syncthreads();
            // the pixel's loss terms as k_iwe_loss forms them (max_ts = 1: the division by it is exact)
            float t3[3] = {0.0f, 0.0f, 0.0f};
            if (tid < np) {
                const float cp = img.get(0, tid), cn = img.get(1, tid), tp = img.get(2, tid), tn = img.get(3, tid);
                const float A = tp / (cp + 1e-9f), Bv = tn / (cn + 1e-9f);
                t3[0] = A * A;
                t3[1] = Bv * Bv;
                t3[2] = (cp + cn > 0.0f) ? 1.0f : 0.0f;
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float w = wave_total(t3[j]);
                if (lane == 0) red[wv][j] = w;
            }
            __syncthreads();  // (the next band's barriers keep red until it is read)
            if (tid < 3) {
                double t = 0.0;
#pragma unroll
                for (int w2 = 0; w2 < SPLAT_NT / 64; ++w2) t += (double)red[w2][tid];
                run[d] += t;
            }
        }
    }
    if (tid < 3) {
        fin[tid] = run[0];
        fin[3 + tid] = run[1];
    }
    __syncthreads();
    if (tid != 0) return;
    float total = 0.0f;  // k_iwe_finalize's arithmetic for one sample
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const float sp = (float)fin[3 * d], sn = (float)fin[3 * d + 1], nz = (float)fin[3 * d + 2];
        float lb = sp + sn;
        if (a.loss_scaling) lb = lb / nz;
        total += lb;
    }
    a.out[(int64_t)b * a.K + k] = total;
}

bool land_shape_ok(int B, int N, int K, int H, int W) {
    return B >= 1 && N >= 1 && K >= 1 && H >= 1 && W >= 1 && (int64_t)H * W <= ((int64_t)1 << 21) &&
           (int64_t)B * K <= 0x7fffffffLL;
}

}  // namespace

extern "C" {

int64_t snnflow_iwe_landscape_scratch_floats(int B, int N, int K, int H, int W) {
    if (!land_shape_ok(B, N, K, H, W)) return -1;
    return LandScratch(B, N, H).total;
}

int snnflow_iwe_landscape(const snnflow_landscape_args* a, void* stream) {
    if (!a) SNN_FAIL(SNNFLOW_E_ARG, "iwe_landscape: missing arguments");
    if (a->B < 1 || a->N < 1 || a->K < 1 || a->H < 1 || a->W < 1)
        SNN_FAIL(SNNFLOW_E_ARG, "iwe_landscape: bad shape (B, N, K, H, W >= 1)");
    if ((int64_t)a->H * a->W > ((int64_t)1 << 21)) SNN_FAIL(SNNFLOW_E_ARG, "iwe_landscape: H * W above 2^21 pixels");
    if ((int64_t)a->B * a->K > 0x7fffffffLL) SNN_FAIL(SNNFLOW_E_ARG, "iwe_landscape: B * K above 2^31 - 1 blocks");
    if (!a->events || !a->pol || !a->cand || !a->out || !a->scratch) SNN_FAIL(SNNFLOW_E_ARG, "iwe_landscape: missing buffer");
    if ((reinterpret_cast<uintptr_t>(a->events) & 15) != 0 || (reinterpret_cast<uintptr_t>(a->scratch) & 15) != 0 ||
        (reinterpret_cast<uintptr_t>(a->pol) & 7) != 0)
        SNN_FAIL(SNNFLOW_E_ARG, "iwe_landscape: events / scratch not 16-B aligned (pol: 8-B)");
    const LandScratch ls(a->B, a->N, a->H);
    if (a->scratch_floats < ls.total) SNN_FAIL(SNNFLOW_E_ARG, "iwe_landscape: scratch too small");
    const hipStream_t s = (hipStream_t)stream;
    float4* rec4 = reinterpret_cast<float4*>(a->scratch);
    float* rec1 = a->scratch + ls.rec1;
    int* rows = reinterpret_cast<int*>(a->scratch + ls.rows);
    float* trange = a->scratch + ls.trange;
    hipLaunchKernelGGL(k_land_bin, dim3(a->B), dim3(LB_NT), 0, s, *a, ls.rg, ls.nrb, rec4, rec1, rows, trange);
    hipLaunchKernelGGL(k_land_splat, dim3(a->B * a->K), dim3(SPLAT_NT), 0, s, *a, ls.rg, ls.nrb,
                       splat_bands((int64_t)a->H * a->W), rec4, rec1, rows, trange);
    SNN_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
