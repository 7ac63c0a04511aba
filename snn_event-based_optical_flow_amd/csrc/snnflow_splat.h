// The LDS-privatised IWE band shared by the loss forward (iwe_loss.hip k_iwe_splat) and the
// contrast-maximisation landscape (landscape.hip): the four images (cnt+, cnt-, ts+, ts-) of one band of
// SB_BAND pixels, owned by one block of SPLAT_NT threads.
// Deterministic accumulation (SNNFLOW_SPLAT_FIXED, default): every corner contribution v is split
// exactly into two 64-bit fixed-point integers, v = H 2^-32 + L 2^-75 (H = rint(v 2^32) in double,
// L = rint((v - H 2^-32) 2^75): exact for |v| >= 2^-51), and the two are added with integer LDS
// atomics.  Integer addition is associative, so the band totals -- the whole IWE -- are the same
// bits on every run whatever order the records' atomics land in, and they are the exact sums of the
// fp32 contributions (rounded once to fp32 at the end).  Two words because the loss reads ratios
// (ts image / count image, loss/flow.py:219-233) that do not shrink with the weights: a pixel hit
// only by a 1e-7 corner still contributes ts^2 to the loss, so the fraction needs relative, not
// absolute, precision.  Range: |sum| < 2^31 per pixel and image.  (0: fp32 LDS atomics,
// order-dependent rounding.)
#pragma once

#include <type_traits>

#include "snnflow_dev.h"

namespace snnflow {

#ifndef SNNFLOW_SPLAT_FIXED
#define SNNFLOW_SPLAT_FIXED 1
#endif
constexpr bool kSplatFixed = SNNFLOW_SPLAT_FIXED != 0;
constexpr int SPLAT_NT = 1024, SB_BAND = 1024, kMaxSBands = 2048;  // H W <= 2^21 pixels

struct SplatLdsF {  // fp32 images
    float v[4][SB_BAND];
    __device__ void zero(int tid) { for (int j = tid; j < 4 * SB_BAND; j += SPLAT_NT) (&v[0][0])[j] = 0.0f; }
    __device__ void add(int q, int i, float x) { atomicAdd(&v[q][i], x); }
    __device__ float get(int q, int i) const { return v[q][i]; }
};
struct SplatLdsX {  // exact two-word fixed point
    unsigned long long hi[4][SB_BAND], lo[4][SB_BAND];
    __device__ void zero(int tid) {
        for (int j = tid; j < 4 * SB_BAND; j += SPLAT_NT) (&hi[0][0])[j] = 0, (&lo[0][0])[j] = 0;
    }
    __device__ void add(int q, int i, float x) {
        // corner weights (x ts) lie in [0, 1]; the clamp keeps any input inside the fixed-point range
        // (|d| < 2^30: rint(d 2^32) fits a 64-bit word with room for 2^31 additions)
        const double d = fmin(fmax((double)x, -0x1p30), 0x1p30);
        const double h = rint(d * 0x1p32);               // exact: x has 24 significant bits
        const double r = d - h * 0x1p-32;                // exact, |r| <= 2^-33
        const long long l = (long long)rint(r * 0x1p75);
        atomicAdd(&hi[q][i], (unsigned long long)(long long)h);
        if (l != 0) atomicAdd(&lo[q][i], (unsigned long long)l);  // zero for every |x| >= 2^-9
    }
    __device__ float get(int q, int i) const {
        return (float)((double)(long long)hi[q][i] * 0x1p-32 + (double)(long long)lo[q][i] * 0x1p-75);
    }
};
typedef std::conditional_t<kSplatFixed, SplatLdsX, SplatLdsF> SplatLds;

__host__ __device__ inline int splat_bands(int64_t HWp) { return (int)((HWp + SB_BAND - 1) / SB_BAND); }

}  // namespace snnflow
