// Device and launch helpers shared by more than one of the LIFFireNet translation units
// (lif_layers.hip, wgrad.hip, train_util.hip).  What only one unit uses stays in that unit.
// A private header of those units, not of the library: internal linkage throughout, and, like
// them, written inside `using namespace snnflow`.
#pragma once

#include "snnflow_dev.h"
#include "snnflow_tile.h"

using namespace snnflow;

namespace {

// Up to 16 descriptors passed by value in the kernarg segment; blockIdx.y picks one
// through constant-index selects (a dynamic index would copy the array to scratch).
template <typename D>
struct DescBatch {
    D d[SNNFLOW_MAX_BATCH];
    __device__ inline D pick(int k) const {
        D r = d[0];
#pragma unroll
        for (int i = 1; i < SNNFLOW_MAX_BATCH; ++i)
            if (k == i) r = d[i];
        return r;
    }
};

// BatchNorm backward of one float4 of channels (torch batch_norm_cpu_backward, train):
// dx = ((g - grad_mean) - (y - mean) * k) * invstd * gamma.
struct BnBwdLds { float mean, inv, gm, k, w; };

__device__ inline float4 bn_bwd4(const float4& g, const float4& y, const BnBwdLds* bp) {
    const float gi[4] = {g.x, g.y, g.z, g.w}, yi[4] = {y.x, y.y, y.z, y.w};
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const BnBwdLds c = bp[j];
        const float dx = (yi[j] - c.mean) * c.k;
        o[j] = (((gi[j] - c.gm) - dx) * c.inv) * c.w;
    }
    return make_float4(o[0], o[1], o[2], o[3]);
}

// Accumulator set of one (conv, thread): item q (tap, co-block of 4, ci-block of VW) and
// pixel group g of the tile, summed over the steps.  Threads [TOFF, TOFF+NTH) of the block
// take part; items x groups fill them (groups reduced in fixed order by flush).
template <int CIN, int C, int NTH, int TOFF>
struct WAcc {
    static constexpr int VW = VecW<CIN>::v;
    static constexpr int Q = 9 * (C / 4) * (CIN / VW);
    static constexpr int GR0 = (Q >= NTH) ? 1 : NTH / Q;
    static constexpr int GR = GR0 > 16 ? 16 : GR0;
    static constexpr int NM = (GR > 1) ? 1 : (Q + NTH - 1) / NTH;
    static constexpr int SCRATCH = (GR > 1) ? GR * Q * 4 * VW : 1;
    float acc[NM][4][VW];
    __device__ void zero() {
#pragma unroll
        for (int m = 0; m < NM; ++m)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < VW; ++j) acc[m][i][j] = 0.f;
    }
    // Gi: interior G tile [NT][Pad<C>] (HG: the halo G tile [HN][Pad<C>] of the backward task, read at
    // the interior pixels); X: halo input tile [HN][Pad<CIN>]
    template <bool HG = false>
    __device__ void step(const float* Gi, const float* X) {
        constexpr int PC = Pad<C>::v, PX = Pad<CIN>::v;
        const int tid = (int)threadIdx.x - TOFF;
        if (tid < 0 || tid >= NTH) return;
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            const int q = (GR > 1) ? tid % Q : tid + m * NTH;
            const int g = (GR > 1) ? tid / Q : 0;
            if ((GR > 1) ? (g >= GR) : (q >= Q)) continue;
            const int kidx = q % 9, rest = q / 9, cob = rest % (C / 4), cib = rest / (C / 4);
            const int ky = kidx / 3, kx = kidx % 3;
#pragma unroll 4
            for (int p = g; p < NT; p += GR) {
                const int ty = p / TW, tx = p - ty * TW;
                const int gp = HG ? (ty + 1) * HWD + tx + 1 : p;
                const float4 gv4 = *reinterpret_cast<const float4*>(Gi + gp * PC + cob * 4);
                const float gv[4] = {gv4.x, gv4.y, gv4.z, gv4.w};
                const float* xp = X + ((ty + ky) * HWD + tx + kx) * PX + cib * VW;
                float xv[VW];
                if constexpr (VW == 4) {
                    const float4 v = *reinterpret_cast<const float4*>(xp);
                    xv[0] = v.x; xv[1] = v.y; xv[2] = v.z; xv[3] = v.w;
                } else if constexpr (VW == 2) {
                    const float2 v = *reinterpret_cast<const float2*>(xp);
                    xv[0] = v.x; xv[1] = v.y;
                } else {
                    xv[0] = xp[0];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < VW; ++j) acc[m][i][j] = fmaf(gv[i], xv[j], acc[m][i][j]);
            }
        }
    }
    // slab element of reduction item e (0 <= e < Q * 4 * VW) of the group-scratch flush
    static __device__ int slab_index(int e) {
        const int qq = e / (4 * VW), ij = e - qq * 4 * VW, i = ij / VW, j = ij - i * VW;
        const int kk = qq % 9, rest = qq / 9, cb = rest % (C / 4), ib = rest / (C / 4);
        return ((cb * 4 + i) * CIN + ib * VW + j) * 9 + kk;
    }
    static constexpr int NOLD = (Q * 4 * VW + NTH - 1) / NTH;  // reduction items per thread
    // flush (GR > 1) with the slab's old values already in registers (old[k]: item tid + k NTH),
    // loaded by the caller long before: the read-modify-write then waits on no global load
    __device__ void flush_prefetched(float* __restrict__ slab, int accumulate, float* scratch, const float (&old)[NOLD]) {
        static_assert(GR > 1, "group-scratch form");
        const int tid = (int)threadIdx.x - TOFF;
        const bool mine = tid >= 0 && tid < NTH;
        const int q = tid % Q, g = tid / Q;
        if (mine && g < GR) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < VW; ++j) scratch[((g * Q + q) * 4 + i) * VW + j] = acc[0][i][j];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NOLD; ++k) {
            const int e = tid + k * NTH;
            if (mine && e < Q * 4 * VW) {
                float sum = 0.f;
                for (int gg = 0; gg < GR; ++gg) sum += scratch[gg * Q * 4 * VW + e];
                slab[slab_index(e)] = accumulate ? old[k] + sum : sum;
            }
        }
    }
    // cross-group reduction in fixed order, then one write (or add) of the block's slab
    __device__ void flush(float* __restrict__ slab, int accumulate, float* scratch) {
        const int tid = (int)threadIdx.x - TOFF;
        const bool mine = tid >= 0 && tid < NTH;
        if constexpr (GR > 1) {
            const int q = tid % Q, g = tid / Q;
            if (mine && g < GR) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < VW; ++j) scratch[((g * Q + q) * 4 + i) * VW + j] = acc[0][i][j];
            }
            __syncthreads();
            for (int e = mine ? tid : Q * 4 * VW; e < Q * 4 * VW; e += NTH) {
                float sum = 0.f;
                for (int gg = 0; gg < GR; ++gg) sum += scratch[gg * Q * 4 * VW + e];
                const int qq = e / (4 * VW), ij = e - qq * 4 * VW, i = ij / VW, j = ij - i * VW;
                const int kk = qq % 9, rest = qq / 9, cb = rest % (C / 4), ib = rest / (C / 4);
                const int idx = ((cb * 4 + i) * CIN + ib * VW + j) * 9 + kk;
                slab[idx] = accumulate ? slab[idx] + sum : sum;
            }
            __syncthreads();
        } else {
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                const int q = tid + m * NTH;
                if (!mine || q >= Q) continue;
                const int kk = q % 9, rest = q / 9, cb = rest % (C / 4), ib = rest / (C / 4);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < VW; ++j) {
                        const int idx = ((cb * 4 + i) * CIN + ib * VW + j) * 9 + kk;
                        slab[idx] = accumulate ? slab[idx] + acc[m][i][j] : acc[m][i][j];
                    }
            }
        }
    }
};

int elem_grid(int64_t n) {
    int64_t g = (n + NT - 1) / NT;
    return (int)(g < 1 ? 1 : g);
}

}  // namespace
