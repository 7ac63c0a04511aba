// Host-side driver of one LIFFireNet time step (forward / backward) and of a BPTT window's deferred
// weight gradients: builds the kernel arguments of snnflow_conv_fwd / snnflow_lif_fwd /
// snnflow_lif_bwd / snnflow_layer_bwd / snnflow_wgrad / snnflow_slab_reduce from a per-model plan
// and per-step pointers, so that the eager drop-in loop (one model() call per window,
// train_flow.py:231-279) pays one library call per time step and direction instead of building
// about twenty argument structs in Python.  The accumulator hand-over (which kernel zeroes which
// batch-sum accumulator) is the chain order of snnflow/engine.py FireNetStep.
#include <cstring>

#include "snnflow_dev.h"
#include "snnflow_host.h"

namespace {

inline int check_plan(const snnflow_firenet_plan* p) {
    if (!p || p->L < 1 || p->L > SNNFLOW_MAX_LAYERS || p->B <= 0 || p->H <= 0 || p->W <= 0 || p->c <= 0 ||
        p->cin0 <= 0 || !p->fwd_acc || !p->bwd_acc)
        return -1;
    return 0;
}

inline const float* spike_half(const float* state, const snnflow_firenet_plan* p) {
    return state + (int64_t)p->B * p->H * p->W * p->c;
}

// One time step's tensors as the backward argument builders read them; built by the caller (the
// one-step driver from its io struct, the wavefront driver per step of its window).
struct bwd_step {
    const float* ys; const float* stats; const float* flow;   // the forward's [L] rows / flow
    const float* g_flow; int64_t gflow_sb, gflow_sc;          // dL/dflow or NULL
    float* g_cur; float* bnc;                                  // [L] rows, written
    const float* mem_in[SNNFLOW_MAX_LAYERS];                   // incoming membranes
    const float* g_state[SNNFLOW_MAX_LAYERS];                  // gradients of the step's output states
    float* g_prev[SNNFLOW_MAX_LAYERS];                         // gradients of its incoming states (or NULL)
    float* g_mem[SNNFLOW_MAX_LAYERS];                          // ... their membrane half, external states only
    int zero_mem_half[SNNFLOW_MAX_LAYERS];                     // a recurrent layer's g_prev: zero-fill that half
    double* acc[SNNFLOW_MAX_LAYERS];                           // backward batch-sum accumulators
    const snnflow_neuron_grad* ng; float* g_pred_w; float* g_pred_b;
    int accumulate;                                            // add into the neuron / pred gradients
    float* g_x; const int64_t* gxs;                            // head input gradient (optional)
    // weight gradients inside the tasks (optional): layers >= 1 into the plan's slabs (fused, reads
    // s_prev), the head's (fuse_head, reads x with strides xs); wslab_accumulate stays the caller's
    int fused, fuse_head;
    const float* s_prev[SNNFLOW_MAX_LAYERS];
    const float* x; const int64_t* xs;
};

// pred backward + LIF backward of layer L-1
void fill_top_bwd(snnflow_lif_bwd_args& b, const snnflow_firenet_plan* p, const bwd_step& v) {
    const int C = p->c, top = p->L - 1;
    const int64_t ny = (int64_t)p->B * p->H * p->W * C;
    memset(&b, 0, sizeof(b));
    b.B = p->B; b.H = p->H; b.W = p->W; b.c = C;
    b.y = v.ys + top * ny; b.mem = v.mem_in[top]; b.stats = v.stats + (int64_t)top * 2 * C; b.n = p->n[top];
    b.g_state = v.g_state[top];
    b.pred_w = p->pred_w; b.flow = v.flow;
    if (v.g_flow) {
        b.g_flow = v.g_flow; b.gflow_sb = v.gflow_sb; b.gflow_sc = v.gflow_sc;
    }
    b.g_cur = v.g_cur + top * ny; b.g_mem = v.g_mem[top];
    b.acc = v.acc[top];
}

// BN backward + dgrad of layer l's convs [+ LIF backward of layer l-1]
void fill_layer_bwd(snnflow_layer_bwd_args& a, const snnflow_firenet_plan* p, const bwd_step& v, int l) {
    const int C = p->c;
    const int64_t ny = (int64_t)p->B * p->H * p->W * C;
    memset(&a, 0, sizeof(a));
    a.B = p->B; a.H = p->H; a.W = p->W; a.c = C;
    a.y = v.ys + l * ny; a.stats = v.stats + (int64_t)l * 2 * C; a.g_cur = v.g_cur + l * ny;
    a.acc_in = v.acc[l];
    a.n = p->n[l];
    a.ng = v.ng[l];
    a.accumulate = v.accumulate;
    a.bnc_out = v.bnc + (int64_t)l * 2 * C;
    if (l == p->L - 1) {
        a.has_pred = 1; a.g_pred_w = v.g_pred_w; a.g_pred_b = v.g_pred_b;
    }
    if (p->rec[l]) {
        a.wt_bwd_rec = p->wt_bwd_rec[l]; a.wt_fwd_rec = p->wt_fwd_rec[l];
        if (v.g_prev[l]) {
            a.g_state_prev = v.g_prev[l];
            a.zero_mem_half = v.zero_mem_half[l];
        }
    }
    a.wd_ff = p->wd_ff[l]; a.wd_rec = p->wd_rec[l];
    if (l > 0) {
        a.cin = C; a.lif_in = 1;
        a.wt_bwd_ff = p->wt_bwd_ff[l]; a.wt_fwd_ff = p->wt_fwd_ff[l];
        a.prev_y = v.ys + (l - 1) * ny; a.prev_mem = v.mem_in[l - 1];
        a.prev_stats = v.stats + (int64_t)(l - 1) * 2 * C; a.prev = p->n[l - 1];
        a.prev_g_state = v.g_state[l - 1];
        a.prev_g_cur = v.g_cur + (l - 1) * ny; a.prev_g_mem = v.g_mem[l - 1];
        a.acc_out = v.acc[l - 1];
        if (v.fused) {
            a.wslab_ff = p->slab_ff[l];
            if (p->rec[l]) {
                a.wslab_rec = p->slab_rec[l];
                a.s_prev = v.s_prev[l];
            }
        }
    } else {
        a.cin = p->cin0; a.lif_in = 0;
        if (v.g_x) {
            a.wt_bwd_ff = p->wt_bwd_ff[0]; a.wt_fwd_ff = p->wt_fwd_ff[0];
            a.g_x = v.g_x;
            a.gxs_b = v.gxs[0]; a.gxs_c = v.gxs[1]; a.gxs_h = v.gxs[2]; a.gxs_w = v.gxs[3];
        }
        if (v.fuse_head) {  // ABI 40: the head's weight gradient of this step in this task
            a.x = v.x;
            a.xs_b = v.xs[0]; a.xs_c = v.xs[1]; a.xs_h = v.xs[2]; a.xs_w = v.xs[3];
            a.wslab_ff = p->slab_ff[0];
        }
    }
}

}  // namespace

extern "C" {

int snnflow_firenet_fwd(const snnflow_firenet_plan* p, const snnflow_firenet_fwd_io* io, void* stream) {
    if (check_plan(p) || !io || !io->x || !io->ys || !io->stats || !io->states || !io->flow)
        SNN_FAIL(SNNFLOW_E_ARG, "firenet_fwd: bad arguments");
    const int L = p->L, C = p->c;
    const int64_t npix = (int64_t)p->B * p->H * p->W;
    const int64_t ny = npix * C, nst = 2 * npix * C;
    const int zn = (int)p->fwd_acc_stride;
    for (int l = 0; l < L; ++l) {
        snnflow_conv_fwd_args a;
        memset(&a, 0, sizeof(a));
        a.B = p->B; a.H = p->H; a.W = p->W; a.c = C;
        if (l == 0) {
            a.cin = p->cin0; a.lif_in = 0;
            a.x = io->x;
            a.xs_b = io->xs[0]; a.xs_c = io->xs[1]; a.xs_h = io->xs[2]; a.xs_w = io->xs[3];
            a.zero0 = p->fwd_acc + (int64_t)(L - 1) * p->fwd_acc_stride;
            a.zero_n = zn;
        } else {
            a.cin = C; a.lif_in = 1;
            a.prev_y = io->ys + (l - 1) * ny;
            a.prev_mem = io->mem_in[l - 1];
            a.prev_acc = p->fwd_acc + (int64_t)(l - 1) * p->fwd_acc_stride;
            a.prev_stats = io->stats + (int64_t)(l - 1) * 2 * C;
            a.prev = p->n[l - 1];
            a.prev_state = io->states + (l - 1) * nst;
            if (l >= 2) {
                a.zero0 = p->fwd_acc + (int64_t)(l - 2) * p->fwd_acc_stride;
                a.zero_n = zn;
            }
        }
        a.wt_ff = p->wt_fwd_ff[l]; a.wt_rec = p->wt_fwd_rec[l];
        a.wt_ff_t = p->wt_bwd_ff[l]; a.wt_rec_t = p->wt_bwd_rec[l];
        a.s_prev = io->s_prev[l];
        a.y = io->ys + l * ny;
        a.acc = p->train[l] ? p->fwd_acc + (int64_t)l * p->fwd_acc_stride : nullptr;
        a.wf_ff = p->wf_ff[l]; a.wf_rec = p->wf_rec[l];
        int rc = snnflow_conv_fwd(&a, stream);
        if (rc) return rc;
    }
    snnflow_lif_fwd_args f;
    memset(&f, 0, sizeof(f));
    f.B = p->B; f.H = p->H; f.W = p->W; f.c = C;
    f.y = io->ys + (L - 1) * ny;
    f.mem = io->mem_in[L - 1];
    f.acc = p->fwd_acc + (int64_t)(L - 1) * p->fwd_acc_stride;
    f.stats = io->stats + (int64_t)(L - 1) * 2 * C;
    f.n = p->n[L - 1];
    f.state = io->states + (L - 1) * nst;
    f.pred_w = p->pred_w; f.pred_b = p->pred_b; f.flow = io->flow;
    if (L >= 2) {
        f.zero0 = p->fwd_acc + (int64_t)(L - 2) * p->fwd_acc_stride;
        f.zero_n = zn;
    }
    return snnflow_lif_fwd(&f, stream);
}

int snnflow_firenet_bwd(const snnflow_firenet_plan* p, const snnflow_firenet_bwd_io* io, void* stream) {
    if (check_plan(p) || !io || !io->ys || !io->stats || !io->flow || !io->g_cur || !io->bnc)
        SNN_FAIL(SNNFLOW_E_ARG, "firenet_bwd: bad arguments");
    const int L = p->L;
    const int zn = (int)p->bwd_acc_stride;
    bwd_step v;
    memset(&v, 0, sizeof(v));
    v.ys = io->ys; v.stats = io->stats; v.flow = io->flow;
    v.g_flow = io->g_flow; v.gflow_sb = io->gflow_sb; v.gflow_sc = io->gflow_sc;
    v.g_cur = io->g_cur; v.bnc = io->bnc;
    for (int l = 0; l < L; ++l) {
        v.mem_in[l] = io->mem_in[l]; v.g_state[l] = io->g_state[l]; v.g_prev[l] = io->g_prev[l];
        // gradients flowing into the membrane input: only for states this model did not produce
        v.g_mem[l] = (io->g_prev[l] && io->ext[l]) ? io->g_prev[l] : nullptr;
        v.zero_mem_half[l] = io->ext[l] ? 0 : 1;
        v.acc[l] = p->bwd_acc + (int64_t)l * p->bwd_acc_stride;
    }
    v.ng = io->ng; v.g_pred_w = io->g_pred_w; v.g_pred_b = io->g_pred_b; v.accumulate = io->accumulate;
    v.g_x = io->g_x; v.gxs = io->gxs;

    // the accumulator hand-over: the top kernel zeroes bwd_acc[0], layer l's kernel bwd_acc[l+1]
    snnflow_lif_bwd_args b;
    fill_top_bwd(b, p, v);
    b.zero0 = p->bwd_acc;
    b.zero_n = zn;
    int rc = snnflow_lif_bwd(&b, stream);
    if (rc) return rc;

    for (int l = L - 1; l >= 0; --l) {
        snnflow_layer_bwd_args a;
        fill_layer_bwd(a, p, v, l);
        if (l + 1 <= L - 1) {
            a.zero0 = p->bwd_acc + (int64_t)(l + 1) * p->bwd_acc_stride;
            a.zero_n = zn;
        }
        rc = snnflow_layer_bwd(&a, stream);
        if (rc) return rc;
    }
    return 0;
}

int snnflow_firenet_bwd_seq(const snnflow_firenet_plan* p, const snnflow_firenet_seq_bwd* q, int* slab_live,
                            void* stream) {
    if (check_plan(p) || !q || q->T < 1 || q->T > SNNFLOW_MAX_WINDOWS || !q->bwd_acc || !q->g_cur || !q->bnc ||
        q->acc_stride < SNNFLOW_ACC_LEN(SNNFLOW_BWD_ACC(p->c)) || !slab_live)
        SNN_FAIL(SNNFLOW_E_ARG, "firenet_bwd_seq: bad arguments");
    const int L = p->L, C = p->c, K = L + 1, T = q->T;
    if (q->fused && C != 8) SNN_FAIL(SNNFLOW_E_ARG, "firenet_bwd_seq: fused weight gradients need c = 8");
    const int64_t npix = (int64_t)p->B * p->H * p->W;
    const int64_t ny = npix * C, nst = 2 * ny;
    int rslot[SNNFLOW_MAX_LAYERS], nrec = 0;  // recurrent layer -> its g_out slot within a step
    for (int l = 0; l < L; ++l) rslot[l] = p->rec[l] ? nrec++ : -1;
    if (T > 1 && nrec && !q->g_out) SNN_FAIL(SNNFLOW_E_ARG, "firenet_bwd_seq: g_out missing");
    for (int t = 0; t < T; ++t)
        if (!q->ys[t] || !q->stats[t] || !q->flow[t] || !q->states[t] || (q->fuse_head && !q->x[t]))
            SNN_FAIL(SNNFLOW_E_ARG, "firenet_bwd_seq: incomplete step");
    if (q->fuse_head && (p->rec[0] || !(p->cin0 == 2 || p->cin0 == 4) || !p->slab_ff[0]))
        SNN_FAIL(SNNFLOW_E_ARG, "firenet_bwd_seq: fuse_head needs a feed-forward 2- or 4-channel head and its slab");
    // every launch's layer-task count, checked before the first launch (the call refuses cleanly or runs
    // to completion: no half-written gradients or slab rows)
    for (int d = 0; d < K + 2 * (T - 1); ++d) {
        int n = 0;
        for (int j = 1; j < K; ++j)
            if ((d - j) >= 0 && (d - j) % 2 == 0 && (d - j) / 2 < T) ++n;
        if (n > SNNFLOW_MAX_SLOT_TASKS) SNN_FAIL(SNNFLOW_E_ARG, "firenet_bwd_seq: too many layers for a launch");
    }
    // gradient of step t's incoming state of layer l (t >= 1: inside the chain, recurrent layers only)
    auto g_in = [&](int t, int l) -> float* {
        if (t == 0) return q->g_prev0[l];
        return rslot[l] >= 0 ? q->g_out + ((int64_t)(t - 1) * nrec + rslot[l]) * nst : nullptr;
    };
    // gradient flowing into step t's output state of layer l
    auto g_st = [&](int t, int l) -> const float* { return t == T - 1 ? q->g_state_last[l] : g_in(t + 1, l); };
    auto mem_in = [&](int t, int l) -> const float* { return t == 0 ? q->mem_in0[l] : q->states[t - 1] + l * nst; };
    auto s_prev = [&](int t, int l) -> const float* {
        return t == 0 ? q->s_prev0[l] : (p->rec[l] ? q->states[t - 1] + l * nst + ny : nullptr);
    };
    // step t's tensors as the argument builders read them
    auto step_view = [&](int t, bwd_step& v) {
        memset(&v, 0, sizeof(v));
        v.ys = q->ys[t]; v.stats = q->stats[t]; v.flow = q->flow[t];
        v.g_flow = q->g_flow[t]; v.gflow_sb = q->gflow_sb[t]; v.gflow_sc = q->gflow_sc[t];
        v.g_cur = q->g_cur + (int64_t)t * L * ny; v.bnc = q->bnc + (int64_t)t * L * 2 * C;
        for (int l = 0; l < L; ++l) {
            v.mem_in[l] = mem_in(t, l); v.g_state[l] = g_st(t, l); v.g_prev[l] = g_in(t, l);
            v.g_mem[l] = (t == 0 && q->ext0[l] && q->g_prev0[l]) ? q->g_prev0[l] : nullptr;
            // steps t >= 1: the gradient stays inside the chain and its membrane half is never
            // read (the cells detach the reset); step 0's leaves the chain zero-filled
            v.zero_mem_half[l] = (t == 0 && !q->ext0[l]) ? 1 : 0;
            v.acc[l] = q->bwd_acc + ((int64_t)t * L + l) * q->acc_stride;
            v.s_prev[l] = s_prev(t, l);
        }
        v.ng = q->ng; v.g_pred_w = q->g_pred_w; v.g_pred_b = q->g_pred_b;
        v.accumulate = (q->fresh && t == T - 1) ? 0 : 1;
        v.fused = q->fused; v.fuse_head = q->fuse_head;
        v.x = q->x[t]; v.xs = q->xs[t];
    };
    for (int d = 0; d < K + 2 * (T - 1); ++d) {
        snnflow_layer_bwd_args la[SNNFLOW_MAX_SLOT_TASKS];
        snnflow_lif_bwd_args tb;
        int nl = 0;
        bool has_top = false;
        for (int j = 0; j < K; ++j) {
            if ((d - j) % 2 || (d - j) < 0 || (d - j) / 2 >= T) continue;
            bwd_step v;
            step_view(T - 1 - (d - j) / 2, v);
            if (j == 0) {
                fill_top_bwd(tb, p, v);
                has_top = true;
                continue;
            }
            const int l = L - j;
            if (nl == SNNFLOW_MAX_SLOT_TASKS) SNN_FAIL(SNNFLOW_E_ARG, "firenet_bwd_seq: too many layers for a launch");
            snnflow_layer_bwd_args& a = la[nl++];
            fill_layer_bwd(a, p, v, l);
            if (l > 0 ? q->fused : q->fuse_head) {  // the task adds its weight gradient to the layer's slab rows
                a.wslab_accumulate = slab_live[l] ? 1 : 0;
                slab_live[l] = 1;
            }
        }
        const int rc = snnflow_bwd_slot(la, nl, has_top ? &tb : nullptr, stream);
        if (rc) return rc;
    }
    return 0;
}

int snnflow_firenet_wgrad(const snnflow_firenet_plan* p, const snnflow_firenet_wgrad_step* steps, int nsteps,
                          float* const* g_ff, float* const* g_rec, void* stream) {
    if (check_plan(p) || !steps || nsteps < 1 || !g_ff || p->nblk <= 0)
        SNN_FAIL(SNNFLOW_E_ARG, "firenet_wgrad: bad arguments");
    const int L = p->L, C = p->c;
    const int64_t npix = (int64_t)p->B * p->H * p->W;
    const int64_t ny = npix * C;
    snnflow_wgrad_args a;  // ~3 KB (32 steps)
    for (int l = 0; l < L; ++l) {
        if (!p->slab_ff[l] || (p->rec[l] && !p->slab_rec[l])) SNN_FAIL(SNNFLOW_E_ARG, "firenet_wgrad: slabs");
        for (int i0 = 0; i0 < nsteps; i0 += SNNFLOW_MAX_WGRAD_STEPS) {
            const int n = nsteps - i0 < SNNFLOW_MAX_WGRAD_STEPS ? nsteps - i0 : SNNFLOW_MAX_WGRAD_STEPS;
            memset(&a, 0, sizeof(a));
            a.B = p->B; a.H = p->H; a.W = p->W; a.c = C;
            a.cin = l == 0 ? p->cin0 : C;
            a.nsteps = n; a.accumulate = i0 ? 1 : 0; a.rec = p->rec[l];
            a.exact_inputs = l > 0 ? 1 : 0;   // layers >= 1 read this model's spikes (exact in bf16)
            a.bn_weight = p->n[l].bn_weight;
            a.slab_ff = p->slab_ff[l]; a.slab_rec = p->slab_rec[l];
            for (int k = 0; k < n; ++k) {
                const snnflow_firenet_wgrad_step& s = steps[i0 + k];
                snnflow_wgrad_step& st = a.steps[k];
                st.g_cur = s.g_cur + l * ny; st.y = s.ys + l * ny;
                st.stats = s.stats + (int64_t)l * 2 * C; st.bnc = s.bnc + (int64_t)l * 2 * C;
                if (l == 0) {
                    st.x = s.x;
                    st.xs_b = s.xs[0]; st.xs_c = s.xs[1]; st.xs_h = s.xs[2]; st.xs_w = s.xs[3];
                } else {  // spike half of the previous layer's state, NHWC
                    st.x = spike_half(s.states + (l - 1) * 2 * ny, p);
                    st.xs_b = (int64_t)p->H * p->W * C; st.xs_c = 1; st.xs_h = (int64_t)p->W * C; st.xs_w = C;
                }
                st.s_prev = p->rec[l] ? s.s_prev[l] : nullptr;
            }
            int rc = snnflow_wgrad(&a, stream);
            if (rc) return rc;
        }
    }
    snnflow_slab_desc d[SNNFLOW_MAX_SLABS];
    int nd = 0;
    for (int l = 0; l < L; ++l) {
        const int cin = l == 0 ? p->cin0 : C;
        d[nd].slab = p->slab_ff[l]; d[nd].out = g_ff[l]; d[nd].elems = C * cin * 9; ++nd;
        if (p->rec[l]) {
            d[nd].slab = p->slab_rec[l]; d[nd].out = g_rec[l]; d[nd].elems = C * C * 9; ++nd;
        }
        if (nd > SNNFLOW_MAX_SLABS - 2 || l == L - 1) {
            int rc = snnflow_slab_reduce(d, nd, p->nblk, stream);
            if (rc) return rc;
            nd = 0;
        }
    }
    return 0;
}

}  // extern "C"
