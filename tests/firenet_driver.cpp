// Stand-alone check of the host-side step driver (csrc/firenet_step.hip) without a GPU or the HIP
// runtime: this program links firenet_step.o against recording stubs of the eight functions it calls,
// drives snnflow_firenet_fwd / _bwd / _bwd_seq / _wgrad with synthetic plans whose "pointers" are
// fixed integers (nothing is dereferenced), and writes every argument struct the stubs received, in
// call order, to the log file named on the command line.  tests/test_firenet_driver_cpu.py compares
// the log byte for byte with tests/golden/firenet_driver_case.npz.
//
// Log: records of a 4-character tag, a 32-bit length and that many bytes.  "CASE" opens a driver
// call (its number), "RETC" closes it (its return code); in between come the stubs' records.  The
// driver memsets every argument struct before filling it, so the raw bytes are deterministic; the
// slab descriptors (not memset) are logged field by field.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "snnflow.h"

static std::vector<unsigned char> g_log;

static void rec(const char* tag, const void* data, size_t n) {
    const uint32_t len = (uint32_t)n;
    g_log.insert(g_log.end(), tag, tag + 4);
    const unsigned char* l = reinterpret_cast<const unsigned char*>(&len);
    g_log.insert(g_log.end(), l, l + 4);
    const unsigned char* d = static_cast<const unsigned char*>(data);
    g_log.insert(g_log.end(), d, d + n);
}

static void rec_int(const char* tag, int64_t v) { rec(tag, &v, sizeof(v)); }

// ---- the recording stubs -------------------------------------------------------------------------
int snnflow_set_error(int code, const char* msg) {  // C++ linkage, as csrc/snnflow_host.h declares it
    rec_int("ERRC", code);
    rec("ERRM", msg, strlen(msg));
    return code;
}

extern "C" {

int snnflow_conv_fwd(const snnflow_conv_fwd_args* a, void*) { rec("CONV", a, sizeof(*a)); return 0; }
int snnflow_lif_fwd(const snnflow_lif_fwd_args* a, void*) { rec("LIFF", a, sizeof(*a)); return 0; }
int snnflow_lif_bwd(const snnflow_lif_bwd_args* a, void*) { rec("LIFB", a, sizeof(*a)); return 0; }
int snnflow_layer_bwd(const snnflow_layer_bwd_args* a, void*) { rec("LAYB", a, sizeof(*a)); return 0; }

int snnflow_bwd_slot(const snnflow_layer_bwd_args* layer, int nlayer, const snnflow_lif_bwd_args* lif, void*) {
    rec_int("SLOT", nlayer);
    for (int i = 0; i < nlayer; ++i) rec("SLAY", &layer[i], sizeof(layer[i]));
    if (lif) rec("STOP", lif, sizeof(*lif));
    return 0;
}

int snnflow_wgrad(const snnflow_wgrad_args* a, void*) { rec("WGRD", a, sizeof(*a)); return 0; }

int snnflow_slab_reduce(const snnflow_slab_desc* d, int n, int nblk, void*) {
    rec_int("SLBN", n);
    rec_int("SLBB", nblk);
    for (int i = 0; i < n; ++i) {
        rec_int("SLBS", (int64_t)(uintptr_t)d[i].slab);
        rec_int("SLBO", (int64_t)(uintptr_t)d[i].out);
        rec_int("SLBE", d[i].elems);
    }
    return 0;
}

}  // extern "C"

// ---- synthetic plans -----------------------------------------------------------------------------
template <class T>
static T* fake(uint64_t id) {  // distinct, 16 MiB apart, never dereferenced
    return reinterpret_cast<T*>((uintptr_t)(0x100000000ull + id * 0x1000000ull));
}

struct Net { int L; int rec[4]; };
static const Net NETS[3] = {{4, {0, 1, 0, 1}}, {2, {0, 0, 0, 0}}, {2, {1, 1, 0, 0}}};
static const int B = 1, H = 2, W = 3;
static void* const STREAM = fake<void>(999);

static void make_plan(snnflow_firenet_plan& p, const Net& net, int c, int train) {
    memset(&p, 0, sizeof(p));
    p.L = net.L; p.B = B; p.H = H; p.W = W; p.c = c; p.cin0 = 2;
    for (int l = 0; l < net.L; ++l) {
        p.rec[l] = net.rec[l];
        p.train[l] = train;
        snnflow_neuron& n = p.n[l];
        n.bn_weight = fake<float>(100 + l); n.bn_bias = fake<float>(110 + l);
        n.running_mean = fake<float>(120 + l); n.running_var = fake<float>(130 + l);
        n.num_batches_tracked = fake<int64_t>(140 + l);
        n.beta = fake<float>(150 + l); n.threshold = fake<float>(160 + l);
        n.momentum = 0.1; n.eps = 1e-5; n.bn_train = train; n.zero_reset = l & 1;
        p.wt_fwd_ff[l] = fake<float>(200 + l); p.wt_bwd_ff[l] = fake<float>(220 + l);
        p.wd_ff[l] = fake<uint16_t>(260 + l);
        p.slab_ff[l] = fake<float>(280 + l);
        if (c >= 16) p.wf_ff[l] = fake<uint16_t>(240 + l);
        if (net.rec[l]) {
            p.wt_fwd_rec[l] = fake<float>(210 + l); p.wt_bwd_rec[l] = fake<float>(230 + l);
            p.wd_rec[l] = fake<uint16_t>(270 + l);
            p.slab_rec[l] = fake<float>(290 + l);
            if (c >= 16) p.wf_rec[l] = fake<uint16_t>(250 + l);
        }
    }
    p.fwd_acc = fake<double>(300); p.fwd_acc_stride = SNNFLOW_ACC_LEN(2 * c);
    p.bwd_acc = fake<double>(301); p.bwd_acc_stride = SNNFLOW_ACC_LEN(SNNFLOW_BWD_ACC(c));
    p.pred_w = fake<float>(302); p.pred_b = fake<float>(303);
    p.nblk = 5;
}

static snnflow_neuron_grad fake_ng(int l) {
    snnflow_neuron_grad g;
    memset(&g, 0, sizeof(g));
    g.bn_weight = fake<float>(400 + l); g.bn_bias = fake<float>(410 + l);
    g.beta = fake<float>(420 + l); g.threshold = fake<float>(430 + l);
    return g;
}

static int g_case = 0;
static std::vector<int> g_rc;

static void open_case() { rec_int("CASE", g_case++); }
static void close_case(int rc) { rec_int("RETC", rc); g_rc.push_back(rc); }

static void run_fwd(const Net& net, int train, bool with_prev) {
    snnflow_firenet_plan p;
    make_plan(p, net, 8, train);
    snnflow_firenet_fwd_io io;
    memset(&io, 0, sizeof(io));
    io.x = fake<float>(500); io.xs[0] = 2 * H * W; io.xs[1] = H * W; io.xs[2] = W; io.xs[3] = 1;
    io.ys = fake<float>(501); io.stats = fake<float>(502); io.states = fake<float>(503); io.flow = fake<float>(504);
    for (int l = 0; l < net.L; ++l) {
        if (!with_prev) continue;
        io.mem_in[l] = fake<float>(510 + l);
        if (net.rec[l]) io.s_prev[l] = fake<float>(520 + l);
    }
    open_case();
    close_case(snnflow_firenet_fwd(&p, &io, STREAM));
}

// ext: -1 none, else the one layer whose incoming state is external; g_prev: the previous states'
// gradients are wanted (recurrent and external layers)
static void run_bwd(const Net& net, int ext, bool g_prev, int accumulate, bool g_x, bool g_flow) {
    snnflow_firenet_plan p;
    make_plan(p, net, 8, 1);
    snnflow_firenet_bwd_io io;
    memset(&io, 0, sizeof(io));
    io.ys = fake<float>(600); io.stats = fake<float>(601); io.flow = fake<float>(602);
    for (int l = 0; l < net.L; ++l) {
        io.mem_in[l] = fake<float>(610 + l);
        if (l != 0) io.g_state[l] = fake<float>(620 + l);  // (layer 0's state output without a gradient)
        io.ext[l] = l == ext;
        if (g_prev && (net.rec[l] || l == ext)) io.g_prev[l] = fake<float>(630 + l);
        io.ng[l] = fake_ng(l);
    }
    if (g_flow) { io.g_flow = fake<float>(603); io.gflow_sb = 2 * H * W; io.gflow_sc = H * W; }
    io.g_cur = fake<float>(604); io.bnc = fake<float>(605);
    if (g_x) { io.g_x = fake<float>(606); io.gxs[0] = 2 * H * W; io.gxs[1] = H * W; io.gxs[2] = W; io.gxs[3] = 1; }
    io.g_pred_w = fake<float>(607); io.g_pred_b = fake<float>(608);
    io.accumulate = accumulate;
    open_case();
    close_case(snnflow_firenet_bwd(&p, &io, STREAM));
}

struct SeqOpt {
    int T, ext, fresh, fused, fuse_head, c;
    bool g_prev, g_out;
};

static void run_bwd_seq(const Net& net, const SeqOpt& o) {
    snnflow_firenet_plan p;
    make_plan(p, net, o.c, 1);
    static snnflow_firenet_seq_bwd q;  // (large: kept off the stack)
    memset(&q, 0, sizeof(q));
    q.T = o.T; q.fresh = o.fresh; q.fused = o.fused; q.fuse_head = o.fuse_head;
    for (int t = 0; t < o.T; ++t) {
        q.ys[t] = fake<float>(700 + t); q.stats[t] = fake<float>(710 + t);
        q.flow[t] = fake<float>(720 + t); q.states[t] = fake<float>(730 + t);
        if (!(o.T >= 2 && t == 1)) {  // one step without a flow gradient
            q.g_flow[t] = fake<float>(740 + t); q.gflow_sb[t] = 2 * H * W; q.gflow_sc[t] = H * W;
        }
        q.x[t] = fake<float>(750 + t);
        q.xs[t][0] = 2 * H * W + t; q.xs[t][1] = H * W; q.xs[t][2] = W; q.xs[t][3] = 1;
    }
    for (int l = 0; l < net.L; ++l) {
        q.mem_in0[l] = fake<float>(760 + l);
        if (net.rec[l]) q.s_prev0[l] = fake<float>(770 + l);
        q.ext0[l] = l == o.ext;
        if (o.g_prev && (net.rec[l] || l == o.ext)) q.g_prev0[l] = fake<float>(780 + l);
        if (l != 0) q.g_state_last[l] = fake<float>(790 + l);
        q.ng[l] = fake_ng(l);
    }
    if (o.g_out) q.g_out = fake<float>(800);
    q.g_cur = fake<float>(801); q.bnc = fake<float>(802);
    q.bwd_acc = fake<double>(803); q.acc_stride = SNNFLOW_ACC_LEN(SNNFLOW_BWD_ACC(o.c)) + 3;
    q.g_pred_w = fake<float>(804); q.g_pred_b = fake<float>(805);
    int live[SNNFLOW_MAX_LAYERS] = {0};
    if (!o.fresh)
        for (int l = 0; l < net.L; ++l) live[l] = (l & 1) ? 0 : 1;
    open_case();
    const int rc = snnflow_firenet_bwd_seq(&p, &q, live, STREAM);
    rec("LIVE", live, sizeof(live));
    close_case(rc);
}

static void run_wgrad(const Net& net, int nsteps) {
    snnflow_firenet_plan p;
    make_plan(p, net, 8, 1);
    std::vector<snnflow_firenet_wgrad_step> steps(nsteps);
    memset(steps.data(), 0, nsteps * sizeof(steps[0]));
    for (int k = 0; k < nsteps; ++k) {
        snnflow_firenet_wgrad_step& s = steps[k];
        s.g_cur = fake<float>(900 + 8 * k); s.bnc = fake<float>(901 + 8 * k); s.ys = fake<float>(902 + 8 * k);
        s.stats = fake<float>(903 + 8 * k); s.x = fake<float>(904 + 8 * k); s.states = fake<float>(905 + 8 * k);
        s.xs[0] = 2 * H * W; s.xs[1] = H * W; s.xs[2] = W; s.xs[3] = 1 + k;
        for (int l = 0; l < net.L; ++l)
            if (net.rec[l]) s.s_prev[l] = fake<float>(2000 + 8 * k + l);
    }
    float* gff[SNNFLOW_MAX_LAYERS] = {nullptr};
    float* grec[SNNFLOW_MAX_LAYERS] = {nullptr};
    for (int l = 0; l < net.L; ++l) {
        gff[l] = fake<float>(1500 + l);
        if (net.rec[l]) grec[l] = fake<float>(1510 + l);
    }
    open_case();
    close_case(snnflow_firenet_wgrad(&p, steps.data(), nsteps, gff, grec, STREAM));
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <log file>\n", argv[0]);
        return 2;
    }
    for (const Net& net : NETS) {
        for (int train = 0; train < 2; ++train)
            for (int prev = 0; prev < 2; ++prev) run_fwd(net, train, prev);
        const int hot = 1;  // the layer of the one-hot ext0
        for (int ext : {-1, hot})
            for (int gp = 0; gp < 2; ++gp) {
                for (int acc = 0; acc < 2; ++acc)
                    for (int gx = 0; gx < 2; ++gx)
                        for (int gf = 0; gf < 2; ++gf) run_bwd(net, ext, gp, acc, gx, gf);
                for (int T = 1; T <= 3; ++T)
                    for (int fresh = 0; fresh < 2; ++fresh)
                        for (int fused = 0; fused < 2; ++fused)
                            for (int fh = 0; fh < 2; ++fh)  // (a recurrent head with fuse_head: refused)
                                run_bwd_seq(net, SeqOpt{T, ext, fresh, fused, fh, 8, gp != 0, true});
            }
        for (int n : {1, 2, 3, SNNFLOW_MAX_WGRAD_STEPS + 1}) run_wgrad(net, n);
    }
    // refused calls
    run_bwd_seq(NETS[0], SeqOpt{0, -1, 1, 0, 0, 8, true, true});    // T = 0
    run_bwd_seq(NETS[2], SeqOpt{2, -1, 1, 0, 1, 8, true, true});    // fuse_head with a recurrent head
    run_bwd_seq(NETS[0], SeqOpt{2, -1, 1, 1, 0, 16, true, true});   // fused with c = 16
    run_bwd_seq(NETS[0], SeqOpt{2, -1, 1, 0, 0, 8, true, false});   // g_out missing
    run_bwd_seq(NETS[0], SeqOpt{2, -1, 1, 0, 0, 16, true, true});   // (c = 16 unfused: accepted)

    FILE* f = fopen(argv[1], "wb");
    if (!f || fwrite(g_log.data(), 1, g_log.size(), f) != g_log.size() || fclose(f)) {
        fprintf(stderr, "cannot write %s\n", argv[1]);
        return 2;
    }
    for (int rc : g_rc) printf("%d\n", rc);
    return 0;
}
