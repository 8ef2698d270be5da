// api.hip -- C-ABI of libmdgen_amd.so (include/mdgen_amd.h): context, weight packing, workspace
// layout, the denoiser forward / Euler rollout orchestration and hipGraph capture.
#include "../../include/mdgen_amd.h"
#include "kernels.h"
#include "linear.h"
#include "philox.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <climits>
#include <functional>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

using namespace mdg;

// ---------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
// Plan mode (mdgen_debug_dispatch_plan): the orchestration code below runs on the host ONLY -- every HIP call (HIPCHK) and every
// launch (launch()) is skipped, and each launch's profile class is appended to g_dry->rec instead, with the sub-batch view it
// belongs to (for_each_view; -1: the call's shared preparation).  The plan is therefore the product's own dispatch logic, not a
// restatement of it.
struct DryPlan {
    int view = -1;
    std::vector<std::pair<int, const char*>> rec;
};
static thread_local DryPlan* g_dry = nullptr;
#define HIPCHK(expr)                                                                           \
    do {                                                                                       \
        if (g_dry) break;                                                                      \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) return fail((int)e_, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
#define LAUNCHCHK()                                                                            \
    do {                                                                                       \
        hipError_t e_ = hipGetLastError();                                                     \
        if (e_ != hipSuccess) return fail((int)e_, "kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), __FILE__, __LINE__); \
        if (const char* m_ = k32_take_launch_error()) return fail(-7, "internal: %s (%s:%d)", m_, __FILE__, __LINE__); \
    } while (0)

extern "C" const char* mdgen_last_error(void) { return g_err; }
extern "C" int32_t mdgen_abi_version(void) { return MDGEN_ABI_VERSION; }
// 0 for a product library; 1 when this .so was built with an experiment switch (csrc/dev.h): cycle stamps in the kernels
extern "C" int32_t mdgen_dev_build(void) {
#ifdef MDGEN_DEV_BUILD
    return 1;
#else
    return 0;
#endif
}

// ---------------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------------
constexpr int kMaxPos = 8160;        // positions covered by the rotary table / flash mask table
constexpr int kKS = 24;              // k-steps at K = 384
constexpr size_t kPackCC = (size_t)12 * kKS * 64;  // bf16x8 elements of a packed [384][384] matrix

// A parameter is addressed by its SLOT: its index in mdgen_ctx::weights = registration order = the index of mdgen_ctx_weight_name,
// of mdgen_train_bind_params' offsets and of mdgen_train_forward_backward's grad_offsets.  The structs below keep, next to the
// packed bf16 operands of the sampler, the slots of their parameters (`slot`): the fp32 path and the training step read
// mdgen_ctx::f32(slot) at the moment of use.  -1: the model has no such parameter.
struct Lin { int w = -1, b = -1; };   // a linear layer: the slots of its weight and its bias
struct MhaW {
    bf16x8 *wq = nullptr, *wk = nullptr, *wv_flash = nullptr, *wv_small = nullptr, *wo = nullptr;
    float *bq = nullptr, *bk = nullptr, *bv_flash = nullptr, *bv_small = nullptr, *bo = nullptr;
    float *bias_k = nullptr, *bias_v = nullptr;
    uint32_t* l4tab = nullptr;   // bias key / value as k_ln_qkv_attn4 reads them (launch_l4_bias_table; written by mdgen_ctx_finalize)
    struct { Lin q, k, v, o; int bias_k = -1, bias_v = -1; } slot;
};
struct FfnW {
    bf16x8 *w1 = nullptr, *w2 = nullptr;
    float *b1 = nullptr, *b2 = nullptr;
    bf16x8* wstream = nullptr;   // both matrices as ONE fragment stream in the consumption order of k_mlp_rows (mlp_stream_table)
    float* w2f = nullptr;        // trunk layers: fp32 fc2.weight [384][1536], the source of the per-step gate-folded streams (option mlp_fold)
    struct { Lin fc1, fc2; } slot;
};
struct TrunkW {
    MhaW mha_l, mha_t;
    FfnW ffn;
    Lin ada;                     // slots of the block's adaLN head
};
struct IpaW {
    float* gamma_beta = nullptr;  // [gamma(C) | beta(C)]
    bf16x8* wproj = nullptr;      // [21 ftile][24][64][8]
    float* bproj = nullptr;       // [672]
    float* head_w = nullptr;      // [4]
    bf16x8* wout = nullptr;       // [12 ftile][16][64][8]
    float* bout = nullptr;
    MhaW mha_l;
    FfnW ffn;
    struct { Lin ada, norm, q, kv, q_points, kv_points, out; int head_w = -1; } slot;
};

struct ProfRec {
    const char* cls;
    hipEvent_t a, b;
};

struct GraphEntry {
    std::vector<uint64_t> key;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
};

struct WeightSlot {
    std::string name;            // the reference's state_dict key
    std::function<int(const float*, const int64_t*, int, hipStream_t)> set;   // packs / copies the tensor into the sampler's operands
    bool provided = false;
    float* f32 = nullptr;        // fp32 copy, natural layout (option keep_fp32_weights) ...
    bool bound = false;          // ... or a pointer into the caller's flat parameter buffer (mdgen_train_bind_params)
};

struct mdgen_ctx {
    mdgen_model_desc d;
    int nl = 0, D = 0, modrow = 0;
    std::vector<void*> allocs;
    std::vector<WeightSlot> weights;
    std::map<std::string, int> slot_of;   // name -> slot, for the entry point that receives a name (mdgen_ctx_set_weight)
    struct { Lin latent, cond, t0, t2, rel_f, rel_r, fin, fin_ada; int mask = -1, aatype = -1; } slot;   // parameters outside the layers
    bool finalized = false;
    // fp32 small weights
    float *wl = nullptr, *bl = nullptr, *wc = nullptr, *bc = nullptr, *mask_emb = nullptr, *aa_emb = nullptr;
    float *wl_pack = nullptr, *wc_pack = nullptr;   // latent_to_emb / cond_to_emb in k_embed's operand order (launch_pack_embed)
    float* mask_delta = nullptr;                    // mask_to_emb[1] - mask_to_emb[0]
    // ... as bf16 pairs, K padded to 32 in kappa order (the embedding as the tail of the last layer's MLP kernel: rows_embed_tail)
    bf16x8 *wl_hi = nullptr, *wl_lo = nullptr, *wc_hi = nullptr, *wc_lo = nullptr;
    float *pos_embed = nullptr, *t_w0 = nullptr, *t_b0 = nullptr, *t_w2 = nullptr, *t_b2 = nullptr;
    float *wf7 = nullptr, *bf7 = nullptr, *wr7 = nullptr, *br7 = nullptr;
    float *ada_w = nullptr, *ada_b = nullptr;
    float *inv_freq = nullptr, *rope = nullptr;
    bf16x8* wfin = nullptr;
    bf16x8* wfin_k = nullptr;   // the same tile with the K dimension in rows.h's kappa order (k_mlp_rows<., TAIL>)
    float* bfin = nullptr;
    std::vector<TrunkW> trunk;
    std::vector<IpaW> ipa;
    // device index maps
    int *map_nat = nullptr, *map_qk = nullptr, *map_vflash = nullptr, *map_vsmall = nullptr, *map_fin = nullptr;
    int *perm_qk = nullptr, *perm_vsmall = nullptr;
    int* mlp_tab = nullptr;     // device copy of mlp_stream_table()
    std::vector<GraphEntry> graphs;
    bool inv_freq_set = false;
    bool prof_on = false;
    // run-time options (mdgen_ctx_set_option)
    int opt_precision = 16;     // GEMM / attention operand precision: 16 = bf16 MFMA path, 32 = fp32 path (k_fp32.hip)
    int opt_keep_fp32 = 0;      // keep an fp32 copy of every weight handed over (required by precision 32)
    int opt_streams = 2;        // concurrent sub-batch streams of the Euler rollout (1 = caller's stream only)
    bool opt_streams_auto = true;   // not set by the caller: the count also follows the fill of the chip (n_streams)
    int opt_attn_path = 0;      // tiled attention: 0 fixed-anchor fast loop with overflow check + fallback, 1 robust loop always
    int opt_mlp_path = 1;       // MLP block: 0 resident-panel kernel (k_mlp), 1 row-owner kernel (k_mlp_rows) when the launch
                                // fills the chip, 2 row-owner kernel always
    int opt_fuse_proj_qkv = 1;  // tiled residue axis (L > 8): its out-projection + gated residual runs inside the temporal q / k / v kernel
    int opt_fuse_proj = 3;      // the temporal attention's out-projection inside the panel MLP kernel: 0 off, 3 (default) where the launch
                                // takes the panel kernel (small N: +2 %)
    int opt_panel_waves = 0;    // 64-row panel kernels with a four- and an eight-wave form (k_mlp / k_mlp8, k_ln_qkv<false> / k_ln_qkv8): 0 (default)
                                // eight waves where a launch is at most one workgroup per CU, 4 / 8 force one form (tests, A/B runs)
    int ncu = 256;              // compute units of the device the context was created on (hipDeviceAttributeMultiprocessorCount)
    int opt_small_split = 1;    // launches far below one workgroup per CU (B = 1, the IPA stack): a panel's work over several workgroups --
                                // k_mlp8<., kMlpSplit> (hidden chunks over 3 workgroups, last arriver finishes; panels <= ncu / 3) and
                                // k_ln_qkv8<true> (q, k | v over 2 workgroups; panels <= ncu / 2).  0 off, 1 (default) on
    bool xcd_round_robin = false;   // placement probe: workgroups with equal blockIdx % 8 share an XCD (k_mlp8's split form relies on it)
    long n_split_launches = 0;  // k_mlp8<., kMlpSplit> launches enqueued (or captured) since the last mdgen_profile_report
    int opt_flash_rotate = 1;   // tiled attention: the 64-query chunks of a sequence start their walk over the key tiles at different tiles (k_flash.hip)
    int opt_flash_proj_form = 0;   // ... 0 (default): k_flash_proj8 (eight waves, 128-row panel, four query tiles per wave) for sequences of >= 512
                                   // positions whose launch gives every CU such a workgroup (cfg-2), else k_flash_proj (four waves, 64-row
                                   // panel; ATLAS); 4 / 8: one form always
    int opt_flash_proj = 1;     // tiled attention + its out-projection + gated residual in ONE launch (k_flash_proj): 0 off (k_flash, then
                                // k_proj<0> or a deferred projection), 1 (default) when the launch has >= 2 x CUs workgroups
                                // of (sequence, 64 queries), 2 always
    int opt_train_precision = 32;   // operands of the training step's linear layers / weight gradients: 32 exact fp32, 16 bf16 MFMA
    int opt_train_streams = 2;      // training step: 2 = weight / bias gradients of the linear layers on a second stream (train.inc)
    hipStream_t train_side = nullptr;   // that stream (created on first use, default priority)
    // Turned weights of the small launches' dX products (train.inc `turned`): the requests of one call in order, their images in
    // tr_buf, computed on the second stream at the start of the next call with the same requests (bf16 operands, train_streams 2)
    struct TurnReq { const float* w[3]; int nseg, rows, cols; size_t off; };
    std::vector<TurnReq> tr_plan;
    float* tr_buf = nullptr;
    size_t tr_buf_floats = 0;
    bool tr_plan_ok = false;
    std::vector<hipEvent_t> train_ev;   // event pool of that fork / join traffic (created on first use, round-robin)
    size_t train_ev_next = 0;
    double* ode_host = nullptr;     // mdgen_sample_dopri5: pinned 2 x fp64 the norms / error ratio are read back through (first use)
    int opt_mlp_fold = 1;       // sampling (t shared by the batch): the MLP gate folded into per-(step, layer) fc2 streams, k_mlp_rows starts its
                                // accumulators from the residual rows and only stores (one HBM read of the rows instead of two)
    int opt_mlp_tail = 2;       // ... and the FinalLayer + Euler update run inside the last layer's (folded) MLP kernel, which then does not store
                                // its rows: no k_final launch, 196 MB less traffic per network evaluation
    int opt_residue_l4 = 2;     // residue axis, L == 4: 0 general L <= 8 path, 1 attention fused, 2 whole sub-layer fused
    std::vector<void*> milestone_events;          // mdgen_train_set_milestone_events (hipEvent_t handles, caller-owned)
    unsigned long long* phase_trace = nullptr;   // mdgen_profile_phase_trace target (device), consumed by one launch
    long phase_trace_cap = 0;
    std::vector<ProfRec> prof;
    static constexpr int kMaxSide = 7;
    hipStream_t side[kMaxSide] = {};
    hipEvent_t ev_fork = nullptr, ev_join[kMaxSide] = {};

    const float* f32(int slot) const { return weights[slot].f32; }
    bool any_f32() const {
        return std::any_of(weights.begin(), weights.end(), [](const WeightSlot& w) { return w.f32 != nullptr; });
    }
    template <typename T>
    int dalloc(T** p, size_t count) {
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, count * sizeof(T));
        if (e != hipSuccess) return fail((int)e, "hipMalloc(%zu) failed: %s", count * sizeof(T), hipGetErrorString(e));
        allocs.push_back(q);
        *p = (T*)q;
        return 0;
    }
    int trunk_off(int i) const { return i * 9 * kC; }
    int ipa_off(int i) const { return nl * 9 * kC + i * 6 * kC; }
    int final_off() const { return nl * 15 * kC; }
};

// ---- host-side index maps (DESIGN.md "fragment layout") -------------------------------------
// Row rho (0..95) of wave-tile w of a TRANSPOSED projection -> (head, lane-half h, slot e):
//   ft = rho/32, m = rho%32 = b + 8a + 4h, a' = 4ft + a, head = 4w + a'/3, e = 4(a'%3) + b
static void decode_T(int rho, int& hd, int& h, int& e) {
    const int ft = rho / 32, m = rho % 32;
    const int b = m & 3, hh = (m >> 2) & 1, a = m >> 3;
    const int ap = 4 * ft + a;
    hd = ap / 3;
    h = hh;
    e = 4 * (ap % 3) + b;
}
// rotary-pair order for Q/K: slot e of half h is feature 6h + e/2 (+12 for odd e)
static int feat_qk(int w, int rho) {
    int hd, h, e;
    decode_T(rho, hd, h, e);
    return (4 * w + hd) * kDH + 6 * h + (e >> 1) + 12 * (e & 1);
}
// natural order for the SMALL-layout V: slot e of half h is feature 12h + e
static int feat_vsmall(int w, int rho) {
    int hd, h, e;
    decode_T(rho, hd, h, e);
    return (4 * w + hd) * kDH + 12 * h + e;
}
// FLASH-layout V (non-transposed): column col (0..95) of wave-tile w -> head 4w + col/24, V^T row
// d = col%24 carries feature psi(d) = 12*((d>>2)&1) + 4*(d>>3) + (d&3)
static int feat_vflash(int w, int col) {
    const int hd = col / kDH, d = col % kDH;
    return (4 * w + hd) * kDH + 12 * ((d >> 2) & 1) + 4 * (d >> 3) + (d & 3);
}

static void build_maps(std::vector<int>& qk, std::vector<int>& vf, std::vector<int>& vs, std::vector<int>& pqk,
                       std::vector<int>& pvs) {
    qk.assign(kC, 0); vf.assign(kC, 0); vs.assign(kC, 0); pqk.assign(kC, 0); pvs.assign(kC, 0);
    for (int w = 0; w < 4; ++w)
        for (int r = 0; r < 96; ++r) {
            qk[w * 96 + r] = feat_qk(w, r);
            vs[w * 96 + r] = feat_vsmall(w, r);
            vf[w * 96 + r] = feat_vflash(w, r);
        }
    // lane-order bias permutations: index ((w*2+h)*4+hd)*12 + e
    for (int w = 0; w < 4; ++w)
        for (int h = 0; h < 2; ++h)
            for (int hd = 0; hd < 4; ++hd)
                for (int e = 0; e < 12; ++e) {
                    const int i = ((w * 2 + h) * 4 + hd) * 12 + e;
                    pqk[i] = (4 * w + hd) * kDH + 6 * h + (e >> 1) + 12 * (e & 1);
                    pvs[i] = (4 * w + hd) * kDH + 12 * h + e;
                }
}

extern "C" int32_t mdgen_debug_layout_maps(int32_t* map_qk, int32_t* map_vflash, int32_t* map_vsmall,
                                           int32_t* perm_qk, int32_t* perm_vsmall) {
    if (!map_qk || !map_vflash || !map_vsmall || !perm_qk || !perm_vsmall) return fail(-1, "null argument");
    std::vector<int> qk, vf, vs, pqk, pvs;
    build_maps(qk, vf, vs, pqk, pvs);
    for (int i = 0; i < kC; ++i) {
        map_qk[i] = qk[i]; map_vflash[i] = vf[i]; map_vsmall[i] = vs[i]; perm_qk[i] = pqk[i]; perm_vsmall[i] = pvs[i];
    }
    return 0;
}

// Weight stream of k_mlp_rows (csrc/k_rows.hip): 2304 fragments, entry = mat << 16 | row tile << 8 | k-step with mat 0 = fc1
// (48 hidden tiles x 24 k-steps), 1 = fc2 (12 feature tiles x 96 k-steps).  Chunk c = hidden units 64 c .. 64 c + 63 =
// fc1 tiles 2c, 2c + 1 = fc2 k-steps 4c .. 4c + 3.  Order = the kernel's software pipeline:
//   [X(0)] [X(1)] { X(c+1) ks 0-5 | Y(c-1) kk 0 | X ks 6-11 | Y kk 1 | X ks 12-17 | Y kk 2 | X ks 18-23 | Y kk 3 } c = 1..22 [Y(22)] [Y(23)]
// X block: (k-step, tile) pairs, tile fastest; Y block: the 12 feature tiles of one k-step.
static std::vector<int> mlp_stream_table() {
    std::vector<int> t;
    auto xblock = [&](int c, int kx) {
        for (int q = 0; q < 12; ++q) t.push_back(0 << 16 | (2 * c + (q & 1)) << 8 | (6 * kx + (q >> 1)));
    };
    auto yblock = [&](int c, int kk) {
        for (int ft = 0; ft < 12; ++ft) t.push_back(1 << 16 | ft << 8 | (4 * c + kk));
    };
    for (int c = 0; c < 2; ++c)
        for (int kx = 0; kx < 4; ++kx) xblock(c, kx);
    for (int c = 1; c < 23; ++c)
        for (int b = 0; b < 4; ++b) {
            xblock(c + 1, b);
            yblock(c - 1, b);
        }
    for (int c = 22; c < 24; ++c)
        for (int kk = 0; kk < 4; ++kk) yblock(c, kk);
    return t;
}
constexpr int kMlpFrags = 2304;
extern "C" int32_t mdgen_debug_mlp_stream_table(int32_t* out, int32_t capacity) {
    const std::vector<int> t = mlp_stream_table();
    if (!out || capacity < (int)t.size()) return fail(-1, "need room for %d entries", (int)t.size());
    for (size_t i = 0; i < t.size(); ++i) out[i] = t[i];
    return (int32_t)t.size();
}

static int upload_ints(mdgen_ctx* c, int** dst, const std::vector<int>& v) {
    if (int r = c->dalloc(dst, v.size())) return r;
    HIPCHK(hipMemcpy(*dst, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice));
    return 0;
}

static bool shape_is(const int64_t* s, int nd, std::initializer_list<int64_t> want) {
    // accept exact shape, ignoring leading singleton dims (bias_k is (1,1,C), pos_embed (1,crop,C))
    std::vector<int64_t> a(s, s + nd), b(want);
    while (a.size() > b.size() && a.front() == 1) a.erase(a.begin());
    return a == b;
}

// registers a parameter; the value of the expression is its slot
static int add_weight(mdgen_ctx* c, const std::string& key, std::function<int(const float*, const int64_t*, int, hipStream_t)> set) {
    c->slot_of[key] = (int)c->weights.size();
    c->weights.push_back(WeightSlot{key, std::move(set)});
    return (int)c->weights.size() - 1;
}
#define SETTER(key, body)                                                                          \
    add_weight(c, key, [=](const float* data, const int64_t* shp, int nd, hipStream_t s) -> int {  \
        (void)shp; (void)nd; body; return 0; })
#define WANT(...) \
    if (!shape_is(shp, nd, {__VA_ARGS__})) return fail(-3, "unexpected shape for weight")

static int copy_f32(float* dst, const float* src, size_t n, hipStream_t s) {
    HIPCHK(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}

static int register_mha(mdgen_ctx* c, const std::string& pre, MhaW* m) {
    const float qscale = (1.0f / std::sqrt((float)kDH)) * kLog2e;
    if (int r = c->dalloc(&m->wq, kPackCC)) return r;
    if (int r = c->dalloc(&m->wk, kPackCC)) return r;
    if (int r = c->dalloc(&m->wv_flash, kPackCC)) return r;
    if (int r = c->dalloc(&m->wv_small, kPackCC)) return r;
    if (int r = c->dalloc(&m->wo, kPackCC)) return r;
    for (float** p : {&m->bq, &m->bk, &m->bv_flash, &m->bv_small, &m->bo, &m->bias_k, &m->bias_v})
        if (int r = c->dalloc(p, (size_t)kC)) return r;
    if (int r = c->dalloc(&m->l4tab, (size_t)2 * kL4Tab)) return r;
    m->slot.q.w = SETTER(pre + "q_proj.weight", {
        WANT(kC, kC);
        launch_pack_rows(data, kC, c->map_qk, 12, kKS, qscale, m->wq, s);
    });
    m->slot.q.b = SETTER(pre + "q_proj.bias", { WANT(kC); launch_gather_f32(data, c->perm_qk, qscale, m->bq, kC, s); });
    m->slot.k.w = SETTER(pre + "k_proj.weight", {
        WANT(kC, kC);
        launch_pack_rows(data, kC, c->map_qk, 12, kKS, 1.f, m->wk, s);
    });
    m->slot.k.b = SETTER(pre + "k_proj.bias", { WANT(kC); launch_gather_f32(data, c->perm_qk, 1.f, m->bk, kC, s); });
    m->slot.v.w = SETTER(pre + "v_proj.weight", {
        WANT(kC, kC);
        launch_pack_rows(data, kC, c->map_vflash, 12, kKS, 1.f, m->wv_flash, s);
        launch_pack_rows(data, kC, c->map_vsmall, 12, kKS, 1.f, m->wv_small, s);
    });
    m->slot.v.b = SETTER(pre + "v_proj.bias", {
        WANT(kC);
        launch_gather_f32(data, c->map_vflash, 1.f, m->bv_flash, kC, s);
        launch_gather_f32(data, c->perm_vsmall, 1.f, m->bv_small, kC, s);
    });
    m->slot.o.w = SETTER(pre + "out_proj.weight", {
        WANT(kC, kC);
        launch_pack_rows(data, kC, c->map_nat, 12, kKS, 1.f, m->wo, s);
    });
    m->slot.o.b = SETTER(pre + "out_proj.bias", { WANT(kC); if (int r = copy_f32(m->bo, data, kC, s)) return r; });
    m->slot.bias_k = SETTER(pre + "bias_k", { WANT(kC); if (int r = copy_f32(m->bias_k, data, kC, s)) return r; });
    m->slot.bias_v = SETTER(pre + "bias_v", { WANT(kC); if (int r = copy_f32(m->bias_v, data, kC, s)) return r; });
    SETTER(pre + "rot_emb.inv_freq", {
        WANT(12);
        if (int r = copy_f32(c->inv_freq, data, 12, s)) return r;
        c->inv_freq_set = true;
    });
    return 0;
}

static int register_ffn(mdgen_ctx* c, const std::string& pre, FfnW* f, bool trunk) {
    if (trunk)
        if (int r = c->dalloc(&f->w2f, (size_t)kC * kF)) return r;
    if (int r = c->dalloc(&f->w1, (size_t)48 * kKS * 64)) return r;
    if (int r = c->dalloc(&f->w2, (size_t)12 * 96 * 64)) return r;
    if (int r = c->dalloc(&f->b1, (size_t)kF)) return r;
    if (int r = c->dalloc(&f->b2, (size_t)kC)) return r;
    if (int r = c->dalloc(&f->wstream, (size_t)kMlpFrags * 64)) return r;
    f->slot.fc1.w = SETTER(pre + "fc1.weight", {
        WANT(kF, kC);
        launch_pack_rows(data, kC, c->map_nat, 48, kKS, 1.f, f->w1, s);
        launch_pack_stream(data, kC, 0, c->mlp_tab, kMlpFrags, 1.f, 1, f->wstream, s);
    });
    f->slot.fc1.b = SETTER(pre + "fc1.bias", { WANT(kF); if (int r = copy_f32(f->b1, data, kF, s)) return r; });
    f->slot.fc2.w = SETTER(pre + "fc2.weight", {
        WANT(kC, kF);
        launch_pack_rows(data, kF, c->map_nat, 12, 96, 1.f, f->w2, s);
        launch_pack_stream(data, kF, 1, c->mlp_tab, kMlpFrags, 1.f, 1, f->wstream, s);
        if (f->w2f)
            if (int r = copy_f32(f->w2f, data, (size_t)kC * kF, s)) return r;
    });
    f->slot.fc2.b = SETTER(pre + "fc2.bias", { WANT(kC); if (int r = copy_f32(f->b2, data, kC, s)) return r; });
    return 0;
}

extern "C" int32_t mdgen_ctx_create(mdgen_ctx** out, const mdgen_model_desc* d) {
    if (!out || !d) return fail(-1, "null argument");
    if (d->embed_dim != kC || d->mha_heads != kH) return fail(-2, "this build supports embed_dim=384, mha_heads=16 only");
    if (d->ipa_heads != 4 || d->ipa_head_dim != 32 || d->ipa_qk != 8 || d->ipa_v != 8)
        return fail(-2, "this build supports ipa_heads=4, ipa_head_dim=32, ipa_qk=ipa_v=8 only");
    if (d->num_layers < 1 || d->num_layers > 8) return fail(-2, "num_layers must be in 1..8");
    if (d->latent_dim != 21 && d->latent_dim != 28)   // wrapper.py:57-60: 21, or 28 with two-sided conditioning
        return fail(-2, "latent_dim must be 21 (forward simulation) or 28 (two-sided conditioning)");
    if (d->tps_condition && d->latent_dim != 28) return fail(-2, "tps_condition requires latent_dim 28");
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (ndev < 1) return fail(-9, "no HIP device");
    mdgen_ctx* c = new mdgen_ctx();
    {   // "one workgroup per CU" thresholds (eight-wave panel kernels, stream count) follow the device, not a constant
        int dev = 0, ncu = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && ncu > 0)
            c->ncu = ncu;
    }
    {   // placement probe for k_mlp8's split form: do workgroups with the same blockIdx % 8 run on the same XCD?
        // (a performance hint since round 6: the hand-over is a release / acquire pair at agent scope.)  Private non-blocking stream,
        // no legacy-stream launch; any error is consumed here and reads as "rule does not hold".
        int* dp = nullptr;
        int hx[64];
        hipStream_t ps = nullptr;
        if (hipStreamCreateWithFlags(&ps, hipStreamNonBlocking) == hipSuccess) {
            if (hipMalloc((void**)&dp, sizeof(hx)) == hipSuccess) {
                launch_xcc_probe(dp, 64, ps);
                if (hipGetLastError() == hipSuccess &&
                    hipMemcpyAsync(hx, dp, sizeof(hx), hipMemcpyDeviceToHost, ps) == hipSuccess &&
                    hipStreamSynchronize(ps) == hipSuccess) {
                    bool ok = true;
                    for (int i = 8; i < 64; ++i) ok = ok && hx[i] == hx[i & 7];
                    c->xcd_round_robin = ok;
                }
                (void)hipFree(dp);
            }
            (void)hipStreamDestroy(ps);
        }
        (void)hipGetLastError();   // nothing sticky is left for the next LAUNCHCHK
    }
    c->d = *d;
    c->nl = d->num_layers;
    c->D = d->latent_dim;
    c->modrow = (15 * c->nl + 2) * kC;
    const int D = c->D, nl = c->nl;
    // index maps
    std::vector<int> nat(kF), qk, vf, vs, fin(32), pqk, pvs;
    for (int i = 0; i < kF; ++i) nat[i] = i;
    build_maps(qk, vf, vs, pqk, pvs);
    for (int i = 0; i < 32; ++i) fin[i] = i < D ? i : -1;
#define TRY(x) do { if (int r_ = (x)) { mdgen_ctx_destroy(c); return r_; } } while (0)
    TRY(upload_ints(c, &c->map_nat, nat));
    TRY(upload_ints(c, &c->map_qk, qk));
    TRY(upload_ints(c, &c->map_vflash, vf));
    TRY(upload_ints(c, &c->map_vsmall, vs));
    TRY(upload_ints(c, &c->map_fin, fin));
    TRY(upload_ints(c, &c->mlp_tab, mlp_stream_table()));
    TRY(upload_ints(c, &c->perm_qk, pqk));
    TRY(upload_ints(c, &c->perm_vsmall, pvs));
    TRY(c->dalloc(&c->wl, (size_t)kC * D));
    TRY(c->dalloc(&c->wl_pack, (size_t)kEmbPackFloats));
    TRY(c->dalloc(&c->wc_pack, (size_t)kEmbPackFloats));
    TRY(c->dalloc(&c->mask_delta, (size_t)kC));
    for (bf16x8** q : {&c->wl_hi, &c->wl_lo, &c->wc_hi, &c->wc_lo}) TRY(c->dalloc(q, (size_t)12 * 2 * 64));
    TRY(c->dalloc(&c->bl, (size_t)kC));
    TRY(c->dalloc(&c->wc, (size_t)kC * D));
    TRY(c->dalloc(&c->bc, (size_t)kC));
    TRY(c->dalloc(&c->mask_emb, (size_t)2 * kC));
    TRY(c->dalloc(&c->aa_emb, (size_t)21 * kC));
    TRY(c->dalloc(&c->t_w0, (size_t)kC * 256));
    TRY(c->dalloc(&c->t_b0, (size_t)kC));
    TRY(c->dalloc(&c->t_w2, (size_t)kC * kC));
    TRY(c->dalloc(&c->t_b2, (size_t)kC));
    TRY(c->dalloc(&c->ada_w, (size_t)c->modrow * kC));
    TRY(c->dalloc(&c->ada_b, (size_t)c->modrow));
    TRY(c->dalloc(&c->inv_freq, (size_t)12));
    TRY(c->dalloc(&c->rope, (size_t)(kMaxPos + 1) * kRopeRow));
    // a failing HIP call must not leak the half-built context
#define TRYHIP(expr)                                                                                    \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) {                                                                         \
            mdgen_ctx_destroy(c);                                                                       \
            return fail((int)e_, "%s failed: %s", #expr, hipGetErrorString(e_));                        \
        }                                                                                               \
    } while (0)
    for (int i = 0; i < mdgen_ctx::kMaxSide; ++i) {
        TRYHIP(hipStreamCreateWithFlags(&c->side[i], hipStreamNonBlocking));
        TRYHIP(hipEventCreateWithFlags(&c->ev_join[i], hipEventDisableTiming));
    }
    TRYHIP(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    TRY(c->dalloc(&c->wfin, (size_t)kKS * 64));
    TRY(c->dalloc(&c->wfin_k, (size_t)kKS * 64));
    TRY(c->dalloc(&c->bfin, (size_t)32));
    TRYHIP(hipMemset(c->bfin, 0, 32 * sizeof(float)));
#undef TRYHIP
    c->slot.latent.w = SETTER("latent_to_emb.weight", { WANT(kC, c->D); if (int r = copy_f32(c->wl, data, (size_t)kC * c->D, s)) return r; launch_pack_embed(c->wl, c->D, c->wl_pack, s);
        launch_pack_rows(c->wl, c->D, c->map_nat, 12, 2, 1.f, c->wl_hi, s, 1, 0); launch_pack_rows(c->wl, c->D, c->map_nat, 12, 2, 1.f, c->wl_lo, s, 1, 1); });
    c->slot.latent.b = SETTER("latent_to_emb.bias", { WANT(kC); if (int r = copy_f32(c->bl, data, kC, s)) return r; });
    c->slot.cond.w = SETTER("cond_to_emb.weight", { WANT(kC, c->D); if (int r = copy_f32(c->wc, data, (size_t)kC * c->D, s)) return r; launch_pack_embed(c->wc, c->D, c->wc_pack, s);
        launch_pack_rows(c->wc, c->D, c->map_nat, 12, 2, 1.f, c->wc_hi, s, 1, 0); launch_pack_rows(c->wc, c->D, c->map_nat, 12, 2, 1.f, c->wc_lo, s, 1, 1); });
    c->slot.cond.b = SETTER("cond_to_emb.bias", { WANT(kC); if (int r = copy_f32(c->bc, data, kC, s)) return r; });
    c->slot.mask = SETTER("mask_to_emb.weight", { WANT(2, kC); if (int r = copy_f32(c->mask_emb, data, 2 * kC, s)) return r; launch_sub_f32(c->mask_emb + kC, c->mask_emb, c->mask_delta, kC, s); });
    c->slot.aatype = SETTER("aatype_to_emb.weight", { WANT(21, kC); if (int r = copy_f32(c->aa_emb, data, 21 * kC, s)) return r; });
    c->slot.t0.w = SETTER("t_embedder.mlp.0.weight", { WANT(kC, 256); if (int r = copy_f32(c->t_w0, data, (size_t)kC * 256, s)) return r; });
    c->slot.t0.b = SETTER("t_embedder.mlp.0.bias", { WANT(kC); if (int r = copy_f32(c->t_b0, data, kC, s)) return r; });
    c->slot.t2.w = SETTER("t_embedder.mlp.2.weight", { WANT(kC, kC); if (int r = copy_f32(c->t_w2, data, (size_t)kC * kC, s)) return r; });
    c->slot.t2.b = SETTER("t_embedder.mlp.2.bias", { WANT(kC); if (int r = copy_f32(c->t_b2, data, kC, s)) return r; });
    if (d->abs_pos_emb) {
        if (d->crop < 1) { mdgen_ctx_destroy(c); return fail(-2, "abs_pos_emb requires crop >= 1"); }
        TRY(c->dalloc(&c->pos_embed, (size_t)d->crop * kC));
        SETTER("pos_embed", { WANT(c->d.crop, kC); if (int r = copy_f32(c->pos_embed, data, (size_t)c->d.crop * kC, s)) return r; });
    }
    if (d->tps_condition) {
        TRY(c->dalloc(&c->wf7, (size_t)kC * 7));
        TRY(c->dalloc(&c->bf7, (size_t)kC));
        TRY(c->dalloc(&c->wr7, (size_t)kC * 7));
        TRY(c->dalloc(&c->br7, (size_t)kC));
        c->slot.rel_f.w = SETTER("latent_to_emb_f.weight", { WANT(kC, 7); if (int r = copy_f32(c->wf7, data, kC * 7, s)) return r; });
        c->slot.rel_f.b = SETTER("latent_to_emb_f.bias", { WANT(kC); if (int r = copy_f32(c->bf7, data, kC, s)) return r; });
        c->slot.rel_r.w = SETTER("latent_to_emb_r.weight", { WANT(kC, 7); if (int r = copy_f32(c->wr7, data, kC * 7, s)) return r; });
        c->slot.rel_r.b = SETTER("latent_to_emb_r.bias", { WANT(kC); if (int r = copy_f32(c->br7, data, kC, s)) return r; });
    }
    c->slot.fin.w = SETTER("emb_to_latent.linear.weight",
           { WANT(c->D, kC); launch_pack_rows(data, kC, c->map_fin, 1, kKS, 1.f, c->wfin, s); launch_pack_rows(data, kC, c->map_fin, 1, kKS, 1.f, c->wfin_k, s, 1); });
    c->slot.fin.b = SETTER("emb_to_latent.linear.bias", { WANT(c->D); if (int r = copy_f32(c->bfin, data, c->D, s)) return r; });
    c->slot.fin_ada.w = SETTER("emb_to_latent.adaLN_modulation.1.weight", {
        WANT(2 * kC, kC);
        if (int r = copy_f32(c->ada_w + (size_t)c->final_off() * kC, data, (size_t)2 * kC * kC, s)) return r;
    });
    c->slot.fin_ada.b = SETTER("emb_to_latent.adaLN_modulation.1.bias",
           { WANT(2 * kC); if (int r = copy_f32(c->ada_b + c->final_off(), data, 2 * kC, s)) return r; });
    c->trunk.resize(nl);
    c->ipa.resize(nl);
    for (int i = 0; i < nl; ++i) {
        const std::string p = "layers." + std::to_string(i) + ".";
        TrunkW* t = &c->trunk[i];
        t->ada.w = SETTER(p + "adaLN_modulation.1.weight", {
            WANT(9 * kC, kC);
            if (int r = copy_f32(c->ada_w + (size_t)c->trunk_off(i) * kC, data, (size_t)9 * kC * kC, s)) return r;
        });
        t->ada.b = SETTER(p + "adaLN_modulation.1.bias",
               { WANT(9 * kC); if (int r = copy_f32(c->ada_b + c->trunk_off(i), data, 9 * kC, s)) return r; });
        TRY(register_mha(c, p + "mha_t.attn.", &t->mha_t));
        TRY(register_mha(c, p + "mha_l.attn.", &t->mha_l));
        TRY(register_ffn(c, p, &t->ffn, true));
    }
    for (int i = 0; i < nl; ++i) {
        const std::string p = "ipa_layers." + std::to_string(i) + ".";
        IpaW* w = &c->ipa[i];
        TRY(c->dalloc(&w->gamma_beta, (size_t)2 * kC));
        TRY(c->dalloc(&w->wproj, (size_t)21 * kKS * 64));
        TRY(c->dalloc(&w->bproj, (size_t)kIpaProj));
        TRY(c->dalloc(&w->head_w, (size_t)4));
        TRY(c->dalloc(&w->wout, (size_t)12 * 16 * 64));
        TRY(c->dalloc(&w->bout, (size_t)kC));
        w->slot.ada.w = SETTER(p + "adaLN_modulation.1.weight", {
            WANT(6 * kC, kC);
            if (int r = copy_f32(c->ada_w + (size_t)c->ipa_off(i) * kC, data, (size_t)6 * kC * kC, s)) return r;
        });
        w->slot.ada.b = SETTER(p + "adaLN_modulation.1.bias",
               { WANT(6 * kC); if (int r = copy_f32(c->ada_b + c->ipa_off(i), data, 6 * kC, s)) return r; });
        w->slot.norm.w = SETTER(p + "ipa_norm.weight", { WANT(kC); if (int r = copy_f32(w->gamma_beta, data, kC, s)) return r; });
        w->slot.norm.b = SETTER(p + "ipa_norm.bias", { WANT(kC); if (int r = copy_f32(w->gamma_beta + kC, data, kC, s)) return r; });
        w->slot.head_w = SETTER(p + "ipa.head_weights", { WANT(4); if (int r = copy_f32(w->head_w, data, 4, s)) return r; });
        w->slot.q.w = SETTER(p + "ipa.linear_q.weight", { WANT(128, kC); launch_pack_rows(data, kC, c->map_nat, 4, kKS, 1.f, w->wproj, s); });
        w->slot.q.b = SETTER(p + "ipa.linear_q.bias", { WANT(128); if (int r = copy_f32(w->bproj, data, 128, s)) return r; });
        w->slot.kv.w = SETTER(p + "ipa.linear_kv.weight",
               { WANT(256, kC); launch_pack_rows(data, kC, c->map_nat, 8, kKS, 1.f, w->wproj + (size_t)4 * kKS * 64, s); });
        w->slot.kv.b = SETTER(p + "ipa.linear_kv.bias", { WANT(256); if (int r = copy_f32(w->bproj + 128, data, 256, s)) return r; });
        w->slot.q_points.w = SETTER(p + "ipa.linear_q_points.weight",
               { WANT(96, kC); launch_pack_rows(data, kC, c->map_nat, 3, kKS, 1.f, w->wproj + (size_t)12 * kKS * 64, s); });
        w->slot.q_points.b = SETTER(p + "ipa.linear_q_points.bias", { WANT(96); if (int r = copy_f32(w->bproj + 384, data, 96, s)) return r; });
        w->slot.kv_points.w = SETTER(p + "ipa.linear_kv_points.weight",
               { WANT(192, kC); launch_pack_rows(data, kC, c->map_nat, 6, kKS, 1.f, w->wproj + (size_t)15 * kKS * 64, s); });
        w->slot.kv_points.b = SETTER(p + "ipa.linear_kv_points.bias", { WANT(192); if (int r = copy_f32(w->bproj + 480, data, 192, s)) return r; });
        w->slot.out.w = SETTER(p + "ipa.linear_out.weight",
               { WANT(kC, kIpaFeat); launch_pack_rows(data, kIpaFeat, c->map_nat, 12, 16, 1.f, w->wout, s); });
        w->slot.out.b = SETTER(p + "ipa.linear_out.bias", { WANT(kC); if (int r = copy_f32(w->bout, data, kC, s)) return r; });
        TRY(register_mha(c, p + "mha_l.attn.", &w->mha_l));
        TRY(register_ffn(c, p, &w->ffn, false));
    }
#undef TRY
    *out = c;
    return 0;
}

extern "C" int32_t mdgen_ctx_destroy(mdgen_ctx* c) {
    if (!c) return 0;
    for (auto& g : c->graphs) {
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
        if (g.graph) (void)hipGraphDestroy(g.graph);
    }
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    for (hipEvent_t e : c->train_ev) (void)hipEventDestroy(e);
    if (c->train_side) (void)hipStreamDestroy(c->train_side);
    if (c->tr_buf) (void)hipFree(c->tr_buf);
    if (c->ode_host) (void)hipHostFree(c->ode_host);
    for (int i = 0; i < mdgen_ctx::kMaxSide; ++i) {
        if (c->ev_join[i]) (void)hipEventDestroy(c->ev_join[i]);
        if (c->side[i]) (void)hipStreamDestroy(c->side[i]);
    }
    for (void* p : c->allocs) (void)hipFree(p);
    delete c;
    return 0;
}

extern "C" int32_t mdgen_ctx_num_weights(const mdgen_ctx* c) { return c ? (int32_t)c->weights.size() : 0; }
extern "C" const char* mdgen_ctx_weight_name(const mdgen_ctx* c, int32_t i) {
    if (!c || i < 0 || i >= (int32_t)c->weights.size()) return nullptr;
    return c->weights[i].name.c_str();
}

extern "C" int32_t mdgen_ctx_set_weight(mdgen_ctx* c, const char* key, const float* data, const int64_t* shape,
                                        int32_t ndim, void* stream) {
    if (!c || !key || !data || !shape) return fail(-1, "null argument");
    auto it = c->slot_of.find(key);
    if (it == c->slot_of.end()) return fail(-4, "unknown weight key '%s'", key);
    WeightSlot& w = c->weights[it->second];
    const int r = w.set(data, shape, ndim, (hipStream_t)stream);
    if (r) {
        if (r == -3) {
            char buf[160] = "";
            int o = 0;
            for (int i = 0; i < ndim && o < 140; ++i) o += snprintf(buf + o, sizeof(buf) - o, "%lld,", (long long)shape[i]);
            return fail(-3, "unexpected shape (%s) for weight '%s'", buf, key);
        }
        return r;
    }
    LAUNCHCHK();
    if (c->opt_keep_fp32) {
        size_t n = 1;
        for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
        if (!w.f32)
            if (int e = c->dalloc(&w.f32, n)) return e;
        // a BOUND entry (mdgen_train_bind_params) is the caller's master copy of the parameter: never written from here -- a
        // set_weight with other values (EMA weights swapped in for validation) only re-packs the sampler's operands
        if (w.f32 != data && !w.bound)
            HIPCHK(hipMemcpyAsync(w.f32, data, n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    }
    w.provided = true;
    c->finalized = false;
    return 0;
}

extern "C" int32_t mdgen_ctx_finalize(mdgen_ctx* c, void* stream) {
    if (!c) return fail(-1, "null context");
    for (const WeightSlot& w : c->weights)
        if (!w.provided) return fail(-5, "weight '%s' was not provided", w.name.c_str());
    if (!c->inv_freq_set) return fail(-5, "rot_emb.inv_freq was not provided");
    launch_rope_table(c->rope, c->inv_freq, kMaxPos + 1, (hipStream_t)stream);
    LAUNCHCHK();
    // tables that depend on two weights (the learned bias key and the rotary frequencies): after both, in stream order
    auto l4tab = [&](const MhaW& m) { launch_l4_bias_table(m.bias_k, m.bias_v, c->rope, m.l4tab, (hipStream_t)stream); };
    for (const TrunkW& t : c->trunk) l4tab(t.mha_l);
    for (const IpaW& w : c->ipa) l4tab(w.mha_l);
    LAUNCHCHK();
    c->finalized = true;
    return 0;
}

extern "C" int32_t mdgen_ctx_set_option(mdgen_ctx* c, const char* name, int32_t value) {
    if (!c || !name) return fail(-1, "null argument");
    const std::string n(name);
    if (n == "streams") {
        if (value < 1 || value > mdgen_ctx::kMaxSide + 1) return fail(-2, "streams must be in 1..%d", mdgen_ctx::kMaxSide + 1);
        c->opt_streams = value;
        c->opt_streams_auto = false;
    } else if (n == "keep_fp32_weights") {
        if (value != 0 && value != 1) return fail(-2, "keep_fp32_weights must be 0 or 1");
        c->opt_keep_fp32 = value;
    } else if (n == "precision") {
        if (value != 16 && value != 32) return fail(-2, "precision must be 16 (bf16 operands) or 32 (fp32 operands)");
        if (value == 32 && (!c->opt_keep_fp32 || !c->any_f32()))
            return fail(-6, "precision 32 needs the fp32 weight copies: set option keep_fp32_weights = 1 before loading weights");
        c->opt_precision = value;
    } else if (n == "attention_path") {
        if (value != 0 && value != 1) return fail(-2, "attention_path must be 0 (auto) or 1 (robust loop always)");
        c->opt_attn_path = value;
    } else if (n == "fuse_proj") {
        if (value != 0 && value != 3) return fail(-2, "fuse_proj must be 0 (off) or 3 (inside the panel MLP kernel where that kernel runs)");
        c->opt_fuse_proj = value;
    } else if (n == "fuse_proj_qkv") {
        if (value != 0 && value != 1) return fail(-2, "fuse_proj_qkv must be 0 or 1");
        c->opt_fuse_proj_qkv = value;
    } else if (n == "small_split") {
        if (value != 0 && value != 1) return fail(-2, "small_split must be 0 or 1");
        c->opt_small_split = value;
    } else if (n == "panel_waves") {
        if (value != 0 && value != 4 && value != 8) return fail(-2, "panel_waves must be 0 (by launch size), 4 or 8");
        c->opt_panel_waves = value;
    } else if (n == "flash_rotate") {
        if (value != 0 && value != 1) return fail(-2, "flash_rotate must be 0 or 1");
        c->opt_flash_rotate = value;
    } else if (n == "flash_proj_form") {
        if (value != 0 && value != 4 && value != 8) return fail(-2, "flash_proj_form must be 0 (by shape), 4 or 8");
        c->opt_flash_proj_form = value;
    } else if (n == "flash_proj") {
        if (value < 0 || value > 2) return fail(-2, "flash_proj must be 0 (off), 1 (launches that fill the chip) or 2 (always)");
        c->opt_flash_proj = value;
    } else if (n == "mlp_path") {
        if (value < 0 || value > 2) return fail(-2, "mlp_path must be 0 (panel kernel), 1 (row-owner kernel when it fills the chip) or 2 (always)");
        c->opt_mlp_path = value;
    } else if (n == "train_precision") {
        if (value != 16 && value != 32) return fail(-2, "train_precision must be 32 (fp32 operands, exact) or 16 (bf16 operands, fp32 accumulate)");
        c->opt_train_precision = value;
    } else if (n == "train_streams") {
        if (value != 1 && value != 2) return fail(-2, "train_streams must be 1 (one stream) or 2 (weight gradients on a second stream)");
        c->opt_train_streams = value;
    } else if (n == "mlp_fold") {
        if (value != 0 && value != 1) return fail(-2, "mlp_fold must be 0 or 1");
        c->opt_mlp_fold = value;
    } else if (n == "mlp_tail") {
        if (value < 0 || value > 2) return fail(-2, "mlp_tail must be 0 (off), 1 (FinalLayer + Euler update) or 2 (... + the next step's token embedding)");
        c->opt_mlp_tail = value;
    } else if (n == "residue_l4_path") {
        if (value < 0 || value > 2) return fail(-2, "residue_l4_path must be 0, 1 or 2");
        c->opt_residue_l4 = value;
    } else {
        return fail(-4, "unknown option '%s'", name);
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------
// workspace
// ---------------------------------------------------------------------------------------------
static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// panels the split scratch of a call covers, and its bytes (counters first: make_run zeroes them in every call): the largest launch that
// can take the split form has ncu / kMlpSplit panels; nothing but the counter block when the option is off
static long split_panels(const mdgen_ctx* c, long maxrows) {
    if (!c->opt_small_split) return 0;
    const long pn = (maxrows + kPanel - 1) / kPanel, cap = c->ncu / kMlpSplit < kMlpSplitMaxPanels ? c->ncu / kMlpSplit : kMlpSplitMaxPanels;
    return pn < cap ? pn : cap;
}
constexpr size_t kSplitCounterBytes = 1024;   // kMlpSplitMaxPanels counters, padded
static_assert(kMlpSplitMaxPanels * sizeof(unsigned) <= kSplitCounterBytes, "counter block");
static size_t split_bytes(long panels) { return kSplitCounterBytes + 2 * (size_t)panels * kMlpSplit * kPanel * kC * 4; }

// Row-owner MLP kernel: one workgroup = 4 waves x 32 rows and one workgroup per CU, so it needs ~200 workgroups to fill the
// chip; smaller launches (IPA stack, B = 1 tetrapeptides) stay on the 64-row panel kernel.  Monotone in nrows.
static bool mlp_uses_rows(const mdgen_ctx* c, long nrows) {
    const long tiles = (nrows + 31) / 32;
    return c->opt_mlp_path == 2 || (c->opt_mlp_path == 1 && tiles >= 3L * c->ncu);   // (768 row tiles = 192 four-wave workgroups on the 256-CU part)
}
// Gate fold (option mlp_fold): per (step, trunk layer) one MLP weight stream with that step's gate folded into fc2, and b2' = gate * b2.
// For a call that shares t across the batch and whose trunk launches of `nrows` rows take the row-owner kernel.  Asked with two
// row counts: mdgen_workspace_layout (public, knows no views) carves the region from the whole call's N, an upper bound of any
// view's rows; prepare() packs the streams when the call's largest VIEW passes, the launches that would consume them.
constexpr size_t kFoldStreamBytes = (size_t)kMlpFrags * 1024;
constexpr size_t kFoldMaxBytes = (size_t)8 << 30;   // a call with so many steps that its streams would pass 8 GiB keeps the unfolded kernel
static size_t fold_bytes(const mdgen_ctx* c, int S) { return (size_t)S * c->nl * (kFoldStreamBytes + (size_t)kC * 4); }
static bool fold_on(const mdgen_ctx* c, long nrows, int t_shared, int S) {
    return t_shared && c->opt_mlp_fold && c->opt_precision == 16 && mlp_uses_rows(c, nrows) && fold_bytes(c, S) <= kFoldMaxBytes;
}
// ... and (option mlp_tail 2) steps 1 .. S-1 take their token embedding from the previous step's last MLP launch, which needs the
// embedding's base rows per (step, b, l)
static bool embed_base_on(const mdgen_ctx* c, long nrows, int t_shared, int S) {
    return fold_on(c, nrows, t_shared, S) && c->opt_mlp_tail == 2 && S > 1;
}

static size_t frag_bytes(long nseq, int len) { return (size_t)nseq * kH * (len / 32 + 1) * kFragBytes; }
// K tiles are stored compact and packed back to back (kFragK each: three quarters of a Q / V^T tile's allocation) ...
static size_t k_frag_bytes(long nseq, int len) { return (size_t)nseq * kH * (len / 32 + 1) * kFragK; }
// ... so nothing of a tile's own allocation lies behind the last K fragment any more, while k_flash loads K tiles ahead of their
// use UNCONDITIONALLY: up to two tiles past the end of a (sequence, head), whose values it never uses but which must be mapped (and
// are kept finite: prepare() zeroes the region).  The region therefore ends with this slack -- two tiles, rounded up to 4 KiB.
constexpr size_t kFragSlackK = 4096;
static_assert(kFragSlackK >= 2 * (size_t)kFragK, "k_flash reads up to two K tiles past the last fragment");

// The panel prologues / epilogues (csrc/panel.h) address the residual stream as a uniform base + a 32-bit byte
// offset token * 1536, so ONE launch may cover at most kMaxViewTokens token rows.  Larger batches are run as
// several contiguous sub-batch views (plan_views); one sample (T * L tokens) must fit a view by itself.
constexpr long kMaxViewTokens = 0xFFFFFFFFL / (kC * 4);   // 2 796 202

// Contiguous sub-batch views of a call: at least `streams` of them (capped by B), and as many as the per-launch
// token limit requires.  Returns the number of views, 0 if a single sample already exceeds the limit.
static int plan_views(long B, long T, long L, int streams) {
    const long tl = T * L;
    if (tl > kMaxViewTokens) return 0;
    const long per = kMaxViewTokens / tl;              // samples per view at most
    long nv = (B + per - 1) / per;
    if (nv < streams) nv = streams;
    if (nv > B) nv = B;
    while ((B + nv - 1) / nv > per) ++nv;              // the largest view (ceil(B / nv) samples) must fit
    return (int)nv;
}

extern "C" int32_t mdgen_debug_view_plan(const mdgen_shape* sh, int32_t streams, int32_t* n_views,
                                         int32_t* max_batch_per_view) {
    if (!sh || !n_views || !max_batch_per_view) return fail(-1, "null argument");
    if (sh->B < 1 || sh->T < 1 || sh->L < 1 || streams < 1) return fail(-2, "B, T, L, streams must be >= 1");
    const int nv = plan_views(sh->B, sh->T, sh->L, streams);
    if (nv == 0) return fail(-2, "one sample (T*L = %ld tokens) exceeds the per-launch limit of %ld tokens",
                             (long)sh->T * sh->L, kMaxViewTokens);
    *n_views = nv;
    *max_batch_per_view = (sh->B + nv - 1) / nv;
    return 0;
}

static int check_shape(const mdgen_ctx* c, const mdgen_shape* sh, int S) {
    if (!c || !sh) return fail(-1, "null argument");
    if (sh->B < 1 || sh->T < 1 || sh->L < 1 || S < 1) return fail(-2, "B, T, L, n_steps must be >= 1");
    if (sh->T > kMaxPos - 1 || sh->L > kMaxPos - 1) return fail(-2, "T and L must be < %d", kMaxPos - 1);
    if ((long)sh->B * sh->T * sh->L > 1500000000L) return fail(-2, "token count too large");
    if ((long)sh->T * sh->L > kMaxViewTokens)
        return fail(-2, "one sample (T*L = %ld tokens) exceeds the per-launch limit of %ld tokens", (long)sh->T * sh->L,
                    kMaxViewTokens);
    if ((long)S * sh->B * sh->L > kMaxViewTokens)
        return fail(-2, "n_steps*B*L = %ld rows of the IPA table exceed the per-launch limit of %ld", (long)S * sh->B * sh->L,
                    kMaxViewTokens);
    if (c->d.abs_pos_emb && sh->L > c->d.crop) return fail(-2, "L=%d exceeds pos_embed crop=%d", sh->L, c->d.crop);
    return 0;
}

extern "C" int32_t mdgen_workspace_layout(const mdgen_ctx* c, const mdgen_shape* sh, int32_t S, int32_t t_shared,
                                          mdgen_ws_layout* o) {
    if (!o) return fail(-1, "null argument");
    if (int r = check_shape(c, sh, S)) return r;
    const long B = sh->B, T = sh->T, L = sh->L;
    const long N = B * T * L, Mp = (long)S * B * L, R = t_shared ? S : (long)S * B;
    const long maxrows = N > Mp ? N : Mp;
    size_t fq = (size_t)maxrows * 3 * kC * 2;  // SMALL layout lives in the q region
    size_t fkv = 0, fk = 0;   // V^T region (the key-validity words live in its tiles' slack, kernels.h), K region
    auto upd = [&](long nseq, int len) {
        const size_t b = frag_bytes(nseq, len), k = k_frag_bytes(nseq, len);
        if (b > fq) fq = b;
        if (b > fkv) fkv = b;
        if (k > fk) fk = k;
    };
    upd(B * L, (int)T);
    if (L > 8) {
        upd(B * T, (int)L);
        upd((long)S * B, (int)L);
    }
    if (fkv == 0) fkv = 256;
    fk += kFragSlackK;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t a = off; off += align256(bytes); return a; };
    o->h = take((size_t)N * kC * 4);
    o->qf = take(fq);
    o->kf = take(fk);
    o->vf = take(fkv);
    o->obuf = take((size_t)maxrows * kC * 2);
    o->mod = take((size_t)R * c->modrow * 4);
    o->silu_t = take((size_t)R * kC * 4);
    o->ipa_out = take((size_t)Mp * kC * 4);
    o->h_ipa = take((size_t)Mp * kC * 4 * (c->d.tps_condition ? 2 : 1));
    o->ipa_proj = take((size_t)Mp * kIpaProj * 4);
    o->ipa_feat = take((size_t)Mp * kIpaFeat * 2);
    o->mask_bl = take((size_t)B * L * 4);
    o->rel7 = take((size_t)2 * B * L * 7 * 4);
    o->tgrid = take((size_t)S * B * 4);
    // fp32 path scratch: LN output [rows][384] | q,k,v [rows][1152] | attention output [rows][384] | MLP hidden
    // [rows][1536] | IPA features [Mp][256]   (only when the context keeps fp32 weights)
    o->f32_scratch = take(c->opt_keep_fp32 ? (size_t)maxrows * (kC + 3 * kC + kC + kF) * 4 + (size_t)Mp * kIpaFeat * 4 : 0);
    // k_mlp8's split form (launches of <= ncu / kMlpSplit panels): counters [kMlpSplitMaxPanels] | fc2 partials | private residual rows,
    // the latter two [panels][kMlpSplit][64][384] fp32 each
    o->split = take(split_bytes(split_panels(c, maxrows)));
    // per-(step, layer) gate-folded MLP streams [S][nl][2304 KiB] | b2' [S][nl][384] fp32 (0 bytes unless fold_on)
    o->fold = take(fold_on(c, N, t_shared, S) ? fold_bytes(c, S) : 0);
    // base rows of the token embedding per (step, b, l) for the embedding-as-tail form [S][B*L][384] fp32 (0 bytes unless embed_base_on)
    o->embase = take(embed_base_on(c, N, t_shared, S) ? (size_t)Mp * kC * 4 : 0);
    o->total_bytes = off;
    return 0;
}

// ---------------------------------------------------------------------------------------------
// orchestration
// ---------------------------------------------------------------------------------------------
struct Run {
    mdgen_ctx* c;
    int B, T, L, D, S;
    long N, Mp;
    int t_shared;
    long mod_step_stride, mod_group_stride;
    unsigned char* ws;
    mdgen_ws_layout lay;
    const float *mask, *start_rot, *start_trans, *end_rot, *end_trans, *x_cond;
    const float* rel7_in;        // caller-supplied relative-frame 7-vectors (2,B,L,7) of the two-sided model, or null
    const int64_t *x_cond_mask, *aatype;
    hipStream_t s;
    // trunk buffers (a sub-batch view shifts these; see sub_run)
    float* hp;
    unsigned char *qfp, *kfp, *vfp;
    __bf16* obufp;
    float* modp;                 // adaLN table row of (step 0, first batch element of this view)
    const float* ipa_out_p;      // IPA table of (step 0, first batch element of this view)
    long ipa_step_stride;        // floats between consecutive steps of the IPA table
    // split scratch (layout.split): arrival counters, fc2 partials, private residual rows; split_cap panels
    unsigned* split_counters;
    float *split_part, *split_hupd;
    long split_cap;
    // gate fold: streams [S][nl][kFoldStreamBytes], then b2' [S][nl][384]; null when off for this call
    unsigned char* fold_streams;
    float* fold_b2g;
    bool fold_ready;   // prepare() has packed them for this call (its views' MLP launches take the row-owner kernel)
    // embedding-as-tail: base rows [S][B*L][384] (step 0, first batch element of this view), null when off; floats between steps
    const float* embase_p;
    long embase_step_stride;
    bool no_embed_tail;          // the call never runs the embedding-as-tail form (mdgen_sample_dopri5, mdgen_sample_rk): prepare() skips its base rows
    const RkState* rk;           // stage descriptor of a fixed-grid Runge-Kutta evaluation (ode.inc): denoise_step embeds the state it
                                 // describes (k_rk_embed) instead of x; pointers of THIS view.  Null: x is embedded as it is
    const SdeState* sde;         // the same for an SDE state (sde.inc, k_sde_embed); at most one of rk / sde is set
    bool concurrent;             // a view whose launches run beside other views' on other streams: kernels that use the call's split
                                 // scratch (one launch at a time) stay off meanwhile (for_each_view)
    float* h() const { return hp; }
    float* mod() const { return modp; }
};

// View of the contiguous sub-batch [b0, b0+Bs) of a prepared call: every trunk buffer is per-token (or per
// sequence) and batch-major, so a sub-batch is a pointer shift.  Used to run two halves of the batch on two
// streams: their kernels are in different phases (HBM-bound prologues/epilogues, VALU-bound attention,
// MFMA-bound GEMMs) and overlap on the CUs instead of queueing behind each other.
static Run sub_run(const Run& r, int b0, int Bs, hipStream_t stream) {
    Run v = r;
    const long tl = (long)r.T * r.L;
    v.B = Bs;
    v.N = (long)Bs * tl;
    v.s = stream;
    v.mask = r.mask + b0 * tl;
    v.x_cond = r.x_cond + b0 * tl * r.D;
    v.x_cond_mask = r.x_cond_mask + b0 * tl;
    v.hp = r.hp + b0 * tl * kC;
    v.obufp = r.obufp + b0 * tl * kC;
    // q region: max(SMALL layout, fragment layouts) per batch element; k/v regions: fragment layouts
    const size_t per_b_small = (size_t)tl * 3 * kC * 2;
    const size_t per_b_fragT = (size_t)r.L * kH * (r.T / 32 + 1) * kFragBytes;
    const size_t per_b_fragL = r.L > 8 ? (size_t)r.T * kH * (r.L / 32 + 1) * kFragBytes : 0;
    const size_t per_b_kv = per_b_fragT > per_b_fragL ? per_b_fragT : per_b_fragL;
    const size_t per_b_q = per_b_small > per_b_kv ? per_b_small : per_b_kv;
    v.qfp = r.qfp + (size_t)b0 * per_b_q;
    v.kfp = r.kfp + (size_t)b0 * (per_b_kv / kFragBytes * kFragK);   // (K tiles are kFragK apart)
    v.vfp = r.vfp + (size_t)b0 * per_b_kv;
    v.modp = r.modp + (long)b0 * r.mod_group_stride;
    v.ipa_out_p = r.ipa_out_p + (long)b0 * r.L * kC;
    if (r.embase_p) v.embase_p = r.embase_p + (long)b0 * r.L * kC;
    return v;
}

// The nv contiguous sub-batch views of a prepared call (plan_views), view i on stream i % ns (0: the call's own): fn(view, b0), b0 =
// the view's first sample.  The launches that follow belong to the view (plan mode), until the loop ends.
template <typename F>
static int for_each_view(const Run& r, int nv, int ns, F&& fn) {
    int b0 = 0, e = 0;
    for (int i = 0; i < nv && !e; ++i) {
        const int Bs = r.B / nv + (i < r.B % nv ? 1 : 0);
        Run v = sub_run(r, b0, Bs, i % ns == 0 ? r.s : r.c->side[i % ns - 1]);
        v.concurrent = ns > 1;
        if (g_dry) g_dry->view = i;
        e = fn(v, b0);
        b0 += Bs;
    }
    if (g_dry) g_dry->view = -1;
    return e;
}
// token rows of the largest of them: what prepare() sizes its decisions by
static long largest_view_rows(const Run& r, int nv) { return (long)((r.B + nv - 1) / nv) * r.T * r.L; }

// ---- the model's geometry: every axis, mask and modulation map of the network, written here and nowhere else ----
// Tokens are (b, t, l) in the trunk and (group, l) in the IPA stack (G = S * B groups: prepared step, batch element).
// residue axis: one sequence of L tokens per frame (b, t)
static AxisMap axis_res(long B, long T, long L) { return AxisMap{(int)(B * T), (int)L, (int)(B * T), 0, (int)L, 1}; }
// temporal axis: one sequence of T tokens, L apart, per residue (b, l)
static AxisMap axis_time(long B, long T, long L) { return AxisMap{(int)(B * L), (int)T, (int)L, (int)(T * L), 1, (int)L}; }
// the IPA stack's residue axis
static AxisMap axis_ipa(long G, long L) { return AxisMap{(int)G, (int)L, (int)G, 0, (int)L, 1}; }
static AxisMap axis_res(const Run& r) { return axis_res(r.B, r.T, r.L); }
static AxisMap axis_time(const Run& r) { return axis_time(r.B, r.T, r.L); }
static AxisMap axis_ipa(const Run& r) { return axis_ipa((long)r.S * r.B, r.L); }
// key-padding masks: the trunk's per token; the IPA stack's mask[b][0][l], compacted by prepare() / the training forward
static MaskMap mask_trunk(const Run& r) { return MaskMap{r.mask, 0}; }
static MaskMap mask_ipa(const Run& r) { return MaskMap{(const float*)(r.ws + r.lay.mask_bl), (long)r.B * r.L}; }
// adaLN rows: the IPA layers' for all prepared steps at once (groups of L tokens), the trunk's and the final layer's of one step
static ModMap mod_ipa(const Run& r, int i) {
    return ModMap{r.mod() + r.c->ipa_off(i), r.L, r.B, r.mod_step_stride, r.mod_group_stride};
}
static ModMap mod_step(const Run& r, int off, int step) {
    return ModMap{r.mod() + (long)step * r.mod_step_stride + off, r.T * r.L, r.B, 0, r.mod_group_stride};
}
static ModMap mod_trunk(const Run& r, int i, int step) { return mod_step(r, r.c->trunk_off(i), step); }
static ModMap mod_final(const Run& r, int step) { return mod_step(r, r.c->final_off(), step); }
// an affine LayerNorm as a modulation: the one row gamma - 1 | beta for every token
static ModMap mod_affine(const float* gamma_beta) { return ModMap{gamma_beta, 1, 1, 0, 0}; }

// One sub-layer's site: the rows it updates, its three adaLN chunks (shift, scale, gate = chunk0, +1, +2), the axis and mask of
// an attention sub-layer, and in the training step the sub-layer's rows of d mod (dmod, addressed like mm.mod)
struct Rows {
    float* h;
    long nrows;
    ModMap mm;
    int chunk0;
    float* dmod;
    AxisMap ax;      // (attention only)
    MaskMap mk;
    int shift() const { return chunk0; }
    int scale() const { return chunk0 + 1; }
    int gate() const { return chunk0 + 2; }
    long tpg() const { return mm.tokens_per_group; }   // tokens per modulation group
};
// The sites of IPA layer i on the stream's rows h, and of trunk layer i at prepared step `step`; dmod: the call's d mod table (the
// training step), or null.  The sampler, the training forward and the training backward all take a layer's sites from here.
struct IpaSites { Rows attn, mlp; };
struct TrunkSites { Rows l, t, mlp; };
static IpaSites ipa_sites(const Run& r, int i, float* h, float* dmod) {
    const ModMap mm = mod_ipa(r, i);
    float* dm = dmod ? dmod + r.c->ipa_off(i) : nullptr;
    return IpaSites{Rows{h, r.Mp, mm, 0, dm, axis_ipa(r), mask_ipa(r)}, Rows{h, r.Mp, mm, 3, dm}};
}
static TrunkSites trunk_sites(const Run& r, int i, int step, float* dmod) {
    const ModMap mm = mod_trunk(r, i, step);
    float* dm = dmod ? dmod + r.c->trunk_off(i) : nullptr;
    return TrunkSites{Rows{r.h(), r.N, mm, 0, dm, axis_res(r), mask_trunk(r)}, Rows{r.h(), r.N, mm, 3, dm, axis_time(r), mask_trunk(r)},
                      Rows{r.h(), r.N, mm, 6, dm}};
}
// ... of the final layer (shift, scale = chunks 0, 1; it has no gate)
static Rows final_site(const Run& r, int step, float* dmod) {
    return Rows{r.h(), r.N, mod_final(r, step), 0, dmod ? dmod + r.c->final_off() : nullptr};
}

// ---- fp32-operand path (option "precision" = 32; kernels in k_fp32.hip) ------------------------------------------
struct F32Bufs {
    float *y, *qkv, *att, *hid, *feat;
};
static F32Bufs f32_bufs(const Run& r) {
    const long maxrows = r.N > r.Mp ? r.N : r.Mp;
    float* b = (float*)(r.ws + r.lay.f32_scratch);
    F32Bufs o;
    o.y = b;
    o.qkv = o.y + maxrows * kC;
    o.att = o.qkv + maxrows * 3 * kC;
    o.hid = o.att + maxrows * kC;
    o.feat = o.hid + maxrows * kF;
    return o;
}
// The fp32 path and the training step read every parameter's fp32 copy: all of them are checked here, before the call's first
// launch (make_run), so that the code below reads c->f32(slot) without a test.  A slot lacks its copy when option keep_fp32_weights
// was switched on after that weight had been handed over.
static int check_f32_weights(const mdgen_ctx* c) {
    for (const WeightSlot& w : c->weights)
        if (!w.f32) return fail(-6, "fp32 copy of weight '%s' is missing (option keep_fp32_weights)", w.name.c_str());
    return 0;
}

static const ModMap kNoMod{nullptr, 1, 1, 0, 0};
// the IPA block's four input projections q | kv | q_points | kv_points of LN(x): output columns [col0, col0 + m) of the kIpaProj-wide rows
struct IpaProjCols { int col0, m; };
static const IpaProjCols kIpaProjCols[4] = {{0, 128}, {128, 256}, {384, 96}, {480, 192}};
// The operands of one linear layer c[n][0 .. m) (ldc) = a[n][k] (lda) w[m][k]^T (ldw) + bias, plain store (linear.h LinearParams);
// the caller sets what its launch has beyond that: mode and the mode's operands, col0, wtrans, the bf16-operand mode's fields
static LinearParams lin_op(const float* a, int lda, const float* w, int ldw, const float* bias, long n, int m, int k, float* c, int ldc) {
    LinearParams p{};
    p.a = a; p.lda = lda; p.w = w; p.ldw = ldw; p.bias = bias;
    p.n = n; p.m = m; p.k = k;
    p.mode = kLinStore;
    p.c = c; p.ldc = ldc;
    p.mm = kNoMod;
    return p;
}
// ... with the gated residual as the epilogue: c += gate * (a w^T + bias), gate = chunk `gate` of the row's modulation
static LinearParams lin_op_gated(LinearParams p, const ModMap& mm, int gate) {
    p.mode = kLinGated; p.mm = mm; p.gate_chunk = gate; p.gated = 1;
    return p;
}

// one attention sub-layer, fp32: LN + modulate -> q, k, v -> RoPE -> softmax attention -> out-projection + gated residual
static int attn_sublayer_fp32(const Run& r, const MhaW& m, const Rows& rw) {
    const mdgen_ctx* c = r.c;
    const F32Bufs b = f32_bufs(r);
    const auto& p = m.slot;
    float* h = rw.h;
    const long nrows = rw.nrows;
    launch32_ln_mod(h, nrows, rw.mm, rw.shift(), rw.scale(), 0, 1e-6f, b.y, r.s, nullptr, false);
    LinearParams q = lin_op(b.y, kC, c->f32(p.q.w), kC, c->f32(p.q.b), nrows, kC, kC, b.qkv, 3 * kC);
    q.mode = kLinScaled;
    q.scalar = 1.0f / std::sqrt((float)kDH);   // mha.py:263 q *= head_dim ** -0.5
    LinearParams k = lin_op(b.y, kC, c->f32(p.k.w), kC, c->f32(p.k.b), nrows, kC, kC, b.qkv, 3 * kC);
    k.col0 = kC;
    LinearParams v = lin_op(b.y, kC, c->f32(p.v.w), kC, c->f32(p.v.b), nrows, kC, kC, b.qkv, 3 * kC);
    v.col0 = 2 * kC;
    launch32_linear(q, r.s);
    launch32_linear(k, r.s);
    launch32_linear(v, r.s);
    launch32_rope(b.qkv, nrows, 3 * kC, rw.ax.pos_stride, rw.ax.len, c->inv_freq, r.s);   // position = (token / pos_stride) % len
    launch32_attn(b.qkv, 3 * kC, rw.ax, rw.mk, c->f32(p.bias_k), c->f32(p.bias_v), c->inv_freq, b.att, r.s, nullptr);
    launch32_linear(lin_op_gated(lin_op(b.att, kC, c->f32(p.o.w), kC, c->f32(p.o.b), nrows, kC, kC, h, kC), rw.mm, rw.gate()), r.s);
    LAUNCHCHK();
    return 0;
}

static int mlp_sublayer_fp32(const Run& r, const FfnW& f, const Rows& rw) {
    const mdgen_ctx* c = r.c;
    const F32Bufs b = f32_bufs(r);
    float* h = rw.h;
    const long nrows = rw.nrows;
    launch32_ln_mod(h, nrows, rw.mm, rw.shift(), rw.scale(), 0, 1e-6f, b.y, r.s, nullptr, false);
    LinearParams fc1 = lin_op(b.y, kC, c->f32(f.slot.fc1.w), kC, c->f32(f.slot.fc1.b), nrows, kF, kC, b.hid, kF);
    fc1.mode = kLinGelu;
    launch32_linear(fc1, r.s);
    launch32_linear(lin_op_gated(lin_op(b.hid, kF, c->f32(f.slot.fc2.w), kF, c->f32(f.slot.fc2.b), nrows, kC, kF, h, kC), rw.mm, rw.gate()), r.s);
    LAUNCHCHK();
    return 0;
}

// a linear layer in the form a plan gives it (kernels.h LinearForm; F32 = launch32_linear)
static void step_linear(LinearParams p, LinearForm form, hipStream_t s) {
    p.fast_gelu = form != LinearForm::F32;    // (see linear.h)
    p.a_bf16 = form == LinearForm::StreamBf16Rows;
    launch_linear(p, form, s);
}

// The IPA block of one layer on fp32 rows: hx += linear_out(point_attention(q | kv | q_points | kv_points of LN_affine(hx)))
// (latent_model.py:373).  The precision-32 sampler runs it on workspace scratch with every layer in the F32 form; the training
// forward on its tape (proj, feat, stats: read again by the backward) with the forms of its plan.
struct IpaBlockOp {
    float *y, *proj, *feat;          // LN output [Mp][384], projections [Mp][kIpaProj], attention features [Mp][kIpaFeat]
    float* stats;                    // nullable: the attention's softmax statistics [Mp][4]
    float* part;                     // nullable: split scratch of the attention's key loop (few groups)
    size_t part_floats;
    LinearForm proj_form[4], out_form;
};
static int ipa_block_fp32(const Run& r, const IpaW& w, float* hx, const float* rot, const float* trans, const IpaBlockOp& o) {
    const mdgen_ctx* c = r.c;
    const auto& p = w.slot;
    launch32_ln_mod(hx, r.Mp, mod_affine(w.gamma_beta), 1, 0, 1, 1e-5f, o.y, r.s, nullptr, false);
    const Lin* lins[4] = {&p.q, &p.kv, &p.q_points, &p.kv_points};
    for (int j = 0; j < 4; ++j) {
        LinearParams q = lin_op(o.y, kC, c->f32(lins[j]->w), kC, c->f32(lins[j]->b), r.Mp, kIpaProjCols[j].m, kC, o.proj, kIpaProj);
        q.col0 = kIpaProjCols[j].col0;
        step_linear(q, o.proj_form[j], r.s);
    }
    IpaAttnParams ap{};
    ap.proj = o.proj; ap.rot = rot; ap.trans = trans;
    ap.mask_bl = mask_ipa(r).mask;
    ap.head_w = w.head_w; ap.feat = nullptr; ap.feat32 = o.feat; ap.stats = o.stats;
    ap.ngroups = r.S * r.B; ap.B = r.B; ap.L = r.L;
    ap.part = o.part; ap.part_floats = o.part_floats;
    launch_ipa_attn(ap, r.s);
    LinearParams lo = lin_op(o.feat, kIpaFeat, c->f32(p.out.w), kIpaFeat, c->f32(p.out.b), r.Mp, kC, kIpaFeat, hx, kC);
    lo.mode = kLinGated;   // (gated = 0: the ungated residual hx += linear_out(feat))
    step_linear(lo, o.out_form, r.s);
    LAUNCHCHK();
    return 0;
}

// Every token-local kernel addresses the residual stream with 32-bit byte offsets (token * 1536; rows.h, panel.h): one
// launch may cover at most kMaxViewTokens rows.  The trunk is cut into views accordingly (plan_views); this guard is for
// whatever reaches a launcher directly (the IPA stack's S * B * L rows).
static int check_launch_rows(long nrows) {
    if (nrows > kMaxViewTokens)
        return fail(-7, "%ld token rows in one launch exceed the 32-bit offset limit of %ld (use a smaller batch per call)", nrows,
                    kMaxViewTokens);
    return 0;
}

// One launch of the bf16 sampler: the enqueue between a hipEvent pair on its stream (profiling mode only), then the launch check;
// in plan mode only its class is recorded.  cls == nullptr: a set-up kernel outside the profile classes.
template <typename F>
static int launch(const Run& r, const char* cls, F&& enqueue) {
    if (!g_dry) {
        ProfRec pr{cls, nullptr, nullptr};
        const bool prof = r.c->prof_on && cls && hipEventCreate(&pr.a) == hipSuccess && hipEventCreate(&pr.b) == hipSuccess &&
                          hipEventRecord(pr.a, r.s) == hipSuccess;
        enqueue();
        if (prof && hipEventRecord(pr.b, r.s) == hipSuccess) r.c->prof.push_back(pr);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail((int)e, "kernel launch failed: %s (%s)", hipGetErrorString(e), cls ? cls : "set-up");
        if (const char* m = k32_take_launch_error()) return fail(-7, "internal: %s (%s)", m, cls ? cls : "set-up");
    } else if (cls) {
        g_dry->rec.emplace_back(g_dry->view, cls);
    }
    return 0;
}

// ---- kernel forms: which instantiation each launch of a sub-layer takes (kernels.h), decided here, ONCE, from the options, the
// device and the launch's size; the launchers switch on the form and the profile class (tag) is a function of (position, form) ----
enum class Pos { Ipa, ResL, TimeT };   // attention sub-layer: IPA stack (residue axis), trunk residue axis, trunk temporal axis
static const char* by_pos(Pos p, const char* ipa, const char* l, const char* t) { return p == Pos::Ipa ? ipa : p == Pos::ResL ? l : t; }
static const char* tag(Pos p, QkvForm f) {
    switch (f) {
    case QkvForm::Small:
    case QkvForm::Panel4: return by_pos(p, "ipa.ln_qkv", "ln_qkv_L", "ln_qkv_T");
    case QkvForm::Panel8: return by_pos(p, "ipa.ln_qkv@p8", "ln_qkv_L@p8", "ln_qkv_T@p8");
    case QkvForm::Panel8Split: return by_pos(p, "ipa.ln_qkv@p8x2", "ln_qkv_L@p8x2", "ln_qkv_T@p8x2");
    case QkvForm::Panel8SplitHalf: return by_pos(p, "ipa.ln_qkv@h32x2", "ln_qkv_L@h32x2", "ln_qkv_T@h32x2");
    case QkvForm::PreProj: return "projL_qkvT";
    }
    return nullptr;
}
static const char* tag(Pos p, Attn4Form f) {
    switch (f) {
    case Attn4Form::AttnOnly: return by_pos(p, "ipa.ln_qkv", "ln_qkv_L", "ln_qkv_T");
    case Attn4Form::Fused: return by_pos(p, "ipa.ln_qkv", "attn_L_fused", "ln_qkv_T");
    case Attn4Form::FusedHalf: return by_pos(p, "ipa.ln_qkv@h32", "attn_L_fused@h32", "ln_qkv_T@h32");
    }
    return nullptr;
}
static const char* tag(Pos p, FlashProjForm f) {
    switch (f) {
    case FlashProjForm::Q64: return by_pos(p, "ipa.flash_proj@q64", "flash_proj_L@q64", "flash_proj_T@q64");
    case FlashProjForm::Q128: return by_pos(p, "ipa.flash_proj@q128", "flash_proj_L@q128", "flash_proj_T@q128");
    }
    return nullptr;
}
static const char* tag_flash(Pos p) { return by_pos(p, "ipa.flash", "flash_L", "flash_T"); }
static const char* tag_proj(Pos p) { return by_pos(p, "ipa.proj", "proj_L", "proj_T"); }
static const char* tag(bool trunk, MlpRowsForm f) {
    if (!trunk) return "ipa.mlp";
    switch (f) {
    case MlpRowsForm::Plain: return "mlp";
    case MlpRowsForm::Fold: return "mlp@fold";
    case MlpRowsForm::FoldFinal: return "mlp@fold+final";
    case MlpRowsForm::FoldFinalEmbed: return "mlp@fold+final+embed";
    }
    return nullptr;
}
static const char* tag(bool trunk, MlpPanelForm f) {
    switch (f) {
    case MlpPanelForm::W4: return trunk ? "mlp@p4" : "ipa.mlp@p4";
    case MlpPanelForm::W8: return trunk ? "mlp@p8" : "ipa.mlp@p8";
    case MlpPanelForm::W8Split: return trunk ? "mlp@p8x3" : "ipa.mlp@p8x3";
    case MlpPanelForm::PreW4: return trunk ? "proj_mlp@p4" : "ipa.mlp@p4";
    case MlpPanelForm::PreW8: return trunk ? "proj_mlp@p8" : "ipa.mlp@p8";
    case MlpPanelForm::PreW8Split: return trunk ? "proj_mlp@p8x3" : "ipa.mlp@p8x3";
    }
    return nullptr;
}

// Four or eight waves per 64-row panel (k_mlp / k_mlp8, k_ln_qkv<false> / k_ln_qkv8): eight where a launch is at most one
// workgroup per CU, unless option panel_waves forces one form
static int panel_waves_for(const mdgen_ctx* c, long panels) {
    return c->opt_panel_waves == 4 || c->opt_panel_waves == 8 ? c->opt_panel_waves : (panels <= c->ncu ? 8 : 4);
}
// q, k, v of a tiled-attention sub-layer in a launch of its own.  Far below one workgroup per CU (option small_split): q, k | v
// over a workgroup pair per panel, and 32 positions per pair where even those fit one per CU (B = 1 at T 1000: 256)
static QkvForm qkv_form(const mdgen_ctx* c, const AxisMap& ax) {
    const long panels = (long)ax.nseq * ((ax.len + kPanel - 1) / kPanel);
    if (panel_waves_for(c, panels) != 8) return QkvForm::Panel4;
    if (!c->opt_small_split || 2 * panels > c->ncu) return QkvForm::Panel8;
    return 2L * ax.nseq * ((ax.len + 31) / 32) <= c->ncu ? QkvForm::Panel8SplitHalf : QkvForm::Panel8Split;
}
// the whole L == 4 residue sub-layer in one kernel: launches of at most one 32-row workgroup per CU (B <= 2 at T 1000, the IPA
// stack) take half panels, twice the CUs at work (option small_split)
static Attn4Form attn4_fused_form(const mdgen_ctx* c, long nrows) {
    return c->opt_small_split && (nrows + 31) / 32 <= c->ncu ? Attn4Form::FusedHalf : Attn4Form::Fused;
}
// k_flash_proj owns a (sequence, 64-query chunk) for all 16 heads: four times the work of a k_flash workgroup, a quarter of the
// workgroups.  It pays where those still fill the chip (cfg-2: 1024 per launch, ATLAS: 1000 / 1024); small launches (B = 1: 64,
// the IPA stack) keep the finer-grained k_flash + projection.
// (two such workgroups per CU: 512 on the 256-CU part)
static bool flash_proj_on(const mdgen_ctx* c, const AxisMap& ax) {
    return c->opt_precision == 16 && (c->opt_flash_proj == 2 || (c->opt_flash_proj == 1 && flash_proj_jobs(ax) >= 2L * c->ncu));
}
// ... in the 128-row form where that still gives every CU a workgroup (cfg-2: 256 per sub-batch stream)
static FlashProjForm flash_proj_form(const mdgen_ctx* c, const AxisMap& ax) {
    const long jobs8 = (long)ax.nseq * ((ax.len + 2 * kPanel - 1) / (2 * kPanel));
    const int w = c->opt_flash_proj_form ? c->opt_flash_proj_form : (ax.len >= 512 && jobs8 >= c->ncu) ? 8 : 4;
    return w == 8 ? FlashProjForm::Q128 : FlashProjForm::Q64;
}

// An attention sub-layer's launches.  Quad: L == 4, the 5-key attention inside the q / k / v kernel (k_ln_qkv_attn4); Micro: L <= 8,
// attention inside the projection kernel (k_proj<2>); Tiled: k_ln_qkv -> k_flash -> out-projection, or k_flash_proj.
enum class AttnPath { Quad, Micro, Tiled };
// Where the out-projection + gated residual runs: a k_proj launch of its own, the kernel that computed the attention
// (k_ln_qkv_attn4<true>, k_flash_proj), the prologue of the temporal sub-layer's q / k / v kernel, the prologue of the panel MLP kernel
enum class ProjAt { Own, Attention, NextQkv, Mlp };
struct AttnPlan {
    Pos pos;
    AttnPath path;
    Attn4Form a4;        // Quad
    QkvForm qkv;         // Micro, Tiled
    bool flash_proj;     // Tiled: one k_flash_proj launch (form fp) instead of k_flash + projection
    FlashProjForm fp;
    ProjAt proj;
};
// pre: the previous sub-layer left its out-projection to this one's q / k / v kernel; later: where a tiled sub-layer without
// k_flash_proj may leave its own (Own, NextQkv or Mlp)
static AttnPlan attn_plan(const mdgen_ctx* c, Pos pos, const AxisMap& ax, long nrows, bool pre, ProjAt later) {
    AttnPlan a{pos, AttnPath::Tiled, Attn4Form::AttnOnly, QkvForm::Small, false, FlashProjForm::Q64, ProjAt::Own};
    const bool small = pos != Pos::TimeT && ax.len <= 8;
    if (small && ax.len == 4 && c->opt_residue_l4 != 0) {
        a.path = AttnPath::Quad;
        if (c->opt_residue_l4 == 2) {   // whole residue-axis sub-layer in one kernel (option 1: attention only)
            a.a4 = attn4_fused_form(c, nrows);
            a.proj = ProjAt::Attention;
        }
    } else if (small) {
        a.path = AttnPath::Micro;
    } else {
        a.qkv = pre ? QkvForm::PreProj : qkv_form(c, ax);
        a.flash_proj = flash_proj_on(c, ax);
        a.fp = flash_proj_form(c, ax);
        a.proj = a.flash_proj ? ProjAt::Attention : later;
    }
    return a;
}

// The MLP block's launch: the row-owner kernel (rows) or the 64-row panel kernel
struct MlpPlan {
    bool trunk, use_rows;
    MlpRowsForm rows;
    MlpPanelForm panel;
};
// pre: the temporal sub-layer left its out-projection to this launch (ProjAt::Mlp; only where the panel kernel runs anyway);
// rows: the form a row-owner launch takes (trunk: a Fold* form where the call's gate-folded streams are packed); concurrent: other
// views' launches run beside this one; split_cap: panels the call's split scratch covers; trace: this launch records phase stamps
static MlpPlan mlp_plan(const mdgen_ctx* c, bool trunk, long nrows, bool pre, MlpRowsForm rows, bool concurrent, long split_cap, bool trace) {
    MlpPlan m{trunk, !pre && mlp_uses_rows(c, nrows), rows, MlpPanelForm::W4};
    if (m.use_rows) return m;
    const long panels = (nrows + kPanel - 1) / kPanel;
    // (the phase stamps stay with k_mlp: a traced launch takes the four-wave kernel)
    const int pw = trace ? 4 : panel_waves_for(c, panels);
    // the split form: the call's scratch serves one launch at a time (one stream), and its workgroups must meet in one L2
    const bool split = pw == 8 && c->opt_small_split && c->xcd_round_robin && !concurrent && panels * kMlpSplit <= c->ncu && panels <= split_cap;
    m.panel = split ? (pre ? MlpPanelForm::PreW8Split : MlpPanelForm::W8Split)
              : pw == 8 ? (pre ? MlpPanelForm::PreW8 : MlpPanelForm::W8)
                        : (pre ? MlpPanelForm::PreW4 : MlpPanelForm::W4);
    return m;
}

// One trunk layer: residue-axis attention, temporal attention, MLP
struct LayerPlan {
    AttnPlan l, t;
    MlpPlan mlp;
};
// in an Euler rollout on view `r`, the last layer's (folded, row-owner) MLP launch writes the next step's token embedding
static bool embed_tail_runs(const Run& r) { return r.fold_ready && mlp_uses_rows(r.c, r.N) && r.c->opt_mlp_tail && r.embase_p; }
// last: the trunk's last layer, without a residual-stream trace: its folded MLP launch may run the FinalLayer as its tail (then h is
// NOT written), and with embed_next the next step's embedding; trace: the layer's MLP launch records phase stamps
static LayerPlan layer_plan(const Run& r, const AxisMap& axL, const AxisMap& axT, bool last, bool embed_next, bool trace) {
    const mdgen_ctx* c = r.c;
    LayerPlan p;
    const MlpRowsForm rows = !r.fold_ready                   ? MlpRowsForm::Plain
                             : !(last && c->opt_mlp_tail)    ? MlpRowsForm::Fold
                             : embed_next                    ? MlpRowsForm::FoldFinalEmbed
                                                             : MlpRowsForm::FoldFinal;
    // residue axis on the tiled-attention path (L > 8): its out-projection may run inside the temporal q / k / v kernel
    const bool fuse_lt = c->opt_fuse_proj_qkv && r.L > 8 && r.T > 8;
    p.l = attn_plan(c, Pos::ResL, axL, r.N, false, fuse_lt ? ProjAt::NextQkv : ProjAt::Own);
    // the temporal out-projection inside the panel MLP kernel, where that kernel runs
    const bool fuse = c->opt_fuse_proj == 3 && !mlp_uses_rows(c, r.N);
    p.t = attn_plan(c, Pos::TimeT, axT, r.N, p.l.proj == ProjAt::NextQkv, fuse ? ProjAt::Mlp : ProjAt::Own);
    p.mlp = mlp_plan(c, true, r.N, p.t.proj == ProjAt::Mlp, rows, r.concurrent, r.split_cap, trace);
    return p;
}

// An out-projection + gated residual that another sub-layer's kernel runs in its prologue (attention output rows: r.obufp)
struct OutProj {
    const bf16x8* w;
    const float* bias;
    int gate_chunk;
};

// pre: the previous sub-layer's out-projection (pl.qkv == QkvForm::PreProj only)
static int attn_sublayer(const Run& r, const AttnPlan& pl, const MhaW& m, const Rows& rw, const OutProj& pre) {
    if (int e = check_launch_rows(rw.nrows)) return e;
    const AxisMap& ax = rw.ax;
    const MaskMap& mk = rw.mk;
    const int gate = rw.gate();
    QkvParams q{};
    q.h = rw.h;
    q.nrows = rw.nrows;
    q.ax = ax;
    q.mm = rw.mm;
    q.shift_chunk = rw.chunk0;
    q.scale_chunk = rw.chunk0 + 1;
    q.wq = m.wq;
    q.wk = m.wk;
    q.bq = m.bq;
    q.bk = m.bk;
    q.rope = r.c->rope;
    q.qf = r.qfp;
    q.kf = r.kfp;
    q.vf = r.vfp;
    q.qkv_small = (__bf16*)r.qfp;
    const int ppanel = pl.qkv == QkvForm::Panel8SplitHalf ? 32 : kPanel;   // positions per workgroup (pair)
    q.panels_per_seq = (ax.len + ppanel - 1) / ppanel;
    ProjParams p{};
    p.h = rw.h;
    p.nrows = rw.nrows;
    p.mm = rw.mm;
    p.gate_chunk = gate;
    p.gated = 1;
    p.w = m.wo;
    p.bias = m.bo;
    p.a_bf16 = r.obufp;
    switch (pl.path) {
    case AttnPath::Quad:
        // L == 4: the 5-key attention runs inside the QKV kernel (quad-local), which writes the attention output
        q.wv = m.wv_small;
        q.bv = m.bv_small;
        q.bias_k = m.bias_k;
        q.bias_v = m.bias_v;
        q.l4tab = m.l4tab;
        q.mk = mk;
        q.obuf = r.obufp;
        if (pl.proj == ProjAt::Attention) {
            q.h_rw = rw.h;
            q.wo = m.wo;
            q.bo = m.bo;
            q.gate_chunk = gate;
        }
        if (int e = launch(r, tag(pl.pos, pl.a4), [&] { launch_ln_qkv_attn4(q, pl.a4, r.s); })) return e;
        break;
    case AttnPath::Micro:
        q.wv = m.wv_small;
        q.bv = m.bv_small;
        if (int e = launch(r, tag(pl.pos, pl.qkv), [&] { launch_ln_qkv(q, pl.qkv, r.s); })) return e;
        p.a_bf16 = nullptr;
        p.qkv_small = q.qkv_small;
        p.ax = ax;
        p.mk = mk;
        p.bias_k = m.bias_k;
        p.bias_v = m.bias_v;
        p.rope = r.c->rope;
        return launch(r, tag_proj(pl.pos), [&] { launch_proj(p, ProjMode::MicroAttn, r.s); });
    case AttnPath::Tiled: {
        q.wv = m.wv_flash;
        q.bv = m.bv_flash;
        q.bias_k = m.bias_k;   // written into key slot `len` of the K / V^T fragments by the sequence's last panel
        q.bias_v = m.bias_v;
        q.mk = mk;   // key-validity words for the attention kernel, in the slack behind the V^T fragments
        q.vmask = (uint32_t*)(q.vf + flash_vmask_offset(ax.nseq, ax.ntile()));
        q.vmask_stride = flash_vmask_stride(ax.ntile());
        if (pl.qkv == QkvForm::PreProj) {
            // the PREVIOUS sub-layer's out-projection + gated residual runs in this kernel's panels first (option fuse_proj_qkv):
            // its rows then come back from L2 for the LayerNorm instead of from HBM in a launch of their own
            q.obuf = r.obufp;
            q.wo = pre.w;
            q.bo = pre.bias;
            q.gate_chunk = pre.gate_chunk;
            q.h_rw = rw.h;
        }
        if (int e = launch(r, tag(pl.pos, pl.qkv), [&] { launch_ln_qkv(q, pl.qkv, r.s); })) return e;
        FlashParams f{};
        f.ax = ax;
        f.mk = mk;
        f.qf = q.qf;
        f.kf = q.kf;
        f.vf = q.vf;
        f.bias_k = m.bias_k;
        f.bias_v = m.bias_v;
        f.rope = r.c->rope;
        f.obuf = r.obufp;
        f.force_robust = r.c->opt_attn_path;
        f.rotate = r.c->opt_flash_rotate;
        f.vmask = q.vmask;
        f.vmask_stride = q.vmask_stride;
        if (pl.flash_proj) {   // attention of all heads + out-projection + gated residual in one launch
            FlashProjParams fp{};
            fp.f = f;
            fp.h = rw.h;
            fp.mm = rw.mm;
            fp.gate_chunk = gate;
            fp.wo = m.wo;
            fp.bo = m.bo;
            return launch(r, tag(pl.pos, pl.fp), [&] { launch_flash_proj(fp, pl.fp, r.s); });
        }
        if (int e = launch(r, tag_flash(pl.pos), [&] { launch_flash(f, r.s); })) return e;
        break;
    }
    }
    if (pl.proj != ProjAt::Own) return 0;
    return launch(r, tag_proj(pl.pos), [&] { launch_proj(p, ProjMode::Plain, r.s); });
}

// Operands of the forms only a trunk MLP launch takes
struct MlpTrunk {
    long fold_sl;                // index step * nl + layer of the launch's folded stream / b2'
    const FinalParams* fin;      // the FinalLayer (FoldFinal, FoldFinalEmbed)
    int next_step;               // the step whose token embedding the launch writes (FoldFinalEmbed)
    unsigned long long* trace;   // phase stamps of this launch, or null (mdgen_profile_phase_trace)
    long trace_cap;
};
// pre: the temporal sub-layer's out-projection (panel forms Pre* only); tk: null for the IPA stack
static int mlp_sublayer(const Run& r, const MlpPlan& pl, const FfnW& f, const Rows& rw, const OutProj& pre, const MlpTrunk* tk) {
    if (int e = check_launch_rows(rw.nrows)) return e;
    if (pl.use_rows) {
        MlpRowsParams q{};
        q.h = rw.h;
        q.nrows = rw.nrows;
        q.mm = rw.mm;
        q.shift_chunk = rw.chunk0;
        q.scale_chunk = rw.chunk0 + 1;
        q.gate_chunk = rw.chunk0 + 2;
        q.wstream = (const unsigned char*)f.wstream;
        q.b1 = f.b1;
        q.b2 = f.b2;
        if (pl.rows != MlpRowsForm::Plain) {
            q.wstream = r.fold_streams + (size_t)tk->fold_sl * kFoldStreamBytes;
            q.b2g = r.fold_b2g + (size_t)tk->fold_sl * kC;
        }
        if (pl.rows == MlpRowsForm::FoldFinal || pl.rows == MlpRowsForm::FoldFinalEmbed) {
            const FinalParams* tail = tk->fin;
            q.tail_w = r.c->wfin_k;
            q.tail_b = tail->bias;
            q.tail_mod = tail->mm.mod;
            q.tail_D = tail->D;
            q.tail_euler = tail->euler;
            q.tail_dt = tail->dt;
            q.tail_x = tail->x;
            q.tail_out = tail->out;
        }
        if (pl.rows == MlpRowsForm::FoldFinalEmbed) {   // ... and the next step's token embedding
            q.emb_wl_hi = r.c->wl_hi;
            q.emb_wl_lo = r.c->wl_lo;
            q.emb_wc_hi = r.c->wc_hi;
            q.emb_wc_lo = r.c->wc_lo;
            q.emb_base = r.embase_p + (long)tk->next_step * r.embase_step_stride;
            q.emb_mdelta = r.c->mask_delta;
            q.emb_xcond = r.x_cond;
            q.emb_cmask = r.x_cond_mask;
            q.emb_T = r.T;
            q.emb_L = r.L;
        }
        if (tk && tk->trace) {
            q.trace = tk->trace;
            q.trace_cap = tk->trace_cap;
        }
        return launch(r, tag(pl.trunk, pl.rows), [&] { launch_mlp_rows(q, pl.rows, r.s); });
    }
    MlpParams p{};
    const bool fused = pl.panel == MlpPanelForm::PreW4 || pl.panel == MlpPanelForm::PreW8 || pl.panel == MlpPanelForm::PreW8Split;
    if (fused) {   // the temporal out-projection runs in the panel kernel's prologue
        p.o = r.obufp;
        p.wo = pre.w;
        p.bo = pre.bias;
        p.gate_chunk_o = pre.gate_chunk;
    }
    p.h = rw.h;
    p.nrows = rw.nrows;
    p.mm = rw.mm;
    p.shift_chunk = rw.chunk0;
    p.scale_chunk = rw.chunk0 + 1;
    p.gate_chunk = rw.chunk0 + 2;
    p.w1 = f.w1;
    p.w2 = f.w2;
    p.b1 = f.b1;
    p.b2 = f.b2;
    if (tk && tk->trace) {
        p.trace = tk->trace;
        p.trace_cap = tk->trace_cap;
    }
    if (pl.panel == MlpPanelForm::W8Split || pl.panel == MlpPanelForm::PreW8Split) {
        ++r.c->n_split_launches;
        p.part = r.split_part;
        p.hupd = r.split_hupd;
        p.counters = r.split_counters;
    }
    return launch(r, tag(pl.trunk, pl.panel), [&] { launch_mlp(p, pl.panel, r.s); });
}

// IPA stack for all prepared steps at once (latent_model.py:175-210): tokens (step, b, l).
static int ipa_stack(const Run& r, float* hbuf, const float* rel7, const float* w7, const float* b7, const float* rot,
                     const float* trans) {
    mdgen_ctx* c = r.c;
    const int G = r.S * r.B;
    if (int e = launch(r, nullptr, [&] { launch_ipa_init(c->aa_emb, r.aatype, rel7, w7, b7, hbuf, G, r.B, r.L, r.s); })) return e;
    for (int i = 0; i < c->nl; ++i) {
        const IpaW& w = c->ipa[i];
        const IpaSites st = ipa_sites(r, i, hbuf, nullptr);
        if (c->opt_precision == 32) {   // ---- fp32 operands: ipa_norm -> four projections -> point attention -> linear_out
            const F32Bufs fb = f32_bufs(r);
            const LinearForm f32 = LinearForm::F32;
            const IpaBlockOp o{fb.y, (float*)(r.ws + r.lay.ipa_proj), fb.feat, nullptr, nullptr, 0, {f32, f32, f32, f32}, f32};
            if (int e = ipa_block_fp32(r, w, hbuf, rot, trans, o)) return e;
            if (int e = attn_sublayer_fp32(r, w.mha_l, st.attn)) return e;
            if (int e = mlp_sublayer_fp32(r, w.ffn, st.mlp)) return e;
            continue;
        }
        LnLinearParams lp{};
        lp.h = hbuf;
        lp.nrows = r.Mp;
        lp.mm = mod_affine(w.gamma_beta);
        lp.w = w.wproj;
        lp.bias = w.bproj;
        lp.out = (float*)(r.ws + r.lay.ipa_proj);
        lp.nout = kIpaProj;
        if (int e = launch(r, "ipa.ln_linear", [&] { launch_ln_linear(lp, r.s); })) return e;
        IpaAttnParams ap{};
        ap.proj = lp.out;
        ap.rot = rot;
        ap.trans = trans;
        ap.mask_bl = mask_ipa(r).mask;
        ap.head_w = w.head_w;
        ap.feat = (__bf16*)(r.ws + r.lay.ipa_feat);
        ap.ngroups = G;
        ap.B = r.B;
        ap.L = r.L;
        if (int e = launch(r, "ipa.point_attn", [&] { launch_ipa_attn(ap, r.s); })) return e;
        ProjParams pp{};
        pp.h = hbuf;
        pp.nrows = r.Mp;
        pp.mm = st.attn.mm;
        pp.gated = 0;
        pp.w = w.wout;
        pp.bias = w.bout;
        pp.a_bf16 = ap.feat;
        if (int e = launch(r, "ipa.linear_out", [&] { launch_proj(pp, ProjMode::Linear, r.s); })) return e;
        const OutProj none{};
        if (int e = attn_sublayer(r, attn_plan(c, Pos::Ipa, st.attn.ax, r.Mp, false, ProjAt::Own), w.mha_l, st.attn, none)) return e;
        const MlpPlan mp = mlp_plan(c, false, r.Mp, false, MlpRowsForm::Plain, r.concurrent, r.split_cap, false);
        if (int e = mlp_sublayer(r, mp, w.ffn, st.mlp, none, nullptr)) return e;
    }
    return 0;
}

// Step-invariant work: adaLN table for every prepared time row, compact mask, IPA table.
// t values: t_dev (device, [S][B]) when non-null, else t_host[step] baked into the launch.
// view_rows: token rows of the call's largest trunk launch (a sub-batch view)
static int prepare(Run& r, const float* t_dev, const float* t_host, long view_rows) {
    mdgen_ctx* c = r.c;
    float* silu = (float*)(r.ws + r.lay.silu_t);
    const int R = r.t_shared ? r.S : r.S * r.B;
    // K/V fragment regions: key slots past a sequence's end are never written by k_ln_qkv but are read (and
    // masked to P = 0) by k_flash, so they must hold FINITE values: zero them once per call.
    HIPCHK(hipMemsetAsync(r.ws + r.lay.kf, 0, r.lay.obuf - r.lay.kf, r.s));
    if (t_dev) {
        if (r.t_shared && r.B > 1) return fail(-2, "device t rows require t_shared == 0 or B == 1");
        if (int e = launch(r, nullptr, [&] { launch_temb(t_dev, R, c->d.time_multiplier, c->t_w0, c->t_b0, c->t_w2, c->t_b2, silu, r.s); })) return e;
    } else {
        // the (tiny) host time grid travels as kernel arguments: capturable, no host buffer lifetime issue
        float* tg = (float*)(r.ws + r.lay.tgrid);
        if (int e = launch(r, nullptr, [&] { launch_write_floats(t_host, r.S, tg, r.s); })) return e;
        if (int e = launch(r, nullptr, [&] { launch_temb(tg, r.S, c->d.time_multiplier, c->t_w0, c->t_b0, c->t_w2, c->t_b2, silu, r.s); })) return e;
    }
    if (int e = launch(r, "adaln_table", [&] { launch_adaln(silu, R, c->ada_w, c->ada_b, c->modrow, r.mod(), r.s); })) return e;
    // (view_rows, not N: see fold_on.  r.S may be below the S the workspace was carved for: ode.inc)
    r.fold_ready = r.fold_streams && fold_on(c, view_rows, r.t_shared, r.S);
    if (r.fold_ready) {   // the steps' MLP gates folded into per-(step, layer) fc2 streams (t_shared: R == S rows)
        int goff[8];
        const float *w2[8], *b2[8];
        const bf16x8* base[8];
        for (int i = 0; i < c->nl; ++i) {
            goff[i] = c->trunk_off(i) + 8 * kC;
            w2[i] = c->trunk[i].ffn.w2f;
            b2[i] = c->trunk[i].ffn.b2;
            base[i] = c->trunk[i].ffn.wstream;
        }
        if (int e = launch(r, "fold_pack", [&] { launch_pack_fold(r.mod(), r.mod_step_stride, r.S, c->nl, goff, w2, b2, base, c->mlp_tab, (bf16x8*)r.fold_streams, r.fold_b2g, r.s); })) return e;
    }
    // mask_bl[b][l] = mask[b][0][l]  (latent_model.py:246 passes mask[:,0])
    HIPCHK(hipMemcpy2DAsync(r.ws + r.lay.mask_bl, (size_t)r.L * 4, r.mask, (size_t)r.T * r.L * 4, (size_t)r.L * 4, r.B,
                            hipMemcpyDeviceToDevice, r.s));
    float* ipa_out = (float*)(r.ws + r.lay.ipa_out);
    if (!c->d.tps_condition) {
        if (int e = ipa_stack(r, ipa_out, nullptr, nullptr, nullptr, r.start_rot, r.start_trans)) return e;
    } else {
        if (!r.end_rot || !r.end_trans) return fail(-2, "tps_condition requires end frames");
        float* rel = (float*)(r.ws + r.lay.rel7);
        const long BL = (long)r.B * r.L;
        // x_f = (start^-1 o end).to_tensor_7(), x_r = (end^-1 o start).to_tensor_7()   (latent_model.py:194-195)
        // The quaternion's SIGN is whatever torch.linalg.eigh returns in the reference (rigid_utils.py:191-210) and it does
        // reach a Linear: a caller that needs the reference's exact inputs passes its own to_tensor_7() outputs (rel7_in);
        // otherwise the library computes them with the sign fixed to w >= 0.
        if (r.rel7_in) {
            HIPCHK(hipMemcpyAsync(rel, r.rel7_in, (size_t)2 * BL * 7 * 4, hipMemcpyDeviceToDevice, r.s));
        } else {
            if (int e = launch(r, nullptr, [&] {
                    launch_rel7(r.start_rot, r.start_trans, r.end_rot, r.end_trans, rel, BL, r.s);
                    launch_rel7(r.end_rot, r.end_trans, r.start_rot, r.start_trans, rel + BL * 7, BL, r.s);
                }))
                return e;
        }
        float* h2 = (float*)(r.ws + r.lay.h_ipa);
        // x_r stream runs on the start frames, x_f stream on the end frames (latent_model.py:203-205)
        if (int e = ipa_stack(r, ipa_out, rel + BL * 7, c->wr7, c->br7, r.start_rot, r.start_trans)) return e;
        if (int e = ipa_stack(r, h2, rel, c->wf7, c->bf7, r.end_rot, r.end_trans)) return e;
        if (int e = launch(r, nullptr, [&] { launch_add_inplace(ipa_out, h2, r.Mp * kC, r.s); })) return e;
    }
    if (r.fold_ready && embed_base_on(c, view_rows, r.t_shared, r.S) && !r.no_embed_tail) {
        // steps 1 .. S-1 take their token embedding from the previous step's last MLP launch (rows_embed_tail): the part of it that does
        // not depend on x, per (step, b, l)
        float* eb = (float*)(r.ws + r.lay.embase);
        if (int e = launch(r, "embed_base", [&] { launch_embed_base(c->bl, c->bc, c->mask_emb, c->d.abs_pos_emb ? c->pos_embed : nullptr, ipa_out, r.S, r.B * r.L, r.L, eb, r.s); })) return e;
        r.embase_p = eb;
    }
    return 0;
}

// the token embedding of x (B, T, L, D) into h (latent_model.py:233-246) with the context's weights and its abs_pos_emb; ipa_out: the
// IPA table's rows [B*L][384] of the step
static EmbedParams embed_params(const mdgen_ctx* c, const mdgen_shape& sh, const float* x, const float* x_cond, const int64_t* x_cond_mask,
                                const float* ipa_out, float* h) {
    EmbedParams e{};
    e.x = x; e.x_cond = x_cond; e.x_cond_mask = x_cond_mask;
    e.wl = c->wl; e.bl = c->bl; e.wc = c->wc; e.bc = c->bc; e.mask_emb = c->mask_emb;
    e.wl_pack = c->wl_pack; e.wc_pack = c->wc_pack;
    e.pos_embed = c->d.abs_pos_emb ? c->pos_embed : nullptr;
    e.ipa_out = ipa_out; e.h = h; e.N = (long)sh.B * sh.T * sh.L; e.T = sh.T; e.L = sh.L; e.D = c->D;
    return e;
}
// ... of a made run (a view: its own B), into r.h()
static EmbedParams embed_op(const Run& r, const float* x, const float* ipa_out) {
    return embed_params(r.c, mdgen_shape{r.B, r.T, r.L}, x, r.x_cond, r.x_cond_mask, ipa_out, r.h());
}

// One network evaluation at prepared step `step`: x -> velocity (out) or Euler update of x in place.
// euler: the call runs the prepared steps 0 .. S-1 in order on this view (euler_steps).  Where embed_tail_runs(r), step i's last MLP
// launch then writes step i + 1's token embedding into h, and step i + 1 launches no k_embed.
static int denoise_step(const Run& r, int step, float* x, float* out, int euler, float dt, float* trace_h) {
    mdgen_ctx* c = r.c;
    const bool embed_tail = euler && embed_tail_runs(r);
    float* h = r.h();
    const EmbedParams e = embed_op(r, x, r.ipa_out_p + (long)step * r.ipa_step_stride);
    if (r.rk) {
        if (int er = launch(r, "rk_embed", [&] { launch_rk_embed(e, *r.rk, r.s); })) return er;
    } else if (r.sde) {
        if (int er = launch(r, "sde_embed", [&] { launch_sde_embed(e, *r.sde, r.s); })) return er;
    } else if (!(embed_tail && step > 0)) {
        if (int er = launch(r, "embed", [&] { launch_embed(e, r.s); })) return er;
    }
    const size_t hbytes = (size_t)r.N * kC * 4;
    if (trace_h) HIPCHK(hipMemcpyAsync(trace_h, h, hbytes, hipMemcpyDeviceToDevice, r.s));
    if (c->opt_precision == 32) {   // ---- fp32 operands (k_fp32.hip): same dataflow, one kernel per reference op group
        for (int i = 0; i < c->nl; ++i) {
            const TrunkW& w = c->trunk[i];
            const TrunkSites st = trunk_sites(r, i, step, nullptr);
            if (int er = attn_sublayer_fp32(r, w.mha_l, st.l)) return er;
            if (int er = attn_sublayer_fp32(r, w.mha_t, st.t)) return er;
            if (int er = mlp_sublayer_fp32(r, w.ffn, st.mlp)) return er;
            if (trace_h) HIPCHK(hipMemcpyAsync(trace_h + (size_t)(i + 1) * r.N * kC, h, hbytes, hipMemcpyDeviceToDevice, r.s));
        }
        const F32Bufs fb = f32_bufs(r);
        launch32_ln_mod(h, r.N, mod_final(r, step), 0, 1, 0, 1e-6f, fb.y, r.s, nullptr, false);
        LinearParams fin = lin_op(fb.y, kC, c->f32(c->slot.fin.w), kC, c->f32(c->slot.fin.b), r.N, r.D, kC, euler ? x : out, r.D);
        fin.mode = euler ? kLinEuler : kLinStore;
        fin.scalar = dt;
        launch32_linear(fin, r.s);
        LAUNCHCHK();
        return 0;
    }
    FinalParams f{};
    f.h = h;
    f.nrows = r.N;
    f.mm = mod_final(r, step);
    f.shift_chunk = 0;
    f.scale_chunk = 1;
    f.w = c->wfin;
    f.bias = c->bfin;
    f.D = r.D;
    f.euler = euler;
    f.dt = dt;
    f.x = x;
    f.out = out;
    // the one-shot phase trace (mdgen_profile_phase_trace) goes to the first trunk MLP launch after it was armed: taken here
    MlpTrunk tk{0, &f, step + 1, c->phase_trace, c->phase_trace_cap};
    c->phase_trace = nullptr;
    bool final_done = false;
    for (int i = 0; i < c->nl; ++i) {
        const TrunkW& w = c->trunk[i];
        const TrunkSites st = trunk_sites(r, i, step, nullptr);
        const LayerPlan pl = layer_plan(r, st.l.ax, st.t.ax, i == c->nl - 1 && !trace_h, embed_tail && step + 1 < r.S, tk.trace != nullptr);
        const OutProj proj_l{w.mha_l.wo, w.mha_l.bo, st.l.gate()}, proj_t{w.mha_t.wo, w.mha_t.bo, st.t.gate()};
        if (int er = attn_sublayer(r, pl.l, w.mha_l, st.l, OutProj{})) return er;
        if (int er = attn_sublayer(r, pl.t, w.mha_t, st.t, proj_l)) return er;
        tk.fold_sl = (long)step * c->nl + i;
        if (int er = mlp_sublayer(r, pl.mlp, w.ffn, st.mlp, proj_t, &tk)) return er;
        tk.trace = nullptr;
        final_done = pl.mlp.use_rows && (pl.mlp.rows == MlpRowsForm::FoldFinal || pl.mlp.rows == MlpRowsForm::FoldFinalEmbed);
        if (trace_h) HIPCHK(hipMemcpyAsync(trace_h + (size_t)(i + 1) * r.N * kC, h, hbytes, hipMemcpyDeviceToDevice, r.s));
    }
    if (final_done) return 0;
    return launch(r, "final_euler", [&] { launch_final(f, r.s); });
}

// reads_f32: the call reads the fp32 weight copies (the sampler with option precision = 32: f32_path(c); the training step always)
static bool f32_path(const mdgen_ctx* c) { return c && c->opt_precision == 32; }
static int make_run(Run* r, mdgen_ctx* c, const mdgen_shape* sh, int S, int t_shared, bool reads_f32, void* ws, size_t ws_bytes,
                    void* stream) {
    if (int e = check_shape(c, sh, S)) return e;
    if (!c->finalized) return fail(-6, "context not finalized (mdgen_ctx_finalize)");
    if (!ws) return fail(-1, "null workspace");
    if (int e = mdgen_workspace_layout(c, sh, S, t_shared, &r->lay)) return e;
    if (ws_bytes < r->lay.total_bytes)
        return fail(-7, "workspace too small: %zu < %zu bytes", ws_bytes, r->lay.total_bytes);
    if (((uintptr_t)ws & 255) != 0) return fail(-7, "workspace must be 256-byte aligned");
    if (reads_f32 && !c->opt_keep_fp32) return fail(-6, "precision 32 requires option keep_fp32_weights");
    if (reads_f32)
        if (int e = check_f32_weights(c)) return e;
    r->c = c;
    r->B = sh->B;
    r->T = sh->T;
    r->L = sh->L;
    r->D = c->D;
    r->S = S;
    r->N = (long)sh->B * sh->T * sh->L;
    r->Mp = (long)S * sh->B * sh->L;
    r->t_shared = t_shared;
    r->mod_step_stride = t_shared ? c->modrow : (long)sh->B * c->modrow;
    r->mod_group_stride = t_shared ? 0 : c->modrow;
    r->ws = (unsigned char*)ws;
    r->s = (hipStream_t)stream;
    r->hp = (float*)(r->ws + r->lay.h);
    r->qfp = r->ws + r->lay.qf;
    r->kfp = r->ws + r->lay.kf;
    r->vfp = r->ws + r->lay.vf;
    r->obufp = (__bf16*)(r->ws + r->lay.obuf);
    r->modp = (float*)(r->ws + r->lay.mod);
    r->ipa_out_p = (const float*)(r->ws + r->lay.ipa_out);
    r->ipa_step_stride = (long)sh->B * sh->L * kC;
    {
        const long maxrows = r->N > r->Mp ? r->N : r->Mp;
        r->split_cap = split_panels(c, maxrows);
        r->split_counters = (unsigned*)(r->ws + r->lay.split);
        r->split_part = (float*)(r->ws + r->lay.split + kSplitCounterBytes);
        r->split_hupd = r->split_part + (size_t)r->split_cap * kMlpSplit * kPanel * kC;
        // the counters must be zero when a launch starts (every launch leaves them so); the caller's workspace holds anything.
        // Eagerly on the call's stream, ahead of the (possibly replayed) graph.
        HIPCHK(hipMemsetAsync(r->split_counters, 0, kSplitCounterBytes, r->s));
    }
    r->fold_streams = nullptr;
    r->fold_b2g = nullptr;
    r->fold_ready = false;
    r->embase_p = nullptr;
    r->embase_step_stride = (long)sh->B * sh->L * kC;
    r->no_embed_tail = false;
    r->rk = nullptr;
    r->sde = nullptr;
    r->concurrent = false;
    if (fold_on(c, r->N, t_shared, S)) {
        r->fold_streams = r->ws + r->lay.fold;
        r->fold_b2g = (float*)(r->fold_streams + (size_t)S * c->nl * kFoldStreamBytes);
    }
    return 0;
}

// The conditioning of a call (include/mdgen_amd.h mdgen_cond): refused when the struct or a required field is null ...
static_assert(sizeof(mdgen_cond) == 9 * sizeof(void*), "mdgen_cond is nine pointers (GraphKey::add_struct, _lib.py Cond)");
static int check_cond(const mdgen_cond* cd) {
    if (!cd) return fail(-1, "null conditioning (mdgen_cond)");
    if (!cd->mask || !cd->start_rot || !cd->start_trans || !cd->x_cond || !cd->x_cond_mask || !cd->aatype)
        return fail(-1, "null tensor argument");
    return 0;
}
// ... and the one place that hands it to a made run
static void bind_cond(Run& r, const mdgen_cond& cd) {
    r.mask = cd.mask;
    r.start_rot = cd.start_rot;
    r.start_trans = cd.start_trans;
    r.end_rot = cd.end_rot;
    r.end_trans = cd.end_trans;
    r.rel7_in = cd.rel7;
    r.x_cond = cd.x_cond;
    r.x_cond_mask = cd.x_cond_mask;
    r.aatype = cd.aatype;
}

// mdgen_denoiser_forward on a made run: the batch's views one after the other on the caller's stream
static int forward_body(Run& r, const float* x, const float* t, float* out, float* trace_h, float* trace_ipa) {
    const int nv = r.c->opt_precision == 32 ? 1 : plan_views(r.B, r.T, r.L, 1);
    if (nv == 0) return fail(-2, "sample too large for one launch");
    if (int e = prepare(r, t, nullptr, largest_view_rows(r, nv))) return e;
    if (trace_ipa)
        HIPCHK(hipMemcpyAsync(trace_ipa, r.ws + r.lay.ipa_out, (size_t)r.B * r.L * kC * 4, hipMemcpyDeviceToDevice, r.s));
    if (nv > 1 && trace_h) return fail(-2, "trace_h is not available when the batch needs more than one launch view");
    return for_each_view(r, nv, 1, [&](const Run& v, int b0) {
        const long o = (long)b0 * r.T * r.L * r.D;
        return denoise_step(v, 0, const_cast<float*>(x) + o, out + o, 0, 0.f, trace_h);
    });
}

extern "C" int32_t mdgen_denoiser_forward(mdgen_ctx* c, const mdgen_shape* sh, const float* x, const float* t,
                                          const mdgen_cond* cond, float* out, float* trace_h, float* trace_ipa, void* ws,
                                          size_t ws_bytes, void* stream) {
    if (!x || !t || !out) return fail(-1, "null tensor argument");
    if (int e = check_cond(cond)) return e;
    Run r{};
    const int t_shared = (sh && sh->B == 1) ? 1 : 0;
    if (int e = make_run(&r, c, sh, 1, t_shared, f32_path(c), ws, ws_bytes, stream)) return e;
    bind_cond(r, *cond);
    return forward_body(r, x, t, out, trace_h, trace_ipa);
}

// torch.linspace(0, 1, n) in fp32 (ATen RangeFactories: symmetric evaluation around the midpoint)
static void linspace01(int n, std::vector<float>* out) {
    out->resize(n);
    const float step = 1.0f / (float)(n - 1);
    const int half = n / 2;
    for (int i = 0; i < n; ++i) (*out)[i] = i < half ? 0.0f + step * (float)i : 1.0f - step * (float)(n - 1 - i);
}

// Number of concurrent sub-batch streams for the Euler rollout (option "streams", default 2; 1 disables).
// Sub-batch streams pay when every piece still fills the chip by itself (cfg-2: 2 x 500 panels, +9 ... 12 %); pieces of
// fewer than 256 64-row panels leave CUs idle in BOTH streams (TPS shard B32 T100: 2 x 100 panels 68.3k frames/s, one stream
// 73.4k, profiles/r04_experiments.txt): the batch is then cut into fewer pieces, down to one.
static int n_streams(const Run& r) {
    int n = r.c->opt_streams;
    if (n > r.B) n = r.B;
    const long fill = (long)r.c->ncu * kPanel;
    if (r.c->opt_streams_auto && (long)n * fill > r.N) n = (int)(r.N / fill);
    if (n < 2 || r.c->prof_on || r.N < 4096 || r.c->opt_precision == 32) return 1;
    return n;
}

static int euler_steps(const Run& v, const std::vector<float>& tg, float* x) {
    for (int i = 0; i < v.S; ++i)
        if (int e = denoise_step(v, i, x, nullptr, 1, tg[i + 1] - tg[i], nullptr)) return e;
    return 0;
}

static int euler_body(const Run& r_in, const std::vector<float>& tg, float* x) {
    Run r = r_in;
    mdgen_ctx* c = r.c;
    const int ns = n_streams(r);
    // >= ns views; more when a view would exceed kMaxViewTokens (the fp32 kernels index with 64 bits: one view)
    const int nv = c->opt_precision == 32 ? 1 : plan_views(r.B, r.T, r.L, ns);
    if (nv == 0) return fail(-2, "sample too large for one launch");
    if (int e = prepare(r, nullptr, tg.data(), largest_view_rows(r, nv))) return e;
    // contiguous sub-batch views, view i on stream i % ns (fork after the shared preparation, join at the end)
    if (ns > 1) HIPCHK(hipEventRecord(c->ev_fork, r.s));
    for (int i = 1; i < ns; ++i) HIPCHK(hipStreamWaitEvent(c->side[i - 1], c->ev_fork, 0));
    if (int e = for_each_view(r, nv, ns, [&](const Run& v, int b0) { return euler_steps(v, tg, x + (long)b0 * r.T * r.L * r.D); })) return e;
    for (int i = 1; i < ns; ++i) {
        HIPCHK(hipEventRecord(c->ev_join[i - 1], c->side[i - 1]));
        HIPCHK(hipStreamWaitEvent(r.s, c->ev_join[i - 1], 0));
    }
    return 0;
}

// The part of a graph's cache key that the run-time options give: every option that changes what a captured call launches,
// four bits each (mdgen_ctx_set_option keeps every value below 16; precision is 16 or 32)
static uint64_t graph_option_key(const mdgen_ctx* c) {
    const int v[] = {c->opt_precision == 32, c->opt_attn_path, c->opt_residue_l4, c->opt_mlp_path, c->opt_fuse_proj,
                     c->opt_fuse_proj_qkv, c->opt_flash_proj, c->opt_panel_waves, c->opt_flash_rotate, c->opt_flash_proj_form,
                     c->opt_small_split, c->opt_mlp_fold, c->opt_mlp_tail};
    uint64_t k = 0;
    for (int x : v) k = k << 4 | (uint64_t)x;
    return k;
}

// A graph's cache key: every value and every pointer that the captured body bakes into the graph.  A body reads its pointers from
// structs (mdgen_cond, mdgen_residue_tables); those structs go into the key whole, word by word -- never a chosen subset of them.
struct GraphKey {
    std::vector<uint64_t> v;
    GraphKey& add(uint64_t x) { v.push_back(x); return *this; }
    GraphKey& ptr(const void* p) { return add((uint64_t)(uintptr_t)p); }
    template <class T> GraphKey& add_struct(const T& t) {
        static_assert(sizeof(T) % sizeof(uint64_t) == 0 && std::is_trivially_copyable<T>::value, "a struct of pointer-sized words");
        const size_t n = v.size();
        v.resize(n + sizeof(T) / sizeof(uint64_t));
        std::memcpy(&v[n], &t, sizeof(T));
        return *this;
    }
};
// The part every capturing entry point shares: its tag, the shape, the conditioning it bound, the workspace and the options.  The entry
// point adds its scalar arguments, its state / output pointers, its residue tables and, where its body forks, n_streams(r).
static GraphKey graph_key(uint64_t tag, const Run& r, const mdgen_cond& cd) {
    GraphKey k;
    k.add(tag).add(r.B).add(r.T).add(r.L).add_struct(cd).ptr(r.ws).add(graph_option_key(r.c));
    return k;
}

// Replay the cached hipGraph for `key`, or capture `body` (which enqueues work on `s`, possibly forking onto the
// context's side streams and joining back) into a new one, cache it (LRU, 8 entries) and launch it.
static int replay_or_capture(mdgen_ctx* c, const std::vector<uint64_t>& key, hipStream_t s, const std::function<int()>& body) {
    if (!s) return fail(-8, "use_graph requires a non-default stream");
    for (size_t gi = 0; gi < c->graphs.size(); ++gi)
        if (c->graphs[gi].key == key) {
            if (gi + 1 != c->graphs.size()) {   // most recently used goes to the back (eviction takes the front)
                GraphEntry hit = c->graphs[gi];
                c->graphs.erase(c->graphs.begin() + gi);
                c->graphs.push_back(hit);
            }
            HIPCHK(hipGraphLaunch(c->graphs.back().exec, s));
            return 0;
        }
    GraphEntry ge;
    ge.key = key;
    HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    const int e = body();
    hipError_t ce = hipStreamEndCapture(s, &ge.graph);
    if (e) {
        if (ge.graph) (void)hipGraphDestroy(ge.graph);
        return e;
    }
    if (ce != hipSuccess) {
        if (ge.graph) (void)hipGraphDestroy(ge.graph);
        return fail((int)ce, "hipStreamEndCapture failed: %s", hipGetErrorString(ce));
    }
    {
        hipError_t ie = hipGraphInstantiate(&ge.exec, ge.graph, nullptr, nullptr, 0);
        if (ie != hipSuccess) {
            (void)hipGraphDestroy(ge.graph);
            return fail((int)ie, "hipGraphInstantiate failed: %s", hipGetErrorString(ie));
        }
    }
    if (c->graphs.size() >= 8) {
        (void)hipGraphExecDestroy(c->graphs.front().exec);
        (void)hipGraphDestroy(c->graphs.front().graph);
        c->graphs.erase(c->graphs.begin());
    }
    c->graphs.push_back(ge);
    HIPCHK(hipGraphLaunch(ge.exec, s));
    return 0;
}

// Test hook (host only): how many captured graphs the context holds (at most 8: replay_or_capture's LRU)
extern "C" int32_t mdgen_debug_graph_count(const mdgen_ctx* c, int32_t* count) {
    if (!c || !count) return fail(-1, "null argument");
    *count = (int32_t)c->graphs.size();
    return 0;
}

// The capture gate of every capturing entry point: `body` runs directly without use_graph and while profiling (see mdgen_profile_enable)
static int run_or_replay(const Run& r, int use_graph, const GraphKey& key, const std::function<int()>& body) {
    if (!use_graph || r.c->prof_on) return body();
    return replay_or_capture(r.c, key.v, r.s, body);
}

extern "C" int32_t mdgen_sample_euler(mdgen_ctx* c, const mdgen_shape* sh, int32_t S, float* x, const mdgen_cond* cond, void* ws,
                                      size_t ws_bytes, int32_t use_graph, void* stream) {
    if (!x) return fail(-1, "null tensor argument");
    if (int e = check_cond(cond)) return e;
    Run r{};
    if (int e = make_run(&r, c, sh, S, 1, f32_path(c), ws, ws_bytes, stream)) return e;
    bind_cond(r, *cond);
    std::vector<float> tg;
    linspace01(S + 1, &tg);   // integrators.py:88  th.linspace(t0, t1, num_steps)
    GraphKey key = graph_key(0, r, *cond);
    key.add(S).ptr(x).add(n_streams(r));
    return run_or_replay(r, use_graph, key, [&]() { return euler_body(r, tg, x); });
}

#include "ode.inc"
#include "sde.inc"
#include "drivers.inc"

// ---------------------------------------------------------------------------------------------
// dispatch plan (host only)
// ---------------------------------------------------------------------------------------------
// Which kernel classes a call of this shape launches, and how often: the entry points' own bodies (euler_body, forward_body,
// ode.inc dopri5_attempt) run in plan mode (g_dry) on a context that owns no device memory -- the same view loop, layer plans and
// launch sites as a real call.  mode 0: mdgen_sample_euler as the product runs it (sub-batch streams);
// 1: mdgen_denoiser_forward; 2: mdgen_sample_euler as mdgen_profile_enable sees it (one stream); 3: mdgen_denoiser_forward with trace_h;
// 4: one attempted step of mdgen_sample_dopri5; 5, 6, 7: one step of mdgen_sample_rk with method 1 (midpoint), 2 (heun3), 3 (rk4) (n_steps
// is ignored in modes 4 .. 7).  options: "name=value,..."
// (mdgen_ctx_set_option names).  ncu / xcd_round_robin: what mdgen_ctx_create would have found on the device.
// Output: {"streams": n, "prepare": {"<class>": launches, ...}, "views": [{"B": samples of the view, "classes": {...}}, ...]}
// and, mode 4, "integrator": {"ode_combine": 6, "ode_norm": 1}; modes 5 .. 7, "integrator": {"ode_rk_update": 1}.
static int plan_json(const DryPlan& plan, int B, int nv, int ns, bool integrator, char* buf, size_t buflen) {
    std::map<std::string, long> prep, integ;
    std::vector<std::map<std::string, long>> views(nv);
    for (const auto& k : plan.rec) {
        if (k.first >= nv) return fail(-7, "internal: %d views planned, view %d recorded", nv, k.first);
        ++(std::strncmp(k.second, "ode_", 4) == 0 ? integ : k.first < 0 ? prep : views[k.first])[k.second];
    }
    auto dump = [](const std::map<std::string, long>& agg) {
        std::string o = "{";
        bool first = true;
        for (const auto& kv : agg) {
            o += std::string(first ? "" : ", ") + "\"" + kv.first + "\": " + std::to_string(kv.second);
            first = false;
        }
        return o + "}";
    };
    std::string js = "{\"streams\": " + std::to_string(ns) + ", \"prepare\": " + dump(prep) + ", \"views\": [";
    for (int i = 0; i < nv; ++i)
        js += std::string(i ? ", " : "") + "{\"B\": " + std::to_string(B / nv + (i < B % nv ? 1 : 0)) + ", \"classes\": " + dump(views[i]) + "}";
    js += "]";
    if (integrator) js += ", \"integrator\": " + dump(integ);
    js += "}";
    if (js.size() + 1 > buflen) return fail(-7, "plan buffer too small");
    std::memcpy(buf, js.c_str(), js.size() + 1);
    return 0;
}

// the context of a plan-mode run: no device memory, no streams (plan mode never touches them)
static int dry_ctx(mdgen_ctx* c, int tps_condition, int num_layers, int ncu, int xcd_round_robin, bool prof_on, const char* options) {
    if (num_layers < 1 || num_layers > 8 || ncu < 1) return fail(-2, "num_layers in 1..8, ncu >= 1");
    c->nl = num_layers;
    c->D = tps_condition ? 28 : 21;
    c->d.num_layers = num_layers;
    c->d.latent_dim = c->D;
    c->d.tps_condition = tps_condition;
    c->d.abs_pos_emb = 0;
    c->modrow = (15 * c->nl + 2) * kC;
    c->trunk.resize(c->nl);
    c->ipa.resize(c->nl);
    c->finalized = true;
    c->ncu = ncu;
    c->xcd_round_robin = xcd_round_robin != 0;
    c->prof_on = prof_on;
    for (std::string rest = options ? options : ""; !rest.empty();) {
        const size_t comma = rest.find(',');
        const std::string kv = rest.substr(0, comma);
        rest = comma == std::string::npos ? "" : rest.substr(comma + 1);
        const size_t eq = kv.find('=');
        if (eq == std::string::npos) return fail(-2, "options: name=value[,name=value...]");
        if (int e = mdgen_ctx_set_option(c, kv.substr(0, eq).c_str(), std::atoi(kv.c_str() + eq + 1))) return e;
    }
    return 0;
}
static mdgen_cond fake_cond() {   // never dereferenced: plan mode launches nothing
    const float* fake = (const float*)4096;
    return {fake, fake, fake, fake, fake, nullptr, fake, (const int64_t*)fake, (const int64_t*)fake};
}
// A plan-mode call of S prepared time rows: its context, the launches it records while it lives, and its made run with a workspace
// and a conditioning that are never followed.
struct DryCall {
    mdgen_ctx ctx;
    DryPlan plan;
    Run r{};
    ~DryCall() { g_dry = nullptr; }
    int open(const mdgen_shape* sh, int S, int t_shared, int tps_condition, int num_layers, int ncu, int xcd_round_robin, bool prof_on,
             const char* options) {
        if (int e = dry_ctx(&ctx, tps_condition, num_layers, ncu, xcd_round_robin, prof_on, options)) return e;
        g_dry = &plan;
        if (int e = make_run(&r, &ctx, sh, S, t_shared, f32_path(&ctx), (void*)4096, (size_t)1 << 60, nullptr)) return e;
        bind_cond(r, fake_cond());
        return 0;
    }
};

extern "C" int32_t mdgen_debug_dispatch_plan(const mdgen_shape* sh, int32_t n_steps, int32_t mode, int32_t tps_condition,
                                             int32_t num_layers, int32_t ncu, int32_t xcd_round_robin, const char* options,
                                             char* buf, size_t buflen) {
    if (!sh || !buf || buflen < 64) return fail(-1, "null argument");
    if (mode < 0 || mode > 7)
        return fail(-2, "mode: 0 sample_euler, 1 forward, 2 sample_euler under the profiler, 3 forward with trace_h, 4 one dopri5 step, "
                        "5 / 6 / 7 one midpoint / heun3 / rk4 step");
    const bool fwd = mode == 1 || mode == 3;
    const bool rkm = mode >= 5;   // one step of mdgen_sample_rk, method mode - 4: its time rows
    const int S = mode == 4 ? ode::kStages : rkm ? rk_method(mode - 4)->stages : fwd ? 1 : n_steps;
    const int t_shared = fwd ? (sh->B == 1 ? 1 : 0) : 1;
    DryCall dry;
    if (int e = dry.open(sh, S, t_shared, tps_condition, num_layers, ncu, xcd_round_robin, mode == 2, options)) return e;
    Run& r = dry.r;
    float* fake = (float*)4096;   // never dereferenced: plan mode launches nothing
    const int ns = fwd || mode >= 4 ? 1 : n_streams(r);
    const int nv = plan_views(r.B, r.T, r.L, ns);
    if (mode == 4) {
        if (int e = dopri5_plan(r, nv)) return e;
    } else if (rkm) {
        if (int e = rk_dispatch_plan(r, nv, mode - 4)) return e;
    } else if (fwd) {
        if (int e = forward_body(r, fake, fake, fake, mode == 3 ? fake : nullptr, nullptr)) return e;
    } else {
        std::vector<float> tg;
        linspace01(S + 1, &tg);
        if (int e = euler_body(r, tg, fake)) return e;
    }
    return plan_json(dry.plan, r.B, nv, ns, mode >= 4, buf, buflen);
}

// mdgen_debug_dispatch_plan for ONE step of mdgen_sample_sde with `opts` (n_points is taken as 2): the same JSON, "integrator":
// {"ode_sde_update": 1}
extern "C" int32_t mdgen_debug_sde_dispatch_plan(const mdgen_shape* sh, const mdgen_sde_opts* opts, int32_t tps_condition,
                                                 int32_t num_layers, int32_t ncu, int32_t xcd_round_robin, const char* options,
                                                 char* buf, size_t buflen) {
    if (!sh || !opts || !buf || buflen < 64) return fail(-1, "null argument");
    mdgen_sde_opts o = *opts;
    o.n_points = 2;
    SdePlan pl;
    if (int e = sde_plan(o, &pl)) return e;
    DryCall dry;
    if (int e = dry.open(sh, (int)pl.rows.size(), 1, tps_condition, num_layers, ncu, xcd_round_robin, false, options)) return e;
    Run& r = dry.r;
    r.no_embed_tail = true;
    const int nv = plan_views(r.B, r.T, r.L, 1);
    if (nv == 0) return fail(-2, "sample too large for one launch");
    float* fake = (float*)4096;
    float* v[2] = {fake, fake};
    if (int e = sde_body(r, o, pl, nv, fake, v, SdeNoise{fake, 0, nullptr, 0})) return e;
    return plan_json(dry.plan, r.B, nv, 1, true, buf, buflen);
}

// ---------------------------------------------------------------------------------------------
// measurement
// ---------------------------------------------------------------------------------------------
extern "C" int32_t mdgen_profile_enable(mdgen_ctx* c, int32_t on) {
    if (!c) return fail(-1, "null context");
    c->prof_on = on != 0;
    return 0;
}

extern "C" int32_t mdgen_profile_phase_trace(mdgen_ctx* c, uint64_t* dev_buf, int64_t capacity_words) {
    if (!c) return fail(-1, "null context");
    c->phase_trace = (unsigned long long*)dev_buf;
    c->phase_trace_cap = dev_buf ? capacity_words : 0;
    return 0;
}

extern "C" int32_t mdgen_profile_report(mdgen_ctx* c, void* stream, char* buf, size_t buflen) {
    if (!c || !buf || buflen < 8) return fail(-1, "null argument");
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    std::map<std::string, std::pair<long, double>> agg;
    for (auto& r : c->prof) {
        float ms = 0.f;
        if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            auto& a = agg[r.cls];
            a.first += 1;
            a.second += ms;
        }
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    c->prof.clear();
    std::string js = "{";
    bool first = true;
    for (auto& kv : agg) {
        char tmp[160];
        snprintf(tmp, sizeof(tmp), "%s\"%s\": {\"count\": %ld, \"ms\": %.6f}", first ? "" : ", ", kv.first.c_str(),
                 kv.second.first, kv.second.second);
        js += tmp;
        first = false;
    }
    {   // not a kernel class: the context's placement-probe result and the split-form launches since the last report
        char tmp[200];
        snprintf(tmp, sizeof(tmp), "%s\"@context\": {\"count\": %ld, \"ms\": 0.0, \"xcd_round_robin\": %d, \"ncu\": %d}", first ? "" : ", ",
                 c->n_split_launches, c->xcd_round_robin ? 1 : 0, c->ncu);
        js += tmp;
        c->n_split_launches = 0;
    }
    js += "}";
    if (js.size() + 1 > buflen) return fail(-7, "profile buffer too small");
    std::memcpy(buf, js.c_str(), js.size() + 1);
    return 0;
}

// ---------------------------------------------------------------------------------------------
// SE(3) / pre / post
// ---------------------------------------------------------------------------------------------
static bool any_null(std::initializer_list<const void*> ps) {
    for (const void* p : ps)
        if (!p) return true;
    return false;
}
#define NONNULL(...) \
    if (any_null({__VA_ARGS__})) return fail(-1, "null tensor argument")

extern "C" int32_t mdgen_rigid_compose(int64_t n, const float* r1, const float* t1, const float* r2, const float* t2,
                                       float* ro, float* to, void* stream) {
    NONNULL(r1, t1, r2, t2, ro, to);
    if (n <= 0) return 0;
    launch_rigid_compose(n, r1, t1, r2, t2, ro, to, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}
extern "C" int32_t mdgen_rigid_invert(int64_t n, const float* r, const float* t, float* ro, float* to, void* stream) {
    NONNULL(r, t, ro, to);
    if (n <= 0) return 0;
    launch_rigid_invert(n, r, t, ro, to, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}
extern "C" int32_t mdgen_rigid_apply(int64_t n, int64_t ppf, const float* r, const float* t, const float* pts,
                                     float* out, int32_t inverse, void* stream) {
    NONNULL(r, t, pts, out);
    if (n <= 0 || ppf <= 0) return 0;
    launch_rigid_apply(n, ppf, r, t, pts, out, inverse, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}
extern "C" int32_t mdgen_quat_to_rot(int64_t n, const float* q, int32_t normalize, float* rot, void* stream) {
    NONNULL(q, rot);
    if (n <= 0) return 0;
    launch_quat_to_rot(n, q, normalize, rot, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}
extern "C" int32_t mdgen_rot_to_quat(int64_t n, const float* rot, float* q, void* stream) {
    NONNULL(rot, q);
    if (n <= 0) return 0;
    launch_rot_to_quat(n, rot, q, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}
extern "C" int32_t mdgen_prep_latents(const mdgen_shape* sh, int32_t tps, int32_t cond_interval, const float* rots, const float* trans,
                                      const float* torsions, float* latents, float* x_cond, int64_t* x_cond_mask,
                                      void* stream) {
    if (!sh) return fail(-1, "null shape");
    NONNULL(rots, trans, torsions, latents, x_cond, x_cond_mask);
    if (sh->B < 1 || sh->T < 1 || sh->L < 1) return fail(-2, "B, T, L must be >= 1");
    if (cond_interval < 0) return fail(-2, "cond_interval must be >= 0 (0 = none)");
    launch_prep_latents(sh->B, sh->T, sh->L, tps, 0, cond_interval, rots, trans, torsions, latents, x_cond, x_cond_mask,
                        (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}
extern "C" int32_t mdgen_prep_keyframes(const mdgen_shape* sh, int32_t cond_interval, const float* key_rots,
                                        const float* key_trans, const float* key_torsions, float* x_cond,
                                        int64_t* x_cond_mask, float* start_rot, float* start_trans, void* stream) {
    if (!sh) return fail(-1, "null shape");
    NONNULL(key_rots, key_trans, key_torsions, x_cond, x_cond_mask, start_rot, start_trans);
    if (sh->B < 1 || sh->T < 1 || sh->L < 1) return fail(-2, "B, T, L must be >= 1");
    if (cond_interval < 1) return fail(-2, "cond_interval must be >= 1");
    launch_prep_keyframes(sh->B, sh->T, sh->L, cond_interval, key_rots, key_trans, key_torsions, x_cond, x_cond_mask, start_rot,
                          start_trans, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}
extern "C" int32_t mdgen_samples_to_atom14(const mdgen_shape* sh, int32_t D, int32_t tps, const float* samples,
                                           const float* rot0, const float* trans0, const int64_t* seqres,
                                           const float* default_frames, const float* lit_positions,
                                           const int64_t* atom14_group, const float* atom14_mask, float* atom14,
                                           void* stream) {
    if (!sh) return fail(-1, "null shape");
    NONNULL(samples, rot0, trans0, seqres, default_frames, lit_positions, atom14_group, atom14_mask, atom14);
    if (sh->B < 1 || sh->T < 1 || sh->L < 1) return fail(-2, "B, T, L must be >= 1");
    if (D < (tps ? 28 : 21)) return fail(-2, "latent_dim too small");
    launch_samples_to_atom14(sh->B, sh->T, sh->L, D, tps, samples, rot0, trans0, seqres, default_frames, lit_positions,
                             atom14_group, atom14_mask, atom14, sh->T, 0, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}
extern "C" int32_t mdgen_atom14_to_cond(int32_t B, int32_t L, const float* atom14, const int64_t* seqres,
                                        const int64_t* a37to14, const float* a37mask, const int64_t* chi_idx,
                                        const float* chi_mask, float* rots, float* trans, float* tors, float* tmask,
                                        void* stream) {
    NONNULL(atom14, seqres, a37to14, a37mask, chi_idx, chi_mask, rots, trans, tors, tmask);
    if (B < 1 || L < 1) return fail(-2, "B, L must be >= 1");
    launch_atom14_to_cond(B, L, atom14, (long)L * 42, seqres, a37to14, a37mask, chi_idx, chi_mask, rots, trans, tors, tmask,
                          (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}
extern "C" int32_t mdgen_pdb_format(int64_t M, int32_t L, int64_t model_base, const float* atom14, const int64_t* aatype,
                                    const int64_t* a37to14, const float* a37mask, const uint8_t* templates,
                                    const uint8_t* ter_template, int64_t* offsets, uint8_t* text, int64_t text_capacity,
                                    int64_t* status, void* stream) {
    NONNULL(atom14, aatype, a37to14, a37mask, templates, ter_template, offsets, text, status);
    if (M < 1 || L < 1 || L > 9999) return fail(-2, "M must be >= 1 and L in 1 .. 9999 (the residue number has four columns)");
    if (model_base < 0 || model_base > INT64_MAX - M) return fail(-2, "model_base must be >= 0 (and model_base + M fit int64)");
    if (text_capacity < 0) return fail(-2, "text_capacity must be >= 0");
    HIPCHK(hipMemsetAsync(status, 0, 2 * sizeof(int64_t), (hipStream_t)stream));
    launch_pdb_format(M, L, model_base, atom14, aatype, a37to14, a37mask, templates, ter_template, offsets, text, text_capacity,
                      status, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

// ---------------------------------------------------------------------------------------------
// trajectory analysis (k_analysis.hip): every refusal is decided on the host, before a device call
// ---------------------------------------------------------------------------------------------
constexpr int64_t kTrajMaxFrames = (int64_t)1 << 40;
constexpr int32_t kTrajMaxFeatures = 32768;

extern "C" int32_t mdgen_traj_dihedrals(int64_t F, int32_t L, int32_t NF, const float* atom14, const int32_t* quad, float* angles,
                                        void* stream) {
    if (F < 1 || F > kTrajMaxFrames) return fail(-2, "F must be in 1 .. 2^40");
    if (L < 1 || L > (1 << 20)) return fail(-2, "L must be in 1 .. 2^20");
    if (NF < 0 || NF > kTrajMaxFeatures) return fail(-2, "NF must be in 0 .. 32768");
    if (NF == 0) return 0;
    NONNULL(atom14, quad, angles);
    for (int64_t i = 0; i < (int64_t)NF * 4; ++i)
        if (quad[i] < 0 || quad[i] >= L * 14)
            return fail(-2, "quad[%lld][%d] = %d is outside the frame's %d atoms", (long long)(i / 4), (int)(i % 4), quad[i], L * 14);
    launch_dihedrals(F, L, NF, atom14, quad, angles, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

extern "C" int32_t mdgen_traj_histograms(int64_t F, int32_t NF, const float* angles, int32_t bins1, const double* edges1, int32_t P,
                                         const int32_t* pairs, int32_t bins2, const double* edges2, int64_t* hist1, int64_t* hist2,
                                         int64_t* dropped, void* stream) {
    if (F < 1 || F > kTrajMaxFrames) return fail(-2, "F must be in 1 .. 2^40");
    if (NF < 0 || NF > kTrajMaxFeatures) return fail(-2, "NF must be in 0 .. 32768");
    if (P < 0 || P > kTrajMaxFeatures) return fail(-2, "P must be in 0 .. 32768");
    if (bins1 < 1 || bins1 > kHistMaxCells) return fail(-2, "bins1 must be in 1 .. %d", kHistMaxCells);
    if (bins2 < 1 || bins2 * (int64_t)bins2 > kHistMaxCells) return fail(-2, "bins2 must be in 1 .. 128");
    if (NF == 0 && P > 0) return fail(-2, "pairs of no features");
    if (NF == 0) return 0;
    NONNULL(angles, edges1, hist1, dropped);
    if (P > 0) {
        NONNULL(pairs, edges2, hist2);
    }
    for (int64_t i = 0; i < (int64_t)P * 2; ++i)
        if (pairs[i] < 0 || pairs[i] >= NF)
            return fail(-2, "pairs[%lld][%d] = %d is outside the %d features", (long long)(i / 2), (int)(i % 2), pairs[i], NF);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(hist1, 0, (size_t)NF * bins1 * sizeof(int64_t), s));
    if (P > 0) HIPCHK(hipMemsetAsync(hist2, 0, (size_t)P * bins2 * bins2 * sizeof(int64_t), s));
    HIPCHK(hipMemsetAsync(dropped, 0, (size_t)(NF + P) * sizeof(int64_t), s));
    launch_torsion_hist(F, NF, angles, bins1, edges1, P, pairs, bins2, edges2, hist1, hist2, dropped, s);
    LAUNCHCHK();
    return 0;
}

static int traj_acov_shape(int64_t n, int32_t NF, int64_t K) {
    if (n < 1 || n > kTrajMaxFrames) return fail(-2, "n must be in 1 .. 2^40");
    if (NF < 0 || NF > kTrajMaxFeatures) return fail(-2, "NF must be in 0 .. 32768");
    if (K < 0 || K > n - 1) return fail(-2, "K must be in 0 .. n - 1 (n = %lld, K = %lld)", (long long)n, (long long)K);
    if (NF > 0 && acov_groups(n, NF, K) >= ((int64_t)1 << 31)) return fail(-2, "NF * (K + 1) is beyond one launch's grid");
    return 0;
}

extern "C" int32_t mdgen_traj_acov_workspace_bytes(int64_t n, int32_t NF, int64_t K, size_t* bytes) {
    NONNULL(bytes);
    if (int rc = traj_acov_shape(n, NF, K)) return rc;
    *bytes = NF == 0 ? 0 : acov_workspace_bytes(n, NF, K);
    return 0;
}

extern "C" int32_t mdgen_traj_acov(int64_t n, int32_t NF, int64_t K, const float* angles, double* acov, double* mean_sin,
                                   double* mean_cos, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = traj_acov_shape(n, NF, K)) return rc;
    if (NF == 0) return 0;
    NONNULL(angles, acov, mean_sin, mean_cos, workspace);
    const size_t need = acov_workspace_bytes(n, NF, K);
    if (workspace_bytes < need) return fail(-3, "workspace too small: %zu < %zu", workspace_bytes, need);
    if ((uintptr_t)workspace % 16) return fail(-2, "workspace must be 16-byte aligned");
    launch_sincos_acov(n, NF, K, angles, acov, mean_sin, mean_cos, workspace, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

// tICA (k_tica.hip): the same conventions
static int traj_moments_shape(int64_t n, int32_t NF, int64_t lag) {
    if (n < 1 || n > kTrajMaxFrames) return fail(-2, "n must be in 1 .. 2^40");
    if (NF < 0 || NF > kTicaMaxFeatures) return fail(-2, "NF must be in 0 .. %d", kTicaMaxFeatures);
    if (lag < 0 || lag > n - 1) return fail(-2, "lag must be in 0 .. n - 1 (n = %lld, lag = %lld)", (long long)n, (long long)lag);
    return 0;
}

extern "C" int32_t mdgen_traj_lagged_moments_workspace_bytes(int64_t n, int32_t NF, int64_t lag, size_t* bytes) {
    NONNULL(bytes);
    if (int rc = traj_moments_shape(n, NF, lag)) return rc;
    *bytes = NF == 0 ? 0 : moments_workspace_bytes(n, NF, lag);
    return 0;
}

extern "C" int32_t mdgen_traj_lagged_moments(int64_t n, int32_t NF, int64_t lag, const float* angles, double* sx, double* sy,
                                             double* cxx, double* cyy, double* cxy, void* workspace, size_t workspace_bytes,
                                             void* stream) {
    if (int rc = traj_moments_shape(n, NF, lag)) return rc;
    if (NF == 0) return 0;
    NONNULL(angles, sx, sy, cxx, cyy, cxy, workspace);
    const size_t need = moments_workspace_bytes(n, NF, lag);
    if (workspace_bytes < need) return fail(-3, "workspace too small: %zu < %zu", workspace_bytes, need);
    if ((uintptr_t)workspace % 16) return fail(-2, "workspace must be 16-byte aligned");
    launch_lagged_moments(n, NF, lag, angles, sx, sy, cxx, cyy, cxy, workspace, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

extern "C" int32_t mdgen_traj_project(int64_t n, int32_t NF, int32_t d, const float* angles, const float* mean, const float* W,
                                      float* out, void* stream) {
    if (n < 1 || n > kTrajMaxFrames) return fail(-2, "n must be in 1 .. 2^40");
    if (NF < 0 || NF > kTicaMaxFeatures) return fail(-2, "NF must be in 0 .. %d", kTicaMaxFeatures);
    if (NF == 0) return 0;
    if (d < 1 || d > 2 * NF) return fail(-2, "d must be in 1 .. 2 NF (NF = %d, d = %d)", NF, d);
    NONNULL(angles, mean, W, out);
    launch_project(n, NF, d, angles, mean, W, out, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

extern "C" int32_t mdgen_traj_series_acov_workspace_bytes(int64_t n, int32_t NS, int64_t K, size_t* bytes) {
    NONNULL(bytes);
    if (int rc = traj_acov_shape(n, NS, K)) return rc;
    *bytes = NS == 0 ? 0 : series_acov_workspace_bytes(n, NS, K);
    return 0;
}

extern "C" int32_t mdgen_traj_series_acov(int64_t n, int32_t NS, int64_t K, const float* x, double* acov, double* mean,
                                          void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = traj_acov_shape(n, NS, K)) return rc;
    if (NS == 0) return 0;
    NONNULL(x, acov, mean, workspace);
    const size_t need = series_acov_workspace_bytes(n, NS, K);
    if (workspace_bytes < need) return fail(-3, "workspace too small: %zu < %zu", workspace_bytes, need);
    if ((uintptr_t)workspace % 16) return fail(-2, "workspace must be 16-byte aligned");
    launch_series_acov(n, NS, K, x, acov, mean, workspace, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

extern "C" int32_t mdgen_traj_histograms_xy(int64_t F, int32_t NC, const float* values, int32_t P, const int32_t* pairs, int32_t bins,
                                            const double* edges_x, const double* edges_y, int64_t* hist2, int64_t* dropped,
                                            void* stream) {
    if (F < 1 || F > kTrajMaxFrames) return fail(-2, "F must be in 1 .. 2^40");
    if (NC < 1 || NC > kTrajMaxFeatures) return fail(-2, "NC must be in 1 .. 32768");
    if (P < 0 || P > kTrajMaxFeatures) return fail(-2, "P must be in 0 .. 32768");
    if (bins < 1 || bins * (int64_t)bins > kHistMaxCells) return fail(-2, "bins must be in 1 .. 128");
    if (P == 0) return 0;
    NONNULL(values, pairs, edges_x, edges_y, hist2, dropped);
    for (int64_t i = 0; i < (int64_t)P * 2; ++i)
        if (pairs[i] < 0 || pairs[i] >= NC)
            return fail(-2, "pairs[%lld][%d] = %d is outside the %d columns", (long long)(i / 2), (int)(i % 2), pairs[i], NC);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(hist2, 0, (size_t)P * bins * bins * sizeof(int64_t), s));
    HIPCHK(hipMemsetAsync(dropped, 0, (size_t)P * sizeof(int64_t), s));
    launch_hist_xy(F, NC, values, P, pairs, bins, edges_x, edges_y, hist2, dropped, s);
    LAUNCHCHK();
    return 0;
}

// k-means / MSM (k_msm.hip): the same conventions
static int traj_kmeans_shape(int64_t n, int32_t d, int32_t k) {
    if (n < 1 || n > kTrajMaxFrames) return fail(-2, "n must be in 1 .. 2^40");
    if (d < 1 || d > kKmMaxDim) return fail(-2, "d must be in 1 .. %d", kKmMaxDim);
    if (k < 1 || k > kKmMaxCenters) return fail(-2, "k must be in 1 .. %d", kKmMaxCenters);
    return 0;
}

extern "C" int32_t mdgen_traj_kmeans_assign(int64_t n, int32_t d, int32_t k, const float* x, const float* centers, int32_t* assign,
                                            float* dist2, void* stream) {
    if (int rc = traj_kmeans_shape(n, d, k)) return rc;
    NONNULL(x, centers, assign);
    launch_kmeans_assign(n, d, k, x, centers, assign, dist2, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

extern "C" int32_t mdgen_traj_kmeans_step_workspace_bytes(int64_t n, int32_t d, int32_t k, size_t* bytes) {
    NONNULL(bytes);
    if (int rc = traj_kmeans_shape(n, d, k)) return rc;
    *bytes = kmeans_step_workspace_bytes(n, d, k);
    return 0;
}

extern "C" int32_t mdgen_traj_kmeans_step(int64_t n, int32_t d, int32_t k, const float* x, float* centers, int32_t* assign,
                                          double* sums, int64_t* counts, double* cost, int32_t* state, double tol, void* workspace,
                                          size_t workspace_bytes, void* stream) {
    if (int rc = traj_kmeans_shape(n, d, k)) return rc;
    if (!(tol >= 0.0)) return fail(-2, "tol must be >= 0");
    NONNULL(x, centers, assign, sums, counts, cost, state, workspace);
    const size_t need = kmeans_step_workspace_bytes(n, d, k);
    if (workspace_bytes < need) return fail(-3, "workspace too small: %zu < %zu", workspace_bytes, need);
    if ((uintptr_t)workspace % 16) return fail(-2, "workspace must be 16-byte aligned");
    launch_kmeans_step(n, d, k, x, centers, assign, sums, counts, cost, state, tol, workspace, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

extern "C" int32_t mdgen_traj_kmeans_pp_workspace_bytes(int64_t n, int32_t d, int32_t k, size_t* bytes) {
    NONNULL(bytes);
    if (int rc = traj_kmeans_shape(n, d, k)) return rc;
    *bytes = kmeans_pp_workspace_bytes(n);
    return 0;
}

extern "C" int32_t mdgen_traj_kmeans_pp(int64_t n, int32_t d, int32_t k, const float* x, const double* u, int32_t r0, int32_t r1,
                                        int64_t* chosen, float* mind2, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = traj_kmeans_shape(n, d, k)) return rc;
    if (r0 < 0 || r0 > r1 || r1 > k) return fail(-2, "rounds must satisfy 0 <= r0 <= r1 <= k (r0 = %d, r1 = %d, k = %d)", r0, r1, k);
    NONNULL(x, u, chosen, mind2, workspace);
    for (int32_t r = r0; r < r1; ++r)
        if (!(u[r] >= 0.0 && u[r] < 1.0)) return fail(-2, "u[%d] = %g is outside [0, 1)", r, u[r]);
    const size_t need = kmeans_pp_workspace_bytes(n);
    if (workspace_bytes < need) return fail(-3, "workspace too small: %zu < %zu", workspace_bytes, need);
    if ((uintptr_t)workspace % 16) return fail(-2, "workspace must be 16-byte aligned");
    launch_kmeans_pp(n, d, x, u, r0, r1, chosen, mind2, workspace, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

extern "C" int32_t mdgen_traj_count_matrix(int64_t n, int64_t lag, int32_t k, const int32_t* dtraj, int64_t* counts,
                                           int64_t* dropped, void* stream) {
    if (n < 1 || n > kTrajMaxFrames) return fail(-2, "n must be in 1 .. 2^40");
    if (lag < 0) return fail(-2, "lag must be >= 0 (lag = %lld)", (long long)lag);
    if (k < 1 || k > kKmMaxCenters) return fail(-2, "k must be in 1 .. %d", kKmMaxCenters);
    NONNULL(dtraj, counts, dropped);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(counts, 0, (size_t)k * k * sizeof(int64_t), s));
    HIPCHK(hipMemsetAsync(dropped, 0, sizeof(int64_t), s));
    if (lag >= n) return 0;   // no pair: all zeros
    launch_count_matrix(n, lag, k, dtraj, counts, dropped, s);
    LAUNCHCHK();
    return 0;
}

// transition paths (k_tps.hip): the same conventions; phi is a host array, checked here
extern "C" int32_t mdgen_tp_sample(int64_t n_samples, int32_t N, int32_t k, const double* Ta, const double* Ba, int32_t start,
                                   int32_t end, uint64_t seed, uint32_t stream_id, uint64_t sample_base, int32_t kb,
                                   const double* Tb, const double* Bb, const int32_t* phi, int32_t* paths, double* prob,
                                   void* stream) {
    if (n_samples < 1 || n_samples > kTrajMaxFrames) return fail(-2, "n_samples must be in 1 .. 2^40");
    if (N < 2 || N > kTpMaxLen) return fail(-2, "N must be in 2 .. %d", kTpMaxLen);
    if (k < 1 || k > kTpMaxStates) return fail(-2, "k must be in 1 .. %d", kTpMaxStates);
    if (kb < 0 || kb > kTpMaxStates) return fail(-2, "kb must be in 1 .. %d (0: no scoring set)", kTpMaxStates);
    if (start < 0 || start >= k || end < 0 || end >= k)
        return fail(-2, "start = %d / end = %d is outside the %d states", start, end, k);
    NONNULL(Ta, Ba, paths);
    TpPhi map = {};
    if (kb > 0) {
        NONNULL(Tb, Bb, phi, prob);
        for (int32_t i = 0; i < k; ++i) {
            if (phi[i] < 0 || phi[i] >= kb) return fail(-2, "phi[%d] = %d is outside the %d scoring states", i, phi[i], kb);
            map.v[i] = (uint8_t)phi[i];
        }
    }
    launch_tp_sample(n_samples, N, k, Ta, Ba, start, end, seed, stream_id, sample_base, kb, Tb, Bb, map, paths, prob,
                     (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

// Cartesian ensemble statistics (k_ensemble.hip): the same conventions, but for mdgen_ens_superpose's weight check
static int ens_frames_atoms(int64_t F, int32_t A, int32_t min_atoms) {
    if (F < 1 || F > kTrajMaxFrames) return fail(-2, "F must be in 1 .. 2^40");
    if (A < min_atoms || A > kEnsMaxAtoms) return fail(-2, "A must be in %d .. %d", min_atoms, kEnsMaxAtoms);
    return 0;
}

extern "C" int32_t mdgen_ens_superpose(int64_t F, int32_t A, const float* x, const float* ref, const float* w, const uint8_t* exists,
                                       float* out, double* rot, double* rmsd, void* stream) {
    if (int rc = ens_frames_atoms(F, A, 3)) return rc;
    NONNULL(x, ref, w, out);
    hipStream_t s = (hipStream_t)stream;
    std::vector<float> hw((size_t)A);
    HIPCHK(hipMemcpyAsync(hw.data(), w, (size_t)A * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    int positive = 0;
    for (int32_t a = 0; a < A; ++a) {
        if (!(hw[a] >= 0.f) || std::isinf(hw[a])) return fail(-2, "w[%d] = %g: weights must be finite and >= 0", a, (double)hw[a]);
        positive += hw[a] > 0.f;
    }
    if (positive < 3) return fail(-2, "a superposition needs at least 3 atoms of positive weight, got %d", positive);
    launch_ens_superpose(F, A, x, ref, w, exists, out, rot, rmsd, s);
    LAUNCHCHK();
    return 0;
}

extern "C" int32_t mdgen_ens_moments_workspace_bytes(int64_t F, int32_t A, size_t* bytes) {
    NONNULL(bytes);
    if (int rc = ens_frames_atoms(F, A, 1)) return rc;
    *bytes = ens_moments_workspace_bytes(F, A);
    return 0;
}

extern "C" int32_t mdgen_ens_moments(int64_t F, int32_t A, const float* x, double* mean, double* cov, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    if (int rc = ens_frames_atoms(F, A, 1)) return rc;
    NONNULL(x, mean, cov, workspace);
    const size_t need = ens_moments_workspace_bytes(F, A);
    if (workspace_bytes < need) return fail(-3, "workspace too small: %zu < %zu", workspace_bytes, need);
    if ((uintptr_t)workspace % 16) return fail(-2, "workspace must be 16-byte aligned");
    launch_ens_moments(F, A, x, mean, cov, workspace, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

static int ens_pairwise_shape(int64_t Fa, int64_t Fb, int32_t A) {
    if (Fa < 1 || Fa > kEnsMaxPairFrames || Fb < 1 || Fb > kEnsMaxPairFrames)
        return fail(-2, "Fa and Fb must be in 1 .. 2^20 - 1 (Fa = %lld, Fb = %lld)", (long long)Fa, (long long)Fb);
    if (A < 1 || A > kEnsMaxAtoms) return fail(-2, "A must be in 1 .. %d", kEnsMaxAtoms);
    return 0;
}

extern "C" int32_t mdgen_ens_pairwise_d2_workspace_bytes(int64_t Fa, int64_t Fb, int32_t A, size_t* bytes) {
    NONNULL(bytes);
    if (int rc = ens_pairwise_shape(Fa, Fb, A)) return rc;
    *bytes = ens_pairwise_workspace_bytes(Fa, Fb);
    return 0;
}

extern "C" int32_t mdgen_ens_pairwise_d2(int64_t Fa, int64_t Fb, int32_t A, const float* xa, const float* xb, float* d2, double* sums,
                                         void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = ens_pairwise_shape(Fa, Fb, A)) return rc;
    NONNULL(xa, xb, sums, workspace);
    const size_t need = ens_pairwise_workspace_bytes(Fa, Fb);
    if (workspace_bytes < need) return fail(-3, "workspace too small: %zu < %zu", workspace_bytes, need);
    if ((uintptr_t)workspace % 16) return fail(-2, "workspace must be 16-byte aligned");
    launch_ens_pairwise_d2(Fa, Fb, A, xa, xb, d2, sums, workspace, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

extern "C" int32_t mdgen_ens_contact_counts(int64_t F, int32_t N, const float* ca, float cutoff2, int32_t* counts, void* stream) {
    if (F < 1 || F > INT32_MAX) return fail(-2, "F must be in 1 .. 2^31 - 1");
    if (N < 1 || N > kEnsMaxResidues) return fail(-2, "N must be in 1 .. %d", kEnsMaxResidues);
    if (!(cutoff2 >= 0.f) || std::isinf(cutoff2)) return fail(-2, "cutoff2 = %g: the squared cutoff must be finite and >= 0", (double)cutoff2);
    NONNULL(ca, counts);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(counts, 0, (size_t)N * N * sizeof(int32_t), s));
    launch_ens_contact_counts(F, N, ca, cutoff2, counts, s);
    LAUNCHCHK();
    return 0;
}

static int ens_sasa_shape(int32_t A, int32_t P) {
    if (A < 1 || A > kEnsMaxAtoms) return fail(-2, "A must be in 1 .. %d", kEnsMaxAtoms);
    if (P < 1 || P > kEnsSasaMaxPoints) return fail(-2, "P must be in 1 .. %d", kEnsSasaMaxPoints);
    return 0;
}

extern "C" int32_t mdgen_ens_sasa_workspace_bytes(int32_t A, int32_t P, size_t* bytes) {
    NONNULL(bytes);
    if (int rc = ens_sasa_shape(A, P)) return rc;
    *bytes = ens_sasa_workspace_bytes(A, P);
    return 0;
}

// radius and points are host arrays, checked here and staged into the workspace with R = radius + probe and R2 = R R
extern "C" int32_t mdgen_ens_sasa_counts(int64_t F, int32_t A, int32_t P, const float* x, const float* radius, const float* points,
                                         float probe, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    if (F < 1 || F > INT32_MAX) return fail(-2, "F must be in 1 .. 2^31 - 1");
    if (int rc = ens_sasa_shape(A, P)) return rc;
    if (!(probe >= 0.f && probe <= kEnsSasaMaxRadius)) return fail(-2, "probe = %g: the probe radius must be in 0 .. 16", (double)probe);
    NONNULL(x, radius, points, counts, workspace);
    const size_t need = ens_sasa_workspace_bytes(A, P);
    if (workspace_bytes < need) return fail(-3, "workspace too small: %zu < %zu", workspace_bytes, need);
    if ((uintptr_t)workspace % 16) return fail(-2, "workspace must be 16-byte aligned");
    std::vector<float> host(need / sizeof(float), 0.f);
    float *R = host.data(), *R2 = R + A, *pts = R2 + A;
    for (int32_t a = 0; a < A; ++a) {
        const float r = radius[a];
        if (!(r >= 0.f && r <= kEnsSasaMaxRadius)) return fail(-2, "radius[%d] = %g: a radius must be in 0 .. 16 (0: no atom)", a, (double)r);
        R[a] = r == 0.f ? 0.f : r + probe;   // one fp32 add, one fp32 multiply
        R2[a] = R[a] * R[a];
    }
    for (int32_t k = 0; k < P; ++k) {
        const double u0 = points[3 * k], u1 = points[3 * k + 1], u2 = points[3 * k + 2];
        const double norm = std::sqrt(u0 * u0 + u1 * u1 + u2 * u2);
        if (!(std::fabs(norm - 1.0) <= 1e-3))
            return fail(-2, "points[%d] = (%g, %g, %g) is not a unit vector (|u| = %g)", k, u0, u1, u2, norm);
        for (int ax = 0; ax < 3; ++ax) pts[(size_t)ax * P + k] = points[3 * k + ax];
    }
    hipStream_t s = (hipStream_t)stream;
    // (pageable host memory: the runtime has taken the bytes when the call returns)
    HIPCHK(hipMemcpyAsync(workspace, host.data(), need, hipMemcpyHostToDevice, s));
    launch_ens_sasa_counts(F, A, P, x, (const float*)workspace, counts, s);
    LAUNCHCHK();
    return 0;
}

// ---------------------------------------------------------------------------------------------
// flow-matching training target and loss (forward only)
// ---------------------------------------------------------------------------------------------
extern "C" int32_t mdgen_path_plan(int64_t B, int64_t per_sample, int32_t path_type, const float* t, const float* x0,
                                   const float* x1, float* xt, float* ut, void* stream) {
    NONNULL(t, x0, x1, xt, ut);
    if (B < 1 || per_sample < 1) return fail(-2, "B, per_sample must be >= 1");
    if (path_type != 0 && path_type != 1) return fail(-2, "path_type: 0 = Linear, 1 = GVP");
    launch_path_plan(t, x0, x1, xt, ut, per_sample, B, path_type, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

extern "C" int32_t mdgen_masked_mse(int64_t B, int64_t per_sample, const float* pred, const float* target,
                                    const float* mask, float* loss, void* stream) {
    NONNULL(pred, target, mask, loss);
    if (B < 1 || per_sample < 1) return fail(-2, "B, per_sample must be >= 1");
    launch_masked_mse(pred, target, mask, loss, per_sample, B, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

extern "C" int32_t mdgen_from_3_points(int64_t n, const float* p_neg_x, const float* origin, const float* p_xy,
                                       float* rot, float* trans, void* stream) {
    NONNULL(p_neg_x, origin, p_xy, rot, trans);
    if (n < 1) return fail(-2, "n must be >= 1");
    launch_from_3_points(n, p_neg_x, origin, p_xy, rot, trans, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

// ---------------------------------------------------------------------------------------------
// optimiser side of the training step (flat fp32 buffers; csrc/k_optim.hip)
// ---------------------------------------------------------------------------------------------
extern "C" int32_t mdgen_grad_sumsq(int64_t n, const float* grads, float scale, float* scratch, int32_t scratch_floats,
                                    float* out, void* stream) {
    NONNULL(grads, scratch, out);
    if (n < 1) return fail(-2, "n must be >= 1");
    if (scratch_floats < 2) return fail(-2, "scratch_floats must be >= 2");
    if (((uintptr_t)scratch & 7) != 0) return fail(-2, "scratch must be 8-byte aligned");
    const int nb = scratch_floats / 2 < 512 ? scratch_floats / 2 : 512;   // fp64 partial sums
    launch_sumsq(grads, n, scale, scratch, nb, out, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

extern "C" int32_t mdgen_adam_step(int64_t n, float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                                   int32_t step, float lr, float beta1, float beta2, float eps, float weight_decay,
                                   int32_t adamw, float grad_scale, const float* sumsq, float max_norm, void* stream) {
    NONNULL(params, grads, exp_avg, exp_avg_sq);
    if (n < 1 || step < 1) return fail(-2, "n and step must be >= 1");
    if (!(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f) || !(eps > 0.f) || !(lr >= 0.f))
        return fail(-2, "invalid Adam hyper-parameters");
    const double bc1 = 1.0 - std::pow((double)beta1, (double)step);          // torch: 1 - beta ** step (python floats)
    const double bc2 = 1.0 - std::pow((double)beta2, (double)step);
    launch_adam(params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, adamw, (float)bc1,
                (float)std::sqrt(bc2), grad_scale, sumsq, max_norm, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

extern "C" int32_t mdgen_ema_update(int64_t n, float* ema, const float* params, float decay, void* stream) {
    NONNULL(ema, params);
    if (n < 1) return fail(-2, "n must be >= 1");
    launch_ema(ema, params, n, 1.0f - decay, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

#include "train.inc"
