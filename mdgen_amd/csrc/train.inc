// train.inc -- forward + backward of the training step (SURVEY.md section 8(f) #3), included at the end of api.hip.
//
// Reference: `NewMDGenWrapper.general_step` (wrapper.py:367-403): prep_batch -> transport.training_losses (xt, ut from
// the GVP plan; model forward; masked MSE) -> loss.mean().backward().  Here: the fp32 form of the network (k_fp32.hip)
// run with a tape (inputs of every sub-layer, q/k/v after RoPE, attention output, projection / fc2 output before the
// gate, fc1 pre-activation), then the chain rule backwards with the kernels of k_fp32_bwd.hip; gradients are ADDED
// into the caller's flat fp32 buffer at the offsets it gives per state_dict key.
// Parity: reference autograd at fp32 tolerance (tests/golden/train_grads_sim.npz; oracle autograd on the box).
// Scope: forward-simulation models and the two-sided (TPS) model, whose IPA stack runs twice on shared weights -- on the
// start frames with x_r = (end^-1 o start) and on the end frames with x_f = (start^-1 o end) (latent_model.py:193-205):
// two tapes, two backward passes into the same gradients.  Frozen buffers (pos_embed, rot_emb.inv_freq) get no gradient.

namespace {

// ---- the plan of a sub-layer: the form of every launch whose kernel depends on the operand mode, the row count, the axis or the
// alignment of the weights (kernels.h form functions), made once before the sub-layer's first launch (plan_* below) and kept beside
// its tape entry: the backward pass reads what the forward pass decided.
enum class DxRoute {
    Streamed,       // W^T as a bf16 fragment stream, packed in front of the product (launch16_pack_wstream, turned)
    TurnedWeight,   // W^T as an fp32 matrix (turned()): the forward layers' kernels
    Wtrans          // W as stored, LinearParams::wtrans
};
struct DxPlan { DxRoute route; LinearForm form; };
struct DwPlan { DwForm form; bool bias_rides; };   // bias_rides: the pass yields the bias gradient too (kernels.h dw_bias_rides)
struct AttnPlan {
    bool rows16;                 // y and du are stored as bf16 rows (see plan_attn) ...
    bool dqkv16;                 // ... and dq | dk | dv (sequence-resident attention only)
    bool qkv_one_pass;           // q | k | v as one product of 1152 columns (form qkv[0]), else three
    LinearForm qkv[3], out;
    TrainAttnForm attn;
    GateBwdForm gate;
    LnBwdForm ln;
    DxPlan dx_out, dx_qkv;       // dx_qkv / dw_qkv: bf16 operands: one product over q | k | v; fp32: each of the three
    DwPlan dw_out, dw_qkv;
};
struct MlpPlan {
    bool rows16;                 // y, hid, du and d pre are stored as bf16 rows
    LinearForm fc1, fc2;
    GateBwdForm gate;
    LnBwdForm ln;
    DxPlan dx_fc2, dx_fc1;
    DwPlan dw_fc2, dw_fc1;
};
struct IpaPlan {                 // [j]: q | kv | q_points | kv_points (kIpaProjCols)
    LinearForm proj[4], out;
    DxPlan dx_proj[4], dx_out;
    DwPlan dw_proj[4], dw_out;
};
struct FinalPlan { LinearForm lin; DxPlan dx; DwPlan dw; LnBwdForm ln; };

struct SubTapeAttn { float *h_in, *y, *qkv, *att, *u, *lse; AttnPlan plan; };   // y = LN-modulate(h_in): the q/k/v layers' input, taped
struct SubTapeMlp { float *h_in, *y, *pre, *hid, *u; MlpPlan plan; };   // hid = gelu(pre): fc2's input, taped rather than recomputed
struct SubTapeIpa { float *h_in, *proj, *feat, *stats; IpaPlan plan; };

// One pass of the IPA stack.  The one-sided model has one (on the start frames); the two-sided model two on shared weights, stream 0 =
// x_r on the start frames, stream 1 = x_f on the end frames (latent_model.py:193-205), forward and backward in that order.
struct IpaStream {
    float *h, *dh;                        // residual rows [B*L][384] (workspace) and their gradient
    const float* rel;                     // relative-frame input [B*L][7] of the two-sided model, else null ...
    const float *w7, *b7;                 // ... its embedder as ipa_init reads it ...
    Lin rel7;                             // ... and the embedder's gradient slots
    const float *rot, *trans;             // the frames its point attention runs on
    std::vector<SubTapeIpa> ip;           // the tape, per layer
    std::vector<SubTapeAttn> il;
    std::vector<SubTapeMlp> im;
};

struct Train {
    Run r;
    mdgen_ctx* c;
    // the caller's tensors beyond those of the Run
    const float *xt, *tvals, *target, *loss_mask;
    float *loss, *pred;
    float* grads;
    const int64_t* goff;     // per weight slot; < 0: no gradient wanted
    // Operand mode of the call's linear layers / weight gradients (option train_precision): false = exact fp32 products
    // (k32_linear / k32_dw), true = bf16-rounded operands on the bf16 MFMA with fp32 accumulation (the k16_* forms).
    bool bf16 = false;
    // scratch (backward)
    float *dh, *dy, *ytmp, *act, *stats, *part, *cpart, *dmod, *dsilu, *wt;
    size_t part_floats, cpart_floats;
    // Second stream (option train_streams = 2).  The weight / bias gradients of the linear layers are off the critical path of
    // the backward pass (nothing reads them before the optimiser): they run on `side`, beside the dX products, the attention
    // backward and the element-wise passes of the main stream, with partial-sum scratch of their own.  What they read as dY is
    // main-stream scratch that the NEXT sub-layer would overwrite, so du / dhid / dqkv exist twice and alternate per sub-layer;
    // a sub-layer starts once the second stream has finished the sub-layer before the previous one (begin_sub / end_sub).
    // Forward pass of the trunk (defer_gate): a sub-layer does not apply its gated residual update; it leaves it PENDING (the stream
    // is x + gate * u with x = the sub-layer's taped input), and the next sub-layer's LayerNorm launch forms it in registers, tapes it
    // and normalises it (k32_gate_ln_mod).  flush_pending() materialises the stream into h (after the last layer).  14 launches and
    // 28 passes over the 98 MB stream less per ATLAS step (26.9 -> 25.9 ms).  The IPA stack applies its updates at once.
    struct Pending { const float* x = nullptr; const float* u = nullptr; ModMap mm{}; int gate = 0; long nrows = 0; };
    Pending pend;
    bool defer_gate = false;
    // Turned weights (dX = dY W of the launches too small for the streamed kernel runs through the forward kernel on W^T): with a
    // second stream and bf16 operands the images of ALL such products of the call are computed there at the start of the call, while
    // the main stream runs the forward pass, from the list of requests the previous call recorded (mdgen_ctx::tr_plan); a request that
    // does not match the list falls back to a k32_transpose launch in place, and a call that deviates from the list or leaves part of
    // it unused has the next call record it anew.  (The second stream is otherwise idle during the forward pass, and the IPA stack's
    // backward, ~330 launches of 5-12 us on 256 rows, leaves the chip half idle: its 50 transposes moved off the critical path took
    // the ATLAS step 25.6 -> 25.2 ms.  Packing the streamed kernel's bf16 fragment streams ahead the same way is slower: a stream
    // packed right in front of its consumer is read out of the L2 it was just written to.)
    size_t tr_cursor = 0;
    bool tr_use = false, tr_waited = false, tr_record = false;
    hipEvent_t tr_done = nullptr;
    std::vector<mdgen_ctx::TurnReq> tr_new;
    hipStream_t side = nullptr;                  // null: one stream
    float *du = nullptr, *dhid = nullptr, *dqkv = nullptr, *dbias = nullptr;   // the instance of the current sub-layer
    float *du_[2], *dhid_[2], *dqkv_[2], *dbias_[2], *part2, *cpart2;
    int sub = 0;
    hipEvent_t done[2] = {nullptr, nullptr};
    // Event pool of the fork / join traffic, round-robin.  A call takes 6 events per attention sub-layer, 5 per IPA block, 3 per
    // MLP block, plus heads, milestones and the join: 80 per layer of the stack (two-sided model) is a safe bound, and the pool is
    // sized from that, so an event is not re-recorded within one call.  (Re-recording would still be safe -- a wait captures the
    // record that precedes it at enqueue time, and done[p] is consumed ~15 events later -- but the pool does not rely on it.)
    int events_used = 0;
    hipEvent_t next_event() {
        const size_t want = (size_t)96 * (size_t)(c->nl > 0 ? c->nl : 1) + 64;
        while (c->train_ev.size() < want) {
            hipEvent_t e = nullptr;
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) break;
            c->train_ev.push_back(e);
        }
        if (c->train_ev.empty() || (size_t)++events_used > c->train_ev.size()) return nullptr;   // (callers report -8)
        return c->train_ev[c->train_ev_next++ % c->train_ev.size()];
    }
    int begin_sub() {
        const int p = sub & 1;
        if (side && done[p]) HIPCHK(hipStreamWaitEvent(r.s, done[p], 0));
        du = du_[p]; dhid = dhid_[p]; dqkv = dqkv_[p]; dbias = dbias_[p];
        return 0;
    }
    int end_sub() {
        if (side) {
            hipEvent_t e = next_event();
            if (!e) return fail(-8, "hipEventCreate failed (training event pool)");
            HIPCHK(hipEventRecord(e, side));
            done[sub & 1] = e;
        }
        ++sub;
        return 0;
    }
    // where a weight gradient whose operands are complete on the main stream NOW is to be launched, with the partial-sum scratch
    // of that stream: the second stream if there is one and a gradient is wanted, else the main one
    struct Fork { hipStream_t s; float *part, *cpart; };
    int fork(bool wanted, Fork* f) {
        *f = Fork{r.s, part, cpart};
        if (!side || !wanted) return 0;
        hipEvent_t e = next_event();
        if (!e) return fail(-8, "hipEventCreate failed (training event pool)");
        HIPCHK(hipEventRecord(e, r.s));
        HIPCHK(hipStreamWaitEvent(side, e, 0));
        *f = Fork{side, part2, cpart2};
        return 0;
    }
    // Milestones: when the gradients of a parameter group are complete the caller's event for it is recorded on the
    // stream, so that its all-reduce can start on another stream while the rest of the backward pass runs
    // (mdgen_train_set_milestone_events).  Order: 0 final layer | 1 .. nl trunk layers nl-1 .. 0 | nl+1 token
    // embedders | nl+2 .. 2nl+1 IPA layers nl-1 .. 0 | 2nl+2 everything (embedding tables, time embedder).
    int milestone = 0;
    int mark() {
        if (milestone < (int)c->milestone_events.size() && c->milestone_events[milestone]) {
            hipStream_t ms = r.s;
            if (side) {   // the group's gradients come from both streams: the second one waits for the main one and carries the event
                hipEvent_t e = next_event();
                if (!e) return fail(-8, "hipEventCreate failed (training event pool)");
                HIPCHK(hipEventRecord(e, r.s));
                HIPCHK(hipStreamWaitEvent(side, e, 0));
                ms = side;
            }
            HIPCHK(hipEventRecord((hipEvent_t)c->milestone_events[milestone], ms));
        }
        ++milestone;
        return 0;
    }
    std::vector<SubTapeAttn> tl, tt;       // the trunk's tape: residue / temporal attention, MLP
    std::vector<SubTapeMlp> tm;
    IpaStream st[2];
    int nst = 1;
    float* rel7 = nullptr;                 // x_f | x_r [2][B*L][7] (two-sided model)
    FinalPlan fin{};                       // the final layer's plan, made in the forward pass
    const float* w(int slot) const { return c->f32(slot); }   // (every slot has its copy: check_f32_weights ran before the first launch)
    float* grad(int slot) const { return goff[slot] < 0 ? nullptr : grads + goff[slot]; }
};

struct Carver {
    unsigned char* base;
    size_t off = 0;
    float* take(size_t floats) {
        float* p = (float*)(base + off);
        off += (floats * 4 + 255) & ~(size_t)255;
        return p;
    }
};

constexpr size_t kPartFloats = (size_t)16 << 20;    // 64 MB of dW split partials
constexpr size_t kCpartFloats = (size_t)4 << 20;    // ... of column-sum partials
// all tape / scratch sizes in one place (used for the size query and for carving)
// `two_streams`: the second instances of du / dhid / dqkv / dbias and of the partial-sum scratch exist only then (option train_streams = 2;
// ~0.9 GB at ATLAS B1 T250 L256); with one stream the [1] pointers alias the [0] ones.
static size_t carve_train(Train* out, const mdgen_ctx* c, long B, long T, long L, unsigned char* base) {
    Train query;   // (the size query carves into a Train of its own)
    Train& t = out ? *out : query;
    const bool two_streams = c->opt_train_streams == 2;
    const long N = B * T * L, Mp = B * L, maxr = N > Mp ? N : Mp;
    Carver cv{base};
    auto attn = [&](long rows) { SubTapeAttn a; a.h_in = cv.take(rows * kC); a.y = cv.take(rows * kC); a.qkv = cv.take(rows * 3 * kC); a.att = cv.take(rows * kC); a.u = cv.take(rows * kC); a.lse = cv.take(rows * kH); return a; };
    auto mlp = [&](long rows) { SubTapeMlp a; a.h_in = cv.take(rows * kC); a.y = cv.take(rows * kC); a.pre = cv.take(rows * kF); a.hid = cv.take(rows * kF); a.u = cv.take(rows * kC); return a; };
    t.nst = c->d.tps_condition ? 2 : 1;
    for (int i = 0; i < c->nl; ++i) {
        t.tl.push_back(attn(N)); t.tt.push_back(attn(N)); t.tm.push_back(mlp(N));
        for (int k = 0; k < t.nst; ++k) {
            SubTapeIpa s; s.h_in = cv.take(Mp * kC); s.proj = cv.take(Mp * kIpaProj); s.feat = cv.take(Mp * kIpaFeat); s.stats = cv.take(Mp * 4);
            t.st[k].ip.push_back(s); t.st[k].il.push_back(attn(Mp)); t.st[k].im.push_back(mlp(Mp));
        }
    }
    if (t.nst == 2) {
        t.st[1].dh = cv.take(Mp * kC);
        t.rel7 = cv.take(2 * Mp * 7);
        t.st[0].rel = t.rel7 + Mp * 7;   // x_r
        t.st[1].rel = t.rel7;            // x_f
    } else {
        t.st[0].rel = nullptr;
    }
    t.dh = cv.take(N * kC);
    t.dy = cv.take(maxr * kC);
    for (int p = 0; p < 2; ++p) {
        if (p == 1 && !two_streams) {
            t.dqkv_[1] = t.dqkv_[0]; t.dhid_[1] = t.dhid_[0]; t.du_[1] = t.du_[0];
            break;
        }
        t.dqkv_[p] = cv.take(maxr * 3 * kC);
        t.dhid_[p] = cv.take(maxr * kF);
        t.du_[p] = cv.take(maxr * kC);
    }
    t.dqkv = t.dqkv_[0]; t.dhid = t.dhid_[0]; t.du = t.du_[0];
    t.ytmp = cv.take(maxr * kC);
    t.act = cv.take(maxr * kF);
    t.stats = cv.take(maxr * kH * 2);
    const long nseq_max = std::max(std::max(B * T, B * L), B);
    t.dbias_[0] = cv.take(nseq_max * kH * 2 * kDH);
    t.dbias_[1] = two_streams ? cv.take(nseq_max * kH * 2 * kDH) : t.dbias_[0];
    t.dbias = t.dbias_[0];
    t.part_floats = kPartFloats;
    t.part = cv.take(t.part_floats);
    t.cpart_floats = kCpartFloats;
    t.cpart = cv.take(t.cpart_floats);
    t.part2 = two_streams ? cv.take(t.part_floats) : t.part;              // the second stream's partial sums
    t.cpart2 = two_streams ? cv.take(t.cpart_floats) : t.cpart;
    t.dmod = cv.take((size_t)B * c->modrow);
    t.st[0].dh = cv.take(Mp * kC);
    t.dsilu = cv.take((size_t)B * (kC * 4 + 256));
    t.wt = cv.take((size_t)kF * kC);               // one transposed weight (lin_bwd, bf16-operand mode)
    return cv.off;
}

// ---- the plans -------------------------------------------------------------------------------------------------------
// Every activation the step's products read (tape, scratch, workspace) is carved at a 256-byte boundary and addressed at column
// offsets that are multiples of four floats: the plans take them as 16-byte aligned (the launchers check).  What varies is the
// alignment of the weights: a bound parameter buffer may put them anywhere (mdgen_train_bind_params).
static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static DwPlan dw_plan(const Train& t, const DwShape& q, bool x_bf16, bool dy_bf16) {
    const DwForm f = dw_form(t.bf16, q, t.part_floats, x_bf16, dy_bf16);
    return DwPlan{f, dw_bias_rides(f, q, t.part_floats)};
}
// dX[n][K] = dY[n][M] (ldy) W of a layer W [M][K].  bf16-operand mode: the weight turned once per use -- as a bf16 fragment stream
// for the streamed kernel, else as an fp32 matrix [K][M] (the contraction contiguous: turned()) for the forward layers' kernels
static DxPlan dx_plan(bool bf16, long n, int M, int K, int ldy, bool w_al, bool dy_bf16) {
    if (bf16 && M % 64 == 0 && (size_t)M * K <= (size_t)kF * kC) {
        const LinearForm f = linear_form(true, LinShape{n, K, M, ldy, K, 0, true, w_al, dy_bf16}, true);
        if (linear_streams(f)) return DxPlan{DxRoute::Streamed, f};
        return DxPlan{DxRoute::TurnedWeight, linear_form(true, LinShape{n, K, M, ldy, M, 0, true, true, false}, false)};
    }
    return DxPlan{DxRoute::Wtrans, linear_form(bf16, LinShape{n, K, M, ldy, K, 1, true, w_al, false}, false)};
}

// Rows as bf16: a sub-layer with >= 4096 rows stores its GEMM-only tensors as bf16 rows: the GELU output SubTapeMlp::hid, the taped
// LayerNorm + modulate output y (token rows of the q | k | v / fc1 products, X of their weight gradients), du = gate * dh, d pre =
// d hid * gelu'(pre) and, on axes of the sequence-resident attention, dq | dk | dv.  Each is only ever the token operand of a dX
// product and dY / X of a weight gradient, whose kernels round it to bf16 on its way into LDS anyway (k16_linear_wdma<true>,
// k16_dw_wide<XBF, DYBF>): written rounded by its producer, the same values enter the MFMAs and half the bytes cross HBM two or
// three times (ATLAS step: y 25.2 -> 24.6, dq | dk | dv -> 24.2, du -0.3, d pre -0.2 ms).  Weight and activation gradients are
// unchanged; the bias gradients of the layers whose dY is stored rounded are column sums of the stored values.
// Only the streamed / wide kernels read such rows, so a plan is first made with them and kept if every consumer's form is one of
// those and the one-pass gate kernel writes du; else it is made again with fp32 rows.
// (ln_bwd_form's `adjacent`: a site's scale chunk lies right behind its shift chunk, Rows::scale)
static AttnPlan plan_attn(const Train& t, long n, const AxisMap& ax, long tpg, const bool (&w_al)[4]) {
    AttnPlan p{};
    p.attn = train_attn_form(t.bf16, ax);
    p.gate = gate_bwd_form(n, tpg, t.cpart_floats);
    p.ln = ln_bwd_form(n, tpg, t.cpart_floats, true);
    const bool w3_al = w_al[0] && w_al[1] && w_al[2];
    for (int r16 = t.bf16 ? 1 : 0; r16 >= 0; --r16) {
        p.rows16 = r16 != 0;
        p.dqkv16 = p.rows16 && attn_seq(p.attn);
        const LinearForm one = linear_form(t.bf16, LinShape{n, 3 * kC, kC, kC, kC, 0, true, w3_al, p.rows16}, true);
        p.qkv_one_pass = t.bf16 && one != LinearForm::Plain;
        for (int j = 0; j < 3; ++j)
            p.qkv[j] = p.qkv_one_pass ? one : linear_form(t.bf16, LinShape{n, kC, kC, kC, kC, 0, true, w_al[j], false}, false);
        p.out = linear_form(t.bf16, LinShape{n, kC, kC, kC, kC, 0, true, w_al[3], false}, true);
        p.dx_out = dx_plan(t.bf16, n, kC, kC, kC, w_al[3], p.rows16);
        p.dw_out = dw_plan(t, DwShape{n, kC, kC, kC, kC, true}, false, p.rows16);
        // bf16 operands: q | k | v as one layer of 1152 outputs; fp32: three layers, each with this plan
        const int mq = t.bf16 ? 3 * kC : kC;
        p.dx_qkv = dx_plan(t.bf16, n, mq, kC, 3 * kC, w3_al, p.dqkv16);
        p.dw_qkv = dw_plan(t, DwShape{n, mq, kC, 3 * kC, kC, true}, p.rows16, p.dqkv16);
        if (!p.rows16 || (p.gate == GateBwdForm::Sums && p.qkv[0] == LinearForm::StreamBf16Rows &&
                          p.dx_out.route == DxRoute::Streamed && dw_wide(p.dw_out.form) && dw_wide(p.dw_qkv.form) &&
                          (!p.dqkv16 || p.dx_qkv.route == DxRoute::Streamed)))
            break;
    }
    return p;
}
static MlpPlan plan_mlp(const Train& t, long n, long tpg, const bool (&w_al)[2]) {
    MlpPlan p{};
    p.gate = gate_bwd_form(n, tpg, t.cpart_floats);
    p.ln = ln_bwd_form(n, tpg, t.cpart_floats, true);
    for (int r16 = t.bf16 ? 1 : 0; r16 >= 0; --r16) {   // (y, hid, du and d pre alike)
        p.rows16 = r16 != 0;
        p.fc1 = linear_form(t.bf16, LinShape{n, kF, kC, kC, kC, 0, true, w_al[0], p.rows16}, true);
        p.fc2 = linear_form(t.bf16, LinShape{n, kC, kF, kF, kF, 0, true, w_al[1], p.rows16}, true);
        p.dx_fc2 = dx_plan(t.bf16, n, kC, kF, kC, w_al[1], p.rows16);
        p.dw_fc2 = dw_plan(t, DwShape{n, kC, kF, kC, kF, true}, p.rows16, p.rows16);
        p.dx_fc1 = dx_plan(t.bf16, n, kF, kC, kF, w_al[0], p.rows16);
        p.dw_fc1 = dw_plan(t, DwShape{n, kF, kC, kF, kC, true}, p.rows16, p.rows16);
        if (!p.rows16 || (p.gate == GateBwdForm::Sums && p.fc1 == LinearForm::StreamBf16Rows &&
                          p.fc2 == LinearForm::StreamBf16Rows && p.dx_fc2.route == DxRoute::Streamed &&
                          p.dx_fc1.route == DxRoute::Streamed && dw_wide(p.dw_fc2.form) && dw_wide(p.dw_fc1.form)))
            break;
    }
    return p;
}
// the IPA block's linear layers (w_al: q | kv | q_points | kv_points | linear_out); their rows are fp32 always
static IpaPlan plan_ipa(const Train& t, long n, const bool (&w_al)[5]) {
    IpaPlan p{};
    for (int j = 0; j < 4; ++j) {
        const int m = kIpaProjCols[j].m;
        p.proj[j] = linear_form(t.bf16, LinShape{n, m, kC, kC, kC, 0, true, w_al[j], false}, false);
        p.dx_proj[j] = dx_plan(t.bf16, n, m, kC, kIpaProj, w_al[j], false);
        p.dw_proj[j] = dw_plan(t, DwShape{n, m, kC, kIpaProj, kC, true}, false, false);
    }
    p.out = linear_form(t.bf16, LinShape{n, kC, kIpaFeat, kIpaFeat, kIpaFeat, 0, true, w_al[4], false}, false);
    p.dx_out = dx_plan(t.bf16, n, kC, kIpaFeat, kC, w_al[4], false);
    p.dw_out = dw_plan(t, DwShape{n, kC, kIpaFeat, kC, kIpaFeat, true}, false, false);
    return p;
}
// the final layer: D outputs per token
static FinalPlan plan_final(const Train& t, long n, int D, long tpg, bool w_al) {
    FinalPlan p{};
    p.lin = linear_form(t.bf16, LinShape{n, D, kC, kC, kC, 0, true, w_al, false}, false);
    p.dx = dx_plan(t.bf16, n, D, kC, D, w_al, false);
    p.dw = dw_plan(t, DwShape{n, D, kC, D, kC, true}, false, false);
    p.ln = ln_bwd_form(n, tpg, t.cpart_floats, true);
    return p;
}

// the operands of a weight gradient dW += dY^T X, db += colsum(dY) where the plan says the bias gradient rides along
static DwParams dw_op(const float* dy, int ldy, const float* x, int ldx, long n, int m, int k, float* dw, float* db, float* part,
                      const Train& t) {
    return DwParams{dy, ldy, x, ldx, n, m, 1, k, {dw, nullptr, nullptr}, {db, nullptr, nullptr}, part, t.part_floats};
}
// ... of a layer outside the sub-layers (embedders, adaLN heads, time embedder): planned where it is launched
static void step_dw_now(const Train& t, const DwParams& p, hipStream_t s) { launch_dw(p, dw_plan(t, dw_shape(p), false, false).form, s); }

// the weight W(col < m, kk < k) of ONE layer as a bf16 fragment stream in the scratch t.wt for the streamed forms (turned: the fp32
// matrix is [k][m], dX = dY W).  The scratch is reused by the next call on the stream.
static const unsigned char* wpack1(const Train& t, const float* w, int ld, int m, int k, int turned) {
    launch16_pack_wstream(&w, 1, turned ? k : m, ld, m, k, turned, t.wt, t.r.s);
    return (const unsigned char*)t.wt;
}

// ---- forward sub-layers with tape ---------------------------------------------------------------------------------
// LayerNorm + modulate of the residual stream into y, the stream's rows copied to the tape (h_in) -- with the previous sub-layer's
// pending gated update formed on the way when there is one (Train::Pending)
// y_bf16: y is stored as bf16 rows (the plan's rows16: it is only ever a GEMM operand)
static int ln_mod_tape(Train& t, const Rows& rw, float* y, float* h_in, bool y_bf16) {
    if (!t.pend.x) {
        launch32_ln_mod(rw.h, rw.nrows, rw.mm, rw.shift(), rw.scale(), 0, 1e-6f, y, t.r.s, h_in, y_bf16);
        return 0;
    }
    if (t.pend.nrows != rw.nrows)
        return fail(-7, "internal: pending gated update of %ld rows before a LayerNorm of %ld", t.pend.nrows, rw.nrows);
    launch32_gate_ln_mod(t.pend.x, t.pend.u, rw.nrows, t.pend.mm, t.pend.gate, rw.mm, rw.shift(), rw.scale(), 1e-6f, y, h_in, t.r.s, y_bf16);
    t.pend = Train::Pending{};
    return 0;
}
// the sub-layer's residual update h += gate * u, or its deferral (x = the sub-layer's taped input rows = the stream before it)
static void gated_update(Train& t, const Rows& rw, const float* x, const float* u) {
    if (t.defer_gate) t.pend = Train::Pending{x, u, rw.mm, rw.gate(), rw.nrows};
    else launch32_gated_add(rw.h, u, rw.nrows, rw.mm, rw.gate(), 1, t.r.s);
}
static void flush_pending(Train& t, float* h) {
    if (!t.pend.x) return;
    launch32_gated_sum(h, t.pend.x, t.pend.u, t.pend.nrows, t.pend.mm, t.pend.gate, t.r.s);
    t.pend = Train::Pending{};
}
static TrainAttnParams attn_op(const Train& t, const MhaW& m, const Rows& rw, const SubTapeAttn& tp) {
    TrainAttnParams a{};
    a.qkv = tp.qkv; a.ld = 3 * kC; a.ax = rw.ax; a.mk = rw.mk;
    a.bias_k = t.w(m.slot.bias_k); a.bias_v = t.w(m.slot.bias_v); a.inv_freq = t.c->inv_freq;
    a.out = tp.att; a.lse = tp.lse;
    return a;
}

static int attn_fwd_tape(Train& t, const MhaW& m, const Rows& rw, SubTapeAttn& tp) {
    const Run& r = t.r;
    const auto& p = m.slot;
    const long nrows = rw.nrows;
    const float* w3[3] = {t.w(p.q.w), t.w(p.k.w), t.w(p.v.w)};
    const float* b3[3] = {t.w(p.q.b), t.w(p.k.b), t.w(p.v.b)};
    const float* wo = t.w(p.o.w);
    const bool w_al[4] = {al16(w3[0]), al16(w3[1]), al16(w3[2]), al16(wo)};
    const AttnPlan& pl = tp.plan = plan_attn(t, nrows, rw.ax, rw.tpg(), w_al);
    if (int e = ln_mod_tape(t, rw, tp.y, tp.h_in, pl.rows16)) return e;     // y (taped), and the tape's copy of h
    const float qscale = 1.0f / std::sqrt((float)kDH);
    if (pl.qkv_one_pass) {   // bf16 operands: one pass over y, c[n][j kC + i] = (y . w3[j][i] + b3[j][i]) * scale[j]
        LinearParams q = lin_op(tp.y, kC, w3[0], kC, nullptr, nrows, 3 * kC, kC, tp.qkv, 3 * kC);
        q.seg_cols = kC;
        for (int j = 0; j < 3; ++j) { q.w_seg[j] = w3[j]; q.bias_seg[j] = b3[j]; q.scale_seg[j] = j == 0 ? qscale : 1.0f; }
        if (linear_streams(pl.qkv[0])) {   // ... the three weights as one fragment stream (k_wide16.hip)
            launch16_pack_wstream(w3, 3, kC, kC, 3 * kC, kC, 0, t.wt, r.s);
            q.wpack = (const unsigned char*)t.wt;
        }
        step_linear(q, pl.qkv[0], r.s);
    } else {
        for (int j = 0; j < 3; ++j) {
            LinearParams q = lin_op(tp.y, kC, w3[j], kC, b3[j], nrows, kC, kC, tp.qkv, 3 * kC);
            q.col0 = j * kC;
            if (j == 0) { q.mode = kLinScaled; q.scalar = qscale; }
            step_linear(q, pl.qkv[j], r.s);
        }
    }
    // (the sequence-resident bf16-operand kernels rotate q, k while they convert them: no RoPE pass, the tape keeps them unrotated)
    // (position of a token on the axis: (token / pos_stride) % len)
    if (pl.attn != TrainAttnForm::SeqRope) launch32_rope(tp.qkv, nrows, 3 * kC, rw.ax.pos_stride, rw.ax.len, t.c->inv_freq, r.s);
    launch_train_attn(attn_op(t, m, rw, tp), pl.attn, r.s);
    // (the gated residual as an epilogue of this product, with u kept at a second address, was measured: the store phase is
    // what bounds the wide kernels, and the heavier epilogue cost 1.5 ms per step where the separate pass costs 1.3)
    LinearParams o = lin_op(tp.att, kC, wo, kC, t.w(p.o.b), nrows, kC, kC, tp.u, kC);
    if (linear_streams(pl.out)) o.wpack = wpack1(t, wo, kC, kC, kC, 0);
    step_linear(o, pl.out, r.s);
    gated_update(t, rw, tp.h_in, tp.u);
    LAUNCHCHK();
    return 0;
}

static int mlp_fwd_tape(Train& t, const FfnW& f, const Rows& rw, SubTapeMlp& tp) {
    const Run& r = t.r;
    const long nrows = rw.nrows;
    const float *w1 = t.w(f.slot.fc1.w), *w2 = t.w(f.slot.fc2.w);
    const bool w_al[2] = {al16(w1), al16(w2)};
    const MlpPlan& pl = tp.plan = plan_mlp(t, nrows, rw.tpg(), w_al);
    if (int e = ln_mod_tape(t, rw, tp.y, tp.h_in, pl.rows16)) return e;     // y (taped), and the tape's copy of h
    LinearParams fc1 = lin_op(tp.y, kC, w1, kC, t.w(f.slot.fc1.b), nrows, kF, kC, tp.pre, kF);
    fc1.mode = kLinStoreGelu;
    fc1.c2 = tp.hid;               // hid = gelu(pre), as bf16 rows with the plan's rows16
    fc1.c2_bf16 = pl.rows16;
    if (linear_streams(pl.fc1)) fc1.wpack = wpack1(t, w1, kC, kF, kC, 0);
    step_linear(fc1, pl.fc1, r.s);
    LinearParams fc2 = lin_op(tp.hid, kF, w2, kF, t.w(f.slot.fc2.b), nrows, kC, kF, tp.u, kC);
    if (linear_streams(pl.fc2)) fc2.wpack = wpack1(t, w2, kF, kC, kF, 0);
    step_linear(fc2, pl.fc2, r.s);
    gated_update(t, rw, tp.h_in, tp.u);
    LAUNCHCHK();
    return 0;
}

// W^T of one weight [rows][cols] (nseg = 1) or of three [rows][cols] weights side by side (row stride 3 * rows): the image computed
// ahead (Train::tr_*), else a launch in place into t.wt
static const float* turned(Train& t, const float* const* w, int nseg, int rows, int cols) {
    hipStream_t s = t.r.s;
    if (t.tr_use && t.tr_cursor < t.c->tr_plan.size()) {
        const mdgen_ctx::TurnReq& q = t.c->tr_plan[t.tr_cursor];
        bool same = q.nseg == nseg && q.rows == rows && q.cols == cols;
        for (int j = 0; j < nseg && same; ++j) same = q.w[j] == w[j];
        if (same) {
            if (!t.tr_waited) {
                (void)hipStreamWaitEvent(s, t.tr_done, 0);
                t.tr_waited = true;
            }
            ++t.tr_cursor;
            return t.c->tr_buf + q.off;
        }
        t.tr_use = false;            // the call differs from the recorded one: in place from here on, and record anew
        t.c->tr_plan_ok = false;
    }
    if (t.tr_record) {
        mdgen_ctx::TurnReq q{{w[0], nseg > 1 ? w[1] : nullptr, nseg > 2 ? w[2] : nullptr}, nseg, rows, cols, 0};
        t.tr_new.push_back(q);
    }
    for (int j = 0; j < nseg; ++j) launch32_transpose(w[j], rows, cols, t.wt + (size_t)j * rows, s, nseg * rows);
    return t.wt;
}

// ---- backward helpers ---------------------------------------------------------------------------------------------
// dX = dY W of nseg layers W_j [mseg][K] whose dY sit side by side (M = nseg mseg), along the plan's route.  q: the product's
// operands but for the weight (a = dY, lda, n, c = dX, ldc, mode and its operands)
static void step_dx(Train& t, LinearParams q, const float* const* w, int nseg, int mseg, int K, const DxPlan& pl) {
    const int M = nseg * mseg;
    q.m = K; q.k = M; q.w = w[0]; q.ldw = M;
    if (pl.route == DxRoute::Streamed) {
        launch16_pack_wstream(w, nseg, mseg, K, K, M, 1, t.wt, t.r.s);
        q.wpack = (const unsigned char*)t.wt;
    } else if (pl.route == DxRoute::TurnedWeight) {
        q.w = turned(t, w, nseg, mseg, K);
    } else {
        q.ldw = K; q.wtrans = 1;
    }
    step_linear(q, pl.form, t.r.s);
}
// The backward of y = x W^T + b (the layer `lin`, W [M][K]):  dx (store / accumulate) = dy W;  dW += dy^T x;  db += colsum(dy)
struct LinBwdOp {
    const float* dy; int ldy;        // dY [n][M]
    const float* x; int ldx;         // the layer's input [n][K]
    float* dx; int ldx_out;          // dX [n][K]
    bool accumulate;                 // dx += (the layer shares its input with the one before)
    const float* gelu_pre;           // non-null: dx = (dy W) * gelu'(gelu_pre) (same shape and row stride as dx; not with accumulate)
    bool dx_bf16;                    // ... written as bf16 rows
    bool main_stream;                // dy is a buffer the main stream goes on updating in place (the IPA block's ungated residual):
                                     // the weight gradient stays on the main stream
};
static int lin_bwd(Train& t, const Lin& lin, long n, int M, int K, const DxPlan& dxp, const DwPlan& dwp, const LinBwdOp& o) {
    const float* W = t.w(lin.w);
    // dW / db: second stream (dy and x are complete at this point of the main stream)
    float* gb = t.grad(lin.b);
    float* gw = t.grad(lin.w);
    Train::Fork f;
    if (int e = t.fork((gw || gb) && !o.main_stream, &f)) return e;
    LinearParams q = lin_op(o.dy, o.ldy, nullptr, 0, nullptr, n, K, M, o.dx, o.ldx_out);
    q.mode = o.gelu_pre ? kLinGeluBwd : o.accumulate ? kLinAccumulate : kLinStore;
    q.c2 = const_cast<float*>(o.gelu_pre);
    q.c_bf16 = o.dx_bf16;
    step_dx(t, q, &W, 1, M, K, dxp);
    // (dY stored as bf16 rows: only the wide pass reads them, so a bias gradient wanted alone takes that pass too, as q | k | v's does)
    const bool pass = gw || (gb && dw_dy_bf16(dwp.form));
    if (pass) launch_dw(dw_op(o.dy, o.ldy, o.x, o.ldx, n, M, K, gw, gb, f.part, t), dwp.form, f.s);
    if (gb && !(pass && dwp.bias_rides)) launch32_colsum(o.dy, o.ldy, nullptr, 0, nullptr, 0, n, M, n, 0.f, gb, 0, f.cpart, t.cpart_floats, f.s);
    LAUNCHCHK();
    return 0;
}

// gated residual h_out = h_in + gate * u:  du = gate * dh (into t.du; du16: as bf16 rows -- it is only ever the token operand of the
// dX product and dY of the weight gradient of the sub-layer's last linear layer);  dgate[g] += sum_t dh * u
static void gate_bwd(const Train& t, GateBwdForm form, const Rows& rw, const float* dh, const float* u, bool du16) {
    launch32_gate_bwd(GateBwdParams{dh, u, rw.nrows, rw.mm, rw.gate(), t.du, du16, rw.tpg(), rw.dmod + rw.gate() * kC, (long)t.c->modrow,
                                    t.cpart, t.cpart_floats}, form, t.r.s);
}
// LN + modulate backward: dshift[g] += sum dy; dscale[g] += sum dy * xhat; dh (+)= LN'(dy * (1 + scale))
static void lnmod_bwd(const Train& t, LnBwdForm form, const Rows& rw, const float* h_in, const float* dy, float* dh, bool accumulate) {
    launch32_ln_mod_bwd(LnBwdParams{h_in, dy, rw.nrows, rw.mm, rw.scale(), 1e-6f, dh, accumulate ? 1 : 0, rw.tpg(),
                                    rw.dmod + rw.shift() * kC, rw.dmod + rw.scale() * kC, (long)t.c->modrow, t.cpart, t.cpart_floats}, form, t.r.s);
}

// backward of one MLP sub-layer; dh is updated in place (dh_in = dh_out + ...)
static int mlp_bwd(Train& t, const FfnW& f, const Rows& rw, float* dh, const SubTapeMlp& tp) {
    const MlpPlan& pl = tp.plan;   // hid, y, du = gate * dh and d pre as bf16 rows (rows16), or all of them fp32
    const long nrows = rw.nrows;
    if (int e = t.begin_sub()) return e;
    gate_bwd(t, pl.gate, rw, dh, tp.u, pl.rows16);   // t.du = gate * dh
    LinBwdOp fc2{};   // d pre = (du W2) * gelu'(pre) into t.dhid: the GELU derivative is the epilogue of the dX product
    fc2.dy = t.du; fc2.ldy = kC;
    fc2.x = tp.hid; fc2.ldx = kF;
    fc2.dx = t.dhid; fc2.ldx_out = kF;
    fc2.gelu_pre = tp.pre; fc2.dx_bf16 = pl.rows16;
    if (int e = lin_bwd(t, f.slot.fc2, nrows, kC, kF, pl.dx_fc2, pl.dw_fc2, fc2)) return e;
    LinBwdOp fc1{};   // t.dy = d pre W1
    fc1.dy = t.dhid; fc1.ldy = kF;
    fc1.x = tp.y; fc1.ldx = kC;
    fc1.dx = t.dy; fc1.ldx_out = kC;
    if (int e = lin_bwd(t, f.slot.fc1, nrows, kF, kC, pl.dx_fc1, pl.dw_fc1, fc1)) return e;
    lnmod_bwd(t, pl.ln, rw, tp.h_in, t.dy, dh, true);
    LAUNCHCHK();
    return t.end_sub();
}

// backward of one attention sub-layer
static int attn_bwd(Train& t, const MhaW& m, const Rows& rw, float* dh, const SubTapeAttn& tp) {
    hipStream_t s = t.r.s;
    const long nrows = rw.nrows;
    const AxisMap& ax = rw.ax;
    const auto& p = m.slot;
    const AttnPlan& pl = tp.plan;   // (as attn_fwd_tape stored the tape: y as bf16 rows or fp32, q and k rotated or not)
    if (int e = t.begin_sub()) return e;
    gate_bwd(t, pl.gate, rw, dh, tp.u, pl.rows16);   // t.du
    LinBwdOp o{};   // t.dy = d att = du Wo
    o.dy = t.du; o.ldy = kC;
    o.x = tp.att; o.ldx = kC;
    o.dx = t.dy; o.ldx_out = kC;
    if (int e = lin_bwd(t, p.o, nrows, kC, kC, pl.dx_out, pl.dw_out, o)) return e;
    TrainAttnParams a = attn_op(t, m, rw, tp);
    a.dout = t.dy; a.dqkv = t.dqkv; a.stats = t.stats; a.dbias = t.dbias;
    a.dqkv_bf16 = pl.dqkv16;       // the sequence-resident kernels write dq | dk | dv as bf16 rows
    launch_train_attn_bwd(a, pl.attn, s);
    // bias key / value: rows [seq][dk: head x 24 | dv: head x 24] summed over sequences = the (1, 1, C) tensors
    {
        float *gk = t.grad(p.bias_k), *gv = t.grad(p.bias_v);
        Train::Fork f;
        if (int e = t.fork(gk || gv, &f)) return e;
        if (gk) launch32_colsum(t.dbias, 2 * kC, nullptr, 0, nullptr, 0, ax.nseq, kC, ax.nseq, 0.f, gk, 0, f.cpart, t.cpart_floats, f.s);
        if (gv) launch32_colsum(t.dbias + kC, 2 * kC, nullptr, 0, nullptr, 0, ax.nseq, kC, ax.nseq, 0.f, gv, 0, f.cpart, t.cpart_floats, f.s);
    }
    if (pl.attn == TrainAttnForm::Exact)    // (the bf16-operand attention backward stores dq, dk already taken back through RoPE)
        launch32_rope_bwd(t.dqkv, nrows, 3 * kC, ax.pos_stride, ax.len, t.c->inv_freq, 1.0f / std::sqrt((float)kDH), s);
    const Lin l3[3] = {p.q, p.k, p.v};
    if (t.bf16) {
        // q | k | v as one layer of 1152 outputs: dy = dqkv [Wq; Wk; Wv] (one product with the contraction over all three,
        // the weights streamed or turned side by side into the scratch), dW and db of all three from one pass over (dqkv, y)
        const float* w3[3] = {t.w(p.q.w), t.w(p.k.w), t.w(p.v.w)};
        DwParams g = dw_op(t.dqkv, 3 * kC, tp.y, kC, nrows, kC, kC, nullptr, nullptr, t.part, t);
        g.nseg = 3;
        bool want_g = false, want_b = false;
        for (int j = 0; j < 3; ++j) {
            g.dw[j] = t.grad(l3[j].w); g.db[j] = t.grad(l3[j].b);
            want_g = want_g || g.dw[j] || g.db[j];
            want_b = want_b || g.db[j];
        }
        Train::Fork f;                                 // (dqkv, y) are complete: the gradients go to the second stream
        if (int e = t.fork(want_g, &f)) return e;
        g.part = f.part;
        step_dx(t, lin_op(t.dqkv, 3 * kC, nullptr, 0, nullptr, nrows, 0, 0, t.dy, kC), w3, 3, kC, kC, pl.dx_qkv);
        if (want_g) {
            launch_dw(g, pl.dw_qkv.form, f.s);
            for (int j = 0; j < 3 && !(want_b && pl.dw_qkv.bias_rides); ++j)
                if (g.db[j])
                    launch32_colsum(t.dqkv + j * kC, 3 * kC, nullptr, 0, nullptr, 0, nrows, kC, nrows, 0.f, g.db[j], 0, f.cpart,
                                    t.cpart_floats, f.s);
        }
        LAUNCHCHK();
    } else {
        for (int j = 0; j < 3; ++j) {   // t.dy = dq Wq + dk Wk + dv Wv
            LinBwdOp q{};
            q.dy = t.dqkv + j * kC; q.ldy = 3 * kC;
            q.x = tp.y; q.ldx = kC;
            q.dx = t.dy; q.ldx_out = kC; q.accumulate = j > 0;
            if (int e = lin_bwd(t, l3[j], nrows, kC, kC, pl.dx_qkv, pl.dw_qkv, q)) return e;
        }
    }
    lnmod_bwd(t, pl.ln, rw, tp.h_in, t.dy, dh, true);
    LAUNCHCHK();
    return t.end_sub();
}

// backward of the IPA block of layer i:  x_out = x_in + linear_out(ipa(LN_affine(x_in)))   (latent_model.py:373)
static int ipa_block_bwd(Train& t, const IpaW& w, const SubTapeIpa& tp, const IpaStream& st) {
    const Run& r = t.r;
    hipStream_t s = r.s;
    const auto& p = w.slot;
    const IpaPlan& pl = tp.plan;
    const long Mp = r.Mp;
    float* dhi = st.dh;
    if (int e = t.begin_sub()) return e;
    float* dfeat = t.dhid;                    // [Mp][256]
    float* dproj = t.dqkv;                    // [Mp][672]
    float* dhw = t.stats;                     // [Mp][4]
    float* qrec = t.act;                      // [Mp][4][49]
    // linear_out (ungated residual: d u = d x_out)
    // (its dY is the residual stream's gradient itself, which this block updates in place below: main stream)
    LinBwdOp o{};
    o.dy = dhi; o.ldy = kC;
    o.x = tp.feat; o.ldx = kIpaFeat;
    o.dx = dfeat; o.ldx_out = kIpaFeat;
    o.main_stream = true;
    if (int e = lin_bwd(t, p.out, Mp, kC, kIpaFeat, pl.dx_out, pl.dw_out, o)) return e;
    IpaAttnParams ap{};
    ap.proj = tp.proj; ap.rot = st.rot; ap.trans = st.trans;
    ap.mask_bl = mask_ipa(r).mask;
    ap.head_w = w.head_w; ap.feat = nullptr; ap.feat32 = tp.feat; ap.stats = tp.stats;
    ap.ngroups = r.B; ap.B = r.B; ap.L = r.L;
    launch32_ipa_bwd(ap, dfeat, dproj, dhw, qrec, t.grad(p.head_w), s, t.part, t.part_floats);
    LAUNCHCHK();
    // the four input projections of xn = LN_affine(x_in): t.dy = sum_j dproj_j W_j
    launch32_ln_mod(tp.h_in, Mp, mod_affine(w.gamma_beta), 1, 0, 1, 1e-5f, t.ytmp, s, nullptr, false);
    const Lin lins[4] = {p.q, p.kv, p.q_points, p.kv_points};
    for (int j = 0; j < 4; ++j) {
        LinBwdOp q{};
        q.dy = dproj + kIpaProjCols[j].col0; q.ldy = kIpaProj;
        q.x = t.ytmp; q.ldx = kC;
        q.dx = t.dy; q.ldx_out = kC; q.accumulate = j > 0;
        if (int e = lin_bwd(t, lins[j], Mp, kIpaProjCols[j].m, kC, pl.dx_proj[j], pl.dw_proj[j], q)) return e;
    }
    // affine LayerNorm (eps 1e-5): d gamma = sum dy * xhat, d beta = sum dy, d x
    if (float* g = t.grad(p.norm.w))
        launch32_colsum(t.dy, kC, tp.h_in, kC, nullptr, 2, Mp, kC, Mp, 1e-5f, g, 0, t.cpart, t.cpart_floats, s);
    if (float* g = t.grad(p.norm.b))
        launch32_colsum(t.dy, kC, nullptr, 0, nullptr, 0, Mp, kC, Mp, 0.f, g, 0, t.cpart, t.cpart_floats, s);
    launch32_ln_bwd(tp.h_in, t.dy, Mp, mod_affine(w.gamma_beta), 0, 1, 1e-5f, dhi, 1, s);
    LAUNCHCHK();
    return t.end_sub();
}

// ---- the phases of the step -----------------------------------------------------------------------------------------
// the streams' operands beyond what carve_train gives them: rows, embedder, frames
static void bind_ipa_streams(Train& t) {
    const Run& r = t.r;
    const mdgen_ctx* c = t.c;
    IpaStream& a = t.st[0];
    a.h = (float*)(r.ws + r.lay.ipa_out);   // IPA-stack residual stream [B*L][384] (G = B groups)
    a.rot = r.start_rot; a.trans = r.start_trans;
    a.w7 = a.b7 = nullptr;
    a.rel7 = Lin{};
    if (t.nst == 2) {   // the x_r stream runs on the start frames, the x_f stream on the end frames (latent_model.py:203-205)
        a.w7 = c->wr7; a.b7 = c->br7; a.rel7 = c->slot.rel_r;
        IpaStream& b = t.st[1];
        b.h = (float*)(r.ws + r.lay.h_ipa);
        b.rot = r.end_rot; b.trans = r.end_trans;
        b.w7 = c->wf7; b.b7 = c->bf7; b.rel7 = c->slot.rel_f;
    }
}

// the second stream of the call (option train_streams = 2)
static int open_side_stream(Train& t) {
    mdgen_ctx* c = t.c;
    // (same priority as the caller's stream: with the second stream at the lowest OR the highest priority of the device's range
    // the step took 53 / 60 ms instead of 30.7 -- profiles/r04_experiments.txt)
    // (default stream priority: created with ANY other priority -- lowest or highest -- the step takes 51-54 ms instead of 27.4:
    // profiles/r06_experiments.txt #19)
    if (c->opt_train_streams == 2 && !c->train_side) HIPCHK(hipStreamCreateWithFlags(&c->train_side, hipStreamNonBlocking));
    t.side = c->opt_train_streams == 2 ? c->train_side : nullptr;
    return 0;
}

// Turned weights, start of the call (Train::tr_*): every image the previous call recorded, on the second stream beside the forward
// pass; without a usable list this call records one.  `caller`: the stream on which the weights are final.
static int prefetch_turned(Train& t, hipStream_t caller) {
    mdgen_ctx* c = t.c;
    if (!t.side || !t.bf16) return 0;
    if (!(c->tr_plan_ok && c->tr_buf)) {
        t.tr_record = true;
        return 0;
    }
    hipEvent_t e0 = t.next_event(), e1 = t.next_event();
    if (e0 && e1) {
        HIPCHK(hipEventRecord(e0, caller));
        HIPCHK(hipStreamWaitEvent(t.side, e0, 0));
        for (const mdgen_ctx::TurnReq& q : c->tr_plan)
            for (int j = 0; j < q.nseg; ++j)
                launch32_transpose(q.w[j], q.rows, q.cols, c->tr_buf + q.off + (size_t)j * q.rows, t.side, q.nseg * q.rows);
        HIPCHK(hipEventRecord(e1, t.side));
        t.tr_done = e1;
        t.tr_use = true;
    }
    return 0;
}
// ... end of the call: a list that was not used up is recorded anew by the next call; a recorded one becomes the next call's list
static void finish_turned(Train& t) {
    mdgen_ctx* c = t.c;
    if (t.tr_use && t.tr_cursor != c->tr_plan.size()) c->tr_plan_ok = false;
    if (!t.tr_record) return;
    size_t off = 0;
    for (mdgen_ctx::TurnReq& q : t.tr_new) {
        q.off = off;
        off += ((size_t)q.nseg * q.rows * q.cols + 63) & ~(size_t)63;
    }
    bool ok = !t.tr_new.empty();
    if (ok && off > c->tr_buf_floats) {
        if (c->tr_buf) (void)hipFree(c->tr_buf);
        c->tr_buf = nullptr;
        c->tr_buf_floats = 0;
        if (hipMalloc((void**)&c->tr_buf, off * 4) == hipSuccess) c->tr_buf_floats = off;
        else { (void)hipGetLastError(); ok = false; }
    }
    c->tr_plan = t.tr_new;
    c->tr_plan_ok = ok;
}

// Join on EVERY exit path: whatever this call has launched on the second stream is ordered before what the caller enqueues next
// on its own stream -- also when the call returns an error half-way (a caller that then zeroes or reuses `grads` or the tape
// must not race with gradient kernels still running over there).  The error path's own HIP status is not reported twice.
struct Join {
    Train& t;
    bool done = false;
    int run() {
        if (done || !t.side) return 0;
        done = true;
        hipEvent_t e = t.next_event();
        if (!e) {   // no event to be had: fall back to a host-side wait for the second stream
            (void)hipStreamSynchronize(t.side);
            return 0;
        }
        if (hipEventRecord(e, t.side) != hipSuccess || hipStreamWaitEvent(t.r.s, e, 0) != hipSuccess) (void)hipStreamSynchronize(t.side);
        return 0;
    }
    ~Join() { (void)run(); }
};

// one pass of the IPA stack over the stream's rows on its frames, taped
static int ipa_forward(Train& t, IpaStream& st) {
    const Run& r = t.r;
    const mdgen_ctx* c = t.c;
    hipStream_t s = r.s;
    launch_ipa_init(c->aa_emb, r.aatype, st.rel, st.w7, st.b7, st.h, r.B, r.B, r.L, s);
    for (int i = 0; i < c->nl; ++i) {
        const IpaW& w = c->ipa[i];
        const auto& p = w.slot;
        const IpaSites site = ipa_sites(r, i, st.h, t.dmod);
        SubTapeIpa& tp = st.ip[i];
        const bool w_al[5] = {al16(t.w(p.q.w)), al16(t.w(p.kv.w)), al16(t.w(p.q_points.w)), al16(t.w(p.kv_points.w)), al16(t.w(p.out.w))};
        const IpaPlan& pl = tp.plan = plan_ipa(t, r.Mp, w_al);
        HIPCHK(hipMemcpyAsync(tp.h_in, st.h, (size_t)r.Mp * kC * 4, hipMemcpyDeviceToDevice, s));
        // (few groups: the attention's key loop is sliced over workgroups, with t.part as its scratch)
        const IpaBlockOp o{f32_bufs(r).y, tp.proj, tp.feat, tp.stats, t.part, t.part_floats,
                           {pl.proj[0], pl.proj[1], pl.proj[2], pl.proj[3]}, pl.out};
        if (int e = ipa_block_fp32(r, w, st.h, st.rot, st.trans, o)) return e;
        if (int e = attn_fwd_tape(t, w.mha_l, site.attn, st.il[i])) return e;
        if (int e = mlp_fwd_tape(t, w.ffn, site.mlp, st.im[i])) return e;
    }
    return 0;
}

// forward (fp32 path, with tape): tables, the IPA streams, token embedding, trunk, final layer and loss
static int train_forward(Train& t) {
    const Run& r = t.r;
    mdgen_ctx* c = t.c;
    hipStream_t s = r.s;
    const long N = r.N, Mp = r.Mp, TL = (long)r.T * r.L;
    {   // time embedding, adaLN table, compact mask  (as prepare(), per-sample t)
        float* silu = (float*)(r.ws + r.lay.silu_t);
        launch_temb(t.tvals, r.B, c->d.time_multiplier, c->t_w0, c->t_b0, c->t_w2, c->t_b2, silu, s);
        launch_adaln(silu, r.B, c->ada_w, c->ada_b, c->modrow, r.mod(), s);
        HIPCHK(hipMemcpy2DAsync(r.ws + r.lay.mask_bl, (size_t)r.L * 4, r.mask, (size_t)r.T * r.L * 4, (size_t)r.L * 4, r.B,
                                hipMemcpyDeviceToDevice, s));
        LAUNCHCHK();
    }
    if (t.nst == 2) {
        // x_f = (start^-1 o end).to_tensor_7(), x_r = (end^-1 o start).to_tensor_7()   (latent_model.py:194-195)
        if (r.rel7_in) {   // the caller's own to_tensor_7() outputs (quaternion sign as the reference's eigh chose it)
            HIPCHK(hipMemcpyAsync(t.rel7, r.rel7_in, (size_t)2 * Mp * 7 * 4, hipMemcpyDeviceToDevice, s));
        } else {
            launch_rel7(r.start_rot, r.start_trans, r.end_rot, r.end_trans, t.rel7, Mp, s);
            launch_rel7(r.end_rot, r.end_trans, r.start_rot, r.start_trans, t.rel7 + Mp * 7, Mp, s);
            LAUNCHCHK();
        }
    }
    for (int k = 0; k < t.nst; ++k)
        if (int e = ipa_forward(t, t.st[k])) return e;
    float* hi = t.st[0].h;
    if (t.nst == 2) {
        launch_add_inplace(hi, t.st[1].h, Mp * kC, s);
        LAUNCHCHK();
    }
    float* h = r.h();
    launch_embed(embed_op(r, t.xt, hi), s);
    LAUNCHCHK();
    t.defer_gate = true;   // the trunk's residual updates ride in the next sub-layer's LayerNorm launch
    for (int i = 0; i < c->nl; ++i) {
        const TrunkW& w = c->trunk[i];
        const TrunkSites site = trunk_sites(r, i, 0, t.dmod);
        if (int e = attn_fwd_tape(t, w.mha_l, site.l, t.tl[i])) return e;
        if (int e = attn_fwd_tape(t, w.mha_t, site.t, t.tt[i])) return e;
        if (int e = mlp_fwd_tape(t, w.ffn, site.mlp, t.tm[i])) return e;
    }
    t.defer_gate = false;
    flush_pending(t, h);
    LAUNCHCHK();
    const Rows fs = final_site(r, 0, t.dmod);
    t.fin = plan_final(t, N, r.D, fs.tpg(), al16(t.w(c->slot.fin.w)));
    launch32_ln_mod(h, N, fs.mm, fs.shift(), fs.scale(), 0, 1e-6f, f32_bufs(r).y, s, nullptr, false);
    step_linear(lin_op(f32_bufs(r).y, kC, t.w(c->slot.fin.w), kC, t.w(c->slot.fin.b), N, r.D, kC, t.pred, r.D), t.fin.lin, s);
    launch_masked_mse(t.pred, t.target, t.loss_mask, t.loss, TL * r.D, r.B, s, t.cpart, t.cpart_floats);
    LAUNCHCHK();
    return 0;
}

// adaLN head of one parameter block: mod[b] = W_ada silu_t[b] + b_ada  (its d mod rows are complete once the
// block's own backward is done)
static int ada_head_bwd(Train& t, const Lin& ada, int off, int rows) {
    const Run& r = t.r;
    const float* silu = (const float*)(r.ws + r.lay.silu_t);
    const int modld = (int)t.c->modrow;
    float *gw = t.grad(ada.w), *gb = t.grad(ada.b);
    Train::Fork f;   // (the block's d mod rows are complete here and nothing writes them again)
    if (int e = t.fork(gw || gb, &f)) return e;
    if (gw) step_dw_now(t, dw_op(t.dmod + off, modld, silu, kC, r.B, rows, kC, gw, nullptr, f.part, t), f.s);
    if (gb) launch32_colsum(t.dmod + off, modld, nullptr, 0, nullptr, 0, r.B, rows, r.B, 0.f, gb, 0, f.cpart, t.cpart_floats, f.s);
    return 0;
}

// final layer: out = linear(modulate(LN(h)))
static int final_bwd(Train& t) {
    const Run& r = t.r;
    const mdgen_ctx* c = t.c;
    hipStream_t s = r.s;
    const long N = r.N, TL = (long)r.T * r.L;
    float* h = r.h();
    const Rows fs = final_site(r, 0, t.dmod);
    if (int e = t.begin_sub()) return e;
    float* dpred = t.dqkv;   // [N][D] fits the (idle) dqkv scratch
    launch32_loss_grad(t.pred, t.target, t.loss_mask, TL * r.D, r.B, t.dsilu, dpred, s, t.cpart, t.cpart_floats);   // t.dsilu[0..B) = mask sums (scratch)
    launch32_ln_mod(h, N, fs.mm, fs.shift(), fs.scale(), 0, 1e-6f, t.ytmp, s, nullptr, false);
    LinBwdOp o{};   // t.dy = d pred W
    o.dy = dpred; o.ldy = r.D;
    o.x = t.ytmp; o.ldx = kC;
    o.dx = t.dy; o.ldx_out = kC;
    if (int e = lin_bwd(t, c->slot.fin, N, r.D, kC, t.fin.dx, t.fin.dw, o)) return e;
    lnmod_bwd(t, t.fin.ln, fs, h, t.dy, t.dh, false);
    if (int e = ada_head_bwd(t, c->slot.fin_ada, c->final_off(), 2 * kC)) return e;
    LAUNCHCHK();
    if (int e = t.end_sub()) return e;
    return t.mark();
}

// token embedding (latent_model.py:233-246): h0 = Wl x + bl [+ pos] + Wc x_cond + bc + mask_emb[cm] + ipa_out[b, l]
static int embed_bwd(Train& t) {
    const Run& r = t.r;
    const mdgen_ctx* c = t.c;
    hipStream_t s = r.s;
    const long N = r.N;
    {   // (t.dh is final here: second stream)
        Train::Fork f;
        if (int e = t.fork(true, &f)) return e;
        if (float* g = t.grad(c->slot.latent.w)) step_dw_now(t, dw_op(t.dh, kC, t.xt, r.D, N, kC, r.D, g, nullptr, f.part, t), f.s);
        if (float* g = t.grad(c->slot.cond.w)) step_dw_now(t, dw_op(t.dh, kC, r.x_cond, r.D, N, kC, r.D, g, nullptr, f.part, t), f.s);
        if (float* g = t.grad(c->slot.latent.b)) launch32_colsum(t.dh, kC, nullptr, 0, nullptr, 0, N, kC, N, 0.f, g, 0, f.cpart, t.cpart_floats, f.s);
        if (float* g = t.grad(c->slot.cond.b)) launch32_colsum(t.dh, kC, nullptr, 0, nullptr, 0, N, kC, N, 0.f, g, 0, f.cpart, t.cpart_floats, f.s);
    }
    if (float* g = t.grad(c->slot.mask)) {
        float* ind0 = t.stats;          // [N] + [N] floats fit the stats scratch (N * 32 floats)
        float* ind1 = t.stats + N;
        launch32_indicator(r.x_cond_mask, N, ind0, ind1, s);
        launch32_colsum(t.dh, kC, nullptr, 0, ind0, 3, N, kC, N, 0.f, g, 0, t.cpart, t.cpart_floats, s);
        launch32_colsum(t.dh, kC, nullptr, 0, ind1, 3, N, kC, N, 0.f, g + kC, 0, t.cpart, t.cpart_floats, s);
    }
    launch32_sum_frames(t.dh, r.B, r.T, r.L, t.st[0].dh, s);    // d ipa_out
    LAUNCHCHK();
    return t.mark();
}

// one pass of the IPA stack backwards.  last: the stream after which a layer's gradients are complete -- it runs the adaLN
// heads and the milestones (the two-sided model's first stream leaves every layer's gradients half done)
static int ipa_backward(Train& t, const IpaStream& st, bool last) {
    const Run& r = t.r;
    const mdgen_ctx* c = t.c;
    hipStream_t s = r.s;
    const long Mp = r.Mp;
    for (int i = c->nl - 1; i >= 0; --i) {
        const IpaW& w = c->ipa[i];
        const IpaSites site = ipa_sites(r, i, st.h, t.dmod);
        if (int e = mlp_bwd(t, w.ffn, site.mlp, st.dh, st.im[i])) return e;
        if (int e = attn_bwd(t, w.mha_l, site.attn, st.dh, st.il[i])) return e;
        if (int e = ipa_block_bwd(t, w, st.ip[i], st)) return e;
        if (last) {
            if (int e = ada_head_bwd(t, w.slot.ada, c->ipa_off(i), 6 * kC)) return e;
            LAUNCHCHK();
            if (int e = t.mark()) return e;
        }
    }
    // stack input: aatype_to_emb[aatype] (+ latent_to_emb_{f,r}(rel7))
    if (float* g = t.grad(c->slot.aatype)) launch32_embed_rows_bwd(st.dh, r.aatype, r.B, r.B, r.L, g, s);
    if (st.rel) {
        if (float* g = t.grad(st.rel7.w)) step_dw_now(t, dw_op(st.dh, kC, st.rel, 7, Mp, kC, 7, g, nullptr, t.part, t), s);
        if (float* g = t.grad(st.rel7.b)) launch32_colsum(st.dh, kC, nullptr, 0, nullptr, 0, Mp, kC, Mp, 0.f, g, 0, t.cpart, t.cpart_floats, s);
    }
    LAUNCHCHK();
    return 0;
}

// the time embedder behind all adaLN heads: d silu_t = d mod . W_ada
static int time_embedder_bwd(Train& t) {
    const Run& r = t.r;
    const mdgen_ctx* c = t.c;
    hipStream_t s = r.s;
    const int modld = (int)c->modrow;
    float* dst = t.dsilu;                         // [B][384]
    float* emb = dst + (size_t)r.B * kC;          // [B][256]
    float* h1 = emb + (size_t)r.B * 256;          // [B][384]
    float* dp1 = h1 + (size_t)r.B * kC;
    float* dp2 = dp1 + (size_t)r.B * kC;
    if (!launch32_skinny_wt(t.dmod, modld, c->ada_w, kC, r.B, kC, c->modrow, dst, t.cpart, t.cpart_floats, s)) {
        LinearParams q = lin_op(t.dmod, modld, c->ada_w, kC, nullptr, r.B, kC, c->modrow, dst, kC);
        q.wtrans = 1;   // (W_ada as stored)
        step_linear(q, linear_form(t.bf16, LinShape{q.n, q.m, q.k, q.lda, q.ldw, 1, true, true, false}, false), s);
    }
    launch32_temb_bwd(t.tvals, r.B, c->d.time_multiplier, c->t_w0, c->t_b0, c->t_w2, c->t_b2, dst, emb, h1, dp1, dp2, s);
    if (float* g = t.grad(c->slot.t2.w)) step_dw_now(t, dw_op(dp2, kC, h1, kC, r.B, kC, kC, g, nullptr, t.part, t), s);
    if (float* g = t.grad(c->slot.t2.b)) launch32_colsum(dp2, kC, nullptr, 0, nullptr, 0, r.B, kC, r.B, 0.f, g, 0, t.cpart, t.cpart_floats, s);
    if (float* g = t.grad(c->slot.t0.w)) step_dw_now(t, dw_op(dp1, kC, emb, 256, r.B, kC, 256, g, nullptr, t.part, t), s);
    if (float* g = t.grad(c->slot.t0.b)) launch32_colsum(dp1, kC, nullptr, 0, nullptr, 0, r.B, kC, r.B, 0.f, g, 0, t.cpart, t.cpart_floats, s);
    LAUNCHCHK();
    return t.mark();
}

// backward: final layer, trunk layers, token embedding, IPA streams, time embedder; a milestone (Train::mark) after each group
static int train_backward(Train& t) {
    const Run& r = t.r;
    const mdgen_ctx* c = t.c;
    HIPCHK(hipMemsetAsync(t.dmod, 0, (size_t)r.B * c->modrow * 4, r.s));
    if (int e = final_bwd(t)) return e;
    for (int i = c->nl - 1; i >= 0; --i) {
        const TrunkW& w = c->trunk[i];
        const TrunkSites site = trunk_sites(r, i, 0, t.dmod);
        if (int e = mlp_bwd(t, w.ffn, site.mlp, t.dh, t.tm[i])) return e;
        if (int e = attn_bwd(t, w.mha_t, site.t, t.dh, t.tt[i])) return e;
        if (int e = attn_bwd(t, w.mha_l, site.l, t.dh, t.tl[i])) return e;
        if (int e = ada_head_bwd(t, w.ada, c->trunk_off(i), 9 * kC)) return e;
        LAUNCHCHK();
        if (int e = t.mark()) return e;
    }
    if (int e = embed_bwd(t)) return e;
    // IPA stack(s), tokens (b, l): groups of L tokens.  d ipa_out reaches both streams of the two-sided model unchanged.
    for (int k = 1; k < t.nst; ++k)
        HIPCHK(hipMemcpyAsync(t.st[k].dh, t.st[0].dh, (size_t)r.Mp * kC * 4, hipMemcpyDeviceToDevice, r.s));
    for (int k = 0; k < t.nst; ++k)
        if (int e = ipa_backward(t, t.st[k], k == t.nst - 1)) return e;
    return time_embedder_bwd(t);
}

}  // namespace

extern "C" int32_t mdgen_train_workspace_bytes(const mdgen_ctx* c, const mdgen_shape* sh, size_t* bytes) {
    if (!c || !sh || !bytes) return fail(-1, "null argument");
    if (int e = check_shape(c, sh, 1)) return e;
    *bytes = carve_train(nullptr, c, sh->B, sh->T, sh->L, nullptr);
    return 0;
}

extern "C" int32_t mdgen_train_forward_backward(mdgen_ctx* c, const mdgen_shape* sh, const float* xt, const float* tvals,
                                                const mdgen_cond* cond, const float* target, const float* loss_mask, float* loss, float* pred,
                                                float* grads, const int64_t* grad_offsets, void* ws, size_t ws_bytes,
                                                void* tape, size_t tape_bytes, void* stream) {
    if (!xt || !tvals || !target || !loss_mask || !loss || !pred || !grads || !grad_offsets || !tape)
        return fail(-1, "null tensor argument");
    if (int e = check_cond(cond)) return e;
    if (!c) return fail(-1, "null context");
    const bool two = c->d.tps_condition != 0;
    mdgen_cond cd = *cond;
    if (!two) cd.end_rot = cd.end_trans = cd.rel7 = nullptr;   // a one-sided model reads neither
    if (two && (!cd.end_rot || !cd.end_trans)) return fail(-2, "tps_condition requires end frames");
    if (!c->opt_keep_fp32 || !c->any_f32()) return fail(-6, "the training step runs on the fp32 weight copies: option keep_fp32_weights");
    Train t;
    t.c = c;
    t.xt = xt; t.tvals = tvals; t.target = target; t.loss_mask = loss_mask; t.loss = loss; t.pred = pred;
    t.grads = grads;
    t.goff = grad_offsets;
    // option train_precision = 16: the linear layers and weight gradients of this call multiply bf16-rounded operands on
    // the bf16 MFMA (fp32 accumulate, fp32 master weights, everything else fp32)
    t.bf16 = c->opt_train_precision == 16;
    if (int e = make_run(&t.r, c, sh, 1, 0, true, ws, ws_bytes, stream)) return e;   // (true: with check_f32_weights)
    Run& r = t.r;
    bind_cond(r, cd);
    if (((uintptr_t)tape & 255) != 0) return fail(-7, "tape must be 256-byte aligned");
    const size_t need = carve_train(&t, c, r.B, r.T, r.L, (unsigned char*)tape);
    if (tape_bytes < need) return fail(-7, "tape too small: %zu < %zu bytes", tape_bytes, need);
    bind_ipa_streams(t);
    if (int e = open_side_stream(t)) return e;
    if (int e = prefetch_turned(t, (hipStream_t)stream)) return e;
    Join join{t};
    if (int e = train_forward(t)) return e;
    if (int e = train_backward(t)) return e;
    finish_turned(t);
    return join.run();   // (the destructor covers the error returns above)
}

// The training kernels read the fp32 weights through WeightSlot::f32 (natural layout).  Binding makes
// those pointers POINT INTO the caller's flat parameter buffer instead of at private copies, so an optimiser step that
// updates the flat buffer in place is seen by the next mdgen_train_forward_backward without any hand-back
// (round 2 re-uploaded and re-packed all 124 tensors through mdgen_ctx_set_weight after every step).
// The bf16 fragment-packed weights of the SAMPLER are not touched: refresh them with mdgen_ctx_set_weight before sampling.
extern "C" int32_t mdgen_train_bind_params(mdgen_ctx* c, float* flat, const int64_t* offsets) {
    if (!c || !flat || !offsets) return fail(-1, "null argument");
    if (!c->opt_keep_fp32) return fail(-6, "binding needs option keep_fp32_weights = 1 (fp32 training path)");
    c->tr_plan_ok = false;   // the recorded weight-image requests point at the old locations: never read through them again
    c->tr_plan.clear();
    for (size_t i = 0; i < c->weights.size(); ++i) {
        WeightSlot& w = c->weights[i];
        if (offsets[i] < 0) continue;
        if (!w.f32) return fail(-5, "weight '%s' has not been loaded yet", w.name.c_str());
        w.f32 = flat + offsets[i];   // (the private copy stays owned by the context and is freed with it)
        w.bound = true;
    }
    return 0;
}

extern "C" int32_t mdgen_train_num_milestones(const mdgen_ctx* c) { return c ? 2 * c->nl + 3 : 0; }

extern "C" int32_t mdgen_train_set_milestone_events(mdgen_ctx* c, void* const* events, int32_t n) {
    if (!c) return fail(-1, "null context");
    if (n < 0 || (n > 0 && !events)) return fail(-2, "bad event list");
    c->milestone_events.assign(events, events + n);
    return 0;
}

// ---- test hooks: one linear layer / one weight gradient / one attention through the training step's form functions ---------
extern "C" int32_t mdgen_debug_train_linear(int32_t precision, const float* a, int32_t lda, const float* w, int32_t ldw,
                                            const float* bias, int64_t n, int32_t m, int32_t k, float* c, int32_t ldc, void* scratch,
                                            void* stream) {
    NONNULL(a, w, c);
    if ((precision != 16 && precision != 32) || n < 1 || m < 1 || k < 1) return fail(-2, "precision 16 | 32; n, m, k >= 1");
    hipStream_t s = (hipStream_t)stream;
    LinearParams p = lin_op(a, lda, w, ldw, bias, n, m, k, c, ldc);
    const LinearForm form = linear_form(precision == 16, LinShape{n, m, k, lda, ldw, 0, al16(a), al16(w), false}, scratch != nullptr);
    if (linear_streams(form)) {
        launch16_pack_wstream(&w, 1, m, ldw, m, k, 0, scratch, s);
        p.wpack = (const unsigned char*)scratch;
    }
    step_linear(p, form, s);
    LAUNCHCHK();
    return 0;
}
extern "C" int32_t mdgen_debug_train_dw(int32_t precision, const float* dy, int32_t ldy, const float* x, int32_t ldx, int64_t n,
                                        int32_t m, int32_t k, float* dw, float* db, float* part, int64_t part_floats, void* stream) {
    NONNULL(dy, x, dw, part);
    if ((precision != 16 && precision != 32) || n < 1 || m < 1 || k < 1) return fail(-2, "precision 16 | 32; n, m, k >= 1");
    if (part_floats < (int64_t)2 * m * (k + 1)) return fail(-2, "part_floats must be >= 2 m (k + 1)");
    hipStream_t s = (hipStream_t)stream;
    const DwParams p{dy, ldy, x, ldx, n, m, 1, k, {dw, nullptr, nullptr}, {db, nullptr, nullptr}, part, (size_t)part_floats};
    const DwForm form = dw_form(precision == 16, dw_shape(p), p.part_floats, false, false);
    launch_dw(p, form, s);
    if (db && !dw_bias_rides(form, dw_shape(p), p.part_floats))
        launch32_colsum(dy, ldy, nullptr, 0, nullptr, 0, n, m, n, 0.f, db, 0, part, (size_t)part_floats, s);
    LAUNCHCHK();
    return 0;
}

extern "C" int32_t mdgen_debug_train_attention(int32_t precision, const float* qkv, int64_t ntok, int32_t nseq, int32_t len,
                                               int32_t inner, int32_t outer_stride, int32_t inner_stride, int32_t pos_stride,
                                               const float* mask, const float* bias_k, const float* bias_v, const float* inv_freq,
                                               const float* dout, float* out, float* lse, float* dqkv, float* dbias, float* stats,
                                               void* stream) {
    NONNULL(qkv, mask, bias_k, bias_v, inv_freq, dout, out, lse, dqkv, dbias, stats);
    if ((precision != 16 && precision != 160 && precision != 161 && precision != 32) || ntok < 1 || nseq < 1 || len < 1 || inner < 1)
        return fail(-2, "precision 16 | 160 | 161 | 32; ntok, nseq, len, inner >= 1");
    hipStream_t s = (hipStream_t)stream;
    const AxisMap ax{nseq, len, inner, outer_stride, inner_stride, pos_stride};
    // 32 / 16: the training step's attention form for the axis, q and k given rotated (so Seq where the step takes SeqRope);
    // 160: the chunked kernels for every length; 161: q, k given UNROTATED, the sequence-resident kernels rotate them (as the
    // training step runs them)
    TrainAttnForm form = train_attn_form(precision != 32, ax);
    if (precision == 161 && form != TrainAttnForm::SeqRope)
        return fail(-2, "precision 161: only axes of 129 .. 256 positions rotate q, k inside the kernels");
    if (precision == 16 && form == TrainAttnForm::SeqRope) form = TrainAttnForm::Seq;
    if (precision == 160) form = TrainAttnForm::Chunked;
    TrainAttnParams a{qkv, 3 * kC, ax, MaskMap{mask, 0}, bias_k, bias_v, inv_freq, out, lse, dout, dqkv, stats, dbias, false};
    launch_train_attn(a, form, s);
    launch_train_attn_bwd(a, form, s);
    if (form == TrainAttnForm::Exact)   // position of a token on this axis, as k32_rope_bwd wants it: (token / pos_stride) % len
        launch32_rope_bwd(dqkv, ntok, 3 * kC, pos_stride, len, inv_freq, 1.0f / std::sqrt((float)kDH), s);
    LAUNCHCHK();
    return 0;
}

// The IPA point attention alone: launch_ipa_attn as ipa_block_fp32 fills it (features in fp32, lse, the split scratch) and
// launch32_ipa_bwd as ipa_block_bwd does; feat_bf16: a second forward launch as the bf16 sampler path makes it (no scratch)
extern "C" int32_t mdgen_debug_ipa_slices(int32_t ngroups, int32_t len, int32_t has_part, int64_t part_floats, int32_t* fwd_slices,
                                          int32_t* bwd_slices, int32_t* fwd_tiled) {
    if (!fwd_slices || !bwd_slices || !fwd_tiled) return fail(-1, "null argument");
    if (ngroups < 1 || len < 1 || part_floats < 0) return fail(-2, "ngroups, len >= 1; part_floats >= 0");
    *fwd_slices = ipa_fwd_nsplit(ngroups, len, has_part != 0, (size_t)part_floats);
    *bwd_slices = ipa_bwd_nsplit(ngroups, len, has_part != 0, (size_t)part_floats);
    *fwd_tiled = ipa_attn_tiled(len) ? 1 : 0;
    return 0;
}
extern "C" int32_t mdgen_debug_ipa_attention(const float* proj, const float* rot, const float* trans, const float* mask,
                                             const float* head_w, int32_t ngroups, int32_t nbatch, int32_t len, float* part,
                                             int64_t part_floats, const float* dfeat, float* feat, void* feat_bf16, float* lse,
                                             float* dproj, float* dhead_w, float* bwd_scratch, int32_t* fwd_slices,
                                             int32_t* bwd_slices, void* stream) {
    NONNULL(proj, rot, trans, mask, head_w, feat, lse);
    if (!fwd_slices || !bwd_slices) return fail(-1, "null argument");
    if (ngroups < 1 || nbatch < 1 || len < 1 || ngroups % nbatch != 0 || part_floats < 0)
        return fail(-2, "ngroups, nbatch, len >= 1; ngroups a multiple of nbatch; part_floats >= 0");
    if (dfeat && ngroups != nbatch) return fail(-2, "the backward runs with ngroups == nbatch only (the training step)");
    if (dfeat) NONNULL(dproj, dhead_w, bwd_scratch);
    hipStream_t s = (hipStream_t)stream;
    const long M = (long)ngroups * len;
    const size_t pf = part ? (size_t)part_floats : 0;
    IpaAttnParams ap{};
    ap.proj = proj; ap.rot = rot; ap.trans = trans;
    ap.mask_bl = mask;
    ap.head_w = head_w; ap.feat = nullptr; ap.feat32 = feat; ap.stats = lse;
    ap.ngroups = ngroups; ap.B = nbatch; ap.L = len;
    ap.part = part; ap.part_floats = pf;
    *fwd_slices = ipa_fwd_nsplit(ngroups, len, part != nullptr, pf);
    *bwd_slices = dfeat ? ipa_bwd_nsplit(ngroups, len, part != nullptr, pf) : 0;
    launch_ipa_attn(ap, s);
    if (feat_bf16) {
        IpaAttnParams bp{};
        bp.proj = proj; bp.rot = rot; bp.trans = trans;
        bp.mask_bl = mask;
        bp.head_w = head_w;
        bp.feat = (__bf16*)feat_bf16;
        bp.ngroups = ngroups; bp.B = nbatch; bp.L = len;
        launch_ipa_attn(bp, s);
    }
    if (dfeat) {
        IpaAttnParams bp{};   // as ipa_block_bwd fills it: the forward's tape, no forward scratch
        bp.proj = proj; bp.rot = rot; bp.trans = trans;
        bp.mask_bl = mask;
        bp.head_w = head_w; bp.feat = nullptr; bp.feat32 = feat; bp.stats = lse;
        bp.ngroups = ngroups; bp.B = nbatch; bp.L = len;
        launch32_ipa_bwd(bp, dfeat, dproj, bwd_scratch, bwd_scratch + M * 4, dhead_w, s, part, pf);
    }
    LAUNCHCHK();
    return 0;
}

// ---- the plans of a step, host only ---------------------------------------------------------------------------------------
namespace {
const char* form_name(LinearForm f) {
    static const char* const n[] = {"k32_linear", "k16_linear_wdma<false>", "k16_linear_wdma<true>", "k16_linear_wide",
                                    "k16_linear_small", "k16_linear_fast", "k16_linear"};
    return n[(int)f];
}
const char* form_name(DwForm f) {
    static const char* const n[] = {"k32_dw", "k16_dw_wide<false, false>", "k16_dw_wide<true, false>", "k16_dw_wide<false, true>",
                                    "k16_dw_wide<true, true>", "k16_dw<true>", "k16_dw<false>"};
    return n[(int)f];
}
const char* form_name(TrainAttnForm f) {
    static const char* const n[] = {"k32_attn", "k16_attn", "k16_attn_seq", "k16_attn_seq+rope"};
    return n[(int)f];
}
const char* form_name(GateBwdForm f) { return f == GateBwdForm::Sums ? "k32_gate_bwd_sums" : "k32_gate_mul"; }
const char* form_name(LnBwdForm f) { return f == LnBwdForm::Sums ? "k32_ln_bwd_sums" : "k32_ln_bwd"; }
struct PlanJson {
    char* buf;
    size_t cap, len = 0;
    void add(const char* fmt, ...) __attribute__((format(printf, 2, 3))) {
        va_list ap;
        va_start(ap, fmt);
        const int n = len < cap ? vsnprintf(buf + len, cap - len, fmt, ap) : 0;
        va_end(ap);
        len = n < 0 || len + (size_t)n >= cap ? cap : len + (size_t)n;   // (cap: did not fit)
    }
    void dx(const char* key, const DxPlan& p) {
        add(", \"%s\": [\"%s\", \"%s\"]", key, p.route == DxRoute::Streamed ? "streamed" : p.route == DxRoute::TurnedWeight ? "turned" : "wtrans",
            form_name(p.form));
    }
    void dw(const char* key, const DwPlan& p) { add(", \"%s\": [\"%s\", %s]", key, form_name(p.form), p.bias_rides ? "true" : "false"); }
    void attn(const char* key, const AttnPlan& p) {
        add("\"%s\": {\"rows\": \"%s\", \"dqkv\": \"%s\", \"qkv\": [", key, p.rows16 ? "bf16" : "fp32", p.dqkv16 ? "bf16" : "fp32");
        if (p.qkv_one_pass) add("\"%s\"", form_name(p.qkv[0]));
        else add("\"%s\", \"%s\", \"%s\"", form_name(p.qkv[0]), form_name(p.qkv[1]), form_name(p.qkv[2]));
        add("], \"attn\": \"%s\", \"out\": \"%s\", \"gate\": \"%s\", \"ln\": \"%s\"", form_name(p.attn), form_name(p.out), form_name(p.gate),
            form_name(p.ln));
        dx("dx_out", p.dx_out); dw("dw_out", p.dw_out); dx("dx_qkv", p.dx_qkv); dw("dw_qkv", p.dw_qkv);
        add("}");
    }
    void mlp(const char* key, const MlpPlan& p) {
        add("\"%s\": {\"rows\": \"%s\", \"fc1\": \"%s\", \"fc2\": \"%s\", \"gate\": \"%s\", \"ln\": \"%s\"", key, p.rows16 ? "bf16" : "fp32",
            form_name(p.fc1), form_name(p.fc2), form_name(p.gate), form_name(p.ln));
        dx("dx_fc2", p.dx_fc2); dw("dw_fc2", p.dw_fc2); dx("dx_fc1", p.dx_fc1); dw("dw_fc1", p.dw_fc1);
        add("}");
    }
};
}  // namespace

extern "C" int32_t mdgen_debug_train_plan(const mdgen_shape* sh, int32_t tps_condition, int32_t num_layers, int32_t train_precision,
                                          int32_t weight_misalign_bytes, char* buf, size_t buflen) {
    if (!sh || !buf) return fail(-1, "null argument");
    if (num_layers < 1 || num_layers > 8 || (train_precision != 16 && train_precision != 32) || sh->B < 1 || sh->T < 1 || sh->L < 1)
        return fail(-2, "num_layers in 1..8, train_precision 16 | 32, B, T, L >= 1");
    Train t;   // (the plan functions read the operand mode and the scratch sizes only)
    t.bf16 = train_precision == 16;
    t.part_floats = kPartFloats;
    t.cpart_floats = kCpartFloats;
    const bool al = (weight_misalign_bytes & 15) == 0;   // every weight of the step alike
    const bool w_al[5] = {al, al, al, al, al};
    const bool w4[4] = {al, al, al, al}, w2[2] = {al, al};
    const long B = sh->B, T = sh->T, L = sh->L, N = B * T * L, Mp = B * L, TL = T * L;
    PlanJson js{buf, buflen};
    const IpaPlan ip = plan_ipa(t, Mp, w_al);
    js.add("{\"rows\": {\"ipa\": %ld, \"trunk\": %ld}, \"ipa_block\": {\"proj\": [\"%s\", \"%s\", \"%s\", \"%s\"], \"out\": \"%s\"", Mp, N,
           form_name(ip.proj[0]), form_name(ip.proj[1]), form_name(ip.proj[2]), form_name(ip.proj[3]), form_name(ip.out));
    const char* const dxn[4] = {"dx_q", "dx_kv", "dx_q_points", "dx_kv_points"};
    const char* const dwn[4] = {"dw_q", "dw_kv", "dw_q_points", "dw_kv_points"};
    for (int j = 0; j < 4; ++j) {
        js.dx(dxn[j], ip.dx_proj[j]);
        js.dw(dwn[j], ip.dw_proj[j]);
    }
    js.dx("dx_out", ip.dx_out);
    js.dw("dw_out", ip.dw_out);
    js.add("}, ");
    js.attn("ipa_attn", plan_attn(t, Mp, axis_ipa(B, L), L, w4));
    js.add(", ");
    js.mlp("ipa_mlp", plan_mlp(t, Mp, L, w2));
    js.add(", ");
    js.attn("trunk_attn_l", plan_attn(t, N, axis_res(B, T, L), TL, w4));
    js.add(", ");
    js.attn("trunk_attn_t", plan_attn(t, N, axis_time(B, T, L), TL, w4));
    js.add(", ");
    js.mlp("trunk_mlp", plan_mlp(t, N, TL, w2));
    // (latent_dim: 21, 28 for the two-sided model -- mdgen_ctx_create's D; every sub-layer's scale chunk lies behind its shift chunk)
    const FinalPlan fin = plan_final(t, N, tps_condition ? 28 : 21, TL, al);
    js.add(", \"final\": {\"lin\": \"%s\", \"ln\": \"%s\"", form_name(fin.lin), form_name(fin.ln));
    js.dx("dx", fin.dx);
    js.dw("dw", fin.dw);
    js.add("}}");
    if (js.len >= js.cap) return fail(-7, "plan buffer too small (%zu bytes)", buflen);
    return 0;
}
