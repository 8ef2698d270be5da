// kernels.h -- parameter blocks and launchers shared between the kernels (*.hip) and api.cpp
#pragma once
#include "common.h"

namespace mdg {

struct QkvParams {
    const float* h;        // residual stream [N][384] fp32
    long nrows;            // N (SMALL layout: natural-order panels)
    AxisMap ax;            // attention axis
    ModMap mm;
    int shift_chunk, scale_chunk;
    const bf16x8 *wq, *wk, *wv;   // packed fragments [12 ftile][24 kstep][64 lane][8]
    const float *bq, *bk, *bv;    // permuted biases [384]
    const float* rope;     // [P][kRopeRow]: per half h: cos(6) | pad | sin(6) | pad
    unsigned char *qf, *kf, *vf;  // FLASH layout fragment buffers
    __bf16* qkv_small;     // SMALL layout [token][3][16 head][2 half][12]
    int panels_per_seq;
    uint32_t* vmask;       // FLASH layout: key-validity words [seq][vmask_stride], one per 32-key tile (see flash_vmask)
    int vmask_stride;
    // k_ln_qkv_attn4 only (residue axis, L == 4: attention inside the QKV kernel)
    const float *bias_k, *bias_v;   // learned bias key / value [384]
    const uint32_t* l4tab;          // ... as the L == 4 kernel consumes them (launch_l4_bias_table), [2][kL4Tab] bf16 pairs
    MaskMap mk;                     // key-padding mask
    __bf16* obuf;                   // attention output [token][384] bf16 (PROJ == false)
    // k_ln_qkv_attn4<true>: the out-projection + gated residual of the same sub-layer, in the same kernel
    float* h_rw;                    // == h (the rows a workgroup normalised are the rows it updates)
    const bf16x8* wo;               // packed out-projection weights
    const float* bo;
    int gate_chunk;
};

struct ProjParams {
    float* h;
    long nrows;
    ModMap mm;
    int gate_chunk;
    int gated;
    const bf16x8* w;       // packed [12 ftile][K/16][64][8]
    const float* bias;
    const __bf16* a_bf16;  // MODE 0/1 A rows
    // MODE 2 (micro attention)
    const __bf16* qkv_small;
    AxisMap ax;
    MaskMap mk;
    const float *bias_k, *bias_v;
    const float* rope;
};

struct MlpParams {
    float* h;
    long nrows;
    ModMap mm;
    int shift_chunk, scale_chunk, gate_chunk;
    const bf16x8 *w1, *w2;  // w1 [48 ftile][24][64][8]; w2 [12 ftile][96][64][8]
    const float *b1, *b2;
    unsigned long long* trace;   // measurement only (mdgen_profile_phase_trace): [wave][32] s_memtime stamps, or null
    long trace_cap;              // capacity of `trace` in 64-bit words
    // k_mlp<PF1, true>: the preceding (temporal) attention sub-layer's out-projection + gated residual runs in the same panels
    // first (k_proj<0>'s work: attention output rows `o`, packed W_o, bias, gate chunk), o == null: off
    const __bf16* o;
    const bf16x8* wo;
    const float* bo;
    int gate_chunk_o;
    // k_mlp8<PRE, kMlpSplit> (part != null): the hidden chunks of a panel over kMlpSplit workgroups.  part: fp32 partials of the fc2
    // product [panel][kMlpSplit][64][384]; hupd: each workgroup's private copy of the panel's residual rows after the fused
    // out-projection (same shape; PRE only); counters: one per panel, zero before the first launch (the last arriver resets it)
    float* part;
    float* hupd;
    unsigned* counters;
};
constexpr int kMlpSplit = 3;            // workgroups per panel in the split form
constexpr int kMlpSplitMaxPanels = 96;  // panels the context's split scratch covers (the form is for launches of <= ncu / 3 panels)

// k_mlp_rows (k_rows.hip): the MLP block in row-owner form; `wstream` = both weight matrices as one fragment stream in
// consumption order (api.hip mlp_stream_table)
struct MlpRowsParams {
    float* h;
    long nrows;
    ModMap mm;
    int shift_chunk, scale_chunk, gate_chunk;
    const unsigned char* wstream;   // 2304 fragments of 1 KiB
    const float *b1, *b2;
    unsigned long long* trace;      // measurement only: [wave][8] s_memtime stamps, or null
    long trace_cap;
    // gate fold (non-null; every row of the launch shares the modulation row): `wstream` is the (step, layer) stream with
    // the gate folded into fc2 and b2g = gate * b2 (launch_pack_fold): accumulators start from the residual rows, store-only epilogue
    const float* b2g;
    // tail (with b2g, the trunk's LAST layer): FinalLayer + Euler update (layers.py:57-74, integrators.py:106) run on the updated rows while
    // they are still in registers, and the rows are NOT stored (nothing reads the residual stream after the last layer): k_final's
    // launch, its 98 MB read and this kernel's 98 MB write are gone.  tail_w: emb_to_latent.linear.weight as 24 fragments in kappa
    // order (rows >= D zero), tail_b [32], tail_mod: the step's final adaLN row (shift chunk 0, scale chunk 1).
    const bf16x8* tail_w;
    const float* tail_b;
    const float* tail_mod;
    int tail_D, tail_euler;
    float tail_dt;
    float* tail_x;      // euler: state updated in place
    float* tail_out;    // !euler: velocity
    // ... and (emb_base != null; euler) the NEXT step's token embedding from the updated state (k_embed's work) written to h: see rows.h
    // rows_embed_tail.  emb_base: the next step's base rows of this view (launch_embed_base)
    const float *emb_base, *emb_mdelta, *emb_xcond;
    const bf16x8 *emb_wl_hi, *emb_wl_lo, *emb_wc_hi, *emb_wc_lo;   // the weights as bf16 pairs (launch_pack_rows kappa = 1, part 0 / 1)
    const int64_t* emb_cmask;
    int emb_T, emb_L;
};
void launch_sub_f32(const float* a, const float* b, float* dst, int n, hipStream_t s);   // dst = a - b
// base[s][bl][c] = bl[c] + bc[c] + mask_emb[0][c] + (pos_embed ? pos_embed[l][c] : 0) + ipa_out[s][bl][c]   (S * BL rows)
void launch_embed_base(const float* bl, const float* bc, const float* mask_emb, const float* pos_embed, const float* ipa_out, int S,
                       int BL, int L, float* base, hipStream_t s);

struct LnLinearParams {
    const float* h;
    long nrows;
    ModMap mm;              // mm.mod = [gamma | beta]
    const bf16x8* w;        // packed [nout/32][24][64][8]
    const float* bias;
    float* out;             // [nrows][nout] fp32
    int nout;               // multiple of 96
};

struct FinalParams {
    const float* h;
    long nrows;
    ModMap mm;
    int shift_chunk, scale_chunk;
    const bf16x8* w;        // packed [1 ftile][24][64][8] (rows >= D are zero)
    const float* bias;      // [32]
    int D;
    int euler;
    float dt;
    float* x;               // euler: state updated in place
    float* out;             // !euler: velocity
};

// Key-validity words of the tiled attention: one uint32 per (sequence, 32-key tile); bit set = the key is real (inside
// the sequence and not padded, or the learned bias key at position len).  Per sequence `stride` words, a multiple of
// 64 >= ntile + 1, zero beyond the last tile (k_flash reads them in 64-tile windows, one tile ahead).  They live in the
// slack of the V^T fragment region (a tile is allocated kFragBytes, V^T uses kFragV of it), behind the last fragment.
static_assert((kFragBytes - kFragV) * kH >= 4 * 64 + 4 * 1 + 256,
              "the key-validity words (<= ntile + 64 of them per sequence, 256-byte aligned) must fit the slack the V^T fragments leave");
__host__ __device__ inline int flash_vmask_stride(int ntile) { return (ntile + 64) & ~63; }
__host__ __device__ inline size_t flash_vmask_offset(long nseq, int ntile) {
    return (((size_t)nseq * kH * ntile * kFragV) + 255) & ~(size_t)255;
}

struct FlashParams {
    AxisMap ax;
    MaskMap mk;
    const unsigned char *qf, *kf, *vf;
    const float *bias_k, *bias_v;  // natural fp32 [384]
    const float* rope;
    __bf16* obuf;           // [N][384]
    const uint32_t* vmask;  // [seq][vmask_stride]: bit k of word t = key 32 t + k may be attended (written by k_ln_qkv)
    int vmask_stride;
    int force_robust;       // option attention_path: 1 = skip the fixed-anchor loop, always run the moving-shift loop
    int rotate;             // option flash_rotate: 1 = every 64-query chunk starts its walk over the key tiles at a different tile
};

// k_flash_proj: k_flash for all 16 heads of 64 queries + the sub-layer's out-projection + gated residual (k_proj<0>'s work)
struct FlashProjParams {
    FlashParams f;          // (f.obuf is not used: the attention output stays in LDS)
    float* h;               // residual stream, updated in place
    ModMap mm;
    int gate_chunk;
    const bf16x8* wo;       // packed out-projection weights [12 ftile][24 kstep][64 lane][8]
    const float* bo;
};

struct EmbedParams {
    const float *x, *x_cond;
    const int64_t* x_cond_mask;
    const float *wl, *bl, *wc, *bc;  // latent_to_emb / cond_to_emb fp32 [C][D], [C]
    const float *wl_pack, *wc_pack;  // the two weights in the kernel's B-operand order (launch_pack_embed): coalesced prologue loads
    const float* mask_emb;           // [2][C]
    const float* pos_embed;          // [crop][C] or nullptr
    const float* ipa_out;            // [B*L][C] for this step
    float* h;
    long N;
    int T, L, D;
};

struct IpaAttnParams {
    const float* proj;      // [M][672]
    const float *rot, *trans;  // [B][L][3][3], [B][L][3]
    const float* mask_bl;   // [B][L]
    const float* head_w;    // [4]
    __bf16* feat;           // [M][256]
    float* feat32;          // fp32 mode: features written here (fp32) instead of `feat`
    float* stats;           // training tape (nullable): [M][4 heads] log-sum-exp of the logits (m + log(sum exp))
    int ngroups, B, L;
    // k_ipa_attn_tiled with few groups (training at B = 1: four workgroups, one wave per SIMD, 185 us): the key loop cut
    // into `nsplit` slices (blockIdx.y) that leave (running max, denominator, o, o_pt) per (slice, token, head) in `part`
    // ([nsplit][M][4][58] floats) for k_ipa_attn_merge.  Set by launch_ipa_attn when `part` is given; 0 / null: one slice.
    int nsplit;
    float* part;
    size_t part_floats;
};
constexpr int kIpaFwdRec = 58;   // m | den | o(32) | o_pt(24)

struct FloatChunk {
    float v[128];
    int n;
};

// Kernel forms: one value = one kernel instantiation.  The orchestration (api.hip) decides the form of a launch and fills the
// operands the form reads; the launcher switches on it.  A form whose operands are missing launches nothing and leaves a message
// for k32_take_launch_error (error -7 from the entry point).
enum class QkvForm {
    Small,             // k_ln_qkv<true>: SMALL layout (L <= 8)
    Panel4,            // k_ln_qkv<false>: fragment layout, four waves per 64-row panel
    Panel8,            // k_ln_qkv8<false>: eight waves
    Panel8Split,       // k_ln_qkv8<true>: q, k | v over a workgroup pair
    Panel8SplitHalf,   // k_ln_qkv8<true, true>: ... of 32 positions (panels_per_seq counts 32-position panels)
    PreProj            // k_ln_qkv<false, true>: the previous sub-layer's out-projection + gated residual first (obuf, wo, bo, h_rw)
};
enum class Attn4Form {
    AttnOnly,    // k_ln_qkv_attn4<false>: writes the attention output (obuf)
    Fused,       // k_ln_qkv_attn4<true>: ... and runs the out-projection + gated residual (wo, bo, h_rw)
    FusedHalf    // k_ln_qkv_attn4<true, true>: 32-row workgroups
};
enum class ProjMode { Plain, Linear, MicroAttn };   // k_proj<0 | 1 | 2>: attention output rows, IPA linear_out (K = 256), micro attention (L <= 8)
enum class MlpPanelForm {   // Pre*: the temporal out-projection in the prologue (o, wo, bo); *Split: part, hupd, counters
    W4, W8, W8Split,             // k_mlp<3>, k_mlp8<false>, k_mlp8<false, kMlpSplit>
    PreW4, PreW8, PreW8Split     // k_mlp<3, true>, k_mlp8<true>, k_mlp8<true, kMlpSplit>
};
enum class MlpRowsForm {
    Plain,            // k_mlp_rows<4, uni>, uni: no 32-row tile straddles two modulation groups (follows from the ModMap)
    Fold,             // k_mlp_rows<4, true, true>: gate folded into the stream (b2g); one modulation group
    FoldFinal,        // k_mlp_rows<4, true, true, true>: ... + FinalLayer tail (tail_*) ...
    FoldFinalEmbed    // ... + the next step's token embedding (emb_*): the same instantiation, which tests emb_base
};
enum class FlashProjForm { Q64, Q128 };   // k_flash_proj (four waves, 64-row panel), k_flash_proj8 (eight waves, 128-row panel)

void launch_ln_qkv(const QkvParams& p, QkvForm form, hipStream_t s);
void launch_xcc_probe(int* out, int nblocks, hipStream_t s);
void launch_ln_qkv_attn4(const QkvParams& p, Attn4Form form, hipStream_t s);
void launch_proj(const ProjParams& p, ProjMode mode, hipStream_t s);
void launch_mlp(const MlpParams& p, MlpPanelForm form, hipStream_t s);
void launch_mlp_rows(const MlpRowsParams& p, MlpRowsForm form, hipStream_t s);
constexpr int kMlpStreamFrags = 2304;   // 1 KiB fragments of one MLP weight stream (api.hip mlp_stream_table)
// per-(step, layer) MLP streams with the step's gate folded into fc2 (+ b2g = gate * b2); S * nl streams, nl <= 8
void launch_pack_fold(const float* mod, long mod_step_stride, int S, int nl, const int* goff, const float* const* w2,
                      const float* const* b2, const bf16x8* const* base, const int* tab, bf16x8* dst, float* b2g, hipStream_t s);
// rowmap (nullable): source row of packed row r (a permutation of the matrix's rows); kappa: K order inside a k-step -- 0
// natural, 1 rows.h kappa (operand = LayerNorm / GELU registers)
void launch_pack_stream(const float* w, int ld, int which, const int* tab, int nfrag, float scale, int kappa, bf16x8* dst,
                        hipStream_t s, const int* rowmap = nullptr);
void launch_ln_linear(const LnLinearParams& p, hipStream_t s);
void launch_final(const FinalParams& p, hipStream_t s);
void launch_flash(const FlashParams& p, hipStream_t s);
long flash_proj_jobs(const AxisMap& ax);
void launch_flash_proj(const FlashProjParams& p, FlashProjForm form, hipStream_t s);
void launch_pack_embed(const float* w, int D, float* pack, hipStream_t s);   // pack: kEmbPackFloats floats
constexpr int kEmbPackFloats = 4 * 3 * 14 * 64;
void launch_embed(const EmbedParams& p, hipStream_t s);
void launch_path_plan(const float* t, const float* x0, const float* x1, float* xt, float* ut, long per_sample, long B,
                      int gvp, hipStream_t s);
void launch_masked_mse(const float* pred, const float* target, const float* mask, float* loss, long per_sample, long B,
                       hipStream_t s, float* scratch = nullptr, size_t scratch_floats = 0, float* den_out = nullptr);
void launch_ipa_attn(const IpaAttnParams& p, hipStream_t s);

// fp32-operand path (k_fp32.hip) and the training step (k_fp32_bwd.hip, k_wide16.hip, k_attn16.hip)
extern thread_local const char* g_k32_launch_error;   // set by a launcher that refused a shape (nothing launched)
const char* k32_take_launch_error();                  // ... and cleared by the entry point that reports it

// Kernel forms of the training step, as above: one value = one instantiation or one fixed launch sequence.  The form
// functions below are pure host functions of the operand mode (bf16: option train_precision = 16), the shape, the strides and the
// 16-byte alignment of the operands; the step evaluates them once per sub-layer, before its first launch (train.inc *Plan), and
// the launchers check with the same predicates that the operands fit the form they are handed.
enum class LinearForm {
    F32,              // k32_linear: exact fp32 products
    StreamF32Rows,    // k16_linear_wdma<false>: the weight as a bf16 fragment stream (wpack), fp32 token rows
    StreamBf16Rows,   // k16_linear_wdma<true>: ... token rows stored as bf16 (a_bf16)
    Wide,             // k16_linear_wide: 128 x 384 tiles, fp32 weight rows
    Small,            // k16_linear_small: one wave per 32 x 32 tile (at most 2048 rows)
    Fast,             // k16_linear_fast
    Plain             // k16_linear: any stride, alignment or wtrans
};
enum class DwForm {
    F32,                                        // k32_dw
    Wide, WideXbf, WideDYbf, WideXbfDYbf,       // k16_dw_wide<XBF, DYBF>: X / dY stored as bf16 rows
    Fast, Plain                                 // k16_dw<true>, k16_dw<false>
};
enum class GateBwdForm { Sums, MulColsum };     // k32_gate_bwd_sums + k32_colsum_final | k32_gate_mul, k32_colsum + k32_colsum_final
enum class LnBwdForm { Sums, ColsumsLnBwd };    // k32_ln_bwd_sums + k32_colsum_final | two launch32_colsum, k32_ln_bwd
enum class TrainAttnForm {
    Exact,     // k32_attn | k32_attn_bwd_q, k32_attn_bwd_kv (q, k rotated by k32_rope before, dq, dk taken back by k32_rope_bwd)
    Chunked,   // k16_attn<8 | 4> | k16_attn_bwd_q<4>, k16_attn_bwd_kv<4> (q, k rotated before; dq, dk come back unrotated)
    Seq,       // k16_attn_seq | k16_attn_bwd_seq: axes of 129 .. 256 positions (attn16_seq_form)
    SeqRope    // ... which rotate q, k while they convert them: no k32_rope pass, the tape keeps them unrotated
};
inline bool linear_streams(LinearForm f) { return f == LinearForm::StreamF32Rows || f == LinearForm::StreamBf16Rows; }
inline bool dw_wide(DwForm f) { return f >= DwForm::Wide && f <= DwForm::WideXbfDYbf; }
inline bool dw_x_bf16(DwForm f) { return f == DwForm::WideXbf || f == DwForm::WideXbfDYbf; }
inline bool dw_dy_bf16(DwForm f) { return f == DwForm::WideDYbf || f == DwForm::WideXbfDYbf; }
inline bool attn_seq(TrainAttnForm f) { return f == TrainAttnForm::Seq || f == TrainAttnForm::SeqRope; }

// y[n][m] = a[n][k] w[m][k]^T as the form function sees it.  ldw: row stride of the fp32 weight; *_al: 16-byte aligned (w_al: every
// segment's weight); a_bf16: the token rows are stored as bf16
struct LinShape { long n; int m, k, lda, ldw, wtrans; bool a_al, w_al, a_bf16; };
inline bool linear_vec(const LinShape& q) {   // 16-byte operand loads: every form but F32 and Plain
    return !q.wtrans && q.k % 64 == 0 && (q.lda & (q.a_bf16 ? 7 : 3)) == 0 && (q.ldw & 3) == 0 && q.a_al && q.w_al;
}
// stream: a bf16 fragment stream of the weight is wanted where the launch is big enough for the streamed 128 x 384 kernel
inline LinearForm linear_form(bool bf16, const LinShape& q, bool stream) {
    if (!bf16) return LinearForm::F32;
    if (!linear_vec(q)) return LinearForm::Plain;
    if (stream && q.n >= 1024 && q.m % 384 == 0) return q.a_bf16 ? LinearForm::StreamBf16Rows : LinearForm::StreamF32Rows;
    if (q.n >= 1024 && q.m > 128) return LinearForm::Wide;
    return q.n <= 2048 ? LinearForm::Small : LinearForm::Fast;
}

// dW[m][k] += dy[n][m]^T x[n][k] in n-slices whose partial sums go to part[nsplit][m][k] (+ [nsplit][m] of the bias gradient)
struct DwShape { long n; int m, k, ldy, ldx; bool al; };   // al: dy and x 16-byte aligned
inline bool dw_vec(const DwShape& q) { return ((q.ldy | q.m | q.ldx | q.k) & 7) == 0 && q.al; }
// Slices of the k32_dw / k16_dw grid over n: enough to fill the chip ONCE with 128 x 128 tiles at two workgroups per CU (a
// 384 x 384 weight is only 9 of them); more slices only add partial-sum traffic (113 slices of a 384 x 384 weight: 66 MB
// written and read back)
inline int dw_nsplit(long n, int m, int k, size_t part_floats) {
    const int tiles = ((m + 127) / 128) * ((k + 127) / 128);
    int nsplit = (int)((n + 511) / 512);
    const int want = (512 + tiles - 1) / tiles;
    if (nsplit > want) nsplit = want;
    if (nsplit > 128) nsplit = 128;
    if (nsplit < 1) nsplit = 1;
    while (nsplit > 1 && (size_t)nsplit * m * (k + 1) > part_floats) --nsplit;
    return nsplit;
}
// Invariant point attention (launch_ipa_attn, launch32_ipa_bwd): the per-thread kernel below 24 residues, the LDS-tiled one from
// there; and the slices (blockIdx.y) that the tiled kernels cut their key loop (backward key pass: query loop) into when the
// groups are few: enough for ~64 workgroups, at most one 32-row tile per slice, at most 16, and no more than part_floats holds
// partial sums for.  A slice is ceil(tiles / nsplit) WHOLE tiles, so the last slices can lie past L (5 tiles in 4 slices of 2:
// slice 3 is empty); an empty slice writes the neutral record (forward: m = -3e38, den = 0; backward: zeros).
inline bool ipa_attn_tiled(int L) { return L >= 24; }
constexpr int kIpaPartRow = kIpaProj + 4;   // backward partial row: dproj (672) | dhw (4)
inline int ipa_slices(int ngroups, int L, bool has_part, size_t part_floats, size_t floats_per_slice) {
    const int nqt = (L + 255) / 256;
    const long nblk = (long)ngroups * 4 * nqt;
    int nsplit = has_part ? (int)((64 + nblk - 1) / nblk) : 1;
    const int ntile = (L + kIpaKT - 1) / kIpaKT;
    if (nsplit > ntile) nsplit = ntile;
    if (nsplit > 16) nsplit = 16;
    while (nsplit > 1 && (size_t)nsplit * floats_per_slice > part_floats) --nsplit;
    return nsplit;
}
inline int ipa_fwd_nsplit(int ngroups, int L, bool has_part, size_t part_floats) {   // part[nsplit][M][4][kIpaFwdRec]
    return ipa_attn_tiled(L) ? ipa_slices(ngroups, L, has_part, part_floats, (size_t)ngroups * L * 4 * kIpaFwdRec) : 1;
}
inline int ipa_bwd_nsplit(int ngroups, int L, bool has_part, size_t part_floats) {   // part[nsplit][M][kIpaPartRow]
    return ipa_slices(ngroups, L, has_part, part_floats, (size_t)ngroups * L * kIpaPartRow);
}
inline DwForm dw_form(bool bf16, const DwShape& q, size_t part_floats, bool x_bf16, bool dy_bf16) {
    if (!bf16) return DwForm::F32;
    if (!dw_vec(q)) return DwForm::Plain;
    if (q.n >= 4096 && (size_t)q.m * (q.k + 1) <= part_floats)
        return x_bf16 ? (dy_bf16 ? DwForm::WideXbfDYbf : DwForm::WideXbf) : (dy_bf16 ? DwForm::WideDYbf : DwForm::Wide);
    return DwForm::Fast;
}
// whether the pass also yields the bias gradient (column sums of dY, partials behind the dW partials); else launch32_colsum
inline bool dw_bias_rides(DwForm f, const DwShape& q, size_t part_floats) {
    return dw_wide(f) || (f == DwForm::Fast && (size_t)dw_nsplit(q.n, q.m, q.k, part_floats) * q.m * (q.k + 1) <= part_floats);
}

// slices of the fused element-wise backward + column-sum kernels; false: their partial sums do not fit part_floats
inline bool slice_plan(long nrows, long tokens_per_group, int ncols, size_t part_floats, long* ng, int* rps, int* spg) {
    *ng = (nrows + tokens_per_group - 1) / tokens_per_group;
    *rps = 64;
    while (*rps > 4 && *ng * ((tokens_per_group + *rps - 1) / *rps) < 256) *rps /= 2;   // a few hundred rows: still fill the chip
    *spg = (int)((tokens_per_group + *rps - 1) / *rps);
    while ((size_t)*ng * *spg * ncols > part_floats && *rps < (1 << 24)) {
        *rps *= 2;
        *spg = (int)((tokens_per_group + *rps - 1) / *rps);
    }
    return (size_t)*ng * *spg * ncols <= part_floats;
}
inline bool slices_fit(long nrows, long tokens_per_group, int ncols, size_t part_floats) {
    long ng; int rps, spg;
    return slice_plan(nrows, tokens_per_group, ncols, part_floats, &ng, &rps, &spg);
}
inline GateBwdForm gate_bwd_form(long nrows, long tokens_per_group, size_t part_floats) {
    return slices_fit(nrows, tokens_per_group, kC, part_floats) ? GateBwdForm::Sums : GateBwdForm::MulColsum;
}
// adjacent: the scale chunk lies right behind the shift chunk in the modulation row (one pass writes both gradient chunks)
inline LnBwdForm ln_bwd_form(long nrows, long tokens_per_group, size_t part_floats, bool adjacent) {
    return adjacent && slices_fit(nrows, tokens_per_group, 2 * kC, part_floats) ? LnBwdForm::Sums : LnBwdForm::ColsumsLnBwd;
}
bool attn16_seq_form(const AxisMap& ax);   // k_attn16.hip: 129 .. 256 positions
inline TrainAttnForm train_attn_form(bool bf16, const AxisMap& ax) {
    return !bf16 ? TrainAttnForm::Exact : attn16_seq_form(ax) ? TrainAttnForm::SeqRope : TrainAttnForm::Chunked;
}

void launch32_ln_mod(const float* x, long nrows, const ModMap& mm, int shift_chunk, int scale_chunk, int affine, float eps,
                     float* y, hipStream_t s, float* keep, bool y_bf16);   // keep (nullable): copy of x (training tape); y_bf16: y holds bf16 rows
// The linear layer (linear.h LinearParams): launch32_linear = the F32 form (the sampler's precision-32 path calls it directly).
// Stream*: p.wpack from launch16_pack_wstream, p.a_bf16 as the form says; p.c_bf16 with mode kLinGeluBwd only.
struct LinearParams;
void launch32_linear(const LinearParams& p, hipStream_t s);
void launch_linear(const LinearParams& p, LinearForm form, hipStream_t s);
// bf16 fragment stream of a weight for k16_linear_wdma: W(col, kk), col < m (a multiple of 384), kk < k (a multiple of 64),
// from nsrc <= 3 16-byte aligned fp32 matrices of row stride ld: turned == 0: src[col / seg] is [seg][k] (layers side by side along
// the columns); turned == 1: src[kk / seg] is [seg][m] (dX = dY W: the contraction runs over the weights' rows).  out: m * k * 2 bytes.
void launch16_pack_wstream(const float* const* src, int nsrc, int seg, int ld, int m, int k, int turned, void* out, hipStream_t s);
// backward kernels of the training step (k_fp32_bwd.hip)
// dW[j] += dY_j^T X of nseg <= 3 layers that share the input x and whose dY sit side by side (dy[n][j mseg + i]): one pass over x
// and dY.  dw[j] / db[j] may be null; db[j] += column sums of dY_j where dw_bias_rides(form, ...) -- else the caller runs launch32_colsum.
struct DwParams {
    const float* dy; int ldy;
    const float* x; int ldx;
    long n; int mseg, nseg, k;
    float* dw[3];
    float* db[3];
    float* part; size_t part_floats;
};
inline DwShape dw_shape(const DwParams& p) {
    return DwShape{p.n, p.mseg * p.nseg, p.k, p.ldy, p.ldx, (((unsigned long long)p.dy | (unsigned long long)p.x) & 15) == 0};
}
void launch_dw(const DwParams& p, DwForm form, hipStream_t s);
void launch32_colsum(const float* a, int lda, const float* b, int ldb, const float* roww, int mode, long nrows, int ncols,
                     long tokens_per_group, float eps, float* out, long ldo, float* part, size_t part_floats, hipStream_t s);
void launch32_ln_bwd(const float* x, const float* dy, long nrows, const ModMap& mm, int scale_chunk, int affine, float eps,
                     float* dx, int accumulate, hipStream_t s);
void launch32_gate_mul(const float* a, long nrows, const ModMap& mm, int gate_chunk, int gated, float* out, hipStream_t s);
void launch32_attn_bwd(const float* qkv, int ld, const AxisMap& ax, const MaskMap& mk, const float* bias_k,
                       const float* bias_v, const float* inv_freq, const float* o, const float* dout, float* dqkv,
                       float* stats, float* dbias, hipStream_t s, const float* lse_in);
void launch32_rope_bwd(float* buf, long ntok, int ld, long pos_div, int pos_mod, const float* inv_freq, float qscale,
                       hipStream_t s);
void launch32_loss_grad(const float* pred, const float* target, const float* mask, long per_sample, long B, float* den,
                        float* dpred, hipStream_t s, float* scratch, size_t scratch_floats);
void launch32_sum_frames(const float* a, int B, int T, int L, float* out, hipStream_t s);
void launch32_ipa_bwd(const IpaAttnParams& f, const float* dfeat, float* dproj, float* dhw, float* qrec, float* dheadw,
                      hipStream_t s, float* part, size_t part_floats);   // part: scratch for the sliced form
void launch32_gated_add(float* h, const float* u, long nrows, const ModMap& mm, int gate_chunk, int gated, hipStream_t s);
void launch32_gated_sum(float* h, const float* x, const float* u, long nrows, const ModMap& mm, int gate_chunk, hipStream_t s);
void launch32_gate_ln_mod(const float* xp, const float* up, long nrows, const ModMap& gm, int gate_chunk, const ModMap& mm,
                          int shift_chunk, int scale_chunk, float eps, float* y, float* keep, hipStream_t s, bool y_bf16);
void launch32_indicator(const int64_t* cm, long n, float* ind0, float* ind1, hipStream_t s);
void launch32_embed_rows_bwd(const float* dx0, const int64_t* aatype, int ngroups, int B, int L, float* dw, hipStream_t s);
void launch32_temb_bwd(const float* t_rows, int nrows, float tmul, const float* w0, const float* b0, const float* w2,
                       const float* b2, const float* dst, float* emb, float* h1, float* dpre1, float* dpre2, hipStream_t s);
void launch32_rope(float* buf, long ntok, int ld, long pos_div, int pos_mod, const float* inv_freq, hipStream_t s);
// out[nb][m] = x[nb][K] W[K][m], nb small and K long (split over K); false: partial buffer too small, nothing launched
bool launch32_skinny_wt(const float* x, int ldx, const float* W, int ldw, int nb, int m, long K, float* out, float* part,
                        size_t part_floats, hipStream_t s);
// gated residual h_out = h_in + gate * u, backward: du = gate * dh (du_bf16: written as bf16 rows, Sums only);
// out[g][0:384] += sum over group g of dh u.  part: partial sums (slice_plan)
struct GateBwdParams {
    const float *dh, *u;
    long nrows; ModMap mm; int gate_chunk;
    float* du; bool du_bf16;
    long tokens_per_group; float* out; long ldo;
    float* part; size_t part_floats;
};
void launch32_gate_bwd(const GateBwdParams& p, GateBwdForm form, hipStream_t s);
// LN + modulate backward: dx (+)= LN'(dy (1 + scale)); dshift[g][0:384] += sum dy, dscale[g][0:384] += sum dy xhat (the group's
// modulation-gradient row; Sums: the scale chunk right behind the shift chunk)
struct LnBwdParams {
    const float *x, *dy;
    long nrows; ModMap mm; int scale_chunk; float eps;
    float* dx; int accumulate;
    long tokens_per_group; float *dshift, *dscale; long ldo;
    float* part; size_t part_floats;
};
void launch32_ln_mod_bwd(const LnBwdParams& p, LnBwdForm form, hipStream_t s);
void launch32_transpose(const float* src, int rows, int cols, float* dst, hipStream_t s, int ldd);   // dst[c][r] (ld ldd) = src[r][c]
// Attention of the training step with its tape (lse: log-sum-exp per (token, head), written by the forward pass, read by the
// backward pass).  Exact: k_fp32.hip / k_fp32_bwd.hip; the bf16-operand (MFMA) forms: k_attn16.hip.  dqkv_bf16 (Seq* only): dq | dk |
// dv are written as bf16 rows (ld in elements).  Forward and backward of a sub-layer take the same form.
struct TrainAttnParams {
    const float* qkv; int ld;
    AxisMap ax; MaskMap mk;
    const float *bias_k, *bias_v, *inv_freq;
    float *out, *lse;
    const float* dout;                  // backward only, as what follows
    float *dqkv, *stats, *dbias;
    bool dqkv_bf16;
};
void launch_train_attn(const TrainAttnParams& p, TrainAttnForm form, hipStream_t s);
void launch_train_attn_bwd(const TrainAttnParams& p, TrainAttnForm form, hipStream_t s);
void launch32_attn(const float* qkv, int ld, const AxisMap& ax, const MaskMap& mk, const float* bias_k, const float* bias_v,
                   const float* inv_freq, float* out, hipStream_t s, float* lse_out);

// optimiser (k_optim.hip)
void launch_sumsq(const float* g, long n, float scale, float* partial, int nblocks, float* out, hipStream_t s);
void launch_adam(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                 float weight_decay, int adamw, float bc1, float bc2_sqrt, float grad_scale, const float* sumsq,
                 float max_norm, hipStream_t s);
void launch_ema(float* ema, const float* p, long n, float one_minus_decay, hipStream_t s);

// small kernels (k_small.hip)
void launch_temb(const float* t_rows, int nrows, float tmul, const float* w0, const float* b0, const float* w2,
                 const float* b2, float* silu_out, hipStream_t s);
void launch_adaln(const float* st, int nrows, const float* w, const float* b, int nout, float* mod, hipStream_t s);
void launch_rope_table(float* rope, const float* inv_freq, int npos, hipStream_t s);
// The learned bias key / value of the L == 4 residue-axis kernel (k_ln_qkv_attn4), functions of the weights alone: the key rotated at
// position 4 and rounded to bf16, the value rounded to bf16, as bf16 pairs in the order a (wave w, lane half hh) reads them for its heads
// 4w .. 4w+3: tab[((2w + hh) 4 + hd) 6 + q] = (value 2q, value 2q + 1) of the lane half's twelve; tab[kL4Tab + ...]: the bias value alike.
constexpr int kL4Tab = 192;
void launch_l4_bias_table(const float* bias_k, const float* bias_v, const float* rope, uint32_t* tab, hipStream_t s);
void launch_gather_f32(const float* src, const int* idx, float scale, float* dst, int n, hipStream_t s);
// part: 0 the weight rounded to bf16, 1 the bf16 of its rounding error (w - float(bf16(w))): the lo half of a bf16 pair
void launch_pack_rows(const float* w, int ld, const int* rowmap, int nft, int ksteps, float scale, bf16x8* dst,
                      hipStream_t s, int kappa = 0, int part = 0);
void launch_ipa_init(const float* aa_emb, const int64_t* aatype, const float* rel7, const float* w7, const float* b7,
                     float* h, int ngroups, int B, int L, hipStream_t s);
void launch_add_inplace(float* dst, const float* src, long n, hipStream_t s);
void launch_write_floats(const float* host_vals, int n, float* dst, hipStream_t s);
void launch_rel7(const float* r1, const float* t1, const float* r2, const float* t2, float* out7, long n, hipStream_t s);

// adaptive dopri5 sampler (k_ode.hip; orchestration in ode.inc).  Buffers: fp32 (B, T, L, D) states, 16-byte aligned.
constexpr int kOdeMaxTerms = 7;
constexpr int kOdeMaxParts = 1024;   // workgroups of a norm launch (its partials: [parts][2] fp64)
struct OdeTerms {                    // y = y0 + sum_{j < nk} c[j] k[j]
    const float* k[kOdeMaxTerms];
    float c[kOdeMaxTerms];
    int nk;
};
struct OdeNorm {
    // mode 0: a = x0, b = k1 -> rms(x0 / scale), rms(k1 / scale) with scale = atol + |x0| rtol
    // mode 1: a = x0, b = k1, k[0] = f1 -> rms((f1 - k1) / scale)
    // mode 2: a = y0, b = y1, k[0..6], e -> rms(sum_j e_j k_j / (atol + rtol max(|y0|, |y1|)))
    const float *a, *b;
    const float* k[kOdeMaxTerms];
    float e[kOdeMaxTerms];
    double atol, rtol;
    int mode;
};
void launch_ode_combine(float* out, const float* y0, const OdeTerms& p, long n, hipStream_t s);
int ode_norm_parts(long n);
void launch_ode_norm(const OdeNorm& p, long n, double* part, double* out, hipStream_t s);   // out[0], out[1]: the two rms values
void launch_ode_dense(float* out, const float* y0, const float* y1, const float* f0, const float* f1, const float* ym, float dt,
                      float sfrac, long n, hipStream_t s);

// fixed-grid Runge-Kutta sampler (k_rk.hip; tableau and orchestration in ode.inc).  A stage's state is never written to HBM: the
// launch that embeds it forms it from y0 and the step's velocities.  RkForm: the arithmetic of one state, every written operation
// one rounded fp32 operation (no contraction), k0 .. k3 = RkState::k[0 .. 3]:
enum RkForm : int {
    kRkY0 = 0,     // y0                                            (first stage of the first step)
    kRkAxk,        // y0 + k0 * c0                                  (c0 already holds the step size)
    kRkDtCk,       // y0 + dt * (c0 * k0)
    kRkDtkC,       // y0 + (dt * k0) * c0
    kRkDtLin2,     // y0 + dt * (c0 * k0 + c1 * k1)
    kRkDtLin3,     // y0 + dt * ((c0 * k0 + c1 * k1) + c2 * k2)
    kRk38,         // y0 + (((k0 + c0 * (k1 + k2)) + k3) * dt) * c1  (the 3/8 rule's result)
    kRkForms
};
constexpr int kRkMaxK = 4;
struct RkState {
    int form, nk;                  // RkForm; velocities the form reads (k[0 .. nk - 1])
    int store;                     // the state is the step's result y1: it is also stored over y (each element by the thread that read it)
    float dt, c[3];
    const float* k[kRkMaxK];
    float* y;                      // y0 (B, T, L, D)
};
// k_embed on the state `st` describes -- literally: one device body (state_embed.h) and one launch selection (embed_dispatch) serve
// k_embed, this kernel and k_sde_embed.  p.x is not read: st.y is
void launch_rk_embed(const EmbedParams& p, const RkState& st, hipStream_t s);
// y <- the state `st` describes, elementwise over n values (the result of the last step)
void launch_rk_update(const RkState& st, long n, hipStream_t s);

// SDE sampler (k_sde.hip; plan and orchestration in sde.inc): the states of an Euler-Maruyama or Heun step, formed like the
// Runge-Kutta states inside the launch that embeds them.  With the coefficients of evaluation time j (SdeState::R[j], iV[j], D[j])
//   F_j(v, x) = v + D_j * (((R_j * v) - x) * iV_j)        (velocity + diffusion * score)
// and xi the step's noise, every written operation one rounded fp32 operation:
enum SdeForm : int {
    kSdeX = 0,       // x                                                   (first evaluation of an Euler-Maruyama solve)
    kSdeNoise,       // x + G * (xi * q)                                    (Heun: xh of the first step)
    kSdeEm,          // (x + F_0(v0, x) * dt) + G * (xi * q)                (an Euler-Maruyama step)
    kSdeDrift,       // x + dt * F_0(v0, x)                                 (Heun's predictor xp; the Mean last step, dt = its size)
    kSdeHeun,        // x + hdt * (K1 + K2), K1 = F_0(v0, x), K2 = F_1(v1, x + dt * K1)
    kSdeHeunNoise,   // kSdeHeun + G * (xi * q)                             (G, xi: the NEXT step's)
    kSdeTweedie,     // x * c0 + c1 * (((R_0 * v0) - x) * iV_0)             (c0 = 1 / alpha, c1 = sigma^2 / alpha)
    kSdeEuler,       // x + v0 * dt                                         (the Euler last step, dt = its size)
    kSdeForms
};
struct SdeState {
    int form;
    int store;                     // the state is also stored over y (each element by the thread that read it)
    float dt, hdt, q, G;           // step size, 0.5 dt, sqrtf(dt), sqrtf(2 D) of the noise term's time
    float R[2], iV[2], D[2];       // coefficients of up to two evaluation times
    float c[2];
    const float* v[2];             // velocities; null where the form reads none
    const float* xi;               // the noise of one step (B, T, L, D), or null
    float* y;                      // x (B, T, L, D)
    // the generated noise (philox.h) in the buffer's place: with `rng` the noise-reading forms compute xi at the element's coordinates
    const uint64_t* rng;           // device: {seed, sample_base, block_base, 0}, read inside the kernel; null: xi is read from the buffer
    int step, block;               // counter words c2 and (added to block_base) c3
    int b0;                        // the first sample of the launch within the call's batch (a view: set by its loop)
    unsigned per_b;                // T L D: elements of one sample
};
void launch_sde_embed(const EmbedParams& p, const SdeState& st, hipStream_t s);
void launch_sde_update(const SdeState& st, long n, hipStream_t s);

// SE(3) / pre / post (k_se3.hip)
void launch_rigid_compose(long n, const float* r1, const float* t1, const float* r2, const float* t2, float* ro,
                          float* to, hipStream_t s);
void launch_rigid_invert(long n, const float* r, const float* t, float* ro, float* to, hipStream_t s);
void launch_rigid_apply(long n, long ppf, const float* r, const float* t, const float* pts, float* out, int inverse,
                        hipStream_t s);
void launch_quat_to_rot(long n, const float* q, int normalize, float* rot, hipStream_t s);
void launch_from_3_points(long n, const float* pnx, const float* org, const float* pxy, float* rot, float* trans,
                          hipStream_t s);
void launch_rot_to_quat(long n, const float* rot, float* q, hipStream_t s);
void launch_prep_latents(int B, int T, int L, int tps, int bcast, int cond_interval, const float* rots, const float* trans,
                         const float* tors, float* latents, float* x_cond, int64_t* x_cond_mask, hipStream_t s);
void launch_prep_keyframes(int B, int T, int L, int cond_interval, const float* key_rots, const float* key_trans,
                           const float* key_tors, float* x_cond, int64_t* x_cond_mask, float* start_rot, float* start_trans,
                           hipStream_t s);
void launch_samples_to_atom14(int B, int T, int L, int D, int tps, const float* samples, const float* rot0,
                              const float* trans0, const int64_t* seqres, const float* default_frames,
                              const float* lit_positions, const int64_t* atom14_group, const float* atom14_mask,
                              float* atom14, int out_T, int out_t0, hipStream_t s);
void launch_atom14_to_cond(int B, int L, const float* atom14, long in_bstride, const int64_t* seqres,
                           const int64_t* a37to14, const float* a37mask, const int64_t* chi_idx, const float* chi_mask,
                           float* rots, float* trans, float* tors, float* tmask, hipStream_t s);

// multi-model PDB text (k_pdb.hip): count -> scan -> format; status[0] must be zero on entry
void launch_pdb_format(long M, int L, long model_base, const float* atom14, const int64_t* aatype, const int64_t* a37to14,
                       const float* a37mask, const uint8_t* templates, const uint8_t* ter_template, int64_t* offsets,
                       uint8_t* text, long text_capacity, int64_t* status, hipStream_t s);

// trajectory analysis (k_analysis.hip).  The index tables are HOST arrays, checked by the caller: they travel as kernel arguments,
// kQuadChunk quadruples / kPairChunk pairs a launch.
constexpr int kQuadChunk = 64;
constexpr int kPairChunk = 64;
constexpr int kHistMaxCells = 16384;   // ints of LDS a histogram may take: bins1 and bins2 * bins2
struct QuadChunk {
    int q[kQuadChunk][4];
};
struct PairChunk {
    int p[kPairChunk][2];
};
void launch_dihedrals(long F, int L, int NF, const float* atom14, const int32_t* quad_host, float* angles, hipStream_t s);
// hist1 [NF][bins1], hist2 [P][bins2][bins2] and dropped [NF + P] must be zero on entry
void launch_torsion_hist(long F, int NF, const float* angles, int bins1, const double* edges1, int P, const int32_t* pairs_host,
                         int bins2, const double* edges2, int64_t* hist1, int64_t* hist2, int64_t* dropped, hipStream_t s);
int acov_splits(long n, int NF, long K);
size_t acov_workspace_bytes(long n, int NF, long K);
long acov_groups(long n, int NF, long K);   // workgroups of k_sincos_acov
void launch_sincos_acov(long n, int NF, long K, const float* angles, double* acov, double* mean_sin, double* mean_cos, void* ws,
                        hipStream_t s);
// acov[f][k] = (sum over the splits, in split order, of partial[f][split][k]) / (n - k)
void launch_acov_finish(const double* partial, long n, long K, int NF, int splits, double* acov, hipStream_t s);

// tICA (k_tica.hip): lagged second moments of the cos/sin features, the projection, a plain series' autocovariance, and 2-D
// histograms with an edge table per pair and axis
constexpr int kTicaMaxFeatures = 64;   // torsions: D = 2 NF <= 128 features
size_t moments_workspace_bytes(long n, int NF, long lag);
void launch_lagged_moments(long n, int NF, long lag, const float* angles, double* sx, double* sy, double* cxx, double* cyy, double* cxy,
                           void* ws, hipStream_t s);
void launch_project(long n, int NF, int d, const float* angles, const float* mean, const float* W, float* out, hipStream_t s);
size_t series_acov_workspace_bytes(long n, int NS, long K);
void launch_series_acov(long n, int NS, long K, const float* x, double* acov, double* mean, void* ws, hipStream_t s);
// hist2 [P][bins][bins] and dropped [P] must be zero on entry
void launch_hist_xy(long F, int NC, const float* values, int P, const int32_t* pairs_host, int bins, const double* edges_x,
                    const double* edges_y, int64_t* hist2, int64_t* dropped, hipStream_t s);

// k-means / MSM (k_msm.hip): the nearest centre of every point, one Lloyd step, k-means++ rounds and the sliding-window count matrix
constexpr int kKmMaxDim = 128;       // d: tICA components
constexpr int kKmMaxCenters = 256;   // k
size_t kmeans_step_workspace_bytes(long n, int d, int k);
size_t kmeans_pp_workspace_bytes(long n);
void launch_kmeans_assign(long n, int d, int k, const float* x, const float* centers, int32_t* assign, float* dist2, hipStream_t s);
void launch_kmeans_step(long n, int d, int k, const float* x, float* centers, int32_t* assign, double* sums, int64_t* counts,
                        double* cost, int32_t* state, double tol, void* ws, hipStream_t s);
// rounds r0 .. r1 - 1; u_host [k] in [0, 1)
void launch_kmeans_pp(long n, int d, const float* x, const double* u_host, int r0, int r1, int64_t* chosen, float* mind2, void* ws,
                      hipStream_t s);
// counts [k][k] and dropped [1] must be zero on entry; lag < n
void launch_count_matrix(long n, long lag, int k, const int32_t* dtraj, int64_t* counts, int64_t* dropped, hipStream_t s);

// transition paths (k_tps.hip): Markov-bridge paths of a k-state chain and their likelihood under a second chain of kb states
constexpr int kTpMaxStates = 64;     // k, kb
constexpr int kTpMaxLen = 4096;      // N
struct TpPhi {                       // the checked host map from Ta's states into Tb's: it travels as a kernel argument
    uint8_t v[kTpMaxStates];
};
// kb = 0: no scoring set (Tb, Bb, prob unused)
void launch_tp_sample(long n_samples, int N, int k, const double* Ta, const double* Ba, int start, int end, uint64_t seed,
                      uint32_t stream_id, uint64_t sample_base, int kb, const double* Tb, const double* Bb, const TpPhi& phi,
                      int32_t* paths, double* prob, hipStream_t s);

// Cartesian ensemble statistics (k_ensemble.hip): superposition, per-atom moments, all-pairs squared distances, contact counts
constexpr int kEnsMaxAtoms = 16384;             // A
constexpr long kEnsMaxPairFrames = (1l << 20) - 1;   // Fa, Fb of the all-pairs distances
constexpr int kEnsMaxResidues = 4096;           // N of the contact counts
constexpr int kEnsWaveAtoms = 256;              // superposition: up to here a wave owns a frame, beyond a workgroup does
constexpr int kEnsPairTileA = 128;              // all-pairs distances: xa frames of a tile ...
constexpr int kEnsPairTileB = 64;               // ... xb frames ...
constexpr int kEnsPairChunk = 24;               // ... and the coordinates staged at a time
// w is device memory and has passed the caller's check (>= 0, three positive)
void launch_ens_superpose(long F, int A, const float* x, const float* ref, const float* w, const uint8_t* exists, float* out,
                          double* rot, double* rmsd, hipStream_t s);
size_t ens_moments_workspace_bytes(long F, int A);
void launch_ens_moments(long F, int A, const float* x, double* mean, double* cov, void* ws, hipStream_t s);
size_t ens_pairwise_workspace_bytes(long Fa, long Fb);
void launch_ens_pairwise_d2(long Fa, long Fb, int A, const float* xa, const float* xb, float* d2, double* sums, void* ws,
                            hipStream_t s);
// counts [N][N] must be zero on entry
void launch_ens_contact_counts(long F, int N, const float* ca, float cutoff2, int32_t* counts, hipStream_t s);
// Shrake-Rupley counts: ws holds fp32 R [A] (0: no atom), R2 [A] and the points axis-major [3][P], staged by the caller
constexpr int kEnsSasaMaxPoints = 4096;         // P
constexpr int kEnsSasaMaxNeighbours = 512;      // a wave's LDS neighbour list; more within reach: every atom is tested instead
constexpr float kEnsSasaMaxRadius = 16.f;       // every radius, and the probe
size_t ens_sasa_workspace_bytes(int A, int P);
void launch_ens_sasa_counts(long F, int A, int P, const float* x, const float* ws, int32_t* counts, hipStream_t s);

}  // namespace mdg
