/*
 * mdgen_amd.h -- C-ABI of the MI355X-native MDGen denoising sampler (libmdgen_amd.so).
 *
 * The reference (bjing2016/mdgen) is pure Python/PyTorch and has no FFI of its own; its boundary
 * for this path is the Python call surface.  Each entry point below
 * names the reference code it replaces (paths relative to the reference repo).  The Python host
 * (`mdgen_amd/`) keeps the reference's signatures and calls these through ctypes.
 *
 * Conventions
 *   - plain C, no C++/torch types.  All tensor arguments are DEVICE pointers (row-major,
 *     contiguous, layouts exactly as the reference's tensors) unless the name ends in `_host`.
 *   - the caller owns every input/output/workspace buffer; the library owns only the packed
 *     weights and cached hipGraph handles inside the opaque context.
 *   - every launch goes on the caller's `stream` (a hipStream_t passed as void*) and nothing inside a
 *     call synchronises the device (graph-capturable).  One exception, documented: `mdgen_sample_euler`
 *     forks the second half of the batch onto one context-owned stream and joins it back onto `stream`
 *     before returning (event fork/join, no host wait; option "streams" = 1 disables it).  A second:
 *     `mdgen_sample_dopri5` reads its error ratio back once per attempted step (8 bytes, stream synchronised).
 *   - return 0 on success, negative = invalid argument / state, positive = hipError_t.
 *     `mdgen_last_error()` returns a thread-local message.  No exceptions cross the ABI.
 *   - a context is not thread-safe; use one per device per process.
 *   - compiled for gfx950 only; C = 384, heads = 16, head_dim = 24, ffn = 1536 are compile-time.
 */
#ifndef MDGEN_AMD_H
#define MDGEN_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever a public struct or signature changes; mdgen_amd/_lib.py refuses a library whose version differs. */
#define MDGEN_ABI_VERSION 8   /* 6: mdgen_ws_layout.split; 7: mdgen_ws_layout.fold; 8: mdgen_cond replaces nine pointer arguments */

typedef struct mdgen_ctx mdgen_ctx;

/* 0 for a product library; 1 if the .so was built with a kernel experiment switch (csrc/dev.h, scripts/micro/): measurement
 * builds with cycle stamps in the kernels.  mdgen_amd/_lib.py loads such a library only when MDGEN_AMD_LIB names it explicitly. */
int32_t mdgen_dev_build(void);

/* Model hyper-parameters (reference argparse flags, mdgen/parsing.py:79-120). */
typedef struct mdgen_model_desc {
    int32_t embed_dim;      /* must be 384 */
    int32_t mha_heads;      /* must be 16  */
    int32_t num_layers;     /* trunk layers == IPA layers (reference default 5), 1..8 */
    int32_t latent_dim;     /* 21 (forward-sim) or 28 (TPS); wrapper.py:196 */
    int32_t ipa_heads;      /* must be 4  */
    int32_t ipa_head_dim;   /* must be 32 */
    int32_t ipa_qk;         /* must be 8  */
    int32_t ipa_v;          /* must be 8  */
    int32_t abs_pos_emb;    /* 1: add pos_embed[1,crop,C] (latent_model.py:234-235) */
    int32_t crop;           /* rows of pos_embed (>= L when abs_pos_emb) */
    int32_t tps_condition;  /* 1: two-stream IPA with relative-frame inputs (latent_model.py:193-207) */
    float   time_multiplier;/* latent_model.py:243 (100) */
} mdgen_model_desc;

/* Problem shape of one call: x is (B,T,L,D). */
typedef struct mdgen_shape {
    int32_t B, T, L;
} mdgen_shape;

/* Byte offsets into the caller-provided workspace (for tests / debugging / profiling). */
typedef struct mdgen_ws_layout {
    size_t total_bytes;
    size_t h;          /* fp32 residual stream        [N][384]                         */
    size_t qf, kf, vf; /* bf16 attention operand fragments (DESIGN.md "fragment layout") */
    size_t obuf;       /* bf16 attention output       [N][384]                         */
    size_t mod;        /* fp32 adaLN table            [R][77*384]                      */
    size_t silu_t;     /* fp32 SiLU(t_embedder(t))    [R][384]                         */
    size_t ipa_out;    /* fp32 IPA-stack table        [S][B*L][384]                    */
    size_t h_ipa;      /* fp32 IPA-stack residual     [S*B*L][384] (x2 when TPS)       */
    size_t ipa_proj;   /* fp32 IPA projections        [S*B*L][672]                     */
    size_t ipa_feat;   /* bf16 IPA concat features    [S*B*L][256]                     */
    size_t mask_bl;    /* fp32 compact mask[:,0]      [B][L]                           */
    size_t rel7;       /* fp32 TPS relative frames    [2][B][L][7]                     */
    size_t tgrid;      /* fp32 per-step times         [S][B]                           */
    size_t f32_scratch;/* fp32 path: LN out | q,k,v | attention out | MLP hidden | IPA features (0 bytes unless the
                          context keeps fp32 weights)                                            */
    size_t split;      /* scratch of the split-panel MLP kernel (option "small_split"): arrival counters (1 KiB) | fp32 partials |
                          private residual rows, [panels <= 96][3][64][384] each                 */
    size_t fold;       /* option "mlp_fold": per (step, trunk layer) the MLP weight stream with that step's gate folded into fc2
                          [S][layers][2304 KiB bf16 fragments] | gate * fc2.bias [S][layers][384] fp32 (0 bytes unless t_shared and
                          the trunk's MLP launches take the row-owner kernel)                    */
    size_t embase;     /* option "mlp_tail": the x-independent part of the token embedding per (step, b, l), [S][B*L][384] fp32, for the
                          steps whose embedding is computed by the previous step's last MLP launch (0 bytes unless `fold` and S > 1) */
} mdgen_ws_layout;

const char* mdgen_last_error(void);
int32_t     mdgen_abi_version(void);

/* ---- context / weights -------------------------------------------------------------------
 * Replaces `NewMDGenWrapper.load_from_checkpoint(...).eval().to('cuda')` (sim_inference.py:129-130)
 * for the `model.*` sub-tree of the Lightning state_dict.  Weights are handed over one tensor
 * at a time under the reference's own state_dict key (e.g. "layers.0.mha_t.attn.q_proj.weight");
 * `data` is an fp32 DEVICE pointer; the library re-packs into its MFMA fragment formats on
 * `stream`.  `mdgen_ctx_finalize` fails if any required key was not provided. */
int32_t mdgen_ctx_create(mdgen_ctx** out, const mdgen_model_desc* desc);
int32_t mdgen_ctx_destroy(mdgen_ctx* ctx);
int32_t mdgen_ctx_set_weight(mdgen_ctx* ctx, const char* key, const float* data,
                             const int64_t* shape, int32_t ndim, void* stream);
int32_t mdgen_ctx_finalize(mdgen_ctx* ctx, void* stream);
/* Run-time options (no environment variables are read by the library):
 *   "streams"          1..8, default 2: contiguous sub-batches of an Euler rollout run on this many concurrent
 *                      streams (the caller's + context-owned ones, fork/join by events inside the call).  While the
 *                      option has not been set, the count is also limited to pieces of >= 256 64-row panels (a piece that
 *                      does not fill the chip by itself gains nothing from running beside another one);
 *   "keep_fp32_weights" 0/1, default 0; set to 1 BEFORE handing weights over to keep an fp32 copy of each (137 MB);
 *   "precision"        16 (default): bf16 MFMA operands, fp32 accumulate / softmax / LayerNorm / residual stream
 *                      (rel-L2 4-6e-3 per network evaluation against the fp32 reference);
 *                      32: fp32 operands everywhere (v_mfma_f32_32x32x2_f32, csrc/k_fp32.hip), the reference's own
 *                      arithmetic -- a tolerance mode ~10x slower; needs keep_fp32_weights;
 *   "residue_l4_path"  residue-axis attention sub-layer when L == 4: 2 (default) one kernel for the whole
 *                      sub-layer, 1 attention inside the QKV kernel + separate out-projection, 0 the general
 *                      L <= 8 path.  All three compute mha.py:258-397 + latent_model.py:457-462.
 *   "attention_path"   tiled attention (sequence > 8 positions; mha.py:359-396): 0 (default) softmax with a FIXED
 *                      shift anchored on the first key tile, an overflow test per query row at the end and an
 *                      automatic re-run of the affected (head, 64 queries) on the robust loop; 1 the robust loop
 *                      (running row max, shift re-anchored as it grows) for everything.  Same results to fp32
 *                      rounding; 1 is ~1.5x slower.
 *   "mlp_path"         the MLP block (latent_model.py:478-481, layers.py:77-84): 0 the 64-row resident-panel kernel
 *                      (csrc/k_gemm.hip k_mlp); 1 (default) the row-owner kernel (csrc/k_rows.hip k_mlp_rows: a wave owns 32
 *                      rows, activations in registers, weights as one LDS-DMA stream) for launches of >= 768 row tiles,
 *                      which fill the chip, and the panel kernel below that; 2 the row-owner kernel always.
 *   "mlp_fold"         1 (default) / 0: calls whose batch shares t (mdgen_sample_euler / mdgen_rollout_euler; integrators.py:99) have ONE
 *                      MLP gate vector per (step, layer): it is folded into the weights once per call -- W2' = diag(gate) W2 rounded to
 *                      bf16 once from the fp32 weight, b2' = gate * b2 -- so that h + gate * (W2 u + b2) (latent_model.py:481) becomes
 *                      "accumulators start at h + b2', accumulate W2' u, store": the row-owner kernel reads the residual rows once
 *                      instead of twice.  Same values to the bf16 rounding of gate * w instead of w.  Workspace: mdgen_ws_layout.fold
 *                      (S x layers x 2.36 MB); the report tags such launches "mlp@fold".
 *   "mlp_tail"         2 (default) / 1 / 0: with mlp_fold, the FinalLayer (layers.py:57-74: LN + modulate, Linear C -> D) and the Euler update of x
 *                      (integrators.py:106) run inside the LAST trunk layer's folded MLP kernel, on the updated rows while they are in
 *                      registers; that kernel then does not store its rows (nothing reads the residual stream after the last layer) and
 *                      there is no k_final launch: 196 MB less HBM traffic per network evaluation.  Not with trace_h.  Same values to
 *                      fp32 summation order; the report tags the launch "mlp@fold+final".  In a rollout the same launch goes on to
 *                      compute the NEXT step's token embedding (latent_model.py:233-246) from the state it has just updated and
 *                      writes it as that step's residual stream ("mlp@fold+final+embed"): steps 1 .. S-1 launch no k_embed (value 2;
 *                      1: the FinalLayer + Euler update only; workspace: mdgen_ws_layout.embase).
 *                      The products of that embedding tail (W_l x, W_c x_cond: K = 21 / 28) run on the bf16 MFMA with each operand
 *                      split into a bf16 pair hi + lo (16 mantissa bits per side, the lo x lo term dropped: 2^-17 of a product).
 *   "fuse_proj"        the temporal attention's out-projection + gated residual (mha.py:397, latent_model.py:476) as a prologue
 *                      phase of the 64-row panel MLP kernel (k_mlp<3, true>), ahead of the MLP: 3 (default) where the launch
 *                      takes the panel kernel (fewer than 768 row tiles, or mlp_path 0: one launch less per layer, +2 %), 0 off.
 *   "fuse_proj_qkv"    1 (default) / 0: residue axis on the tiled-attention path (L > 8): its out-projection + gated residual
 *                      (mha.py:397, latent_model.py:462) runs inside the temporal sub-layer's LN -> q, k, v kernel, whose panels
 *                      then normalise rows that are still in L2 (k_ln_qkv<false, true>; one launch and one HBM read of the
 *                      residual stream less per layer).
 *   "flash_proj"       tiled attention (sequence > 8 positions) and the sub-layer's out-projection + gated residual (mha.py:359-397,
 *                      latent_model.py:462,476) in ONE launch (csrc/k_flash.hip k_flash_proj: a workgroup owns 64 queries of a
 *                      sequence for all 16 heads, the attention output stays in LDS as the projection's A operand): 1 (default)
 *                      for launches of >= 512 such workgroups (cfg-2, ATLAS), 0 never (k_flash, then k_proj<0> or a projection
 *                      deferred into the next kernel per fuse_proj / fuse_proj_qkv), 2 always.  Same values as the separate
 *                      kernels (same operands, same summation order).
 *   "flash_rotate"     1 (default) / 0: tiled attention, fixed-anchor loop: the 64-query chunks of a sequence walk its key tiles from
 *                      different starting tiles (chunk c of n starts at tile c * tiles / n and wraps): chunks that start together then
 *                      miss on different fragments instead of queueing behind one chain of HBM misses.  A sum over keys: same
 *                      values to fp32 rounding.
 *   "flash_proj_form"  0 (default) / 4 / 8: which fused kernel: k_flash_proj (four waves, a 64-query panel, two workgroups per CU) or
 *                      k_flash_proj8 (eight waves, a 128-query panel, four query tiles per wave, one workgroup per CU).  0: the
 *                      128-query form for sequences of >= 512 positions whose launch gives every CU a workgroup, else the 64-query
 *                      form.  Same values up to the order in which a query's keys are summed (fp32 rounding).
 *   "panel_waves"      0 (default) / 4 / 8: the 64-row panel kernels that exist in a four- and an eight-wave form (k_mlp / k_mlp8,
 *                      k_ln_qkv<false> / k_ln_qkv8) take the eight-wave form for launches of at most one workgroup per CU; 4 / 8
 *                      force one form whatever the launch size (tests, A/B runs).  mdgen_profile_report tags the class of such
 *                      a launch with "@p4" / "@p8".
 *   "small_split"      1 (default) / 0: launches far below one workgroup per CU (B = 1: sim_inference.py runs one trajectory; the IPA
 *                      stack) give a 64-row panel to several workgroups: the MLP block's twelve hidden chunks go to three workgroups
 *                      on one XCD (k_mlp8<., 3>, launches of <= CUs / 3 panels; fp32 partials of the second product meet in L2, the
 *                      last arriver adds them in a fixed order and runs the gated residual epilogue -- bit-reproducible, nobody
 *                      waits) and q, k | v of the temporal LN -> q, k, v kernel to two (k_ln_qkv8<true>, <= CUs / 2 panels).
 *                      Scratch: mdgen_ws_layout.split.  Same values to fp32 rounding (a three-term instead of a two-term sum);
 *                      the report tags such launches "@p8x3" / "@p8x2".  Off while a call runs sub-batch streams.
 *                      Round 6: ... and give the L = 4 residue sub-layer kernel and the split q, k | v kernel 32-ROW workgroups where
 *                      even those fit one per CU (k_ln_qkv_attn4<true, true>: B <= 2 at T 1000, the IPA stack; k_ln_qkv8<true, true>:
 *                      B = 1 at T 1000): twice the workgroups on twice the CUs, half the rows per SIMD -- a small launch lasts as long
 *                      as one wave's chain of work.  Same arithmetic per row; tags "@h32" / "@h32x2"; no scratch, so these two stay
 *                      on while a call runs sub-batch streams.
 *   "train_precision"  operands of the matrix products of mdgen_train_forward_backward (linear layers, weight gradients,
 *                      the attention's q k^T / p v and their backward): 32 (default) fp32, the exact mode; 16 rounded to
 *                      bf16 on the MFMA, fp32 accumulation, fp32 master weights and activations (train.py:13
 *                      set_float32_matmul_precision('medium')); softmax, LayerNorm, reductions stay fp32, GELU to 5e-6.
 *                      With 16, attention axes of 129 .. 256 positions take the sequence-resident kernels (RoPE applied inside),
 *                      the trunk's GEMM-only tensors are stored as bf16 rows, and with train_streams 2 the turned weights of the
 *                      small dX products are computed ahead on the second stream (~30 MB context-owned buffer at cfg-5).
 *   "train_streams"    2 (default) / 1: mdgen_train_forward_backward launches the weight / bias gradients (nothing reads them
 *                      before the optimiser) on a second stream of the context, beside the backward pass's critical path on the
 *                      caller's stream; it joins the caller's stream before the call returns, and milestone events are recorded
 *                      once both streams have reached them.  Bit-identical gradients; 33.9 -> 29.9 ms per step at cfg-5's
 *                      per-GPU size.
 * Returns -4 for an unknown name, -2 for a value out of range. */
int32_t mdgen_ctx_set_option(mdgen_ctx* ctx, const char* name, int32_t value);
/* number of state_dict keys the model needs; name of the i-th (for loaders / tests) */
int32_t mdgen_ctx_num_weights(const mdgen_ctx* ctx);
const char* mdgen_ctx_weight_name(const mdgen_ctx* ctx, int32_t i);

/* ---- workspace ---------------------------------------------------------------------------
 * `n_steps` = number of distinct time rows prepared per call (1 for a single forward, S for an
 * S-step Euler rollout).  `t_shared` = 1 when all batch elements share t within a step (always true
 * in sampling, integrators.py:99), which de-duplicates the adaLN table. */
int32_t mdgen_workspace_layout(const mdgen_ctx* ctx, const mdgen_shape* shape, int32_t n_steps,
                               int32_t t_shared, mdgen_ws_layout* out);

/* ---- conditioning ------------------------------------------------------------------------
 * What every network evaluation reads besides x and t: the arguments mask, start_frames, end_frames, x_cond, x_cond_mask, aatype
 * of `LatentMDGenModel.forward` (latent_model.py:212-216).  mask in {0,1}; x_cond_mask int64 in {0,1}; aatype int64 in [0,20];
 * start / end frames: rot + trans, the fields of the reference's `Rigid`; end_* may be NULL unless tps_condition.
 * rel7 (nullable; two-sided models only): the relative-frame inputs of latent_to_emb_f / _r exactly as the caller's reference
 * computes them -- rel7[0] = (start^-1 o end).to_tensor_7(), rel7[1] = (end^-1 o start).to_tensor_7() (latent_model.py:193-195).
 * Their quaternion SIGN is whatever torch.linalg.eigh returns (rigid_utils.py:191-210, never canonicalised on this path) and it
 * reaches a Linear, so a checkpoint trained with the reference sees exactly its own inputs only when they are handed over; NULL:
 * the library computes them from the frames with the sign fixed to w >= 0.
 * A NULL struct or a NULL required field (all but end_rot, end_trans, rel7) is refused with -1. */
typedef struct mdgen_cond {
    const float*   mask;          /* (B,T,L) */
    const float*   start_rot;     /* (B,L,3,3) */
    const float*   start_trans;   /* (B,L,3) */
    const float*   end_rot;       /* nullable unless tps_condition */
    const float*   end_trans;
    const float*   rel7;          /* nullable; (2,B,L,7) */
    const float*   x_cond;        /* (B,T,L,D) */
    const int64_t* x_cond_mask;   /* (B,T,L) */
    const int64_t* aatype;        /* (B,L) */
} mdgen_cond;

/* ---- denoiser ----------------------------------------------------------------------------
 * `LatentMDGenModel.forward` / `.forward_inference` (latent_model.py:212-269), non-design path:
 *   out[B,T,L,D] = model(x, t, mask, start_frames, end_frames, x_cond, x_cond_mask, aatype)
 * x, out: fp32 (B,T,L,D); t: fp32 (B); the conditioning: mdgen_cond above.  trace_h (nullable): fp32 [(num_layers+1)][N][384],
 * the residual stream before layer 0 and after every trunk layer; trace_ipa (nullable): fp32
 * [B*L][384], the IPA-stack output (latent_model.py:245-246). */
int32_t mdgen_denoiser_forward(mdgen_ctx* ctx, const mdgen_shape* shape,
                               const float* x, const float* t, const mdgen_cond* cond,
                               float* out, float* trace_h, float* trace_ipa,
                               void* workspace, size_t workspace_bytes, void* stream);

/* `Sampler.sample_ode(sampling_method='euler', num_steps=n_steps+1)` -> `ode.sample` ->
 * torchdiffeq fixed-grid Euler (transport.py:408-451, integrators.py:95-114) with the velocity
 * drift (transport.py:242-244): x <- x + (t[i+1]-t[i]) * model(x, t[i]) on t = linspace(0,1,n_steps+1).
 * `x` holds the noise zs on entry and samples[-1] on exit (the only state the wrapper reads,
 * wrapper.py:447).  use_graph=1 captures the whole rollout into a hipGraph on first use (keyed on
 * shape + pointers) and replays it afterwards; `stream` must then be a non-default stream. */
int32_t mdgen_sample_euler(mdgen_ctx* ctx, const mdgen_shape* shape, int32_t n_steps,
                           float* x, const mdgen_cond* cond,
                           void* workspace, size_t workspace_bytes, int32_t use_graph, void* stream);

/* The reference's default solver: `sample_ode(sampling_method='dopri5')` -> torchdiffeq 0.2.x
 * odeint(f, x0, linspace(0, 1, 50), method='dopri5', atol=[atol], rtol=[rtol])[-1] (transport.py:408-451,
 * integrators.py:74-113; wrapper.py:441-447 takes the method from the checkpoint's args, default 'dopri5', parsing.py:102).
 * Adaptive Dormand-Prince with torchdiffeq's mixed precision (fp32 state, fp64 times / tolerances / norms; csrc/ode.inc):
 * the error norm is the RMS over the WHOLE (B, T, L, D) state, so one step size is shared by the batch -- a B = 2 call is a
 * valid solve, but not the two B = 1 solves the reference would run for two separate calls.
 *   x            (B,T,L,D) fp32, 16-byte aligned: the noise on entry, the state at t = 1 on exit (the step's dense output)
 *   max_steps    limit on attempted steps (an error when exceeded)
 *   stats_host   [3] out: network evaluations (2 + 6 x attempted steps), accepted steps, rejected steps (also on error)
 *   steps_host   nullable, [max_steps][2] out: (t0, dt) of every accepted step, fp64
 *   workspace    mdgen_dopri5_workspace_bytes: the network workspace for six t-shared time rows + 9 state buffers + partials
 * Exception to "nothing synchronises": after every attempted step the error ratio (8 bytes) is copied into pinned memory
 * and `stream` is synchronised.  A stream that is being captured is refused (-8) before anything is enqueued.  Errors:
 * -9 non-finite norm / error ratio, -10 more than max_steps attempts, -11 dt underflow (t0 + dt == t0). */
int32_t mdgen_sample_dopri5(mdgen_ctx* ctx, const mdgen_shape* shape, double atol, double rtol, int32_t max_steps,
                            float* x, const mdgen_cond* cond,
                            void* workspace, size_t workspace_bytes, int32_t* stats_host, double* steps_host, void* stream);
int32_t mdgen_dopri5_workspace_bytes(const mdgen_ctx* ctx, const mdgen_shape* shape, size_t* bytes);

/* Host-only test hook (no GPU): mdgen_sample_dopri5's step-size controller replayed on given norms.  init = {d0, d1,
 * rms((f1 - k1) / scale)} of the initial-step rule; ratios[i]: the error ratio of attempted step i.  Writes per attempt
 * t0[i], dt[i], the six stage times as fp32 bits stage_bits[6 i .. 6 i + 5], accept[i]; probe[2]: the fp32 coefficient
 * of x0 + h0 k1 and the probe's model time; *dense_s: the dense-output fraction once an accepted step reached t = 1.
 * Returns 0 (reached t = 1), 1 (ratios ran out first) or the sampler's error codes (-9, -10, -11). */
int32_t mdgen_debug_dopri5_controller(const double* init, const double* ratios, int32_t n_ratios, int32_t max_steps,
                                      float* probe, double* t0, double* dt, uint32_t* stage_bits, int32_t* accept,
                                      float* dense_s, int32_t* n_attempts);

/* Fixed-grid Runge-Kutta sampling on t = linspace(0, 1, n_steps + 1) (fp32): `sample_ode(sampling_method='midpoint' | 'heun3' |
 * 'rk4', num_steps = n_steps + 1)` -> torchdiffeq 0.2.x fixed_grid.py Midpoint, Heun3, RK4 (the 3/8 rule), one step per grid
 * interval (integrators.py:106-113; formulas and rounding: csrc/ode.inc).  method: 1 midpoint (2 evaluations per step), 2 heun3
 * (3), 3 rk4 (4).  Every sample sees the same time grid: a sample's solution does not depend on its batch mates.  Nothing
 * synchronises and nothing is read back; with use_graph != 0 the whole solve is captured / replayed as ONE hipGraph (non-default
 * stream; cached per shape, method, n_steps and pointers, like mdgen_sample_euler).  Both precision modes.
 *   x            (B,T,L,D) fp32, 16-byte aligned: the noise on entry, the state at t = 1 on exit
 *   workspace    mdgen_rk_workspace_bytes: the network workspace for the call's t-shared time rows (2 S, 3 S, 3 S + 1) + 4 velocities
 * The state of a stage is formed inside the launch that embeds it (k_rk_embed: the token-embedding kernel's own body on a state
 * computed in its staging prologue) and never written to memory.
 * Errors: -1 null argument, -2 unknown method or n_steps < 1, -7 alignment / workspace size. */
int32_t mdgen_sample_rk(mdgen_ctx* ctx, const mdgen_shape* shape, int32_t method, int32_t n_steps, float* x, const mdgen_cond* cond,
                        void* workspace, size_t workspace_bytes, int32_t use_graph, void* stream);
int32_t mdgen_rk_workspace_bytes(const mdgen_ctx* ctx, const mdgen_shape* shape, int32_t method, int32_t n_steps, size_t* bytes);

/* Host-only test hook (no GPU): the time rows mdgen_sample_rk prepares for (method, n_steps) as fp32 bits (row_bits, room for
 * cap_rows; *n_rows of them) and the row of every (step, stage): row_of[step * *n_stages + stage]. */
int32_t mdgen_debug_rk_plan(int32_t method, int32_t n_steps, uint32_t* row_bits, int32_t cap_rows, int32_t* n_rows,
                            int32_t* row_of, int32_t* n_stages);
/* Test hook: the sampler's state-forming embedding kernel (k_rk_embed) alone.  State `stage` of a step of `method` with step size
 * dt: 0 is y itself, 1 .. stages - 1 a stage input, `stages` the step's result in the storing form (the launch that opens the next
 * step).  y (B,T,L,D): the step's y0, overwritten by the result in the storing form; k0 .. k3: the velocities of stages 1 .. 4
 * (null where the state does not read one); ipa_out: [B L][384] rows or null; h out: [B T L][384].  Weights and abs_pos_emb: the
 * context's. */
int32_t mdgen_debug_rk_stage(mdgen_ctx* ctx, const mdgen_shape* shape, int32_t method, int32_t stage, float dt, float* y,
                             const float* k0, const float* k1, const float* k2, const float* k3, const float* x_cond,
                             const int64_t* x_cond_mask, const float* ipa_out, float* h, void* stream);

/* SDE sampling: `Sampler.sample_sde(sampling_method='Euler' | 'Heun', diffusion_form=..., diffusion_norm=..., last_step=...,
 * last_step_size=..., num_steps = n_points)` of transport.py:295-406 / integrators.py:5-72 for a velocity model on the Linear or GVP
 * path (formulas and rounding: csrc/sde.inc).  t = linspace(t0, t1, n_points) in fp32 with t0 = sample_eps for SBDM, else 0, and
 * t1 = 1 - last_step_size with a last step of non-zero size, else 1 - sample_eps; n_points - 1 stochastic steps of ONE size
 * t[1] - t[0], then the last step at t1.  Network evaluations: n_points - 1 (Euler-Maruyama) or 2 (n_points - 1) (Heun), one more
 * with a last step. */
typedef struct mdgen_sde_opts {
    int32_t method;           /* 1 Euler-Maruyama, 2 Heun */
    int32_t path;             /* 0 Linear, 1 GVP (as mdgen_path_plan) */
    int32_t diffusion_form;   /* 0 constant, 1 SBDM, 2 sigma, 3 linear, 4 decreasing, 5 increasing-decreasing (path.py:53-60) */
    int32_t last_step;        /* 0 none, 1 Mean, 2 Tweedie, 3 Euler */
    int32_t n_points;         /* the reference's num_steps: grid points */
    double  diffusion_norm;
    double  last_step_size;   /* in [0, 1); ignored without a last step */
    double  sample_eps;       /* in [0, 1); SBDM needs it > 0 */
} mdgen_sde_opts;
/*   x            (B,T,L,D) fp32, 16-byte aligned: the initial state on entry, the sample on exit
 *   noise        n_points - 1 tensors of (B,T,L,D) standard normals, 16-byte aligned; step i's starts at noise + i * noise_step_stride
 *                floats.  The stride is a multiple of 4 and at least B T L D (a state ends on 16 bytes only for some shapes).  The
 *                caller owns the noise: a replay with new noise in the same buffer gives a new sample.
 *   workspace    mdgen_sde_workspace_bytes: the network workspace for the call's time rows + 2 velocities
 * Every state is formed inside the launch that embeds it (k_sde_embed); nothing synchronises and nothing is read back, and with
 * use_graph != 0 the solve is ONE hipGraph (non-default stream; cached per shape, options, stride and pointers).  Both precision modes.
 * Errors, all decided on the host before any device call: -1 null argument; -2 unknown code, n_points < 2, last_step_size or
 * sample_eps outside [0, 1), t0 >= t1, or a coefficient some state reads is not finite (the message names the time and the
 * coefficient: SBDM with sample_eps = 0, Heun on the Linear path reaching t = 1); -7 alignment, stride or workspace size. */
int32_t mdgen_sample_sde(mdgen_ctx* ctx, const mdgen_shape* shape, const mdgen_sde_opts* opts, float* x, const float* noise,
                         int64_t noise_step_stride, const mdgen_cond* cond, void* workspace, size_t workspace_bytes,
                         int32_t use_graph, void* stream);
int32_t mdgen_sde_workspace_bytes(const mdgen_ctx* ctx, const mdgen_shape* shape, const mdgen_sde_opts* opts, size_t* bytes);

/* Host-only test hook (no GPU): the plan of mdgen_sample_sde for `opts` as fp32 bits.  row_bits: the prepared time rows (room for
 * cap_rows; *n_rows of them; a time equal to the row before it shares that row); coef_bits[row][4]: R = alpha / alpha',
 * iV = 1 / (sigma^2 - R sigma' sigma), D, G = sqrtf(2 D); row_of[step * *n_stages + stage]; *last_row: the row of t1, -1 without a
 * last step; scalar_bits[6]: dt, q = sqrtf(dt), 0.5 dt, the last step's size, Tweedie's 1 / alpha and sigma^2 / alpha. */
int32_t mdgen_debug_sde_plan(const mdgen_sde_opts* opts, uint32_t* row_bits, uint32_t* coef_bits, int32_t cap_rows, int32_t* n_rows,
                             int32_t* row_of, int32_t* n_stages, int32_t* last_row, uint32_t* scalar_bits);
/* Host only: mdgen_debug_dispatch_plan's JSON for ONE step of mdgen_sample_sde with `opts` (n_points is taken as 2); "integrator":
 * {"ode_sde_update": 1}. */
int32_t mdgen_debug_sde_dispatch_plan(const mdgen_shape* shape, const mdgen_sde_opts* opts, int32_t tps_condition, int32_t num_layers,
                                      int32_t ncu, int32_t xcd_round_robin, const char* options, char* buf, size_t buflen);
/* Test hook: the state-forming embedding kernel (k_sde_embed) alone on one state of step `step` of the solve `opts` describes.
 * state: 0 x itself, 1 x + noise term (Heun's xh of the first step), 2 the Euler-Maruyama step, 3 Heun's predictor, 4 Heun's result,
 * 5 Heun's result + the noise term of step + 1; the last steps at t1: 6 Tweedie, 7 Euler, 8 Mean.  x (B,T,L,D) is overwritten by
 * every state but 0 and 3; v0, v1: the velocities the state reads, xi: ONE step's noise (null where the state reads none);
 * ipa_out: [B L][384] rows or null; h out: [B T L][384]. */
int32_t mdgen_debug_sde_stage(mdgen_ctx* ctx, const mdgen_shape* shape, const mdgen_sde_opts* opts, int32_t state, int32_t step,
                              float* x, const float* v0, const float* v1, const float* xi, const float* x_cond,
                              const int64_t* x_cond_mask, const float* ipa_out, float* h, void* stream);

/* SDE sampling with the noise generated inside the kernels: mdgen_sample_sde without `noise` and `noise_step_stride`.  No buffer of
 * (n_points - 1) x state floats exists; the kernels that read a step's noise compute it, element by element, with a counter-based
 * generator (csrc/philox.h) from
 *   rng   a device pointer, 8-byte aligned, to four uint64 words {seed, sample_base, block_base, 0}, read INSIDE the kernels: a replay
 *         of the captured graph draws from whatever the words hold then.  Write them on the call's stream before the call.
 * The stream, so that an outside caller can reproduce it.  The deviate of element (b, t, l, d) of the (B,T,L,D) state, stochastic
 * step i (0-based; Heun's noise term of step i is step i's), block k of a driver call (0 for this entry point):
 *   counter  c0 = (t L + l) D + d           the element within its sample (a shape with T L D >= 2^32 is refused, -2)
 *            c1 = sample_base + b           b: the position in the WHOLE call's batch
 *            c2 = i
 *            c3 = block_base + k            every word mod 2^32
 *   key      {seed & 0xffffffff, seed >> 32}
 *   w        = Philox4x32-10(counter; key): multipliers 0xD2511F53 (on c0), 0xCD9E8D57 (on c2), key increments 0x9E3779B9,
 *              0xBB67AE85, ten rounds (Random123's philox4x32; mdgen_debug_philox is the same function on the host)
 *   u1       = ((w0 >> 9) + 0.5) 2^-23      exact in fp32, in (0, 1), at least 2^-24: |xi| <= 5.77
 *   u2       = (w1 >> 8) 2^-24              exact in fp32, in [0, 1)
 *   xi       = sqrtf(-2 logf(u1)) * cosf(6.2831855f * u2)     fp32, every operation rounded once, accurate math functions
 * w2 and w3 are unused: a value depends on its coordinates alone -- not on the batch a sample travels in (give the sample its
 * sample_base), on how the library splits the batch, or on the kernel form a launch size picks.
 * Refusals, plan, workspace (mdgen_sde_workspace_bytes) and launch sequence are mdgen_sample_sde's; the graph is cached per shape,
 * options and pointers (x, rng).  Further errors: -1 rng null; -7 rng alignment. */
int32_t mdgen_sample_sde_rng(mdgen_ctx* ctx, const mdgen_shape* shape, const mdgen_sde_opts* opts, float* x, const uint64_t* rng,
                             const mdgen_cond* cond, void* workspace, size_t workspace_bytes, int32_t use_graph, void* stream);
/* Test hook: xi of ONE stochastic step `step` of block `block` under the words at `rng`, (B,T,L,latent_dim) fp32 to `out` (16-byte
 * aligned), through the device function the sampler's kernels call (the elementwise kernel's generator form on a zero state). */
int32_t mdgen_debug_sde_noise(const mdgen_shape* shape, int32_t latent_dim, const uint64_t* rng, int32_t step, int32_t block,
                              float* out, void* stream);
/* Test hook: mdgen_debug_sde_stage with the generator in xi's place: states 1 and 2 draw the noise of step `step`, state 5 that of
 * step `step` + 1, of block `block`; the other states read no noise and run exactly as mdgen_debug_sde_stage runs them. */
int32_t mdgen_debug_sde_stage_rng(mdgen_ctx* ctx, const mdgen_shape* shape, const mdgen_sde_opts* opts, int32_t state, int32_t step,
                                  int32_t block, float* x, const float* v0, const float* v1, const uint64_t* rng,
                                  const float* x_cond, const int64_t* x_cond_mask, const float* ipa_out, float* h, void* stream);
/* Host only: the number of captured hipGraphs the context holds (at most 8, least recently used evicted): a replay leaves it as it
 * is, a capture adds one. */
int32_t mdgen_debug_graph_count(const mdgen_ctx* ctx, int32_t* count);
/* Host only: out[4] = Philox4x32-10(ctr[4]; key[2]), csrc/philox.h compiled for the host. */
int32_t mdgen_debug_philox(const uint32_t* ctr, const uint32_t* key, uint32_t* out);

/* Residue constant tables (device pointers; data of mdgen/residue_constants.py:1124-1216, 1367-1480), as the two
 * geometry entry points below take them one by one. */
typedef struct mdgen_residue_tables {
    const float*   default_frames;     /* [21][8][4][4] */
    const float*   lit_positions;      /* [21][14][3]   */
    const int64_t* atom14_group;       /* [21][14]      */
    const float*   atom14_mask;        /* [21][14]      */
    const int64_t* atom37_to_atom14;   /* [21][37]      */
    const float*   atom37_mask;        /* [21][37]      */
    const int64_t* chi_atom_indices;   /* [21][4][4]    */
    const float*   chi_angles_mask;    /* [21][4]       */
} mdgen_residue_tables;

/* The driver loop of `sim_inference.py:100-113` (`do`: num_rollouts x `rollout`, :61-98) in ONE call and -- with
 * use_graph -- one hipGraph: for block r < n_blocks
 *     ex      = conditioning frame expanded over T                      (sim_inference.py:72-79)
 *     prep    = prep_batch(ex)  -> x_cond, x_cond_mask                  (wrapper.py:298-342)
 *     samples = Euler(zs[r], model(., start_frames = cond frame))       (wrapper.py:439-447; as mdgen_sample_euler)
 *     atom14[:, r*T:(r+1)*T] = frames_torsions_to_atom14(cond o offsets, torsions)   (wrapper.py:456-478)
 *     cond frame <- atom14_to_frames / atom37_to_torsions of the block's last frame   (sim_inference.py:91-96)
 * with nothing returning to the host between blocks.  Forward-simulation models only (sim_condition).
 *   zs            (n_blocks, B, T, L, D) fp32: noise on entry, each block's samples[-1] on exit
 *   mask          (B, T, L) fp32;  seqres (B, L) int64 (residue types: the model's aatype AND the geometry's)
 *   cond_*        the conditioning frame: rots (B,L,3,3), trans (B,L,3), torsions (B,L,7,2); UPDATED in place to
 *                 the frame that would condition block n_blocks (so a further call continues the trajectory)
 *   x_cond, x_cond_mask   caller-owned scratch (B,T,L,D) fp32 / (B,T,L) int64
 *   atom14        (B, n_blocks*T, L, 14, 3) fp32 out
 * workspace: as mdgen_sample_euler (mdgen_workspace_layout with n_steps, t_shared = 1). */
int32_t mdgen_rollout_euler(mdgen_ctx* ctx, const mdgen_shape* shape, int32_t n_steps, int32_t n_blocks,
                            float* zs, const float* mask,
                            float* cond_rots, float* cond_trans, float* cond_torsions,
                            const int64_t* seqres, float* x_cond, int64_t* x_cond_mask,
                            const mdgen_residue_tables* tables, float* atom14,
                            void* workspace, size_t workspace_bytes, int32_t use_graph, void* stream);

/* Trajectory upsampling: the window loop of `upsampling_inference.py:47-82` around `NewMDGenWrapper.inference`
 * (`wrapper.py:283-365` prep_batch with --cond_interval, `:405-484` inference) in ONE call and -- with use_graph -- one
 * hipGraph.  The B windows of a call are independent samples (windows are the batch axis); per window
 *     x_cond, x_cond_mask, start frames = key frames at t = k * cond_interval, relative to key frame 0   (mdgen_prep_keyframes)
 *     samples = Euler(zs, model(., start_frames = key frame 0))            (wrapper.py:439-447; exactly as mdgen_sample_euler)
 *     atom14  = frames_torsions_to_atom14(key frame 0 o offsets, torsions)  (wrapper.py:456-478)
 * The preparation is part of the graph and ordered before the sub-batch streams fork: a replay with new key frames in the
 * same buffers gives new results.  Forward-simulation models only (sim_condition, latent_dim 21).
 *   zs            (B, T, L, 21) fp32: noise on entry, samples[-1] on exit
 *   mask          (B, T, L) fp32;  seqres (B, L) int64
 *   key_*         K = ceil(T / cond_interval) key frames: rots (B,K,L,3,3), trans (B,K,L,3), torsions (B,K,L,7,2)
 *   x_cond (B,T,L,21) fp32, x_cond_mask (B,T,L) int64, start_rot (B,L,3,3), start_trans (B,L,3)   caller-owned scratch
 *   atom14        (B, T, L, 14, 3) fp32 out
 * workspace: as mdgen_sample_euler (mdgen_workspace_layout with n_steps, t_shared = 1).
 * Returns -1 for a null pointer; -2 for cond_interval < 1, a two-sided (tps_condition) context or a shape the sampler
 * refuses -- all decided before any device call. */
int32_t mdgen_upsample_euler(mdgen_ctx* ctx, const mdgen_shape* shape, int32_t n_steps, int32_t cond_interval,
                             float* zs, const float* mask,
                             const float* key_rots, const float* key_trans, const float* key_torsions,
                             const int64_t* seqres,
                             float* x_cond, int64_t* x_cond_mask, float* start_rot, float* start_trans,
                             const mdgen_residue_tables* tables, float* atom14,
                             void* workspace, size_t workspace_bytes, int32_t use_graph, void* stream);

/* mdgen_rollout_euler with a fixed-grid Runge-Kutta solve per block (method, n_steps: as mdgen_sample_rk) in the Euler loop's
 * place: prep -> solve -> atom14 -> next conditioning frame for n_blocks blocks in ONE call and -- with use_graph -- one hipGraph
 * (cached per method, n_steps, n_blocks, stride, pointers and residue tables).  Arguments as mdgen_rollout_euler, except
 *   zs                block r's noise / samples (B,T,L,D) fp32 start at zs + r * zs_block_stride floats; zs 16-byte aligned
 *   zs_block_stride   in floats; a multiple of 4 and >= B*T*L*D.  The solver's last update reads and writes a block's state 16
 *                     bytes at a time, and B*T*L*D (D = 21) is a multiple of 4 only for some shapes: a (n_blocks,B,T,L,D) tensor
 *                     without padding is accepted exactly when it is (stride = B*T*L*D); otherwise round the stride up.
 *   workspace         mdgen_rk_workspace_bytes(shape, method, n_steps): one block's time rows are prepared again for every block
 *                     (the IPA stack reads the block's conditioning frame)
 * Errors, all decided before any device call: -1 null pointer; -2 unknown method, n_steps < 1, n_blocks < 1, a two-sided
 * (tps_condition) context or a shape the sampler refuses; -7 zs alignment, zs_block_stride, workspace size. */
int32_t mdgen_rollout_rk(mdgen_ctx* ctx, const mdgen_shape* shape, int32_t method, int32_t n_steps, int32_t n_blocks,
                         float* zs, int64_t zs_block_stride, const float* mask,
                         float* cond_rots, float* cond_trans, float* cond_torsions,
                         const int64_t* seqres, float* x_cond, int64_t* x_cond_mask,
                         const mdgen_residue_tables* tables, float* atom14,
                         void* workspace, size_t workspace_bytes, int32_t use_graph, void* stream);

/* mdgen_upsample_euler with a fixed-grid Runge-Kutta solve (method, n_steps: as mdgen_sample_rk): mdgen_prep_keyframes -> solve
 * -> atom14 relative to key frame 0 in ONE call and -- with use_graph -- one hipGraph; a replay with new key frames in the same
 * buffers gives new results.  Arguments as mdgen_upsample_euler; zs (B,T,L,21) must be 16-byte aligned (the only state of the
 * call: no stride); workspace: mdgen_rk_workspace_bytes(shape, method, n_steps).
 * Errors, all decided before any device call: -1 null pointer; -2 unknown method, n_steps < 1, cond_interval < 1, a two-sided
 * context or a shape the sampler refuses; -7 zs alignment, workspace size. */
int32_t mdgen_upsample_rk(mdgen_ctx* ctx, const mdgen_shape* shape, int32_t method, int32_t n_steps, int32_t cond_interval,
                          float* zs, const float* mask,
                          const float* key_rots, const float* key_trans, const float* key_torsions,
                          const int64_t* seqres,
                          float* x_cond, int64_t* x_cond_mask, float* start_rot, float* start_trans,
                          const mdgen_residue_tables* tables, float* atom14,
                          void* workspace, size_t workspace_bytes, int32_t use_graph, void* stream);

/* mdgen_rollout_rk / mdgen_upsample_rk with the SDE solve of mdgen_sample_sde_rng (opts, rng: as there) in the Runge-Kutta solve's
 * place: ONE call and -- with use_graph -- one hipGraph (cached per options, n_blocks / cond_interval, stride and pointers, rng's
 * among them).  No noise is staged: block k of a rollout draws with counter word c3 = block_base + k, an upsampling call with
 * c3 = block_base.  The other arguments, the workspace rule (mdgen_sde_workspace_bytes) and the errors are the Runge-Kutta
 * drivers', with mdgen_sample_sde's option refusals (-2) in the method's and n_steps' place; all decided before any device call. */
int32_t mdgen_rollout_sde(mdgen_ctx* ctx, const mdgen_shape* shape, const mdgen_sde_opts* opts, const uint64_t* rng, int32_t n_blocks,
                          float* zs, int64_t zs_block_stride, const float* mask,
                          float* cond_rots, float* cond_trans, float* cond_torsions,
                          const int64_t* seqres, float* x_cond, int64_t* x_cond_mask,
                          const mdgen_residue_tables* tables, float* atom14,
                          void* workspace, size_t workspace_bytes, int32_t use_graph, void* stream);
int32_t mdgen_upsample_sde(mdgen_ctx* ctx, const mdgen_shape* shape, const mdgen_sde_opts* opts, const uint64_t* rng,
                           int32_t cond_interval, float* zs, const float* mask,
                           const float* key_rots, const float* key_trans, const float* key_torsions,
                           const int64_t* seqres,
                           float* x_cond, int64_t* x_cond_mask, float* start_rot, float* start_trans,
                           const mdgen_residue_tables* tables, float* atom14,
                           void* workspace, size_t workspace_bytes, int32_t use_graph, void* stream);

/* ---- measurement ----------------------------------------------------------------------------
 * Per-kernel-class timing with hipEvents recorded on the launch stream (bench.py's roofline leg).
 * While enabled, launches are bracketed by event pairs and hipGraph capture/replay is bypassed.
 * `mdgen_profile_report` synchronises `stream`, writes a JSON object
 *   {"<class>": {"count": n, "ms": total_ms}, ...}   into buf (NUL-terminated) and resets the log.  Classes of the 64-row panel
 * kernels that exist in two forms carry "@p4" / "@p8" (four / eight waves per panel; option panel_waves), "@p8x3" / "@p8x2" the split
 * forms, the fused attention "@q64" / "@q128" (k_flash_proj / k_flash_proj8), the gate-folded row-owner MLP "mlp@fold" ("+final", "+final+embed": its
 * tails, option mlp_tail).  One entry is
 * not a kernel class: "@context": {"count": split-form MLP launches since the last report, "xcd_round_robin": 0/1 (the placement
 * probe of mdgen_ctx_create: workgroups with equal blockIdx % 8 share an XCD -- where it fails the split MLP form is never picked),
 * "ncu": compute units}. */
int32_t mdgen_profile_enable(mdgen_ctx* ctx, int32_t on);
/* Measurement only: the NEXT trunk MLP launch (the dominant kernel) writes per-wave s_memtime phase stamps into
 * dev_buf ([workgroup*4 + wave][32] uint64; slot meaning: csrc/k_gemm.hip `stamp`).  One-shot; pass NULL to cancel.
 * Only meaningful with profiling enabled or use_graph == 0 (a captured graph would replay the pointer).
 * Which kernel is traced: the row-owner kernel (k_mlp_rows) where the launch takes it, else the FOUR-wave panel kernel k_mlp<3> --
 * also for launches that would otherwise take the eight-wave k_mlp8 (at most one workgroup per CU), which carries no stamps: a
 * trace of such a launch measures k_mlp<3>, not the product's kernel for that size. */
int32_t mdgen_profile_phase_trace(mdgen_ctx* ctx, uint64_t* dev_buf, int64_t capacity_words);
int32_t mdgen_profile_report(mdgen_ctx* ctx, void* stream, char* buf, size_t buflen);
/* Host only (no device, no context): which kernel classes a call of this shape launches and how often -- the library's own
 * orchestration code (the code path of latent_model.py:212-260 / transport.py:408-451's replacements above) run in a plan mode
 * that skips every HIP call; a call the entry point refuses (trace_h with a batch of several launch views) is refused here too.  mode 0: mdgen_sample_euler as the product runs it (sub-batch streams); 1: mdgen_denoiser_forward;
 * 2: mdgen_sample_euler as it runs under mdgen_profile_enable (one stream); 3: mdgen_denoiser_forward with trace_h; 4: one attempted
 * step of mdgen_sample_dopri5; 5 / 6 / 7: one step of mdgen_sample_rk with method 1 / 2 / 3 (modes 4 .. 7: n_steps ignored; they add
 * "integrator": {class: launches}).  options: "name=value,..." with mdgen_ctx_set_option's
 * names (bf16 path only).  ncu / xcd_round_robin: the two device facts mdgen_ctx_create would have probed (see "@context" of
 * mdgen_profile_report).  Writes {"streams": n, "prepare": {"<class>": launches, ...} (the step-invariant part: adaLN table, IPA stack, fold pack),
 * "views": [{"B": samples of the sub-batch view, "classes": {...}}, ...]} with the class names of mdgen_profile_report.  tests/test_dispatch_cpu.py sweeps shapes with it and fails when a combination of
 * kernel forms has no oracle-backed GPU test registered. */
int32_t mdgen_debug_dispatch_plan(const mdgen_shape* shape, int32_t n_steps, int32_t mode, int32_t tps_condition,
                                  int32_t num_layers, int32_t ncu, int32_t xcd_round_robin, const char* options,
                                  char* buf, size_t buflen);

/* Host-only (no GPU): how a call of `shape` is cut into contiguous sub-batch launch views.  One launch addresses
 * the residual stream with 32-bit byte offsets (token * 1536), i.e. at most 2 796 202 token rows; larger batches
 * run as several views (at least `streams` of them).  Fails with -2 if a single sample (T*L tokens) exceeds the
 * limit -- `mdgen_workspace_layout`, `mdgen_denoiser_forward` and `mdgen_sample_euler` reject such shapes too. */
int32_t mdgen_debug_view_plan(const mdgen_shape* shape, int32_t streams, int32_t* n_views,
                              int32_t* max_batch_per_view);

/* Host-only (no GPU): the weight-row / bias permutations behind the attention fragment layout
 * (DESIGN.md "fragment layout"), each int32[384], for layout tests:
 *   map_qk[w*96+rho], map_vflash[w*96+col], map_vsmall[w*96+rho] = source feature of a packed weight row;
 *   perm_qk[((w*2+h)*4+hd)*12+e], perm_vsmall[...] = source feature of lane-ordered bias slot. */
int32_t mdgen_debug_layout_maps(int32_t* map_qk, int32_t* map_vflash, int32_t* map_vsmall,
                                int32_t* perm_qk, int32_t* perm_vsmall);

/* Host-only (no GPU): the weight-fragment stream of the row-owner MLP kernel (csrc/k_rows.hip), for layout tests.
 * out[f] = mat << 16 | row_tile << 8 | k_step for fragment f (2304 of them); mat 0 = fc1 (layers.py:77-84 `fc1`), 1 = fc2.
 * Returns the number of entries, or a negative status. */
int32_t mdgen_debug_mlp_stream_table(int32_t* out, int32_t capacity);

/* Test hooks (GPU): the training step's linear layer and weight gradient on raw device buffers, launched in the form that the
 * form functions of mdgen_train_forward_backward give for the shape -- precision 32: fp32 products (k32_linear / k32_dw); 16: bf16-rounded
 * operands with fp32 accumulation (128 x 384-tile streamed kernels for >= 1024 / 4096 rows, one-wave tiles for a few
 * hundred rows, the general kernels otherwise).  All pointers are fp32 device memory.
 *   linear: c[n][m] (row stride ldc) = a[n][k] (lda) . w[m][k]^T (ldw) + bias[m] (bias may be NULL);
 *           scratch: >= m * k * 2 bytes (the bf16 weight stream of the streamed kernel), may be NULL (then the weight is
 *           read as fp32 rows);
 *   dw:     dw[m][k] += dy[n][m]^T (ldy) . x[n][k] (ldx), db[m] += column sums of dy (db may be NULL);
 *           part: scratch of part_floats floats for the split partial sums (>= 2 m (k + 1)).
 * Reference: torch.nn.functional.linear and its autograd (mdgen/model/layers.py Mlp, mha.py projections). */
int32_t mdgen_debug_train_linear(int32_t precision, const float* a, int32_t lda, const float* w, int32_t ldw, const float* bias,
                                 int64_t n, int32_t m, int32_t k, float* c, int32_t ldc, void* scratch, void* stream);
int32_t mdgen_debug_train_dw(int32_t precision, const float* dy, int32_t ldy, const float* x, int32_t ldx, int64_t n, int32_t m,
                             int32_t k, float* dw, float* db, float* part, int64_t part_floats, void* stream);

/* Test hook (GPU): the training step's attention of one axis, forward + backward, on raw device buffers (fp32):
 *   qkv[ntok][1152]: q (already scaled and rotated) | k (rotated) | v of 16 heads x 24 (mha.py:258-268); sequence `s`, position
 *   `i` is token (s / inner) * outer_stride + (s % inner) * inner_stride + i * pos_stride; mask[ntok]: 0 = padded key;
 *   bias_k, bias_v[384]: the learned bias key / value (rotated at position len by the kernels); inv_freq[12].
 * Forward: out[ntok][384], lse[ntok][16].  Backward from dout[ntok][384]: dqkv[ntok][1152] = (d q, d k taken back through RoPE,
 * d q also through the q scale; d v), dbias[nseq][768] = per-sequence (d bias_k | d bias_v); stats[ntok][16][2] scratch.
 * precision 32: k32_attn* + k32_rope_bwd; 16: k16_attn* (bf16 operands on the MFMA, inverse RoPE in the store stage) as the training
 * step dispatches them; 160: the chunked k16 kernels for every length (against the sequence-resident ones); 161 (len 129 .. 256
 * only): q, k of `qkv` are given UNROTATED (q scaled) and the sequence-resident kernels rotate them while they convert them,
 * as the training step runs them (it launches no RoPE pass for such an axis). */
int32_t mdgen_debug_train_attention(int32_t precision, const float* qkv, int64_t ntok, int32_t nseq, int32_t len, int32_t inner,
                                    int32_t outer_stride, int32_t inner_stride, int32_t pos_stride, const float* mask,
                                    const float* bias_k, const float* bias_v, const float* inv_freq, const float* dout,
                                    float* out, float* lse, float* dqkv, float* dbias, float* stats, void* stream);

/* Test hook (GPU): the invariant point attention core alone (ipa.py:126-254 between the input projections and linear_out),
 * forward + backward on raw fp32 device buffers, launched as the training step launches it.  M = ngroups * len token rows;
 * group g uses the frames and the mask of sample g % nbatch (the sampler runs ngroups = steps * nbatch, the training step
 * ngroups = nbatch).
 *   proj[M][672]: linear_q (128: head * 32 + c) | linear_kv (256: head * 64 + [k 32 | v 32]) | linear_q_points (96: x | y | z
 *   blocks of head * 8 + point) | linear_kv_points (192: x | y | z blocks of head * 16 + [k points 8 | v points 8]);
 *   rot[nbatch][len][3][3], trans[nbatch][len][3], mask[nbatch][len] (0 = padded residue), head_w[4] (before the softplus);
 *   part: scratch of part_floats floats for the slices of the key loop (forward [slices][M][4][58], backward
 *   [slices][M][676]); NULL: one slice.  Fewer floats than the wanted slices need: fewer slices.
 * Forward: feat[M][256] = o (128) | o_pt.x | o_pt.y | o_pt.z | |o_pt| (32 each), lse[M][4] = log-sum-exp of the logits;
 *   feat_bf16 (nullable): [M][256] bf16, the same rows from a second launch as the bf16 sampler path makes it (one slice).
 * Backward (dfeat[M][256] nullable: forward only; needs ngroups == nbatch): dproj[M][672], dhead_w[4] += d head_w (accumulated
 *   into, as a parameter gradient); bwd_scratch: caller buffer of >= 200 * M floats (dhw[M][4] | the per-query record
 *   [M][4][49]), NOT carved from `part`.
 * *fwd_slices, *bwd_slices: the slices launched (bwd 0 without dfeat).  mdgen_debug_ipa_slices (host only, no HIP call): the same two
 * counts for a shape and scratch size, and *fwd_tiled = 1 where the forward runs the LDS-tiled kernel, 0: one thread per
 * (query, head).  tests/test_ipa_attention_{cpu,gpu}.py. */
int32_t mdgen_debug_ipa_attention(const float* proj, const float* rot, const float* trans, const float* mask, const float* head_w,
                                  int32_t ngroups, int32_t nbatch, int32_t len, float* part, int64_t part_floats,
                                  const float* dfeat, float* feat, void* feat_bf16, float* lse, float* dproj, float* dhead_w,
                                  float* bwd_scratch, int32_t* fwd_slices, int32_t* bwd_slices, void* stream);
int32_t mdgen_debug_ipa_slices(int32_t ngroups, int32_t len, int32_t has_part, int64_t part_floats, int32_t* fwd_slices,
                               int32_t* bwd_slices, int32_t* fwd_tiled);

/* Host-only (no GPU): the plans of one mdgen_train_forward_backward call -- the kernel form of every launch whose kernel depends on
 * train_precision (16 | 32), the row count, the attention axis or the 16-byte alignment of the weights (weight_misalign_bytes: every
 * weight that many bytes off a 16-byte boundary, as a bound parameter buffer may put them; 0 = aligned).  Writes JSON: {"rows",
 * "ipa_block", "ipa_attn", "ipa_mlp" (B L rows), "trunk_attn_l", "trunk_attn_t", "trunk_mlp" (B T L rows), "final"}; a form is named by
 * its kernel, a dX product as [route ("streamed" | "turned" | "wtrans"), form], a weight gradient as [form, the bias gradient rides
 * along], "rows" of a sub-layer: its GEMM-only tensors are stored as "bf16" or "fp32" rows.  tests/test_train_plan_cpu.py. */
int32_t mdgen_debug_train_plan(const mdgen_shape* shape, int32_t tps_condition, int32_t num_layers, int32_t train_precision,
                               int32_t weight_misalign_bytes, char* buf, size_t buflen);

/* ---- SE(3) frame algebra, fp32 (mdgen/rigid_utils.py) --------------------------------------
 * n = number of frames; rot: [n][3][3]; trans/pts: [n][3]; quat: [n][4] (w,x,y,z). */
int32_t mdgen_rigid_compose(int64_t n, const float* r1, const float* t1, const float* r2, const float* t2,
                            float* r_out, float* t_out, void* stream);            /* :1031-1045 */
int32_t mdgen_rigid_invert(int64_t n, const float* r, const float* t, float* r_out, float* t_out,
                           void* stream);                                          /* :1075-1085 */
int32_t mdgen_rigid_apply(int64_t n, int64_t pts_per_frame, const float* r, const float* t,
                          const float* pts, float* out, int32_t inverse, void* stream); /* :1047-1073 */
int32_t mdgen_quat_to_rot(int64_t n, const float* quat, int32_t normalize, float* rot, void* stream); /* :168-188, :324 */
int32_t mdgen_rot_to_quat(int64_t n, const float* rot, float* quat, void* stream); /* :191-210 (sign: w >= 0) */
/* Rigid.from_3_points(p_neg_x, origin, p_xy, eps = 1e-8) (:1175-1218): Gram-Schmidt frame, R columns e0, e1, e2,
 * t = origin.  Points (n, 3); rot (n, 3, 3); trans (n, 3). */
int32_t mdgen_from_3_points(int64_t n, const float* p_neg_x, const float* origin, const float* p_xy, float* rot,
                            float* trans, void* stream);

/* ---- sampler pre/post-processing (mdgen/wrapper.py) ----------------------------------------
 * `NewMDGenWrapper.prep_batch` latents (wrapper.py:298-327, 339-342, 362) incl. `utils.get_offsets`
 * (utils.py:7-14): offsets = rigid[b,0]^-1 o rigid[b,t] as [quat(w>=0) | trans], TPS appends the
 * offsets w.r.t. frame T-1; latents = [offsets | torsions(14)]; cond frames = 0 (and T-1 for TPS), plus every
 * cond_interval-th frame when cond_interval > 0 (`--cond_interval`, wrapper.py:343-344: the upsampling models; 0 = none).
 * rots (B,T,L,3,3), trans (B,T,L,3), torsions (B,T,L,7,2) -> latents, x_cond (B,T,L,D),
 * x_cond_mask int64 (B,T,L). */
int32_t mdgen_prep_latents(const mdgen_shape* shape, int32_t tps, int32_t cond_interval, const float* rots, const float* trans,
                           const float* torsions, float* latents, float* x_cond, int64_t* x_cond_mask,
                           void* stream);

/* Key-frame conditioning of the upsampling models: what `split_batch` (upsampling_inference.py:47-66) + `prep_batch` with
 * --cond_interval (wrapper.py:304-309, 327, 343-344, 362) give, from the key frames alone.  With K = ceil(T / cond_interval)
 * key frames key_rots (B,K,L,3,3), key_trans (B,K,L,3), key_torsions (B,K,L,7,2), key frame k standing at t = k * cond_interval:
 *   x_cond (B,T,L,21)      row t = k * cond_interval: [quat(w>=0) of R_0^T R_k | R_0^T (t_k - t_0) | torsions(14)]; other rows 0
 *   x_cond_mask (B,T,L)    int64, (t % cond_interval == 0)
 *   start_rot (B,L,3,3), start_trans (B,L,3)   contiguous copies of key frame 0
 * The offsets are the arithmetic of mdgen_prep_latents (one device function).  cond_interval >= T: K = 1, the plain
 * forward-simulation conditioning; T need not be a multiple of cond_interval.  -1: null pointer; -2: cond_interval < 1 or a
 * dimension < 1. */
int32_t mdgen_prep_keyframes(const mdgen_shape* shape, int32_t cond_interval,
                             const float* key_rots, const float* key_trans, const float* key_torsions,
                             float* x_cond, int64_t* x_cond_mask, float* start_rot, float* start_trans, void* stream);

/* `NewMDGenWrapper.inference` tail (wrapper.py:456-478) + `geometry.frames_torsions_to_atom14`
 * (geometry.py:61-79, 236-334): samples (B,T,L,D) + first-frame rigids (rot0 (B,L,3,3), trans0
 * (B,L,3)) + seqres int64 (B,L) -> atom14 (B,T,L,14,3).  Residue constant tables (device):
 * default_frames [21][8][4][4], lit_positions [21][14][3], atom14_group int64 [21][14],
 * atom14_mask [21][14] (mdgen/residue_constants.py:1124-1216). */
int32_t mdgen_samples_to_atom14(const mdgen_shape* shape, int32_t latent_dim, int32_t tps,
                                const float* samples, const float* rot0, const float* trans0,
                                const int64_t* seqres, const float* default_frames,
                                const float* lit_positions, const int64_t* atom14_group,
                                const float* atom14_mask, float* atom14, void* stream);

/* Rollout glue (sim_inference.py:91-96): last frame atom14 (B,L,14,3) -> next block's conditioning
 * frame: `geometry.atom14_to_frames` (geometry.py:218-231) + `atom14_to_atom37` + `atom37_to_torsions`
 * (geometry.py:9-27, 82-202).  Tables: atom37_to_atom14 int64 [21][37], atom37_mask [21][37],
 * chi_atom_indices int64 [21][4][4], chi_angles_mask [21][4].  Outputs rots (B,L,3,3),
 * trans (B,L,3), torsions (B,L,7,2), torsion_mask (B,L,7). */
int32_t mdgen_atom14_to_cond(int32_t B, int32_t L, const float* atom14, const int64_t* seqres,
                             const int64_t* atom37_to_atom14, const float* atom37_mask,
                             const int64_t* chi_atom_indices, const float* chi_angles_mask,
                             float* rots, float* trans, float* torsions, float* torsion_mask,
                             void* stream);

/* The text `mdgen.utils.atom14_to_pdb` writes (utils.py:58-102 -> protein.py:321-443) for M frames of one sequence, formatted
 * on the device: per frame `MODEL <model_base + m>` (unpadded), one ATOM record per present atom in (residue, atom37) order, a
 * TER record, `ENDMDL`; byte for byte what mdgen_amd/pdb.py frames_to_pdb_string gives for frames model_base .. model_base + M - 1
 * of a trajectory.  An atom37 slot is present when (|x| + |y|) + |z| > 1e-7f (fp32, that order) of its gathered, masked position
 * (utils.py:77).  A coordinate prints as Python's f"{x:>8.3f}": n = rint((double) x * 1000) (exact product, ties to even), then
 * |n| / 1000, '.', |n| % 1000 in three digits, '-' when signbit(x); it fits its field when x is finite and
 * -999999 <= n <= 9999999.  The kernels know no names:
 *   atom14        (M, L, 14, 3) fp32;  aatype int64 (L), in [0, 20];  atom37_to_atom14 int64 [21][37], atom37_mask [21][37]
 *   templates     uint8 [L][37][81]: the 80-column ATOM record of (residue, atom37 slot) + '\n' with the serial (columns 7-11) and
 *                 the coordinates (columns 31-54) blank;  ter_template uint8 [81]: the TER record of the last residue, serial blank
 *                 (mdgen_amd/pdb.py record_templates)
 *   offsets       int64 [M + 1] out: frame m's text is text[offsets[m] .. offsets[m + 1]); no alignment of either is assumed
 *   text          uint8 [text_capacity] out; M * (27 + 81 * (A + 1) + 7) bytes always suffice, A = atoms atom37_mask gives the sequence
 *   status        int64 [2] out: [0] coordinates that do not fit their field (+ one per frame whose TER serial passes 99999, + one
 *                 per table entry out of range); [1] the bytes needed, offsets[M]
 * Three launches on `stream` (count, one-workgroup scan, format; csrc/k_pdb.hip), nothing synchronises.  The format pass writes
 * NOTHING when status[0] > 0 or offsets[M] > text_capacity: the caller reads status back once and, for a trajectory with a field
 * that overflows, formats on the host, where such fields come out as the reference writes them.
 * -1: null pointer; -2: M < 1, L < 1, L > 9999 (the residue number has four columns), model_base < 0, text_capacity < 0. */
int32_t mdgen_pdb_format(int64_t M, int32_t L, int64_t model_base, const float* atom14, const int64_t* aatype,
                         const int64_t* atom37_to_atom14, const float* atom37_mask,
                         const uint8_t* templates, const uint8_t* ter_template,
                         int64_t* offsets /* M + 1 */, uint8_t* text, int64_t text_capacity,
                         int64_t* status /* [2]: records that do not fit, bytes needed */, void* stream);

/* Analysis of a sampled trajectory on the device (csrc/k_analysis.hip; mdgen_amd/analysis.py): the parts of the reference's
 * scripts/analyze_peptide_sim.py that need no third-party estimator.  All three run on `stream` and synchronise nothing.  The index
 * tables `quad` and `pairs` are HOST arrays: they are checked here and travel as kernel arguments; every other pointer is device
 * memory.  Every refusal is decided before any device call.  NF = 0 succeeds and writes nothing.
 *
 * mdgen_traj_dihedrals: angles[f][j] = the IUPAC dihedral of atoms quad[j][0 .. 3] of frame f, in fp32:
 *   b1 = p1 - p0, b2 = p2 - p1, b3 = p3 - p2, c1 = b2 x b3, c2 = b1 x b2, atan2(|b2| (b1 . c1), c1 . c2); 0 when both arguments
 *   are zero (coincident or collinear atoms), never NaN for finite input.
 *   atom14 (F, L, 14, 3) fp32;  quad int32 [NF][4], indices into a frame's L * 14 atoms;  angles (F, NF) fp32 out.
 * -1: null pointer; -2: F < 1, L < 1, NF < 0 or > 32768, a quadruple index outside 0 .. L * 14 - 1. */
int32_t mdgen_traj_dihedrals(int64_t F, int32_t L, int32_t NF, const float* atom14, const int32_t* quad /* host */,
                             float* angles, void* stream);

/* mdgen_traj_histograms: NF one-dimensional histograms of the columns of angles (F, NF) and P two-dimensional ones of the column
 * pairs (pairs[p][0], pairs[p][1]), in one launch per 64 pairs.  edges1 fp64 [bins1 + 1] and edges2 fp64 [bins2 + 1] are ascending
 * bin edges (np.linspace(-np.pi, np.pi, bins + 1) for the reference's histograms).  A value x, widened to fp64, goes to bin
 * searchsorted(edges, x, 'right') - 1, a value equal to the last edge to the last bin, a value outside [edges[0], edges[bins]] (or
 * NaN) nowhere: it is counted in dropped.  float32(pi) > np.pi is such a value, as it is for np.histogram.  A 2-D sample is dropped
 * when either coordinate is.
 *   hist1 int64 [NF][bins1], hist2 int64 [P][bins2][bins2] (first index: the pair's first feature), dropped int64 [NF + P]
 *   (features, then pairs): all three are zeroed and filled.  Counts gather per workgroup in LDS (integer atomics), then in global memory.
 * -1: null pointer; -2: F < 1, bins1 < 1 or > 16384, bins2 < 1 or > 128, NF or P < 0 or > 32768, a pair index outside 0 .. NF - 1. */
int32_t mdgen_traj_histograms(int64_t F, int32_t NF, const float* angles, int32_t bins1, const double* edges1, int32_t P,
                              const int32_t* pairs /* host */, int32_t bins2, const double* edges2, int64_t* hist1,
                              int64_t* hist2, int64_t* dropped, void* stream);

/* mdgen_traj_acov: for every column f of angles (n, NF) and lag k = 0 .. K
 *   acov[f][k] = (sum_{t = 0}^{n - k - 1} sin a_t sin a_{t + k} + cos a_t cos a_{t + k}) / (n - k)
 * -- statsmodels' acovf(sin) + acovf(cos) with demean=False, adjusted=True -- and mean_sin[f], mean_cos[f], the means over t.
 * sin and cos are evaluated in fp64 and rounded to fp32 once; products and sums of 256 samples are fp32, everything beyond is fp64
 * in a fixed order, without floating-point atomics: two calls give the same bits.
 *   acov fp64 [NF][K + 1], mean_sin, mean_cos fp64 [NF] out;  workspace: mdgen_traj_acov_workspace_bytes(n, NF, K), 16-byte aligned.
 * -1: null pointer; -2: n < 1, K < 0, K > n - 1, NF < 0 or > 32768, NF * (K + 1) beyond one launch; -3: workspace too small. */
int32_t mdgen_traj_acov_workspace_bytes(int64_t n, int32_t NF, int64_t K, size_t* bytes);
int32_t mdgen_traj_acov(int64_t n, int32_t NF, int64_t K, const float* angles, double* acov, double* mean_sin, double* mean_cos,
                        void* workspace, size_t workspace_bytes, void* stream);

/* tICA of a trajectory's torsion angles (csrc/k_tica.hip; mdgen_amd/analysis.py tica_fit / tica_transform): the parts of the
 * reference's `pyemma.coordinates.tica(lag, kinetic_map=True)` (scripts/analyze_peptide_sim.py:104-150) that scale with the
 * trajectory length.  The four entries follow the conventions above: they run on `stream` and synchronise nothing, every refusal is
 * decided before any device call (-1 null pointer, -2 bad shape, -3 workspace too small), NF = 0 / NS = 0 / P = 0 succeeds and
 * writes nothing, no floating-point atomics, two calls give the same bits.
 *
 * Features.  For angles (n, NF) fp32 in `torsion_features`' order, frame t has x_t in R^D, D = 2 NF, x[2j] = cos a_j,
 * x[2j + 1] = sin a_j -- pyemma's cossin=True interleaving as the maintainers recall it, unchecked; tICA's results do not depend on
 * the order beyond rounding.  cos and sin are evaluated in fp64 and rounded to fp32 once.
 * Moments at lag tau.  With m = n - tau, X = x[0 .. m), Y = x[tau .. n):  sx = sum X, sy = sum Y, cxx = X'X, cyy = Y'Y, cxy = X'Y,
 * raw (un-centred).
 * Estimator (host, NumPy fp64: analysis.tica_solve; pyemma's defaults reversible, var_cutoff 0.95, epsilon 1e-6):
 *   mu = (sx + sy) / 2m,  C0 = (cxx + cyy) / 2m - mu mu',  Ctau = (cxy + cxy') / 2m - mu mu';
 *   C0 = Q S Q', the eigenvalues s > epsilon kept, rank r their number, L = Q_r S_r^(-1/2);
 *   L' Ctau L = R diag(lambda) R', lambda descending;  W = (L R) diag(lambda), the kinetic map; in every column of W the entry of
 *   largest magnitude is positive (the first such entry on ties);  dim = the smallest d with
 *   sum_{i<d} lambda_i^2 / sum lambda_i^2 >= 0.95;  transform: (x_t - mu) W[:, :d].
 *
 * mdgen_traj_lagged_moments: sx, sy fp64 [D], cxx, cyy, cxy fp64 [D][D] of angles (n, NF) at `lag`, 0 <= lag <= n - 1.
 *   1 <= NF <= 64: tetrapeptides have at most 22 torsions; ATLAS-size proteins are not this tool's subject and are refused.
 *   Products and sums of 64 frames are fp32, everything beyond is fp64; per-workgroup partial sums go to the workspace and are added
 *   in a fixed order.  At lag 0 the three matrices are equal to the bit, and so are sx and sy.
 *   workspace: mdgen_traj_lagged_moments_workspace_bytes(n, NF, lag), 16-byte aligned.
 * -2: n < 1, lag < 0 or > n - 1, NF < 0 or > 64. */
int32_t mdgen_traj_lagged_moments_workspace_bytes(int64_t n, int32_t NF, int64_t lag, size_t* bytes);
int32_t mdgen_traj_lagged_moments(int64_t n, int32_t NF, int64_t lag, const float* angles, double* sx, double* sy, double* cxx,
                                  double* cyy, double* cxy, void* workspace, size_t workspace_bytes, void* stream);

/* mdgen_traj_project: out[t][c] = sum_j (x_t[j] - mean[j]) W[j][c] for the features x_t of angles (n, NF): the subtraction first,
 * then fp32 FMAs with j ascending.  mean fp32 [D], W fp32 [D][d] row-major, out (n, d) fp32.
 * -2: n < 1, NF < 0 or > 64, d < 1 or > D. */
int32_t mdgen_traj_project(int64_t n, int32_t NF, int32_t d, const float* angles, const float* mean, const float* W, float* out,
                           void* stream);

/* mdgen_traj_series_acov: for every column s of x (n, NS) fp32 and lag k = 0 .. K
 *   acov[s][k] = sum_{t = 0}^{n - k - 1} x_t x_{t + k} / (n - k)
 * -- statsmodels' acovf(demean=False, adjusted=True) -- and mean[s], the mean over t.  mdgen_traj_acov's kernel body on one row,
 * the same refusals and launch limit, the same precision rule (fp32 over at most 256 samples, fp64 beyond, fixed order) -- here
 * fp32 over 8 samples: a series with an offset has products of one sign, whose fp32 rounding errors add up instead of cancelling.
 *   acov fp64 [NS][K + 1], mean fp64 [NS] out;  workspace: mdgen_traj_series_acov_workspace_bytes(n, NS, K), 16-byte aligned. */
int32_t mdgen_traj_series_acov_workspace_bytes(int64_t n, int32_t NS, int64_t K, size_t* bytes);
int32_t mdgen_traj_series_acov(int64_t n, int32_t NS, int64_t K, const float* x, double* acov, double* mean, void* workspace,
                               size_t workspace_bytes, void* stream);

/* mdgen_traj_histograms_xy: P two-dimensional histograms of the column pairs (pairs[p][0], pairs[p][1]) of values (F, NC) fp32, with
 * an edge table per pair and per axis: edges_x, edges_y fp64 [P][bins + 1], ascending (mdgen_traj_histograms has one table for both
 * axes of every pair).  The same binning rule: searchsorted(edges, x, 'right') - 1 of the value widened to fp64, the last edge in the
 * last bin, a value outside (or NaN) in no bin; a sample with such a coordinate is counted in dropped.
 *   hist2 int64 [P][bins][bins] (first index: the pair's first column), dropped int64 [P]: both are zeroed and filled.
 * -2: F < 1, NC < 1 or > 32768, P < 0 or > 32768, bins < 1 or > 128, a pair index outside 0 .. NC - 1. */
int32_t mdgen_traj_histograms_xy(int64_t F, int32_t NC, const float* values, int32_t P, const int32_t* pairs /* host */,
                                 int32_t bins, const double* edges_x, const double* edges_y, int64_t* hist2, int64_t* dropped,
                                 void* stream);

/* k-means and the Markov-state-model counts of a trajectory (csrc/k_msm.hip; mdgen_amd/analysis.py kmeans_fit / count_matrix): the
 * parts of the reference's k-means -> MSM -> PCCA+ chain (mdgen/analysis.py get_kmeans / get_msm) that scale with the trajectory
 * length.  The k x k estimators are the host's (mdgen_amd/msm.py, NumPy fp64).  The conventions above: the entries run on `stream`
 * and synchronise nothing, read nothing back, every refusal is decided before any device call and leaves the outputs untouched
 * (-1 null pointer, -2 bad shape, -3 workspace too small), no floating-point atomics, two calls give the same bits.
 *
 * x (n, d) fp32 row-major, 1 <= d <= 128;  centers fp32 [k][d], 1 <= k <= 256;  n <= 2^40.
 * Distance: dist2(x_t, c) = sum_j (x_tj - c_j)^2 in the direct form -- the fp32 difference, then fp32 FMAs over j ascending.
 *
 * mdgen_traj_kmeans_assign: assign[t] = the index of the centre of smallest dist2, ties to the lowest index; dist2[t] that distance
 *   (dist2 may be NULL).  This is also the discretisation of a trajectory by fitted centres.
 *
 * mdgen_traj_kmeans_step: one Lloyd iteration.  state int32 [2] = {done flag, steps taken} and cost fp64 [2] = {this step's, the
 *   previous step's} live on the device; a call that finds the done flag set changes nothing.  Otherwise: assign as above;
 *   cost = sum_t dist2_t, the fp32 values added in fp64; sums fp64 [k][d] = per-cluster sums of the fp32 rows, counts int64 [k];
 *   centers[c] = fp32(sums[c] / counts[c]), an empty cluster keeps its centre; cost[1] <- cost[0] <- cost; steps + 1; the done flag
 *   is set when steps >= 1 before the call and |cost[1] - cost[0]| <= tol * cost[0].  Sums and cost: per-workgroup partial sums
 *   added in a fixed order.  Zero state and cost before the first step.
 *   workspace: mdgen_traj_kmeans_step_workspace_bytes(n, d, k), 16-byte aligned.  -2 also: tol < 0 or NaN.
 *
 * mdgen_traj_kmeans_pp: rounds r0 .. r1 - 1 of k-means++ with the caller's uniforms u (HOST fp64 [k], each in [0, 1)).
 *   Round 0: chosen[0] = floor(u[0] n), mind2[t] = +inf.  Round r >= 1: mind2[t] = min(mind2[t], dist2(x_t, x_chosen[r - 1]));
 *   total = sum_t mind2[t] in fp64 (256 points in a tree, the 256-point sums in order); chosen[r] = the smallest i with
 *   sum_{t <= i} mind2[t] > u[r] total, or floor(u[r] n) when total == 0.  chosen int64 [k] and mind2 fp32 [n] stay on the device
 *   between rounds and calls: 0 <= r0 <= r1 <= k.  After round k - 1 the rows x[chosen] are the initial centres.
 *   workspace: mdgen_traj_kmeans_pp_workspace_bytes(n, d, k), 16-byte aligned.
 *
 * mdgen_traj_count_matrix: counts[i][j] = #{t < n - lag : dtraj[t] = i, dtraj[t + lag] = j}, the sliding-window count; a pair with
 *   either state outside [0, k) is counted in dropped[0].  counts int64 [k][k] and dropped are zeroed and filled (integer atomics,
 *   per workgroup in LDS where k <= 110: exact and order-independent).  lag >= n gives zeros.  -2: n < 1, lag < 0, k < 1 or > 256. */
int32_t mdgen_traj_kmeans_assign(int64_t n, int32_t d, int32_t k, const float* x, const float* centers, int32_t* assign,
                                 float* dist2 /* or NULL */, void* stream);
int32_t mdgen_traj_kmeans_step_workspace_bytes(int64_t n, int32_t d, int32_t k, size_t* bytes);
int32_t mdgen_traj_kmeans_step(int64_t n, int32_t d, int32_t k, const float* x, float* centers /* in/out */, int32_t* assign,
                               double* sums, int64_t* counts, double* cost /* [2] in/out */, int32_t* state /* [2] in/out */,
                               double tol, void* workspace, size_t workspace_bytes, void* stream);
int32_t mdgen_traj_kmeans_pp_workspace_bytes(int64_t n, int32_t d, int32_t k, size_t* bytes);
int32_t mdgen_traj_kmeans_pp(int64_t n, int32_t d, int32_t k, const float* x, const double* u /* host */, int32_t r0, int32_t r1,
                             int64_t* chosen /* [k] in/out */, float* mind2 /* [n] in/out */, void* workspace,
                             size_t workspace_bytes, void* stream);
int32_t mdgen_traj_count_matrix(int64_t n, int64_t lag, int32_t k, const int32_t* dtraj, int64_t* counts, int64_t* dropped,
                                void* stream);

/* Transition paths of a Markov-state model (csrc/k_tps.hip; mdgen_amd/analysis.py tp_sample): the reference's `sample_tp`
 * (mdgen/analysis.py:61-76) and, with a scoring set, `get_tp_likelihood(...).prod(-1)` (:79-95) of every sampled path.  The
 * conventions of the mdgen_traj_* entries: it runs on `stream`, synchronises nothing and reads nothing back; every refusal is
 * decided before any device call and leaves the outputs untouched; no atomics, two calls give the same bits.
 *
 * mdgen_tp_sample: n_samples paths of length N of the k-state chain Ta, pinned at paths[s][0] = start and paths[s][N - 1] = end.
 *   Ta fp64 [k][k] row-stochastic;  Ba fp64 [N][k] the bridge table, Ba[m][i] = (Ta^m)[i][end] (msm.bridge_table: Ba[0] = e_end,
 *   Ba[m] = Ta Ba[m - 1]);  both device memory.  One thread per path.
 *   The draw, for t = 1 .. N - 2 from state a = paths[s][t - 1]:
 *     w_j = Ta[a][j] * Ba[N - t - 1][j]        each product rounded to fp64 before it is added (no contraction into an FMA)
 *     c_j = c_{j-1} + w_j                      j ascending, c_{-1} = 0
 *     u   = ((x0 >> 5) 2^26 + (x1 >> 6)) 2^-53 53 bits, exact, in [0, 1); x = Philox4x32-10(counter; key) (mdgen_sample_sde_rng's
 *                                              generator) with
 *       counter  c0 = sample & 0xffffffff, c1 = sample >> 32, c2 = t, c3 = stream_id;   sample = sample_base + s mod 2^64
 *       key      {seed & 0xffffffff, seed >> 32}                                        x2, x3 are unused
 *     paths[s][t] = the smallest j with c_j > u * c_{k-1} (one rounded fp64 product); if rounding leaves none, the largest j with
 *                   w_j > 0.
 *   A path depends on (seed, stream_id, sample) alone: not on n_samples, on the launch shape or on the other paths of the call.
 *   c_{k-1} = 0 (or NaN) cannot occur when Ba[N - 1][start] > 0; where it does, positions t .. N - 1 of that path are -1 and its
 *   prob is 0.
 *   Scoring set (kb >= 1; kb = 0: none, and Tb, Bb, phi, prob are ignored): Tb fp64 [kb][kb] and Bb fp64 [N][kb], its bridge table
 *   to phi[end], device memory; phi int32 [k], a HOST array, checked here: state i of Ta is state phi[i] of Tb.
 *     prob[s] = prod_{t = 1}^{N - 1} Tb[pa][pb] * Bb[N - t - 1][pb] / Bb[N - t][pa],  pa = phi[paths[s][t - 1]], pb = phi[paths[s][t]],
 *   evaluated left to right, a NaN factor (0 / 0) counting as 0 and t ascending: `get_tp_likelihood(phi(paths), Tb).prod(-1)`.
 *   paths int32 [n_samples][N] out;  prob fp64 [n_samples] out (scoring set only).
 * -1: null pointer (Ta, Ba, paths; with kb >= 1 also Tb, Bb, phi, prob); -2: n_samples < 1 or > 2^40, N < 2 or > 4096, k < 1 or
 * > 64, kb < 0 or > 64, start or end outside 0 .. k - 1, an entry of phi outside 0 .. kb - 1. */
int32_t mdgen_tp_sample(int64_t n_samples, int32_t N, int32_t k, const double* Ta, const double* Ba, int32_t start, int32_t end,
                        uint64_t seed, uint32_t stream_id, uint64_t sample_base, int32_t kb, const double* Tb /* or NULL */,
                        const double* Bb /* or NULL */, const int32_t* phi /* host, or NULL */, int32_t* paths,
                        double* prob /* or NULL */, void* stream);

/* Cartesian ensemble statistics of protein trajectories (csrc/k_ensemble.hip; mdgen_amd/ensemble.py): superposition, per-atom mean
 * and covariance (RMSF), all-pairs RMSD, contact counts and Shrake-Rupley surface counts -- the parts of an AlphaFlow-style ensemble
 * evaluation that scale with frames x atoms or frames x frames.  Every quantity is defined here by its equation; agreement with AlphaFlow's script and with
 * mdtraj is unverified.  Units: Angstrom.  The conventions of the mdgen_traj_* entries: coordinates x (F, A, 3) fp32 contiguous
 * device memory (the sampler's (T, L, 14, 3) is A = 14 L; atom subsets are made by the caller, the kernels are dense); the entries run
 * on `stream`, every refusal is decided before any launch and leaves the outputs untouched (-1 null pointer, -2 bad shape or value,
 * -3 workspace too small), no floating-point atomics, every fp sum has a fixed order, two calls give the same bits.  Entries with a
 * workspace synchronise nothing and read nothing back; mdgen_ens_superpose alone copies w to the host, see there.
 *
 * mdgen_ens_superpose: every frame rotated and translated onto `ref` (A, 3) fp32 under the weights w fp32 [A].  3 <= A <= 16384,
 *   1 <= F <= 2^40.  w is device memory and is CHECKED ON THE HOST: the entry copies it back on `stream` and synchronises that stream
 *   once before its launch (it cannot be captured into a graph); -2 unless every w is finite and >= 0 and at least 3 are > 0.
 *   Per frame, in fp64 from the fp32 values:
 *     cx = sum_a w_a x_a / sum_a w_a,  cr likewise of ref;   H = sum_a w_a (x_a - cx)(ref_a - cr)^T
 *     R  = the proper rotation (det +1) minimising sum_a w_a |R (x_a - cx) - (ref_a - cr)|^2: the unit quaternion that is the
 *          eigenvector of the largest eigenvalue of Horn's 4 x 4 matrix N(H), by cyclic Jacobi in fp64 (csrc/ensemble.h).  No 3 x 3
 *          SVD, no reflection case: a mirror image of ref still gets a proper rotation.
 *     rmsd = sqrt(sum_a w_a |R (x_a - cx) - (ref_a - cr)|^2 / sum_a w_a), summed directly in fp64 (not from the eigenvalue).
 *   out_a = R (x_a - cx) + cr in fp32 -- cx, cr and R rounded to fp32, one subtraction, three FMAs ending on cr -- for every atom
 *   with exists[a] != 0 (uint8 [A]; NULL: every atom); the other atoms are copied unchanged (atom14 padding slots stay zero).
 *   out (F, A, 3) may be x.  rot fp64 [F][9] row-major and rmsd fp64 [F] may each be NULL.
 *   Up to A = 256 a wave owns a frame (four frames a workgroup), beyond a workgroup does.
 *
 * mdgen_ens_moments: mean fp64 [A][3] and cov fp64 [A][3][3] of every atom over the frames (divided by F), accumulated in fp64 about
 *   frame 0: u_t = x_t - x_0, mean = x_0 + mean(u), cov = mean(u u^T) - mean(u) mean(u)^T.  F = 1 gives cov = 0 exactly.
 *   1 <= A <= 16384, 1 <= F <= 2^40.  workspace: mdgen_ens_moments_workspace_bytes(F, A) (partial sums, 18 MB at the most),
 *   16-byte aligned.  RMSF_a = sqrt(trace cov_a).
 *
 * mdgen_ens_pairwise_d2: d2[i][j] = sum over atoms and axes of (xa_i - xb_j)^2 for every frame i of xa (Fa, A, 3) and j of xb
 *   (Fb, A, 3), in the direct form -- the fp32 difference, then one chain of fp32 FMAs over the 3 A coordinates ascending (the
 *   distance of mdgen_traj_kmeans_assign).  sums fp64 [2]: sums[0] = sum_ij sqrt((double)d2 / A), sums[1] = sum_ij (double)d2 / A,
 *   over all Fa Fb pairs (xa == xb: the zero diagonal included).  d2 fp32 [Fa][Fb] may be NULL: then nothing of that size exists
 *   and the sums have the same bits.  1 <= Fa, Fb <= 2^20 - 1, 1 <= A <= 16384.
 *   workspace: mdgen_ens_pairwise_d2_workspace_bytes(Fa, Fb, A) (1 MB at the most), 16-byte aligned.
 *   Tiles of 128 x 64 frames, 24 coordinates staged in LDS at a time, 8 x 4 pairs a thread.
 *
 * mdgen_ens_contact_counts: counts[i][j] = #{t : d2_t(i, j) < cutoff2} over ca (F, N, 3), with d2 = fmaf(dz, dz, fmaf(dy, dy, dx dx))
 *   of the three fp32 differences.  counts int32 [N][N] is zeroed and filled (integer atomics: exact in any order); it is
 *   symmetric, and its diagonal is F when cutoff2 > 0.  1 <= N <= 4096, 1 <= F <= 2^31 - 1; -2 also: cutoff2 negative, NaN or
 *   infinite.
 *
 * mdgen_ens_sasa_counts: Shrake-Rupley.  counts[f][i] = the number of the P sphere points of atom i of frame f that no other atom
 *   buries; the solvent-accessible area of the atom is 4 pi R_i^2 counts / P.  counts int32 [F][A] device memory, every entry
 *   written.  radius fp32 [A] and points fp32 [P][3] are HOST arrays (as phi of mdgen_tp_sample): the entry checks them and stages
 *   them on `stream` into the workspace, with R and R2 below; pageable memory, which the runtime has read when the entry returns.
 *   1 <= A <= 16384, 1 <= P <= 4096, 1 <= F <= 2^31 - 1; -2 also: probe or a radius NaN or outside 0 .. 16, a point that is not
 *   finite or whose norm (in fp64) is further than 1e-3 from 1.  workspace: mdgen_ens_sasa_workspace_bytes(A, P), 16-byte aligned.
 *     existence   an atom with radius[a] == 0 does not exist: its count is 0 and it buries nothing (atom14 padding slots hold zeros
 *                 and are no atoms at the origin).  Otherwise R_a = radius[a] + probe (one fp32 add), R2_a = R_a R_a (one fp32
 *                 multiply, rounded).
 *     point k of atom i   q = (fmaf(R_i, u_kx, c_ix), fmaf(R_i, u_ky, c_iy), fmaf(R_i, u_kz, c_iz))
 *     buried      iff some existing j != i has d2 < R2_j, d2 = fmaf(dz, dz, fmaf(dy, dy, dx dx)) of the three fp32 differences
 *                 q - c_j: the distance of mdgen_ens_contact_counts.
 *     counts[f][i] = #{k : point k of atom i is not buried}.  Integers, independent of any order: two calls give the same bits.
 *   A wave owns an atom: it compacts the atoms within reach (|c_i - c_j| < R_i + R_j, kept with slack: the counts are those of the
 *   definition above) into a list of 512 in LDS, and tests every point against all atoms when more are within reach. */
int32_t mdgen_ens_superpose(int64_t F, int32_t A, const float* x, const float* ref, const float* w, const uint8_t* exists /* or NULL */,
                            float* out, double* rot /* or NULL */, double* rmsd /* or NULL */, void* stream);
int32_t mdgen_ens_moments_workspace_bytes(int64_t F, int32_t A, size_t* bytes);
int32_t mdgen_ens_moments(int64_t F, int32_t A, const float* x, double* mean, double* cov, void* workspace, size_t workspace_bytes,
                          void* stream);
int32_t mdgen_ens_pairwise_d2_workspace_bytes(int64_t Fa, int64_t Fb, int32_t A, size_t* bytes);
int32_t mdgen_ens_pairwise_d2(int64_t Fa, int64_t Fb, int32_t A, const float* xa, const float* xb, float* d2 /* or NULL */,
                              double* sums, void* workspace, size_t workspace_bytes, void* stream);
int32_t mdgen_ens_contact_counts(int64_t F, int32_t N, const float* ca, float cutoff2, int32_t* counts, void* stream);
int32_t mdgen_ens_sasa_workspace_bytes(int32_t A, int32_t P, size_t* bytes);
int32_t mdgen_ens_sasa_counts(int64_t F, int32_t A, int32_t P, const float* x, const float* radius /* host */,
                              const float* points /* host */, float probe, int32_t* counts, void* workspace, size_t workspace_bytes,
                              void* stream);

/* Flow-matching training target (transport.py:138-189 `training_losses`, velocity model; path.py:113-135 `plan`
 * with GVPCPlan :177-187 or the linear ICPlan): per sample b with time t[b],
 *   xt = alpha x1 + sigma x0,  ut = alpha' x1 + sigma' x0;   GVP: alpha = sin(pi t/2), sigma = cos(pi t/2);
 *   Linear: alpha = t, sigma = 1 - t.   x0/x1/xt/ut: (B, per_sample) fp32; path_type 0 = Linear, 1 = GVP. */
int32_t mdgen_path_plan(int64_t B, int64_t per_sample, int32_t path_type, const float* t, const float* x0,
                        const float* x1, float* xt, float* ut, void* stream);

/* Masked mean squared error per sample (transport.py:13-17 `mean_flat`, :184):
 *   loss[b] = sum((pred - target)^2 * mask) / sum(mask)  over the per_sample elements of sample b. */
int32_t mdgen_masked_mse(int64_t B, int64_t per_sample, const float* pred, const float* target, const float* mask,
                         float* loss, void* stream);

/* ---- optimiser side of the training step ----------------------------------------------
 * Parameters, gradients and the two Adam moments each live in ONE flat fp32 device buffer of n elements.
 *
 * mdgen_grad_sumsq: out[0] = sum((grads[i] * scale)^2), deterministic (fixed block slices, fp64 accumulation); `scratch`: 1024 floats, 8-byte aligned.
 *   Feeds gradient clipping (train.py:56 gradient_clip_val -> torch.nn.utils.clip_grad_norm_, 2-norm) without a
 *   host round trip: pass `out` as `sumsq` below.
 * mdgen_adam_step: torch.optim.Adam / AdamW (wrapper.py:167-172; betas (0.9, 0.999), eps 1e-8 are torch's defaults;
 *   adamw != 0: decoupled weight decay).  g = grads * grad_scale * min(1, max_norm / (sqrt(sumsq) + 1e-6)) when sumsq is
 *   non-NULL (clip_grad_norm_), else grads * grad_scale (grad_scale = 1 / world_size averages a summed all-reduce).
 *   `step` is the 1-based update count (bias correction 1 - beta^step).
 * mdgen_ema_update: ema -= (ema - params) * (1 - decay)   (ema.py:41-58). */
int32_t mdgen_grad_sumsq(int64_t n, const float* grads, float scale, float* scratch, int32_t scratch_floats,
                         float* out, void* stream);
int32_t mdgen_adam_step(int64_t n, float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                        int32_t step, float lr, float beta1, float beta2, float eps, float weight_decay,
                        int32_t adamw, float grad_scale, const float* sumsq, float max_norm, void* stream);
int32_t mdgen_ema_update(int64_t n, float* ema, const float* params, float decay, void* stream);

/* ---- training step: forward + backward -------------------------------------------------
 * `NewMDGenWrapper.general_step` (wrapper.py:367-403) after the flow-matching plan: pred = model(xt, t, ...);
 * loss[b] = mean_flat((pred - target)^2, loss_mask) (transport.py:13-17,184); total = mean_b loss[b]; and
 * d total / d theta for every trainable tensor, ADDED into `grads` (flat fp32) at grad_offsets[i] (in floats) for the
 * context's i-th state_dict key (mdgen_ctx_weight_name; -1 = do not compute / frozen).  Runs the fp32-operand form of
 * the network (option keep_fp32_weights must have been set before the weights were handed over), with a tape in
 * `tape` (mdgen_train_workspace_bytes; 256-byte aligned); `workspace` as for mdgen_denoiser_forward (n_steps 1,
 * t_shared 0).  Forward-simulation models (end_rot, end_trans, rel7 of `cond` are not read) and the two-sided TPS model (end frames
 * required; its IPA stack runs twice on shared weights, latent_model.py:193-205).  xt, target, loss_mask, pred:
 * (B,T,L,D); t, loss: (B). */
int32_t mdgen_train_workspace_bytes(const mdgen_ctx* ctx, const mdgen_shape* shape, size_t* bytes);
/* Gradient milestones, for overlapping the DDP all-reduce with the backward pass (Lightning DDP's bucketed hooks,
 * train.py:46-77): the backward pass completes parameter groups in the order
 *   0: emb_to_latent.* | 1 .. nl: layers.{nl-1 .. 0}.* | nl+1: latent_to_emb, cond_to_emb, mask_to_emb |
 *   nl+2 .. 2nl+1: ipa_layers.{nl-1 .. 0}.* | 2nl+2: everything else (aatype_to_emb, latent_to_emb_f/_r, t_embedder)
 * and records the caller's hipEvent_t events[k] (NULL = skip) on the training stream when group k's gradients are
 * final.  The list stays in force until replaced (n = 0 clears it); the events remain the caller's. */
/* Point the fp32 weights the training kernels read at `flat + offsets[i]` (i = index of mdgen_ctx_weight_name; -1: keep the
 * context's own copy, e.g. frozen buffers): the optimiser then updates what the next step reads, with no hand-back.
 * Needs keep_fp32_weights = 1 and loaded weights.  The caller keeps `flat` alive as long as the context trains. */
int32_t mdgen_train_bind_params(mdgen_ctx* ctx, float* flat, const int64_t* offsets);
int32_t mdgen_train_num_milestones(const mdgen_ctx* ctx);
int32_t mdgen_train_set_milestone_events(mdgen_ctx* ctx, void* const* events, int32_t n);
int32_t mdgen_train_forward_backward(mdgen_ctx* ctx, const mdgen_shape* shape, const float* xt, const float* t,
                                     const mdgen_cond* cond, const float* target, const float* loss_mask, float* loss, float* pred,
                                     float* grads, const int64_t* grad_offsets, void* workspace, size_t workspace_bytes,
                                     void* tape, size_t tape_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDGEN_AMD_H */
