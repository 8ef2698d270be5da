// -*- c++ -*-  The fused drivers (included by api.hip after ode.inc and sde.inc): the Euler, the Runge-Kutta and the SDE entry point
// of a driver share its refusals and its captured body -- the glue kernels around a solve -- and differ in the solve: euler_body on
// the entry point's time grid, or RkCall::solve (ode.inc) / SdeCall::solve (sde.inc, with generated noise), which prepare their own
// time rows on the stream.

// the conditioning a driver fills from the caller's buffers: start frames alone (forward-simulation models)
static mdgen_cond driver_cond(const float* mask, const float* rot, const float* trans, const float* x_cond, const int64_t* x_cond_mask,
                              const int64_t* seqres) {
    return {mask, rot, trans, nullptr, nullptr, nullptr, x_cond, x_cond_mask, seqres};
}
// the refusals of both drivers that need no context: that conditioning, and the residue tables a driver reads
static int driver_check_pointers(const mdgen_cond& cd, const mdgen_residue_tables* tb, bool next_frame) {
    if (int e = check_cond(&cd)) return e;
    if (!tb->default_frames || !tb->lit_positions || !tb->atom14_group || !tb->atom14_mask) return fail(-1, "null residue table");
    if (next_frame && (!tb->atom37_to_atom14 || !tb->atom37_mask || !tb->chi_atom_indices || !tb->chi_angles_mask))
        return fail(-1, "null residue table");   // (atom14 -> the next block's conditioning frame reads these four)
    return 0;
}
// ... and the ones about its count (n_blocks, cond_interval) and the model
static int driver_check_model(const mdgen_ctx* c, int count, const char* count_name, const char* driver) {
    if (count < 1) return fail(-2, "%s must be >= 1", count_name);
    if (c && c->d.tps_condition) return fail(-2, "%s is defined for forward-simulation models (sim_condition)", driver);
    return 0;
}

// Multi-block rollout (sim_inference.py:61-98, 110-113) as ONE call / ONE hipGraph: per block
//   conditioning frame (B, L) expanded over T -> prep_batch latents (wrapper.py:298-342)
//   -> the solve from the block's noise (wrapper.py:439-447) -> atom14 (wrapper.py:456-478)
//   -> last frame -> next block's conditioning frame (sim_inference.py:91-96),
// nothing returning to the host in between; whatever the solve prepares, it prepares per block: the IPA stack reads the block's
// conditioning frame.  `r`: the made run with the call's conditioning bound; `solve(x)` solves one block in place; block b is
// zs + b * stride floats; `key`: the entry point's tag and scalars; `forks`: n_streams(r) where the solve forks onto the sub-batch
// streams (it closes the key), 0 where it does not.
static int rollout_too_long(const mdgen_shape* sh, int n_blocks) {   // (the shape has been judged: make_run, or mdgen_rollout_rk itself)
    if ((long)n_blocks * sh->T > 2000000000L / ((long)sh->L * 42)) return fail(-2, "trajectory too long for one call");
    return 0;
}
template <class Solve>
static int rollout_run(const Run& r, int use_graph, GraphKey key, int forks, int n_blocks, float* zs, long stride, float* cond_rots,
                       float* cond_trans, float* cond_torsions, const int64_t* seqres, float* x_cond, int64_t* x_cond_mask,
                       const mdgen_residue_tables& t, float* atom14, Solve solve) {
    float* tmask_scratch = (float*)(r.ws + r.lay.rel7);   // (B, L, 7) fp32: fits the (unused, non-TPS) 2 x (B, L, 7) slot
    auto body = [&]() -> int {
        for (int b = 0; b < n_blocks; ++b) {
            float* x = zs + (long)b * stride;
            launch_prep_latents(r.B, r.T, r.L, 0, 1, 0, cond_rots, cond_trans, cond_torsions, nullptr, x_cond, x_cond_mask, r.s);
            LAUNCHCHK();
            if (int e = solve(x)) return e;
            launch_samples_to_atom14(r.B, r.T, r.L, r.D, 0, x, cond_rots, cond_trans, seqres, t.default_frames,
                                     t.lit_positions, t.atom14_group, t.atom14_mask, atom14, n_blocks * r.T, b * r.T, r.s);
            LAUNCHCHK();
            // last frame of this block (frame b*T + T-1 of every trajectory) -> conditioning frame of the next
            const float* last = atom14 + ((long)(b + 1) * r.T - 1) * r.L * 42;
            launch_atom14_to_cond(r.B, r.L, last, (long)n_blocks * r.T * r.L * 42, seqres, t.atom37_to_atom14, t.atom37_mask,
                                  t.chi_atom_indices, t.chi_angles_mask, cond_rots, cond_trans, cond_torsions,
                                  tmask_scratch, r.s);
            LAUNCHCHK();
        }
        return 0;
    };
    key.ptr(zs).ptr(cond_torsions).ptr(atom14).add_struct(t);
    if (forks) key.add(forks);
    return run_or_replay(r, use_graph, key, body);
}

extern "C" int32_t mdgen_rollout_euler(mdgen_ctx* c, const mdgen_shape* sh, int32_t S, int32_t n_blocks, float* zs,
                                       const float* mask, float* cond_rots, float* cond_trans, float* cond_torsions,
                                       const int64_t* seqres, float* x_cond, int64_t* x_cond_mask,
                                       const mdgen_residue_tables* tb, float* atom14, void* ws, size_t ws_bytes,
                                       int32_t use_graph, void* stream) {
    if (!zs || !cond_torsions || !tb || !atom14) return fail(-1, "null tensor argument");
    const mdgen_cond cd = driver_cond(mask, cond_rots, cond_trans, x_cond, x_cond_mask, seqres);
    if (int e = driver_check_pointers(cd, tb, true)) return e;
    if (int e = driver_check_model(c, n_blocks, "n_blocks", "the block rollout")) return e;
    Run r{};
    if (int e = make_run(&r, c, sh, S, 1, f32_path(c), ws, ws_bytes, stream)) return e;
    if (int e = rollout_too_long(sh, n_blocks)) return e;
    bind_cond(r, cd);
    std::vector<float> tg;
    linspace01(S + 1, &tg);
    const long blk = (long)sh->B * sh->T * sh->L * r.D;   // the blocks lie contiguous
    GraphKey key = graph_key(1, r, cd);
    key.add(S).add(n_blocks);
    return rollout_run(r, use_graph, key, n_streams(r), n_blocks, zs, blk, cond_rots, cond_trans, cond_torsions, seqres, x_cond,
                       x_cond_mask, *tb, atom14, [&](float* x) { return euler_body(r, tg, x); });
}

// k_rk_update reads and writes the state 16 bytes at a time, and a block of B T L D floats (D = 21) ends on 16 bytes only for some
// shapes (T = 250, L = 251: B T L D % 4 == 2), so the caller chooses the stride: a multiple of 4 floats, at least one block.  Every
// refusal comes before rk_open, the first to touch the device.
extern "C" int32_t mdgen_rollout_rk(mdgen_ctx* c, const mdgen_shape* sh, int32_t method, int32_t S, int32_t n_blocks, float* zs,
                                    int64_t stride, const float* mask, float* cond_rots, float* cond_trans, float* cond_torsions,
                                    const int64_t* seqres, float* x_cond, int64_t* x_cond_mask, const mdgen_residue_tables* tb,
                                    float* atom14, void* ws, size_t ws_bytes, int32_t use_graph, void* stream) {
    if (!sh || !zs || !cond_torsions || !tb || !atom14 || !ws) return fail(-1, "null argument");
    const mdgen_cond cd = driver_cond(mask, cond_rots, cond_trans, x_cond, x_cond_mask, seqres);
    if (int e = driver_check_pointers(cd, tb, true)) return e;
    if (int e = rk_check(method, S)) return e;
    if (int e = driver_check_model(c, n_blocks, "n_blocks", "the block rollout")) return e;
    if (sh->B < 1 || sh->T < 1 || sh->L < 1) return fail(-2, "B, T, L must be >= 1");
    if (int e = rollout_too_long(sh, n_blocks)) return e;
    const long blk = (long)sh->B * sh->T * sh->L * (c ? c->D : 21);   // (forward-simulation latents: 21 floats a token)
    if (((uintptr_t)zs & 15) != 0) return fail(-7, "zs must be 16-byte aligned");
    if (stride % 4 != 0) return fail(-7, "zs_block_stride must be a multiple of 4 floats (got %lld)", (long long)stride);
    if (stride < blk) return fail(-7, "zs_block_stride %lld is below one block of %ld floats", (long long)stride, blk);
    RkCall q;
    if (int e = rk_open(&q, c, sh, method, S, zs, cd, ws, ws_bytes, stream)) return e;
    GraphKey key = graph_key(4, q.r, cd);
    key.add(method).add(S).add(n_blocks).add((uint64_t)stride);
    return rollout_run(q.r, use_graph, key, 0, n_blocks, zs, (long)stride, cond_rots, cond_trans, cond_torsions, seqres, x_cond,
                       x_cond_mask, *tb, atom14, [&](float* x) { return q.solve(S, x); });
}

// mdgen_rollout_rk with the SDE solve (sde.inc) per block, its noise generated in the kernels: block b draws with counter word
// block_base + b, so the call needs no noise at all.  The refusals are mdgen_rollout_rk's with sde_plan's in rk_check's place.
extern "C" int32_t mdgen_rollout_sde(mdgen_ctx* c, const mdgen_shape* sh, const mdgen_sde_opts* o, const uint64_t* rng, int32_t n_blocks,
                                     float* zs, int64_t stride, const float* mask, float* cond_rots, float* cond_trans,
                                     float* cond_torsions, const int64_t* seqres, float* x_cond, int64_t* x_cond_mask,
                                     const mdgen_residue_tables* tb, float* atom14, void* ws, size_t ws_bytes, int32_t use_graph,
                                     void* stream) {
    if (!sh || !o || !rng || !zs || !cond_torsions || !tb || !atom14 || !ws) return fail(-1, "null argument");
    const mdgen_cond cd = driver_cond(mask, cond_rots, cond_trans, x_cond, x_cond_mask, seqres);
    if (int e = driver_check_pointers(cd, tb, true)) return e;
    if (int e = sde_check(o)) return e;
    if (int e = driver_check_model(c, n_blocks, "n_blocks", "the block rollout")) return e;
    if (sh->B < 1 || sh->T < 1 || sh->L < 1) return fail(-2, "B, T, L must be >= 1");
    if (int e = rollout_too_long(sh, n_blocks)) return e;
    const long blk = (long)sh->B * sh->T * sh->L * (c ? c->D : 21);
    if (stride % 4 != 0) return fail(-7, "zs_block_stride must be a multiple of 4 floats (got %lld)", (long long)stride);
    if (stride < blk) return fail(-7, "zs_block_stride %lld is below one block of %ld floats", (long long)stride, blk);
    SdeCall q;
    if (int e = sde_open(&q, c, sh, o, zs, SdeNoise{nullptr, 0, rng, 0}, cd, ws, ws_bytes, stream)) return e;
    GraphKey key = graph_key(8, q.r, cd);
    key.add_struct(q.key).add(n_blocks).add((uint64_t)stride).ptr(rng);
    return rollout_run(q.r, use_graph, key, 0, n_blocks, zs, (long)stride, cond_rots, cond_trans, cond_torsions, seqres, x_cond,
                       x_cond_mask, *tb, atom14,
                       [&](float* x) { return q.solve(x, SdeNoise{nullptr, 0, rng, (int)((x - zs) / stride)}); });
}

// Trajectory upsampling (upsampling_inference.py:47-82 around wrapper.py:283-365, 405-484) as ONE call / ONE hipGraph:
//   key frames (B, K, L) -> x_cond, x_cond_mask, start frames (k_prep_keyframes; no (B, T, L) window of zeros on the way)
//   -> the solve, exactly as mdgen_sample_euler / mdgen_sample_rk run it -> atom14 relative to key frame 0.
// The preparation kernel is enqueued on the call's stream ahead of the solve (euler_body records its fork event after it): every
// sub-batch stream sees the conditioning of THIS call, also when the graph is replayed on new key frames in the same buffers.
// `r`, `solve`, `key` and `forks` as rollout_run takes them.
template <class Solve>
static int upsample_run(const Run& r, int use_graph, GraphKey key, int forks, int cond_interval, float* zs, const float* key_rots,
                        const float* key_trans, const float* key_torsions, const int64_t* seqres, float* x_cond, int64_t* x_cond_mask,
                        float* start_rot, float* start_trans, const mdgen_residue_tables& t, float* atom14, Solve solve) {
    auto body = [&]() -> int {
        launch_prep_keyframes(r.B, r.T, r.L, cond_interval, key_rots, key_trans, key_torsions, x_cond, x_cond_mask, start_rot,
                              start_trans, r.s);
        LAUNCHCHK();
        if (int e = solve(zs)) return e;
        launch_samples_to_atom14(r.B, r.T, r.L, r.D, 0, zs, start_rot, start_trans, seqres, t.default_frames, t.lit_positions,
                                 t.atom14_group, t.atom14_mask, atom14, r.T, 0, r.s);
        LAUNCHCHK();
        return 0;
    };
    key.ptr(zs).ptr(key_rots).ptr(key_trans).ptr(key_torsions).ptr(atom14).add_struct(t);
    if (forks) key.add(forks);
    return run_or_replay(r, use_graph, key, body);
}

extern "C" int32_t mdgen_upsample_euler(mdgen_ctx* c, const mdgen_shape* sh, int32_t S, int32_t cond_interval, float* zs,
                                        const float* mask, const float* key_rots, const float* key_trans,
                                        const float* key_torsions, const int64_t* seqres, float* x_cond, int64_t* x_cond_mask,
                                        float* start_rot, float* start_trans, const mdgen_residue_tables* tb, float* atom14,
                                        void* ws, size_t ws_bytes, int32_t use_graph, void* stream) {
    if (!zs || !key_rots || !key_trans || !key_torsions || !tb || !atom14) return fail(-1, "null tensor argument");
    const mdgen_cond cd = driver_cond(mask, start_rot, start_trans, x_cond, x_cond_mask, seqres);
    if (int e = driver_check_pointers(cd, tb, false)) return e;
    if (int e = driver_check_model(c, cond_interval, "cond_interval", "upsampling")) return e;
    Run r{};
    if (int e = make_run(&r, c, sh, S, 1, f32_path(c), ws, ws_bytes, stream)) return e;
    bind_cond(r, cd);
    std::vector<float> tg;
    linspace01(S + 1, &tg);
    GraphKey key = graph_key(2, r, cd);
    key.add(S).add(cond_interval);
    return upsample_run(r, use_graph, key, n_streams(r), cond_interval, zs, key_rots, key_trans, key_torsions, seqres, x_cond,
                        x_cond_mask, start_rot, start_trans, *tb, atom14, [&](float* x) { return euler_body(r, tg, x); });
}

extern "C" int32_t mdgen_upsample_rk(mdgen_ctx* c, const mdgen_shape* sh, int32_t method, int32_t S, int32_t cond_interval, float* zs,
                                     const float* mask, const float* key_rots, const float* key_trans, const float* key_torsions,
                                     const int64_t* seqres, float* x_cond, int64_t* x_cond_mask, float* start_rot,
                                     float* start_trans, const mdgen_residue_tables* tb, float* atom14, void* ws, size_t ws_bytes,
                                     int32_t use_graph, void* stream) {
    if (!sh || !zs || !key_rots || !key_trans || !key_torsions || !tb || !atom14 || !ws) return fail(-1, "null argument");
    const mdgen_cond cd = driver_cond(mask, start_rot, start_trans, x_cond, x_cond_mask, seqres);
    if (int e = driver_check_pointers(cd, tb, false)) return e;
    if (int e = rk_check(method, S)) return e;
    if (int e = driver_check_model(c, cond_interval, "cond_interval", "upsampling")) return e;
    if (((uintptr_t)zs & 15) != 0) return fail(-7, "zs must be 16-byte aligned");
    RkCall q;
    if (int e = rk_open(&q, c, sh, method, S, zs, cd, ws, ws_bytes, stream)) return e;
    GraphKey key = graph_key(5, q.r, cd);
    key.add(method).add(S).add(cond_interval);
    return upsample_run(q.r, use_graph, key, 0, cond_interval, zs, key_rots, key_trans, key_torsions, seqres, x_cond, x_cond_mask,
                        start_rot, start_trans, *tb, atom14, [&](float* x) { return q.solve(S, x); });
}

// mdgen_upsample_rk with the SDE solve, its noise generated in the kernels (block counter word: block_base)
extern "C" int32_t mdgen_upsample_sde(mdgen_ctx* c, const mdgen_shape* sh, const mdgen_sde_opts* o, const uint64_t* rng,
                                      int32_t cond_interval, float* zs, const float* mask, const float* key_rots, const float* key_trans,
                                      const float* key_torsions, const int64_t* seqres, float* x_cond, int64_t* x_cond_mask,
                                      float* start_rot, float* start_trans, const mdgen_residue_tables* tb, float* atom14, void* ws,
                                      size_t ws_bytes, int32_t use_graph, void* stream) {
    if (!sh || !o || !rng || !zs || !key_rots || !key_trans || !key_torsions || !tb || !atom14 || !ws) return fail(-1, "null argument");
    const mdgen_cond cd = driver_cond(mask, start_rot, start_trans, x_cond, x_cond_mask, seqres);
    if (int e = driver_check_pointers(cd, tb, false)) return e;
    if (int e = sde_check(o)) return e;
    if (int e = driver_check_model(c, cond_interval, "cond_interval", "upsampling")) return e;
    const SdeNoise nz{nullptr, 0, rng, 0};
    SdeCall q;
    if (int e = sde_open(&q, c, sh, o, zs, nz, cd, ws, ws_bytes, stream)) return e;
    GraphKey key = graph_key(9, q.r, cd);
    key.add_struct(q.key).add(cond_interval).ptr(rng);
    return upsample_run(q.r, use_graph, key, 0, cond_interval, zs, key_rots, key_trans, key_torsions, seqres, x_cond, x_cond_mask,
                        start_rot, start_trans, *tb, atom14, [&](float* x) { return q.solve(x, nz); });
}
