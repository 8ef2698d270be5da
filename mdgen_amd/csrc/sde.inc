// sde.inc -- included by api.hip after ode.inc: the SDE sampler (mdgen_sample_sde, mdgen_sample_sde_rng)
// ---------------------------------------------------------------------------------------------
// Euler-Maruyama and Heun on t = linspace(t0, t1, n_points), then a last step
// ---------------------------------------------------------------------------------------------
// The reference's Sampler.sample_sde (transport.py:295-406) integrates dx = F dt + sqrt(2 D) dW with the `sde` class of
// integrators.py:5-72 and finishes with one deterministic step at t1.  With velocity prediction the drift is the velocity plus
// diffusion times score (transport.py:306-308, path.py:69-83); restated with R = alpha / alpha', iV = 1 / (sigma^2 - R sigma' sigma),
// D = compute_diffusion(form, norm) (path.py:53-60) and G = sqrt(2 D) at evaluation time tau:
//   F(v, x; tau) = v + D * (((R * v) - x) * iV)
// Interval (check_interval(..., sde=True), transport.py:95-124): t0 = sample_eps for SBDM, else 0; t1 = 1 - last_step_size with a
// last step of non-zero size, else 1 - sample_eps.  ONE dt = t[1] - t[0] for all steps, q = sqrtf(dt).  With xi_i the noise of step i:
//   Euler-Maruyama   x <- (x + F(model(x, t_i), x; t_i) * dt) + G(t_i) * (xi_i * q)
//   Heun             xh = x + G(t_i) * (xi_i * q); K1 = F(model(xh, t_i), xh; t_i); xp = xh + dt * K1;
//                    K2 = F(model(xp, t_i + dt), xp; t_i + dt); x <- xh + (0.5 * dt) * (K1 + K2)         (t_i + dt: an fp32 sum, not t[i + 1])
//   last step at t1  none: x;  Mean: x + F(v, x; t1) * h;  Tweedie: x * (1 / alpha) + (sigma^2 / alpha) * (((R * v) - x) * iV);
//                    Euler: x + v * h            (h = last_step_size, v = model(x, t1))
// The reference evaluates the model twice per (state, time) with the same arguments, once for the drift and once for the score;
// one evaluation gives the same numbers.  Every coefficient is computed on the host in fp64 from the fp32 time and rounded once to
// fp32 (G = sqrtf(2 * D) in fp32); every written operation above is one rounded fp32 operation on the device (k_sde.hip), which
// never divides.  A plan with a non-finite coefficient that a state reads is refused (SBDM at sample_eps = 0 evaluates pi / (2 tan 0);
// Heun on the Linear path without a last step reaches t = 1 where sigma = 0).
// Orchestration as rk_body: ONE prepare() for all time rows, the states formed inside the embedding launches (k_sde_embed), views
// one after the other on the caller's stream, nothing read back: the whole solve is one hipGraph.  The caller owns the noise: a staged
// buffer (mdgen_sample_sde), or four seed words on the device from which the kernels generate it (philox.h: mdgen_sample_sde_rng and
// the fused drivers mdgen_rollout_sde / mdgen_upsample_sde of drivers.inc).
struct SdeCoef {
    float R, iV, D, G;
};
enum { kSdeUseScore = 1, kSdeUseD = 2, kSdeUseG = 4 };   // which coefficients of a row some state reads
struct SdePlan {
    std::vector<float> tg, rows;
    std::vector<SdeCoef> coef;   // per row
    std::vector<int> use;        // per row: kSdeUse* bits
    std::vector<int> row_of;     // [n_points - 1][stages]
    int stages, last_row;        // last_row: the row of t1, -1 without a last step
    float dt, hdt, q, h, c0, c1; // h: the last step's size; c0, c1: Tweedie's 1 / alpha, sigma^2 / alpha at t1
};

// th.linspace(start, end, n) in fp32 (ATen RangeFactories: symmetric evaluation around the midpoint), every operation rounded by itself
static void linspace_f32(float start, float end, int n, std::vector<float>* out) {
#pragma clang fp contract(off)
    out->resize(n);
    const float step = (end - start) / (float)(n - 1);
    const int half = n / 2;
    for (int i = 0; i < n; ++i) (*out)[i] = i < half ? start + step * (float)i : end - step * (float)(n - 1 - i);
}

static const double kSdePi = 3.14159265358979323846;
// alpha, alpha', sigma, sigma' and alpha' / alpha of path.py's ICPlan (path 0) / GVPCPlan (path 1) at t, in fp64
static void sde_path(int path, double t, double* al, double* dal, double* sg, double* dsg, double* ar) {
    if (path == 1) {
        const double a = t * kSdePi / 2;
        *al = std::sin(a); *dal = kSdePi / 2 * std::cos(a); *sg = std::cos(a); *dsg = -kSdePi / 2 * std::sin(a);
        *ar = kSdePi / (2 * std::tan(a));
    } else {
        *al = t; *dal = 1; *sg = 1 - t; *dsg = -1;
        *ar = 1 / t;
    }
}
static SdeCoef sde_coef(const mdgen_sde_opts& o, float tau) {
    const double t = tau, norm = o.diffusion_norm;
    double al, dal, sg, dsg, ar, D;
    sde_path(o.path, t, &al, &dal, &sg, &dsg, &ar);
    const double R = al / dal;
    switch (o.diffusion_form) {
    case 0: D = norm; break;
    case 1: D = norm * (ar * (sg * sg) - sg * dsg); break;                                 // SBDM: compute_drift(x, t)[1]
    case 2: D = norm * sg; break;
    case 3: D = norm * (1 - t); break;
    case 4: { const double u = norm * std::cos(kSdePi * t) + 1; D = 0.25 * (u * u); break; }
    default: { const double u = std::sin(kSdePi * t); D = norm * (u * u); break; }
    }
    SdeCoef c;
    c.R = (float)R;
    c.iV = (float)(1 / (sg * sg - R * dsg * sg));
    c.D = (float)D;
    c.G = sqrtf(2.f * c.D);
    return c;
}

// the options alone: judged without a context
static int sde_check(const mdgen_sde_opts* o) {
    if (!o) return fail(-1, "null argument");
    if (o->method < 1 || o->method > 2) return fail(-2, "method: 1 Euler-Maruyama, 2 Heun (got %d)", o->method);
    if (o->path < 0 || o->path > 1) return fail(-2, "path: 0 Linear, 1 GVP (got %d)", o->path);
    if (o->diffusion_form < 0 || o->diffusion_form > 5)
        return fail(-2, "diffusion_form: 0 constant, 1 SBDM, 2 sigma, 3 linear, 4 decreasing, 5 increasing-decreasing (got %d)", o->diffusion_form);
    if (o->last_step < 0 || o->last_step > 3) return fail(-2, "last_step: 0 none, 1 Mean, 2 Tweedie, 3 Euler (got %d)", o->last_step);
    if (o->n_points < 2) return fail(-2, "n_points must be >= 2");
    if (o->n_points > 100001) return fail(-2, "n_points too large");
    if (!(o->last_step_size >= 0 && o->last_step_size < 1)) return fail(-2, "last_step_size must be in [0, 1)");
    if (!(o->sample_eps >= 0 && o->sample_eps < 1)) return fail(-2, "sample_eps must be in [0, 1)");
    if (!std::isfinite(o->diffusion_norm)) return fail(-2, "diffusion_norm is not finite");
    return 0;
}

static int sde_plan(const mdgen_sde_opts& o, SdePlan* p) {
#pragma clang fp contract(off)
    if (int e = sde_check(&o)) return e;
    const double hs = o.last_step == 0 ? 0.0 : o.last_step_size;        // sample_sde: without a last step its size is 0
    const double t0d = o.diffusion_form == 1 ? o.sample_eps : 0.0, t1d = hs == 0.0 ? 1.0 - o.sample_eps : 1.0 - hs;
    const float t0 = (float)t0d, t1 = (float)t1d;
    if (!(t0 < t1)) return fail(-2, "the SDE sampler runs forward in time: t0 = %g >= t1 = %g", (double)t0, (double)t1);
    const int S = o.n_points - 1;
    linspace_f32(t0, t1, o.n_points, &p->tg);
    p->dt = p->tg[1] - p->tg[0];
    p->hdt = 0.5f * p->dt;
    p->q = sqrtf(p->dt);
    p->h = (float)hs;
    p->stages = o.method;
    p->rows.clear();
    p->use.clear();
    p->row_of.assign((size_t)S * p->stages, 0);
    auto row = [&](float t, int use) {   // a time equal to the row before it shares that row
        if (p->rows.empty() || std::memcmp(&p->rows.back(), &t, sizeof(float)) != 0) {
            p->rows.push_back(t);
            p->use.push_back(0);
        }
        p->use.back() |= use;
        return (int)p->rows.size() - 1;
    };
    for (int i = 0; i < S; ++i) {
        p->row_of[(size_t)i * p->stages] = row(p->tg[i], kSdeUseScore | kSdeUseD | kSdeUseG);
        if (o.method == 2) p->row_of[(size_t)i * 2 + 1] = row(p->tg[i] + p->dt, kSdeUseScore | kSdeUseD);
    }
    p->last_row = o.last_step == 0 ? -1 : row(t1, o.last_step == 1 ? kSdeUseScore | kSdeUseD : o.last_step == 2 ? kSdeUseScore : 0);
    p->coef.resize(p->rows.size());
    for (size_t k = 0; k < p->rows.size(); ++k) {
        const SdeCoef c = p->coef[k] = sde_coef(o, p->rows[k]);
        const int u = p->use[k];
        const char* bad = (u & kSdeUseScore) && !std::isfinite(c.R) ? "R = alpha / alpha'"
                        : (u & kSdeUseScore) && !std::isfinite(c.iV) ? "iV = 1 / (sigma^2 - R sigma' sigma)"
                        : (u & kSdeUseD) && !std::isfinite(c.D) ? "D (the diffusion)"
                        : (u & kSdeUseG) && !std::isfinite(c.G) ? "G = sqrt(2 D)" : nullptr;
        if (bad) return fail(-2, "coefficient %s is not finite at t = %.9g (SBDM needs sample_eps > 0; the Linear path cannot be evaluated at t = 1)",
                             bad, (double)p->rows[k]);
    }
    p->c0 = p->c1 = 0.f;
    if (o.last_step == 2) {
        double al, dal, sg, dsg, ar;
        sde_path(o.path, (double)t1, &al, &dal, &sg, &dsg, &ar);
        p->c0 = (float)(1 / al);
        p->c1 = (float)(sg * sg / al);
        if (!std::isfinite(p->c0) || !std::isfinite(p->c1)) return fail(-2, "coefficient 1 / alpha is not finite at t = %.9g", (double)t1);
    }
    return 0;
}

extern "C" int32_t mdgen_sde_workspace_bytes(const mdgen_ctx* c, const mdgen_shape* sh, const mdgen_sde_opts* o, size_t* bytes) {
    if (!bytes || !o) return fail(-1, "null argument");
    SdePlan pl;
    mdgen_ws_layout lay;
    if (int e = sde_plan(*o, &pl)) return e;
    if (int e = mdgen_workspace_layout(c, sh, (int)pl.rows.size(), 1, &lay)) return e;
    *bytes = grid_ws_bytes(c, sh, lay, 2);
    return 0;
}

// the device descriptor of a state: coefficients of rows r0 (R[0] ...) and r1, the noise term's G of row rg (-1: none)
static SdeState sde_state_of(const SdePlan& pl, int form, bool store, int r0, int r1, int rg, float dt, float* y, const float* v0,
                             const float* v1, const float* xi) {
    SdeState s{};
    s.form = form;
    s.store = store ? 1 : 0;
    s.dt = dt;
    s.hdt = pl.hdt;
    s.q = pl.q;
    const int rr[2] = {r0, r1};
    for (int j = 0; j < 2; ++j)
        if (rr[j] >= 0) { s.R[j] = pl.coef[rr[j]].R; s.iV[j] = pl.coef[rr[j]].iV; s.D[j] = pl.coef[rr[j]].D; }
    if (rg >= 0) s.G = pl.coef[rg].G;
    s.c[0] = pl.c0;
    s.c[1] = pl.c1;
    s.v[0] = v0; s.v[1] = v1; s.xi = xi; s.y = y;
    return s;
}

// Where a solve's noise comes from: the caller's buffer (step i's at buf + i * stride), or -- rng: the device words {seed,
// sample_base, block_base, 0} -- philox.h evaluated in the kernels at (element, sample, step, block_base + block)
struct SdeNoise {
    const float* buf;
    long stride;
    const uint64_t* rng;
    int block;
};
// `s`, a noise-reading state, with step `step`'s noise
static SdeState with_noise(SdeState s, const SdeNoise& nz, int step) {
    if (nz.rng) { s.rng = nz.rng; s.step = step; s.block = nz.block; }
    else s.xi = nz.buf + (long)step * nz.stride;
    return s;
}

// the state the first launch after step i (0 <= i < S) forms: the step's result, for Heun with the next step's noise term where
// there is a next step
static SdeState sde_result_of(const mdgen_sde_opts& o, const SdePlan& pl, int i, float* x, float* const* v, const SdeNoise& nz) {
    const int S = o.n_points - 1;
    if (o.method == 1)
        return with_noise(sde_state_of(pl, kSdeEm, true, pl.row_of[i], -1, pl.row_of[i], pl.dt, x, v[0], nullptr, nullptr), nz, i);
    const int r0 = pl.row_of[(size_t)i * 2], r1 = pl.row_of[(size_t)i * 2 + 1];
    if (i + 1 < S)
        return with_noise(sde_state_of(pl, kSdeHeunNoise, true, r0, r1, pl.row_of[(size_t)(i + 1) * 2], pl.dt, x, v[0], v[1], nullptr), nz, i + 1);
    return sde_state_of(pl, kSdeHeun, true, r0, r1, -1, pl.dt, x, v[0], v[1], nullptr);
}
static SdeState sde_last_of(const mdgen_sde_opts& o, const SdePlan& pl, float* x, float* const* v) {
    const int form = o.last_step == 1 ? kSdeDrift : o.last_step == 2 ? kSdeTweedie : kSdeEuler;
    return sde_state_of(pl, form, true, pl.last_row, -1, -1, pl.h, x, v[0], nullptr, nullptr);
}

// the solve on a made run: x in place, v[0 .. 1] the velocities, the noise from `nz`
static int sde_body(const Run& r_in, const mdgen_sde_opts& o, const SdePlan& pl, int nv, float* x, float* const* v, const SdeNoise& nz) {
    Run r = r_in;
    if (int e = ode_prepare(r, pl.rows.data(), (int)pl.rows.size(), largest_view_rows(r, nv))) return e;
    const long per_b = (long)r.T * r.L * r.D;
    const int S = o.n_points - 1;
    auto update = [&](SdeState st) {   // the whole call's state in one launch
        st.per_b = (unsigned)per_b;
        return launch(r, "ode_sde_update", [&] { launch_sde_update(st, (long)r.N * r.D, r.s); });
    };
    for (int i = 0; i < S; ++i) {
        // the first launch of step i forms the previous step's result (Heun: with this step's noise term) and stores it over x
        const SdeState first = i > 0 ? sde_result_of(o, pl, i - 1, x, v, nz)
                               : o.method == 1 ? sde_state_of(pl, kSdeX, false, -1, -1, -1, pl.dt, x, nullptr, nullptr, nullptr)
                                               : with_noise(sde_state_of(pl, kSdeNoise, true, -1, -1, pl.row_of[0], pl.dt, x, nullptr, nullptr, nullptr), nz, 0);
        if (int e = eval_state(r, nv, first, pl.row_of[(size_t)i * pl.stages], v[0])) return e;
        if (o.method == 2) {   // the predictor xp: in registers only
            const SdeState xp = sde_state_of(pl, kSdeDrift, false, pl.row_of[(size_t)i * 2], -1, -1, pl.dt, x, v[0], nullptr, nullptr);
            if (int e = eval_state(r, nv, xp, pl.row_of[(size_t)i * 2 + 1], v[1])) return e;
        }
    }
    const SdeState res = sde_result_of(o, pl, S - 1, x, v, nz);
    if (o.last_step == 0) return update(res);
    if (int e = eval_state(r, nv, res, pl.last_row, v[0])) return e;
    return update(sde_last_of(o, pl, x, v));
}

// What mdgen_sample_sde, mdgen_sample_sde_rng, mdgen_rollout_sde and mdgen_upsample_sde share once their own arguments are judged (as
// RkCall, ode.inc): the plan, the GridCall with two velocity buffers and the options as they enter a graph key.  `state` is the
// buffer k_sde_update will see (16-byte accesses).
struct SdeCall : GridCall {
    mdgen_sde_opts o, key;
    SdePlan pl;
    int solve(float* x, const SdeNoise& nz) const { return sde_body(r, o, pl, nv, x, vel, nz); }
};
static int sde_open(SdeCall* q, mdgen_ctx* c, const mdgen_shape* sh, const mdgen_sde_opts* o, const float* state, const SdeNoise& nz,
                    const mdgen_cond& cd, void* ws, size_t ws_bytes, void* stream) {
    if (!sh) return fail(-1, "null argument");
    if (int e = sde_plan(*o, &q->pl)) return e;
    q->o = *o;
    if (nz.rng) {
        if (((uintptr_t)state & 15) != 0) return fail(-7, "x must be 16-byte aligned");
        if (((uintptr_t)nz.rng & 7) != 0) return fail(-7, "rng must be 8-byte aligned");
        // counter word c0 is the element's index within its sample
        if (sh->T > 0 && sh->L > 0 && (uint64_t)sh->T * sh->L * (c ? c->D : 21) >= (1ull << 32))
            return fail(-2, "T * L * D = %llu elements of one sample do not fit the generator's 32-bit element counter",
                        (unsigned long long)sh->T * sh->L * (c ? c->D : 21));
    } else {
        if (((uintptr_t)state & 15) != 0 || ((uintptr_t)nz.buf & 15) != 0) return fail(-7, "x and noise must be 16-byte aligned");
        // k_sde_update reads a step's noise 16 bytes at a time, and a state of B T L D floats ends on 16 bytes only for some shapes:
        // the caller chooses the stride (as zs_block_stride of mdgen_rollout_rk)
        const long n = (long)sh->B * sh->T * sh->L * (c ? c->D : 21);
        if (nz.stride % 4 != 0) return fail(-7, "noise_step_stride must be a multiple of 4 floats (got %lld)", (long long)nz.stride);
        if (nz.stride < n) return fail(-7, "noise_step_stride %lld is below one state of %ld floats", (long long)nz.stride, n);
    }
    mdgen_ws_layout lay;
    if (int e = mdgen_workspace_layout(c, sh, (int)q->pl.rows.size(), 1, &lay)) return e;
    if (int e = grid_open(q, lay, (int)q->pl.rows.size(), 2, "mdgen_sde_workspace_bytes", c, sh, cd, ws, ws_bytes, stream)) return e;
    mdgen_sde_opts& k = q->key;   // (field by field: the struct's padding does not reach the key)
    std::memset(&k, 0, sizeof(k));
    k.method = o->method; k.path = o->path; k.diffusion_form = o->diffusion_form; k.last_step = o->last_step; k.n_points = o->n_points;
    k.diffusion_norm = o->diffusion_norm; k.last_step_size = o->last_step_size; k.sample_eps = o->sample_eps;
    return 0;
}

extern "C" int32_t mdgen_sample_sde(mdgen_ctx* c, const mdgen_shape* sh, const mdgen_sde_opts* o, float* x, const float* noise,
                                    int64_t stride, const mdgen_cond* cond, void* ws, size_t ws_bytes, int32_t use_graph, void* stream) {
    if (!x || !noise || !o) return fail(-1, "null argument");
    if (int e = check_cond(cond)) return e;
    const SdeNoise nz{noise, (long)stride, nullptr, 0};
    SdeCall q;
    if (int e = sde_open(&q, c, sh, o, x, nz, *cond, ws, ws_bytes, stream)) return e;
    GraphKey key = graph_key(6, q.r, *cond);
    key.add_struct(q.key).add((uint64_t)stride).ptr(x).ptr(noise);   // (the body does not fork: no n_streams)
    return run_or_replay(q.r, use_graph, key, [&]() { return q.solve(x, nz); });
}

// mdgen_sample_sde with the noise generated in the kernels: no buffer, no stride.  The seed words are read on the device, so the key
// holds their address and a replay draws what they hold then.
extern "C" int32_t mdgen_sample_sde_rng(mdgen_ctx* c, const mdgen_shape* sh, const mdgen_sde_opts* o, float* x, const uint64_t* rng,
                                        const mdgen_cond* cond, void* ws, size_t ws_bytes, int32_t use_graph, void* stream) {
    if (!x || !rng || !o) return fail(-1, "null argument");
    if (int e = check_cond(cond)) return e;
    const SdeNoise nz{nullptr, 0, rng, 0};
    SdeCall q;
    if (int e = sde_open(&q, c, sh, o, x, nz, *cond, ws, ws_bytes, stream)) return e;
    GraphKey key = graph_key(7, q.r, *cond);
    key.add_struct(q.key).ptr(x).ptr(rng);
    return run_or_replay(q.r, use_graph, key, [&]() { return q.solve(x, nz); });
}

// Test hook: one step's generated noise, xi (B, T, L, D) to `out` -- k_sde_update's generator instantiation forming 0 + 1 * (xi * 1).
extern "C" int32_t mdgen_debug_sde_noise(const mdgen_shape* sh, int32_t latent_dim, const uint64_t* rng, int32_t step, int32_t block,
                                         float* out, void* stream) {
    if (!sh || !rng || !out) return fail(-1, "null argument");
    if (sh->B < 1 || sh->T < 1 || sh->L < 1 || latent_dim < 1) return fail(-2, "B, T, L, latent_dim must be >= 1");
    if ((uint64_t)sh->T * sh->L * latent_dim >= (1ull << 32)) return fail(-2, "T * L * D does not fit the generator's 32-bit element counter");
    if (((uintptr_t)out & 15) != 0 || ((uintptr_t)rng & 7) != 0) return fail(-7, "out must be 16-byte aligned, rng 8-byte aligned");
    const long n = (long)sh->B * sh->T * sh->L * latent_dim;
    SdeState st{};
    st.form = kSdeNoise;
    st.store = 1;
    st.q = st.G = 1.f;
    st.y = out;
    st.rng = rng;
    st.step = step;
    st.block = block;
    st.per_b = (unsigned)((long)sh->T * sh->L * latent_dim);
    HIPCHK(hipMemsetAsync(out, 0, (size_t)n * sizeof(float), (hipStream_t)stream));
    launch_sde_update(st, n, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

// Host-only test hook: philox.h's Philox4x32-10 compiled for the host.  ctr[4], key[2] -> out[4].
extern "C" int32_t mdgen_debug_philox(const uint32_t* ctr, const uint32_t* key, uint32_t* out) {
    if (!ctr || !key || !out) return fail(-1, "null argument");
    const uint32_t c[4] = {ctr[0], ctr[1], ctr[2], ctr[3]}, k[2] = {key[0], key[1]};
    uint32_t w[4];
    philox4x32_10(c, k, w);
    std::memcpy(out, w, sizeof(w));
    return 0;
}

// Host-only test hook: the plan of mdgen_sample_sde for `o`, as fp32 bits.  row_bits[cap_rows], coef_bits[cap_rows][4] (R, iV, D, G per
// row), row_of[n_points - 1][*n_stages], *last_row (-1 without a last step), scalar_bits[6]: dt, q, 0.5 dt, h, Tweedie's c0, c1.
extern "C" int32_t mdgen_debug_sde_plan(const mdgen_sde_opts* o, uint32_t* row_bits, uint32_t* coef_bits, int32_t cap_rows, int32_t* n_rows,
                                        int32_t* row_of, int32_t* n_stages, int32_t* last_row, uint32_t* scalar_bits) {
    if (!o || !row_bits || !coef_bits || !n_rows || !row_of || !n_stages || !last_row || !scalar_bits) return fail(-1, "null argument");
    SdePlan pl;
    if (int e = sde_plan(*o, &pl)) return e;
    *n_rows = (int32_t)pl.rows.size();
    *n_stages = pl.stages;
    *last_row = pl.last_row;
    if (cap_rows < *n_rows) return fail(-7, "row buffer too small: %d < %d", cap_rows, *n_rows);
    std::memcpy(row_bits, pl.rows.data(), pl.rows.size() * sizeof(float));
    static_assert(sizeof(SdeCoef) == 4 * sizeof(float), "four packed floats");
    std::memcpy(coef_bits, pl.coef.data(), pl.coef.size() * sizeof(SdeCoef));
    for (size_t i = 0; i < pl.row_of.size(); ++i) row_of[i] = pl.row_of[i];
    const float sc[6] = {pl.dt, pl.q, pl.hdt, pl.h, pl.c0, pl.c1};
    std::memcpy(scalar_bits, sc, sizeof(sc));
    return 0;
}

// Test hook: k_sde_embed alone on one state of the solve `o` describes.  state: an SdeForm (kernels.h) of step `step` -- 0 x, 1 x +
// noise term, 2 the Euler-Maruyama step, 3 Heun's predictor, 4 Heun's result, 5 Heun's result + the noise term of step + 1 -- or a last
// step at t1: 6 Tweedie, 7 Euler, 8 Mean.  x (B, T, L, D) is overwritten by every state but 0 and 3; v0, v1, xi: what the state reads
// (xi: ONE step's noise); with `rng` the noise-reading states generate theirs: the noise of step `step` (states 1, 2) or `step` + 1
// (state 5) of block `block`.
static int sde_stage(mdgen_ctx* c, const mdgen_shape* sh, const mdgen_sde_opts* o, int state, int step, float* x, const float* v0,
                     const float* v1, const float* xi, const uint64_t* rng, int block, const float* x_cond, const int64_t* x_cond_mask,
                     const float* ipa_out, float* h, void* stream) {
    if (!x || !x_cond || !x_cond_mask || !h || !o) return fail(-1, "null argument");
    SdePlan pl;
    if (int e = sde_plan(*o, &pl)) return e;
    const int S = o->n_points - 1;
    if (state < 0 || state > 8) return fail(-2, "state must be in 0 .. 8");
    if (step < 0 || step >= S || (state == 5 && step + 1 >= S)) return fail(-2, "step out of range");
    const bool heun = state >= 3 && state <= 5, last = state >= 6;
    if (heun && o->method != 2) return fail(-2, "state %d is a state of the Heun method", state);
    if (last && o->last_step != (state == 6 ? 2 : state == 7 ? 3 : 1)) return fail(-2, "state %d is not the last step of these options", state);
    if (int e = check_shape(c, sh, 1)) return e;
    if (!c->finalized) return fail(-6, "context not finalized (mdgen_ctx_finalize)");
    const bool reads_v0 = state >= 2, reads_v1 = state == 4 || state == 5, reads_xi = state == 1 || state == 2 || state == 5;
    if ((reads_v0 && !v0) || (reads_v1 && !v1) || (reads_xi && !xi && !rng)) return fail(-1, "the state reads an operand that is null");
    float* vv[2] = {const_cast<float*>(v0), const_cast<float*>(v1)};
    const int r0 = pl.row_of[(size_t)step * pl.stages], r1 = pl.stages == 2 ? pl.row_of[(size_t)step * 2 + 1] : -1;
    const SdeNoise nz{xi, 0, rng, block};   // (stride 0: xi is the one step's noise whichever step the state names)
    SdeState st;
    switch (state) {
    case 0: st = sde_state_of(pl, kSdeX, false, -1, -1, -1, pl.dt, x, nullptr, nullptr, nullptr); break;
    case 1: st = with_noise(sde_state_of(pl, kSdeNoise, true, -1, -1, r0, pl.dt, x, nullptr, nullptr, nullptr), nz, step); break;
    case 2: st = with_noise(sde_state_of(pl, kSdeEm, true, r0, -1, r0, pl.dt, x, v0, nullptr, nullptr), nz, step); break;
    case 3: st = sde_state_of(pl, kSdeDrift, false, r0, -1, -1, pl.dt, x, v0, nullptr, nullptr); break;
    case 4: st = sde_state_of(pl, kSdeHeun, true, r0, r1, -1, pl.dt, x, v0, v1, nullptr); break;
    case 5: st = with_noise(sde_state_of(pl, kSdeHeunNoise, true, r0, r1, pl.row_of[(size_t)(step + 1) * 2], pl.dt, x, v0, v1, nullptr), nz, step + 1); break;
    default: st = sde_last_of(*o, pl, x, vv); break;
    }
    st.per_b = (unsigned)((long)sh->T * sh->L * c->D);
    launch_sde_embed(embed_params(c, *sh, x, x_cond, x_cond_mask, ipa_out, h), st, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}
extern "C" int32_t mdgen_debug_sde_stage(mdgen_ctx* c, const mdgen_shape* sh, const mdgen_sde_opts* o, int32_t state, int32_t step, float* x,
                                         const float* v0, const float* v1, const float* xi, const float* x_cond, const int64_t* x_cond_mask,
                                         const float* ipa_out, float* h, void* stream) {
    return sde_stage(c, sh, o, state, step, x, v0, v1, xi, nullptr, 0, x_cond, x_cond_mask, ipa_out, h, stream);
}
extern "C" int32_t mdgen_debug_sde_stage_rng(mdgen_ctx* c, const mdgen_shape* sh, const mdgen_sde_opts* o, int32_t state, int32_t step,
                                             int32_t block, float* x, const float* v0, const float* v1, const uint64_t* rng,
                                             const float* x_cond, const int64_t* x_cond_mask, const float* ipa_out, float* h, void* stream) {
    if (!rng) return fail(-1, "null argument");
    if (((uintptr_t)rng & 7) != 0) return fail(-7, "rng must be 8-byte aligned");
    return sde_stage(c, sh, o, state, step, x, v0, v1, nullptr, rng, block, x_cond, x_cond_mask, ipa_out, h, stream);
}
