// ode.inc -- the ODE solvers beyond the Euler rollout (included by api.hip): adaptive Dormand-Prince sampling (kernels in k_ode.hip),
// then, further down, fixed-grid midpoint / heun3 / rk4 (kernels in k_rk.hip).
//
// The reference's NewMDGenWrapper.inference() integrates with the checkpoint's own `sampling_method` (wrapper.py:441-447), by
// default 'dopri5' (parsing.py:102): transport.py:408-451 / integrators.py:74-113 call
//     odeint(f, x0, t = linspace(0, 1, 50) fp32, method='dopri5', atol=[1e-6], rtol=[1e-3])[-1],   f(t, x) = model(x, ones(B) t)
// (velocity drift, transport.py:242-244).  This file restates torchdiffeq 0.2.x's dopri5 (rk_common.py
// RKAdaptiveStepsizeODESolver, misc.py _select_initial_step / _optimal_step_size, dopri5.py tableau) with its mixed precision:
//   - state, stages and k are fp32; time-like values (t0, dt, t1) fp64; atol / rtol are 1-element fp64 tensors, so the
//     tolerances, the norms and the error ratio are fp64; every time that reaches the model is cast to fp32 first;
//   - the norm is the RMS over every element of the whole (B, T, L, D) state (all samples, conditioning frames, padded
//     residues): ONE step size for the whole batch -- a B = 2 call is not two B = 1 solves;
//   - the 50-point output grid only decides where the solve stops: the steps are taken until an accepted step ends at
//     t1 >= 1 (the model is evaluated past t = 1, nothing is clamped) and the output is that step's 4th-order dense output
//     at t = 1;
//   - network evaluations: 2 (k1, and the initial-step probe) + 6 per attempted step (FSAL: k7 of an accepted step is k1
//     of the next).
// Orchestration: per attempted step ONE prepare() for its six stage times as t-shared rows (adaLN table, IPA stack, folded
// fc2 streams), then six denoise_step(..., out = k_i, euler = 0) -- the sampler's own network path; the FinalLayer tail of
// the last MLP launch writes the velocity.  The embedding-as-tail form is not used (the next stage's input is not known
// inside the launch).  Batches that need several launch views run them per stage on the caller's stream.
// Controller: plain host C++ in fp64 (Dopri5Ctl).  Once per attempted step the error ratio (8 bytes) is copied into pinned
// memory and the caller's stream is synchronised -- the documented exception to "nothing synchronises".

namespace ode {
constexpr int kStages = 6;     // network evaluations per attempted step (k2 .. k7)
constexpr int kBufs = 9;       // Y1 (stage inputs; y1 after stage 7), K0 .. K6, Y_mid; Y0 starts as the caller's x
// dopri5.py _DORMAND_PRINCE_SHAMPINE_TABLEAU and DPS_C_MID: fp64 expressions, cast to the state's dtype (fp32) by the solver
const double kAlpha[kStages] = {1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0, 1.0};
const double kBeta[kStages][kStages] = {
    {1.0 / 5},
    {3.0 / 40, 9.0 / 40},
    {44.0 / 45, -56.0 / 15, 32.0 / 9},
    {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729},
    {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656},
    {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84}};
const double kErr[7] = {35.0 / 384 - 1951.0 / 21600, 0, 500.0 / 1113 - 22642.0 / 50085, 125.0 / 192 - 451.0 / 720,
                        -2187.0 / 6784 - -12231.0 / 42400, 11.0 / 84 - 649.0 / 6300, -1.0 / 60.0};
const double kMid[7] = {6025192743.0 / 30085553152.0 / 2, 0, 51252292925.0 / 65400821598.0 / 2, -2691868925.0 / 45128329728.0 / 2,
                        187940372067.0 / 1594534317056.0 / 2, -1776094331.0 / 19743644256.0 / 2, 11237099.0 / 235043384.0 / 2};
}  // namespace ode

// The step-size controller: a pure state machine over the norms the device reports (no HIP call).
struct Dopri5Ctl {
    double t0 = 0.0, dt = 0.0;         // time of the current state; step to attempt next
    double last_t0 = 0.0, last_dt = 0.0, last_t1 = 0.0;   // the last accepted step (its dense output gives the result)
    double h0 = 0.0;                   // initial-step probe (misc.py _select_initial_step)
    bool h0_f32 = false;               // ... the d0 | d1 < 1e-5 branch makes h0 an fp32 tensor
    bool done = false;
    int accepted = 0, rejected = 0;

    // from d0 = rms(x0 / scale), d1 = rms(k1 / scale): h0; the probe evaluates f(t0 + h0, x0 + h0 k1)
    void probe(double d0, double d1) {
        if (d0 < 1e-5 || d1 < 1e-5) {
            h0 = (double)1e-6f;
            h0_f32 = true;
        } else {
            h0 = 0.01 * d0 / d1;
            h0_f32 = false;
        }
        h0 = std::fabs(h0);
    }
    float probe_coef() const { return (float)h0; }             // y1 = y0 + h0 * f0 in fp32
    float probe_time() const { return (float)(t0 + h0); }      // t0 + h0 in fp64, cast for the model
    // d2n = rms((f1 - k1) / scale): the first step
    void first_step(double d1, double d2n) {
        const double d2 = std::fabs(d2n / h0);
        double h1;
        if (d1 <= 1e-15 && d2 <= 1e-15) {
            if (h0_f32) {
                const float a = 1e-6f, b = (float)h0 * (float)1e-3;
                h1 = (double)(a < b ? b : a);
            } else {
                const double a = (double)1e-6f, b = h0 * 1e-3;
                h1 = a < b ? b : a;
            }
        } else {
            h1 = std::pow(0.01 / std::max(d1, d2), 1.0 / (double)(4 + 1));   // order - 1 = 4
        }
        h1 = std::fabs(h1);
        const double big = h0_f32 ? (double)(100.f * (float)h0) : 100 * h0;
        dt = std::min(big, h1);
    }
    // model times of the six stages (rk_common.py _runge_kutta_step): fp32 t0 + alpha dt; the alpha = 1 stages at
    // nextafter(fp32(t0 + dt), -inf) (Perturb.PREV)
    void stage_times(float* t) const {
#pragma clang fp contract(off)
        const float t0f = (float)t0, dtf = (float)dt, t1f = (float)(t0 + dt);
        for (int i = 0; i < ode::kStages; ++i) {
            const float a = (float)ode::kAlpha[i];
            t[i] = a == 1.f ? std::nextafter(t1f, -INFINITY) : t0f + a * dtf;
        }
    }
    float dt32() const { return (float)dt; }
    bool underflow() const { return !(t0 + dt > t0); }
    // one attempted step's error ratio: accept iff ratio <= 1; the next dt (misc.py _optimal_step_size: safety 0.9,
    // ifactor 10, dfactor 0.2, order 5)
    bool step(double ratio) {
        const bool accept = ratio <= 1;
        const double t1 = t0 + dt;
        if (accept) {
            last_t0 = t0;
            last_dt = dt;
            last_t1 = t1;
            t0 = t1;
            ++accepted;
            done = t0 >= 1.0;   // torchdiffeq _advance: while next_t (= 1.0) > t1
        } else {
            ++rejected;
        }
        double f;
        if (ratio == 0) {
            f = 10.0;
        } else {
            const double dfac = ratio < 1 ? 1.0 : 0.2;
            const double g = 0.9 / std::pow(ratio, 1.0 / 5.0);
            f = std::min(10.0, std::max(g, dfac));
        }
        dt = dt * f;
        return accept;
    }
    // rk_common.py _interp_evaluate: s = (t - t0) / (t1 - t0) at t = 1, cast to fp32
    float dense_s() const { return (float)((1.0 - last_t0) / (last_t1 - last_t0)); }
};

struct OdeBufs {
    float *y0, *y1, *k[7], *ym;
    double *part, *out;
};

static size_t ode_state_bytes(const mdgen_ctx* c, const mdgen_shape* sh) {
    return align256((size_t)sh->B * sh->T * sh->L * c->D * 4);
}

extern "C" int32_t mdgen_dopri5_workspace_bytes(const mdgen_ctx* c, const mdgen_shape* sh, size_t* bytes) {
    if (!bytes) return fail(-1, "null argument");
    mdgen_ws_layout lay;
    if (int e = mdgen_workspace_layout(c, sh, ode::kStages, 1, &lay)) return e;
    *bytes = align256(lay.total_bytes) + ode::kBufs * ode_state_bytes(c, sh) + align256((size_t)kOdeMaxParts * 2 * 8) + 256;
    return 0;
}

// y = y0 + sum_{j < n} fp32(fp32(coef_j) * dt) k_j
static int ode_combine(const Run& r, float* y, const float* y0, float* const* k, const double* coef, int n, float dt) {
#pragma clang fp contract(off)
    OdeTerms p{};
    for (int j = 0; j < n; ++j) {
        p.k[j] = k[j];
        p.c[j] = (float)coef[j] * dt;
    }
    p.nk = n;
    return launch(r, "ode_combine", [&] { launch_ode_combine(y, y0, p, (long)r.N * r.D, r.s); });
}

static int ode_norm(const Run& r, const OdeBufs& b, const OdeNorm& p) {
    return launch(r, "ode_norm", [&] { launch_ode_norm(p, (long)r.N * r.D, b.part, b.out, r.s); });
}

// prepare() for `n` time rows shared by the batch (the workspace is carved for kStages rows)
static int ode_prepare(Run& r, const float* times, int n, long view_rows) {
    r.S = n;
    r.Mp = (long)n * r.B * r.L;
    return prepare(r, nullptr, times, view_rows);
}

// one network evaluation at prepared row `row`: y -> velocity k, over the call's launch views on the caller's stream
static int ode_eval(const Run& r, int nv, int row, const float* y, float* k) {
    return for_each_view(r, nv, 1, [&](const Run& v, int b0) {
        const long o = (long)b0 * r.T * r.L * r.D;
        return denoise_step(v, row, const_cast<float*>(y) + o, k + o, 0, 0.f, nullptr);
    });
}

// One attempted step from (t0, Y0, K0, dt): prepare the six stage rows, y_i = y0 + sum_j beta_ij dt k_j -> k_i (Y1 = y1
// after stage 7), then the error ratio into b.out[0] (on the device; the caller reads it back).
static int dopri5_attempt(Run& r, const OdeBufs& b, const Dopri5Ctl& ctl, int nv, long view_rows, double atol, double rtol) {
#pragma clang fp contract(off)
    float ts[ode::kStages];
    ctl.stage_times(ts);
    if (int e = ode_prepare(r, ts, ode::kStages, view_rows)) return e;
    const float dtf = ctl.dt32();
    for (int i = 1; i <= ode::kStages; ++i) {
        if (int e = ode_combine(r, b.y1, b.y0, b.k, ode::kBeta[i - 1], i, dtf)) return e;
        if (int e = ode_eval(r, nv, i - 1, b.y1, b.k[i])) return e;
    }
    OdeNorm p{};
    p.a = b.y0;
    p.b = b.y1;
    for (int j = 0; j < 7; ++j) {
        p.k[j] = b.k[j];
        p.e[j] = (float)ode::kErr[j] * dtf;
    }
    p.atol = atol;
    p.rtol = rtol;
    p.mode = 2;
    return ode_norm(r, b, p);
}

static OdeBufs ode_bufs(unsigned char* ws, size_t net_bytes, size_t state_bytes, float* x) {
    OdeBufs b;
    unsigned char* p = ws + align256(net_bytes);
    b.y0 = x;
    b.y1 = (float*)p;
    p += state_bytes;
    for (int j = 0; j < 7; ++j, p += state_bytes) b.k[j] = (float*)p;
    b.ym = (float*)p;
    p += state_bytes;
    b.part = (double*)p;
    b.out = (double*)(p + align256((size_t)kOdeMaxParts * 2 * 8));
    return b;
}

static int ode_read(mdgen_ctx* c, const OdeBufs& b, hipStream_t s, double* v0, double* v1) {
    HIPCHK(hipMemcpyAsync(c->ode_host, b.out, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *v0 = c->ode_host[0];
    if (v1) *v1 = c->ode_host[1];
    return 0;
}

extern "C" int32_t mdgen_sample_dopri5(mdgen_ctx* c, const mdgen_shape* sh, double atol, double rtol, int32_t max_steps, float* x,
                                       const mdgen_cond* cond, void* ws, size_t ws_bytes, int32_t* stats_host, double* steps_host,
                                       void* stream) {
    if (!x || !stats_host) return fail(-1, "null argument");
    if (int e = check_cond(cond)) return e;
    stats_host[0] = stats_host[1] = stats_host[2] = 0;
    if (!(atol >= 0) || !(rtol >= 0) || !(atol + rtol > 0) || !std::isfinite(atol) || !std::isfinite(rtol))
        return fail(-2, "atol, rtol must be finite, >= 0, not both 0");
    if (max_steps < 1) return fail(-2, "max_steps must be >= 1");
    const hipStream_t s = (hipStream_t)stream;
    {   // the controller reads the error ratio back after every attempted step: not capturable
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        const hipError_t e = hipStreamIsCapturing(s, &cs);
        if (e != hipSuccess) return fail((int)e, "hipStreamIsCapturing failed: %s", hipGetErrorString(e));
        if (cs != hipStreamCaptureStatusNone) return fail(-8, "mdgen_sample_dopri5 synchronises its stream: it cannot be captured");
    }
    if (((uintptr_t)x & 15) != 0) return fail(-7, "x must be 16-byte aligned");
    size_t need = 0;
    if (int e = mdgen_dopri5_workspace_bytes(c, sh, &need)) return e;
    if (ws_bytes < need) return fail(-7, "workspace too small: %zu < %zu bytes (mdgen_dopri5_workspace_bytes)", ws_bytes, need);
    mdgen_ws_layout lay;
    if (int e = mdgen_workspace_layout(c, sh, ode::kStages, 1, &lay)) return e;
    Run r{};
    if (int e = make_run(&r, c, sh, ode::kStages, 1, f32_path(c), ws, lay.total_bytes, stream)) return e;
    bind_cond(r, *cond);
    r.no_embed_tail = true;
    if (!c->ode_host) HIPCHK(hipHostMalloc((void**)&c->ode_host, 2 * sizeof(double), hipHostMallocDefault));
    const int nv = c->opt_precision == 32 ? 1 : plan_views(r.B, r.T, r.L, 1);
    if (nv == 0) return fail(-2, "sample too large for one launch");
    const long vrows = largest_view_rows(r, nv);
    OdeBufs b = ode_bufs((unsigned char*)ws, lay.total_bytes, ode_state_bytes(c, sh), x);
    Dopri5Ctl ctl;
    int nfe = 0;
    // ---- initial step (misc.py _select_initial_step, order 4): k1 = f(0, x0), probe f(h0, x0 + h0 k1)
    {
        const float t0f = 0.f;
        if (int e = ode_prepare(r, &t0f, 1, vrows)) return e;
        if (int e = ode_eval(r, nv, 0, b.y0, b.k[0])) return e;
        ++nfe;
        OdeNorm p{};
        p.a = b.y0;
        p.b = b.k[0];
        p.atol = atol;
        p.rtol = rtol;
        p.mode = 0;
        if (int e = ode_norm(r, b, p)) return e;
        double d0 = 0, d1 = 0;
        if (int e = ode_read(c, b, s, &d0, &d1)) return e;
        ctl.probe(d0, d1);
        const double one = 1.0;
        float* k0 = b.k[0];
        if (int e = ode_combine(r, b.y1, b.y0, &k0, &one, 1, ctl.probe_coef())) return e;
        const float th = ctl.probe_time();
        if (int e = ode_prepare(r, &th, 1, vrows)) return e;
        if (int e = ode_eval(r, nv, 0, b.y1, b.k[1])) return e;
        ++nfe;
        p.k[0] = b.k[1];
        p.mode = 1;
        if (int e = ode_norm(r, b, p)) return e;
        double d2n = 0;
        if (int e = ode_read(c, b, s, &d2n, nullptr)) return e;
        if (!std::isfinite(d0) || !std::isfinite(d1) || !std::isfinite(d2n))
            return fail(-9, "non-finite initial-step norm (d0 %g, d1 %g, d2 %g)", d0, d1, d2n);
        ctl.first_step(d1, d2n);
        stats_host[0] = nfe;
    }
    // ---- attempted steps until an accepted one ends at t1 >= 1
    for (int attempt = 0; !ctl.done; ++attempt) {
        if (attempt >= max_steps) return fail(-10, "dopri5: max_steps = %d attempted steps exceeded at t = %.9g", max_steps, ctl.t0);
        if (ctl.underflow()) return fail(-11, "dopri5: underflow in dt %g at t = %.17g", ctl.dt, ctl.t0);
        if (int e = dopri5_attempt(r, b, ctl, nv, vrows, atol, rtol)) return e;
        nfe += ode::kStages;
        stats_host[0] = nfe;
        double ratio = 0;
        if (int e = ode_read(c, b, s, &ratio, nullptr)) return e;
        if (!std::isfinite(ratio)) return fail(-9, "dopri5: non-finite error ratio at t = %.9g, dt = %g", ctl.t0, ctl.dt);
        const double t_start = ctl.t0, dt_used = ctl.dt;
        const bool acc = ctl.step(ratio);
        stats_host[1] = ctl.accepted;
        stats_host[2] = ctl.rejected;
        if (!acc) continue;
        if (steps_host) {
            steps_host[2 * (ctl.accepted - 1)] = t_start;
            steps_host[2 * (ctl.accepted - 1) + 1] = dt_used;
        }
        if (ctl.done) {   // dense output of this step at t = 1 into the caller's x (which is b.y0 or b.y1)
            const float dtf = (float)ctl.last_dt;
            if (int e = ode_combine(r, b.ym, b.y0, b.k, ode::kMid, 7, dtf)) return e;
            if (int e = launch(r, "ode_dense", [&] { launch_ode_dense(x, b.y0, b.y1, b.k[0], b.k[6], b.ym, dtf, ctl.dense_s(), (long)r.N * r.D, s); })) return e;
            break;
        }
        std::swap(b.y0, b.y1);   // FSAL: y1 -> y0, k7 -> k1
        std::swap(b.k[0], b.k[6]);
    }
    return 0;
}

// Host-only test hook: the library's controller replayed on given norms.  init = {d0, d1, rms((f1 - k1) / scale)}; ratios[i] is
// the error ratio of attempted step i.  Per attempt i < *n_attempts: t0[i], dt[i] (fp64), the six stage times as fp32 bits
// stage_bits[6 i ..], accept[i].  probe[0..1]: the probe's x0 + h0 k1 coefficient and model time (fp32); *dense_s: s of the dense
// output (when the replay finished).  Returns 0 when an accepted step reached t = 1 within the ratios, 1 when the ratios ran out
// first, or the sampler's error codes (-9 non-finite ratio, -10 more than max_steps attempts, -11 dt underflow).
extern "C" int32_t mdgen_debug_dopri5_controller(const double* init, const double* ratios, int32_t n_ratios, int32_t max_steps,
                                                 float* probe, double* t0, double* dt, uint32_t* stage_bits, int32_t* accept,
                                                 float* dense_s, int32_t* n_attempts) {
    if (!init || (!ratios && n_ratios > 0) || !probe || !t0 || !dt || !stage_bits || !accept || !dense_s || !n_attempts)
        return fail(-1, "null argument");
    Dopri5Ctl ctl;
    ctl.probe(init[0], init[1]);
    probe[0] = ctl.probe_coef();
    probe[1] = ctl.probe_time();
    ctl.first_step(init[1], init[2]);
    *n_attempts = 0;
    for (int i = 0; !ctl.done; ++i) {
        if (i >= max_steps) return fail(-10, "max_steps exceeded");
        if (ctl.underflow()) return fail(-11, "underflow in dt");
        if (i >= n_ratios) return 1;
        t0[i] = ctl.t0;
        dt[i] = ctl.dt;
        float ts[ode::kStages];
        ctl.stage_times(ts);
        std::memcpy(stage_bits + (size_t)ode::kStages * i, ts, sizeof(ts));
        if (!std::isfinite(ratios[i])) return fail(-9, "non-finite error ratio");
        accept[i] = ctl.step(ratios[i]) ? 1 : 0;
        *n_attempts = i + 1;
    }
    *dense_s = ctl.dense_s();
    return 0;
}

// mdgen_debug_dispatch_plan mode 4: one attempted step of mdgen_sample_dopri5 on a made run, in plan mode
static int dopri5_plan(Run& r, int nv) {
    if (nv == 0) return fail(-2, "sample too large for one launch");
    r.no_embed_tail = true;
    float* fake = (float*)4096;   // never dereferenced: plan mode launches nothing
    OdeBufs b;
    b.y0 = b.y1 = b.ym = fake;
    for (int j = 0; j < 7; ++j) b.k[j] = fake;
    b.part = b.out = (double*)fake;
    Dopri5Ctl ctl;
    ctl.dt = 0.01;
    return dopri5_attempt(r, b, ctl, nv, largest_view_rows(r, nv), 1e-6, 1e-3);
}

// ---------------------------------------------------------------------------------------------
// Fixed-grid Runge-Kutta sampling: midpoint, heun3, rk4 on t = linspace(0, 1, S + 1)   (mdgen_sample_rk)
// ---------------------------------------------------------------------------------------------
// The reference's Sampler.sample_ode(sampling_method=...) hands the method name to torchdiffeq (integrators.py:106-113), whose
// fixed-grid solvers (fixed_grid.py Midpoint, Heun3, RK4; rk_common.py rk3_step_func, rk4_alt_step_func -- the 3/8 rule) take one step
// per grid interval.  With fp32 t0 = t[i], t1 = t[i + 1], dt = t1 - t0, f(t, y) = model(y, ones(B) t):
//   midpoint  k1 = f(t0, y0); k2 = f(t0 + 0.5 dt, y0 + k1 (0.5 dt));                               y1 = y0 + dt k2
//   heun3     k1 = f(t0, y0); k2 = f(t0 + dt/3, y0 + dt (k1/3)); k3 = f(t0 + 2 dt/3, y0 + dt (2/3 k2));   y1 = y0 + dt (k1/4 + 3/4 k3)
//   rk4       k1 = f(t0, y0); k2 = f(t0 + dt/3, y0 + (dt k1)/3); k3 = f(t0 + 2 dt/3, y0 + dt (k2 - k1/3));
//             k4 = f(t1, y0 + dt ((k1 - k2) + k3));                                                 y1 = y0 + (((k1 + 3 (k2 + k3)) + k4) dt) / 8
// 1/3 and 2/3 are (float)(1.0 / 3), (float)(2.0 / 3); every written operation is one rounded fp32 operation.  The table below holds
// each state of a step -- the stage inputs and the result -- as an RkForm (kernels.h) with its coefficients: another explicit
// method whose states fit these forms is one more row.
// Every sample sees the same time grid, so a sample's solution does not depend on its batch mates; nothing is read back, so the
// whole solve is one hipGraph; the cost is S x stages network evaluations.
// Orchestration: ONE prepare() for all the call's time rows (a stage at t1 and the next step's first stage share a row: 3 S + 1 rows
// for rk4), then S x stages denoise_step(..., euler = 0) writing k_i through the FinalLayer tail, each starting with k_rk_embed on the
// stage's RkState: stage inputs never reach HBM.  The first stage of step i + 1 forms y1 of step i and stores it over y0 (= the
// caller's x); after the last step k_rk_update does.  Views run one after the other on the caller's stream (plan_views(..., 1)), as
// in mdgen_sample_dopri5: the network launches take kernel forms the dispatch registry covers.
namespace rk {
const float kThird = (float)(1.0 / 3), kTwoThirds = (float)(2.0 / 3);
struct Node {                  // one state of a step
    float a;                   // model time t0 + a dt (0: t0 itself, 1: the grid's t1 itself); a result has none
    int form;                  // RkForm
    int ki[kRkMaxK];           // the stages whose velocities the form reads as k0 .. k3; -1 ends the list
    float c[3];
    bool c0_dt;                // c[0] is multiplied by dt on the host (one rounded fp32 product)
};
struct Method {
    const char* name;
    int stages;
    Node stage[kRkMaxK];       // stage[0] is y0 itself
    Node result;
};
const Method kMethods[] = {
    {"midpoint", 2,
     {{0.f, kRkY0, {-1, -1, -1, -1}, {}, false}, {0.5f, kRkAxk, {0, -1, -1, -1}, {0.5f}, true}},
     {1.f, kRkAxk, {1, -1, -1, -1}, {1.f}, true}},
    {"heun3", 3,
     {{0.f, kRkY0, {-1, -1, -1, -1}, {}, false}, {kThird, kRkDtCk, {0, -1, -1, -1}, {kThird}, false},
      {kTwoThirds, kRkDtCk, {1, -1, -1, -1}, {kTwoThirds}, false}},
     {1.f, kRkDtLin2, {0, 2, -1, -1}, {0.25f, 0.75f}, false}},
    {"rk4", 4,
     {{0.f, kRkY0, {-1, -1, -1, -1}, {}, false}, {kThird, kRkDtkC, {0, -1, -1, -1}, {kThird}, false},
      {kTwoThirds, kRkDtLin2, {1, 0, -1, -1}, {1.f, -kThird}, false}, {1.f, kRkDtLin3, {0, 1, 2, -1}, {1.f, -1.f, 1.f}, false}},
     {1.f, kRk38, {0, 1, 2, 3}, {3.f, 0.125f}, false}},
};
constexpr int kNumMethods = (int)(sizeof(kMethods) / sizeof(kMethods[0]));
}  // namespace rk

// method codes of the C ABI: 1 midpoint, 2 heun3, 3 rk4
static const rk::Method* rk_method(int code) { return code >= 1 && code <= rk::kNumMethods ? &rk::kMethods[code - 1] : nullptr; }

// The prepared time rows of a solve and the row of every (step, stage)
struct RkPlan {
    std::vector<float> tg, rows;
    std::vector<int> row_of;   // [S][stages]
};
static void rk_plan(const rk::Method& m, int S, RkPlan* p) {
#pragma clang fp contract(off)
    linspace01(S + 1, &p->tg);
    p->rows.clear();
    p->row_of.assign((size_t)S * m.stages, 0);
    for (int i = 0; i < S; ++i) {
        const float t0 = p->tg[i], t1 = p->tg[i + 1], dt = t1 - t0;
        for (int j = 0; j < m.stages; ++j) {
            const float a = m.stage[j].a;
            if (j == 0 && i > 0 && m.stage[m.stages - 1].a == 1.f) {   // the previous step's last stage was evaluated at this t0
                p->row_of[(size_t)i * m.stages] = (int)p->rows.size() - 1;
                continue;
            }
            p->row_of[(size_t)i * m.stages + j] = (int)p->rows.size();
            p->rows.push_back(a == 0.f ? t0 : a == 1.f ? t1 : t0 + a * dt);
        }
    }
}

// ---- what a Runge-Kutta call and an SDE call (sde.inc) share: the workspace, the made run, a state's evaluation view by view ----
// the network workspace of `lay`, then `nvel` velocity buffers of one state each
static size_t grid_ws_bytes(const mdgen_ctx* c, const mdgen_shape* sh, const mdgen_ws_layout& lay, int nvel) {
    return align256(lay.total_bytes) + (size_t)nvel * ode_state_bytes(c, sh) + 256;
}
// The made run with the call's conditioning bound, its launch views and the velocity buffers behind the network workspace.
// `lay`: the layout for the call's `rows` time rows; `sizer`: the entry point that sizes the workspace.  Every refusal, the
// caller's and these, comes before make_run, the first to touch the device.
struct GridCall {
    Run r;
    int nv;
    float* vel[kRkMaxK];
};
static int grid_open(GridCall* q, const mdgen_ws_layout& lay, int rows, int nvel, const char* sizer, mdgen_ctx* c, const mdgen_shape* sh,
                     const mdgen_cond& cd, void* ws, size_t ws_bytes, void* stream) {
    const size_t need = grid_ws_bytes(c, sh, lay, nvel);
    if (ws_bytes < need) return fail(-7, "workspace too small: %zu < %zu bytes (%s)", ws_bytes, need, sizer);
    q->r = Run{};
    if (int e = make_run(&q->r, c, sh, rows, 1, f32_path(c), ws, lay.total_bytes, stream)) return e;
    bind_cond(q->r, cd);
    q->r.no_embed_tail = true;
    q->nv = c->opt_precision == 32 ? 1 : plan_views(sh->B, sh->T, sh->L, 1);
    if (q->nv == 0) return fail(-2, "sample too large for one launch");
    for (int j = 0; j < nvel; ++j) q->vel[j] = (float*)((unsigned char*)ws + align256(lay.total_bytes) + (size_t)j * ode_state_bytes(c, sh));
    return 0;
}

// a view's share of a state descriptor: its pointers moved by the view's offset `off` = b0 * per_b floats
static void to_view(Run& v, RkState& s, long off, int, long) {
    s.y += off;
    for (int j = 0; j < s.nk; ++j) s.k[j] += off;
    v.rk = &s;
}
static void to_view(Run& v, SdeState& s, long off, int b0, long per_b) {
    s.y += off;
    for (int j = 0; j < 2; ++j)
        if (s.v[j]) s.v[j] += off;
    if (s.xi) s.xi += off;
    s.b0 = b0;
    s.per_b = (unsigned)per_b;
    v.sde = &s;
}
// one network evaluation of the state `proto` describes (of the whole batch) at time row `row`, the velocity to `out`
template <class State>
static int eval_state(const Run& r, int nv, const State& proto, int row, float* out) {
    const long per_b = (long)r.T * r.L * r.D;
    return for_each_view(r, nv, 1, [&](const Run& v, int b0) {
        const long off = (long)b0 * per_b;
        State st = proto;
        Run vs = v;
        to_view(vs, st, off, b0, per_b);
        return denoise_step(vs, row, st.y, out + off, 0, 0.f, nullptr);
    });
}

// the device descriptor of state `n` of a step of size dt: y and k[stage] of the whole batch
static RkState rk_state_of(const rk::Node& n, float dt, float* y, float* const* k, bool store) {
#pragma clang fp contract(off)
    RkState s{};
    s.form = n.form;
    s.store = store ? 1 : 0;
    s.dt = dt;
    for (int q = 0; q < 3; ++q) s.c[q] = n.c[q];
    if (n.c0_dt) s.c[0] = n.c[0] * dt;
    for (s.nk = 0; s.nk < kRkMaxK && n.ki[s.nk] >= 0; ++s.nk) s.k[s.nk] = k[n.ki[s.nk]];
    s.y = y;
    return s;
}

// the method and the step count alone: judged without a context
static int rk_check(int method, int S) {
    if (!rk_method(method)) return fail(-2, "method: 1 midpoint, 2 heun3, 3 rk4 (got %d)", method);
    if (S < 1) return fail(-2, "n_steps must be >= 1");
    if (S > 100000) return fail(-2, "n_steps too large");
    return 0;
}

static int rk_layout(const mdgen_ctx* c, const mdgen_shape* sh, int method, int S, RkPlan* pl, mdgen_ws_layout* lay) {
    if (int e = rk_check(method, S)) return e;
    rk_plan(*rk_method(method), S, pl);
    return mdgen_workspace_layout(c, sh, (int)pl->rows.size(), 1, lay);
}

extern "C" int32_t mdgen_rk_workspace_bytes(const mdgen_ctx* c, const mdgen_shape* sh, int32_t method, int32_t S, size_t* bytes) {
    if (!bytes) return fail(-1, "null argument");
    RkPlan pl;
    mdgen_ws_layout lay;
    if (int e = rk_layout(c, sh, method, S, &pl, &lay)) return e;
    *bytes = grid_ws_bytes(c, sh, lay, kRkMaxK);
    return 0;
}

// the solve on a made run: y (= the caller's x) in place, k[stage] the velocities
static int rk_body(const Run& r_in, const rk::Method& m, int S, const RkPlan& pl, int nv, float* y, float* const* k) {
    Run r = r_in;
    if (int e = ode_prepare(r, pl.rows.data(), (int)pl.rows.size(), largest_view_rows(r, nv))) return e;
    for (int i = 0; i < S; ++i) {
        const float dt = pl.tg[i + 1] - pl.tg[i], dt_prev = i > 0 ? pl.tg[i] - pl.tg[i - 1] : 0.f;
        for (int j = 0; j < m.stages; ++j) {
            // the first stage of step i > 0 forms the previous step's result and stores it over y
            const bool first = j == 0;
            const rk::Node& n = first && i > 0 ? m.result : m.stage[j];
            const RkState st = rk_state_of(n, first ? dt_prev : dt, y, k, first && i > 0);
            if (int e = eval_state(r, nv, st, pl.row_of[(size_t)i * m.stages + j], k[j])) return e;
        }
    }
    const RkState last = rk_state_of(m.result, pl.tg[S] - pl.tg[S - 1], y, k, true);
    return launch(r, "ode_rk_update", [&] { launch_rk_update(last, (long)r.N * r.D, r.s); });
}

// What mdgen_sample_rk, mdgen_rollout_rk and mdgen_upsample_rk (drivers.inc) share once their own arguments are judged: the plan and the
// GridCall with the four velocity buffers.  `state` is the buffer k_rk_update will see (16-byte accesses).
struct RkCall : GridCall {
    const rk::Method* m;
    RkPlan pl;
    int solve(int S, float* y) const { return rk_body(r, *m, S, pl, nv, y, vel); }
};
static int rk_open(RkCall* q, mdgen_ctx* c, const mdgen_shape* sh, int method, int S, const float* state, const mdgen_cond& cd,
                   void* ws, size_t ws_bytes, void* stream) {
    mdgen_ws_layout lay;
    if (int e = rk_layout(c, sh, method, S, &q->pl, &lay)) return e;
    q->m = rk_method(method);
    if (((uintptr_t)state & 15) != 0) return fail(-7, "x must be 16-byte aligned");
    return grid_open(q, lay, (int)q->pl.rows.size(), kRkMaxK, "mdgen_rk_workspace_bytes", c, sh, cd, ws, ws_bytes, stream);
}

extern "C" int32_t mdgen_sample_rk(mdgen_ctx* c, const mdgen_shape* sh, int32_t method, int32_t S, float* x, const mdgen_cond* cond,
                                   void* ws, size_t ws_bytes, int32_t use_graph, void* stream) {
    if (!x) return fail(-1, "null argument");
    if (int e = check_cond(cond)) return e;
    RkCall q;
    if (int e = rk_open(&q, c, sh, method, S, x, *cond, ws, ws_bytes, stream)) return e;
    GraphKey key = graph_key(3, q.r, *cond);
    key.add(method).add(S).ptr(x);   // (the body does not fork: no n_streams)
    return run_or_replay(q.r, use_graph, key, [&]() { return q.solve(S, x); });
}

// Host-only test hook: the time rows mdgen_sample_rk prepares for (method, S), as fp32 bits, and the row of every (step, stage).
// row_bits: room for cap_rows values; row_of: [S][stages].
extern "C" int32_t mdgen_debug_rk_plan(int32_t method, int32_t S, uint32_t* row_bits, int32_t cap_rows, int32_t* n_rows,
                                       int32_t* row_of, int32_t* n_stages) {
    if (!row_bits || !n_rows || !row_of || !n_stages) return fail(-1, "null argument");
    if (int e = rk_check(method, S)) return e;
    const rk::Method* m = rk_method(method);
    RkPlan pl;
    rk_plan(*m, S, &pl);
    *n_rows = (int32_t)pl.rows.size();
    *n_stages = m->stages;
    if (cap_rows < *n_rows) return fail(-7, "row buffer too small: %d < %d", cap_rows, *n_rows);
    std::memcpy(row_bits, pl.rows.data(), pl.rows.size() * sizeof(float));
    for (size_t i = 0; i < pl.row_of.size(); ++i) row_of[i] = pl.row_of[i];
    return 0;
}

// Test hook: k_rk_embed alone.  State `stage` of a step of `method` with step size dt: 0 is y itself, 1 .. stages - 1 a stage input,
// `stages` the step's result in the storing form (what the next step's first stage launches).  y (B, T, L, D) is the step's y0 (the
// result is stored over it), k0 .. k3 the velocities of stages 1 .. 4 (those the state does not read may be null); ipa_out: [B L][384]
// rows or null; h: [B T L][384].  The context's weights and its abs_pos_emb decide the rest, as in a sampler call.
extern "C" int32_t mdgen_debug_rk_stage(mdgen_ctx* c, const mdgen_shape* sh, int32_t method, int32_t stage, float dt, float* y,
                                        const float* k0, const float* k1, const float* k2, const float* k3, const float* x_cond,
                                        const int64_t* x_cond_mask, const float* ipa_out, float* h, void* stream) {
    if (!y || !x_cond || !x_cond_mask || !h) return fail(-1, "null argument");
    const rk::Method* m = rk_method(method);
    if (!m) return fail(-2, "method: 1 midpoint, 2 heun3, 3 rk4 (got %d)", method);
    if (stage < 0 || stage > m->stages) return fail(-2, "stage must be in 0 .. %d", m->stages);
    if (int e = check_shape(c, sh, 1)) return e;
    if (!c->finalized) return fail(-6, "context not finalized (mdgen_ctx_finalize)");
    float* k[kRkMaxK] = {const_cast<float*>(k0), const_cast<float*>(k1), const_cast<float*>(k2), const_cast<float*>(k3)};
    const rk::Node& n = stage == m->stages ? m->result : m->stage[stage];
    for (int q = 0; q < kRkMaxK && n.ki[q] >= 0; ++q)
        if (!k[n.ki[q]]) return fail(-1, "the state reads k%d", n.ki[q]);
    const RkState st = rk_state_of(n, dt, y, k, stage == m->stages);
    launch_rk_embed(embed_params(c, *sh, y, x_cond, x_cond_mask, ipa_out, h), st, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

// mdgen_debug_dispatch_plan modes 5 .. 7: one step of mdgen_sample_rk (methods 1 .. 3) on a made run, in plan mode
static int rk_dispatch_plan(Run& r, int nv, int method) {
    if (nv == 0) return fail(-2, "sample too large for one launch");
    r.no_embed_tail = true;
    const rk::Method& m = *rk_method(method);
    RkPlan pl;
    rk_plan(m, 1, &pl);
    float* fake = (float*)4096;   // never dereferenced: plan mode launches nothing
    float* k[kRkMaxK] = {fake, fake, fake, fake};
    return rk_body(r, m, 1, pl, nv, fake, k);
}
