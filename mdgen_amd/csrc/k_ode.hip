// k_ode.hip -- the elementwise side of the adaptive dopri5 sampler (ode.inc): torchdiffeq 0.2.x `dopri5` as the reference's
// transport calls it (transport.py:408-451, integrators.py:74-113).  All of it is HBM-bound over the fp32 state (B, T, L, D):
//   k_ode_combine    y = y0 + sum_j c_j k_j, up to 7 terms (RK stage inputs, y_mid of the dense output, x0 + h0 k1)
//   k_ode_norm_part  per-workgroup fp64 partial sums of the three norm forms (initial step: d0 | d1, d2; the step's error ratio)
//   k_ode_norm_final one workgroup: the partials in a fixed order -> rms = sqrt(sum / n), fp64
//   k_ode_dense      the 4th-order dense output of the last step at s (rk_common.py `_interp_fit` / `_interp_evaluate`)
// No float atomics: the partials are reduced in a fixed order, so two calls with the same inputs give the same bits.
// 16-byte accesses; the caller guarantees 16-byte aligned buffers, n need not be a multiple of 4.
// Every operation is rounded as its own torch op is (no contraction into FMA), except the sums over k_j, which the
// reference evaluates as one matmul (k @ (beta * dt)): those accumulate with fmaf in j order.
#include "kernels.h"

#pragma clang fp contract(off)

namespace mdg {

__global__ __launch_bounds__(256) void k_ode_combine(float* __restrict__ out, const float* __restrict__ y0, OdeTerms p, long n) {
    const long n4 = n >> 2;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n4) {
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int j = 0; j < kOdeMaxTerms; ++j) {
            if (j < p.nk) {
                const float4 k = reinterpret_cast<const float4*>(p.k[j])[i];
                const float c = p.c[j];
                s.x = fmaf(c, k.x, s.x);
                s.y = fmaf(c, k.y, s.y);
                s.z = fmaf(c, k.z, s.z);
                s.w = fmaf(c, k.w, s.w);
            }
        }
        const float4 a = reinterpret_cast<const float4*>(y0)[i];
        reinterpret_cast<float4*>(out)[i] = make_float4(a.x + s.x, a.y + s.y, a.z + s.z, a.w + s.w);
    }
    const long r = (n4 << 2) + i;   // the last n % 4 elements: one thread each
    if (i < (n & 3)) {
        float s = 0.f;
        for (int j = 0; j < p.nk; ++j) s = fmaf(p.c[j], p.k[j][r], s);
        out[r] = y0[r] + s;
    }
}

// contribution of element i to the sums of `mode` (see OdeNorm)
__device__ __forceinline__ void ode_norm_elem(const OdeNorm& p, long i, double& s0, double& s1) {
    const float a = p.a[i], b = p.b[i];
    if (p.mode == 0) {            // scale = atol + |x0| rtol; d0: x0 / scale, d1: k1 / scale
        const double sc = p.atol + (double)fabsf(a) * p.rtol;
        const double u = (double)a / sc, v = (double)b / sc;
        s0 += u * u;
        s1 += v * v;
    } else if (p.mode == 1) {     // d2 (before / h0): (f1 - k1) / scale, f1 - k1 in fp32
        const double sc = p.atol + (double)fabsf(a) * p.rtol;
        const double u = (double)(p.k[0][i] - b) / sc;
        s0 += u * u;
    } else {                      // error ratio: err = sum_j e_j k_j (fp32), tol = atol + rtol max(|y0|, |y1|)
        float e = 0.f;
#pragma unroll
        for (int j = 0; j < kOdeMaxTerms; ++j) e = fmaf(p.e[j], p.k[j][i], e);
        const double tol = p.atol + p.rtol * (double)fmaxf(fabsf(a), fabsf(b));
        const double u = (double)e / tol;
        s0 += u * u;
    }
}

__device__ __forceinline__ double ode_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// fixed slice per workgroup (grid-stride over the element index), fixed tree inside: part[blockIdx][2]
__global__ __launch_bounds__(256) void k_ode_norm_part(OdeNorm p, long n, double* __restrict__ part) {
    __shared__ double red[2][4];
    double s0 = 0.0, s1 = 0.0;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) ode_norm_elem(p, i, s0, s1);
    s0 = ode_wave_sum(s0);
    s1 = ode_wave_sum(s1);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[0][w] = s0;
        red[1][w] = s1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        part[2 * blockIdx.x + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}

__global__ __launch_bounds__(256) void k_ode_norm_final(const double* __restrict__ part, int nparts, long n, double* __restrict__ out) {
    __shared__ double red[2][4];
    double s0 = 0.0, s1 = 0.0;
    for (int i = threadIdx.x; i < nparts; i += blockDim.x) {
        s0 += part[2 * i];
        s1 += part[2 * i + 1];
    }
    s0 = ode_wave_sum(s0);
    s1 = ode_wave_sum(s1);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[0][w] = s0;
        red[1][w] = s1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {   // torch: tensor.abs().pow(2).mean().sqrt()
        out[0] = sqrt(((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) / (double)n);
        out[1] = sqrt(((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) / (double)n);
    }
}

// rk_common.py `_interp_fit` + `_interp_evaluate`, op for op (each line one rounded fp32 op of the reference)
__device__ __forceinline__ float ode_dense_elem(float y0, float y1, float f0, float f1, float ym, float dt, float s) {
    const float a = ((2.f * dt) * (f1 - f0) - 8.f * (y1 + y0)) + 16.f * ym;
    const float b = (((dt * (5.f * f0 - 3.f * f1)) + 18.f * y0) + 14.f * y1) - 32.f * ym;
    const float c = (((dt * (f1 - 4.f * f0)) - 11.f * y0) - 5.f * y1) + 16.f * ym;
    const float d = dt * f0;
    float tot = y0 + s * d;
    float xp = s;
    xp = xp * s;
    tot = tot + xp * c;
    xp = xp * s;
    tot = tot + xp * b;
    xp = xp * s;
    tot = tot + xp * a;
    return tot;
}

__global__ __launch_bounds__(256) void k_ode_dense(float* out, const float* y0, const float* y1, const float* __restrict__ f0,
                                                   const float* __restrict__ f1, const float* __restrict__ ym, float dt, float s, long n) {
    // `out` may alias y0 or y1: every element is read before it is written, by the same thread
    const long n4 = n >> 2;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n4) {
        const float4 a = reinterpret_cast<const float4*>(y0)[i], b = reinterpret_cast<const float4*>(y1)[i];
        const float4 c = reinterpret_cast<const float4*>(f0)[i], d = reinterpret_cast<const float4*>(f1)[i];
        const float4 m = reinterpret_cast<const float4*>(ym)[i];
        reinterpret_cast<float4*>(out)[i] = make_float4(ode_dense_elem(a.x, b.x, c.x, d.x, m.x, dt, s), ode_dense_elem(a.y, b.y, c.y, d.y, m.y, dt, s),
                                                        ode_dense_elem(a.z, b.z, c.z, d.z, m.z, dt, s), ode_dense_elem(a.w, b.w, c.w, d.w, m.w, dt, s));
    }
    const long r = (n4 << 2) + i;
    if (i < (n & 3)) out[r] = ode_dense_elem(y0[r], y1[r], f0[r], f1[r], ym[r], dt, s);
}

static unsigned ode_blocks(long n) {
    const long n4 = n >> 2;
    const long b = (n4 + 255) / 256;
    return (unsigned)(b > 0 ? b : 1);
}

void launch_ode_combine(float* out, const float* y0, const OdeTerms& p, long n, hipStream_t s) {
    hipLaunchKernelGGL(k_ode_combine, dim3(ode_blocks(n)), dim3(256), 0, s, out, y0, p, n);
}

int ode_norm_parts(long n) {
    const long b = (n + 255) / 256;
    return (int)(b < kOdeMaxParts ? b : kOdeMaxParts);
}

void launch_ode_norm(const OdeNorm& p, long n, double* part, double* out, hipStream_t s) {
    const int nb = ode_norm_parts(n);
    hipLaunchKernelGGL(k_ode_norm_part, dim3(nb), dim3(256), 0, s, p, n, part);
    hipLaunchKernelGGL(k_ode_norm_final, dim3(1), dim3(256), 0, s, (const double*)part, nb, n, out);
}

void launch_ode_dense(float* out, const float* y0, const float* y1, const float* f0, const float* f1, const float* ym, float dt,
                      float sfrac, long n, hipStream_t s) {
    hipLaunchKernelGGL(k_ode_dense, dim3(ode_blocks(n)), dim3(256), 0, s, out, y0, y1, f0, f1, ym, dt, sfrac, n);
}

}  // namespace mdg
