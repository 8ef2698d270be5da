// k_pdb.hip -- multi-model PDB text of a sampled trajectory, formatted on the device (mdgen_pdb_format; the bytes of
// mdgen_amd/pdb.py frames_to_pdb_string).  The format is fixed-width: a frame's size follows from its atom count and the digits
// of its model index, and the only arithmetic is %8.3f.  Everything that depends on a name arrives in host-built record
// templates; the kernels know no residue or atom names.
//   k_pdb_count    one wave per frame: present atoms -> the frame's byte size (into offsets[m + 1]); fields that overflow -> status[0]
//   k_pdb_scan     one workgroup: sizes -> offsets[0 .. M] (int64), status[1] = offsets[M]
//   k_pdb_format   one wave per frame: MODEL line, one record per present atom (a lane owns a slot of a 64-slot chunk, its serial
//                  is a prefix over the chunk's ballot), TER, ENDMDL.  Writes nothing when status[0] > 0 or the text does not fit.
// Plain byte stores: a frame never starts on a 4-byte boundary by rule (headers vary in length), and the text rate the sampler
// needs (0.4 GB/s at the headline shape) is two orders below what these reach; the file write dominates.
#include "kernels.h"

namespace mdg {

constexpr int kPdbRec = 81;        // an 80-column record + '\n'
constexpr int kPdbWaves = 4;       // frames per workgroup
constexpr int kPdbMaxSerial = 99999;

struct PdbIn {
    const float* atom14;           // [M][L][14][3]
    const int64_t* aatype;         // [L]
    const int64_t* a37to14;        // [21][37]
    const float* a37mask;          // [21][37]
    int L;
};

// Slot s = residue * 37 + atom37 index of frame `fr`: the gathered, masked position (geometry.py atom14_to_atom37) and whether
// the atom is present -- (|x| + |y|) + |z| > 1e-7f in fp32, what np.abs(a37).sum(-1) > 1e-7 computes (utils.py:77).  `bad`:
// coordinates that have no %8.3f field (not finite, or n = rint(1000 x) outside -999999 .. 9999999); a residue type or table
// entry out of range counts as one and the slot as absent, so that nothing is read out of bounds.
__device__ __forceinline__ bool pdb_slot(const PdbIn& p, const float* fr, int s, float* v, int* bad) {
    *bad = 0;
    if (s >= p.L * 37) return false;
    const int i = s / 37, k = s - i * 37;
    const int64_t aa = p.aatype[i];
    if ((uint64_t)aa > 20u) {
        *bad = 1;
        return false;
    }
    const int64_t j = p.a37to14[aa * 37 + k];
    if ((uint64_t)j > 13u) {
        *bad = 1;
        return false;
    }
    const float m = p.a37mask[aa * 37 + k];
    const float* a = fr + ((long)i * 14 + j) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        v[c] = a[c] * m;
        const double n = __builtin_rint((double)v[c] * 1000.0);   // exact product (24 + 10 bits), ties to even: Python's rounding
        *bad += !(n >= -999999.0 && n <= 9999999.0);              // false for NaN and inf too
    }
    return (fabsf(v[0]) + fabsf(v[1])) + fabsf(v[2]) > 1e-7f;
}

__device__ __forceinline__ int pdb_digits(unsigned long long v) {
    int d = 1;
    while (v >= 10) {
        v /= 10;
        ++d;
    }
    return d;
}

__global__ __launch_bounds__(64 * kPdbWaves) void k_pdb_count(PdbIn p, long M, long model_base, int64_t* __restrict__ offsets,
                                                              int64_t* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int slots = p.L * 37;
    for (long m = (long)blockIdx.x * kPdbWaves + (threadIdx.x >> 6); m < M; m += (long)gridDim.x * kPdbWaves) {
        const float* fr = p.atom14 + m * p.L * 42;
        int n = 0, bad = 0;
        for (int s0 = 0; s0 < slots; s0 += 64) {
            float v[3];
            int b;
            const bool present = pdb_slot(p, fr, s0 + lane, v, &b);
            n += __popcll(__ballot(present));
            bad += b;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
        bad += n + 1 > kPdbMaxSerial;   // the TER record's serial has five columns
        if (lane == 0) {
            offsets[m + 1] = 6 + pdb_digits((unsigned long long)(model_base + m)) + 1 + (long)kPdbRec * (n + 1) + 7;
            if (bad) atomicAdd((unsigned long long*)status, (unsigned long long)bad);
        }
    }
}

// offsets[1 .. M] hold the frame sizes on entry; inclusive scan in place, offsets[0] = 0: offsets[m] is where frame m starts.
__global__ __launch_bounds__(1024) void k_pdb_scan(long M, int64_t* __restrict__ offsets, int64_t* __restrict__ status) {
    __shared__ int64_t wsum[16];
    __shared__ int64_t carry_s;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (long base = 0; base < M; base += 1024) {
        const long m = base + threadIdx.x;
        int64_t x = m < M ? offsets[m + 1] : 0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int64_t y = __shfl_up(x, o);
            if (lane >= o) x += y;
        }
        if (lane == 63) wsum[w] = x;
        __syncthreads();
        int64_t pre = carry_s;
        for (int u = 0; u < w; ++u) pre += wsum[u];
        if (m < M) offsets[m + 1] = pre + x;
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = pre + x;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        offsets[0] = 0;
        status[1] = carry_s;
    }
}

// v right-aligned in out[0 .. width): decimal digits, blanks in front
__device__ __forceinline__ void pdb_put_uint(uint8_t* out, int width, unsigned v) {
    for (int c = width - 1; c >= 0; --c) {
        out[c] = (v || c == width - 1) ? (uint8_t)('0' + v % 10) : (uint8_t)' ';
        v /= 10;
    }
}

// Python's f"{x:>8.3f}" for a coordinate that fits: |n| / 1000, '.', |n| % 1000 as three digits, '-' when signbit(x)
__device__ __forceinline__ void pdb_put_coord(uint8_t* out, float x) {
    const double n = __builtin_rint((double)x * 1000.0);
    unsigned a = (unsigned)fabs(n);
    out[7] = (uint8_t)('0' + a % 10);
    a /= 10;
    out[6] = (uint8_t)('0' + a % 10);
    a /= 10;
    out[5] = (uint8_t)('0' + a % 10);
    a /= 10;
    out[4] = '.';
    int c = 3;
    do {
        out[c--] = (uint8_t)('0' + a % 10);
        a /= 10;
    } while (a && c >= 0);
    if (__builtin_signbit(x) && c >= 0) out[c--] = '-';
    while (c >= 0) out[c--] = ' ';
}

__global__ __launch_bounds__(64 * kPdbWaves) void k_pdb_format(PdbIn p, long M, long model_base,
                                                               const uint8_t* __restrict__ templates,
                                                               const uint8_t* __restrict__ ter_template,
                                                               const int64_t* __restrict__ offsets, uint8_t* __restrict__ text,
                                                               long text_capacity, const int64_t* __restrict__ status) {
    if (status[0] > 0 || offsets[M] > text_capacity) return;
    const int lane = threadIdx.x & 63;
    const int slots = p.L * 37;
    for (long m = (long)blockIdx.x * kPdbWaves + (threadIdx.x >> 6); m < M; m += (long)gridDim.x * kPdbWaves) {
        const float* fr = p.atom14 + m * p.L * 42;
        const long end = offsets[m + 1];   // <= offsets[M] <= text_capacity: every store below stays in front of it
        const unsigned long long idx = (unsigned long long)(model_base + m);
        const int nd = pdb_digits(idx);
        uint8_t* q = text + offsets[m];
        if (lane == 0 && offsets[m] + 7 + nd <= end) {
            const char* h = "MODEL ";
            for (int c = 0; c < 6; ++c) q[c] = (uint8_t)h[c];
            unsigned long long v = idx;
            for (int c = nd - 1; c >= 0; --c) {
                q[6 + c] = (uint8_t)('0' + v % 10);
                v /= 10;
            }
            q[6 + nd] = '\n';
        }
        q += 7 + nd;
        int n = 0;   // present atoms in front of this chunk
        for (int s0 = 0; s0 < slots; s0 += 64) {
            float v[3];
            int b;
            const bool present = pdb_slot(p, fr, s0 + lane, v, &b);
            const unsigned long long bal = __ballot(present);
            const int rank = n + __popcll(bal & ((1ull << lane) - 1));   // serial - 1
            uint8_t* r = q + (long)rank * kPdbRec;
            if (present && r + kPdbRec <= text + end) {
                const uint8_t* t = templates + (long)(s0 + lane) * kPdbRec;
                for (int c = 0; c < kPdbRec; ++c) r[c] = t[c];
                pdb_put_uint(r + 6, 5, (unsigned)(rank + 1));
                pdb_put_coord(r + 30, v[0]);
                pdb_put_coord(r + 38, v[1]);
                pdb_put_coord(r + 46, v[2]);
            }
            n += __popcll(bal);
        }
        uint8_t* r = q + (long)n * kPdbRec;
        if (r + kPdbRec + 7 <= text + end) {
            uint8_t ser[5];
            pdb_put_uint(ser, 5, (unsigned)(n + 1));
            for (int c = lane; c < kPdbRec; c += 64) r[c] = (c >= 6 && c < 11) ? ser[c - 6] : ter_template[c];
            const char* e = "ENDMDL\n";
            if (lane < 7) r[kPdbRec + lane] = (uint8_t)e[lane];
        }
    }
}

void launch_pdb_format(long M, int L, long model_base, const float* atom14, const int64_t* aatype, const int64_t* a37to14,
                       const float* a37mask, const uint8_t* templates, const uint8_t* ter_template, int64_t* offsets,
                       uint8_t* text, long text_capacity, int64_t* status, hipStream_t s) {
    const PdbIn p{atom14, aatype, a37to14, a37mask, L};
    const long want = (M + kPdbWaves - 1) / kPdbWaves;
    const unsigned grid = (unsigned)(want < (1l << 20) ? want : (1l << 20));   // beyond that a wave walks several frames
    // status[0] is zero on entry (the caller's memset on `s`): k_pdb_count adds to it
    hipLaunchKernelGGL(k_pdb_count, dim3(grid), dim3(64 * kPdbWaves), 0, s, p, M, model_base, offsets, status);
    hipLaunchKernelGGL(k_pdb_scan, dim3(1), dim3(1024), 0, s, M, offsets, status);
    hipLaunchKernelGGL(k_pdb_format, dim3(grid), dim3(64 * kPdbWaves), 0, s, p, M, model_base, templates, ter_template, offsets,
                       text, text_capacity, status);
}

}  // namespace mdg
