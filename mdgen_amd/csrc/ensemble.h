// ensemble.h -- the rotation of a weighted superposition from its 3 x 3 correlation matrix, in fp64: Horn's 4 x 4 quaternion matrix
// and its largest eigenvector by cyclic Jacobi.  Plain C++ (no HIP type), host and device: k_ensemble.hip runs it on the device,
// and a host program can include it as it stands.
#pragma once
#ifndef __HIPCC__
#ifndef __host__
#define __host__
#define __device__
#endif
#endif

namespace mdg {

constexpr int kHornSweeps = 24;   // cyclic sweeps at the most; a 4 x 4 symmetric matrix is diagonal to fp64 after 5 to 7

// One Jacobi rotation of the symmetric 4 x 4 `a` in the (P, Q) plane, accumulated into the eigenvector columns of `v`.
template <int P, int Q>
__host__ __device__ inline void horn_rotate(double (&a)[4][4], double (&v)[4][4]) {
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    const double at = theta < 0.0 ? -theta : theta;
    // the smaller root of t^2 + 2 theta t - 1 = 0; for |theta| beyond 1e150 theta^2 overflows and t = 1 / (2 theta)
    double t = at > 1e150 ? 0.5 / at : 1.0 / (at + sqrt(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
    a[P][P] -= t * apq;
    a[Q][Q] += t * apq;
    a[P][Q] = 0.0;
    a[Q][P] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r != P && r != Q) {
            const double arp = a[r][P], arq = a[r][Q];
            a[r][P] = arp - s * (arq + tau * arp);
            a[P][r] = a[r][P];
            a[r][Q] = arq + s * (arp - tau * arq);
            a[Q][r] = a[r][Q];
        }
        const double vrp = v[r][P], vrq = v[r][Q];
        v[r][P] = vrp - s * (vrq + tau * vrp);
        v[r][Q] = vrq + s * (vrp - tau * vrq);
    }
}

// R (row-major, det +1) maximising sum_ij R_ij H_ji, i.e. minimising sum w |R a - b|^2 for H = sum w a b^T (H[3 i + j] = sum w a_i b_j).
// Horn 1987: the unit quaternion is the eigenvector of the largest eigenvalue of N(H).  No 3 x 3 SVD and no reflection case: a
// quaternion is a proper rotation whatever det H is.  H = 0 gives the identity.
__host__ __device__ inline void horn_rotation(const double* H, double* R) {
    const double Sxx = H[0], Sxy = H[1], Sxz = H[2], Syx = H[3], Syy = H[4], Syz = H[5], Szx = H[6], Szy = H[7], Szz = H[8];
    double a[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                      {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                      {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                      {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
    double v[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int sweep = 0; sweep < kHornSweeps; ++sweep) {
        const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[0][3] * a[0][3] + a[1][2] * a[1][2] + a[1][3] * a[1][3] +
                           a[2][3] * a[2][3];
        const double dia = a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2] + a[3][3] * a[3][3];
        if (off <= 1e-40 * dia || off == 0.0) break;   // off-diagonal norm below 1e-20 of the diagonal's: far under fp64
        horn_rotate<0, 1>(a, v);
        horn_rotate<0, 2>(a, v);
        horn_rotate<0, 3>(a, v);
        horn_rotate<1, 2>(a, v);
        horn_rotate<1, 3>(a, v);
        horn_rotate<2, 3>(a, v);
    }
    double best = a[0][0], q0 = v[0][0], q1 = v[1][0], q2 = v[2][0], q3 = v[3][0];
#pragma unroll
    for (int c = 1; c < 4; ++c)
        if (a[c][c] > best) {
            best = a[c][c];
            q0 = v[0][c];
            q1 = v[1][c];
            q2 = v[2][c];
            q3 = v[3][c];
        }
    const double inv = 1.0 / sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    q0 *= inv;
    q1 *= inv;
    q2 *= inv;
    q3 *= inv;
    R[0] = q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3;
    R[1] = 2.0 * (q1 * q2 - q0 * q3);
    R[2] = 2.0 * (q1 * q3 + q0 * q2);
    R[3] = 2.0 * (q1 * q2 + q0 * q3);
    R[4] = q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3;
    R[5] = 2.0 * (q2 * q3 - q0 * q1);
    R[6] = 2.0 * (q1 * q3 - q0 * q2);
    R[7] = 2.0 * (q2 * q3 + q0 * q1);
    R[8] = q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3;
}

}  // namespace mdg
