// Horn's superposition eigen-solve (Horn 1987, J. Opt. Soc. Am. A 4:629): the largest eigenvalue
// of the 4x4 key matrix of a 3x3 cross-covariance by cyclic Jacobi sweeps.  One solver for the
// whole library: the tracing A-steps take it through tracing_common.h, the conformation report
// (report_conformations.hip) directly.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace igm {

constexpr int kSweeps = 10;           // Jacobi sweeps at most (a 4x4 converges in 4-6)

// one Jacobi rotation of the symmetric 4x4 a on the plane (P, Q); VEC: the rotations are
// accumulated in v, whose column j is then the eigenvector of a[j][j]
template <int P, int Q, bool VEC>
__device__ __forceinline__ void jacobi_rotate(double (&a)[4][4], double (&v)[4][4]) {
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));  // 0 for |theta| = inf
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    a[P][P] -= t * apq;
    a[Q][Q] += t * apq;
    a[P][Q] = a[Q][P] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (VEC) {
            const double vrp = v[r][P], vrq = v[r][Q];
            v[r][P] = c * vrp - s * vrq;
            v[r][Q] = s * vrp + c * vrq;
        }
        if (r == P || r == Q) continue;
        const double arp = a[r][P], arq = a[r][Q];
        a[r][P] = a[P][r] = c * arp - s * arq;
        a[r][Q] = a[Q][r] = s * arp + c * arq;
    }
}

// largest eigenvalue of Horn's key matrix of the cross-covariance m[a][b] = sum p_a x_b (Horn 1987,
// J. Opt. Soc. Am. A 4:629), by cyclic Jacobi sweeps, which take any symmetric matrix (collinear
// and coincident spots included); and (VEC) its unit eigenvector: the quaternion of the proper
// rotation R with x ~ R p (quat is not written otherwise)
template <bool VEC>
__device__ double horn(const double (&m)[3][3], double (&quat)[4]) {
    double a[4][4], v[4][4];
    a[0][0] = m[0][0] + m[1][1] + m[2][2];
    a[1][1] = m[0][0] - m[1][1] - m[2][2];
    a[2][2] = -m[0][0] + m[1][1] - m[2][2];
    a[3][3] = -m[0][0] - m[1][1] + m[2][2];
    a[0][1] = a[1][0] = m[1][2] - m[2][1];
    a[0][2] = a[2][0] = m[2][0] - m[0][2];
    a[0][3] = a[3][0] = m[0][1] - m[1][0];
    a[1][2] = a[2][1] = m[0][1] + m[1][0];
    a[1][3] = a[3][1] = m[2][0] + m[0][2];
    a[2][3] = a[3][2] = m[1][2] + m[2][1];
    if (VEC) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) v[r][q] = r == q ? 1.0 : 0.0;
    }
    for (int sweep = 0; sweep < kSweeps; ++sweep) {
        const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[0][3] * a[0][3] + a[1][2] * a[1][2] +
                           a[1][3] * a[1][3] + a[2][3] * a[2][3];
        const double dia = a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2] + a[3][3] * a[3][3];
        if (off <= 1e-30 * dia) break;  // |error of an eigenvalue| <= sqrt(2 off) (Weyl): 1.4e-15 relative
        jacobi_rotate<0, 1, VEC>(a, v);
        jacobi_rotate<0, 2, VEC>(a, v);
        jacobi_rotate<0, 3, VEC>(a, v);
        jacobi_rotate<1, 2, VEC>(a, v);
        jacobi_rotate<1, 3, VEC>(a, v);
        jacobi_rotate<2, 3, VEC>(a, v);
    }
    double lam = a[0][0];
    int j = 0;
#pragma unroll
    for (int q = 1; q < 4; ++q)
        if (a[q][q] > lam) {
            lam = a[q][q];
            j = q;
        }
    if (VEC) {
#pragma unroll
        for (int r = 0; r < 4; ++r) quat[r] = j == 0 ? v[r][0] : j == 1 ? v[r][1] : j == 2 ? v[r][2] : v[r][3];
        const double inv = 1.0 / sqrt(quat[0] * quat[0] + quat[1] * quat[1] + quat[2] * quat[2] + quat[3] * quat[3]);
#pragma unroll
        for (int r = 0; r < 4; ++r) quat[r] *= inv;
    }
    return lam;
}

}  // namespace igm
