// Chromatin tracing A-step for libigmhip (gfx950): the cost of placing every imaged trace on
// every (structure, copy) of the population, and the keep_best cheapest candidates per trace.
//
//   cost     rmsd(t, s, k) = sqrt(max(0, (Ga + Gb - 2 lambda) / n)): the minimum over proper
//            rotations (det = +1) and translations of the distance between the trace's n spots
//            and the beads x_i = xyz[copy_idx[copy_ptr[locus_i] + k], s].  Ga, Gb are the centred
//            sums of squares, lambda the largest eigenvalue of Horn's 4x4 key matrix of the
//            centred cross-covariance (Horn 1987, J. Opt. Soc. Am. A 4:629) -- a quaternion is
//            always a proper rotation, so a mirrored trace does not score 0.  Everything is
//            accumulated in fp64 from the f32 coordinates; lambda comes from cyclic Jacobi
//            sweeps, which take any symmetric matrix (collinear and coincident spots included).
//   select   per trace the keep_best smallest f32 costs over its S * Cmax candidates, ties to the
//            lower candidate index s * Cmax + k: a bitonic sort of (cost bits, index) keys in LDS,
//            and a counting pass once the keys no longer fit.
//
// No atomics anywhere: the result is deterministic.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <limits>
#include <vector>

#include "igm_ctx.h"
#include "tracing_select.h"

namespace {
using namespace igm;

constexpr int kBT = 256;              // threads per workgroup (4 waves of 64)
constexpr int kChunkDefault = 128;    // spots staged in LDS at a time
constexpr int kChunkMax = 1024;
constexpr int kMinSpots = 3;
constexpr int kSortMax = 8192;        // candidates the LDS sort takes (64 KB of 8-byte keys)
constexpr int kCountTile = 2048;      // costs the counting pass holds in LDS at a time
constexpr int kSweeps = 10;           // Jacobi sweeps at most (a 4x4 converges in 4-6)

struct CostArgs {
    const float* xyz;        // (nbead, S, 3)
    int S, Cmax, nsb;        // nsb: blocks of kBT structures
    int chunk;
    const long long* ptr;    // (T + 1) spots of trace t
    const int* ncopy;        // (T) C_t
    const double* ga;        // (T) centred sum of squares of the trace
    const double* pos;       // (n, 3) centred positions
    const int* bead;         // (n, Cmax) bead of spot i in copy k
    float* rmsd;             // (T, S, Cmax)
};

// one Jacobi rotation of the symmetric 4x4 a on the plane (P, Q)
template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(double (&a)[4][4]) {
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
        if (r == P || r == Q) continue;
        const double arp = a[r][P], arq = a[r][Q];
        a[r][P] = a[P][r] = c * arp - s * arq;
        a[r][Q] = a[Q][r] = s * arp + c * arq;
    }
}

// largest eigenvalue of Horn's key matrix of the cross-covariance m[a][b] = sum p_a x_b
__device__ double horn_lambda(const double (&m)[3][3]) {
    double a[4][4];
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
    for (int sweep = 0; sweep < kSweeps; ++sweep) {
        const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[0][3] * a[0][3] + a[1][2] * a[1][2] +
                           a[1][3] * a[1][3] + a[2][3] * a[2][3];
        const double dia = a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2] + a[3][3] * a[3][3];
        if (off <= 1e-30 * dia) break;  // |error of an eigenvalue| <= sqrt(2 off) (Weyl): 1.4e-15 relative
        jacobi_rotate<0, 1>(a);
        jacobi_rotate<0, 2>(a);
        jacobi_rotate<0, 3>(a);
        jacobi_rotate<1, 2>(a);
        jacobi_rotate<1, 3>(a);
        jacobi_rotate<2, 3>(a);
    }
    return fmax(fmax(a[0][0], a[1][1]), fmax(a[2][2], a[3][3]));
}

// One thread per (trace t, copy k, structure s), one block per (t, k, kBT structures): for one
// bead the S structures are contiguous, so a wave reads 768 contiguous bytes per spot.  The
// trace's centred positions and its beads go through LDS in chunks of A.chunk spots.
__global__ void __launch_bounds__(kBT) tracing_cost_kernel(CostArgs A) {
    extern __shared__ double tsm[];
    double* sp = tsm;                                       // (chunk, 3)
    int* sb = reinterpret_cast<int*>(tsm + 3 * A.chunk);    // (chunk)
    const int sblk = blockIdx.x % A.nsb;
    const int tk = blockIdx.x / A.nsb;
    const int k = tk % A.Cmax, t = tk / A.Cmax;
    const int s = sblk * kBT + threadIdx.x;
    const bool live = s < A.S;
    float* out = A.rmsd + ((size_t)t * A.S + (live ? s : 0)) * A.Cmax + k;
    if (k >= A.ncopy[t]) {  // (the whole block)
        if (live) *out = INFINITY;
        return;
    }
    const long long p0 = A.ptr[t];
    const int n = (int)(A.ptr[t + 1] - p0);
    double x0[3] = {0.0, 0.0, 0.0};  // the structure's first bead: the sums run on x - x0
    double sx[3] = {0.0, 0.0, 0.0}, sxx = 0.0;
    double m[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    for (int c0 = 0; c0 < n; c0 += A.chunk) {
        const int nc = min(A.chunk, n - c0);
        __syncthreads();
        for (int i = threadIdx.x; i < nc; i += kBT) {
            const double* p = A.pos + (size_t)(p0 + c0 + i) * 3;
            sp[3 * i] = p[0];
            sp[3 * i + 1] = p[1];
            sp[3 * i + 2] = p[2];
            sb[i] = A.bead[(size_t)(p0 + c0 + i) * A.Cmax + k];
        }
        __syncthreads();
        if (!live) continue;
        if (c0 == 0) {
            const float* q = A.xyz + ((size_t)sb[0] * A.S + s) * 3;
            x0[0] = q[0];
            x0[1] = q[1];
            x0[2] = q[2];
        }
#pragma unroll 4
        for (int i = 0; i < nc; ++i) {
            const float* q = A.xyz + ((size_t)sb[i] * A.S + s) * 3;
            const double x = (double)q[0] - x0[0], y = (double)q[1] - x0[1], z = (double)q[2] - x0[2];
            const double px = sp[3 * i], py = sp[3 * i + 1], pz = sp[3 * i + 2];
            sx[0] += x;
            sx[1] += y;
            sx[2] += z;
            sxx += x * x + y * y + z * z;
            m[0][0] += px * x;
            m[0][1] += px * y;
            m[0][2] += px * z;
            m[1][0] += py * x;
            m[1][1] += py * y;
            m[1][2] += py * z;
            m[2][0] += pz * x;
            m[2][1] += pz * y;
            m[2][2] += pz * z;
        }
    }
    if (!live) return;
    // (the positions are centred, so sum p (x - xbar) = sum p x)
    const double gb = fmax(0.0, sxx - (sx[0] * sx[0] + sx[1] * sx[1] + sx[2] * sx[2]) / n);
    const double lam = horn_lambda(m);
    *out = (float)sqrt(fmax(0.0, (A.ga[t] + gb - 2.0 * lam) / n));
}

// a cost (>= 0 or +inf, never NaN) and its candidate index as one key: unsigned order of the key
// is (cost, index) order
__device__ __forceinline__ unsigned long long cand_key(float v, int i) {
    return ((unsigned long long)__float_as_uint(v) << 32) | (unsigned)i;
}

// keep_best by a bitonic sort of the trace's N keys, padded to npad (a power of two) in LDS
__global__ void __launch_bounds__(kBT) tracing_select_sort_kernel(const float* __restrict__ rmsd, int N, int npad, int kb,
                                                                  int* __restrict__ best_cand,
                                                                  float* __restrict__ best_rmsd) {
    extern __shared__ unsigned long long skey[];
    const int t = blockIdx.x;
    const float* v = rmsd + (size_t)t * N;
    for (int i = threadIdx.x; i < npad; i += kBT) skey[i] = i < N ? cand_key(v[i], i) : ~0ull;
    __syncthreads();
    for (int k = 2; k <= npad; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < npad; i += kBT) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long a = skey[i], b = skey[l];
                    if ((a > b) == ((i & k) == 0)) {
                        skey[i] = b;
                        skey[l] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    for (int r = threadIdx.x; r < kb; r += kBT) {
        const unsigned long long key = skey[r];
        best_cand[(size_t)t * kb + r] = (int)(unsigned)(key & 0xffffffffull);
        best_rmsd[(size_t)t * kb + r] = __uint_as_float((unsigned)(key >> 32));
    }
}

// keep_best by counting every candidate's rank against the whole row, the row passing through
// LDS in tiles: the fallback for rows whose keys do not fit LDS
__global__ void __launch_bounds__(kBT) tracing_select_count_kernel(const float* __restrict__ rmsd, int N, int kb,
                                                                   int* __restrict__ best_cand,
                                                                   float* __restrict__ best_rmsd) {
    __shared__ float tile[kCountTile];
    const int t = blockIdx.x;
    const float* v = rmsd + (size_t)t * N;
    for (int g = 0; g < N; g += kBT) {
        const int i = g + threadIdx.x;
        const float x = i < N ? v[i] : INFINITY;
        int r = 0;
        for (int t0 = 0; t0 < N; t0 += kCountTile) {
            const int nt = min(kCountTile, N - t0);
            __syncthreads();
            for (int q = threadIdx.x; q < nt; q += kBT) tile[q] = v[t0 + q];
            __syncthreads();
            if (i < N && r < kb)
                for (int q = 0; q < nt; ++q) {
                    const float y = tile[q];
                    r += (y < x) | ((y == x) & (t0 + q < i));
                }
        }
        if (i < N && r < kb) {
            best_cand[(size_t)t * kb + r] = i;
            best_rmsd[(size_t)t * kb + r] = x;
        }
    }
}

int pow2_at_least(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

}  // namespace

int igm::tracing_select(igm_ctx* c, const float* cost, int rows, int N, int kb, int* best_cand, float* best_cost) {
    if (N <= kSortMax) {
        const int npad = pow2_at_least(N);
        hipLaunchKernelGGL(tracing_select_sort_kernel, dim3((unsigned)rows), dim3(kBT),
                           (size_t)npad * sizeof(unsigned long long), c->stream, cost, N, npad, kb, best_cand, best_cost);
    } else {
        hipLaunchKernelGGL(tracing_select_count_kernel, dim3((unsigned)rows), dim3(kBT), 0, c->stream, cost, N, kb,
                           best_cand, best_cost);
    }
    IGM_HIP_CHECK(c, hipGetLastError());
    return IGM_OK;
}

extern "C" int igm_tracing_assign(igm_ctx* c, uint32_t flags, const float* xyz, int32_t nbead, int32_t nstruct,
                                  const int32_t* copy_ptr, const int32_t* copy_idx, int32_t nhap, int32_t ntrace,
                                  const int64_t* trace_ptr, const int32_t* locus, const float* position,
                                  int32_t keep_best, float* rmsd_out, int32_t* best_cand, float* best_rmsd) {
    if (!c) return IGM_E_INVALID;
    if (nbead <= 0 || nstruct <= 0 || nhap <= 0 || ntrace < 0 || !xyz || !copy_ptr || !copy_idx || !trace_ptr ||
        !best_cand || !best_rmsd)
        return fail(c, IGM_E_INVALID, "igm_tracing_assign: invalid arguments");
    if (keep_best < 1) return fail(c, IGM_E_INVALID, "igm_tracing_assign: keep_best %d must be >= 1", keep_best);
    if (flags & IGM_DEVICE_PTRS)
        return fail(c, IGM_E_UNSUPPORTED, "igm_tracing_assign: host arrays expected (validated on the host)");
    IGM_HIP_CHECK(c, hipSetDevice(c->device));
    if (ntrace == 0) return IGM_OK;
    // host validation: the kernels trust the tables built here
    if (copy_ptr[0] != 0) return fail(c, IGM_E_INVALID, "igm_tracing_assign: copy_ptr[0] = %d, not 0", copy_ptr[0]);
    for (int h = 0; h < nhap; ++h)
        if (copy_ptr[h + 1] <= copy_ptr[h])
            return fail(c, IGM_E_INVALID, "igm_tracing_assign: locus %d has no copies", h);
    for (int q = 0; q < copy_ptr[nhap]; ++q)
        if (copy_idx[q] < 0 || copy_idx[q] >= nbead)
            return fail(c, IGM_E_INVALID, "igm_tracing_assign: bead %d outside [0, %d)", copy_idx[q], nbead);
    if (trace_ptr[0] != 0)
        return fail(c, IGM_E_INVALID, "igm_tracing_assign: trace_ptr[0] = %lld, not 0", (long long)trace_ptr[0]);
    for (int t = 0; t < ntrace; ++t) {
        if (trace_ptr[t + 1] < trace_ptr[t])
            return fail(c, IGM_E_INVALID, "igm_tracing_assign: trace_ptr is not monotone at trace %d", t);
        if (trace_ptr[t + 1] - trace_ptr[t] < kMinSpots)
            return fail(c, IGM_E_INVALID, "igm_tracing_assign: trace %d has %lld spots, fewer than %d", t,
                        (long long)(trace_ptr[t + 1] - trace_ptr[t]), kMinSpots);
        if (trace_ptr[t + 1] - trace_ptr[t] > 0x7fffffff)
            return fail(c, IGM_E_UNSUPPORTED, "igm_tracing_assign: trace %d has too many spots", t);
    }
    const int64_t nspot = trace_ptr[ntrace];
    if (!locus || !position) return fail(c, IGM_E_INVALID, "igm_tracing_assign: locus or position is NULL");
    std::vector<int> ncopy(ntrace);
    std::vector<double> ga(ntrace), pos((size_t)nspot * 3);
    int Cmax = 1;
    int64_t cand_min = std::numeric_limits<int64_t>::max();
    for (int t = 0; t < ntrace; ++t) {
        const int64_t p0 = trace_ptr[t], p1 = trace_ptr[t + 1];
        double mean[3] = {0.0, 0.0, 0.0};
        for (int64_t i = p0; i < p1; ++i) {
            const int h = locus[i];
            if (h < 0 || h >= nhap)
                return fail(c, IGM_E_INVALID, "igm_tracing_assign: trace %d: locus %d outside [0, %d)", t, h, nhap);
            if (i > p0 && h <= locus[i - 1])
                return fail(c, IGM_E_INVALID, "igm_tracing_assign: trace %d: loci are not increasing", t);
            const int nc = copy_ptr[h + 1] - copy_ptr[h];
            // (the loci of one chromosome have one copy count; the chromosome table itself is the
            // caller's, igm_amd.tracing.read_traces)
            if (i > p0 && nc != ncopy[t])
                return fail(c, IGM_E_INVALID, "igm_tracing_assign: trace %d: loci of more than one chromosome "
                            "(copy counts %d and %d)", t, ncopy[t], nc);
            ncopy[t] = nc;
            for (int d = 0; d < 3; ++d) {
                if (!std::isfinite(position[i * 3 + d]))
                    return fail(c, IGM_E_INVALID, "igm_tracing_assign: trace %d: non-finite position", t);
                mean[d] += (double)position[i * 3 + d];
            }
        }
        const double n = (double)(p1 - p0);
        double g = 0.0;
        for (int64_t i = p0; i < p1; ++i)
            for (int d = 0; d < 3; ++d) {
                const double v = (double)position[i * 3 + d] - mean[d] / n;
                pos[(size_t)i * 3 + d] = v;
                g += v * v;
            }
        ga[t] = g;
        Cmax = std::max(Cmax, ncopy[t]);
        cand_min = std::min(cand_min, (int64_t)nstruct * ncopy[t]);
    }
    if (keep_best > cand_min)
        return fail(c, IGM_E_INVALID, "igm_tracing_assign: keep_best %d exceeds the %lld candidates of a trace",
                    keep_best, (long long)cand_min);
    const int64_t N64 = (int64_t)nstruct * Cmax;
    const int nsb = (int)ceil_div(nstruct, kBT);
    if (N64 > 0x7fffffff || (int64_t)ntrace * Cmax * nsb > 0x7fffffff)
        return fail(c, IGM_E_UNSUPPORTED, "igm_tracing_assign: grid too large");
    const int N = (int)N64;
    std::vector<int> bead((size_t)nspot * Cmax, 0);
    for (int t = 0; t < ntrace; ++t)
        for (int64_t i = trace_ptr[t]; i < trace_ptr[t + 1]; ++i)
            for (int k = 0; k < ncopy[t]; ++k) bead[(size_t)i * Cmax + k] = copy_idx[copy_ptr[locus[i]] + k];
    int chunk = kChunkDefault;
    if (const char* e = getenv("IGM_TRACING_CHUNK")) chunk = std::min(kChunkMax, std::max(1, atoi(e)));  // (tests)

    const float* d_xyz;
    const int64_t* d_ptr;
    const int* d_nc;
    const int* d_bead;
    const double *d_ga, *d_pos;
    IGM_TRY(to_device(c, flags, "tr_xyz", xyz, (size_t)nbead * nstruct * 3, &d_xyz));
    IGM_TRY(to_device(c, flags, "tr_ptr", trace_ptr, (size_t)ntrace + 1, &d_ptr));
    IGM_TRY(to_device(c, flags, "tr_nc", (const int*)ncopy.data(), ncopy.size(), &d_nc));
    IGM_TRY(to_device(c, flags, "tr_bead", (const int*)bead.data(), bead.size(), &d_bead));
    IGM_TRY(to_device(c, flags, "tr_ga", (const double*)ga.data(), ga.size(), &d_ga));
    IGM_TRY(to_device(c, flags, "tr_pos", (const double*)pos.data(), pos.size(), &d_pos));
    void* p_rmsd;
    IGM_TRY(workspace(c, "tr_rmsd", (size_t)ntrace * N * sizeof(float), &p_rmsd));
    int32_t* d_bc = nullptr;
    float* d_bv = nullptr;
    const size_t nb = (size_t)ntrace * keep_best;
    IGM_TRY(out_device(c, flags, "tr_bc", best_cand, nb, &d_bc));
    IGM_TRY(out_device(c, flags, "tr_bv", best_rmsd, nb, &d_bv));
    CostArgs A;
    A.xyz = d_xyz;
    A.S = nstruct;
    A.Cmax = Cmax;
    A.nsb = nsb;
    A.chunk = chunk;
    A.ptr = reinterpret_cast<const long long*>(d_ptr);
    A.ncopy = d_nc;
    A.ga = d_ga;
    A.pos = d_pos;
    A.bead = d_bead;
    A.rmsd = (float*)p_rmsd;
    {
        Timed all(c, "tracing_assign");
        {
            Timed tm(c, "tracing_cost");
            hipLaunchKernelGGL(tracing_cost_kernel, dim3((unsigned)((int64_t)ntrace * Cmax * nsb)), dim3(kBT),
                               (size_t)chunk * (3 * sizeof(double) + sizeof(int)), c->stream, A);
            IGM_HIP_CHECK(c, hipGetLastError());
        }
        {
            Timed tm(c, "tracing_select");
            IGM_TRY(tracing_select(c, (const float*)p_rmsd, ntrace, N, keep_best, d_bc, d_bv));
        }
    }
    IGM_TRY(to_host(c, flags, rmsd_out, (const float*)p_rmsd, (size_t)ntrace * N));
    IGM_TRY(to_host(c, flags, best_cand, (const int32_t*)d_bc, nb));
    IGM_TRY(to_host(c, flags, best_rmsd, (const float*)d_bv, nb));
    return finish(c, flags);  // (synchronises: the host tables above outlive their copies)
}
