// Chromatin tracing A-step for libigmhip (gfx950): the cost of placing every imaged trace on
// every (structure, copy) of the population, and the keep_best cheapest candidates per trace.
//
//   cost     rmsd(t, s, k) = sqrt(max(0, (Ga + Gb - 2 lambda) / n)): the minimum over proper
//            rotations (det = +1) and translations of the distance between the trace's n spots
//            and the beads x_i = xyz[copy_idx[copy_ptr[locus_i] + k], s].  Ga, Gb are the centred
//            sums of squares, lambda the largest eigenvalue of Horn's 4x4 key matrix of the
//            centred cross-covariance (Horn 1987, J. Opt. Soc. Am. A 4:629) -- a quaternion is
//            always a proper rotation, so a mirrored trace does not score 0.  Everything is
//            accumulated in fp64 from the f32 coordinates; the sums and the eigen-solve are the
//            ones igm_tracing_assign_cells uses too (tracing_common.h).
//   select   per trace the keep_best smallest f32 costs over its S * Cmax candidates, ties to the
//            lower candidate index s * Cmax + k: a bitonic sort of (cost bits, index) keys in LDS,
//            and a counting pass once the keys no longer fit.
//
// No atomics anywhere: the result is deterministic.
#include <hip/hip_runtime.h>

#include <limits>

#include "tracing_common.h"
#include "tracing_select.h"

namespace {
using namespace igm;

constexpr int kSortMax = 8192;        // candidates the LDS sort takes (64 KB of 8-byte keys)
constexpr int kCountTile = 2048;      // costs the counting pass holds in LDS at a time

struct CostArgs : SpotArgs {
    const double* ga;        // (T) centred sum of squares of the trace
    float* rmsd;             // (T, S, Cmax)
};

// One thread per (trace t, copy k, structure s), one block per (t, k, kBT structures): the sums of
// spot_sums (tracing_common.h) on the positions centred on the trace, solved in place.  Held to 8
// waves per SIMD (64 VGPRs): left to itself the scheduler clusters the four unrolled loads of the
// sums, as it does in tracing_cell_sums_kernel, and the kernel drops to occupancy 5.
__global__ void __launch_bounds__(kBT, 8) tracing_cost_kernel(CostArgs A) {
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
    double x0[3] = {0.0, 0.0, 0.0};  // the bead of the trace's first spot: the sums run on x - x0
    if (live) {
        const float* q = A.xyz + ((size_t)A.bead[(size_t)p0 * A.Cmax + k] * A.S + s) * 3;
        x0[0] = q[0];
        x0[1] = q[1];
        x0[2] = q[2];
    }
    double sx[3], sxx, m[3][3], unused[4];
    spot_sums(A, t, k, s, live, x0, sx, sxx, m);  // (block-collective: no thread has left)
    if (!live) return;
    // (the positions are centred, so sum p (x - xbar) = sum p x)
    const double gb = fmax(0.0, sxx - (sx[0] * sx[0] + sx[1] * sx[1] + sx[2] * sx[2]) / n);
    const double lam = horn<false>(m, unused);
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
    std::vector<int> ncopy, bead;
    IGM_TRY(check_traces(c, "igm_tracing_assign", nbead, copy_ptr, copy_idx, nhap, ntrace, trace_ptr, locus, position,
                         locus && position ? nullptr : "locus or position", &ncopy));
    // the positions centred on their trace
    std::vector<double> ga(ntrace), pos((size_t)trace_ptr[ntrace] * 3);
    int Cmax = 1;
    int64_t cand_min = std::numeric_limits<int64_t>::max();
    for (int t = 0; t < ntrace; ++t) {
        const int64_t p0 = trace_ptr[t], p1 = trace_ptr[t + 1];
        double mean[3] = {0.0, 0.0, 0.0};
        for (int64_t i = p0; i < p1; ++i)
            for (int d = 0; d < 3; ++d) mean[d] += (double)position[i * 3 + d];
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
    const int chunk = bead_table(copy_ptr, copy_idx, ntrace, trace_ptr, locus, ncopy, Cmax, &bead);

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
