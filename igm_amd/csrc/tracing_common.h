// The superposition core of the chromatin tracing A-steps, shared by tracing_assign.hip (a trace on
// its own) and tracing_cells.hip (the traces of an imaged cell jointly): the 13 fp64 sums of a
// trace on one copy of its chromosome, Horn's 4x4 eigen-solve (horn.h), and the host validation and
// tables both entries start from.  Included by those two translation units only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "horn.h"
#include "igm_ctx.h"

namespace igm {

constexpr int kBT = 256;              // threads per workgroup (4 waves of 64)
constexpr int kChunkDefault = 128;    // spots staged in LDS at a time
constexpr int kChunkMax = 1024;
constexpr int kMinSpots = 3;

// what the kernels that call spot_sums take (tracing_cost_kernel, tracing_cell_sums_kernel)
struct SpotArgs {
    const float* xyz;        // (nbead, S, 3)
    int S, Cmax, nsb;        // nsb: blocks of kBT structures
    int chunk;
    const long long* ptr;    // (T + 1) spots of trace t
    const int* ncopy;        // (T) C_t
    const double* pos;       // (n, 3) centred positions (on the trace, or on its cell)
    const int* bead;         // (n, Cmax) bead of spot i in copy k
};

// The sums of trace t on copy k in structure s: sx = sum x_i, sxx = sum |x_i|^2, m[a][b] = sum p_a x_b,
// p_i the centred position of spot i and x_i its bead minus x0, a bead of the structure near the
// trace, so that the nucleus-scale offset does not enter the cancellation of Gb = sxx - |sx|^2 / n.
// One thread per structure, one block per (t, k, kBT structures): for one bead the S structures are
// contiguous, so a wave reads 768 contiguous bytes per spot.  The trace's positions and its beads
// go through dynamic LDS (28 B per spot) in chunks of A.chunk spots.
// BLOCK-COLLECTIVE: two __syncthreads() per chunk.  Every thread of the block calls it, with the
// block's (t, k); a thread with s >= S passes live = false, takes the barriers and skips only the
// arithmetic.  The only return a kernel may take before the call is one the whole block takes.
__device__ __forceinline__ void spot_sums(const SpotArgs& A, int t, int k, int s, bool live, const double (&x0)[3],
                                          double (&sx)[3], double& sxx, double (&m)[3][3]) {
    extern __shared__ double tsm[];
    double* sp = tsm;                                       // (chunk, 3)
    int* sb = reinterpret_cast<int*>(tsm + 3 * A.chunk);    // (chunk)
    const long long p0 = A.ptr[t];
    const int n = (int)(A.ptr[t + 1] - p0);
    sx[0] = sx[1] = sx[2] = sxx = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) m[a][0] = m[a][1] = m[a][2] = 0.0;
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
}

// Host validation of an entry's trace arrays; the kernels trust the tables built from them.  who:
// the entry's name, the prefix of every message; missing: what to call a NULL among the entry's
// per-spot arrays, nullptr when none is.  Fills ncopy (T): the copies of every trace's chromosome.
inline int check_traces(igm_ctx* c, const char* who, int nbead, const int32_t* copy_ptr, const int32_t* copy_idx,
                        int nhap, int ntrace, const int64_t* trace_ptr, const int32_t* locus, const float* position,
                        const char* missing, std::vector<int>* ncopy) {
    if (copy_ptr[0] != 0) return fail(c, IGM_E_INVALID, "%s: copy_ptr[0] = %d, not 0", who, copy_ptr[0]);
    for (int h = 0; h < nhap; ++h)
        if (copy_ptr[h + 1] <= copy_ptr[h]) return fail(c, IGM_E_INVALID, "%s: locus %d has no copies", who, h);
    for (int q = 0; q < copy_ptr[nhap]; ++q)
        if (copy_idx[q] < 0 || copy_idx[q] >= nbead)
            return fail(c, IGM_E_INVALID, "%s: bead %d outside [0, %d)", who, copy_idx[q], nbead);
    if (trace_ptr[0] != 0)
        return fail(c, IGM_E_INVALID, "%s: trace_ptr[0] = %lld, not 0", who, (long long)trace_ptr[0]);
    for (int t = 0; t < ntrace; ++t) {
        const long long n = trace_ptr[t + 1] - trace_ptr[t];
        if (n < 0) return fail(c, IGM_E_INVALID, "%s: trace_ptr is not monotone at trace %d", who, t);
        if (n < kMinSpots)
            return fail(c, IGM_E_INVALID, "%s: trace %d has %lld spots, fewer than %d", who, t, n, kMinSpots);
        if (n > 0x7fffffff) return fail(c, IGM_E_UNSUPPORTED, "%s: trace %d has too many spots", who, t);
    }
    if (missing) return fail(c, IGM_E_INVALID, "%s: %s is NULL", who, missing);
    ncopy->assign(ntrace, 0);
    for (int t = 0; t < ntrace; ++t)
        for (int64_t i = trace_ptr[t]; i < trace_ptr[t + 1]; ++i) {
            const int h = locus[i];
            if (h < 0 || h >= nhap)
                return fail(c, IGM_E_INVALID, "%s: trace %d: locus %d outside [0, %d)", who, t, h, nhap);
            if (i > trace_ptr[t] && h <= locus[i - 1])
                return fail(c, IGM_E_INVALID, "%s: trace %d: loci are not increasing", who, t);
            const int nc = copy_ptr[h + 1] - copy_ptr[h];
            // (the loci of one chromosome have one copy count; the chromosome table itself is the
            // caller's, igm_amd.tracing.read_traces)
            if (i > trace_ptr[t] && nc != (*ncopy)[t])
                return fail(c, IGM_E_INVALID, "%s: trace %d: loci of more than one chromosome (copy counts %d and %d)",
                            who, t, (*ncopy)[t], nc);
            (*ncopy)[t] = nc;
            for (int d = 0; d < 3; ++d)
                if (!std::isfinite(position[i * 3 + d]))
                    return fail(c, IGM_E_INVALID, "%s: trace %d: non-finite position", who, t);
        }
    return IGM_OK;
}

// Once the entry knows Cmax, the largest of ncopy: bead (nspot, Cmax), the bead of spot i under copy
// k (0 for k >= C_t, never read).  Returns the spots staged per chunk.
inline int bead_table(const int32_t* copy_ptr, const int32_t* copy_idx, int ntrace, const int64_t* trace_ptr,
                      const int32_t* locus, const std::vector<int>& ncopy, int Cmax, std::vector<int>* bead) {
    bead->assign((size_t)trace_ptr[ntrace] * Cmax, 0);
    for (int t = 0; t < ntrace; ++t)
        for (int64_t i = trace_ptr[t]; i < trace_ptr[t + 1]; ++i)
            for (int k = 0; k < ncopy[t]; ++k) (*bead)[(size_t)i * Cmax + k] = copy_idx[copy_ptr[locus[i]] + k];
    const char* e = getenv("IGM_TRACING_CHUNK");  // (tests)
    return e ? std::min(kChunkMax, std::max(1, atoi(e))) : kChunkDefault;
}

}  // namespace igm
