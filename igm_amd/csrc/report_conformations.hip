// Pairwise conformation RMSD of chromosome copies (igm_report_conformations,
// include/igm_hip.h): the minimal RMSD after optimal rigid superposition between every two
// of the M = ncopy * nstruct conformations of one group of loci, and the reductions people
// take from that matrix (row sums, the copies of one cell against each other, a histogram),
// each available without the matrix.  The definitions are this project's.
//
// Preparation.  One workgroup per kT = 64 conformations, kPG groups of 64 threads: a lane
// is a conformation (for one bead the structures are contiguous in xyz), a group owns a
// contiguous run of the loci.  The groups' fp64 sums go through LDS and are added in group
// order, which is the ascending locus order cut in runs: the centre, then the centred
// coordinates written once as fp64, locus-major with the conformations contiguous
// (p[(3 i + c) * Mp + a], Mp = M rounded up to the tile, zeros past M), and g.
//
// Pairs.  A tiled Gram product of 3-vectors with Horn's eigen-solve as its epilogue.  A
// workgroup of 512 threads owns a kT x kT tile of the upper triangle; a thread keeps the
// nine fp64 sums of its 2 x 4 pairs (72 accumulators, 144 VGPRs of the 256 that two waves
// per SIMD leave a lane) and walks the loci in ascending order.  The two tile sides of a
// chunk of loci are staged in LDS (kChunk loci: 24 KB); a lane reads its two rows as a
// broadcast and its four columns as two conflict-free 16-byte reads (col_of), 144 B and nine
// ds_read_b128 for 72 FMAs: half the LDS cycles that the FMAs leave.  The next chunk is fetched into registers while the current one is multiplied.
// Then horn<false> on each of the eight pairs, the value rounded once to float32, written
// with its mirror and (same structure) into `same`.  The tile's float32 values go to LDS and
// 64 threads add each row and each column in ascending order into the slot (tile column, a)
// of a partial plane that nobody else writes; a last kernel adds a conformation's slots in
// tile order.  Counts of histogram bins are integers: LDS atomics, then one global integer
// atomic per bin and tile.  No float atomics; every float sum has one fixed order, and the
// same instructions run whether or not the matrix is asked for.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "horn.h"
#include "igm_ctx.h"

using namespace igm;

namespace {

constexpr int kT = 64;                 // conformations per tile side
constexpr int kPT = 512;               // threads of the pair kernel: 16 x 32, 2 x 4 pairs each
constexpr int kRR = 2, kRC = 4;
constexpr int kChunk = 8;              // loci staged at a time (the most; IGM_CONFORMATION_CHUNK lowers it)
constexpr int kLines = 2 * kChunk * 3; // rows of 64 doubles in LDS: side A, then side B
constexpr int kFetch = kLines * kT / kPT;
constexpr int kMaxBins = 4096;
constexpr int kPG = 16;                // locus groups of the preparation kernel
constexpr int kMaxM = 1 << 20;
static_assert(kT == 16 * kRC && kT == 32 * kRR && kPT == 16 * 32, "a thread's 2 x 4 pairs tile the 64 x 64 block");
static_assert(kLines * kT % kPT == 0, "every thread fetches the same number of staged doubles");

__device__ __forceinline__ double qnan() { return __longlong_as_double(0x7ff8000000000000LL); }

// p (3 nlocus, Mp) and g (Mp); bead (ncopy, nlocus)
__global__ void __launch_bounds__(kT* kPG) conf_prepare_kernel(const float* __restrict__ xyz, int S,
                                                               const int* __restrict__ bead, int nlocus, int M, int Mp,
                                                               double* __restrict__ p, double* __restrict__ g) {
    __shared__ double part[kPG][3][kT];
    __shared__ double ctr[3][kT];
    __shared__ int bad[kT];
    const int lane = threadIdx.x, grp = threadIdx.y;
    const int a = blockIdx.x * kT + lane;
    const bool live = a < M;
    const int k = live ? a / S : 0, s = live ? a - k * S : 0;
    const int seg = (nlocus + kPG - 1) / kPG;
    const int i0 = min(grp * seg, nlocus), i1 = min(i0 + seg, nlocus);
    const int* __restrict__ bk = bead + (size_t)k * nlocus;

    if (grp == 0) bad[lane] = 0;
    __syncthreads();
    double sx = 0.0, sy = 0.0, sz = 0.0;
    bool nonfinite = false;
    if (live)
        for (int i = i0; i < i1; ++i) {
            const float* __restrict__ q = xyz + ((size_t)bk[i] * S + s) * 3;
            const float x = q[0], y = q[1], z = q[2];
            nonfinite = nonfinite || !(isfinite(x) && isfinite(y) && isfinite(z));
            sx += (double)x;
            sy += (double)y;
            sz += (double)z;
        }
    part[grp][0][lane] = sx;
    part[grp][1][lane] = sy;
    part[grp][2][lane] = sz;
    if (nonfinite) atomicOr(&bad[lane], 1);
    __syncthreads();
    if (grp < 3) {
        double acc = 0.0;
        for (int q = 0; q < kPG; ++q) acc += part[q][grp][lane];
        ctr[grp][lane] = acc / (double)nlocus;
    }
    __syncthreads();
    const bool dead = !live || bad[lane] != 0;  // zeros: the pair kernel never multiplies a NaN
    const double cx = ctr[0][lane], cy = ctr[1][lane], cz = ctr[2][lane];
    double gg = 0.0;
    for (int i = i0; i < i1; ++i) {
        double x = 0.0, y = 0.0, z = 0.0;
        if (!dead) {
            const float* __restrict__ q = xyz + ((size_t)bk[i] * S + s) * 3;
            x = (double)q[0] - cx;
            y = (double)q[1] - cy;
            z = (double)q[2] - cz;
        }
        p[((size_t)i * 3) * Mp + a] = x;
        p[((size_t)i * 3 + 1) * Mp + a] = y;
        p[((size_t)i * 3 + 2) * Mp + a] = z;
        gg += x * x + y * y + z * z;
    }
    __syncthreads();  // the centres' partial sums have been read
    part[grp][0][lane] = gg;
    __syncthreads();
    if (grp == 0) {
        double acc = 0.0;
        for (int q = 0; q < kPG; ++q) acc += part[q][0][lane];
        g[a] = live && bad[lane] == 0 ? acc : qnan();
    }
}

struct PairArgs {
    const double* p;      // (3 nlocus, Mp)
    const double* g;      // (Mp)
    int nlocus, M, Mp, S, ncopy, chunk, nt;
    const float* edges;   // (nedge) or NULL
    int nedge;
    float* rmsd;          // (M, M) or NULL
    float* same;          // (S, ncopy, ncopy) or NULL
    double* psum;         // (nt, Mp): the sum over the conformations b of tile column t of rmsd(a, b)
    int* pcnt;            // (nt, Mp)
    unsigned long long* hist;  // (nedge - 1), zeroed, or NULL
};

// The four columns of lane tx: {2 tx, 2 tx + 1} and the same pair 32 columns on.  The 16 lanes
// that one LDS cycle serves then read 16 consecutive 16-byte words: no two on one bank (four
// consecutive columns per lane would put tx and tx + 8 on the same banks, every read twice as long).
__device__ __forceinline__ int col_of(int tx, int c) { return (c >> 1) * 32 + tx * 2 + (c & 1); }

__global__ void __launch_bounds__(kPT) conf_pairs_kernel(const PairArgs A) {
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (ti > tj) return;  // the upper triangle of tiles; the whole workgroup leaves
    __shared__ __attribute__((aligned(16))) double stage[kLines][kT];
    __shared__ float tile[kT][kT + 1];
    __shared__ int hl[kMaxBins];
    const int t = threadIdx.x;
    const int tx = t & 15, ty = t >> 4;
    const int nbin = A.hist ? A.nedge - 1 : 0;
    for (int q = t; q < nbin; q += kPT) hl[q] = 0;

    // thread t fetches column (t & 63) of the lines (t >> 6) + 8 q: lines [0, 24) are side A
    // (locus l, component c: line 3 l + c), [24, 48) side B
    const int fj = t & (kT - 1), fl = t >> 6;
    double fetch[kFetch];
    auto fetch_chunk = [&](int i0) {
        const int rows = 3 * min(A.chunk, A.nlocus - i0);
#pragma unroll
        for (int q = 0; q < kFetch; ++q) {
            const int line = fl + q * (kPT / kT);
            const int side = line >= 3 * kChunk, lr = line - side * 3 * kChunk;
            fetch[q] = lr < rows ? A.p[((size_t)i0 * 3 + lr) * A.Mp + (size_t)(side ? tj : ti) * kT + fj] : 0.0;
        }
    };

    double acc[kRR][kRC][9];
#pragma unroll
    for (int r = 0; r < kRR; ++r)
#pragma unroll
        for (int c = 0; c < kRC; ++c)
#pragma unroll
            for (int u = 0; u < 9; ++u) acc[r][c][u] = 0.0;

    fetch_chunk(0);
    for (int i0 = 0; i0 < A.nlocus; i0 += A.chunk) {
        const int nc = min(A.chunk, A.nlocus - i0);
        __syncthreads();  // the previous chunk has been multiplied
#pragma unroll
        for (int q = 0; q < kFetch; ++q) stage[fl + q * (kPT / kT)][fj] = fetch[q];
        __syncthreads();
        if (i0 + A.chunk < A.nlocus) fetch_chunk(i0 + A.chunk);
        for (int l = 0; l < nc; ++l) {
            double a[kRR][3], b[kRC][3];
#pragma unroll
            for (int u = 0; u < 3; ++u) {
#pragma unroll
                for (int r = 0; r < kRR; ++r) a[r][u] = stage[3 * l + u][ty * kRR + r];
#pragma unroll
                for (int c = 0; c < kRC; ++c) b[c][u] = stage[3 * (kChunk + l) + u][col_of(tx, c)];
            }
#pragma unroll
            for (int r = 0; r < kRR; ++r)
#pragma unroll
                for (int c = 0; c < kRC; ++c)
#pragma unroll
                    for (int u = 0; u < 3; ++u)
#pragma unroll
                        for (int v = 0; v < 3; ++v) acc[r][c][3 * u + v] += a[r][u] * b[c][v];
        }
    }

    // the epilogue: one eigen-solve per pair a < b; a slot of the tile that is no such pair
    // (past M, on or below the diagonal) or whose value is not finite holds NaN: not summed
    const float fnan = __int_as_float(0x7fc00000);
    const double dn = (double)A.nlocus;
#pragma unroll
    for (int r = 0; r < kRR; ++r) {
        const int ra = ty * kRR + r, ia = ti * kT + ra;
        const double ga = ia < A.M ? A.g[ia] : 0.0;
#pragma unroll
        for (int c = 0; c < kRC; ++c) {
            const int cb = col_of(tx, c), ib = tj * kT + cb;
            float out = fnan;
            if (ia < A.M && ib < A.M && ia <= ib) {
                const double gb = A.g[ib];
                float v;
                if (ga != ga || gb != gb) {
                    v = fnan;
                } else if (ia == ib) {
                    v = 0.0f;
                } else {
                    double m[3][3], quat[4];
#pragma unroll
                    for (int u = 0; u < 3; ++u)
#pragma unroll
                        for (int w = 0; w < 3; ++w) m[u][w] = acc[r][c][3 * u + w];
                    const double lam = horn<false>(m, quat);
                    v = (float)sqrt(fmax(0.0, (ga + gb - 2.0 * lam) / dn));
                }
                if (A.rmsd) {
                    A.rmsd[(size_t)ia * A.M + ib] = v;
                    if (ia != ib) A.rmsd[(size_t)ib * A.M + ia] = v;
                }
                const int ka = ia / A.S, sa = ia - ka * A.S, kb = ib / A.S, sb = ib - kb * A.S;
                if (A.same && sa == sb) {
                    float* __restrict__ cell = A.same + (size_t)sa * A.ncopy * A.ncopy;
                    cell[ka * A.ncopy + kb] = v;
                    if (ia != ib) cell[kb * A.ncopy + ka] = v;
                }
                if (ia != ib && isfinite(v)) {
                    out = v;
                    if (nbin > 0 && v >= A.edges[0] && v <= A.edges[nbin]) {
                        int lo = 0, hi = nbin;  // edges[lo] <= v < edges[hi], or v == edges[nbin]: the last bin
                        while (hi - lo > 1) {
                            const int mid = (lo + hi) >> 1;
                            if (A.edges[mid] <= v)
                                lo = mid;
                            else
                                hi = mid;
                        }
                        atomicAdd(&hl[lo], 1);
                    }
                }
            }
            tile[ra][cb] = out;
        }
    }
    __syncthreads();
    for (int q = t; q < nbin; q += kPT)
        if (hl[q]) atomicAdd(A.hist + q, (unsigned long long)hl[q]);
    // the sums of the tile's rows (into the slot of tile column tj) and of its columns (rmsd is
    // symmetric: into the slot of tile column ti), ascending; on a diagonal tile both belong to
    // the same slot, the column part (b < a) first
    if (t < 2 * kT) {
        const int q = t & (kT - 1);
        const bool col = t >= kT;
        if (!(col && ti == tj)) {
            double sum = 0.0;
            int cnt = 0;
            if (col || ti == tj)
                for (int r = 0; r < kT; ++r) {
                    const float v = tile[r][q];
                    if (v == v) {
                        sum += (double)v;
                        ++cnt;
                    }
                }
            if (!col)
                for (int c = 0; c < kT; ++c) {
                    const float v = tile[q][c];
                    if (v == v) {
                        sum += (double)v;
                        ++cnt;
                    }
                }
            const size_t slot = (size_t)(col ? ti : tj) * A.Mp + (size_t)(col ? tj : ti) * kT + q;
            A.psum[slot] = sum;
            A.pcnt[slot] = cnt;
        }
    }
}

__global__ void __launch_bounds__(256) conf_rows_kernel(const double* __restrict__ psum, const int* __restrict__ pcnt,
                                                        int nt, int M, int Mp, double* __restrict__ row_sum,
                                                        int* __restrict__ row_n) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= M) return;
    double sum = 0.0;
    int cnt = 0;
    for (int q = 0; q < nt; ++q) {
        sum += psum[(size_t)q * Mp + a];
        cnt += pcnt[(size_t)q * Mp + a];
    }
    row_sum[a] = sum;
    row_n[a] = cnt;
}

}  // namespace

extern "C" int igm_report_conformations(igm_ctx* c, uint32_t flags, const float* xyz, int32_t nbead, int32_t nstruct,
                                        const int32_t* bead, int32_t ncopy, int32_t nlocus, const float* edges,
                                        int32_t nedge, float* rmsd, double* g, double* row_sum, int32_t* row_n,
                                        float* same, int64_t* hist) {
    static const char* fn = "igm_report_conformations";
    if (!c) return IGM_E_INVALID;
    if (nbead <= 0 || nstruct <= 0 || ncopy <= 0 || nlocus <= 0 || !xyz || !bead)
        return fail(c, IGM_E_INVALID, "%s: invalid arguments (nbead %d, nstruct %d, ncopy %d, nlocus %d)", fn, nbead,
                    nstruct, ncopy, nlocus);
    if (!rmsd && !g && !row_sum && !row_n && !same && !hist)
        return fail(c, IGM_E_INVALID, "%s: every output is NULL", fn);
    if (hist) {
        if (!edges || nedge < 2) return fail(c, IGM_E_INVALID, "%s: a histogram needs at least two edges", fn);
        for (int q = 0; q < nedge; ++q)
            if (!std::isfinite(edges[q]) || (q > 0 && !(edges[q] > edges[q - 1])))
                return fail(c, IGM_E_INVALID, "%s: edges[%d] is not finite or not above its predecessor", fn, q);
        if (nedge - 1 > kMaxBins)
            return fail(c, IGM_E_UNSUPPORTED, "%s: %d histogram bins exceed %d", fn, nedge - 1, kMaxBins);
    }
    if ((int64_t)ncopy * nstruct > kMaxM)
        return fail(c, IGM_E_UNSUPPORTED, "%s: %lld conformations exceed %d", fn, (long long)ncopy * nstruct, kMaxM);
    for (size_t q = 0; q < (size_t)ncopy * nlocus; ++q)
        if (bead[q] < 0 || bead[q] >= nbead)
            return fail(c, IGM_E_INVALID, "%s: bead %d outside [0, %d)", fn, bead[q], nbead);
    const char* e = getenv("IGM_CONFORMATION_CHUNK");  // (tests)
    const int chunk = e ? std::min(kChunk, std::max(1, atoi(e))) : kChunk;

    IGM_HIP_CHECK(c, hipSetDevice(c->device));
    const int M = ncopy * nstruct, nt = (int)ceil_div(M, kT), Mp = nt * kT;
    const size_t mm = (size_t)M * M, ns = (size_t)nstruct * ncopy * ncopy;
    const int nbin = hist ? nedge - 1 : 0;
    const float* d_xyz;
    const int32_t* d_bead;
    const float* d_edges = nullptr;
    float* d_rmsd = rmsd;
    void *p_p, *p_g, *p_ps, *p_pc, *p_rs, *p_rn, *p_same = nullptr, *p_hist = nullptr, *p_rmsd;
    IGM_TRY(to_device(c, flags, "rc_xyz", xyz, (size_t)nbead * nstruct * 3, &d_xyz));
    IGM_TRY(to_device(c, 0u, "rc_bead", bead, (size_t)ncopy * nlocus, &d_bead));
    if (hist) IGM_TRY(to_device(c, 0u, "rc_edges", edges, (size_t)nedge, &d_edges));
    IGM_TRY(workspace(c, "rc_p", sizeof(double) * 3 * (size_t)nlocus * Mp, &p_p));
    IGM_TRY(workspace(c, "rc_g", sizeof(double) * (size_t)Mp, &p_g));
    IGM_TRY(workspace(c, "rc_psum", sizeof(double) * (size_t)nt * Mp, &p_ps));
    IGM_TRY(workspace(c, "rc_pcnt", sizeof(int) * (size_t)nt * Mp, &p_pc));
    IGM_TRY(workspace(c, "rc_rsum", sizeof(double) * (size_t)M, &p_rs));
    IGM_TRY(workspace(c, "rc_rn", sizeof(int32_t) * (size_t)M, &p_rn));
    if (same) IGM_TRY(workspace(c, "rc_same", sizeof(float) * ns, &p_same));
    if (hist) {
        IGM_TRY(workspace(c, "rc_hist", sizeof(int64_t) * (size_t)nbin, &p_hist));
        IGM_HIP_CHECK(c, hipMemsetAsync(p_hist, 0, sizeof(int64_t) * (size_t)nbin, c->stream));
    }
    if (rmsd && !(flags & IGM_DEVICE_PTRS)) {
        IGM_TRY(workspace(c, "rc_rmsd", sizeof(float) * mm, &p_rmsd));
        d_rmsd = (float*)p_rmsd;
    }
    const PairArgs A{(const double*)p_p, (const double*)p_g, (int)nlocus, M, Mp, (int)nstruct, (int)ncopy, chunk, nt,
                     d_edges, (int)nedge, d_rmsd, (float*)p_same, (double*)p_ps, (int*)p_pc,
                     (unsigned long long*)p_hist};
    {
        Timed tm(c, "report_conformations");
        hipLaunchKernelGGL(conf_prepare_kernel, dim3((unsigned)nt), dim3(kT, kPG), 0, c->stream, d_xyz, (int)nstruct,
                           d_bead, (int)nlocus, M, Mp, (double*)p_p, (double*)p_g);
        IGM_HIP_CHECK(c, hipGetLastError());
        hipLaunchKernelGGL(conf_pairs_kernel, dim3((unsigned)nt, (unsigned)nt), dim3(kPT), 0, c->stream, A);
        IGM_HIP_CHECK(c, hipGetLastError());
        hipLaunchKernelGGL(conf_rows_kernel, dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, c->stream,
                           (const double*)p_ps, (const int*)p_pc, nt, M, Mp, (double*)p_rs, (int*)p_rn);
        IGM_HIP_CHECK(c, hipGetLastError());
    }
    if (rmsd) IGM_TRY(to_host(c, flags, rmsd, (const float*)d_rmsd, mm));
    IGM_TRY(to_host(c, 0u, g, (const double*)p_g, (size_t)M));
    IGM_TRY(to_host(c, 0u, row_sum, (const double*)p_rs, (size_t)M));
    IGM_TRY(to_host(c, 0u, row_n, (const int32_t*)p_rn, (size_t)M));
    IGM_TRY(to_host(c, 0u, same, (const float*)p_same, ns));
    IGM_TRY(to_host(c, 0u, hist, (const int64_t*)p_hist, (size_t)nbin));
    IGM_HIP_CHECK(c, hipStreamSynchronize(c->stream));  // all but the matrix are host arrays
    return finish(c, flags);
}
