// Per-bead neighbourhood census of the population report (igm_report_neighbours,
// include/igm_hip.h): for every (bead i, structure s) the number of cis partners and of
// trans partners per class label within the contact map's distance test.  The
// definitions are this project's (the reference has no such report).
//
// Every (i, s) sees all nbead partners: no symmetry, no atomics, one owner thread per
// (i, s), exact integer counters -- the result does not depend on scheduling.
//
// Layout.  A wave is 64 consecutive structures of its beads: in the bead-major population
// those are 768 contiguous bytes per bead, and whether a partner j is cis to bead i, which
// class j has and (radii form) which bound the pair has are the same in every lane.  A
// workgroup of 4 waves owns kNI = 32 beads i (kNR = 8 per thread, in registers) of one
// chunk of 64 structures and streams the partners through LDS in tiles of kNJ; a lane
// reads its structure of a partner at a stride of 3 words (conflict-free) and tests it
// against its 8 beads.  Partner traffic is 12 N^2 S / kNI bytes.
//
// Counters.  The host orders the partners by class (unlabelled last), so the class of a
// partner is not a run-time index into a counter array: one packed counter per bead is
// live at a time -- hits in the low 16 bits, cis hits in the high 16 (a count is at most
// 65534) -- fed by a wave-uniform increment (1 trans, 0x10001 cis, 0 ignored) and written
// out when its class segment ends.  Nothing is indexed at run time: no scratch memory.
//
// Compiled with -ffp-contract=off: d2 = (dx*dx + dy*dy) + dz*dz in float32, compared with
// sq_bound of the pair's bound, the test of igm_contact_map to the bit.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "exact_math.h"
#include "igm_ctx.h"

using namespace igm;

namespace {

constexpr int kNT = 256;                // threads per workgroup: 4 waves on the same 64 structures
constexpr int kNW = kNT / 64;           // waves per workgroup
constexpr int kNR = 8;                  // beads i per thread
constexpr int kNI = kNW * kNR;          // beads i per workgroup
constexpr int kNJ = 32;                 // partners per LDS tile
constexpr int kNRow = 64 * 3;           // floats of one partner's 64 structures
constexpr int kMaxClass = 8;
constexpr int kMaxCol = kMaxClass + 2;
constexpr int kMaxRadii = 16;

// The squared bounds: entry 0 of the centre-to-centre form, the (a, b) table of the
// distinct radius values of the radii form (igm_contact_map's bound, operation by operation)
__global__ void __launch_bounds__(kMaxRadii* kMaxRadii) neighbour_bounds_kernel(const float* __restrict__ vals,
                                                                                 int nval, float cr, float cutoff,
                                                                                 float* __restrict__ tab) {
    const int t = threadIdx.x, a = t / kMaxRadii, b = t % kMaxRadii;
    float v = -1.0f;
    if (nval == 0) {
        if (t == 0) v = sq_bound(cutoff);
    } else if (a < nval && b < nval) {
        v = sq_bound(__fmul_rn(cr, __fadd_rn(vals[a], vals[b])));
    }
    tab[t] = v;
}

// part[p] = {j | radius id << 16, chain of j} of the p-th partner in class order; seg holds
// the nseg + 1 bounds of the class segments (ncol = nseg + 1 columns per (i, s)).
template <bool RADII>
__global__ void __launch_bounds__(kNT) neighbour_census_kernel(const float* __restrict__ xyz, int n, int S,
                                                               const int2* __restrict__ part,
                                                               const int* __restrict__ seg, int nseg,
                                                               const int* __restrict__ chain,
                                                               const int* __restrict__ rid,
                                                               const float* __restrict__ tab, int min_sep,
                                                               int* __restrict__ census) {
    __shared__ float tile[kNJ * kNRow];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int s0 = blockIdx.y * 64, s = s0 + lane;
    const int w3 = min(64, S - s0) * 3;  // floats of this chunk in a bead's row
    const int ib = blockIdx.x * kNI + w * kNR;
    const int ncol = nseg + 1;
    const float cut = tab[0];

    float xi[kNR][3];
    int ca[kNR], ra[kNR];
#pragma unroll
    for (int a = 0; a < kNR; ++a) {
        const int i = min(ib + a, n - 1);  // a bead past the end repeats the last one and stores nothing
        ca[a] = chain[i];
        ra[a] = RADII ? rid[i] * kMaxRadii : 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) xi[a][k] = s < S ? xyz[((size_t)i * S + s) * 3 + k] : 0.f;
    }

    unsigned cis_total[kNR];
#pragma unroll
    for (int a = 0; a < kNR; ++a) cis_total[a] = 0u;

    for (int k = 0; k < nseg; ++k) {
        const int p0 = seg[k], p1 = seg[k + 1];
        unsigned cnt[kNR];
#pragma unroll
        for (int a = 0; a < kNR; ++a) cnt[a] = 0u;
        for (int t0 = p0; t0 < p1; t0 += kNJ) {
            const int nj = min(kNJ, p1 - t0);
            __syncthreads();
            for (int r = w; r < nj; r += kNW) {  // a wave stages whole rows: 3 coalesced loads each
                const int j = part[t0 + r].x & 0xffff;
                const float* __restrict__ src = xyz + ((size_t)j * S + s0) * 3;
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const int c = lane + 64 * q;
                    tile[r * kNRow + c] = c < w3 ? src[c] : 0.f;
                }
            }
            __syncthreads();
#pragma unroll 2
            for (int jj = 0; jj < nj; ++jj) {
                const int2 m = part[t0 + jj];
                const int j = m.x & 0xffff, rj = m.x >> 16;
                const float xj = tile[jj * kNRow + lane * 3], yj = tile[jj * kNRow + lane * 3 + 1],
                            zj = tile[jj * kNRow + lane * 3 + 2];
#pragma unroll
                for (int a = 0; a < kNR; ++a) {
                    // wave-uniform: cis partners count in both fields, ignored ones (i itself, cis
                    // within min_sep) in none
                    const int sep = abs(ib + a - j);
                    const unsigned inc = m.y == ca[a] ? (sep < min_sep ? 0u : 0x10001u) : 1u;
                    const float thr = RADII ? tab[ra[a] + rj] : cut;
                    const float dx = __fsub_rn(xi[a][0], xj), dy = __fsub_rn(xi[a][1], yj),
                                dz = __fsub_rn(xi[a][2], zj);
                    const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
                    cnt[a] += d2 <= thr ? inc : 0u;
                }
            }
        }
#pragma unroll
        for (int a = 0; a < kNR; ++a) {
            const unsigned cis = cnt[a] >> 16, all = cnt[a] & 0xffffu;
            cis_total[a] += cis;
            if (s < S && ib + a < n) census[((size_t)(ib + a) * S + s) * ncol + 1 + k] = (int)(all - cis);
        }
    }
#pragma unroll
    for (int a = 0; a < kNR; ++a)
        if (s < S && ib + a < n) census[((size_t)(ib + a) * S + s) * ncol] = (int)cis_total[a];
}

// One thread per bead walks its structures in order: the integer sums, and icp_sum as the
// sequential float64 sum of trans / (cis + trans) over the structures with a neighbour.
__global__ void __launch_bounds__(64) neighbour_sums_kernel(const int* __restrict__ census, int n, int S, int ncol,
                                                            long long* __restrict__ sums,
                                                            double* __restrict__ icp_sum,
                                                            int* __restrict__ icp_n) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    long long acc[kMaxCol];
#pragma unroll
    for (int c = 0; c < kMaxCol; ++c) acc[c] = 0;
    double f = 0.0;
    int nf = 0;
    for (int s = 0; s < S; ++s) {
        const int* __restrict__ row = census + ((size_t)i * S + s) * ncol;
        const int cis = row[0];
        int trans = 0;
        acc[0] += cis;
#pragma unroll
        for (int c = 1; c < kMaxCol; ++c)
            if (c < ncol) {
                const int v = row[c];
                acc[c] += v;
                trans += v;
            }
        if (cis + trans > 0) {
            f += (double)trans / (double)(cis + trans);
            ++nf;
        }
    }
#pragma unroll
    for (int c = 0; c < kMaxCol; ++c)
        if (c < ncol) sums[(size_t)i * ncol + c] = acc[c];
    icp_sum[i] = f;
    icp_n[i] = nf;
}

}  // namespace

extern "C" int igm_report_neighbours(igm_ctx* c, uint32_t flags, const float* xyz, int32_t nbead, int32_t nstruct,
                                     const int32_t* chain, const int32_t* cls, int32_t nclass, int32_t min_sep,
                                     float cutoff, const float* radii, double contact_range, int32_t* census,
                                     int64_t* sums, double* icp_sum, int32_t* icp_n) {
    static const char* fn = "igm_report_neighbours";
    if (!c) return IGM_E_INVALID;
    if (nbead <= 0 || nstruct <= 0 || !xyz || !chain)
        return fail(c, IGM_E_INVALID, "%s: invalid arguments (nbead %d, nstruct %d)", fn, nbead, nstruct);
    if (nclass < 0 || nclass > kMaxClass || (nclass > 0 && !cls))
        return fail(c, IGM_E_INVALID, "%s: nclass %d outside [0, %d] or cls missing", fn, nclass, kMaxClass);
    if (min_sep < 1) return fail(c, IGM_E_INVALID, "%s: min_sep %d < 1", fn, min_sep);
    if (!census && !sums && !icp_sum && !icp_n) return fail(c, IGM_E_INVALID, "%s: every output is NULL", fn);
    if (radii) {
        if (!(contact_range >= 0.0) || !std::isfinite(contact_range))
            return fail(c, IGM_E_INVALID, "%s: contact_range %g is negative or not finite", fn, contact_range);
    } else if (!(cutoff >= 0.0f) || !std::isfinite(cutoff)) {
        return fail(c, IGM_E_INVALID, "%s: cutoff %g is negative or not finite", fn, (double)cutoff);
    }
    if (nbead > 65535) return fail(c, IGM_E_UNSUPPORTED, "%s: %d beads exceed 65535", fn, nbead);
    const int64_t gy = ceil_div(nstruct, 64);
    if (gy > 65535) return fail(c, IGM_E_UNSUPPORTED, "%s: %d structures exceed the grid", fn, nstruct);
    if (cls)
        for (int b = 0; b < nbead; ++b)
            if (cls[b] < -1 || cls[b] >= nclass)
                return fail(c, IGM_E_INVALID, "%s: cls[%d] = %d outside [-1, %d)", fn, b, cls[b], nclass);
    // the distinct radius values (by bit pattern, in order of appearance) and every bead's id
    std::vector<float> vals;
    std::vector<int32_t> rid;
    if (radii) {
        rid.resize(nbead);
        for (int b = 0; b < nbead; ++b) {
            size_t v = 0;
            while (v < vals.size() && std::memcmp(&vals[v], &radii[b], sizeof(float)) != 0) ++v;
            if (v == vals.size()) {
                if (v == (size_t)kMaxRadii)
                    return fail(c, IGM_E_UNSUPPORTED, "%s: more than %d distinct radii", fn, kMaxRadii);
                vals.push_back(radii[b]);
            }
            rid[b] = (int32_t)v;
        }
    }
    const int nval = (int)vals.size();  // 0: the centre-to-centre form
    vals.resize(kMaxRadii, 0.f);
    // the partners in class order (unlabelled last), bead order inside a class
    const int nseg = nclass + 1, ncol = nclass + 2;
    std::vector<int32_t> seg(nseg + 1, 0);
    for (int b = 0; b < nbead; ++b) ++seg[(cls && cls[b] >= 0 ? cls[b] : nclass) + 1];
    for (int k = 0; k < nseg; ++k) seg[k + 1] += seg[k];
    std::vector<int32_t> part(2 * (size_t)nbead), at(seg.begin(), seg.end() - 1);
    for (int b = 0; b < nbead; ++b) {
        const int p = at[cls && cls[b] >= 0 ? cls[b] : nclass]++;
        part[2 * (size_t)p] = b | (radii ? rid[b] << 16 : 0);
        part[2 * (size_t)p + 1] = chain[b];
    }

    IGM_HIP_CHECK(c, hipSetDevice(c->device));
    const size_t ncen = (size_t)nbead * nstruct * ncol;
    const bool want_sums = sums || icp_sum || icp_n;
    const float* d_xyz;
    const int32_t *d_part, *d_seg, *d_chain, *d_rid = nullptr;
    const float* d_vals = nullptr;
    void *p_tab, *p_cen = nullptr, *p_sums = nullptr, *p_icp = nullptr, *p_icn = nullptr;
    IGM_TRY(to_device(c, flags, "rn_xyz", xyz, (size_t)nbead * nstruct * 3, &d_xyz));
    IGM_TRY(to_device(c, 0u, "rn_part", part.data(), part.size(), &d_part));
    IGM_TRY(to_device(c, 0u, "rn_seg", seg.data(), seg.size(), &d_seg));
    IGM_TRY(to_device(c, 0u, "rn_chain", chain, (size_t)nbead, &d_chain));
    if (radii) {
        IGM_TRY(to_device(c, 0u, "rn_rid", rid.data(), rid.size(), &d_rid));
        IGM_TRY(to_device(c, 0u, "rn_vals", vals.data(), vals.size(), &d_vals));
    }
    IGM_TRY(workspace(c, "rn_tab", sizeof(float) * kMaxRadii * kMaxRadii, &p_tab));
    // the census lives in the caller's device array, else in a plane of the context (staged
    // for a host caller, scratch for the sums when no census is asked for)
    int32_t* d_cen = census;
    if (!census || !(flags & IGM_DEVICE_PTRS)) {
        IGM_TRY(workspace(c, "rn_census", sizeof(int32_t) * ncen, &p_cen));
        d_cen = (int32_t*)p_cen;
    }
    if (want_sums) {
        IGM_TRY(workspace(c, "rn_sums", sizeof(int64_t) * (size_t)nbead * ncol, &p_sums));
        IGM_TRY(workspace(c, "rn_icp", sizeof(double) * (size_t)nbead, &p_icp));
        IGM_TRY(workspace(c, "rn_icn", sizeof(int32_t) * (size_t)nbead, &p_icn));
    }
    {
        Timed tm(c, "report_neighbours");
        hipLaunchKernelGGL(neighbour_bounds_kernel, dim3(1), dim3(kMaxRadii * kMaxRadii), 0, c->stream, d_vals,
                           nval, (float)contact_range, cutoff, (float*)p_tab);
        IGM_HIP_CHECK(c, hipGetLastError());
        const dim3 grid((unsigned)ceil_div(nbead, kNI), (unsigned)gy);
        if (radii)
            hipLaunchKernelGGL(neighbour_census_kernel<true>, grid, dim3(kNT), 0, c->stream, d_xyz, (int)nbead,
                               (int)nstruct, (const int2*)d_part, d_seg, nseg, d_chain, d_rid, (const float*)p_tab,
                               (int)min_sep, (int*)d_cen);
        else
            hipLaunchKernelGGL(neighbour_census_kernel<false>, grid, dim3(kNT), 0, c->stream, d_xyz, (int)nbead,
                               (int)nstruct, (const int2*)d_part, d_seg, nseg, d_chain, d_rid, (const float*)p_tab,
                               (int)min_sep, (int*)d_cen);
        IGM_HIP_CHECK(c, hipGetLastError());
        if (want_sums) {
            hipLaunchKernelGGL(neighbour_sums_kernel, dim3((unsigned)ceil_div(nbead, 64)), dim3(64), 0, c->stream,
                               (const int*)d_cen, (int)nbead, (int)nstruct, ncol, (long long*)p_sums, (double*)p_icp,
                               (int*)p_icn);
            IGM_HIP_CHECK(c, hipGetLastError());
        }
    }
    if (census) IGM_TRY(to_host(c, flags, census, (const int32_t*)d_cen, ncen));
    IGM_TRY(to_host(c, 0u, sums, (const int64_t*)p_sums, (size_t)nbead * ncol));
    IGM_TRY(to_host(c, 0u, icp_sum, (const double*)p_icp, (size_t)nbead));
    IGM_TRY(to_host(c, 0u, icp_n, (const int32_t*)p_icn, (size_t)nbead));
    // the staged tables are locals and the per-bead outputs are host arrays: wait before returning
    IGM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return finish(c, flags);
}
