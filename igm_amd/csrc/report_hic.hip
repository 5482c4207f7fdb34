// Hi-C report on the GPU: the sufficient statistics of report_hic (igm/report/hic.py) --
// the Pearson correlations between the input matrix and the simulated contact map, per
// chromosome and inter-chromosomal, over all / imposed / non-imposed entries, and the two
// 2-D histograms of input against output probability -- from the haploid contact counts
// (igm_contact_map_haploid) and the input matrix's CSR.  include/igm_hip.h states the
// arithmetic.  Compiled with -ffp-contract=off.  Every integer statistic is summed with
// integer atomics after a per-wave reduction (exact in any order); every float64 sum has a
// fixed order -- a lane-strided walk of the row, a fixed shuffle tree, then the rows by a
// second fixed-order step (hic_rows_kernel) -- and there is no floating-point atomic, so a
// rerun is bitwise equal.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "igm_ctx.h"

using namespace igm;

namespace {

constexpr int kHT = 256;  // threads per workgroup
constexpr int kHW = kHT / 64;
constexpr int kMaxLdsHist = 12288;  // bins of a workgroup's private histogram (48 KB of LDS)
constexpr int kHistGroups = 1024;   // workgroups of a histogram launch at most

typedef unsigned long long u64;

// np.histogram's bin of v on the given edges: edges[k] <= v < edges[k+1], the last bin
// closed on the right, -1 outside the range (and for NaN)
__device__ __forceinline__ int bin_of(const double* __restrict__ edges, int nbins, double v) {
    if (!(v >= edges[0]) || !(v <= edges[nbins])) return -1;
    int lo = 0, hi = nbins + 1;  // number of edges <= v
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (edges[mid] <= v) lo = mid + 1;
        else hi = mid;
    }
    return lo > nbins ? nbins - 1 : lo - 1;
}

// c' = min(c, nstruct): the clip of counts / nstruct to [0, 1] decided on integers (a
// negative count, which igm_contact_map_haploid never writes, reads as 0)
__device__ __forceinline__ long long clip_count(int c, int nstruct) {
    return (long long)min(max(c, 0), nstruct);
}

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// Device form of the column check: every stored column of row a lies in [a, nhap)
__global__ void __launch_bounds__(kHT) hic_check_kernel(const long long* __restrict__ indptr,
                                                        const int* __restrict__ indices, int nhap,
                                                        int* __restrict__ bad) {
    const int a = blockIdx.x * kHW + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (a >= nhap) return;
    for (long long k = indptr[a] + lane; k < indptr[a + 1]; k += 64) {
        const int b = indices[k];
        if (b < a) atomicOr(bad, 1);
        else if (b >= nhap) atomicOr(bad, 2);
    }
}

// Integer pass over the dense counts, one workgroup per row a.  An entry (a, b) on one
// chromosome belongs to that chromosome's full symmetric block; an entry on two
// chromosomes belongs to the inter population when a < b.  The row is read 16 bytes per
// lane from the first 16-byte aligned element on, the head and the tail one element per
// lane.  sums: (nchrom + 1, 2) = {sum c', sum c'^2}, row nchrom is the inter population.
__global__ void __launch_bounds__(kHT) hic_dense_kernel(const int* __restrict__ counts, int nhap, int nstruct,
                                                        const int* __restrict__ hap_chrom, int nchrom,
                                                        u64* __restrict__ sums) {
    __shared__ long long red[kHW][4];
    const int a = blockIdx.x, t = threadIdx.x;
    const int ca = hap_chrom[a];
    const int* row = counts + (size_t)a * nhap;
    long long s1 = 0, s2 = 0, e1 = 0, e2 = 0;  // intra, inter

    auto take = [nstruct, ca, a, hap_chrom](int b, int c, long long& i1, long long& i2, long long& x1,
                                            long long& x2) {
        const long long v = clip_count(c, nstruct);
        const bool same = hap_chrom[b] == ca, upper = !same && b > a;
        i1 += same ? v : 0;
        i2 += same ? v * v : 0;
        x1 += upper ? v : 0;
        x2 += upper ? v * v : 0;
    };
    const int head = min(nhap, (int)((4u - (unsigned)(((uintptr_t)row >> 2) & 3u)) & 3u));
    const int nvec = (nhap - head) >> 2;
    if (t < head) take(t, row[t], s1, s2, e1, e2);
    const int4* vrow = reinterpret_cast<const int4*>(row + head);
    for (int q = t; q < nvec; q += kHT) {
        const int4 v = vrow[q];
        const int b = head + 4 * q;
        take(b, v.x, s1, s2, e1, e2);
        take(b + 1, v.y, s1, s2, e1, e2);
        take(b + 2, v.z, s1, s2, e1, e2);
        take(b + 3, v.w, s1, s2, e1, e2);
    }
    const int tail = head + 4 * nvec;
    if (tail + t < nhap) take(tail + t, row[tail + t], s1, s2, e1, e2);  // at most 3 elements

    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    e1 = wave_sum(e1);
    e2 = wave_sum(e2);
    if ((t & 63) == 0) {
        red[t >> 6][0] = s1;
        red[t >> 6][1] = s2;
        red[t >> 6][2] = e1;
        red[t >> 6][3] = e2;
    }
    __syncthreads();
    if (t < 4) {
        long long tot = 0;
        for (int w = 0; w < kHW; ++w) tot += red[w][t];
        const int p = t < 2 ? ca : nchrom;
        if (tot) atomicAdd(&sums[(size_t)p * 2 + (t & 1)], (u64)tot);
    }
}

// Sparse pass 1, one wave per row of the CSR.  A stored entry (a, b), b >= a, with value x
// (float32 widened) and clipped count c' belongs to population slot 0 (the chromosome of
// a, weight 2 off the diagonal and 1 on it) or slot 1 (inter, weight 1) and to the half
// h = 0 (x >= sigma of its population) or 1.
//   ints  (nchrom + 1, 2 halves, 3) = {sum w, sum w c', sum w c'^2}: integer atomics
//   rowx  (nhap, 2 slots, 2 halves) = the row's sum of w x
__global__ void __launch_bounds__(kHT) hic_pass1_kernel(const int* __restrict__ counts, int nhap, int nstruct,
                                                        const long long* __restrict__ indptr,
                                                        const int* __restrict__ indices,
                                                        const float* __restrict__ data,
                                                        const int* __restrict__ hap_chrom, int nchrom,
                                                        double sig_intra, double sig_inter, u64* __restrict__ ints,
                                                        double* __restrict__ rowx) {
    const int a = blockIdx.x * kHW + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (a >= nhap) return;  // the whole wave leaves; no workgroup barrier below
    const int ca = hap_chrom[a];
    const int* row = counts + (size_t)a * nhap;
    long long cnt[4] = {0, 0, 0, 0}, sc[4] = {0, 0, 0, 0}, sc2[4] = {0, 0, 0, 0};
    double sx[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long k = indptr[a] + lane; k < indptr[a + 1]; k += 64) {
        const int b = indices[k];
        const double x = (double)data[k];
        const long long c = clip_count(row[b], nstruct);
        const bool inter = hap_chrom[b] != ca;
        const long long w = (inter || b == a) ? 1 : 2;
        const int idx = (inter ? 2 : 0) + ((x >= (inter ? sig_inter : sig_intra)) ? 0 : 1);
        const double wx = (double)w * x;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool on = q == idx;
            cnt[q] += on ? w : 0;
            sc[q] += on ? w * c : 0;
            sc2[q] += on ? w * c * c : 0;
            sx[q] += on ? wx : 0.0;
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const long long n = wave_sum(cnt[q]), s = wave_sum(sc[q]), s2 = wave_sum(sc2[q]);
        const double x = wave_sum(sx[q]);
        if (lane == 0) {
            const int p = q < 2 ? ca : nchrom;
            u64* o = ints + ((size_t)p * 2 + (q & 1)) * 3;
            if (n) {
                atomicAdd(o, (u64)n);
                atomicAdd(o + 1, (u64)s);
                atomicAdd(o + 2, (u64)s2);
            }
            rowx[(size_t)a * 4 + q] = x;
        }
    }
}

// Sparse pass 2, the same walk.  means: (nchrom + 1, 3 masks, 2) = {ybar, xbar} with the
// masks all / restrained / non-restrained; an entry adds to the mask 'all' and to the
// mask of its half:
//   cross += (w x) (y - ybar)        y = c' / nstruct (one float64 division)
//   varx  += w ((x - xbar) (x - xbar))
//   rowc  (nhap, 2 slots, 3 masks, 2) = the row's {cross, varx}
__global__ void __launch_bounds__(kHT) hic_pass2_kernel(const int* __restrict__ counts, int nhap, int nstruct,
                                                        const long long* __restrict__ indptr,
                                                        const int* __restrict__ indices,
                                                        const float* __restrict__ data,
                                                        const int* __restrict__ hap_chrom, int nchrom,
                                                        double sig_intra, double sig_inter,
                                                        const double* __restrict__ means, double* __restrict__ rowc) {
    const int a = blockIdx.x * kHW + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (a >= nhap) return;
    const int ca = hap_chrom[a];
    const int* row = counts + (size_t)a * nhap;
    double yb[6], xb[6], cr[6], vx[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const int p = q < 3 ? ca : nchrom;
        yb[q] = means[((size_t)p * 3 + q % 3) * 2];
        xb[q] = means[((size_t)p * 3 + q % 3) * 2 + 1];
        cr[q] = 0.0;
        vx[q] = 0.0;
    }
    const double dS = (double)nstruct;
    for (long long k = indptr[a] + lane; k < indptr[a + 1]; k += 64) {
        const int b = indices[k];
        const double x = (double)data[k];
        const double y = (double)clip_count(row[b], nstruct) / dS;
        const bool inter = hap_chrom[b] != ca;
        const double w = (inter || b == a) ? 1.0 : 2.0;
        const int half = (x >= (inter ? sig_inter : sig_intra)) ? 1 : 2;  // the mask of the entry's half
        const double wx = w * x;
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const bool on = (q >= 3) == inter && (q % 3 == 0 || q % 3 == half);
            const double d = x - xb[q];
            cr[q] += on ? wx * (y - yb[q]) : 0.0;
            vx[q] += on ? w * (d * d) : 0.0;
        }
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const double c = wave_sum(cr[q]), v = wave_sum(vx[q]);
        if (lane == 0) {
            rowc[((size_t)a * 6 + q) * 2] = c;
            rowc[((size_t)a * 6 + q) * 2 + 1] = v;
        }
    }
}

// One 2-D histogram of the stored entries: np.histogram2d(y, x, bins=(ey, ex)) over the
// whole symmetric matrix (weight 2 off the diagonal, 1 on it), rows = y, columns = x.
// A workgroup walks the rows blockIdx.x * kHW + wave, + gridDim.x * kHW, ... (one wave per
// row) and counts in a private LDS copy (lds_bins = nx * ny 32-bit counters: a workgroup
// sees fewer than 2^31 entries), flushed with one integer atomic per non-empty bin; with
// lds_bins = 0 (more than kMaxLdsHist bins) it counts in global memory directly.  Measured
// at 200 kb (2.6 M stored entries on a few distinct values): 9.3 ms with global atomics
// per entry against the LDS copy's time in profiles/report_hic_resource_usage.md.
__global__ void __launch_bounds__(kHT) hic_hist_kernel(const int* __restrict__ counts, int nhap, int nstruct,
                                                       const long long* __restrict__ indptr,
                                                       const int* __restrict__ indices,
                                                       const float* __restrict__ data, const double* __restrict__ ex,
                                                       int nx, const double* __restrict__ ey, int ny,
                                                       u64* __restrict__ hist, int lds_bins) {
    extern __shared__ unsigned int lhist[];
    const int t = threadIdx.x, lane = t & 63;
    for (int k = t; k < lds_bins; k += kHT) lhist[k] = 0;
    __syncthreads();
    const double dS = (double)nstruct;
    for (int a = blockIdx.x * kHW + (t >> 6); a < nhap; a += gridDim.x * kHW) {
        const int* row = counts + (size_t)a * nhap;
        for (long long k = indptr[a] + lane; k < indptr[a + 1]; k += 64) {
            const int b = indices[k];
            const int kx = bin_of(ex, nx, (double)data[k]);
            if (kx < 0) continue;
            const int ky = bin_of(ey, ny, (double)clip_count(row[b], nstruct) / dS);
            if (ky < 0) continue;
            const unsigned w = b == a ? 1u : 2u;
            if (lds_bins) atomicAdd(&lhist[ky * nx + kx], w);
            else atomicAdd(&hist[(size_t)ky * nx + kx], (u64)w);
        }
    }
    __syncthreads();
    for (int k = t; k < lds_bins; k += kHT)
        if (lhist[k]) atomicAdd(&hist[k], (u64)lhist[k]);
}

// The rows in a fixed order: rows (nhap, 2 slots, width) -> out (nchrom + 1, width).
// Workgroup p < nchrom adds slot 0 of the rows of chromosome p, workgroup nchrom slot 1 of
// every row.  Per column, thread t adds the rows t, t + 256, ... in ascending order (a row
// of another chromosome adds 0.0), then the 256 partial sums are added by the shuffle tree
// of every wave and the four waves in order.
__global__ void __launch_bounds__(kHT) hic_rows_kernel(const double* __restrict__ rows, int nhap, int width,
                                                       const int* __restrict__ hap_chrom, int nchrom,
                                                       double* __restrict__ out) {
    __shared__ double red[kHW];
    const int p = blockIdx.x, t = threadIdx.x;
    const bool inter = p == nchrom;
    for (int q = 0; q < width; ++q) {
        const double* col = rows + (inter ? width : 0) + q;
        double s = 0.0;
        for (int a = t; a < nhap; a += kHT) {
            const double v = col[(size_t)a * 2 * width];
            s += (inter || hap_chrom[a] == p) ? v : 0.0;
        }
        s = wave_sum(s);
        __syncthreads();
        if ((t & 63) == 0) red[t >> 6] = s;
        __syncthreads();
        if (t == 0) {
            double tot = 0.0;
            for (int w = 0; w < kHW; ++w) tot += red[w];
            out[(size_t)p * width + q] = tot;
        }
    }
}

// a / b correctly rounded to float64 for integers 0 <= a <= b, 0 < b < 2^63: a is
// normalised to 64 bits and shifted by 63 more, so the integer quotient has at least 64
// bits; the remainder is the sticky bit of the one rounding (u128 -> float64).
double ratio_rn(uint64_t a, uint64_t b) {
    if (a == 0) return 0.0;
    const int la = __builtin_clzll(a);
    const unsigned __int128 num = (unsigned __int128)(a << la) << 63;
    unsigned __int128 q = num / b;
    if (num % b) q |= 1;
    return std::ldexp((double)q, -(la + 63));
}

int check_hist_edges(igm_ctx* c, const char* fn, const char* what, const double* e, int nbins) {
    if (!e || nbins < 1)
        return fail(c, IGM_E_INVALID, "%s: %s needs nbins >= 1 (%d) and nbins + 1 edges", fn, what, nbins);
    for (int k = 0; k <= nbins; ++k)
        if (!std::isfinite(e[k])) return fail(c, IGM_E_INVALID, "%s: %s[%d] is not finite", fn, what, k);
    for (int k = 0; k < nbins; ++k)
        if (!(e[k + 1] > e[k]))
            return fail(c, IGM_E_INVALID, "%s: %s not strictly increasing at %d (%.17g, %.17g)", fn, what, k, e[k],
                        e[k + 1]);
    if (!(e[0] > 0.0))
        return fail(c, IGM_E_UNSUPPORTED,
                    "%s: %s[0] = %g <= 0: the entries that are not stored (x = 0) are never binned", fn, what, e[0]);
    return IGM_OK;
}

}  // namespace

extern "C" int igm_report_hic(igm_ctx* c, uint32_t flags, const int32_t* counts, int32_t nhap, int32_t nstruct,
                              const int64_t* indptr, const int32_t* indices, const float* data,
                              const int32_t* hap_chrom, int32_t nchrom, double intra_sigma, double inter_sigma,
                              const double* log_edges_x, int32_t log_nx, const double* log_edges_y, int32_t log_ny,
                              int64_t* log_hist, const double* lin_edges_x, int32_t lin_nx,
                              const double* lin_edges_y, int32_t lin_ny, int64_t* lin_hist, int64_t* dense_sums,
                              int64_t* sparse_ints, double* sparse_sumx, double* means, double* centred) {
    static const char* fn = "igm_report_hic";
    if (!c) return IGM_E_INVALID;
    if (nhap <= 0 || nchrom <= 0 || !counts || !indptr || !hap_chrom || !dense_sums || !sparse_ints ||
        !sparse_sumx || !means || !centred)
        return fail(c, IGM_E_INVALID, "%s: invalid arguments (nhap %d, nchrom %d or a NULL array)", fn, nhap, nchrom);
    if (nstruct < 1) return fail(c, IGM_E_INVALID, "%s: nstruct = %d, expected >= 1", fn, nstruct);
    // sum c'^2 <= nhap^2 nstruct^2 must stay below 2^63
    if ((unsigned __int128)((uint64_t)nhap * (uint64_t)nhap) * ((uint64_t)nstruct * (uint64_t)nstruct) >=
        ((unsigned __int128)1 << 63))
        return fail(c, IGM_E_UNSUPPORTED, "%s: nhap^2 nstruct^2 (%d, %d) reaches 2^63: the integer sums could overflow",
                    fn, nhap, nstruct);
    if (indptr[0] != 0) return fail(c, IGM_E_INVALID, "%s: indptr[0] = %lld, expected 0", fn, (long long)indptr[0]);
    for (int a = 0; a < nhap; ++a)
        if (indptr[a + 1] < indptr[a])
            return fail(c, IGM_E_INVALID, "%s: indptr decreases at row %d (%lld -> %lld)", fn, a, (long long)indptr[a],
                        (long long)indptr[a + 1]);
    const int64_t nnz = indptr[nhap];
    if (nnz > 0 && (!indices || !data))
        return fail(c, IGM_E_INVALID, "%s: %lld entries without indices / data", fn, (long long)nnz);
    std::vector<int64_t> msize(nchrom, 0);
    for (int a = 0; a < nhap; ++a) {
        if (hap_chrom[a] < 0 || hap_chrom[a] >= nchrom)
            return fail(c, IGM_E_INVALID, "%s: hap_chrom[%d] = %d outside [0, %d)", fn, a, hap_chrom[a], nchrom);
        ++msize[hap_chrom[a]];
    }
    if (log_hist) {
        IGM_TRY(check_hist_edges(c, fn, "log_edges_x", log_edges_x, log_nx));
        IGM_TRY(check_hist_edges(c, fn, "log_edges_y", log_edges_y, log_ny));
    }
    if (lin_hist) {
        IGM_TRY(check_hist_edges(c, fn, "lin_edges_x", lin_edges_x, lin_nx));
        IGM_TRY(check_hist_edges(c, fn, "lin_edges_y", lin_edges_y, lin_ny));
    }
    const bool dev = flags & IGM_DEVICE_PTRS;
    if (!dev)
        for (int a = 0; a < nhap; ++a)
            for (int64_t k = indptr[a]; k < indptr[a + 1]; ++k) {
                if (indices[k] < a)
                    return fail(c, IGM_E_INVALID,
                                "%s: entry (%d, %d) lies below the diagonal (upper triangle expected)", fn, a,
                                indices[k]);
                if (indices[k] >= nhap)
                    return fail(c, IGM_E_INVALID, "%s: column %d of row %d outside [0, %d)", fn, indices[k], a, nhap);
            }
    // a sigma that is not given (<= 0 or NaN) puts every stored entry in the half x < sigma
    const double sig_intra = intra_sigma > 0.0 ? intra_sigma : (double)INFINITY;
    const double sig_inter = inter_sigma > 0.0 ? inter_sigma : (double)INFINITY;
    const int P = nchrom + 1;

    IGM_HIP_CHECK(c, hipSetDevice(c->device));
    const int32_t *d_counts, *d_idx, *d_chrom;
    const float* d_data;
    const int64_t* d_ptr;
    IGM_TRY(to_device(c, flags, "rh_counts", counts, (size_t)nhap * nhap, &d_counts));
    IGM_TRY(to_device(c, flags, "rh_idx", indices, (size_t)nnz, &d_idx));
    IGM_TRY(to_device(c, flags, "rh_data", data, (size_t)nnz, &d_data));
    IGM_TRY(to_device(c, 0u, "rh_ptr", indptr, (size_t)nhap + 1, &d_ptr));
    IGM_TRY(to_device(c, 0u, "rh_chrom", hap_chrom, (size_t)nhap, &d_chrom));
    const double *d_lgx = nullptr, *d_lgy = nullptr, *d_lix = nullptr, *d_liy = nullptr;
    u64 *d_lgh = nullptr, *d_lih = nullptr;
    void* p;
    if (log_hist) {
        IGM_TRY(to_device(c, 0u, "rh_lgx", log_edges_x, (size_t)log_nx + 1, &d_lgx));
        IGM_TRY(to_device(c, 0u, "rh_lgy", log_edges_y, (size_t)log_ny + 1, &d_lgy));
        IGM_TRY(workspace(c, "rh_lgh", sizeof(u64) * (size_t)log_nx * log_ny, &p));
        d_lgh = (u64*)p;
        IGM_HIP_CHECK(c, hipMemsetAsync(d_lgh, 0, sizeof(u64) * (size_t)log_nx * log_ny, c->stream));
    }
    if (lin_hist) {
        IGM_TRY(to_device(c, 0u, "rh_lix", lin_edges_x, (size_t)lin_nx + 1, &d_lix));
        IGM_TRY(to_device(c, 0u, "rh_liy", lin_edges_y, (size_t)lin_ny + 1, &d_liy));
        IGM_TRY(workspace(c, "rh_lih", sizeof(u64) * (size_t)lin_nx * lin_ny, &p));
        d_lih = (u64*)p;
        IGM_HIP_CHECK(c, hipMemsetAsync(d_lih, 0, sizeof(u64) * (size_t)lin_nx * lin_ny, c->stream));
    }
    // integer statistics: {bad flag (one 8-byte slot), dense (P, 2), sparse (P, 2, 3)}
    const size_t nint = 1 + (size_t)P * 2 + (size_t)P * 6;
    IGM_TRY(workspace(c, "rh_ints", sizeof(u64) * nint, &p));
    u64* d_ints = (u64*)p;
    u64 *d_dense = d_ints + 1, *d_sparse = d_ints + 1 + (size_t)P * 2;
    IGM_HIP_CHECK(c, hipMemsetAsync(d_ints, 0, sizeof(u64) * nint, c->stream));
    IGM_TRY(workspace(c, "rh_rows", sizeof(double) * (size_t)nhap * 12, &p));
    double* d_rows = (double*)p;
    // float64 statistics: {sum x (P, 2 halves), means (P, 3, 2), centred (P, 3, 2)}
    IGM_TRY(workspace(c, "rh_f64", sizeof(double) * (size_t)P * 14, &p));
    double *d_sumx = (double*)p, *d_means = d_sumx + (size_t)P * 2, *d_cent = d_means + (size_t)P * 6;

    const unsigned grows = (unsigned)ceil_div(nhap, kHW);
    Timed tm(c, "report_hic");
    if (dev && nnz > 0) {
        hipLaunchKernelGGL(hic_check_kernel, dim3(grows), dim3(kHT), 0, c->stream, (const long long*)d_ptr, d_idx,
                           (int)nhap, (int*)d_ints);
        IGM_HIP_CHECK(c, hipGetLastError());
        int bad = 0;
        IGM_HIP_CHECK(c, hipMemcpyAsync(&bad, d_ints, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        IGM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
        if (bad & 1)
            return fail(c, IGM_E_INVALID, "%s: an entry lies below the diagonal (upper triangle expected)", fn);
        if (bad & 2) return fail(c, IGM_E_INVALID, "%s: a column index outside [0, %d)", fn, nhap);
    }
    hipLaunchKernelGGL(hic_dense_kernel, dim3((unsigned)nhap), dim3(kHT), 0, c->stream, d_counts, (int)nhap,
                       (int)nstruct, d_chrom, (int)nchrom, d_dense);
    IGM_HIP_CHECK(c, hipGetLastError());
    hipLaunchKernelGGL(hic_pass1_kernel, dim3(grows), dim3(kHT), 0, c->stream, d_counts, (int)nhap, (int)nstruct,
                       (const long long*)d_ptr, d_idx, d_data, d_chrom, (int)nchrom, sig_intra, sig_inter, d_sparse,
                       d_rows);
    IGM_HIP_CHECK(c, hipGetLastError());
    hipLaunchKernelGGL(hic_rows_kernel, dim3((unsigned)P), dim3(kHT), 0, c->stream, (const double*)d_rows, (int)nhap,
                       2, d_chrom, (int)nchrom, d_sumx);
    IGM_HIP_CHECK(c, hipGetLastError());
    const hipMemcpyKind d2h = hipMemcpyDeviceToHost;
    IGM_HIP_CHECK(c, hipMemcpyAsync(dense_sums, d_dense, sizeof(u64) * (size_t)P * 2, d2h, c->stream));
    IGM_HIP_CHECK(c, hipMemcpyAsync(sparse_ints, d_sparse, sizeof(u64) * (size_t)P * 6, d2h, c->stream));
    IGM_HIP_CHECK(c, hipMemcpyAsync(sparse_sumx, d_sumx, sizeof(double) * (size_t)P * 2, d2h, c->stream));
    IGM_HIP_CHECK(c, hipStreamSynchronize(c->stream));

    // the means of every (population, mask): ybar = sum c' / (n nstruct) from the integers,
    // correctly rounded; xbar = sum x / n, one float64 division; 0 for an empty set
    int64_t sq = 0;
    for (int k = 0; k < nchrom; ++k) sq += msize[k] * msize[k];
    for (int pi = 0; pi < P; ++pi) {
        const int64_t nall = pi < nchrom ? msize[pi] * msize[pi] : ((int64_t)nhap * nhap - sq) / 2;
        const int64_t* si = sparse_ints + (size_t)pi * 6;
        const int64_t n[3] = {nall, si[0], nall - si[0]};
        const int64_t sc[3] = {dense_sums[pi * 2], si[1], dense_sums[pi * 2] - si[1]};
        const double sx[3] = {sparse_sumx[pi * 2] + sparse_sumx[pi * 2 + 1], sparse_sumx[pi * 2],
                              sparse_sumx[pi * 2 + 1]};
        for (int m = 0; m < 3; ++m) {
            double* o = means + ((size_t)pi * 3 + m) * 2;
            o[0] = n[m] > 0 ? ratio_rn((uint64_t)sc[m], (uint64_t)n[m] * (uint64_t)nstruct) : 0.0;
            o[1] = n[m] > 0 ? sx[m] / (double)n[m] : 0.0;
        }
    }
    IGM_HIP_CHECK(c, hipMemcpyAsync(d_means, means, sizeof(double) * (size_t)P * 6, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(hic_pass2_kernel, dim3(grows), dim3(kHT), 0, c->stream, d_counts, (int)nhap, (int)nstruct,
                       (const long long*)d_ptr, d_idx, d_data, d_chrom, (int)nchrom, sig_intra, sig_inter,
                       (const double*)d_means, d_rows);
    IGM_HIP_CHECK(c, hipGetLastError());
    hipLaunchKernelGGL(hic_rows_kernel, dim3((unsigned)P), dim3(kHT), 0, c->stream, (const double*)d_rows, (int)nhap,
                       6, d_chrom, (int)nchrom, d_cent);
    IGM_HIP_CHECK(c, hipGetLastError());
    const unsigned ghist = (unsigned)std::min<int64_t>(grows, kHistGroups);
    if (log_hist && nnz > 0) {
        const int lds = (int64_t)log_nx * log_ny <= kMaxLdsHist ? log_nx * log_ny : 0;
        hipLaunchKernelGGL(hic_hist_kernel, dim3(ghist), dim3(kHT), sizeof(unsigned) * (size_t)lds, c->stream, d_counts,
                           (int)nhap, (int)nstruct, (const long long*)d_ptr, d_idx, d_data, d_lgx, (int)log_nx, d_lgy,
                           (int)log_ny, d_lgh, lds);
        IGM_HIP_CHECK(c, hipGetLastError());
    }
    if (lin_hist && nnz > 0) {
        const int lds = (int64_t)lin_nx * lin_ny <= kMaxLdsHist ? lin_nx * lin_ny : 0;
        hipLaunchKernelGGL(hic_hist_kernel, dim3(ghist), dim3(kHT), sizeof(unsigned) * (size_t)lds, c->stream, d_counts,
                           (int)nhap, (int)nstruct, (const long long*)d_ptr, d_idx, d_data, d_lix, (int)lin_nx, d_liy,
                           (int)lin_ny, d_lih, lds);
        IGM_HIP_CHECK(c, hipGetLastError());
    }
    IGM_HIP_CHECK(c, hipMemcpyAsync(centred, d_cent, sizeof(double) * (size_t)P * 6, hipMemcpyDeviceToHost, c->stream));
    if (log_hist)
        IGM_HIP_CHECK(c, hipMemcpyAsync(log_hist, d_lgh, sizeof(u64) * (size_t)log_nx * log_ny, hipMemcpyDeviceToHost,
                                        c->stream));
    if (lin_hist)
        IGM_HIP_CHECK(c, hipMemcpyAsync(lin_hist, d_lih, sizeof(u64) * (size_t)lin_nx * lin_ny, hipMemcpyDeviceToHost,
                                        c->stream));
    // the outputs and the small staged arrays are the caller's host memory: always wait
    IGM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    IGM_HIP_CHECK(c, hipGetLastError());
    return IGM_OK;
}
