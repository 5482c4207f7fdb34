// Population report on the GPU: the structural numbers of igm/report/*.py on the
// bead-major .hss population (nbead, nstruct, 3) f32 --
//   igm_report_levels        radials.py:15-39,69-87 and shells.py:9-43
//   igm_report_rg            radius_of_gyration.py:9-41
//   igm_report_lamina        damid.py:32-51
//   igm_report_distance_map  distance_map.py:5-22
// and, on an imaged nucleus (the maps of igm_mstep_set_volumes; this project's definitions,
// the reference has no such report) --
//   igm_report_map_levels    the level 1 - depth / depth scale, its means, density and shells
//   igm_report_map_lamina    contacts with the lamina of a nucleus map or with a body
// Compiled with -ffp-contract=off and the default correctly rounded f32 sqrt: every
// per-element value is the reference's NumPy expression operation by operation, and
// every floating-point sum has a fixed order (no floating-point atomics), so a rerun
// is bitwise equal.  Integer histograms use integer atomics (exact in any order).
#include <algorithm>
#include <cmath>

#include "exact_math.h"
#include "exp_map_depth.h"
#include "igm_ctx.h"

using namespace igm;

namespace {

constexpr int kRT = 256;          // threads per workgroup of the level / shell / lamina / tile kernels
constexpr int kLB = 32;           // beads per level tile
constexpr int kLS = 32;           // structures per level tile
constexpr int kMaxLdsBins = 1024; // density bins kept in LDS (more: global atomics)
constexpr int kMaxShell = 256;    // shells per call (boundary values live in LDS)
constexpr int kSelG = 8;          // boundaries selected / shells summed per scan of a structure
constexpr int kMaxLdsShellBins = 4096;

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

// sqrt(((x/a)^2 + (y/b)^2) + (z/c)^2) in f64: np.sqrt(np.sum(np.square(crd / semiaxes)))
__device__ __forceinline__ double level_of(float x, float y, float z, double a, double b, double c) {
    const double u = (double)x / a, v = (double)y / b, w = (double)z / c;
    return sqrt_rn((u * u + v * v) + w * w);
}

// Sum over the workgroup in a fixed order: the shuffle tree of every wave, then the
// waves in order.  The result is valid in thread 0.
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < kRT / 64; ++w) s += red[w];
    return s;
}

// The level source of pass 1 (compile time): what turns one (bead, structure) into its
// level.  stage() runs once per structure tile on the whole workgroup, before a barrier.
//   EllipsoidLevels  level_of on the semiaxes; no LDS, no depth
//   MapLevels        1 - depth / depth scale, clamped at 0, on the structure's staged map:
//                    the at most kLS map headers and scales of the tile sit in LDS, so a
//                    (bead, structure) costs one 16-byte voxel load
struct EllipsoidLevels {
    static constexpr bool kMap = false;
    double a, b, c;
    __device__ __forceinline__ void stage(int, int, int) const {}
    __device__ __forceinline__ double level(const float* p, int, double*) const {
        return level_of(p[0], p[1], p[2], a, b, c);
    }
};

struct MapLevels {
    static constexpr bool kMap = true;
    struct Lds {
        ms::VolMapDev map[kLS];
        double scale[kLS];
        double depth[kLB][kLS + 1];
    };
    const ms::VolMapDev* maps;
    const int4* vox;
    const int* smap;      // (S) map of each structure, or NULL: map 0
    const double* scale;  // (nmap) depth scale
    __device__ static __forceinline__ Lds& lds() {
        __shared__ Lds l;
        return l;
    }
    __device__ __forceinline__ void stage(int s0, int ns, int t) const {
        Lds& l = lds();
        if (t < ns) {
            const int m = smap ? smap[s0 + t] : 0;
            l.map[t] = maps[m];
            l.scale[t] = scale[m];
        }
    }
    __device__ __forceinline__ double level(const float* p, int q, double* depth) const {
        const Lds& l = lds();
        const float x[3] = {p[0], p[1], p[2]};
        const double d = exp_map_depth(x, l.map[q], vox);
        *depth = d;
        const double v = 1.0 - d / l.scale[q];
        return v > 0.0 ? v : 0.0;  // off the centre of a deep voxel depth > scale: the sign bit stays clear
    }
};

// Pass 1: a tile of kLB beads x kLS structures per step.  Levels go to lev (nstruct,
// nbead) through an LDS transpose (both the reads and the writes are coalesced), the
// per-bead sums run over the structures in order, the density counts collect in LDS.
// The map source also sums the signed depths per bead, in the same order.
template <class Src>
__global__ void __launch_bounds__(kRT) levels_kernel(const float* __restrict__ xyz, int n, int S, Src src,
                                                     double* __restrict__ lev, double* __restrict__ level_mean,
                                                     double* __restrict__ depth_mean,
                                                     const double* __restrict__ edges, int nbins,
                                                     u64* __restrict__ density) {
    __shared__ double tile[kLB][kLS + 1];
    __shared__ unsigned int hist[kMaxLdsBins];
    const int t = threadIdx.x, b0 = blockIdx.x * kLB;
    const bool lds_hist = density && nbins <= kMaxLdsBins;
    if (lds_hist)
        for (int k = t; k < nbins; k += kRT) hist[k] = 0;
    double sum = 0.0, dsum = 0.0;
    for (int s0 = 0; s0 < S; s0 += kLS) {
        const int ns = min(kLS, S - s0);
        __syncthreads();
        if constexpr (Src::kMap) {
            src.stage(s0, ns, t);
            __syncthreads();
        }
        for (int e = t; e < kLB * kLS; e += kRT) {
            const int r = e / kLS, q = e - r * kLS;
            double v = 0.0, dep = 0.0;
            if (b0 + r < n && q < ns) {
                const float* p = xyz + ((size_t)(b0 + r) * S + s0 + q) * 3;
                v = src.level(p, q, &dep);
                if (density) {
                    const int k = bin_of(edges, nbins, v);
                    if (k >= 0) {
                        if (lds_hist) atomicAdd(&hist[k], 1u);
                        else atomicAdd(&density[k], (u64)1);
                    }
                }
            }
            tile[r][q] = v;
            if constexpr (Src::kMap) Src::lds().depth[r][q] = dep;
        }
        __syncthreads();
        if (lev)
            for (int e = t; e < kLB * kLS; e += kRT) {
                const int q = e / kLB, r = e - q * kLB;
                if (b0 + r < n && q < ns) lev[(size_t)(s0 + q) * n + b0 + r] = tile[r][q];
            }
        if (t < kLB) {
            for (int q = 0; q < ns; ++q) sum += tile[t][q];
            if constexpr (Src::kMap)
                for (int q = 0; q < ns; ++q) dsum += Src::lds().depth[t][q];
        }
    }
    if (level_mean && t < kLB && b0 + t < n) level_mean[b0 + t] = sum / (double)S;
    if constexpr (Src::kMap)
        if (depth_mean && t < kLB && b0 + t < n) depth_mean[b0 + t] = dsum / (double)S;
    __syncthreads();
    if (lds_hist)
        for (int k = t; k < nbins; k += kRT)
            if (hist[k]) atomicAdd(&density[k], (u64)hist[k]);
}

// Pass 2: one workgroup per structure.  The nshell - 1 boundary ranks bds[1..nshell-1]
// are found by a radix select (8 bits a pass, kSelG boundaries a scan) on the bits of
// the non-negative doubles, which order like the values.  For boundary j the select
// leaves its value T[j], the number of levels below it and the number equal to it.
// A level that equals no boundary value belongs to shell #{j: T[j] < level}; the levels
// equal to a boundary value fill the shells in rank order (the lower shell first), which
// is all np.partition fixes: the multiset of every shell.
__global__ void __launch_bounds__(kRT) shells_kernel(const double* __restrict__ lev, int n, int nshell,
                                                     const int* __restrict__ bds, const double* __restrict__ hedges,
                                                     int hnbins, double* __restrict__ shell_mean,
                                                     u64* __restrict__ shell_hist, int lds_bins) {
    extern __shared__ unsigned int shist[];  // (nshell, hnbins) when lds_bins
    __shared__ unsigned int hist[kSelG][256];
    __shared__ u64 T[kMaxShell];
    __shared__ int cless[kMaxShell], ceq[kMaxShell];
    __shared__ u64 pref[kSelG];
    __shared__ int rem[kSelG], less[kSelG];
    __shared__ double ssum[kMaxShell];
    __shared__ double red[kRT / 64];
    const int t = threadIdx.x, s = blockIdx.x, nb = nshell - 1;
    const double* row = lev + (size_t)s * n;
    const bool want_hist = shell_hist != nullptr;
    if (want_hist && lds_bins)
        for (int k = t; k < lds_bins; k += kRT) shist[k] = 0;
    __syncthreads();

    for (int g0 = 0; g0 < nb; g0 += kSelG) {
        const int ng = min(kSelG, nb - g0);
        if (t < ng) {
            pref[t] = 0;
            rem[t] = bds[g0 + t + 1];
            less[t] = 0;
        }
        for (int pass = 0; pass < 8; ++pass) {
            const int shift = 56 - 8 * pass;
            for (int k = t; k < kSelG * 256; k += kRT) (&hist[0][0])[k] = 0;
            __syncthreads();
            for (int e = t; e < n; e += kRT) {
                const u64 key = (u64)__double_as_longlong(row[e]);
                const unsigned d = (unsigned)(key >> shift) & 255u;
                for (int q = 0; q < ng; ++q)
                    if (pass == 0 || (key >> (shift + 8)) == (pref[q] >> (shift + 8))) atomicAdd(&hist[q][d], 1u);
            }
            __syncthreads();
            if (t < ng) {
                int r = rem[t], cum = 0, d = 0;
                for (; d < 255; ++d) {
                    const int h = (int)hist[t][d];
                    if (r < cum + h) break;
                    cum += h;
                }
                pref[t] |= (u64)d << shift;
                rem[t] = r - cum;
                less[t] += cum;
                if (pass == 7) ceq[g0 + t] = (int)hist[t][d];
            }
            __syncthreads();
        }
        if (t < ng) {
            T[g0 + t] = pref[t];
            cless[g0 + t] = less[t];
        }
        __syncthreads();
    }

    for (int q0 = 0; q0 < nshell; q0 += kSelG) {
        double acc[kSelG];
#pragma unroll
        for (int g = 0; g < kSelG; ++g) acc[g] = 0.0;
        for (int e = t; e < n; e += kRT) {
            const double x = row[e];
            const u64 key = (u64)__double_as_longlong(x);
            int lo = 0, hi = nb;  // number of boundary values below key
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (T[mid] < key) lo = mid + 1;
                else hi = mid;
            }
            if (lo < nb && T[lo] == key) continue;  // a boundary value: placed by rank below
            if (q0 == 0 && want_hist) {
                const int k = bin_of(hedges, hnbins, x);
                if (k >= 0) {
                    if (lds_bins) atomicAdd(&shist[lo * hnbins + k], 1u);
                    else atomicAdd(&shell_hist[(size_t)lo * hnbins + k], (u64)1);
                }
            }
#pragma unroll
            for (int g = 0; g < kSelG; ++g) acc[g] += (lo == q0 + g) ? x : 0.0;
        }
#pragma unroll
        for (int g = 0; g < kSelG; ++g) {
            const double v = block_sum(acc[g], red);
            if (t == 0 && q0 + g < nshell) ssum[q0 + g] = v;
        }
    }
    __syncthreads();
    for (int q = t; q < nshell; q += kRT) {
        const int r0 = bds[q], r1 = bds[q + 1];
        double total = ssum[q];
        for (int j = 0; j < nb; ++j) {
            if (j > 0 && T[j] == T[j - 1]) continue;  // one turn per distinct boundary value
            const int c0 = cless[j], c1 = c0 + ceq[j];
            const int ov = min(c1, r1) - max(c0, r0);
            if (ov <= 0) continue;
            const double v = __longlong_as_double((long long)T[j]);
            total += (double)ov * v;
            if (want_hist) {
                const int k = bin_of(hedges, hnbins, v);
                if (k >= 0) {
                    if (lds_bins) atomicAdd(&shist[q * hnbins + k], (unsigned)ov);
                    else atomicAdd(&shell_hist[(size_t)q * hnbins + k], (u64)ov);
                }
            }
        }
        if (shell_mean) shell_mean[(size_t)s * nshell + q] = r1 > r0 ? total / (double)(r1 - r0) : (double)NAN;
    }
    __syncthreads();
    if (want_hist && lds_bins)
        for (int k = t; k < lds_bins; k += kRT)
            if (shist[k]) atomicAdd(&shell_hist[k], (u64)shist[k]);
}

// Threads over the structures (neighbouring lanes read neighbouring structures of one
// bead), a loop over the chain's beads: the mean, then the squared deviations, in f64
// in bead order.
__global__ void __launch_bounds__(64) rg_kernel(const float* __restrict__ xyz, int S,
                                                const int* __restrict__ chain_ptr,
                                                const int* __restrict__ chain_idx, double* __restrict__ rg) {
    const int ch = blockIdx.x, s = blockIdx.y * 64 + threadIdx.x;
    if (s >= S) return;
    const int p0 = chain_ptr[ch], p1 = chain_ptr[ch + 1];
    const double len = (double)(p1 - p0);
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int p = p0; p < p1; ++p) {
        const float* x = xyz + ((size_t)chain_idx[p] * S + s) * 3;
        sx += (double)x[0];
        sy += (double)x[1];
        sz += (double)x[2];
    }
    const double mx = sx / len, my = sy / len, mz = sz / len;
    double acc = 0.0;
    for (int p = p0; p < p1; ++p) {
        const float* x = xyz + ((size_t)chain_idx[p] * S + s) * 3;
        const double dx = (double)x[0] - mx, dy = (double)x[1] - my, dz = (double)x[2] - mz;
        acc += (dx * dx + dy * dy) + dz * dz;
    }
    rg[(size_t)ch * S + s] = sqrt_rn(acc / len);
}

// One workgroup per haploid locus: snormsq_ellipse (report/utils.py:73-89) of every copy
// in every structure as NumPy 2 evaluates it -- np.square in f32, the divisions and the
// sum in f64 -- counted against 1.
__global__ void __launch_bounds__(kRT) lamina_kernel(const float* __restrict__ xyz, int S,
                                                     const int* __restrict__ copy_ptr,
                                                     const int* __restrict__ copy_idx,
                                                     const double* __restrict__ denoms, long long* __restrict__ counts) {
    __shared__ int red[kRT / 64];
    const int h = blockIdx.x, t = threadIdx.x;
    const int p0 = copy_ptr[h], nc = copy_ptr[h + 1] - p0;
    const double A = denoms[(size_t)h * 3], B = denoms[(size_t)h * 3 + 1], C = denoms[(size_t)h * 3 + 2];
    int cnt = 0;
    for (int k = 0; k < nc; ++k) {
        const float* base = xyz + (size_t)copy_idx[p0 + k] * S * 3;
        for (int s = t; s < S; s += kRT) {
            const float x = base[s * 3], y = base[s * 3 + 1], z = base[s * 3 + 2];
            const double xx = (double)__fmul_rn(x, x), yy = (double)__fmul_rn(y, y), zz = (double)__fmul_rn(z, z);
            cnt += ((xx / A + yy / B) + zz / C) >= 1.0;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
    if ((t & 63) == 0) red[t >> 6] = cnt;
    __syncthreads();
    if (t == 0) {
        long long tot = 0;
        for (int w = 0; w < kRT / 64; ++w) tot += red[w];
        counts[h] = tot;
    }
}

// One workgroup per haploid locus on the staged maps: the signed depth of every copy in every
// structure below the lamina of the structure's map, less the radius of the locus's first
// copy, counted against the map's threshold.  side = +1 a nucleus map (contact towards
// the outside), -1 a body map (contact towards its inside).
__global__ void __launch_bounds__(kRT) map_lamina_kernel(const float* __restrict__ xyz, int S,
                                                         const int* __restrict__ copy_ptr,
                                                         const int* __restrict__ copy_idx,
                                                         const float* __restrict__ radii,
                                                         const ms::VolMapDev* __restrict__ maps,
                                                         const int4* __restrict__ vox, const int* __restrict__ smap,
                                                         const double* __restrict__ thr, int side,
                                                         long long* __restrict__ counts) {
    __shared__ int red[kRT / 64];
    const int h = blockIdx.x, t = threadIdx.x;
    const int p0 = copy_ptr[h], nc = copy_ptr[h + 1] - p0;
    const double r = nc > 0 ? (double)radii[copy_idx[p0]] : 0.0;
    int cnt = 0;
#pragma unroll 1
    for (int s = t; s < S; s += kRT) {
        const int mi = smap ? smap[s] : 0;
        const ms::VolMapDev m = maps[mi];
        const double th = thr[mi];
#pragma unroll 1
        for (int k = 0; k < nc; ++k) {
            const float* x = xyz + ((size_t)copy_idx[p0 + k] * S + s) * 3;
            const float p[3] = {x[0], x[1], x[2]};
            const double d = exp_map_depth(p, m, vox);
            cnt += ((side > 0 ? d : -d) - r) <= th;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
    if ((t & 63) == 0) red[t >> 6] = cnt;
    __syncthreads();
    if (t == 0) {
        long long tot = 0;
        for (int w = 0; w < kRT / 64; ++w) tot += red[w];
        counts[h] = tot;
    }
}

// Average distance map.  One workgroup per 64x64 tile of haploid loci (upper-triangle
// tiles), a 4x4 block of entries per thread.  The outer loops run over the copy ranks
// (ka, kb): a pass streams the ka-th copies of the tile's rows and the kb-th copies of
// its columns through LDS in chunks of kDS structures (the staging of contact_map_kernel)
// and adds the f32 norms in f64 in structure order; at the end of the pass the entries
// whose copy pair exists -- and, on one chromosome, has ka == kb (the reference's zip) --
// take mean = sum / nstruct into their sum of means.  A pass no entry of the tile needs
// is skipped by the whole workgroup.
constexpr int kDT = 64;
constexpr int kDS = 32;
constexpr int kDRow = kDS * 3 + 1;

__global__ void __launch_bounds__(kRT) distance_map_kernel(const float* __restrict__ xyz, int S, int nhap,
                                                           const int* __restrict__ copy_ptr,
                                                           const int* __restrict__ copy_idx,
                                                           const int* __restrict__ hap_chrom, int maxc,
                                                           double* __restrict__ dmap) {
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bj < bi) return;  // the whole workgroup leaves together
    __shared__ float li[kDT * kDRow];
    __shared__ float lj[kDT * kDRow];
    __shared__ int beadi[kDT], beadj[kDT];
    const int t = threadIdx.x, ti = t >> 4, tj = t & 15;
    const int i0 = bi * kDT, j0 = bj * kDT;
    int nci[4], ncj[4], chi[4], chj[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int i = i0 + ti * 4 + a, j = j0 + tj * 4 + a;
        nci[a] = i < nhap ? copy_ptr[i + 1] - copy_ptr[i] : 0;
        ncj[a] = j < nhap ? copy_ptr[j + 1] - copy_ptr[j] : 0;
        chi[a] = i < nhap ? hap_chrom[i] : -1;
        chj[a] = j < nhap ? hap_chrom[j] : -2;
    }
    double acc[4][4];
    int cnt[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            acc[a][b] = 0.0;
            cnt[a][b] = 0;
        }
    for (int ka = 0; ka < maxc; ++ka)
        for (int kb = 0; kb < maxc; ++kb) {
            unsigned valid = 0;
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (ka < nci[a] && kb < ncj[b] && (chi[a] != chj[b] || ka == kb) &&
                        i0 + ti * 4 + a < j0 + tj * 4 + b)
                        valid |= 1u << (a * 4 + b);
            if (!__syncthreads_or((int)valid)) continue;
            if (t < kDT) {
                const int i = i0 + t;
                beadi[t] = (i < nhap && ka < copy_ptr[i + 1] - copy_ptr[i]) ? copy_idx[copy_ptr[i] + ka] : -1;
            } else if (t < 2 * kDT) {
                const int j = j0 + t - kDT;
                beadj[t - kDT] = (j < nhap && kb < copy_ptr[j + 1] - copy_ptr[j]) ? copy_idx[copy_ptr[j] + kb] : -1;
            }
            double sum[4][4];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) sum[a][b] = 0.0;
            for (int s0 = 0; s0 < S; s0 += kDS) {
                const int ns = min(kDS, S - s0), w = ns * 3;
                __syncthreads();
                for (int e = t; e < kDT * kDS * 3; e += kRT) {
                    const int r = e / (kDS * 3), c = e - r * (kDS * 3);
                    float vi = 0.f, vj = 0.f;
                    if (c < w) {
                        const int gi = beadi[r], gj = beadj[r];
                        if (gi >= 0) vi = xyz[((size_t)gi * S + s0) * 3 + c];
                        if (gj >= 0) vj = xyz[((size_t)gj * S + s0) * 3 + c];
                    }
                    li[r * kDRow + c] = vi;
                    lj[r * kDRow + c] = vj;
                }
                __syncthreads();
#pragma unroll 1
                for (int s = 0; s < ns; ++s) {
                    float xi[4][3], xj[4][3];
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            xi[a][k] = li[(ti * 4 + a) * kDRow + s * 3 + k];
                            xj[a][k] = lj[(tj * 4 + a) * kDRow + s * 3 + k];
                        }
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int b = 0; b < 4; ++b) {
                            const float dx = __fsub_rn(xi[a][0], xj[b][0]), dy = __fsub_rn(xi[a][1], xj[b][1]),
                                        dz = __fsub_rn(xi[a][2], xj[b][2]);
                            const float d2 =
                                __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
                            sum[a][b] += (double)__builtin_sqrtf(d2);  // correctly rounded (default lowering)
                        }
                }
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (valid >> (a * 4 + b) & 1u) {
                        acc[a][b] += sum[a][b] / (double)S;
                        ++cnt[a][b];
                    }
        }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int i = i0 + ti * 4 + a;
        if (i >= nhap) continue;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int j = j0 + tj * 4 + b;
            if (j >= nhap || j < i) continue;
            if (i == j) {
                dmap[(size_t)i * nhap + i] = 0.0;
                continue;
            }
            const double v = cnt[a][b] > 0 ? acc[a][b] / (double)cnt[a][b] : (double)NAN;
            dmap[(size_t)i * nhap + j] = v;
            dmap[(size_t)j * nhap + i] = v;
        }
    }
}

// host checks shared by the entry points -------------------------------------------------
int check_csr(igm_ctx* c, const char* fn, const char* what, const int32_t* ptr, const int32_t* idx, int nrow,
              int nbead, int* max_len) {
    if (ptr[0] != 0) return fail(c, IGM_E_INVALID, "%s: %s_ptr[0] = %d, expected 0", fn, what, ptr[0]);
    int ml = 0;
    for (int r = 0; r < nrow; ++r) {
        if (ptr[r + 1] < ptr[r])
            return fail(c, IGM_E_INVALID, "%s: %s_ptr decreases at row %d (%d -> %d)", fn, what, r, ptr[r], ptr[r + 1]);
        ml = std::max(ml, ptr[r + 1] - ptr[r]);
    }
    for (int k = 0; k < ptr[nrow]; ++k)
        if (idx[k] < 0 || idx[k] >= nbead)
            return fail(c, IGM_E_INVALID, "%s: %s_idx[%d] = %d outside [0, %d)", fn, what, k, idx[k], nbead);
    if (max_len) *max_len = ml;
    return IGM_OK;
}

int check_edges(igm_ctx* c, const char* fn, const char* what, const double* e, int nbins) {
    for (int k = 0; k <= nbins; ++k)
        if (!std::isfinite(e[k])) return fail(c, IGM_E_INVALID, "%s: %s[%d] is not finite", fn, what, k);
    for (int k = 0; k < nbins; ++k)
        if (e[k + 1] < e[k])
            return fail(c, IGM_E_INVALID, "%s: %s not sorted at %d (%.17g > %.17g)", fn, what, k, e[k], e[k + 1]);
    return IGM_OK;
}

// the density and shell arguments shared by igm_report_levels and igm_report_map_levels
struct LevelOutputs {
    double* level_mean;
    const double* density_edges;
    int32_t nbins;
    int64_t* density_counts;
    int32_t nshell;
    double* shell_mean;
    const double* shell_edges;
    int32_t hnbins;
    int64_t* shell_hist;
};

int check_level_outputs(igm_ctx* c, const char* fn, const LevelOutputs& o) {
    if (o.density_counts) {
        if (o.nbins < 1 || !o.density_edges)
            return fail(c, IGM_E_INVALID, "%s: density_counts needs nbins >= 1 (%d) and nbins + 1 edges", fn, o.nbins);
        IGM_TRY(check_edges(c, fn, "density_edges", o.density_edges, o.nbins));
    }
    if (o.shell_mean || o.shell_hist) {
        if (o.nshell < 1) return fail(c, IGM_E_INVALID, "%s: nshell = %d, expected >= 1", fn, o.nshell);
        if (o.nshell > kMaxShell)
            return fail(c, IGM_E_UNSUPPORTED, "%s: nshell = %d, at most %d supported", fn, o.nshell, kMaxShell);
        if (o.shell_hist) {
            if (o.hnbins < 1 || !o.shell_edges)
                return fail(c, IGM_E_INVALID, "%s: shell_hist needs hnbins >= 1 (%d) and hnbins + 1 edges", fn,
                            o.hnbins);
            IGM_TRY(check_edges(c, fn, "shell_edges", o.shell_edges, o.hnbins));
        }
    }
    return IGM_OK;
}

// Both passes on checked arguments: the levels of `src` (its device pointers already
// set), then the shells on the stored levels.  depth_mean: the map source's extra output.
template <class Src>
int run_levels(igm_ctx* c, uint32_t flags, const char* timer, const float* xyz, int32_t nbead, int32_t nstruct,
               const Src& src, double* depth_mean, const LevelOutputs& o) {
    double* const level_mean = o.level_mean;
    int64_t *const density_counts = o.density_counts, *const shell_hist = o.shell_hist;
    double* const shell_mean = o.shell_mean;
    const int32_t nbins = o.nbins, nshell = o.nshell, hnbins = o.hnbins;
    const bool shells = shell_mean || shell_hist;
    const float* d_xyz;
    IGM_TRY(to_device(c, flags, "rp_xyz", xyz, (size_t)nbead * nstruct * 3, &d_xyz));
    const double *d_edges = nullptr, *d_hedges = nullptr;
    if (density_counts) IGM_TRY(to_device(c, 0u, "rp_edges", o.density_edges, (size_t)nbins + 1, &d_edges));
    if (shell_hist) IGM_TRY(to_device(c, 0u, "rp_hedges", o.shell_edges, (size_t)hnbins + 1, &d_hedges));
    double *d_mean, *d_smean, *d_dmean;
    int64_t *d_dens, *d_shist;
    IGM_TRY(out_device(c, flags, "rp_mean", level_mean, (size_t)nbead, &d_mean));
    IGM_TRY(out_device(c, flags, "rp_dmean", depth_mean, (size_t)nbead, &d_dmean));
    IGM_TRY(out_device(c, flags, "rp_dens", density_counts, (size_t)nbins, &d_dens));
    IGM_TRY(out_device(c, flags, "rp_smean", shell_mean, (size_t)nstruct * (shells ? nshell : 0), &d_smean));
    IGM_TRY(out_device(c, flags, "rp_shist", shell_hist, (size_t)(shells ? nshell : 0) * hnbins, &d_shist));
    double* d_lev = nullptr;
    const int* d_bds = nullptr;
    if (shells) {
        void* p;
        IGM_TRY(workspace(c, "rp_lev", sizeof(double) * (size_t)nbead * nstruct, &p));
        d_lev = (double*)p;
        // the shell boundaries as the reference computes them: int(j * n / nshell), a float64 division
        std::vector<int> bds(nshell + 1);
        for (int j = 0; j < nshell; ++j) bds[j] = (int)((double)((int64_t)j * nbead) / (double)nshell);
        bds[nshell] = nbead;
        IGM_TRY(to_device(c, 0u, "rp_bds", (const int*)bds.data(), bds.size(), &d_bds));
        IGM_HIP_CHECK(c, hipStreamSynchronize(c->stream));  // bds dies here
    }
    if (density_counts) IGM_HIP_CHECK(c, hipMemsetAsync(d_dens, 0, sizeof(int64_t) * (size_t)nbins, c->stream));
    if (shell_hist) IGM_HIP_CHECK(c, hipMemsetAsync(d_shist, 0, sizeof(int64_t) * (size_t)nshell * hnbins, c->stream));
    {
        Timed tm(c, timer);
        if (level_mean || depth_mean || density_counts || shells) {
            hipLaunchKernelGGL(levels_kernel<Src>, dim3((unsigned)ceil_div(nbead, kLB)), dim3(kRT), 0, c->stream, d_xyz,
                               (int)nbead, (int)nstruct, src, d_lev, d_mean, d_dmean, d_edges, (int)nbins,
                               (u64*)d_dens);
            IGM_HIP_CHECK(c, hipGetLastError());
        }
        if (shells) {
            const int lds_bins = shell_hist && (int64_t)nshell * hnbins <= kMaxLdsShellBins ? nshell * hnbins : 0;
            hipLaunchKernelGGL(shells_kernel, dim3((unsigned)nstruct), dim3(kRT), sizeof(unsigned) * (size_t)lds_bins,
                               c->stream, (const double*)d_lev, (int)nbead, (int)nshell, d_bds, d_hedges, (int)hnbins,
                               d_smean, (u64*)d_shist, lds_bins);
            IGM_HIP_CHECK(c, hipGetLastError());
        }
    }
    IGM_TRY(to_host(c, flags, level_mean, d_mean, (size_t)nbead));
    IGM_TRY(to_host(c, flags, depth_mean, d_dmean, (size_t)nbead));
    IGM_TRY(to_host(c, flags, density_counts, d_dens, (size_t)nbins));
    if (shells) {
        IGM_TRY(to_host(c, flags, shell_mean, d_smean, (size_t)nstruct * nshell));
        IGM_TRY(to_host(c, flags, shell_hist, d_shist, (size_t)nshell * hnbins));
    }
    return finish(c, flags);
}

// The staged maps and the map index of every structure of a call, on the device: smap is
// the caller's struct_map (host, checked against the pool), else the table staged with the
// maps (which must cover the call), else NULL for map 0 -- igm_volume_select's convention.
struct StagedMaps {
    const ms::VolMapDev* maps;
    const int4* vox;
    const int* smap;
};

int staged_maps(igm_ctx* c, const char* fn, const int32_t* struct_map, int32_t nstruct, StagedMaps* out) {
    if (c->vol_nmap <= 0) return fail(c, IGM_E_INVALID, "%s: no map staged (igm_mstep_set_volumes)", fn);
    if (struct_map) {
        for (int s = 0; s < nstruct; ++s)
            if (struct_map[s] < 0 || struct_map[s] >= c->vol_nmap)
                return fail(c, IGM_E_INVALID, "%s: struct_map[%d] = %d outside [0, %d)", fn, s, struct_map[s],
                            c->vol_nmap);
    } else if (c->vol_nsmap > 0 && c->vol_nsmap < nstruct) {
        return fail(c, IGM_E_INVALID, "%s: volume map index staged for %d structures, batch has %d", fn, c->vol_nsmap,
                    nstruct);
    }
    IGM_HIP_CHECK(c, hipSetDevice(c->device));
    void *pm, *pv, *ps;
    IGM_TRY(workspace(c, "vol_maps", 1, &pm));
    IGM_TRY(workspace(c, "vol_vox", 1, &pv));
    out->maps = (const ms::VolMapDev*)pm;
    out->vox = (const int4*)pv;
    out->smap = nullptr;
    if (struct_map) {
        IGM_TRY(to_device(c, 0u, "rp_smap", struct_map, (size_t)nstruct, &out->smap));
    } else if (c->vol_nsmap > 0) {
        IGM_TRY(workspace(c, "vol_smap", 1, &ps));
        out->smap = (const int*)ps;
    }
    return IGM_OK;
}

}  // namespace

extern "C" int igm_report_levels(igm_ctx* c, uint32_t flags, const float* xyz, int32_t nbead, int32_t nstruct,
                                 const double* semiaxes, double* level_mean, const double* density_edges,
                                 int32_t nbins, int64_t* density_counts, int32_t nshell, double* shell_mean,
                                 const double* shell_edges, int32_t hnbins, int64_t* shell_hist) {
    static const char* fn = "igm_report_levels";
    if (!c) return IGM_E_INVALID;
    if (nbead <= 0 || nstruct <= 0 || !xyz || !semiaxes)
        return fail(c, IGM_E_INVALID, "%s: invalid arguments (nbead %d, nstruct %d, xyz %p, semiaxes %p)", fn, nbead,
                    nstruct, (const void*)xyz, (const void*)semiaxes);
    if (nbead > 65535) return fail(c, IGM_E_UNSUPPORTED, "%s: %d beads, at most 65535 supported", fn, nbead);
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(semiaxes[k]) || !(semiaxes[k] > 0.0))
            return fail(c, IGM_E_INVALID, "%s: semiaxes[%d] = %g is not a positive finite number", fn, k, semiaxes[k]);
    const LevelOutputs o{level_mean, density_edges, nbins, density_counts, nshell, shell_mean, shell_edges, hnbins,
                         shell_hist};
    IGM_TRY(check_level_outputs(c, fn, o));
    IGM_HIP_CHECK(c, hipSetDevice(c->device));
    const EllipsoidLevels src{semiaxes[0], semiaxes[1], semiaxes[2]};
    return run_levels(c, flags, "report_levels", xyz, nbead, nstruct, src, nullptr, o);
}

extern "C" int igm_report_map_levels(igm_ctx* c, uint32_t flags, const float* xyz, int32_t nbead, int32_t nstruct,
                                     const int32_t* struct_map, const double* depth_scale, double* level_mean,
                                     double* depth_mean, const double* density_edges, int32_t nbins,
                                     int64_t* density_counts, int32_t nshell, double* shell_mean,
                                     const double* shell_edges, int32_t hnbins, int64_t* shell_hist) {
    static const char* fn = "igm_report_map_levels";
    if (!c) return IGM_E_INVALID;
    if (nbead <= 0 || nstruct <= 0 || !xyz || !depth_scale)
        return fail(c, IGM_E_INVALID, "%s: invalid arguments (nbead %d, nstruct %d, xyz %p, depth_scale %p)", fn, nbead,
                    nstruct, (const void*)xyz, (const void*)depth_scale);
    if (nbead > 65535) return fail(c, IGM_E_UNSUPPORTED, "%s: %d beads, at most 65535 supported", fn, nbead);
    for (int m = 0; m < c->vol_nmap; ++m)
        if (!std::isfinite(depth_scale[m]) || !(depth_scale[m] > 0.0))
            return fail(c, IGM_E_INVALID, "%s: depth_scale[%d] = %g is not a positive finite number", fn, m,
                        depth_scale[m]);
    const LevelOutputs o{level_mean, density_edges, nbins, density_counts, nshell, shell_mean, shell_edges, hnbins,
                         shell_hist};
    IGM_TRY(check_level_outputs(c, fn, o));
    StagedMaps sm;
    IGM_TRY(staged_maps(c, fn, struct_map, nstruct, &sm));
    const double* d_scale;
    IGM_TRY(to_device(c, 0u, "rp_scale", depth_scale, (size_t)c->vol_nmap, &d_scale));
    // struct_map and depth_scale are the caller's and were copied asynchronously: wait before going on
    IGM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    const MapLevels src{sm.maps, sm.vox, sm.smap, d_scale};
    return run_levels(c, flags, "report_map_levels", xyz, nbead, nstruct, src, depth_mean, o);
}

extern "C" int igm_report_rg(igm_ctx* c, uint32_t flags, const float* xyz, int32_t nbead, int32_t nstruct,
                             const int32_t* chain_ptr, const int32_t* chain_idx, int32_t nchain, double* rg) {
    static const char* fn = "igm_report_rg";
    if (!c) return IGM_E_INVALID;
    if (nbead <= 0 || nstruct <= 0 || nchain <= 0 || !xyz || !chain_ptr || !chain_idx || !rg)
        return fail(c, IGM_E_INVALID, "%s: invalid arguments (nbead %d, nstruct %d, nchain %d)", fn, nbead, nstruct,
                    nchain);
    IGM_TRY(check_csr(c, fn, "chain", chain_ptr, chain_idx, nchain, nbead, nullptr));
    const int64_t gy = ceil_div(nstruct, 64);
    if (gy > 65535) return fail(c, IGM_E_UNSUPPORTED, "%s: %d structures exceed the grid", fn, nstruct);
    IGM_HIP_CHECK(c, hipSetDevice(c->device));
    const float* d_xyz;
    const int32_t *d_ptr, *d_idx;
    IGM_TRY(to_device(c, flags, "rp_xyz", xyz, (size_t)nbead * nstruct * 3, &d_xyz));
    IGM_TRY(to_device(c, 0u, "rp_cptr", chain_ptr, (size_t)nchain + 1, &d_ptr));
    IGM_TRY(to_device(c, 0u, "rp_cidx", chain_idx, (size_t)chain_ptr[nchain], &d_idx));
    double* d_rg;
    IGM_TRY(out_device(c, flags, "rp_rg", rg, (size_t)nchain * nstruct, &d_rg));
    {
        Timed tm(c, "report_rg");
        hipLaunchKernelGGL(rg_kernel, dim3((unsigned)nchain, (unsigned)gy), dim3(64), 0, c->stream, d_xyz,
                           (int)nstruct, d_ptr, d_idx, d_rg);
        IGM_HIP_CHECK(c, hipGetLastError());
    }
    IGM_TRY(to_host(c, flags, rg, d_rg, (size_t)nchain * nstruct));
    // the CSR arrays are the caller's and were copied asynchronously: wait before returning
    IGM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return finish(c, flags);
}

extern "C" int igm_report_lamina(igm_ctx* c, uint32_t flags, const float* xyz, int32_t nbead, int32_t nstruct,
                                 const int32_t* copy_ptr, const int32_t* copy_idx, int32_t nhap,
                                 const double* inv_denoms, int64_t* counts) {
    static const char* fn = "igm_report_lamina";
    if (!c) return IGM_E_INVALID;
    if (nbead <= 0 || nstruct <= 0 || nhap <= 0 || !xyz || !copy_ptr || !copy_idx || !inv_denoms || !counts)
        return fail(c, IGM_E_INVALID, "%s: invalid arguments (nbead %d, nstruct %d, nhap %d)", fn, nbead, nstruct, nhap);
    IGM_TRY(check_csr(c, fn, "copy", copy_ptr, copy_idx, nhap, nbead, nullptr));
    for (size_t k = 0; k < (size_t)nhap * 3; ++k)
        if (std::isnan(inv_denoms[k]) || inv_denoms[k] < 0.0)
            return fail(c, IGM_E_INVALID, "%s: inv_denoms[%zu, %zu] = %g is negative or NaN", fn, k / 3, k % 3,
                        inv_denoms[k]);
    IGM_HIP_CHECK(c, hipSetDevice(c->device));
    const float* d_xyz;
    const int32_t *d_ptr, *d_idx;
    const double* d_den;
    IGM_TRY(to_device(c, flags, "rp_xyz", xyz, (size_t)nbead * nstruct * 3, &d_xyz));
    IGM_TRY(to_device(c, 0u, "rp_cptr", copy_ptr, (size_t)nhap + 1, &d_ptr));
    IGM_TRY(to_device(c, 0u, "rp_cidx", copy_idx, (size_t)copy_ptr[nhap], &d_idx));
    IGM_TRY(to_device(c, 0u, "rp_den", inv_denoms, (size_t)nhap * 3, &d_den));
    int64_t* d_cnt;
    IGM_TRY(out_device(c, flags, "rp_lam", counts, (size_t)nhap, &d_cnt));
    {
        Timed tm(c, "report_lamina");
        hipLaunchKernelGGL(lamina_kernel, dim3((unsigned)nhap), dim3(kRT), 0, c->stream, d_xyz, (int)nstruct, d_ptr,
                           d_idx, d_den, (long long*)d_cnt);
        IGM_HIP_CHECK(c, hipGetLastError());
    }
    IGM_TRY(to_host(c, flags, counts, d_cnt, (size_t)nhap));
    IGM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return finish(c, flags);
}

extern "C" int igm_report_map_lamina(igm_ctx* c, uint32_t flags, const float* xyz, int32_t nbead, int32_t nstruct,
                                     const int32_t* copy_ptr, const int32_t* copy_idx, int32_t nhap,
                                     const float* radii, const int32_t* struct_map, const double* thr, int32_t side,
                                     int64_t* counts) {
    static const char* fn = "igm_report_map_lamina";
    if (!c) return IGM_E_INVALID;
    if (nbead <= 0 || nstruct <= 0 || nhap <= 0 || !xyz || !copy_ptr || !copy_idx || !radii || !thr || !counts)
        return fail(c, IGM_E_INVALID, "%s: invalid arguments (nbead %d, nstruct %d, nhap %d)", fn, nbead, nstruct, nhap);
    if (side != 1 && side != -1) return fail(c, IGM_E_INVALID, "%s: side = %d, expected +1 or -1", fn, side);
    IGM_TRY(check_csr(c, fn, "copy", copy_ptr, copy_idx, nhap, nbead, nullptr));
    for (int m = 0; m < c->vol_nmap; ++m)
        if (!std::isfinite(thr[m])) return fail(c, IGM_E_INVALID, "%s: thr[%d] = %g is not finite", fn, m, thr[m]);
    StagedMaps sm;
    IGM_TRY(staged_maps(c, fn, struct_map, nstruct, &sm));
    const float *d_xyz, *d_radii;
    const int32_t *d_ptr, *d_idx;
    const double* d_thr;
    IGM_TRY(to_device(c, flags, "rp_xyz", xyz, (size_t)nbead * nstruct * 3, &d_xyz));
    IGM_TRY(to_device(c, 0u, "rp_cptr", copy_ptr, (size_t)nhap + 1, &d_ptr));
    IGM_TRY(to_device(c, 0u, "rp_cidx", copy_idx, (size_t)copy_ptr[nhap], &d_idx));
    IGM_TRY(to_device(c, 0u, "rp_radii", radii, (size_t)nbead, &d_radii));
    IGM_TRY(to_device(c, 0u, "rp_thr", thr, (size_t)c->vol_nmap, &d_thr));
    int64_t* d_cnt;
    IGM_TRY(out_device(c, flags, "rp_lam", counts, (size_t)nhap, &d_cnt));
    {
        Timed tm(c, "report_map_lamina");
        hipLaunchKernelGGL(map_lamina_kernel, dim3((unsigned)nhap), dim3(kRT), 0, c->stream, d_xyz, (int)nstruct, d_ptr,
                           d_idx, d_radii, sm.maps, sm.vox, sm.smap, d_thr, (int)side, (long long*)d_cnt);
        IGM_HIP_CHECK(c, hipGetLastError());
    }
    IGM_TRY(to_host(c, flags, counts, d_cnt, (size_t)nhap));
    // the host arrays are the caller's and were copied asynchronously: wait before returning
    IGM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return finish(c, flags);
}

extern "C" int igm_report_distance_map(igm_ctx* c, uint32_t flags, const float* xyz, int32_t nbead, int32_t nstruct,
                                       const int32_t* copy_ptr, const int32_t* copy_idx, const int32_t* hap_chrom,
                                       int32_t nhap, double* dmap) {
    static const char* fn = "igm_report_distance_map";
    if (!c) return IGM_E_INVALID;
    if (nbead <= 0 || nstruct <= 0 || nhap <= 0 || !xyz || !copy_ptr || !copy_idx || !hap_chrom || !dmap)
        return fail(c, IGM_E_INVALID, "%s: invalid arguments (nbead %d, nstruct %d, nhap %d)", fn, nbead, nstruct, nhap);
    int maxc = 0;
    IGM_TRY(check_csr(c, fn, "copy", copy_ptr, copy_idx, nhap, nbead, &maxc));
    const int nt = (int)ceil_div(nhap, kDT);
    if (nt > 65535) return fail(c, IGM_E_UNSUPPORTED, "%s: %d loci exceed the tile grid", fn, nhap);
    IGM_HIP_CHECK(c, hipSetDevice(c->device));
    const float* d_xyz;
    const int32_t *d_ptr, *d_idx, *d_chrom;
    IGM_TRY(to_device(c, flags, "rp_xyz", xyz, (size_t)nbead * nstruct * 3, &d_xyz));
    IGM_TRY(to_device(c, 0u, "rp_cptr", copy_ptr, (size_t)nhap + 1, &d_ptr));
    IGM_TRY(to_device(c, 0u, "rp_cidx", copy_idx, (size_t)copy_ptr[nhap], &d_idx));
    IGM_TRY(to_device(c, 0u, "rp_hchr", hap_chrom, (size_t)nhap, &d_chrom));
    double* d_map;
    IGM_TRY(out_device(c, flags, "rp_dmap", dmap, (size_t)nhap * nhap, &d_map));
    {
        Timed tm(c, "report_distance_map");
        hipLaunchKernelGGL(distance_map_kernel, dim3((unsigned)nt, (unsigned)nt), dim3(kRT), 0, c->stream, d_xyz,
                           (int)nstruct, (int)nhap, d_ptr, d_idx, d_chrom, maxc, d_map);
        IGM_HIP_CHECK(c, hipGetLastError());
    }
    IGM_TRY(to_host(c, flags, dmap, d_map, (size_t)nhap * nhap));
    IGM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return finish(c, flags);
}
