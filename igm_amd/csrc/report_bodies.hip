// Nuclear bodies from seed loci (igm_report_seed_bodies, igm_report_body_features,
// include/igm_hip.h): in every structure the seeds that gather within link_cutoff of one
// another form a body (the connected components of the link graph, single linkage), and
// every bead gets its distance to the nearest body, an association count and the TSA-seq
// signal the population predicts.  The definitions are this project's (the reference has no
// such report); single linkage stands in for the Markov clustering of the published recipe,
// which has no order-independent answer.
//
// Components.  One workgroup per structure.  Every seed owns 16 B of dynamic LDS: its three
// float32 coordinates and one word, its parent in a union-find forest.  The pairs (p, q < p)
// are cut into tiles of kRows x kQ that the waves take in turn: a lane holds kRR seeds p in
// registers and reads q as a broadcast.  A linked pair hooks the larger of the two roots
// under the smaller with an LDS compare-and-swap, so a parent is always below its child and
// a root is the smallest rank of its tree: the labels do not depend on the order of the
// work.  Every loop is bounded by nseed (a walk to the root descends strictly, and after a
// lost compare-and-swap the larger root is strictly smaller than before); nothing waits on
// another workgroup.  After one pass over the pairs the trees are flattened, the members
// counted into the upper half of the root's word (integer LDS atomics), the bodies numbered
// in ascending label by a ballot prefix, and one thread per body walks the labels in rank
// order -- every lane reads the same LDS word, a broadcast -- adding its members in float64:
// the fixed summation order.
//
// Features.  The census kernel's lane layout: a wave is 64 consecutive structures of its
// beads (768 contiguous bytes per bead), a workgroup of 4 waves owns kFB = 32 beads (8 per
// wave, in registers) and walks the structures in chunks of 64.  A lane's bodies are not its
// neighbour's: the centres lie in a transposed plane (body, structure, 3), so the lanes of a
// wave read neighbouring addresses, and the loop runs to the wave's largest body count.  The
// nearest distance and t(p, s) of a chunk go to LDS tiles and four threads per bead add them
// in structure order (the reduction of report.hip's level_mean): a rerun is bitwise equal.
//
// Compiled with -ffp-contract=off.  No float atomics anywhere.
#include <algorithm>
#include <cmath>
#include <vector>

#include "exact_math.h"
#include "igm_ctx.h"

using namespace igm;

namespace {

constexpr int kMaxSeeds = 8192;          // 16 B of LDS each: 128 KB
constexpr int kCT = 1024;                // threads of the component kernel: 16 waves
constexpr int kCW = kCT / 64;
constexpr int kSPT = kMaxSeeds / kCT;    // seeds per thread in the per-seed phases
constexpr int kRR = 4;                   // seeds p per lane in the pair pass
constexpr int kRows = 64 * kRR;          // seeds p per tile
constexpr int kQ = 128;                  // seeds q per tile: kRows / kQ tiles per diagonal block
constexpr int kLabelMask = 0xffff;       // a seed's word: label (< 8192) | members << 16 (at the root)

__device__ __forceinline__ int word_load(const int* w) {
    return __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The root of a's tree, halving the path on the way.  A parent is below its child, so the
// walk ends within n steps.  Only a seed that has a parent is written, with one of its
// ancestors, which stays an ancestor: concurrent walks and hooks see a valid forest.
__device__ __forceinline__ int find_root(int* par, int a, int n) {
    for (int it = 0; it < n; ++it) {
        const int pa = word_load(par + 4 * a);
        if (pa == a) break;
        const int g = word_load(par + 4 * pa);
        if (g != pa) __hip_atomic_store(par + 4 * a, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        a = g;
    }
    return a;
}

// the same walk without a store (the flattening pass reads a forest that no longer changes)
__device__ __forceinline__ int root_of(const int* par, int a, int n) {
    for (int it = 0; it < n; ++it) {
        const int pa = word_load(par + 4 * a);
        if (pa == a) break;
        a = pa;
    }
    return a;
}

// Hook the larger root of a and b under the smaller.  A compare-and-swap that loses found
// the larger root hooked by somebody else: the walk goes on from its new parent, and the
// larger of the two roots is then strictly smaller than before, so n rounds suffice.
__device__ __forceinline__ void unite(int* par, int a, int b, int n) {
    for (int it = 0; it < n; ++it) {
        a = find_root(par, a, n);
        b = find_root(par, b, n);
        if (a == b) return;
        const int hi = max(a, b), lo = min(a, b);
        const int old = atomicCAS(par + 4 * hi, hi, lo);
        if (old == hi) return;
        a = old;
        b = lo;
    }
}

__global__ void __launch_bounds__(kCT) seed_bodies_kernel(const float* __restrict__ xyz, int S,
                                                          const int* __restrict__ seed_idx, int n, float link_cutoff,
                                                          int min_size, int max_bodies, int* __restrict__ label,
                                                          int* __restrict__ nbody, int* __restrict__ size,
                                                          double* __restrict__ centre) {
    extern __shared__ __attribute__((aligned(16))) float4 sd[];  // (n): x, y, z, the seed's word
    __shared__ int wsum[kCW];
    const int t = threadIdx.x, lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int s = blockIdx.x;
    int* par = reinterpret_cast<int*>(sd) + 3;  // the word of seed q: par[4 q]
    const float* crd = reinterpret_cast<const float*>(sd);
    const float thr = sq_bound(link_cutoff);

    for (int p = t; p < n; p += kCT) {
        const float* __restrict__ src = xyz + ((size_t)seed_idx[p] * S + s) * 3;
        sd[p] = make_float4(src[0], src[1], src[2], __int_as_float(p));
    }
    __syncthreads();

    // the pairs: row block b (kRows seeds p) against the chunks c of kQ seeds q below its end;
    // tile k = b (b + 1) kRows / kQ / 2 .. : with kRows = 2 kQ block b starts at tile b (b + 1)
    static_assert(kRows == 2 * kQ, "the tile numbering assumes two q chunks per row block");
    const int nrb = (n + kRows - 1) / kRows;
    const int ntile = nrb * (nrb + 1);
    int b = 0;
    for (int k = w; k < ntile; k += kCW) {
        while ((b + 1) * (b + 2) <= k) ++b;  // b < nrb
        const int p0 = b * kRows, q0 = (k - b * (b + 1)) * kQ;
        const int q1 = min(q0 + kQ, n);
        float xi[kRR][3];
        int pi[kRR];
#pragma unroll
        for (int r = 0; r < kRR; ++r) {
            const int p = p0 + 64 * r + lane;
            pi[r] = p < n ? p : -1;  // no q is below a seed past the end
            const int pc = min(p, n - 1);
#pragma unroll
            for (int c = 0; c < 3; ++c) xi[r][c] = crd[4 * pc + c];
        }
        for (int q = q0; q < q1; ++q) {
            const float xq = crd[4 * q], yq = crd[4 * q + 1], zq = crd[4 * q + 2];
#pragma unroll
            for (int r = 0; r < kRR; ++r) {
                const float dx = __fsub_rn(xi[r][0], xq), dy = __fsub_rn(xi[r][1], yq), dz = __fsub_rn(xi[r][2], zq);
                const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
                if (d2 <= thr && q < pi[r]) unite(par, pi[r], q, n);
            }
        }
    }
    __syncthreads();

    // flatten: the roots first (the forest is only read), then every seed's word = its label
    int root[kSPT];
#pragma unroll
    for (int i = 0; i < kSPT; ++i) {
        const int p = i * kCT + t;
        root[i] = p < n ? root_of(par, p, n) : -1;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kSPT; ++i) {
        const int p = i * kCT + t;
        if (p < n) {
            par[4 * p] = root[i];
            if (label) label[(size_t)s * n + p] = root[i];
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kSPT; ++i)
        if (i * kCT + t < n) atomicAdd(par + 4 * root[i], 0x10000);
    __syncthreads();

    // number the bodies in ascending label: ballot prefix inside a wave, the waves in order
    int body[kSPT];
    int running = 0;
#pragma unroll
    for (int i = 0; i < kSPT; ++i) {
        body[i] = -1;
        if (i * kCT < n) {  // the whole workgroup or nobody
            const int p = i * kCT + t;
            const bool isb = p < n && root[i] == p && (par[4 * p] >> 16) >= min_size;
            const unsigned long long m = __ballot(isb);
            if (lane == 0) wsum[w] = __popcll(m);
            __syncthreads();
            int before = running;
            for (int v = 0; v < kCW; ++v) {
                const int c = wsum[v];
                before += v < w ? c : 0;
                running += c;
            }
            if (isb) body[i] = before + __popcll(m & ((1ull << lane) - 1ull));
            __syncthreads();
        }
    }
    if (t == 0) nbody[s] = running;

    // centres: the thread of a body's root walks all labels in rank order
#pragma unroll
    for (int i = 0; i < kSPT; ++i) {
        const int p = i * kCT + t;
        const bool mine = body[i] >= 0 && body[i] < max_bodies;
        if (!__any(mine)) continue;
        if (!centre) {
            if (mine && size) size[(size_t)s * max_bodies + body[i]] = par[4 * p] >> 16;
            continue;
        }
        double sx = 0.0, sy = 0.0, sz = 0.0;
        for (int q = 0; q < n; ++q) {
            const float4 v = sd[q];
            if (mine && (__float_as_int(v.w) & kLabelMask) == p) {
                sx = __dadd_rn(sx, (double)v.x);
                sy = __dadd_rn(sy, (double)v.y);
                sz = __dadd_rn(sz, (double)v.z);
            }
        }
        if (mine) {
            const int cnt = par[4 * p] >> 16;
            const size_t o = (size_t)s * max_bodies + body[i];
            if (size) size[o] = cnt;
            centre[3 * o] = sx / (double)cnt;
            centre[3 * o + 1] = sy / (double)cnt;
            centre[3 * o + 2] = sz / (double)cnt;
        }
    }
    for (int k = min(running, max_bodies) + t; k < max_bodies; k += kCT) {
        const size_t o = (size_t)s * max_bodies + k;
        if (size) size[o] = 0;
        if (centre) centre[3 * o] = centre[3 * o + 1] = centre[3 * o + 2] = __longlong_as_double(0x7ff8000000000000LL);
    }
}

constexpr int kFT = 256;            // threads of the feature kernel: 4 waves on the same 64 structures
constexpr int kFW = kFT / 64;
constexpr int kFR = 8;              // beads per thread
constexpr int kFB = kFW * kFR;      // beads per workgroup
constexpr int kFS = 64;             // structures per chunk

// ct (kmax, S, 3): the centres, body-major; nb (S)
__global__ void __launch_bounds__(kFT) body_features_kernel(const float* __restrict__ xyz, int n, int S,
                                                            const int* __restrict__ nb, const double* __restrict__ ct,
                                                            double assoc_cutoff, double decay,
                                                            double* __restrict__ nearest, double* __restrict__ dist_sum,
                                                            double* __restrict__ dist_sqsum,
                                                            long long* __restrict__ assoc,
                                                            double* __restrict__ tsa_sum) {
    __shared__ double tn[kFB][kFS + 1], tt[kFB][kFS + 1];  // nearest and t(p, s) of a chunk
    __shared__ int nbl[kFS];
    const int t = threadIdx.x, lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int ib = blockIdx.x * kFB + w * kFR;
    const int rb = t & (kFB - 1), rq = t / kFB;  // the reduction: bead rb of the workgroup, sum rq < 4
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const double mdecay = -decay;  // exp(-(decay * d)): negating a factor negates the rounded product
    double acc = 0.0;
    long long hits = 0;

    for (int s0 = 0; s0 < S; s0 += kFS) {
        const int s = s0 + lane;
        const bool live = s < S;
        const int nbs = live ? nb[s] : 0;
        int kmax = nbs;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) kmax = max(kmax, __shfl_xor(kmax, off));
        kmax = __builtin_amdgcn_readfirstlane(kmax);
        __syncthreads();  // the tiles of the previous chunk have been read
        if (w == 0) nbl[lane] = nbs;

        double x[kFR][3], best[kFR], tv[kFR];
        bool fin[kFR];
#pragma unroll
        for (int a = 0; a < kFR; ++a) {
            const int i = min(ib + a, n - 1);  // a bead past the end repeats the last one and stores nothing
            float f[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                f[c] = live ? xyz[((size_t)i * S + s) * 3 + c] : 0.f;
                x[a][c] = (double)f[c];
            }
            fin[a] = isfinite(f[0]) && isfinite(f[1]) && isfinite(f[2]);
            best[a] = nan;
            tv[a] = 0.0;
        }
        for (int k = 0; k < kmax; ++k) {
            const bool on = k < nbs;
            const double* __restrict__ cp = ct + ((size_t)k * S + (on ? s : s0)) * 3;
            const double c0 = cp[0], c1 = cp[1], c2 = cp[2];
#pragma unroll
            for (int a = 0; a < kFR; ++a) {
                const double t0 = __dsub_rn(x[a][0], c0), t1 = __dsub_rn(x[a][1], c1), t2 = __dsub_rn(x[a][2], c2);
                double d = sqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(t0, t0), __dmul_rn(t1, t1)), __dmul_rn(t2, t2)));
                if (!fin[a]) d = nan;
                const double e = exp(__dmul_rn(mdecay, d));
                if (on) {
                    best[a] = (k == 0 || d < best[a]) ? d : best[a];
                    tv[a] = __dadd_rn(tv[a], e);
                }
            }
        }
#pragma unroll
        for (int a = 0; a < kFR; ++a) {
            tn[w * kFR + a][lane] = best[a];
            tt[w * kFR + a][lane] = tv[a];
            if (nearest && live && ib + a < n) nearest[(size_t)(ib + a) * S + s] = best[a];
        }
        __syncthreads();
        if (rq < 4) {  // structure order, one sum per thread
            const int ns = min(kFS, S - s0);
            for (int q = 0; q < ns; ++q) {
                const double d = tn[rb][q];
                const bool has = nbl[q] > 0;
                if (rq == 0) {
                    if (has) acc = __dadd_rn(acc, d);
                } else if (rq == 1) {
                    if (has) acc = __dadd_rn(acc, __dmul_rn(d, d));
                } else if (rq == 2) {
                    hits += d <= assoc_cutoff ? 1 : 0;
                } else {
                    acc = __dadd_rn(acc, tt[rb][q]);
                }
            }
        }
    }
    const int i = blockIdx.x * kFB + rb;
    if (i < n) {
        if (rq == 0 && dist_sum) dist_sum[i] = acc;
        if (rq == 1 && dist_sqsum) dist_sqsum[i] = acc;
        if (rq == 2 && assoc) assoc[i] = hits;
        if (rq == 3 && tsa_sum) tsa_sum[i] = acc;
    }
}

}  // namespace

extern "C" int igm_report_seed_bodies(igm_ctx* c, uint32_t flags, const float* xyz, int32_t nbead, int32_t nstruct,
                                      const int32_t* seed_idx, int32_t nseed, float link_cutoff, int32_t min_size,
                                      int32_t max_bodies, int32_t* label, int32_t* nbody, int32_t* size,
                                      double* centre) {
    static const char* fn = "igm_report_seed_bodies";
    if (!c) return IGM_E_INVALID;
    if (nbead <= 0 || nstruct <= 0 || nseed <= 0 || !xyz || !seed_idx || !nbody)
        return fail(c, IGM_E_INVALID, "%s: invalid arguments (nbead %d, nstruct %d, nseed %d)", fn, nbead, nstruct,
                    nseed);
    if (!(link_cutoff >= 0.0f) || !std::isfinite(link_cutoff))
        return fail(c, IGM_E_INVALID, "%s: link_cutoff %g is negative or not finite", fn, (double)link_cutoff);
    if (min_size < 1) return fail(c, IGM_E_INVALID, "%s: min_size %d < 1", fn, min_size);
    if (max_bodies < 0 || (max_bodies < 1 && (size || centre)))
        return fail(c, IGM_E_INVALID, "%s: max_bodies %d cannot hold the sizes or centres asked for", fn, max_bodies);
    if (nseed > kMaxSeeds) return fail(c, IGM_E_UNSUPPORTED, "%s: %d seeds exceed %d", fn, nseed, kMaxSeeds);
    for (int p = 0; p < nseed; ++p)
        if (seed_idx[p] < 0 || seed_idx[p] >= nbead || (p > 0 && seed_idx[p] <= seed_idx[p - 1]))
            return fail(c, IGM_E_INVALID, "%s: seed_idx[%d] = %d is out of range or not above its predecessor", fn, p,
                        seed_idx[p]);

    IGM_HIP_CHECK(c, hipSetDevice(c->device));
    const size_t nsl = (size_t)nstruct * max_bodies;
    const float* d_xyz;
    const int32_t* d_seed;
    void *p_label = nullptr, *p_nbody, *p_size = nullptr, *p_centre = nullptr;
    IGM_TRY(to_device(c, flags, "rb_xyz", xyz, (size_t)nbead * nstruct * 3, &d_xyz));
    IGM_TRY(to_device(c, 0u, "rb_seed", seed_idx, (size_t)nseed, &d_seed));
    if (label) IGM_TRY(workspace(c, "rb_label", sizeof(int32_t) * (size_t)nstruct * nseed, &p_label));
    IGM_TRY(workspace(c, "rb_nbody", sizeof(int32_t) * (size_t)nstruct, &p_nbody));
    if (size) IGM_TRY(workspace(c, "rb_size", sizeof(int32_t) * nsl, &p_size));
    if (centre) IGM_TRY(workspace(c, "rb_centre", sizeof(double) * 3 * nsl, &p_centre));
    const size_t lds = sizeof(float4) * (size_t)nseed;
    if (lds > 65536)
        IGM_HIP_CHECK(c, hipFuncSetAttribute((const void*)seed_bodies_kernel,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    {
        Timed tm(c, "report_seed_bodies");
        hipLaunchKernelGGL(seed_bodies_kernel, dim3((unsigned)nstruct), dim3(kCT), lds, c->stream, d_xyz,
                           (int)nstruct, d_seed, (int)nseed, link_cutoff, (int)min_size, (int)max_bodies,
                           (int*)p_label, (int*)p_nbody, (int*)p_size, (double*)p_centre);
        IGM_HIP_CHECK(c, hipGetLastError());
    }
    // the counts first: on overflow they are all the caller gets
    std::vector<int32_t> count(nstruct);
    IGM_TRY(to_host(c, 0u, count.data(), (const int32_t*)p_nbody, (size_t)nstruct));
    IGM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    IGM_HIP_CHECK(c, hipGetLastError());
    std::copy(count.begin(), count.end(), nbody);
    const int32_t most = *std::max_element(count.begin(), count.end());
    if (most > max_bodies)
        return fail(c, IGM_E_OVERFLOW, "%s: a structure has %d bodies, max_bodies is %d", fn, most, max_bodies);
    IGM_TRY(to_host(c, 0u, label, (const int32_t*)p_label, (size_t)nstruct * nseed));
    IGM_TRY(to_host(c, 0u, size, (const int32_t*)p_size, nsl));
    IGM_TRY(to_host(c, 0u, centre, (const double*)p_centre, 3 * nsl));
    IGM_HIP_CHECK(c, hipStreamSynchronize(c->stream));  // the outputs are host arrays
    return finish(c, flags);
}

extern "C" int igm_report_body_features(igm_ctx* c, uint32_t flags, const float* xyz, int32_t nbead, int32_t nstruct,
                                        const int32_t* nbody, const double* centre, int32_t max_bodies,
                                        double assoc_cutoff, double decay, double* nearest, double* dist_sum,
                                        double* dist_sqsum, int64_t* assoc, double* tsa_sum) {
    static const char* fn = "igm_report_body_features";
    if (!c) return IGM_E_INVALID;
    if (nbead <= 0 || nstruct <= 0 || max_bodies <= 0 || !xyz || !nbody || !centre)
        return fail(c, IGM_E_INVALID, "%s: invalid arguments (nbead %d, nstruct %d, max_bodies %d)", fn, nbead,
                    nstruct, max_bodies);
    if (!nearest && !dist_sum && !dist_sqsum && !assoc && !tsa_sum)
        return fail(c, IGM_E_INVALID, "%s: every output is NULL", fn);
    if (!(assoc_cutoff >= 0.0) || !std::isfinite(assoc_cutoff))
        return fail(c, IGM_E_INVALID, "%s: assoc_cutoff %g is negative or not finite", fn, assoc_cutoff);
    if (!(decay >= 0.0) || !std::isfinite(decay))
        return fail(c, IGM_E_INVALID, "%s: decay %g is negative or not finite", fn, decay);
    int kmax = 0;
    for (int s = 0; s < nstruct; ++s) {
        if (nbody[s] < 0 || nbody[s] > max_bodies)
            return fail(c, IGM_E_INVALID, "%s: nbody[%d] = %d outside [0, %d]", fn, s, nbody[s], max_bodies);
        kmax = std::max(kmax, nbody[s]);
    }
    // the centres body-major: the lanes of a wave (structures) then read neighbouring addresses
    std::vector<double> ct((size_t)std::max(kmax, 1) * nstruct * 3, 0.0);
    for (int s = 0; s < nstruct; ++s)
        for (int k = 0; k < nbody[s]; ++k)
            for (int a = 0; a < 3; ++a) {
                const double v = centre[((size_t)s * max_bodies + k) * 3 + a];
                if (!std::isfinite(v))
                    return fail(c, IGM_E_INVALID, "%s: centre %d of structure %d is not finite", fn, k, s);
                ct[((size_t)k * nstruct + s) * 3 + a] = v;
            }

    IGM_HIP_CHECK(c, hipSetDevice(c->device));
    const size_t nps = (size_t)nbead * nstruct;
    const float* d_xyz;
    const int32_t* d_nb;
    const double* d_ct;
    double* d_near = nearest;
    void *p_near, *p_ds, *p_dq, *p_as, *p_ts;
    IGM_TRY(to_device(c, flags, "rb_xyz", xyz, nps * 3, &d_xyz));
    IGM_TRY(to_device(c, 0u, "rb_nbody", nbody, (size_t)nstruct, &d_nb));
    IGM_TRY(to_device(c, 0u, "rb_ct", ct.data(), ct.size(), &d_ct));
    if (nearest && !(flags & IGM_DEVICE_PTRS)) {
        IGM_TRY(workspace(c, "rb_nearest", sizeof(double) * nps, &p_near));
        d_near = (double*)p_near;
    }
    IGM_TRY(workspace(c, "rb_dsum", sizeof(double) * (size_t)nbead, &p_ds));
    IGM_TRY(workspace(c, "rb_dsq", sizeof(double) * (size_t)nbead, &p_dq));
    IGM_TRY(workspace(c, "rb_assoc", sizeof(int64_t) * (size_t)nbead, &p_as));
    IGM_TRY(workspace(c, "rb_tsa", sizeof(double) * (size_t)nbead, &p_ts));
    {
        Timed tm(c, "report_body_features");
        hipLaunchKernelGGL(body_features_kernel, dim3((unsigned)ceil_div(nbead, kFB)), dim3(kFT), 0, c->stream, d_xyz,
                           (int)nbead, (int)nstruct, d_nb, d_ct, assoc_cutoff, decay, d_near, (double*)p_ds,
                           (double*)p_dq, (long long*)p_as, (double*)p_ts);
        IGM_HIP_CHECK(c, hipGetLastError());
    }
    if (nearest) IGM_TRY(to_host(c, flags, nearest, (const double*)d_near, nps));
    IGM_TRY(to_host(c, 0u, dist_sum, (const double*)p_ds, (size_t)nbead));
    IGM_TRY(to_host(c, 0u, dist_sqsum, (const double*)p_dq, (size_t)nbead));
    IGM_TRY(to_host(c, 0u, assoc, (const int64_t*)p_as, (size_t)nbead));
    IGM_TRY(to_host(c, 0u, tsa_sum, (const double*)p_ts, (size_t)nbead));
    // the staged plane is a local and the per-bead outputs are host arrays: wait before returning
    IGM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return finish(c, flags);
}
