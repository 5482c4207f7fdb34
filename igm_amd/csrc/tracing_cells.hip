// Chromatin tracing A-step on imaged cells for libigmhip (gfx950): the traces of one cell share
// the cell's frame, so a cell is placed on a structure under ONE proper rigid motion and one
// homologue labelling (every trace a copy of its chromosome, no copy twice).
//
//   sums     per (trace t, copy k, structure s) the 13 fp64 sums of the superposition, from the
//            f32 coordinates: sx = sum x_i, sxx = sum |x_i|^2, m[a][b] = sum q_a x_b, with q_i the
//            spot centred on its CELL and x_i the bead minus the structure's reference bead o_s
//            (the bead of the cell's first spot under copy 0).  The sums are additive over the
//            traces of a cell: the joint superposition of any labelling is a sum of records and
//            one 4x4 eigen-solve.  Stored (trace, copy, 13, S): a wave reads contiguous doubles.
//   search   one thread per (cell, structure).  Start: per chromosome the injective labelling
//            of least total independent cost e(t, k) (the trace's own centred Kabsch, from the
//            same record).  Round: the joint (cost, R, tau) of the labelling, then per
//            chromosome the labelling of least total residual r(t, k) under (R, tau), taken only
//            if strictly below the current one's.  Labellings are walked in lexicographic order
//            and the first minimum wins.  Stops when no chromosome moves or after kCellRounds
//            rounds; neither step can raise the total residual, so the end is a local optimum.
//   select   the keep_best cheapest structures per cell (tracing_select.h) and the labels there.
//
// No atomics anywhere: the result is deterministic, and independent of the batching of the cells
// (a thread only ever reads the records of its own cell and structure).
#include <hip/hip_runtime.h>

#include "tracing_common.h"
#include "tracing_select.h"

namespace {
using namespace igm;

constexpr int kRec = 13;              // doubles of a record: sx[3], sxx, m[3][3]
constexpr int kCellRounds = 16;       // re-labelling rounds at most
constexpr int kMaxCellTraces = 128;   // traces of a cell: 2 bits each in four 64-bit registers
constexpr int kMaxCopies = 4;         // copies of a chromosome: up to 24 labellings
constexpr int64_t kScratchDefault = 1ll << 30;

struct SumsArgs : SpotArgs {
    int t0;                  // first trace of the batch
    const int* ref;          // (T) the reference bead of the trace's cell
    double* rec;             // (traces of the batch, Cmax, kRec, S)
};

// One thread per (trace t, copy k, structure s), one block per (t, k, kBT structures): the sums of
// spot_sums (tracing_common.h) on the positions centred on the cell, stored, not solved.
__global__ void __launch_bounds__(kBT) tracing_cell_sums_kernel(SumsArgs A) {
    const int sblk = blockIdx.x % A.nsb;
    const int tk = blockIdx.x / A.nsb;
    const int k = tk % A.Cmax, tl = tk / A.Cmax, t = A.t0 + tl;
    const int s = sblk * kBT + threadIdx.x;
    const bool live = s < A.S;
    if (k >= A.ncopy[t]) return;  // (the whole block: the search never reads this record)
    double x0[3] = {0.0, 0.0, 0.0};
    if (live) {
        const float* q = A.xyz + ((size_t)A.ref[t] * A.S + s) * 3;
        x0[0] = q[0];
        x0[1] = q[1];
        x0[2] = q[2];
    }
    double sx[3], sxx, m[3][3];
    spot_sums(A, t, k, s, live, x0, sx, sxx, m);  // (block-collective: no thread has left)
    if (!live) return;
    const size_t S = (size_t)A.S;
    double* out = A.rec + ((size_t)tl * A.Cmax + k) * kRec * S + s;
    out[0] = sx[0];
    out[S] = sx[1];
    out[2 * S] = sx[2];
    out[3 * S] = sxx;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) out[(4 + 3 * a + b) * S] = m[a][b];
}

struct SearchArgs {
    int S, Cmax, nsb;
    int c0, t0;                  // first cell and first trace of the batch
    int max_rounds;              // kCellRounds (fewer: measurements only)
    const long long* cell_ptr;   // (ncell + 1) traces of cell c
    const int* gptr;             // (ncell + 1) chromosomes of cell c
    const int2* grp;             // chromosome: x = C | m << 8 (copies, traces of it in the cell),
                                 //             y = the m traces, index in the cell, one per byte
    const double* tstat;         // (T, 5) sq[3], sqq, n_t
    const double* cstat;         // (ncell, 2) Ga, n
    const double* rec;           // the batch's records
    float* cost;                 // (ncell, S)
    unsigned char* label;        // (T, S)
    unsigned char* rounds;       // (ncell, S)
};

__device__ __forceinline__ int get_label(const unsigned long long (&w)[4], int t) {
    const unsigned long long v = t < 64 ? (t < 32 ? w[0] : w[1]) : (t < 96 ? w[2] : w[3]);
    return (int)(v >> ((t & 31) * 2)) & 3;
}

__device__ __forceinline__ void set_label(unsigned long long (&w)[4], int t, int k) {
    const int sh = (t & 31) * 2, word = t >> 5;
    const unsigned long long clear = ~(3ull << sh), bits = (unsigned long long)k << sh;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (word == j) w[j] = (w[j] & clear) | bits;
}

__device__ __forceinline__ double pick4(const double (&v)[4], int k) {
    return k == 0 ? v[0] : k == 1 ? v[1] : k == 2 ? v[2] : v[3];
}

// The injective labelling of the m traces of a chromosome on its C copies with the least
// sum_i tab[i][k_i], the labellings in lexicographic order of (k_0, k_1, ...), the first minimum
// kept; returned 2 bits per trace.  The sum of a labelling is ((tab0 + tab1) + tab2) + tab3.
__device__ __forceinline__ unsigned best_labelling(const double (&tab)[4][4], int m, int C, double* least) {
    double best = INFINITY;
    unsigned lab = 0;
#pragma unroll
    for (int k0 = 0; k0 < kMaxCopies; ++k0) {
        if (k0 >= C) continue;
        const double s0 = tab[0][k0];
        if (m == 1) {
            if (s0 < best) best = s0, lab = k0;
            continue;
        }
#pragma unroll
        for (int k1 = 0; k1 < kMaxCopies; ++k1) {
            if (k1 >= C || k1 == k0) continue;
            const double s1 = s0 + tab[1][k1];
            if (m == 2) {
                if (s1 < best) best = s1, lab = k0 | k1 << 2;
                continue;
            }
#pragma unroll
            for (int k2 = 0; k2 < kMaxCopies; ++k2) {
                if (k2 >= C || k2 == k0 || k2 == k1) continue;
                const double s2 = s1 + tab[2][k2];
                if (m == 3) {
                    if (s2 < best) best = s2, lab = k0 | k1 << 2 | k2 << 4;
                    continue;
                }
                const int k3 = 6 - k0 - k1 - k2;  // (m = 4 = C: the copy that is left)
                const double s3 = s2 + pick4(tab[3], k3);
                if (s3 < best) best = s3, lab = k0 | k1 << 2 | k2 << 4 | k3 << 6;
            }
        }
    }
    *least = best;
    return lab;
}

// One thread per (cell, structure), one block per (cell, kBT structures): the chromosome table
// of the cell is uniform over the block, the labelling and the number of rounds are the thread's.
__global__ void __launch_bounds__(kBT) tracing_cell_search_kernel(SearchArgs A) {
    const int sblk = blockIdx.x % A.nsb, c = A.c0 + blockIdx.x / A.nsb;
    const int s = sblk * kBT + threadIdx.x;
    if (s >= A.S) return;
    const size_t S = (size_t)A.S;
    const int ta = (int)A.cell_ptr[c], nt = (int)A.cell_ptr[c + 1] - ta;
    const int g0 = A.gptr[c], g1 = A.gptr[c + 1];
    const double Ga = A.cstat[2 * c], n = A.cstat[2 * c + 1];
    const double* rec = A.rec + (size_t)(ta - A.t0) * A.Cmax * kRec * S + s;  // record (tl, k): + (tl * Cmax + k) * kRec * S
    const double* tstat = A.tstat + (size_t)ta * 5;
    unsigned long long lab[4] = {0ull, 0ull, 0ull, 0ull};
    double tab[4][4], unused[4];

    // start: every chromosome by the independent costs of its traces
    for (int g = g0; g < g1; ++g) {
        const int2 G = A.grp[g];
        const int C = G.x & 0xff, m = G.x >> 8;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int tl = (G.y >> (8 * i)) & 0xff;
            const double* ts = tstat + 5 * tl;
#pragma unroll
            for (int k = 0; k < kMaxCopies; ++k) {
                tab[i][k] = 0.0;
                if (i >= m || k >= C) continue;
                const double* p = rec + ((size_t)tl * A.Cmax + k) * kRec * S;
                const double nt_ = ts[4], sx0 = p[0], sx1 = p[S], sx2 = p[2 * S];
                const double ga = ts[3] - (ts[0] * ts[0] + ts[1] * ts[1] + ts[2] * ts[2]) / nt_;
                const double gb = p[3 * S] - (sx0 * sx0 + sx1 * sx1 + sx2 * sx2) / nt_;
                const double sxn[3] = {sx0 / nt_, sx1 / nt_, sx2 / nt_};
                double mt[3][3];
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int b = 0; b < 3; ++b) mt[a][b] = p[(4 + 3 * a + b) * S] - ts[a] * sxn[b];
                tab[i][k] = fmax(0.0, ga + gb - 2.0 * horn<false>(mt, unused));
            }
        }
        double least;
        const unsigned L = best_labelling(tab, m, C, &least);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < m) set_label(lab, (G.y >> (8 * i)) & 0xff, (L >> (2 * i)) & 3);
    }

    int round = 0;
    double cost2;
    for (;;) {
        // the joint superposition of the labelling
        double SX[3] = {0.0, 0.0, 0.0}, SXX = 0.0;
        double M[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
        for (int tl = 0; tl < nt; ++tl) {
            const double* p = rec + ((size_t)tl * A.Cmax + get_label(lab, tl)) * kRec * S;
            SX[0] += p[0];
            SX[1] += p[S];
            SX[2] += p[2 * S];
            SXX += p[3 * S];
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) M[a][b] += p[(4 + 3 * a + b) * S];
        }
        const double Gb = fmax(0.0, SXX - (SX[0] * SX[0] + SX[1] * SX[1] + SX[2] * SX[2]) / n);
        double q[4];
        const double lam = horn<true>(M, q);
        cost2 = fmax(0.0, (Ga + Gb - 2.0 * lam) / n);
        if (round == A.max_rounds) break;
        ++round;
        const double tau[3] = {SX[0] / n, SX[1] / n, SX[2] / n};
        const double tt = tau[0] * tau[0] + tau[1] * tau[1] + tau[2] * tau[2];
        double R[3][3];
        R[0][0] = q[0] * q[0] + q[1] * q[1] - q[2] * q[2] - q[3] * q[3];
        R[1][1] = q[0] * q[0] - q[1] * q[1] + q[2] * q[2] - q[3] * q[3];
        R[2][2] = q[0] * q[0] - q[1] * q[1] - q[2] * q[2] + q[3] * q[3];
        R[0][1] = 2.0 * (q[1] * q[2] - q[0] * q[3]);
        R[1][0] = 2.0 * (q[1] * q[2] + q[0] * q[3]);
        R[0][2] = 2.0 * (q[1] * q[3] + q[0] * q[2]);
        R[2][0] = 2.0 * (q[1] * q[3] - q[0] * q[2]);
        R[1][2] = 2.0 * (q[2] * q[3] - q[0] * q[1]);
        R[2][1] = 2.0 * (q[2] * q[3] + q[0] * q[1]);
        double Rt[3];  // tau R: tau . (R sq) = (tau R) . sq
#pragma unroll
        for (int a = 0; a < 3; ++a) Rt[a] = tau[0] * R[0][a] + tau[1] * R[1][a] + tau[2] * R[2][a];

        // every chromosome to its labelling of least residual under (R, tau)
        bool moved = false;
        for (int g = g0; g < g1; ++g) {
            const int2 G = A.grp[g];
            const int C = G.x & 0xff, m = G.x >> 8;
            if (C == 1) continue;  // (one labelling)
            double cur = 0.0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int tl = (G.y >> (8 * i)) & 0xff;
                const double* ts = tstat + 5 * tl;
#pragma unroll
                for (int k = 0; k < kMaxCopies; ++k) {
                    tab[i][k] = 0.0;
                    if (i >= m || k >= C) continue;
                    const double* p = rec + ((size_t)tl * A.Cmax + k) * kRec * S;
                    double rm = 0.0;
#pragma unroll
                    for (int a = 0; a < 3; ++a)
#pragma unroll
                        for (int b = 0; b < 3; ++b) rm += R[b][a] * p[(4 + 3 * a + b) * S];
                    tab[i][k] = ts[3] + p[3 * S] + ts[4] * tt + 2.0 * (Rt[0] * ts[0] + Rt[1] * ts[1] + Rt[2] * ts[2]) -
                                2.0 * (tau[0] * p[0] + tau[1] * p[S] + tau[2] * p[2 * S]) - 2.0 * rm;
                }
                if (i < m) {
                    const double r = pick4(tab[i], get_label(lab, tl));
                    cur = i == 0 ? r : cur + r;
                }
            }
            double least;
            const unsigned L = best_labelling(tab, m, C, &least);
            if (least < cur) {
                moved = true;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < m) set_label(lab, (G.y >> (8 * i)) & 0xff, (L >> (2 * i)) & 3);
            }
        }
        if (!moved) break;
    }
    A.cost[(size_t)c * S + s] = (float)sqrt(cost2);
    A.rounds[(size_t)c * S + s] = (unsigned char)round;
    for (int tl = 0; tl < nt; ++tl) A.label[(size_t)(ta + tl) * S + s] = (unsigned char)get_label(lab, tl);
}

// best_label[t, j] = label[t, best_struct[cell of t, j]]
__global__ void __launch_bounds__(kBT) tracing_cell_labels_kernel(const unsigned char* __restrict__ label,
                                                                  const int* __restrict__ tcell,
                                                                  const int* __restrict__ best_struct, int T, int S,
                                                                  int kb, unsigned char* __restrict__ best_label) {
    const long long i = (long long)blockIdx.x * kBT + threadIdx.x;
    if (i >= (long long)T * kb) return;
    const int t = (int)(i / kb), j = (int)(i % kb);
    best_label[i] = label[(size_t)t * S + best_struct[(size_t)tcell[t] * kb + j]];
}

}  // namespace

#define CELLS "igm_tracing_assign_cells: "

extern "C" int igm_tracing_assign_cells(igm_ctx* c, uint32_t flags, const float* xyz, int32_t nbead, int32_t nstruct,
                                        const int32_t* copy_ptr, const int32_t* copy_idx, int32_t nhap, int32_t ntrace,
                                        const int64_t* trace_ptr, const int32_t* locus, const float* position,
                                        const int32_t* trace_chrom, int32_t ncell, const int64_t* cell_ptr,
                                        int32_t keep_best, int64_t scratch_bytes, float* cost_out, uint8_t* label_out,
                                        uint8_t* rounds_out, int32_t* best_struct, float* best_cost,
                                        uint8_t* best_label) {
    if (!c) return IGM_E_INVALID;
    if (nbead <= 0 || nstruct <= 0 || nhap <= 0 || ntrace < 0 || ncell < 0 || !xyz || !copy_ptr || !copy_idx ||
        !trace_ptr || !cell_ptr || !best_struct || !best_cost || !best_label || scratch_bytes < 0)
        return fail(c, IGM_E_INVALID, CELLS "invalid arguments");
    if (keep_best < 1 || keep_best > nstruct)
        return fail(c, IGM_E_INVALID, CELLS "keep_best %d must be in [1, %d structures]", keep_best, nstruct);
    if (flags & IGM_DEVICE_PTRS)
        return fail(c, IGM_E_UNSUPPORTED, CELLS "host arrays expected (validated on the host)");
    IGM_HIP_CHECK(c, hipSetDevice(c->device));
    // host validation: the kernels trust the tables built here
    if (cell_ptr[0] != 0) return fail(c, IGM_E_INVALID, CELLS "cell_ptr[0] = %lld, not 0", (long long)cell_ptr[0]);
    for (int q = 0; q < ncell; ++q)
        if (cell_ptr[q + 1] <= cell_ptr[q])
            return fail(c, IGM_E_INVALID, CELLS "cell %d has no trace (cell_ptr must increase)", q);
    if (cell_ptr[ncell] != ntrace)
        return fail(c, IGM_E_INVALID, CELLS "cell_ptr ends at %lld, there are %d traces", (long long)cell_ptr[ncell],
                    ntrace);
    if (ntrace == 0) return IGM_OK;
    std::vector<int> ncopy, bead;
    IGM_TRY(check_traces(c, "igm_tracing_assign_cells", nbead, copy_ptr, copy_idx, nhap, ntrace, trace_ptr, locus,
                         position, locus && position && trace_chrom ? nullptr : "locus, position or trace_chrom",
                         &ncopy));
    const int64_t nspot = trace_ptr[ntrace];
    int Cmax = 1;
    // the chromosomes of every cell, in order of first appearance, each with its traces in order
    std::vector<int> gptr(ncell + 1, 0), gchrom, gcopies, gtraces;
    std::vector<int2> grp;
    for (int q = 0; q < ncell; ++q) {
        const int ta = (int)cell_ptr[q], nt = (int)(cell_ptr[q + 1] - cell_ptr[q]);
        const size_t g0 = grp.size();
        for (int tl = 0; tl < nt; ++tl) {
            const int t = ta + tl;
            size_t g = g0;
            while (g < grp.size() && gchrom[g] != trace_chrom[t]) ++g;
            if (g == grp.size()) {
                grp.push_back(make_int2(0, 0));
                gchrom.push_back(trace_chrom[t]);
                gcopies.push_back(ncopy[t]);
                gtraces.push_back(0);
            }
            if (gcopies[g] != ncopy[t])
                return fail(c, IGM_E_INVALID, CELLS "cell %d: chromosome %d has traces of %d and of %d copies", q,
                            trace_chrom[t], gcopies[g], ncopy[t]);
            if (gtraces[g] >= gcopies[g])
                return fail(c, IGM_E_INVALID, CELLS "cell %d has more than %d traces of chromosome %d", q, gcopies[g],
                            trace_chrom[t]);
            if (tl < kMaxCellTraces && gcopies[g] <= kMaxCopies) grp[g].y |= tl << (8 * gtraces[g]);  // (else refused below)
            grp[g].x = gcopies[g] | ++gtraces[g] << 8;
        }
        gptr[q + 1] = (int)grp.size();
    }
    for (int q = 0; q < ncell; ++q) {
        if (cell_ptr[q + 1] - cell_ptr[q] > kMaxCellTraces)
            return fail(c, IGM_E_UNSUPPORTED, CELLS "cell %d has %lld traces, more than %d", q,
                        (long long)(cell_ptr[q + 1] - cell_ptr[q]), kMaxCellTraces);
        for (int64_t t = cell_ptr[q]; t < cell_ptr[q + 1]; ++t)
            if (ncopy[t] > kMaxCopies)
                return fail(c, IGM_E_UNSUPPORTED, CELLS "cell %d: trace %lld is of a chromosome with %d copies, more "
                            "than %d", q, (long long)t, ncopy[t], kMaxCopies);
        Cmax = std::max(Cmax, *std::max_element(ncopy.begin() + cell_ptr[q], ncopy.begin() + cell_ptr[q + 1]));
    }
    // batches of whole cells whose records fit the scratch
    const int64_t scratch = scratch_bytes ? scratch_bytes : kScratchDefault;
    const int64_t per_trace = (int64_t)Cmax * kRec * nstruct * (int64_t)sizeof(double);
    const int nsb = (int)ceil_div(nstruct, kBT);
    std::vector<int> batch{0};  // first cell of every batch, then ncell
    int64_t most = 0;           // traces of the largest batch
    for (int q = 0, b0 = 0; q < ncell; ++q) {
        const int64_t nt = cell_ptr[q + 1] - cell_ptr[q];
        if (nt * per_trace > scratch)
            return fail(c, IGM_E_UNSUPPORTED, CELLS "cell %d needs %lld bytes of scratch, %lld are allowed", q,
                        (long long)(nt * per_trace), (long long)scratch);
        if ((cell_ptr[q + 1] - cell_ptr[b0]) * per_trace > scratch) {
            batch.push_back(q);
            b0 = q;
        }
        most = std::max(most, cell_ptr[q + 1] - cell_ptr[b0]);
    }
    batch.push_back(ncell);
    if (most * Cmax * nsb > 0x7fffffff || (int64_t)ncell * nsb > 0x7fffffff ||
        (int64_t)ntrace * keep_best > 0x7fffffffll * kBT)
        return fail(c, IGM_E_UNSUPPORTED, CELLS "grid too large");
    // the host tables: positions centred on their cell, the per-trace and per-cell sums, the beads
    std::vector<double> pos((size_t)nspot * 3), tstat((size_t)ntrace * 5), cstat((size_t)ncell * 2);
    std::vector<int> ref(ntrace), tcell(ntrace);
    const int chunk = bead_table(copy_ptr, copy_idx, ntrace, trace_ptr, locus, ncopy, Cmax, &bead);
    for (int q = 0; q < ncell; ++q) {
        const int64_t ta = cell_ptr[q], tb = cell_ptr[q + 1];
        const int64_t p0 = trace_ptr[ta], p1 = trace_ptr[tb];
        double mean[3] = {0.0, 0.0, 0.0};
        for (int64_t i = p0; i < p1; ++i)
            for (int d = 0; d < 3; ++d) mean[d] += (double)position[i * 3 + d];
        const double n = (double)(p1 - p0);
        double Ga = 0.0;
        for (int64_t t = ta; t < tb; ++t) {
            double* ts = tstat.data() + (size_t)t * 5;
            for (int64_t i = trace_ptr[t]; i < trace_ptr[t + 1]; ++i)
                for (int d = 0; d < 3; ++d) {
                    const double v = (double)position[i * 3 + d] - mean[d] / n;
                    pos[(size_t)i * 3 + d] = v;
                    ts[d] += v;
                    ts[3] += v * v;
                }
            ts[4] = (double)(trace_ptr[t + 1] - trace_ptr[t]);
            Ga += ts[3];
            ref[t] = copy_idx[copy_ptr[locus[p0]]];
            tcell[t] = q;
        }
        cstat[(size_t)q * 2] = Ga;
        cstat[(size_t)q * 2 + 1] = n;
    }
    int max_rounds = kCellRounds;
    // (scripts/tracing_cells_timing.py: the start alone, one round, two, ... to split the search's time)
    if (const char* e = getenv("IGM_TRACING_CELL_ROUNDS")) max_rounds = std::min(kCellRounds, std::max(0, atoi(e)));

    const float* d_xyz;
    const int64_t *d_ptr, *d_cptr;
    const int *d_nc, *d_ref, *d_bead, *d_gptr, *d_tcell;
    const int2* d_grp;
    const double *d_pos, *d_tstat, *d_cstat;
    IGM_TRY(to_device(c, flags, "tr_xyz", xyz, (size_t)nbead * nstruct * 3, &d_xyz));
    IGM_TRY(to_device(c, flags, "tr_ptr", trace_ptr, (size_t)ntrace + 1, &d_ptr));
    IGM_TRY(to_device(c, flags, "trc_cptr", cell_ptr, (size_t)ncell + 1, &d_cptr));
    IGM_TRY(to_device(c, flags, "tr_nc", (const int*)ncopy.data(), ncopy.size(), &d_nc));
    IGM_TRY(to_device(c, flags, "trc_ref", (const int*)ref.data(), ref.size(), &d_ref));
    IGM_TRY(to_device(c, flags, "tr_bead", (const int*)bead.data(), bead.size(), &d_bead));
    IGM_TRY(to_device(c, flags, "trc_gptr", (const int*)gptr.data(), gptr.size(), &d_gptr));
    IGM_TRY(to_device(c, flags, "trc_tcell", (const int*)tcell.data(), tcell.size(), &d_tcell));
    IGM_TRY(to_device(c, flags, "trc_grp", (const int2*)grp.data(), grp.size(), &d_grp));
    IGM_TRY(to_device(c, flags, "tr_pos", (const double*)pos.data(), pos.size(), &d_pos));
    IGM_TRY(to_device(c, flags, "trc_tstat", (const double*)tstat.data(), tstat.size(), &d_tstat));
    IGM_TRY(to_device(c, flags, "trc_cstat", (const double*)cstat.data(), cstat.size(), &d_cstat));
    void *p_rec, *p_cost, *p_label, *p_rounds, *p_bs, *p_bv, *p_bl;
    const size_t nb = (size_t)ncell * keep_best, nl = (size_t)ntrace * keep_best;
    IGM_TRY(workspace(c, "trc_rec", (size_t)(most * per_trace), &p_rec));
    IGM_TRY(workspace(c, "trc_cost", (size_t)ncell * nstruct * sizeof(float), &p_cost));
    IGM_TRY(workspace(c, "trc_label", (size_t)ntrace * nstruct, &p_label));
    IGM_TRY(workspace(c, "trc_rounds", (size_t)ncell * nstruct, &p_rounds));
    IGM_TRY(workspace(c, "trc_bs", nb * sizeof(int32_t), &p_bs));
    IGM_TRY(workspace(c, "trc_bv", nb * sizeof(float), &p_bv));
    IGM_TRY(workspace(c, "trc_bl", nl, &p_bl));

    SumsArgs A;
    A.xyz = d_xyz;
    A.S = nstruct;
    A.Cmax = Cmax;
    A.nsb = nsb;
    A.chunk = chunk;
    A.ptr = reinterpret_cast<const long long*>(d_ptr);
    A.ncopy = d_nc;
    A.ref = d_ref;
    A.pos = d_pos;
    A.bead = d_bead;
    A.rec = (double*)p_rec;
    SearchArgs B;
    B.S = nstruct;
    B.Cmax = Cmax;
    B.nsb = nsb;
    B.max_rounds = max_rounds;
    B.cell_ptr = reinterpret_cast<const long long*>(d_cptr);
    B.gptr = d_gptr;
    B.grp = d_grp;
    B.tstat = d_tstat;
    B.cstat = d_cstat;
    B.rec = (const double*)p_rec;
    B.cost = (float*)p_cost;
    B.label = (unsigned char*)p_label;
    B.rounds = (unsigned char*)p_rounds;
    // the sums and the search run once per batch: their event times are added up (kms)
    for (const char* name : {"tracing_cells", "tracing_cell_sums", "tracing_cell_search", "tracing_cell_select"})
        c->kms.erase(name);
    double ms_sums = 0.0, ms_search = 0.0;
    for (size_t b = 0; b + 1 < batch.size(); ++b) {
        const int q0 = batch[b], q1 = batch[b + 1];
        const int t0 = (int)cell_ptr[q0], nt = (int)(cell_ptr[q1] - cell_ptr[q0]);
        A.t0 = B.t0 = t0;
        B.c0 = q0;
        {
            Timed tm(c, "tracing_cell_sums");
            hipLaunchKernelGGL(tracing_cell_sums_kernel, dim3((unsigned)((int64_t)nt * Cmax * nsb)), dim3(kBT),
                               (size_t)chunk * (3 * sizeof(double) + sizeof(int)), c->stream, A);
            IGM_HIP_CHECK(c, hipGetLastError());
        }
        {
            Timed tm(c, "tracing_cell_search");
            hipLaunchKernelGGL(tracing_cell_search_kernel, dim3((unsigned)((int64_t)(q1 - q0) * nsb)), dim3(kBT), 0,
                               c->stream, B);
            IGM_HIP_CHECK(c, hipGetLastError());
        }
        ms_sums += igm_last_kernel_ms(c, "tracing_cell_sums");  // (waits for the batch: the next one reuses the scratch)
        ms_search += igm_last_kernel_ms(c, "tracing_cell_search");
    }
    {
        Timed tm(c, "tracing_cell_select");
        IGM_TRY(tracing_select(c, (const float*)p_cost, ncell, nstruct, keep_best, (int*)p_bs, (float*)p_bv));
        hipLaunchKernelGGL(tracing_cell_labels_kernel, dim3((unsigned)ceil_div((int64_t)nl, kBT)), dim3(kBT), 0,
                           c->stream, (const unsigned char*)p_label, d_tcell, (const int*)p_bs, (int)ntrace,
                           (int)nstruct, (int)keep_best, (unsigned char*)p_bl);
        IGM_HIP_CHECK(c, hipGetLastError());
    }
    IGM_TRY(to_host(c, flags, cost_out, (const float*)p_cost, (size_t)ncell * nstruct));
    IGM_TRY(to_host(c, flags, label_out, (const uint8_t*)p_label, (size_t)ntrace * nstruct));
    IGM_TRY(to_host(c, flags, rounds_out, (const uint8_t*)p_rounds, (size_t)ncell * nstruct));
    IGM_TRY(to_host(c, flags, best_struct, (const int32_t*)p_bs, nb));
    IGM_TRY(to_host(c, flags, best_cost, (const float*)p_bv, nb));
    IGM_TRY(to_host(c, flags, best_label, (const uint8_t*)p_bl, nl));
    IGM_TRY(finish(c, flags));  // (synchronises: the host tables above outlive their copies)
    const double ms_select = igm_last_kernel_ms(c, "tracing_cell_select");
    c->kms["tracing_cell_sums"] = ms_sums;
    c->kms["tracing_cell_search"] = ms_search;
    c->kms["tracing_cells"] = ms_sums + ms_search + ms_select;
    return IGM_OK;
}
