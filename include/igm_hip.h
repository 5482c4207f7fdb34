/*
 * igm_hip.h -- C ABI of libigmhip.so, the MI355X (gfx950) engine that replaces
 * the two hot paths of IGM (bonimba87/igm):
 *
 *   A-step  ActivationDistanceStep.get_actdist  (igm/steps/ActivationDistanceStep.py:336-485)
 *           applied to every kept haploid pair   (ActivationDistanceStep.py:196-230)
 *   M-step  serial-LAMMPS anneal + CG per structure, i.e. lammps.optimize
 *           (igm/model/kernel/lammps.py:361-492) driven by ModelingStep.task
 *           (igm/steps/ModelingStep.py:164-573), batched over the population.
 *
 * Plain C types only (no torch types).  Every entry point returns IGM_OK (0) or
 * a negative IGM_E_* code; igm_last_error() then holds a message.  The Python
 * shim maps a nonzero code to RuntimeError(message), which is the reference's
 * behaviour on a failed LAMMPS run (lammps.py:453-457).
 *
 * Ownership: the caller owns every buffer.  With IGM_DEVICE_PTRS set in `flags`
 * all array arguments are device pointers on the context's device (e.g. torch
 * tensors' data_ptr()); otherwise they are host pointers and the library stages
 * them.  Calls are stream-ordered on the context stream and return after the
 * work has completed unless IGM_ASYNC is set (device-pointer mode only).
 * Threading: one igm_ctx per (host thread, GPU); a context is not thread safe.
 */
#ifndef IGM_HIP_H
#define IGM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IGM_OK 0
#define IGM_E_INVALID (-1)     /* bad argument                              */
#define IGM_E_HIP (-2)         /* HIP runtime error                         */
#define IGM_E_NOMEM (-3)       /* device allocation failed                  */
#define IGM_E_OVERFLOW (-4)    /* neighbour list / row capacity exceeded    */
#define IGM_E_UNSUPPORTED (-5) /* size outside the implemented envelope      */

#define IGM_DEVICE_PTRS 0x1u /* array arguments are device pointers        */
#define IGM_ASYNC 0x2u       /* do not synchronise before returning        */
#define IGM_F32_PATH 0x4u    /* igm_mstep_forces: use the f32 MD force path */

typedef struct igm_ctx igm_ctx;

/* ---- context ------------------------------------------------------------- */
int igm_ctx_create(int device, igm_ctx** out);
void igm_ctx_destroy(igm_ctx* ctx);
const char* igm_last_error(const igm_ctx* ctx);
/* Use an external hipStream_t (e.g. torch.cuda.current_stream().cuda_stream);
 * NULL restores the context's own stream. */
int igm_ctx_set_stream(igm_ctx* ctx, void* hip_stream);
int igm_ctx_synchronize(igm_ctx* ctx);
/* Milliseconds of the last launch of the named kernel family measured with
 * HIP events on the context stream ("actdist", "anneal", "hic_select", ...). */
double igm_last_kernel_ms(const igm_ctx* ctx, const char* name);
const char* igm_version(void);

/* ---- A-step: activation distances ------------------------------------------
 * Replaces the per-pair loop ActivationDistanceStep.task (py:215-222) and
 * get_actdist (py:336-485) over the WHOLE kept-pair list in one call, and the
 * text round trip of task/reduce (py:228-230, 249): the emitted dist/prob are
 * float32(float('%10.4f' % ad)) and float32(float('%.4f' % p)), bit-exact.
 */
typedef struct {
    int32_t i, j;  /* haploid loci, i != j expected (i == j -> no rows)  */
    double pwish;  /* target probability (hcs value, f32 widened)        */
    double plast;  /* previous iteration's corrected probability         */
} igm_pair;        /* 24 bytes: the row layout of the reference '<b>.in.npy' batches */

typedef struct {
    int32_t row, col; /* diploid bead indices                                */
    float dist, prob; /* actdist.hdf5 {row i4, col i4, dist f4, prob f4}     */
} igm_actdist_row;

typedef struct {
    double ad;     /* sqrt of the o-th smallest d^2 (f64), NaN if no rows */
    double p;      /* corrected probability used (f64)                    */
    double pnow;   /* count(d^2 <= rcut^2) / (n*S)                        */
    int32_t o;     /* order statistic index, -1 if no rows                */
    int32_t nrows; /* rows emitted: 0, or one per copy combination --     */
                   /* min(|ii|,|jj|) intra, |ii|*|jj| inter (1..16 for    */
                   /* up to four copies per locus)                        */
} igm_pair_result;

int igm_astep_actdist(igm_ctx* ctx, uint32_t flags,
                      const float* xyz, /* bead-major (nbead, nstruct, 3) f32, the .hss layout */
                      int32_t nbead, int32_t nstruct,
                      const float* radii,     /* (nbead)                                      */
                      const int32_t* copy_ptr, /* (nhap+1) CSR of index.copy_index             */
                      const int32_t* copy_idx, /* diploid bead ids                             */
                      int32_t nhap,
                      const int32_t* chrom, /* chrom[i] as the reference indexes it (hss index.chrom) */
                      const igm_pair* pairs, int64_t npairs,
                      double contact_range, int32_t it_corr,
                      igm_pair_result* per_pair,                         /* (npairs) or NULL */
                      igm_actdist_row* rows, int64_t row_capacity,       /* CSR pair order   */
                      int64_t* nrows_out);                               /* host pointer     */

/* Next-iteration plast (ActivationDistanceStep.setup:144-160 applied to the rows
 * this A-step emitted): pairs[q].plast = float32('%.4f' % p_q) if the pair emitted
 * rows, else 0.  Valid when the same pair list is used again (same sigma). */
int igm_astep_update_plast(igm_ctx* ctx, uint32_t flags, igm_pair* pairs, int64_t npairs,
                           const igm_pair_result* per_pair);

/* ---- A-steps of configurations D/E ------------------------------------------
 * DamID: DamidActivationDistanceStep.task over ALL selected loci in one call
 * (igm/steps/DamidActivationDistanceStep.py:223-287; get_damid_actdist_I :376-471),
 * shapes 'sphere' (shape 0, nucleus_param[0] = radius) and 'ellipsoid' (shape 1,
 * nucleus_param[0..2] = semiaxes), followed by the "%6d %.5f %.5f" text round trip
 * of task()/reduce() (:35, :286, :308): rows are bit-exact
 * {i, float32(float('%.5f' % ad)), float32(float('%.5f' % p))} for every copy i of
 * every locus, in locus order.  loci[q] is a haploid locus, p_exp[q]/plast[q] the
 * float32 values setup() stores (:199-217).  per_locus[q] (nullable) reports ad, p,
 * pnow, o (-1 when p <= 0: the dist is then 2) and nrows. */
/* shape 2 = exp_map: get_damid_actdist_exp (:475-577) with snormsq_exp (:79-115) on the
 * volumetric maps staged by igm_mstep_set_volumes (struct_map = the map of every
 * structure, volumes_idx); distances ascending, pnow = count(d^2 >= contact_range),
 * dist 1e-9 when p <= 0 (nucleus_param and radii unused).
 * shape 3 = the nuclear-body form of the same step: get_damid_actdist_exp of
 * igm/steps/NuclDamidActivationDistanceStep.py:476-570, whose snormsq_exp (:78-110)
 * measures voxel to voxel inside the grid, |(voxel - edt(voxel)) * grid|^2; the
 * out-of-grid branch, the sort, pnow and the rows are those of shape 2. */
#define IGM_DAMID_SPHERE 0
#define IGM_DAMID_ELLIPSOID 1
#define IGM_DAMID_EXP_MAP 2
#define IGM_DAMID_EXP_MAP_NUCL 3

typedef struct {
    int32_t loc; /* diploid bead index                               */
    float dist;  /* damid_actdist.hdf5 {loc i4, dist f4, prob f4}    */
    float prob;
} igm_damid_row;

int igm_damid_actdist(igm_ctx* ctx, uint32_t flags,
                      const float* xyz, int32_t nbead, int32_t nstruct, /* bead-major (nbead, nstruct, 3) */
                      const float* radii,
                      const int32_t* copy_ptr, const int32_t* copy_idx, int32_t nhap,
                      const int32_t* loci, const float* p_exp, const float* plast, int32_t nloci,
                      int32_t it_corr, double contact_range, int32_t shape, const double* nucleus_param,
                      igm_pair_result* per_locus,                  /* (nloci) or NULL */
                      igm_damid_row* rows, int64_t row_capacity,
                      int64_t* nrows_out);                         /* host pointer    */

/* FISH: FishAssignmentStep.task (igm/steps/FishAssignmentStep.py:188-242) for all
 * items at once.  kind 0: items = probes (haploid loci), per structure the min and
 * max over the copies of |x| (get_rad_dists, :44-58); kind 1: items = (i, j) pairs,
 * min/max over every copy pair of |x_a - x_b| (get_pair_dists' documented intent,
 * :23-41).  Distances are float32 np.linalg.norm values.  Each structure's rank
 * r = argsort(argsort(d)) (:60-77; ties in structure order) selects the target:
 * out[q, s] = target[q, r].  target_* / out_* / dist_* are (nitems, nstruct) f32;
 * every output pointer may be NULL (then its target may be NULL too). */
int igm_fish_assign(igm_ctx* ctx, uint32_t flags,
                    const float* xyz, int32_t nbead, int32_t nstruct,
                    const int32_t* copy_ptr, const int32_t* copy_idx, int32_t nhap,
                    int32_t kind, const int32_t* items, int32_t nitems,
                    const float* target_min, const float* target_max,
                    float* out_min, float* out_max, float* dist_min, float* dist_max);

/* Polymer distances: PolymerAssignmentStep.task (igm/steps/PolymerAssignmentStep.py:
 * 84-129) for all loci at once.  For locus i (0 <= i < nbead - 1) the S float32
 * distances |x_i - x_(i+1)| (get_polymer_dists, :24-32) are ranked -- argsort(argsort)
 * with ties in structure order -- and structure s receives the rank-th smallest of the
 * S values drawn by np.random.choice(edges, S, p=prob) (:113): uniforms[q, s] are the
 * random_sample() draws of that call for loci[q] (the caller's RandomState, in the
 * reference's locus order), a draw's bin is searchsorted(cumsum(p) / sum, u, 'right').
 * nn_dist (nloci, nstruct) f32 = the float64 edge value rounded to float32 (the 'f4'
 * dataset of reduce(), :158-162); dist (nloci, nstruct) f32 or NULL.  Host pointers
 * for edges / prob (nbins float64 each). */
int igm_polymer_assign(igm_ctx* ctx, uint32_t flags,
                       const float* xyz, int32_t nbead, int32_t nstruct,
                       const int32_t* loci, int32_t nloci, const double* uniforms,
                       int32_t nbins, const double* edges, const double* prob,
                       float* nn_dist, float* dist);

/* Population contact map: the simulated Hi-C counts HicEvaluationStep.reduce
 * (igm/steps/HicEvaluationStep.py:96-179) builds with HssFile.buildContactMap
 * (contactRange) at :109 (alabtools, absent here: the contact test restated is the
 * IGM Hi-C one, |x_i - x_j| (float32 norm, inter_hic.py:47) <= fl32(contact_range *
 * fl32(r_i + r_j))); the commented-out task of HicEvaluationStep.py:89-91 uses a
 * strict '<', which differs only for a distance exactly at the bound).
 * counts (nbead, nbead) int32, symmetric, diagonal included, =
 * the number of structures in contact; the caller divides by nstruct and sums the
 * copies (Contactmatrix.sumCopies, :111-112). */
int igm_contact_map(igm_ctx* ctx, uint32_t flags,
                    const float* xyz, int32_t nbead, int32_t nstruct,
                    const float* radii, double contact_range, int32_t* counts);

/* The same counts with the copies summed on the device (Contactmatrix.sumCopies,
 * HicEvaluationStep.py:111-112): counts (nhap, nhap) int32 = sum over the copy pairs
 * (a_k, b_l) of the diploid counts -- reduce()'s matrix before the division by nstruct,
 * without the (nbead, nbead) intermediate (3.6 GB at 200 kb).  copy_ptr / copy_idx
 * (host pointers, CSR of index.copy_index) must cover every bead exactly once. */
int igm_contact_map_haploid(igm_ctx* ctx, uint32_t flags,
                            const float* xyz, int32_t nbead, int32_t nstruct,
                            const float* radii, double contact_range,
                            const int32_t* copy_ptr, const int32_t* copy_idx, int32_t nhap, int32_t* counts);

/* SPRITE: SpriteAssignmentStep.task (igm/steps/SpriteAssignmentStep.py:105-160):
 * compute_gyration_radius (igm/cython_compiled/sprite.pyx:104-283, get_rg2s_cpp
 * cpp_sprite_assignment.cpp:49-143) for every (cluster, structure), then keep_best.
 * A "region" is a haploid segment with its copies alt_bead[alt_ptr[r]..alt_ptr[r+1]).
 * Cluster c has the segments seg_region[seg_ptr[c]..seg_ptr[c+1]) in output order
 * and the representatives rep_region[rep_ptr[c]..rep_ptr[c+1]) (one per chromosome,
 * drawn by the caller as sprite.pyx:231 does); seg_rep[g] is the slot of segment
 * g's chromosome among its cluster's representatives.  A cluster without
 * representatives is a single-chromosome cluster (every copy k is one group).
 * Outputs: rg2_out (ncluster, nstruct) f32 (nullable); best_idx/best_rg2
 * (ncluster, keep_best); best_sel: cluster c's (keep_best, nseg_c) selected beads at
 * offset seg_ptr[c] * keep_best.  Host pointers only (the CSR arrays are validated). */
int igm_sprite_assign(igm_ctx* ctx, uint32_t flags,
                      const float* xyz, int32_t nbead, int32_t nstruct,
                      int32_t ncluster, const int32_t* seg_ptr, const int32_t* seg_region,
                      const int32_t* seg_rep, const int32_t* rep_ptr, const int32_t* rep_region,
                      int32_t nregion, const int32_t* alt_ptr, const int32_t* alt_bead,
                      int32_t keep_best, float* rg2_out,
                      int32_t* best_idx, float* best_rg2, int32_t* best_sel);

/* Chromatin tracing: the A-step the reference leaves open (bin/igm-run:122-136, its
 * ImagedLociAssignmentStep is commented out).  Trace t is the imaged positions (nm, any
 * frame) of the haploid loci locus[trace_ptr[t]..trace_ptr[t+1]) of one chromosome copy:
 * at least 3 spots, loci strictly increasing, every locus with the same number of copies
 * C_t.  A candidate is (structure s, copy k < C_t) with the beads
 * x_i = xyz[copy_idx[copy_ptr[locus_i] + k], s]; its cost is the minimal RMSD under a proper
 * rigid motion (rotation with det = +1 and translation, no reflection),
 * sqrt(max(0, (Ga + Gb - 2 lambda) / n)) with Ga, Gb the centred sums of squares and lambda the
 * largest eigenvalue of Horn's 4x4 key matrix, accumulated in fp64 from the f32 coordinates.
 * Cmax is the largest C_t of the call.  Outputs: rmsd_out (ntrace, nstruct, Cmax) f32
 * (nullable), +inf where k >= C_t; best_cand / best_rmsd (ntrace, keep_best): the keep_best
 * smallest f32 costs of every trace in increasing order, ties to the lower candidate index
 * s * Cmax + k.  IGM_E_INVALID: a malformed trace, keep_best < 1, keep_best larger than the
 * smallest nstruct * C_t.  Host pointers only (the arrays are validated on the host, before
 * any launch).  Timings: igm_last_kernel_ms "tracing_assign" (= "tracing_cost" +
 * "tracing_select"). */
int igm_tracing_assign(igm_ctx* ctx, uint32_t flags,
                       const float* xyz, int32_t nbead, int32_t nstruct,
                       const int32_t* copy_ptr, const int32_t* copy_idx, int32_t nhap,
                       int32_t ntrace, const int64_t* trace_ptr, const int32_t* locus, const float* position,
                       int32_t keep_best,
                       float* rmsd_out,       /* (ntrace, nstruct, Cmax) f32 or NULL; +inf where k >= C_t */
                       int32_t* best_cand,    /* (ntrace, keep_best): s * Cmax + k                        */
                       float* best_rmsd);     /* (ntrace, keep_best)                                      */

/* Chromatin tracing on imaged cells: the traces cell_ptr[c]..cell_ptr[c+1] were imaged in one
 * cell and share its frame (multiplexed FISH, seqFISH), so cell c is placed on structure s
 * under ONE proper rigid motion and one homologue labelling L: every trace a copy of its
 * chromosome, no copy of a chromosome twice.  trace_chrom[t] is the chromosome of trace t (any
 * ids: the chromosome table is the caller's, as for igm_tracing_assign); a cell holds at most C
 * traces of a chromosome of C copies.  With q_i the spots centred on the cell, x_i the beads
 * minus the bead of the cell's first spot under copy 0, and per (trace, copy) the fp64 sums
 * sx = sum x_i, sxx = sum |x_i|^2, m[a][b] = sum q_a x_b, the cost of L is
 *   sqrt(max(0, (Ga + Gb - 2 lambda) / n)),  n = all spots, Ga = sum |q_i|^2, SX = sum sx(t, L_t),
 *   Gb = max(0, sum sxx - |SX|^2 / n), lambda the largest eigenvalue of Horn's key matrix of
 *   M = sum m(t, L_t); R the rotation of its unit eigenvector, tau = SX / n.
 * L is found by a deterministic alternating search.  Start: per chromosome the injective
 * labelling of least sum of e(t, k), the trace's own centred Kabsch residual.  Round: the joint
 * (cost, R, tau) of L, then per chromosome the labelling of least sum of the residuals
 *   r(t, k) = sqq_t + sxx + n_t |tau|^2 + 2 tau . (R sq_t) - 2 tau . sx - 2 sum_ab R_ba m_ab
 * (sq_t, sqq_t: sum q_i, sum |q_i|^2 of the trace), taken only if strictly below the current
 * labelling's.  Labellings go in lexicographic order of (copy of the chromosome's 1st trace,
 * 2nd, ...), the first minimum wins.  The search stops when no chromosome moves or after 16
 * rounds; the cost never increases, the end is a local optimum.
 * Outputs: cost_out (ncell, nstruct) f32, label_out (ntrace, nstruct) the copy of every trace,
 * rounds_out (ncell, nstruct) the re-labelling rounds made, the last of which moved nothing
 * unless it was the 16th (all nullable); best_struct / best_cost (ncell, keep_best): the
 * keep_best cheapest structures of every cell in increasing order, ties to the lower s;
 * best_label (ntrace, keep_best): the copy of every trace at that candidate.
 * The sums live in a device scratch of scratch_bytes (0: 1 GiB); the cells are processed in
 * batches that fit it, and the outputs do not depend on the batching.
 * IGM_E_INVALID: a malformed trace or cell_ptr, too many traces of a chromosome in a cell,
 * keep_best < 1 or > nstruct.  IGM_E_UNSUPPORTED: a cell of more than 128 traces or a chromosome
 * of more than 4 copies, a single cell whose sums do not fit scratch_bytes.  Host pointers only
 * (validated on the host, before any launch).  Timings: igm_last_kernel_ms "tracing_cells"
 * (= "tracing_cell_sums" + "tracing_cell_search" + "tracing_cell_select", each summed over the
 * batches). */
int igm_tracing_assign_cells(igm_ctx* ctx, uint32_t flags,
                             const float* xyz, int32_t nbead, int32_t nstruct,
                             const int32_t* copy_ptr, const int32_t* copy_idx, int32_t nhap,
                             int32_t ntrace, const int64_t* trace_ptr, const int32_t* locus, const float* position,
                             const int32_t* trace_chrom,
                             int32_t ncell, const int64_t* cell_ptr,
                             int32_t keep_best, int64_t scratch_bytes,
                             float* cost_out,       /* (ncell, nstruct) f32 or NULL  */
                             uint8_t* label_out,    /* (ntrace, nstruct) or NULL     */
                             uint8_t* rounds_out,   /* (ncell, nstruct) or NULL      */
                             int32_t* best_struct,  /* (ncell, keep_best)            */
                             float* best_cost,      /* (ncell, keep_best) ascending, ties to the lower s */
                             uint8_t* best_label);  /* (ntrace, keep_best)           */

/* DamID lamina envelope membership (M-step restraint assembly, config D):
 * Damid._apply_envelope (igm/restraints/damid.py:112-143) for every structure at once.
 * out_flags[s, a] = base_flags[a] | (env_bit if some DamID row {loc = a, dist = d}
 * has snormsq_ellipsoid(x_sa, semiaxes * (1 - contact_range), r_a) >= d^2), bit-exact
 * with the reference's NumPy 1.x arithmetic.  xyz is the M-step layout
 * (nstruct, natom, 3); the result feeds igm_mstep_run with IGM_MSTEP_STRUCT_FLAGS and
 * an envelope whose k is -contact_kspring.  n_selected (nullable): rows selected per
 * structure (the restraint's rnum). */
int igm_damid_select(igm_ctx* ctx, uint32_t flags, int32_t nstruct, int32_t natom, const float* xyz,
                     const float* radii, const igm_damid_row* rows, int64_t nrows,
                     const double* semiaxes, double contact_range, uint32_t env_bit,
                     const uint32_t* base_flags, uint32_t* out_flags, int32_t* n_selected);

/* Volumetric nuclear-body maps (VolumeFile .bin, igm/utils/files.py:137-166): header
 * int32 body_idx (0 nucleus, 1 nucleolus), int32[3] nvoxel, f32[3] center, origin, grid,
 * then int32 [nx][ny][nz][4] = (nearest-lamina voxel i, j, k, inside flag).
 * The LAMMPS fix's force form is not in the reference (lammpgen is external, SURVEY
 * M7d: parity unpinned).  Implemented form, per member atom of a volume envelope:
 *   v = round((x - envf*origin) / (envf*grid)) clamped to the grid; if the voxel
 *   violates the restraint (nucleus, k>0: outside; nucleolus, k>0: inside; k<0: the
 *   opposite, as ExpEnvelope.getScores, forces.py:306-417) the atom is pulled to the
 *   centre of its nearest lamina voxel p = envf*(origin + grid*edt(v)):
 *   E = |k|/2 |x - p|^2, F = -|k| (x - p).
 * Violation scores restate ExpEnvelope.getScores exactly (contact_range 0.95 geometry
 * shrink for k<0, its index quirks included). */
typedef struct {
    int32_t body_idx;
    int32_t nvoxel[3];
    float center[3], origin[3], grid[3];
    const int32_t* voxels; /* host pointer: nx*ny*nz*4 int32 */
} igm_volume_map;

/* Stage maps in the context for later igm_mstep_* calls: struct_map[s] selects the
 * map of structure s of a batch (volumes_idx[sid % len], ModelingStep.py:265-270);
 * NULL = map 0 for every structure.  nmap = 0 clears. */
int igm_mstep_set_volumes(igm_ctx* ctx, int32_t nmap, const igm_volume_map* maps,
                          const int32_t* struct_map, int32_t nstruct);

/* One table per envelope: env_map[s] is the index into the staged maps that envelope
 * `env` (0 <= env < IGM_MAX_ENVELOPES) reads for structure s of the next igm_mstep_*
 * calls, so a nucleolus body can sit beside the nucleus map.  NULL restores the default
 * table (struct_map above); igm_mstep_set_volumes clears every per-envelope table.
 * Host pointer; indices are checked against the staged maps, nstruct against the batch
 * size of the calls that follow. */
int igm_mstep_set_envelope_maps(igm_ctx* ctx, int32_t env, const int32_t* env_map, int32_t nstruct);

/* Volumetric lamina membership (M-step restraint assembly): GenDamid._apply_envelope
 * (igm/restraints/gendamid.py:17-47,101-107) for every structure at once, on the maps
 * staged by igm_mstep_set_volumes.  out_flags[s, a] = base | (env_bit if some row
 * {loc = a, dist = d} has snormsq_exp(x_sa, map struct_map[s]) < d**2), bit-exact with
 * the reference's NumPy 1.x arithmetic (d**2 is float64(d)^2).  struct_map[s] is
 * the index into the staged maps (NULL: the default table of igm_mstep_set_volumes).
 * base_flags is (natom), or (nstruct, natom) when base_per_struct != 0 -- the output of
 * an earlier selection, so the lamina and the nuclear-body selections compose on one
 * array.  Rows whose loc is outside [0, natom) are ignored; nrows = 0 is valid.
 * n_selected (nullable): rows selected per structure.  The result feeds igm_mstep_run
 * with IGM_MSTEP_STRUCT_FLAGS and a volume envelope whose k is -contact_kspring. */
int igm_volume_select(igm_ctx* ctx, uint32_t flags, int32_t nstruct, int32_t natom, const float* xyz,
                      const igm_damid_row* rows, int64_t nrows, const int32_t* struct_map,
                      uint32_t env_bit, const uint32_t* base_flags, int32_t base_per_struct,
                      uint32_t* out_flags, int32_t* n_selected);

/* ---- M-step ---------------------------------------------------------------
 * Batched replacement of lammps.optimize (lammps.py:361-492): the protocol of
 * create_lammps_script (lammps.py:149-358) -- per stage: fix adapt of the soft
 * prefactor, envelope scaling, optional relax run, velocity create, temp/rescale
 * ramp, nve/limit -- followed by min_style cg.  One structure per workgroup:
 * structures of up to 3072 atoms (2 Mb diploid) keep positions and the Verlet
 * list in LDS; larger ones (200 kb diploid: 29 838 beads) keep them in HBM.
 */
#define IGM_MAX_STAGES 16
#define IGM_MAX_ENVELOPES 4

typedef struct {
    int32_t nstages;
    int32_t mdsteps[IGM_MAX_STAGES];
    double tstart[IGM_MAX_STAGES];
    double tstop[IGM_MAX_STAGES];
    double evfactor[IGM_MAX_STAGES];  /* fix adapt 'pair soft a' scale   */
    double envfactor[IGM_MAX_STAGES]; /* semiaxes * envf                 */
    int32_t relax_steps;              /* 0: no relax run                 */
    double relax_temperature;
    double relax_max_velocity;
    double timestep;     /* 0.25                                       */
    double max_velocity; /* nve/limit xmax (distance per step)         */
    double t_window;     /* temp/rescale window (0.1)                  */
    double t_fraction;   /* temp/rescale fraction (1.0)                */
    double etol, ftol;   /* minimize etol ftol                         */
    int32_t max_cg_iter, max_cg_eval;
    double dmax;         /* min_modify dmax (LAMMPS default 0.1)       */
    double evfactor_base;/* Steric k -> LammpsModel.evfactor           */
    double skin;         /* neighbour skin (LAMMPS: 'neighbor maxrad') */
    int32_t nenvelopes;
    double env_semiaxes[IGM_MAX_ENVELOPES][3];
    double env_k[IGM_MAX_ENVELOPES];
    int32_t neigh_capacity; /* HBM neighbour-list budget, mean entries per atom (0 = 64); atoms past
                               the budget take their pair forces from a walk of the build-time cell grid.
                               The population engine (structures too large for LDS) lists up to 256
                               entries per atom when this is 0 or 64, else min(this, 256); its
                               HBM is ~(120 + 2 x entries + 8 x max bond degree) B per atom per
                               structure (the 256-entry lists alone 15.3 GB for 1000 x 29 839 atoms), checked against the free
                               HBM before the run (IGM_E_NOMEM names the per-structure cost) */
    int32_t flags;          /* IGM_MSTEP_* below                        */
    int32_t env_kind[IGM_MAX_ENVELOPES]; /* IGM_ENV_ELLIPSOID (0) or IGM_ENV_VOLUME (1)  */
} igm_mstep_params;

/* envelope kinds (igm_mstep_params.env_kind) */
#define IGM_ENV_ELLIPSOID 0 /* fix ellipsoidalenvelope a b c k (lammps.py:292-303)              */
#define IGM_ENV_VOLUME 1    /* fix volumetricrestraint file envf k (lammps.py:305-310) with the
                               map of igm_mstep_set_volumes; env_semiaxes unused */

/* igm_mstep_params.flags */
#define IGM_MSTEP_FORCE_GLOBAL 0x1 /* use the HBM-resident kernels even when a structure fits in LDS */
#define IGM_MSTEP_STRUCT_FLAGS 0x2 /* atom_flags is (nstruct, natom): per-structure envelope membership
                                      (DamID) and active/inactive centroid slots (SPRITE); the
                                      IGM_ATOM_BEAD bit must be the same in every structure */
/* 0x4 is retired (round 3's domain-decomposed engine, 2x slower than the population engine on
   the 200 kb model, profiles/history_r01_r04.md): igm_mstep_run returns IGM_E_UNSUPPORTED for it */

/* atom flags (per atom, shared by all structures of a batch) */
#define IGM_ATOM_BEAD 0x1u   /* takes part in the soft pair potential       */
#define IGM_ATOM_FIXED 0x2u  /* setforce 0 / not integrated (static dummy)   */
#define IGM_ATOM_ENV0 0x10u  /* member of envelope e: IGM_ATOM_ENV0 << e     */

typedef struct {
    uint32_t i, j; /* atom indices; bit 31 of j set = harmonic_lower_bound */
    float r0, k;   /* E = k (r - r0)^2 beyond the bound (bond_harmonic form) */
} igm_bond;

typedef struct {
    double final_energy; /* E_pair + E_bond + sum E_env after CG ('final-energy') */
    double pair_energy;  /* thermo epair                                        */
    double bond_energy;  /* thermo ebond                                        */
    double env_energy[IGM_MAX_ENVELOPES]; /* thermo f_envelope<e>               */
    double temp;         /* thermo temp (group all)                             */
    double einitial;     /* energy at the start of CG                           */
    double fnorm_final;  /* |F|_2 at the end of CG                              */
    int32_t cg_iters, cg_evals, stop_reason, nrebuild;
} igm_opt_info;

/* Position anchors (chromatin tracing, igm/restraints/tracing.py): a harmonic upper bound
 * between an atom and a fixed point, per structure -- the reference's DUMMY_STATIC centroid
 * with HarmonicUpperBound(centroid, locus, radial_tolerance, k), without the centroid atom.
 *   r = |x_atom - (x, y, z)|:  E = k (r - r0)^2 for r > r0, else 0 (the igm_bond form); the
 *   force on the atom follows from E and is 0 at r = 0.  The target is f32 (as a dummy's
 *   position would be) and no stage's envelope factor scales it.
 * The energy is bond energy (igm_opt_info.bond_energy, energies[2]).  An atom may carry
 * several anchors, evaluated in the order given; an IGM_ATOM_FIXED atom contributes energy
 * and takes no force.  igm_opt_info.temp (thermo temp of group all) counts every anchor of
 * the structure as one more motionless atom, dof = 3 (natom + n_anchor) - 3, which is the
 * reference's count with one centroid atom per restraint; the reference merges consecutive
 * coincident dummies (lammps_model.py:303-312) and that merge is not restated.  Anchors are
 * not atoms: temp/rescale, velocity create and the CG degrees of freedom do not see them. */
typedef struct {
    uint32_t atom;
    float x, y, z; /* target                                             */
    float r0, k;   /* E = k (r - r0)^2 beyond r0                         */
} igm_anchor;      /* 24 bytes */

/* Stage anchors in the context for the igm_mstep_* calls that follow, as igm_mstep_set_volumes
 * stages maps: structure s of a batch has anchors[anchor_ptr[s] .. anchor_ptr[s+1]) (host
 * pointers, copied).  nstruct = 0 clears.  IGM_E_INVALID here: anchor_ptr not monotone from 0,
 * r0 < 0, a non-finite target, r0 or k.  IGM_E_INVALID at the run: nstruct different from the
 * batch of the call, atom >= natom.  igm_mstep_run, igm_mstep_forces (both paths) and
 * igm_mstep_md apply the staged anchors; with nothing staged they launch the kernels of a
 * library without anchors.  Device memory: 24 B per anchor and 4 B per (structure, atom),
 * allocated before the population engine's memory check reads the free HBM. */
int igm_mstep_set_anchors(igm_ctx* ctx, int32_t nstruct, const int64_t* anchor_ptr, const igm_anchor* anchors);

/* Run the whole protocol for `nstruct` structures of `natom` atoms each.
 *   xyz       (nstruct, natom, 3) f32, in/out
 *   radii     (natom) f32; atom_flags (natom), or (nstruct, natom) with IGM_MSTEP_STRUCT_FLAGS
 *   bonds     shared bonds (polymer) + per-structure bonds (Hi-C ...):
 *             shared_bonds[nshared]; sbond_ptr[nstruct+1] into sbonds[]
 *   seeds     (nstruct) LAMMPS 'velocity create' seed of stage 0 (stage k: +k)
 *   info      (nstruct) or NULL                                              */
int igm_mstep_run(igm_ctx* ctx, uint32_t flags, const igm_mstep_params* prm,
                  int32_t nstruct, int32_t natom, float* xyz,
                  const float* radii, const uint32_t* atom_flags,
                  const igm_bond* shared_bonds, int64_t nshared,
                  const int64_t* sbond_ptr, const igm_bond* sbonds,
                  const int32_t* seeds, igm_opt_info* info);

/* Energy/force evaluation only (parity harness for the force field):
 * forces (nstruct, natom, 3) f32 and per-structure energies. evf/envf are the
 * stage factors to apply.  energies: (nstruct, 3 + IGM_MAX_ENVELOPES) f64 =
 * {total, pair, bond, env0..env3}.  Default: the f64 path of the CG kernel;
 * with IGM_F32_PATH: the f32 path of the MD kernel (energies are NaN). */
int igm_mstep_forces(igm_ctx* ctx, uint32_t flags, const igm_mstep_params* prm,
                     int32_t nstruct, int32_t natom, const float* xyz,
                     const float* radii, const uint32_t* atom_flags,
                     const igm_bond* shared_bonds, int64_t nshared,
                     const int64_t* sbond_ptr, const igm_bond* sbonds,
                     double evf, double envf, float* forces, double* energies);

/* Short deterministic MD segment (parity harness): `nsteps` nve/limit steps
 * with temp/rescale ramp t0->t1 from the given velocities (no velocity create).
 * v (nstruct, natom, 3) in/out. */
int igm_mstep_md(igm_ctx* ctx, uint32_t flags, const igm_mstep_params* prm,
                 int32_t nstruct, int32_t natom, float* xyz, float* v,
                 const float* radii, const uint32_t* atom_flags,
                 const igm_bond* shared_bonds, int64_t nshared,
                 const int64_t* sbond_ptr, const igm_bond* sbonds,
                 double evf, double envf, double t0, double t1, double max_velocity,
                 int32_t nsteps);

/* LAMMPS 'velocity <group> create T seed' as the reference script issues it
 * (lammps.py:322,335: dist uniform, loop all, mom yes, Park-Miller RanPark):
 * one velocity set per seed, atoms with IGM_ATOM_FIXED get 0 (not in the
 * 'nonfixed' group) but still consume their random numbers.  v: (nseed, natom, 3). */
int igm_velocity_create(igm_ctx* ctx, uint32_t flags, int32_t nseed, int32_t natom,
                        const uint32_t* atom_flags, const int32_t* seeds, double temperature,
                        float* v);

/* Profiling aid: with IGM_PROF set in the environment, the LDS-path anneal kernel
 * accumulates shader-clock cycles; out[6] = {neighbour builds, force phases, rest,
 * force evaluations, builds, list-fill walks (part of the builds)} summed over the
 * structures of the last launch. */
int igm_mstep_last_profile(igm_ctx* ctx, unsigned long long* out);

/* ---- M-step restraint assembly: Hi-C contact selection ---------------------
 * interHiC/intraHiC._apply (restraints/inter_hic.py:294-312, intra_hic.py) for
 * every actdist row and every structure: a bond (i, j) is imposed when
 * ||x_i - x_j|| <= dist (f32, no FMA) and the chromosome test holds.
 *   xyz (nstruct, natom, 3) struct-major; act rows (n_act): igm_astep_actdist output;
 *   chrom (natom); output per-structure CSR of bonds, inter rows first then
 *   intra rows (the reference order), r0 = cr*(r_i + r_j), k; out_class (may be
 *   NULL) receives inter_class / intra_class for each bond (violation classes).
 * Two-phase: call with out_bonds == NULL to get out_ptr (nstruct+1) filled and
 * the total in *ntotal; then call again with out_bonds sized *ntotal. */
int igm_hic_select(igm_ctx* ctx, uint32_t flags,
                   int32_t nstruct, int32_t natom, const float* xyz,
                   const float* radii, const int32_t* chrom,
                   const igm_actdist_row* act, /* the A-step rows (actdist.hdf5 row/col/dist/prob) */
                   int64_t n_act, double contact_range, double kspring,
                   int32_t inter_class, int32_t intra_class,
                   int64_t* out_ptr, igm_bond* out_bonds, int32_t* out_class, int64_t* ntotal);

/* Population layout change between the .hss / A-step layout (bead-major
 * (nbead, nstruct, 3), core/step.py:373) and the M-step layout (struct-major
 * (nstruct, natom, 3), natom >= nbead; extra atoms left untouched).
 * direction 0: bead-major -> struct-major; 1: struct-major -> bead-major. */
int igm_population_transpose(igm_ctx* ctx, uint32_t flags, int32_t nbead, int32_t nstruct, int32_t natom,
                             const float* src, float* dst, int32_t direction);

/* ---- M-step violation scoring (ModelingStep.py:511-557,859-869) ------------
 * For each structure and each restraint class c -- bond classes 0..nclass_bonds-1
 * (class ids parallel to shared_bonds / sbonds), then envelope e as class
 * nclass_bonds + e -- the ModelingStep.task record: histogram of 100 bins on
 * [0,1] + overflow (np.histogram semantics), violated_restr (ratio != 0),
 * n_violations (ratio > tol) and n_imposed.
 *   bond ratio    k (r - d) / (k d) past the bound, d = class_cr[c] * f32(r_i + r_j)
 *                 in f64 (forces.py:131-139,178-186); class_cr[c] <= 0: d = bond r0
 *   envelope      EllipticEnvelope.getScores (forces.py:222-247) with the base
 *                 semiaxes, scale env_scale[e] (0.1 * mean(abc), envelope.py:51)
 * stats: (nstruct, nclass_bonds + nenvelopes, 104) int64 =
 *        {counts[101], violated_restr, n_violations, n_imposed}. */
int igm_mstep_violations(igm_ctx* ctx, uint32_t flags, const igm_mstep_params* prm,
                         int32_t nstruct, int32_t natom, const float* xyz,
                         const float* radii, const uint32_t* atom_flags,
                         const igm_bond* shared_bonds, const int32_t* shared_class, int64_t nshared,
                         const int64_t* sbond_ptr, const igm_bond* sbonds, const int32_t* sclass,
                         int32_t nclass_bonds, const double* class_cr, const double* env_scale, double tol,
                         int64_t* stats);

/* The ModelingStep record of the staged anchors (vstat key 'Tracing', ModelingStep.py:281-300):
 * stats (nstruct, 104) int64, the record layout above; ratio = (r - r0) / r0 past the bound
 * with r the float32 norm, 0 when r0 == 0 (forces.py:131-139); n_imposed = the structure's
 * anchors.  xyz (nstruct, natom, 3) f32. */
int igm_mstep_anchor_violations(igm_ctx* ctx, uint32_t flags, int32_t nstruct, int32_t natom,
                                const float* xyz, double tol, int64_t* stats);

/* ---- population report (the igm/report modules, driven by bin/igm-report) ----------
 * The structural numbers of the report on the bead-major .hss population: xyz is
 * always (nbead, nstruct, 3) f32.  xyz and the outputs follow `flags`
 * (IGM_DEVICE_PTRS); semiaxes, edges, CSR arrays, hap_chrom and inv_denoms are host
 * pointers in every mode.  Every floating-point sum has a fixed order: a rerun is
 * bitwise equal. */

/* Radial levels: get_radial_level (igm/report/radials.py:15-39), plot_radial_density
 * (:69-87) and report_shells (igm/report/shells.py:9-43).  The level of (bead,
 * structure) is sqrt(((x/a)^2 + (y/b)^2) + (z/c)^2) in float64 on the widened
 * coordinates, bit-equal to np.sqrt(np.sum(np.square(crd / semiaxes), axis=1)).
 * Outputs, each may be NULL:
 *   level_mean     (nbead) f64: the mean over the structures (summed in structure order)
 *   density_counts (nbins) int64: np.histogram of all nbead * nstruct levels on the
 *                  nbins + 1 density_edges (np.linspace(0, vmax, nbins + 1)): bin k holds
 *                  edges[k] <= v < edges[k+1], the last bin is closed, the rest is dropped
 *   shell_mean     (nstruct, nshell) f64 and shell_hist (nshell, hnbins) int64 on the
 *                  hnbins + 1 shell_edges: per structure the levels are ranked, shell j
 *                  holds the ranks [int(j n / nshell), int((j+1) n / nshell)) (np.partition
 *                  at those ranks); its mean, and its histogram summed over the structures.
 *                  An empty shell (nbead < nshell) gives NaN and no counts.
 * nbead <= 65535, nshell <= 256. */
int igm_report_levels(igm_ctx* ctx, uint32_t flags,
                      const float* xyz, int32_t nbead, int32_t nstruct, const double* semiaxes,
                      double* level_mean,
                      const double* density_edges, int32_t nbins, int64_t* density_counts,
                      int32_t nshell, double* shell_mean,
                      const double* shell_edges, int32_t hnbins, int64_t* shell_hist);

/* Radius of gyration: rg / get_chroms_rgs (igm/report/radius_of_gyration.py:9-41).
 * The chains are a CSR (chain_ptr (nchain + 1), chain_idx bead indices) in
 * index.get_chrom_pos(chrom, copy) order.  rg (nchain, nstruct) f64 =
 * sqrt(sum |p - mean(p)|^2 / n), two passes in float64 over the float32 coordinates in
 * bead order (the reference sums in float32: equal to its rounding).  An empty chain
 * gives NaN. */
int igm_report_rg(igm_ctx* ctx, uint32_t flags,
                  const float* xyz, int32_t nbead, int32_t nstruct,
                  const int32_t* chain_ptr, const int32_t* chain_idx, int32_t nchain, double* rg);

/* Lamina (DamID) contacts: report_damid (igm/report/damid.py:32-51) with
 * snormsq_ellipse (igm/report/utils.py:73-89) as NumPy 2 evaluates it.  inv_denoms
 * (nhap, 3) f64 holds the three denominators of every locus,
 * (semiaxes * (1 - contact_range) - r)**2 with r the radius of its first copy; the
 * value of a copy in a structure is (xx/A + yy/B) + zz/C with xx = fl32(x * x) widened
 * to float64.  counts (nhap) int64 = the number of (copy, structure) with value >= 1;
 * the caller divides by nstruct and the copy count (:50). */
int igm_report_lamina(igm_ctx* ctx, uint32_t flags,
                      const float* xyz, int32_t nbead, int32_t nstruct,
                      const int32_t* copy_ptr, const int32_t* copy_idx, int32_t nhap,
                      const double* inv_denoms, int64_t* counts);

/* ---- the report on an imaged nucleus (nucleus_shape exp_map) ---------------------------
 * The reference has no report for imaged nuclei (its get_damid_actdist_exp counts
 * d_sq >= contact_range on sorted squared distances, which is no contact test): the
 * definitions are this project's, chosen so that on a voxelised sphere they reduce to the
 * ellipsoid forms above up to the voxel size.  Both entries read the maps staged by
 * igm_mstep_set_volumes.  struct_map (nstruct) names the map of every structure; NULL
 * means the table staged with the maps, and map 0 when none was staged (the convention
 * of igm_volume_select).  struct_map, depth_scale, thr, radii and the CSR arrays are host
 * pointers in every mode; xyz and the outputs follow `flags`.  Everything is float64 on
 * the widened float32 coordinates and the widened float32 map geometry.  For a bead p
 * and the map m of its structure:
 *   voxel    v_d = rint((f64 p_d - f64 origin_d) / f64 grid_d), half to even, as the DamID
 *            A-step reads it.  Out of the grid v is clamped to [0, n_d - 1] per axis and
 *            the bead counts as outside.
 *   record   (i, j, k, w) = the voxel record at ((v0 n1 + v1) n2 + v2);
 *            L_d = f64(e_d) * grid_d + origin_d, e = (i, j, k); t = p - L;
 *            dist = sqrt((t0^2 + t2^2) + t1^2), correctly rounded
 *   depth    +dist when the voxel is in the grid and w != 0, else -dist: positive inside
 *            the nucleus, 0 on a lamina voxel's centre, negative outside
 *   level    max(0, 1 - depth / depth_scale[m]): 1 on the lamina, 0 on the deepest voxel
 *            centre when depth_scale[m] is the largest |(v - e) * grid| over the voxels
 *            with w != 0 (igm_amd.report.map_depth_scale), above 1 outside.  The clamp is
 *            required: a bead off the centre of a deep voxel has depth > depth_scale, and
 *            the shells are selected on the bit patterns of non-negative doubles.  The
 *            sign bit of a level is clear.
 * IGM_E_INVALID: no maps staged, a struct_map entry outside [0, nmap), a staged table
 * shorter than nstruct, a depth_scale that is not finite and positive, a non-finite thr,
 * side not +1 / -1.  The context stays usable. */

/* Levels on the maps: the outputs of igm_report_levels -- same semantics, limits
 * (nbead <= 65535, nshell <= 256: IGM_E_UNSUPPORTED) and NULL rules -- on the level above,
 * and
 *   depth_mean     (nbead) f64: the mean signed depth over the structures (summed in
 *                  structure order); may be NULL
 * depth_scale (nmap) f64, one per staged map. */
int igm_report_map_levels(igm_ctx* ctx, uint32_t flags,
                          const float* xyz, int32_t nbead, int32_t nstruct,
                          const int32_t* struct_map, const double* depth_scale,
                          double* level_mean, double* depth_mean,
                          const double* density_edges, int32_t nbins, int64_t* density_counts,
                          int32_t nshell, double* shell_mean,
                          const double* shell_edges, int32_t hnbins, int64_t* shell_hist);

/* Contacts with the lamina of the maps, the shape of igm_report_lamina: counts (nhap)
 * int64 = the number of (copy, structure) in contact.  radii (nbead) f32; r is the radius
 * of the locus's FIRST copy, as in igm_report_lamina.  thr (nmap) f64, formed by the
 * caller as contact_range * depth_scale[m].
 *   side = +1  a nucleus map: contact iff depth - f64(r) <= thr[m].  On a sphere this is
 *              the ellipsoid form, |x| >= R (1 - cr) - r  <=>  (R - |x|) - r <= cr R.
 *              Every outside bead is in contact.
 *   side = -1  a body map (a nucleolus; w marks the inside of the body): contact iff
 *              -depth - f64(r) <= thr[m].
 * A locus without copies counts 0. */
int igm_report_map_lamina(igm_ctx* ctx, uint32_t flags,
                          const float* xyz, int32_t nbead, int32_t nstruct,
                          const int32_t* copy_ptr, const int32_t* copy_idx, int32_t nhap,
                          const float* radii, const int32_t* struct_map, const double* thr,
                          int32_t side, int64_t* counts);

/* Average distance map: create_average_distance_map (igm/report/distance_map.py:5-22).
 * dmap (nhap, nhap) f64.  For a copy pair (k, m) the float32 norms
 * sqrt((dx*dx + dy*dy) + dz*dz) (np.linalg.norm(axis=1) on float32) are averaged over
 * the structures in float64, in structure order; entry (a, b), a < b, is the mean of
 * those means over the k-th copy with the k-th copy when hap_chrom[a] == hap_chrom[b]
 * (the reference's zip: up to the smaller copy count), else over every copy of a with
 * every copy of b.  The reference leaves the diagonal and the lower triangle
 * uninitialised: here the diagonal is 0 and the lower triangle mirrors the upper.  An
 * entry without a copy pair is NaN.  copy_ptr / copy_idx: CSR of index.copy_index. */
int igm_report_distance_map(igm_ctx* ctx, uint32_t flags,
                            const float* xyz, int32_t nbead, int32_t nstruct,
                            const int32_t* copy_ptr, const int32_t* copy_idx, const int32_t* hap_chrom,
                            int32_t nhap, double* dmap);

/* Hi-C comparison: the numbers of report_hic (igm/report/hic.py:16-180) as sufficient
 * statistics, from which the caller forms the Pearson correlations, and the two 2-D
 * histograms of input against simulated probability (igm/report/plots.py:28, 98).  No
 * dense floating-point matrix is built anywhere.
 *
 * counts (nhap, nhap) int32: the symmetric output of igm_contact_map_haploid; counts,
 * indices and data follow `flags`.  The input matrix is the CSR hss.read_hcs returns, the
 * upper triangle with the diagonal allowed: indptr (nhap + 1) int64, indices int32, data
 * float32; stored zeros are legal and behave as zeros.  hap_chrom (nhap): any ids in
 * [0, nchrom).  indptr, hap_chrom, the edges and every output are host pointers in every
 * mode.  A sigma <= 0 or NaN means "not given": every stored entry then counts as below it.
 *
 * Per entry (a, b):  y = c' / nstruct (one float64 division) with c' = min(counts[a, b],
 * nstruct) -- the clip of evaluation.contact_map decided on integers; a negative count
 * reads as 0 -- and x = the stored float32 widened to float64, 0 where nothing is stored.
 * Populations p: for a chromosome c every ordered entry with hap_chrom[a] == hap_chrom[b]
 * == c (the full symmetric block with its diagonal, x1d.ravel() of hic.py:60-65: a stored
 * off-diagonal entry has weight w = 2, a diagonal one w = 1, n = m^2 for m loci); p =
 * nchrom is the inter population, the pairs a < b on two chromosomes
 * (np.triu(getInterMask()), :99), w = 1.  Masks: all, restrained (x >= sigma of the
 * population: intra_sigma or inter_sigma), non-restrained (the complement, with every
 * entry that is not stored).
 *
 * Outputs:
 *   dense_sums  (nchrom + 1, 2) int64    {sum c', sum c'^2} over the whole population
 *   sparse_ints (nchrom + 1, 2, 3) int64 over the stored entries with x >= sigma (half 0)
 *               and x < sigma (half 1): {sum w, sum w c', sum w c'^2}
 *   sparse_sumx (nchrom + 1, 2) f64      sum of w x over the two halves
 *   means       (nchrom + 1, 3, 2) f64   per mask (all, restrained, non-restrained)
 *               {ybar, xbar}: ybar = sum c' / (n nstruct), the exact integer quotient
 *               rounded once; xbar = sum x / n, one float64 division; n and the sums of the
 *               mask 'all' are the dense ones (sum x over both halves, half 0 first), of
 *               'restrained' half 0, of 'non-restrained' dense minus half 0 (sum x: half 1);
 *               an empty set has 0
 *   centred     (nchrom + 1, 3, 2) f64   over the stored entries of the mask
 *               {sum (w x) (y - ybar), sum w ((x - xbar) (x - xbar))}.  The first is the
 *               whole cross term (the entries that are not stored have x = 0 and sum (y -
 *               ybar) = 0); the caller adds (n - n_stored) xbar^2 to the second.
 *   log_hist (log_ny, log_nx), lin_hist (lin_ny, lin_nx) int64, each may be NULL:
 *               np.histogram2d(y, x, bins=(edges_y, edges_x)) over the whole symmetric
 *               matrix (an off-diagonal entry counts twice): edges[k] <= v < edges[k+1],
 *               the last bin closed, the rest dropped; rows = output, columns = input.
 *               Only stored entries are binned: a lowest edge <= 0 is IGM_E_UNSUPPORTED.
 * Integer sums use integer atomics (exact in any order).  Every float64 sum has a fixed
 * order: a row is walked by 64 lanes (entry k of the row by lane k mod 64), the lanes are
 * added by a shuffle tree (offsets 32, 16, .. 1); the per-row sums go to a scratch buffer
 * and a second step adds them per population: thread t of 256 the rows t, t + 256, .. in
 * ascending order, then the 256 partial sums by the same tree per wave and the waves in order.
 * Compiled with -ffp-contract=off.  IGM_E_INVALID: indptr not non-decreasing from 0, a
 * column outside [row, nhap), hap_chrom outside [0, nchrom), nstruct < 1, edges not
 * strictly increasing; IGM_E_UNSUPPORTED: nhap^2 nstruct^2 >= 2^63.
 *
 * Unpinned (alabtools -- Contactmatrix.toarray, cm[c], getInterMask, get_simulated_hic --
 * is absent): the symmetric-with-diagonal reading of toarray(), the clip to [0, 1], the
 * '<=' of the contact test, float64 in the correlation (scipy takes the inputs' dtype). */
int igm_report_hic(igm_ctx* ctx, uint32_t flags,
                   const int32_t* counts, int32_t nhap, int32_t nstruct,
                   const int64_t* indptr, const int32_t* indices, const float* data,
                   const int32_t* hap_chrom, int32_t nchrom, double intra_sigma, double inter_sigma,
                   const double* log_edges_x, int32_t log_nx, const double* log_edges_y, int32_t log_ny,
                   int64_t* log_hist,
                   const double* lin_edges_x, int32_t lin_nx, const double* lin_edges_y, int32_t lin_ny,
                   int64_t* lin_hist,
                   int64_t* dense_sums, int64_t* sparse_ints, double* sparse_sumx, double* means,
                   double* centred);

/* Per-bead neighbourhood census: for every (bead, structure) who is next to it -- the
 * numbers behind the inter-chromosomal contact fraction (ICP) and the composition of the
 * trans neighbourhood by class label.  The definitions are this project's: the reference
 * has none.  xyz (nbead, nstruct, 3) f32 as everywhere in the report.
 *
 * Per-bead inputs, host pointers in every mode:
 *   chain (nbead) int32: any values; two beads are cis iff their values are equal.
 *   cls   (nbead) int32 in [-1, nclass): -1 means unlabelled; may be NULL when nclass == 0.
 *         0 <= nclass <= 8.
 *   radii (nbead) f32 or NULL, see below.
 *
 * Neighbour test, igm_contact_map's to the bit: d2 = (dx*dx + dy*dy) + dz*dz in float32
 * with no contraction; j is a neighbour of i iff fl32(sqrt(d2)) <= bound_ij, decided on
 * the squared norm.
 *   radii == NULL: bound_ij = cutoff (float32, finite, >= 0), the centre-to-centre form.
 *   radii given:   bound_ij = fl32(fl32(contact_range) * fl32(r_i + r_j)), exactly
 *                  igm_contact_map's bound; cutoff is then ignored.  At most 16 distinct
 *                  radius values (a table of the squared bounds replaces a per-pair float64
 *                  evaluation): more return IGM_E_UNSUPPORTED.
 * A comparison with NaN is false: a bead with a non-finite coordinate has no neighbours
 * and is nobody's neighbour.  d == 0 with cutoff == 0 is a neighbour.
 *
 * Exclusions: bead i itself is never counted; a cis partner j with |i - j| < min_sep on
 * the bead index is ignored (min_sep >= 1; 1 ignores nothing but i); trans partners are
 * never ignored.
 *
 * Outputs, ncol = nclass + 2: column 0 is cis, column 1 + k holds the trans partners of
 * class k, column nclass + 1 the unlabelled trans partners.  Each may be NULL, not all.
 *   census  (nbead, nstruct, ncol) int32: the counts of every (bead, structure); follows
 *           `flags` (IGM_DEVICE_PTRS) like xyz
 *   sums    (nbead, ncol) int64: census summed over the structures (host pointer)
 *   icp_sum (nbead) f64: the sum, over exactly the structures counted in icp_n and in
 *           structure order, of trans / (cis + trans) -- one float64 division of exact
 *           integers, trans all trans columns together (host pointer).  A rerun is bitwise
 *           equal.
 *   icp_n   (nbead) int32: the number of structures with cis + trans > 0 (host pointer)
 *
 * nbead <= 65535 (IGM_E_UNSUPPORTED).  IGM_E_INVALID: a NULL xyz or chain, nbead or
 * nstruct < 1, nclass outside [0, 8], a cls entry outside [-1, nclass), min_sep < 1, a
 * cutoff (radii NULL) or contact range (radii given) that is negative or not finite, all
 * four outputs NULL.  After any refusal the context stays usable and no output is written.
 * Without a census to return, a scratch plane of its size is taken from the context.
 * Timing: igm_last_kernel_ms "report_neighbours". */
int igm_report_neighbours(igm_ctx* ctx, uint32_t flags,
                          const float* xyz, int32_t nbead, int32_t nstruct,
                          const int32_t* chain, const int32_t* cls, int32_t nclass, int32_t min_sep,
                          float cutoff, const float* radii, double contact_range,
                          int32_t* census, int64_t* sums, double* icp_sum, int32_t* icp_n);

/* Nuclear bodies from seed loci: features measured against bodies that the models do not
 * contain as objects (speckles; nucleoli on a run without body maps).  The loci known to
 * sit at the body are the seeds; in every structure the places where seeds gather are its
 * bodies; every bead then gets its distance to the nearest body, how often it lies within
 * reach of one, and the TSA-seq signal the population predicts.  The definitions are this
 * project's: the reference has none.  The models' length unit applies throughout (nm in
 * IGM's files); xyz (nbead, nstruct, 3) f32 as everywhere in the report.  Two calls: the
 * first finds the bodies, the second measures against any set of centres.
 *
 * The published recipe clusters the seeds with Markov clustering.  That has no
 * order-independent answer (its result depends on inflation, pruning and iteration order),
 * so single linkage at a fixed cutoff stands in for it here: the answer below is unique
 * whatever order the work is done in.
 *
 * Seeds and links.  seed_idx (nseed) int32: bead indices, strictly increasing, in [0, nbead);
 * the rank of a seed is its position in that list.  Two seeds p != q of a structure are
 * linked iff igm_report_neighbours' test in its centre-to-centre form holds for
 * link_cutoff: d2 = (dx*dx + dy*dy) + dz*dz in float32 with no contraction, linked iff
 * fl32(sqrt(d2)) <= link_cutoff, decided on the squared norm.  A comparison with NaN is
 * false: a seed with a non-finite coordinate is linked to nobody.  link_cutoff == 0 links
 * coincident seeds.
 *
 * Bodies.  The components of a structure are the connected components of its link graph;
 * the label of a seed is the smallest rank in its component.  A body is a component with
 * at least min_size seeds (min_size >= 1); the bodies of a structure are numbered in
 * ascending label.  The centre of a body is the sum of its members' coordinates, each
 * widened to float64 and added in ascending rank, divided once by the member count
 * (float64).  A body with a non-finite member has a non-finite centre.
 *
 * Outputs of igm_report_seed_bodies, host pointers in every mode (of the inputs only xyz
 * follows `flags`):
 *   label  (nstruct, nseed) int32: every seed's label; may be NULL
 *   nbody  (nstruct) int32: the number of bodies, the true count also on overflow
 *   size   (nstruct, max_bodies) int32: the member counts, 0 past nbody; may be NULL
 *   centre (nstruct, max_bodies, 3) f64: NaN past nbody; may be NULL
 * IGM_E_INVALID: a NULL xyz, seed_idx or nbody; nbead, nstruct or nseed < 1; seeds not
 * strictly increasing or out of range; a link_cutoff that is negative or not finite;
 * min_size < 1; max_bodies < 0, or < 1 while size or centre is given.
 * IGM_E_UNSUPPORTED: nseed > 8192 (the seeds of one structure live in LDS, 16 B each).
 * IGM_E_OVERFLOW: some structure has more than max_bodies bodies; nbody then holds the
 * true counts and nothing else is written.  After any other refusal no output is written;
 * the context stays usable after every refusal.  max_bodies = nseed / min_size cannot
 * overflow.  Timing: igm_last_kernel_ms "report_seed_bodies". */
int igm_report_seed_bodies(igm_ctx* ctx, uint32_t flags,
                           const float* xyz, int32_t nbead, int32_t nstruct,
                           const int32_t* seed_idx, int32_t nseed, float link_cutoff, int32_t min_size,
                           int32_t max_bodies,
                           int32_t* label, int32_t* nbody, int32_t* size, double* centre);

/* The per-bead features against the bodies of every structure.  nbody (nstruct) int32 in
 * [0, max_bodies] and centre (nstruct, max_bodies, 3) f64 are host pointers and may come
 * from anywhere -- igm_report_seed_bodies, an imaging experiment; only the first nbody[s]
 * centres of structure s are read, and they must be finite.
 *
 * For bead p and body k of structure s: t = f64(p) - c_k and
 * d = sqrt((t0*t0 + t1*t1) + t2*t2), correctly rounded float64 with no contraction; where
 * a coordinate of p in s is not finite, d is NaN for every body.  nearest(p, s) is the
 * minimum of d over the bodies of s in body order (the first on ties), NaN when s has no
 * body.  t(p, s) is the sum over the bodies, in body order from 0, of exp(-(decay * d)),
 * the argument one float64 multiply; a structure without bodies has t = 0.
 *
 * Outputs; each may be NULL, not all.  The float64 sums run over the structures in
 * structure order (as level_mean of igm_report_levels), so a rerun is bitwise equal.
 *   nearest    (nbead, nstruct) f64; follows `flags` (IGM_DEVICE_PTRS) like xyz
 *   dist_sum   (nbead) f64: the sum of nearest over the structures that have a body
 *   dist_sqsum (nbead) f64: the sum of fl64(nearest * nearest) over the same structures
 *   assoc      (nbead) int64: the number of structures with nearest <= assoc_cutoff
 *   tsa_sum    (nbead) f64: the sum of t(p, s) over all structures
 * The per-bead outputs are host pointers in every mode.  A bead with a non-finite
 * coordinate in a structure that has a body has NaN in its float sums and is not
 * associated there.
 * IGM_E_INVALID: a NULL xyz, nbody or centre; nbead, nstruct or max_bodies < 1; an nbody
 * entry outside [0, max_bodies]; a non-finite centre among the first nbody[s] of a
 * structure; assoc_cutoff or decay negative or not finite; every output NULL.  After a
 * refusal the context stays usable and no output is written.
 * Timing: igm_last_kernel_ms "report_body_features". */
int igm_report_body_features(igm_ctx* ctx, uint32_t flags,
                             const float* xyz, int32_t nbead, int32_t nstruct,
                             const int32_t* nbody, const double* centre, int32_t max_bodies,
                             double assoc_cutoff, double decay,
                             double* nearest, double* dist_sum, double* dist_sqsum, int64_t* assoc,
                             double* tsa_sum);

/* Pairwise conformation RMSD of chromosome copies: how different the structures of a
 * population are from each other.  One call takes one group -- the ncopy copies of one
 * chromosome, or of any subset of its loci -- over all nstruct structures and compares
 * every two of its M = ncopy * nstruct conformations by their minimal RMSD after optimal
 * rigid superposition (proper rotations only: a mirror image is not a match).  The
 * definitions are this project's: the reference has no such report.  xyz (nbead, nstruct,
 * 3) f32 as everywhere in the report; the models' length unit applies throughout.
 *
 *   bead (ncopy, nlocus) int32: the bead of locus i under copy k, any index table into
 *        [0, nbead) (host pointer).  Conformation a = k * nstruct + s.
 *
 * Definitions, all float64: the centre c_a is the sum of the nlocus beads of a, widened and
 * added in ascending locus order (in at most 16 contiguous runs whose sums are added in
 * order), divided once by nlocus; p_i = f64(x_i) - c_a; g[a] = sum |p_i|^2 in the same
 * order.  For a != b, m = sum_i p_i^a (x) p_i^b in ascending locus order, lambda the largest
 * eigenvalue of Horn's key matrix of m (the tracing A-steps' solver: cyclic Jacobi, which
 * takes collinear and coincident point sets), and
 *     rmsd(a, b) = sqrt(max(0, (g_a + g_b - 2 lambda) / nlocus)),
 * rounded once to float32.  Each unordered pair is computed once and mirrored: rmsd[a][b]
 * and rmsd[b][a] are the same bits, and rmsd[a][a] = 0 exactly.  Error: within
 * 1e-6 rmsd + sqrt(1e-12 (g_a + g_b) / nlocus) of exact arithmetic while nlocus <= 9000 (the
 * float32 rounding plus the float64 cancellation in g_a + g_b - 2 lambda; identical
 * conformations come out at that floor, not at 0).
 *
 * A conformation with a non-finite coordinate among its beads has g = NaN; its whole row
 * and column of rmsd, the diagonal included, are NaN, and it is left out of row_sum, row_n,
 * hist and everyone else's sums.
 *
 * Outputs; each may be NULL, not all.  Every reduction is available without the matrix
 * (M^2 * 4 bytes) and has identical bytes whether or not rmsd is asked for; a rerun is
 * bitwise equal in every output (fixed summation orders, no float atomics).
 *   rmsd    (M, M) f32; follows `flags` (IGM_DEVICE_PTRS) like xyz.  Every other output is
 *           a host pointer in every mode.
 *   g       (M) f64
 *   row_sum (M) f64: the sum over b != a of the finite rmsd(a, b), the float32 values
 *           widened to float64 and added in ascending b (in runs of 64 conformations whose
 *           sums are added in order)
 *   row_n   (M) int32: the number of terms of row_sum
 *   same    (nstruct, ncopy, ncopy) f32: same[s][k][k'] = rmsd((k, s), (k', s)), the copies
 *           of one cell against each other, the matrix entries themselves (diagonal 0, or
 *           NaN for a conformation with a non-finite coordinate)
 *   hist    (nedge - 1) int64: counts of the finite rmsd(a, b) over a < b with
 *           np.histogram's semantics on the float32 value: bins [e_i, e_i+1), the last one
 *           closed; values outside the edges are not counted.  edges (nedge) f32, finite
 *           and strictly increasing, nedge >= 2 (host pointer; NULL / 0 without hist, and
 *           not read then).
 *
 * IGM_E_INVALID: a NULL xyz or bead; nbead, nstruct, ncopy or nlocus < 1; a bead index
 * outside [0, nbead); hist with NULL edges, nedge < 2 or edges that are not finite and
 * strictly increasing; every output NULL.  IGM_E_UNSUPPORTED: M > 2^20 (the tile grid and
 * every index derived from M stay far inside their types), more than 4096 histogram bins
 * (a workgroup counts them in LDS).  The context takes scratch of 24 * nlocus * M' bytes
 * (the centred coordinates, M' = M rounded up to 64) and 12 * M' * M' / 64 (partial row
 * sums); IGM_E_NOMEM when it cannot.  After any refusal no output is written and the
 * context stays usable.  Timing: igm_last_kernel_ms "report_conformations". */
int igm_report_conformations(igm_ctx* ctx, uint32_t flags,
                             const float* xyz, int32_t nbead, int32_t nstruct,
                             const int32_t* bead, int32_t ncopy, int32_t nlocus,
                             const float* edges, int32_t nedge,
                             float* rmsd, double* g, double* row_sum, int32_t* row_n,
                             float* same, int64_t* hist);

#ifdef __cplusplus
}
#endif
#endif /* IGM_HIP_H */
