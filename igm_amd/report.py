"""Population report: the structural numbers of igm/report/*.py (driven by
bin/igm-report) computed on the GPU from the bead-major population.

  radial_levels        -- get_radial_level (report/radials.py:15-39): the mean radial level
                          of every bead (igm_report_levels); average_copies folds the copies
  radial_density       -- plot_radial_density (:69-87): np.histogram of all levels
  shells               -- report_shells (report/shells.py:9-43): per structure the levels
                          partitioned in nshell rank shells, their means and histograms
  chromosome_rgs       -- get_chroms_rgs (report/radius_of_gyration.py:22-41), igm_report_rg
  lamina_frequency     -- report_damid's contact frequency (report/damid.py:32-51),
                          igm_report_lamina
  average_distance_map -- create_average_distance_map (report/distance_map.py:5-22),
                          igm_report_distance_map
  hic_statistics / hic_correlations / hic_comparison
                       -- report_hic (report/hic.py:16-180): the Pearson correlations between
                          the input Hi-C matrix and the simulated contact map, per chromosome
                          and inter-chromosomal, over all / imposed / non-imposed entries, and
                          the two 2-D histograms of plots.py, igm_report_hic
  map_levels / map_density / map_shells / map_lamina_frequency
                       -- the same numbers inside an imaged nucleus (nucleus_shape exp_map), on
                          the level below the lamina of every structure's map (this project's
                          definitions, include/igm_hip.h: igm_report_map_levels / _map_lamina)
  neighbour_census / inter_chromosomal_fraction / trans_class_fraction / local_compaction
                       -- this project's per-locus features (the reference has none): who is
                          next to every bead in every structure (igm_report_neighbours), the
                          inter-chromosomal contact fraction, the class composition of the
                          trans neighbourhood, and the Rg of a window of the fibre
  seed_bodies / body_features / body_profiles
                       -- nuclear bodies that the models do not contain as objects, from seed
                          loci (this project's definitions too): the places where the seeds
                          gather in every structure (igm_report_seed_bodies), every bead's
                          distance to the nearest one, its association frequency and the
                          TSA-seq signal the population predicts (igm_report_body_features)
  conformation_beads / conformation_rmsd / conformation_summary
                       -- how different the structures are from each other (this project's
                          definitions as well): the minimal RMSD after optimal superposition
                          between every two copies of a chromosome across the population
                          (igm_report_conformations), its mean, the medoid conformation and
                          the homologues of one cell against those of different cells
  report_population    -- the numeric files bin/igm-report leaves in its output directory
                          (names and formats of the reference); plots, images and the HTML
                          page stay with the reference

    python -m igm_amd.report HSS [-c CONFIG] [-l LABEL] [--semiaxes A B C] [--steps ...] [-o DIR]
                             [--hic HCS] [--hic-sigma S] [--hic-inter-sigma S] [--hic-intra-sigma S]
                             [--hic-contact-range R] [--neighbour-cutoff D] [--min-sep N]
                             [--compaction-halfwidth W] [--classes FILE]
                             [--seeds FILE] [--link-cutoff D] [--min-body-size N] [--assoc-cutoff D]
                             [--tsa-decay K]
                             [--conformation-chroms ID[,ID...]] [--conformation-loci FILE] [--save-rmsd]
                             [--rmsd-max D] [--rmsd-bins N]

Every function takes the population as host arrays -- xyz (nbead, nstruct, 3) float32, the
.hss layout -- or as a steps.PopulationStore, which then also supplies the index arrays
left at None.  The arithmetic choices (float64 levels and Rg, the NumPy 2 evaluation of
snormsq_ellipse, the defined diagonal and lower triangle of the distance map) are the
ones include/igm_hip.h states per entry point.
"""
import json
import os

import numpy as np

from . import _lib

STEPS = ('rgs', 'shells', 'radials', 'damid', 'distance_map')
OPTIONAL_STEPS = ('hic',)                    # accepted in `steps`, not run by default
BODY_STEPS = ('bodies',)                     # optional too: the nuclear bodies of an imaged nucleus
FEATURE_STEPS = ('neighbours', 'compaction')  # optional: the per-locus features mined from a finished run
SEED_STEPS = ('seeded_bodies',)               # optional: nuclear bodies from seed loci (needs --seeds)
CONFORMATION_STEPS = ('conformations',)       # optional: pairwise RMSD of the copies of every chromosome
DEFAULT_RMSD_MAX = 10000.0                   # the RMSD histogram: 200 bins up to this, the models' length unit
DEFAULT_RMSD_BINS = 200                      # (this project's choice)
MAX_RMSD_BINS = 4096                         # igm_report_conformations counts the bins in LDS
DEFAULT_NEIGHBOUR_CUTOFF = 500.0             # centre-to-centre neighbourhood radius, the models' length unit
DEFAULT_LINK_CUTOFF = 500.0                  # seeds this close are linked into one body (this project's choice)
DEFAULT_MIN_BODY_SIZE = 3                    # seeds a component needs to count as a body
DEFAULT_ASSOC_CUTOFF = 500.0                 # a bead this close to a body's centre is associated with it
DEFAULT_TSA_DECAY = 0.004                    # per length unit: the TSA-seq signal falls off as exp(-decay * d)
MAX_CLASSES = 8                              # class labels of the neighbour census (igm_report_neighbours)
DEFAULT_SEMIAXES = (5000.0, 5000.0, 5000.0)  # report_radials / report_shells / report_damid
DEFAULT_DAMID_CONTACT_RANGE = 0.05           # restraints/DamID/contact_range of the reference's config defaults


def _population(pop):
    """(xyz, store or None) of a PopulationStore or a host array"""
    if hasattr(pop, 'coordinates') and callable(pop.coordinates):
        return np.ascontiguousarray(pop.coordinates(), np.float32), pop
    xyz = np.ascontiguousarray(pop, np.float32)
    if xyz.ndim != 3 or xyz.shape[2] != 3 or xyz.shape[0] < 1 or xyz.shape[1] < 1:
        raise ValueError('xyz must be (nbead, nstruct, 3) with nbead, nstruct >= 1')
    return xyz, None


def _pick(value, store, name):
    if value is None:
        if store is None:
            raise ValueError('%s is required with host arrays' % name)
        value = getattr(store, name)
    return value


def _semiaxes(semiaxes):
    s = np.ascontiguousarray(semiaxes, np.float64).ravel()
    if s.size == 1:
        s = np.repeat(s, 3)
    if s.shape != (3,) or not np.all(np.isfinite(s)) or not np.all(s > 0):
        raise ValueError('semiaxes must be three positive finite numbers')
    return np.ascontiguousarray(s)


def _csr(ptr, idx, nbead, what):
    ptr = np.ascontiguousarray(ptr, np.int32)
    idx = np.ascontiguousarray(idx, np.int32)
    if ptr.ndim != 1 or len(ptr) < 2 or ptr[0] != 0 or np.any(np.diff(ptr) < 0) or ptr[-1] != len(idx):
        raise ValueError('%s_ptr must be non-decreasing from 0 to len(%s_idx)' % (what, what))
    if len(idx) and (idx.min() < 0 or idx.max() >= nbead):
        raise ValueError('%s_idx holds bead indices outside [0, %d)' % (what, nbead))
    return ptr, idx


def _levels(xyz, semiaxes, ctx, device, want_mean=False, density_edges=None, nshell=0, shell_edges=None):
    nbead, S = xyz.shape[0], xyz.shape[1]
    sx = _semiaxes(semiaxes)
    c = ctx or _lib.context(device)
    mean = np.empty(nbead, np.float64) if want_mean else None
    dens = de = None
    if density_edges is not None:
        de = np.ascontiguousarray(density_edges, np.float64)
        dens = np.empty(len(de) - 1, np.int64)
    smean = shist = se = None
    if nshell:
        se = np.ascontiguousarray(shell_edges, np.float64)
        smean = np.empty((S, nshell), np.float64)
        shist = np.empty((nshell, len(se) - 1), np.int64)
    rc = c.lib.igm_report_levels(c.h, 0, xyz.ctypes.data, nbead, S, sx.ctypes.data, _lib.ptr(mean), _lib.ptr(de),
                                 0 if de is None else len(de) - 1, _lib.ptr(dens), int(nshell), _lib.ptr(smean),
                                 _lib.ptr(se), 0 if se is None else len(se) - 1, _lib.ptr(shist))
    c.check(rc, 'igm_report_levels')
    return mean, dens, smean, shist


def average_copies(v, copy_ptr, copy_idx):
    """aggregate_copies(v, index) with np.nanmean (report/utils.py:5-27): (nhap,) float64"""
    v = np.array(v)
    nhap = len(copy_ptr) - 1
    x = np.zeros(nhap)
    for i in range(nhap):
        x[i] = np.nanmean(v[copy_idx[copy_ptr[i]:copy_ptr[i + 1]]])
    return x


def radial_levels(pop, semiaxes, copy_ptr=None, copy_idx=None, ctx=None, device=0):
    """The mean radial level of every bead, (nbead,) float64; with a copy index (or a
    PopulationStore) the copies are averaged like get_radial_level does: (nhap,)."""
    xyz, store = _population(pop)
    mean = _levels(xyz, semiaxes, ctx, device, want_mean=True)[0]
    if store is not None and copy_ptr is None:
        copy_ptr, copy_idx = store.copy_ptr, store.copy_idx
    if copy_ptr is None:
        return mean
    copy_ptr, copy_idx = _csr(copy_ptr, copy_idx, xyz.shape[0], 'copy')
    return average_copies(mean, copy_ptr, copy_idx)


def radial_density(pop, semiaxes, n=11, vmax=1.1, ctx=None, device=0):
    """(counts (n,) int64, edges (n + 1,)) of np.histogram(levels, bins=n, range=(0, vmax))
    over all nbead * nstruct levels (plot_radial_density)."""
    xyz, _ = _population(pop)
    if n < 1 or not vmax > 0:
        raise ValueError('radial_density needs n >= 1 bins and vmax > 0')
    edges = np.linspace(0, vmax, n + 1)
    return _levels(xyz, semiaxes, ctx, device, density_edges=edges)[1], edges


def shells(pop, semiaxes, nshell=5, hvmax=1.5, hnbins=150, ctx=None, device=0):
    """(shell_mean (nstruct, nshell), shell_hist (nshell, hnbins) int64, edges) of
    report_shells: ave_shell_rad, pos_histos and the histogram edges."""
    xyz, _ = _population(pop)
    if nshell < 1 or hnbins < 1 or not hvmax > 0:
        raise ValueError('shells needs nshell >= 1, hnbins >= 1 and hvmax > 0')
    edges = np.linspace(0, hvmax, hnbins + 1)
    _, _, smean, shist = _levels(xyz, semiaxes, ctx, device, nshell=nshell, shell_edges=edges)
    return smean, shist, edges


def chains(chrom, copy):
    """The chains of get_chroms_rgs as (chromosome ids, CSR over chromosomes of chain numbers,
    chain_ptr, chain_idx): per chromosome (index.get_chromosomes), per copy
    (index.get_chrom_copies), the beads of index.get_chrom_pos(chrom, copy)."""
    chrom = np.asarray(chrom)
    copy = np.asarray(copy)
    ids = np.unique(chrom)
    chrom_ptr, ptr, idx = [0], [0], []
    for cid in ids:
        sel = chrom == cid
        for k in np.unique(copy[sel]):
            ii = np.flatnonzero(sel & (copy == k))
            idx.append(ii)
            ptr.append(ptr[-1] + len(ii))
        chrom_ptr.append(len(ptr) - 1)
    return ids, np.array(chrom_ptr), np.array(ptr, np.int32), np.concatenate(idx).astype(np.int32)


def chain_rgs(pop, chain_ptr, chain_idx, ctx=None, device=0):
    """Rg of every chain in every structure (igm_report_rg): (nchain, nstruct) float64"""
    xyz, _ = _population(pop)
    chain_ptr, chain_idx = _csr(chain_ptr, chain_idx, xyz.shape[0], 'chain')
    c = ctx or _lib.context(device)
    nchain = len(chain_ptr) - 1
    out = np.empty((nchain, xyz.shape[1]), np.float64)
    rc = c.lib.igm_report_rg(c.h, 0, xyz.ctypes.data, xyz.shape[0], xyz.shape[1], chain_ptr.ctypes.data,
                             chain_idx.ctypes.data, nchain, out.ctypes.data)
    c.check(rc, 'igm_report_rg')
    return out


def chromosome_rgs(pop, chrom=None, copy=None, ctx=None, device=0):
    """get_chroms_rgs: (chromosome ids, list with one float64 array per chromosome holding
    the Rg of its copies, copy after copy, nstruct values each)."""
    xyz, store = _population(pop)
    chrom, copy = _pick(chrom, store, 'chrom'), _pick(copy, store, 'copy')
    if len(chrom) != xyz.shape[0] or len(copy) != xyz.shape[0]:
        raise ValueError('chrom and copy must have one entry per bead')
    ids, chrom_ptr, chain_ptr, chain_idx = chains(chrom, copy)
    rgs = chain_rgs(xyz, chain_ptr, chain_idx, ctx=ctx, device=device)
    return ids, [rgs[chrom_ptr[k]:chrom_ptr[k + 1]].ravel() for k in range(len(ids))]


def lamina_denominators(semiaxes, contact_range, radii, copy_ptr, copy_idx):
    """(nhap, 3) float64: snormsq_ellipse's denominators with the reference's own NumPy
    expression, (semiaxes * (1 - contact_range) - r)**2 with r the (float32) radius of the
    locus's first copy (report/damid.py:39-47, report/utils.py:86-89)."""
    nuc_rad = np.array(semiaxes) * (1 - contact_range)
    r = np.asarray(radii, np.float32)[copy_idx[copy_ptr[:-1]]]
    return np.ascontiguousarray((nuc_rad[None, :] - r[:, None]) ** 2, np.float64)


def lamina_counts(pop, radii=None, copy_ptr=None, copy_idx=None, semiaxes=None, contact_range=0.05, ctx=None,
                  device=0):
    """(counts (nhap,) int64, copies (nhap,)) of report_damid: the (copy, structure) pairs
    at the lamina, snormsq_ellipse >= 1 on the envelope shrunk by contact_range."""
    xyz, store = _population(pop)
    radii = _pick(radii, store, 'radii')
    copy_ptr, copy_idx = _csr(_pick(copy_ptr, store, 'copy_ptr'), _pick(copy_idx, store, 'copy_idx'), xyz.shape[0],
                              'copy')
    if semiaxes is None:
        raise ValueError('lamina_frequency needs the semiaxes of the envelope')
    if len(radii) != xyz.shape[0]:
        raise ValueError('radii must have one entry per bead')
    if np.any(np.diff(copy_ptr) < 1):
        raise ValueError('every haploid locus needs at least one copy')
    den = lamina_denominators(_semiaxes(semiaxes), contact_range, radii, copy_ptr, copy_idx)
    c = ctx or _lib.context(device)
    nhap = len(copy_ptr) - 1
    out = np.empty(nhap, np.int64)
    rc = c.lib.igm_report_lamina(c.h, 0, xyz.ctypes.data, xyz.shape[0], xyz.shape[1], copy_ptr.ctypes.data,
                                 copy_idx.ctypes.data, nhap, den.ctypes.data, out.ctypes.data)
    c.check(rc, 'igm_report_lamina')
    return out, np.diff(copy_ptr)


def lamina_frequency(pop, radii=None, copy_ptr=None, copy_idx=None, semiaxes=None, contact_range=0.05, ctx=None,
                     device=0):
    """out_damid_prob of report_damid: float(count) / nstruct / n_copies, (nhap,) float64"""
    xyz, store = _population(pop)
    counts, ncopy = lamina_counts(xyz if store is None else store, radii, copy_ptr, copy_idx, semiaxes, contact_range,
                                  ctx=ctx, device=device)
    return counts.astype(np.float64) / xyz.shape[1] / ncopy


# ------------------------------------------------------------------ imaged nuclei (exp_map)
def _inside_depths(vol):
    """|(v - e) * grid| in float64 of every voxel with w != 0, summed (t0^2 + t2^2) + t1^2"""
    mat = np.asarray(vol['matrice'])
    inside = mat[..., 3] != 0
    v = np.stack(np.nonzero(inside), axis=1).astype(np.int64)
    t = (v - mat[inside][:, :3].astype(np.int64)).astype(np.float64) * np.asarray(vol['grid'], np.float32).astype(
        np.float64)
    t = t * t
    return np.sqrt((t[:, 0] + t[:, 2]) + t[:, 1])


def map_depth_scale(vol):
    """The depth scale of a map: the largest voxel-centre depth |(v - e) * grid| over the
    voxels with w != 0, float64.  ValueError for a map without an inside voxel or whose
    inside voxels are all lamina voxels (scale 0)."""
    d = _inside_depths(vol)
    if d.size == 0:
        raise ValueError('the map has no inside voxel')
    dmax = float(d.max())
    if not (np.isfinite(dmax) and dmax > 0):
        raise ValueError('the map has no voxel below its lamina (depth scale %r)' % dmax)
    return dmax


def map_shell_volumes(vol, edges, depth_scale=None):
    """V[k]: the voxel volume times the number of inside voxels whose centre level
    1 - |(v - e) grid| / depth_scale falls in bin k of np.histogram on `edges`"""
    dmax = map_depth_scale(vol) if depth_scale is None else float(depth_scale)
    lev = 1 - _inside_depths(vol) / dmax
    g = np.asarray(vol['grid'], np.float32).astype(np.float64)
    return np.histogram(lev, bins=np.asarray(edges, np.float64))[0] * (g[0] * g[1] * g[2])


def _stage_maps(c, volumes, struct_map, nstruct):
    """the maps and the per-structure index staged on the context (volume.stage), as the
    DamID A-step's exp_map wrapper does: (nmap, depth scales)"""
    from . import volume as V
    if volumes is None or len(volumes) == 0:
        raise ValueError('the map forms need the volume maps')
    if struct_map is not None:
        struct_map = np.ascontiguousarray(struct_map, np.int32)
        if struct_map.shape != (nstruct,) or struct_map.min() < 0 or struct_map.max() >= len(volumes):
            raise ValueError('struct_map must name one of the %d maps for each of the %d structures'
                             % (len(volumes), nstruct))
    scale = np.array([map_depth_scale(v) for v in volumes], np.float64)
    V.stage(c, volumes, struct_map)
    return scale


def _map_levels(xyz, volumes, struct_map, ctx, device, want_mean=False, want_depth=False, density_edges=None, nshell=0,
                shell_edges=None):
    """igm_report_map_levels on freshly staged maps: (level_mean, depth_mean, density,
    shell_mean, shell_hist), None where not asked for"""
    nbead, S = xyz.shape[0], xyz.shape[1]
    c = ctx or _lib.context(device)
    scale = _stage_maps(c, volumes, struct_map, S)
    mean = np.empty(nbead, np.float64) if want_mean else None
    depth = np.empty(nbead, np.float64) if want_depth else None
    dens = de = None
    if density_edges is not None:
        de = np.ascontiguousarray(density_edges, np.float64)
        dens = np.empty(len(de) - 1, np.int64)
    smean = shist = se = None
    if nshell:
        se = np.ascontiguousarray(shell_edges, np.float64)
        smean = np.empty((S, nshell), np.float64)
        shist = np.empty((nshell, len(se) - 1), np.int64)
    rc = c.lib.igm_report_map_levels(c.h, 0, xyz.ctypes.data, nbead, S, None, scale.ctypes.data, _lib.ptr(mean),
                                     _lib.ptr(depth), _lib.ptr(de), 0 if de is None else len(de) - 1, _lib.ptr(dens),
                                     int(nshell), _lib.ptr(smean), _lib.ptr(se), 0 if se is None else len(se) - 1,
                                     _lib.ptr(shist))
    c.check(rc, 'igm_report_map_levels')
    return mean, depth, dens, smean, shist


def map_levels(pop, volumes, struct_map=None, copy_ptr=None, copy_idx=None, ctx=None, device=0):
    """(level means, mean signed depths) of every bead on the maps of an imaged nucleus:
    volumes are volume.read_volume dicts and struct_map[s] the map of structure s (None:
    map 0).  The level is max(0, 1 - depth / map_depth_scale): 1 on the lamina, 0 on the
    deepest voxel centre.  With a copy index (or a PopulationStore) the copies are averaged
    like radial_levels does: (nhap,) each."""
    xyz, store = _population(pop)
    mean, depth = _map_levels(xyz, volumes, struct_map, ctx, device, want_mean=True, want_depth=True)[:2]
    if store is not None and copy_ptr is None:
        copy_ptr, copy_idx = store.copy_ptr, store.copy_idx
    if copy_ptr is None:
        return mean, depth
    copy_ptr, copy_idx = _csr(copy_ptr, copy_idx, xyz.shape[0], 'copy')
    return average_copies(mean, copy_ptr, copy_idx), average_copies(depth, copy_ptr, copy_idx)


def map_density(pop, volumes, struct_map=None, n=11, vmax=1.1, ctx=None, device=0):
    """(counts (n,) int64, edges, volumes (n,)) of the map levels: np.histogram over all
    nbead * nstruct levels, and the real shell volume behind every bin summed over the
    structures, sum_s V_map(s)[k] (map_shell_volumes)"""
    xyz, _ = _population(pop)
    if n < 1 or not vmax > 0:
        raise ValueError('map_density needs n >= 1 bins and vmax > 0')
    edges = np.linspace(0, vmax, n + 1)
    counts = _map_levels(xyz, volumes, struct_map, ctx, device, density_edges=edges)[2]
    S = xyz.shape[1]
    smap = np.zeros(S, np.int64) if struct_map is None else np.asarray(struct_map, np.int64)
    per_map = np.bincount(smap, minlength=len(volumes)).astype(np.float64)
    vols = np.zeros(n)
    for m, v in enumerate(volumes):
        if per_map[m]:
            vols += per_map[m] * map_shell_volumes(v, edges)
    return counts, edges, vols


def map_shells(pop, volumes, struct_map=None, nshell=5, hvmax=1.5, hnbins=150, ctx=None, device=0):
    """shells() on the map levels: (shell_mean (nstruct, nshell), shell_hist, edges)"""
    xyz, _ = _population(pop)
    if nshell < 1 or hnbins < 1 or not hvmax > 0:
        raise ValueError('map_shells needs nshell >= 1, hnbins >= 1 and hvmax > 0')
    edges = np.linspace(0, hvmax, hnbins + 1)
    _, _, _, smean, shist = _map_levels(xyz, volumes, struct_map, ctx, device, nshell=nshell, shell_edges=edges)
    return smean, shist, edges


def map_lamina_counts(pop, volumes, struct_map=None, radii=None, copy_ptr=None, copy_idx=None, contact_range=0.05,
                      side=1, ctx=None, device=0):
    """(counts (nhap,) int64, copies (nhap,)): the (copy, structure) pairs in contact with
    the lamina of their structure's map, depth - r <= contact_range * map_depth_scale with r
    the radius of the locus's first copy; side = -1 for a body map (a nucleolus, whose w
    marks the inside of the body): -depth - r <= contact_range * map_depth_scale."""
    xyz, store = _population(pop)
    radii = np.ascontiguousarray(_pick(radii, store, 'radii'), np.float32)
    copy_ptr, copy_idx = _csr(_pick(copy_ptr, store, 'copy_ptr'), _pick(copy_idx, store, 'copy_idx'), xyz.shape[0],
                              'copy')
    if len(radii) != xyz.shape[0]:
        raise ValueError('radii must have one entry per bead')
    if np.any(np.diff(copy_ptr) < 1):
        raise ValueError('every haploid locus needs at least one copy')
    if side not in (1, -1):
        raise ValueError('side is +1 (a nucleus map) or -1 (a body map)')
    c = ctx or _lib.context(device)
    thr = np.ascontiguousarray(float(contact_range) * _stage_maps(c, volumes, struct_map, xyz.shape[1]))
    nhap = len(copy_ptr) - 1
    out = np.empty(nhap, np.int64)
    rc = c.lib.igm_report_map_lamina(c.h, 0, xyz.ctypes.data, xyz.shape[0], xyz.shape[1], copy_ptr.ctypes.data,
                                     copy_idx.ctypes.data, nhap, radii.ctypes.data, None, thr.ctypes.data, int(side),
                                     out.ctypes.data)
    c.check(rc, 'igm_report_map_lamina')
    return out, np.diff(copy_ptr)


def map_lamina_frequency(pop, volumes, struct_map=None, radii=None, copy_ptr=None, copy_idx=None, contact_range=0.05,
                         side=1, ctx=None, device=0):
    """lamina_frequency on the maps: float(count) / nstruct / n_copies, (nhap,) float64"""
    xyz, store = _population(pop)
    counts, ncopy = map_lamina_counts(xyz if store is None else store, volumes, struct_map, radii, copy_ptr, copy_idx,
                                      contact_range, side, ctx=ctx, device=device)
    return counts.astype(np.float64) / xyz.shape[1] / ncopy


def average_distance_map(pop, copy_ptr=None, copy_idx=None, hap_chrom=None, ctx=None, device=0):
    """create_average_distance_map: (nhap, nhap) float64.  hap_chrom[a] is the chromosome of
    haploid locus a -- the reference reads index.chrom[a] of the diploid index, the same
    thing whenever beads 0..nhap-1 are the first copies in locus order (the layout alabtools
    writes).  The diagonal is 0 and the lower triangle mirrors the upper (the reference
    leaves both uninitialised)."""
    xyz, store = _population(pop)
    copy_ptr, copy_idx = _csr(_pick(copy_ptr, store, 'copy_ptr'), _pick(copy_idx, store, 'copy_idx'), xyz.shape[0],
                              'copy')
    hap_chrom = np.ascontiguousarray(_pick(hap_chrom, store, 'hap_chrom'), np.int32)
    nhap = len(copy_ptr) - 1
    if hap_chrom.shape != (nhap,):
        raise ValueError('hap_chrom must have one entry per haploid locus')
    c = ctx or _lib.context(device)
    out = np.empty((nhap, nhap), np.float64)
    rc = c.lib.igm_report_distance_map(c.h, 0, xyz.ctypes.data, xyz.shape[0], xyz.shape[1], copy_ptr.ctypes.data,
                                       copy_idx.ctypes.data, hap_chrom.ctypes.data, nhap,
                                       out.ctypes.data)
    c.check(rc, 'igm_report_distance_map')
    return out


# ------------------------------------------------------------------ neighbourhood features
def chain_numbers(chrom, copy):
    """(nbead,) int32: the number of every bead's (chromosome, copy) chain in chains(chrom,
    copy) -- two beads are cis iff they share it, so the homologous copy is trans"""
    _, _, chain_ptr, chain_idx = chains(chrom, copy)
    out = np.empty(len(chain_idx), np.int32)
    out[chain_idx] = np.repeat(np.arange(len(chain_ptr) - 1, dtype=np.int32), np.diff(chain_ptr))
    return out


def neighbour_census(pop, cutoff=DEFAULT_NEIGHBOUR_CUTOFF, chain=None, classes=None, nclass=None, min_sep=1,
                     radii=None, contact_range=None, want_census=True, ctx=None, device=0):
    """igm_report_neighbours: who is next to every bead in every structure.

    j is a neighbour of i when their float32 distance is <= cutoff (centre to centre, in the
    models' length unit) or, with radii (at most 16 distinct values) and contact_range, <=
    contact_range * (r_i + r_j), the contact map's test.  chain (nbead,): equal values are
    cis; a PopulationStore supplies chain_numbers(store.chrom, store.copy).  classes
    (nbead,) labels in [-1, nclass), -1 unlabelled; nclass defaults to max(classes) + 1.
    Bead i itself and its cis partners with |i - j| < min_sep are ignored.

    Returns {'census': (nbead, nstruct, nclass + 2) int32 or None (want_census=False),
    'sums': (nbead, nclass + 2) int64, 'icp_sum': (nbead,) float64, 'icp_n': (nbead,) int32}.
    Column 0 is cis, 1 + k the trans partners of class k, the last one the unlabelled trans
    partners; icp_sum is the sum of trans / (cis + trans) over the icp_n structures in which
    the bead has a neighbour at all."""
    xyz, store = _population(pop)
    nbead, S = xyz.shape[0], xyz.shape[1]
    if chain is None:
        if store is None:
            raise ValueError('chain is required with host arrays')
        chain = chain_numbers(store.chrom, store.copy)
    chain = np.ascontiguousarray(chain, np.int32)
    if chain.shape != (nbead,):
        raise ValueError('chain must have one entry per bead')
    if classes is not None:
        classes = np.ascontiguousarray(classes, np.int32)
        if classes.shape != (nbead,):
            raise ValueError('classes must have one entry per bead')
        if nclass is None:
            nclass = max(int(classes.max()) + 1, 0)
    nclass = int(nclass or 0)
    if classes is None and nclass:
        classes = np.full(nbead, -1, np.int32)
    if radii is not None:
        radii = np.ascontiguousarray(radii, np.float32)
        if radii.shape != (nbead,):
            raise ValueError('radii must have one entry per bead')
        if contact_range is None:
            raise ValueError('the radii form needs a contact_range')
    ncol = nclass + 2
    c = ctx or _lib.context(device)
    census = np.empty((nbead, S, ncol), np.int32) if want_census else None
    sums = np.empty((nbead, ncol), np.int64)
    icp_sum = np.empty(nbead, np.float64)
    icp_n = np.empty(nbead, np.int32)
    rc = c.lib.igm_report_neighbours(c.h, 0, xyz.ctypes.data, nbead, S, chain.ctypes.data, _lib.ptr(classes), nclass,
                                     int(min_sep), float(cutoff), _lib.ptr(radii),
                                     0.0 if contact_range is None else float(contact_range), _lib.ptr(census),
                                     sums.ctypes.data, icp_sum.ctypes.data, icp_n.ctypes.data)
    c.check(rc, 'igm_report_neighbours')
    return {'census': census, 'sums': sums, 'icp_sum': icp_sum, 'icp_n': icp_n}


def _fold_copies(v, copy_ptr, copy_idx):
    """average_copies; a locus whose copies are all NaN stays NaN without NumPy's warning"""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        return average_copies(v, copy_ptr, copy_idx)


def icp_of(icp_sum, icp_n):
    """icp_sum / icp_n per bead, NaN for a bead that never has a neighbour"""
    icp_n = np.asarray(icp_n)
    out = np.full(len(icp_n), np.nan)
    ok = icp_n > 0
    out[ok] = np.asarray(icp_sum, np.float64)[ok] / icp_n[ok]
    return out


def inter_chromosomal_fraction(pop, cutoff=DEFAULT_NEIGHBOUR_CUTOFF, chain=None, min_sep=1, radii=None,
                               contact_range=None, copy_ptr=None, copy_idx=None, ctx=None, device=0):
    """The inter-chromosomal contact fraction (ICP) of every haploid locus, (nhap,) float64:
    per bead the mean over the structures in which it has a neighbour of trans / (cis +
    trans) (neighbour_census), folded over the copies with average_copies.  A bead without
    any neighbour is NaN, and so is a locus whose copies all are."""
    xyz, store = _population(pop)
    copy_ptr, copy_idx = _csr(_pick(copy_ptr, store, 'copy_ptr'), _pick(copy_idx, store, 'copy_idx'), xyz.shape[0],
                              'copy')
    res = neighbour_census(xyz if store is None else store, cutoff, chain, None, 0, min_sep, radii, contact_range,
                           want_census=False, ctx=ctx, device=device)
    return _fold_copies(icp_of(res['icp_sum'], res['icp_n']), copy_ptr, copy_idx)


def trans_class_fraction(census, copy_ptr, copy_idx):
    """(nhap, nclass) float64 from a census (nbead, nstruct, nclass + 2): for class k the
    median over the (copy, structure) pairs of a locus of n_k / (the labelled trans
    partners), skipping the pairs without a labelled trans partner; a locus without such a
    pair is NaN.  Runs on the host."""
    census = np.asarray(census)
    nclass = census.shape[2] - 2
    nhap = len(copy_ptr) - 1
    out = np.full((nhap, nclass), np.nan)
    for h in range(nhap if nclass else 0):
        lab = census[copy_idx[copy_ptr[h]:copy_ptr[h + 1]], :, 1:1 + nclass].reshape(-1, nclass).astype(np.float64)
        tot = lab.sum(axis=1)
        ok = tot > 0
        if nclass and ok.any():
            out[h] = np.median(lab[ok] / tot[ok, None], axis=0)
    return out


def compaction_windows(chrom, copy, halfwidth=2):
    """CSR (ptr (nbead + 1), idx) with one row per bead, in bead order: the beads within
    halfwidth index positions of it on its own chain (chains(chrom, copy)), clipped at the
    chain's ends."""
    halfwidth = int(halfwidth)
    if halfwidth < 0:
        raise ValueError('halfwidth must be >= 0')
    _, _, chain_ptr, chain_idx = chains(chrom, copy)
    rows = [None] * len(chain_idx)
    for c in range(len(chain_ptr) - 1):
        beads = chain_idx[chain_ptr[c]:chain_ptr[c + 1]]
        for p, b in enumerate(beads):
            rows[b] = beads[max(0, p - halfwidth):p + halfwidth + 1]
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return ptr, np.concatenate(rows).astype(np.int32)


def local_compaction(pop, chrom=None, copy=None, halfwidth=2, ctx=None, device=0):
    """The local compaction of the fibre, (nbead, nstruct) float64: the radius of gyration
    (igm_report_rg) of the window of compaction_windows around every bead."""
    xyz, store = _population(pop)
    chrom, copy = _pick(chrom, store, 'chrom'), _pick(copy, store, 'copy')
    if len(chrom) != xyz.shape[0] or len(copy) != xyz.shape[0]:
        raise ValueError('chrom and copy must have one entry per bead')
    ptr, idx = compaction_windows(chrom, copy, halfwidth)
    return chain_rgs(xyz, ptr, idx, ctx=ctx, device=device)


def haploid_classes(labels, copy_ptr, copy_idx):
    """(per-bead labels int32, nclass) from one label per haploid locus (an array or the
    path of a text file; -1 unlabelled), expanded through the copy index.  ValueError for a
    wrong length or a label outside [-1, 8)."""
    if isinstance(labels, (str, os.PathLike)):
        labels = np.loadtxt(os.fspath(labels), dtype=np.int64, ndmin=1)
    labels = np.asarray(labels)
    nhap = len(copy_ptr) - 1
    if labels.shape != (nhap,):
        raise ValueError('the class labels must hold one entry per haploid locus (%d), got shape %s'
                         % (nhap, labels.shape))
    if len(labels) and (labels.min() < -1 or labels.max() >= MAX_CLASSES):
        raise ValueError('class labels must lie in [-1, %d)' % MAX_CLASSES)
    out = np.full(int(copy_ptr[-1]), -1, np.int32)
    out[copy_idx] = np.repeat(labels.astype(np.int32), np.diff(copy_ptr))
    return out, int(max(labels.max() + 1, 0)) if len(labels) else 0


# ------------------------------------------------------------------ nuclear bodies from seed loci
def seed_beads(seeds, copy_ptr, copy_idx):
    """(nseed,) int32: the ascending bead indices of all copies of the seed loci, from one
    0/1 flag per haploid locus (an array or the path of a text file).  ValueError for a
    wrong length, a value outside {0, 1} or no seed at all."""
    if isinstance(seeds, (str, os.PathLike)):
        seeds = np.loadtxt(os.fspath(seeds), dtype=np.int64, ndmin=1)
    seeds = np.asarray(seeds)
    nhap = len(copy_ptr) - 1
    if seeds.shape != (nhap,):
        raise ValueError('the seeds must hold one 0/1 flag per haploid locus (%d), got shape %s'
                         % (nhap, seeds.shape))
    if np.any((seeds != 0) & (seeds != 1)):
        raise ValueError('the seed flags must be 0 or 1')
    if not np.any(seeds == 1):
        raise ValueError('no locus is flagged as a seed')
    flag = np.repeat(seeds == 1, np.diff(copy_ptr))
    return np.sort(np.asarray(copy_idx)[flag]).astype(np.int32)


def seed_bodies(pop, seeds, link_cutoff=DEFAULT_LINK_CUTOFF, min_size=DEFAULT_MIN_BODY_SIZE, want_labels=True,
                ctx=None, device=0):
    """igm_report_seed_bodies: the bodies of every structure, the connected components (at
    least min_size seeds) of the graph that links two seeds whose float32 distance is <=
    link_cutoff.  seeds: the ascending bead indices (seed_beads), at most 8192.

    Returns {'label': (nstruct, nseed) int32 -- the smallest rank in every seed's component
    -- or None (want_labels=False), 'nbody': (nstruct,) int32, 'size': (nstruct, K) int32,
    0 past nbody, 'centre': (nstruct, K, 3) float64, NaN past nbody}, K = nbody.max(); the
    bodies of a structure are numbered in ascending label."""
    xyz, _ = _population(pop)
    nbead, S = xyz.shape[0], xyz.shape[1]
    seeds = np.ascontiguousarray(seeds, np.int32)
    if seeds.ndim != 1 or len(seeds) < 1:
        raise ValueError('seeds must be a non-empty list of bead indices')
    if int(min_size) < 1:
        raise ValueError('min_size must be >= 1')
    nseed = len(seeds)
    maxb = max(nseed // int(min_size), 1)  # cannot overflow
    c = ctx or _lib.context(device)
    label = np.empty((S, nseed), np.int32) if want_labels else None
    nbody = np.empty(S, np.int32)
    size = np.empty((S, maxb), np.int32)
    centre = np.empty((S, maxb, 3), np.float64)
    rc = c.lib.igm_report_seed_bodies(c.h, 0, xyz.ctypes.data, nbead, S, seeds.ctypes.data, nseed, float(link_cutoff),
                                      int(min_size), maxb, _lib.ptr(label), nbody.ctypes.data, size.ctypes.data,
                                      centre.ctypes.data)
    c.check(rc, 'igm_report_seed_bodies')
    K = int(nbody.max())
    return {'label': label, 'nbody': nbody, 'size': np.ascontiguousarray(size[:, :K]),
            'centre': np.ascontiguousarray(centre[:, :K])}


def body_features(pop, nbody, centre, assoc_cutoff=DEFAULT_ASSOC_CUTOFF, decay=DEFAULT_TSA_DECAY, want_nearest=False,
                  ctx=None, device=0):
    """igm_report_body_features: every bead against the bodies of every structure.  nbody
    (nstruct,), centre (nstruct, K, 3) float64 (seed_bodies, or any other source).

    Returns {'nearest': (nbead, nstruct) float64, the distance to the nearest body (NaN in a
    structure without one), or None (want_nearest=False), 'dist_sum' / 'dist_sqsum':
    (nbead,) float64 sums of nearest and its square over the structures with a body,
    'assoc': (nbead,) int64 structures with nearest <= assoc_cutoff, 'tsa_sum': (nbead,)
    float64, the sum over structures and bodies of exp(-decay * distance)}."""
    xyz, _ = _population(pop)
    nbead, S = xyz.shape[0], xyz.shape[1]
    nbody = np.ascontiguousarray(nbody, np.int32)
    centre = np.ascontiguousarray(centre, np.float64)
    if nbody.shape != (S,) or centre.ndim != 3 or centre.shape[0] != S or centre.shape[2] != 3:
        raise ValueError('nbody must be (nstruct,) and centre (nstruct, K, 3)')
    if centre.shape[1] == 0:  # no structure has a body: one unread slot per structure
        centre = np.full((S, 1, 3), np.nan)
    c = ctx or _lib.context(device)
    nearest = np.empty((nbead, S), np.float64) if want_nearest else None
    out = {'nearest': nearest, 'dist_sum': np.empty(nbead, np.float64), 'dist_sqsum': np.empty(nbead, np.float64),
           'assoc': np.empty(nbead, np.int64), 'tsa_sum': np.empty(nbead, np.float64)}
    rc = c.lib.igm_report_body_features(c.h, 0, xyz.ctypes.data, nbead, S, nbody.ctypes.data, centre.ctypes.data,
                                        centre.shape[1], float(assoc_cutoff), float(decay), _lib.ptr(nearest),
                                        out['dist_sum'].ctypes.data, out['dist_sqsum'].ctypes.data,
                                        out['assoc'].ctypes.data, out['tsa_sum'].ctypes.data)
    c.check(rc, 'igm_report_body_features')
    return out


def body_profiles(features, nbody, copy_ptr, copy_idx):
    """(nhap, 4) float64 per haploid locus from body_features: the mean distance to the
    nearest body, its standard deviation, the association frequency and the TSA signal.
    Per bead, over the n structures that have a body: mean = dist_sum / n, std =
    sqrt(max(0, dist_sqsum / n - mean^2)), frequency = assoc / n; TSA = tsa_sum / nstruct;
    then folded over the copies (_fold_copies).  n == 0 gives NaN, except TSA, which is 0."""
    nbody = np.asarray(nbody)
    S, n = len(nbody), int(np.count_nonzero(nbody > 0))
    dsum = np.asarray(features['dist_sum'], np.float64)
    cols = np.full((len(dsum), 4), np.nan)
    cols[:, 3] = np.asarray(features['tsa_sum'], np.float64) / S
    if n:
        with np.errstate(invalid='ignore', over='ignore'):
            mean = dsum / n
            var = np.asarray(features['dist_sqsum'], np.float64) / n - mean * mean
            cols[:, 0] = mean
            cols[:, 1] = np.sqrt(np.where(var < 0, 0.0, var))  # a NaN stays one
            cols[:, 2] = np.asarray(features['assoc'], np.float64) / n
    return np.stack([_fold_copies(cols[:, k], copy_ptr, copy_idx) for k in range(4)], axis=1)


# ------------------------------------------------------------------ pairwise conformation RMSD
def rmsd_edges_of(rmsd_max=DEFAULT_RMSD_MAX, rmsd_bins=DEFAULT_RMSD_BINS):
    """np.linspace(0, rmsd_max, rmsd_bins + 1) as float32: the edges of the RMSD histogram.
    ValueError unless rmsd_max is finite and > 0, rmsd_bins an integer in [1, 4096] and the
    float32 edges come out strictly increasing."""
    if not (np.isfinite(rmsd_max) and rmsd_max > 0):
        raise ValueError('the RMSD histogram needs a finite maximum > 0 (--rmsd-max)')
    if int(rmsd_bins) != rmsd_bins or not 1 <= int(rmsd_bins) <= MAX_RMSD_BINS:
        raise ValueError('the RMSD histogram needs between 1 and %d bins (--rmsd-bins)' % MAX_RMSD_BINS)
    return _rmsd_edges(np.linspace(0.0, float(rmsd_max), int(rmsd_bins) + 1))


def _rmsd_edges(edges):
    e = np.ascontiguousarray(edges, np.float32)
    if e.ndim != 1 or not 2 <= len(e) <= MAX_RMSD_BINS + 1 or not np.all(np.isfinite(e)) or np.any(np.diff(e) <= 0):
        raise ValueError('the RMSD histogram edges must be 2 to %d finite, strictly increasing float32 values'
                         % (MAX_RMSD_BINS + 1))
    return e


def conformation_beads(chrom, copy, copy_ptr, copy_idx, chrom_id, loci=None):
    """(ncopy, nlocus) int32: the beads of the haploid loci of chromosome chrom_id under each
    of its copies (ascending copy number), in locus order -- the `bead` table of
    igm_report_conformations.  loci: one 0/1 flag per haploid locus of the genome (an array
    or the path of a text file, the convention of seed_beads) that restricts the group, to
    one domain say.  ValueError for a wrong length, a flag other than 0 or 1, a chromosome
    that is not there or is left without loci, and loci whose copies are not the
    chromosome's."""
    chrom, copy = np.asarray(chrom), np.asarray(copy)
    copy_ptr, copy_idx = np.asarray(copy_ptr), np.asarray(copy_idx)
    nhap = len(copy_ptr) - 1
    pick = chrom[copy_idx[copy_ptr[:-1]]] == chrom_id
    if loci is not None:
        if isinstance(loci, (str, os.PathLike)):
            loci = np.loadtxt(os.fspath(loci), dtype=np.int64, ndmin=1)
        loci = np.asarray(loci)
        if loci.shape != (nhap,):
            raise ValueError('the loci must hold one 0/1 flag per haploid locus (%d), got shape %s'
                             % (nhap, loci.shape))
        if np.any((loci != 0) & (loci != 1)):
            raise ValueError('the locus flags must be 0 or 1')
        pick = pick & (loci == 1)
    hs = np.flatnonzero(pick)
    if len(hs) == 0:
        raise ValueError('chromosome %s has no loci to compare' % (chrom_id,))
    copies = np.unique(copy[chrom == chrom_id])
    if np.any(np.diff(copy_ptr)[hs] != len(copies)):
        raise ValueError('the loci of chromosome %s do not all have its %d copies' % (chrom_id, len(copies)))
    table = copy_idx[copy_ptr[hs][:, None] + np.arange(len(copies))[None, :]]      # (nlocus, ncopy)
    table = np.take_along_axis(table, np.argsort(copy[table], axis=1, kind='stable'), axis=1)
    if np.any(copy[table] != copies[None, :]) or np.any(chrom[table] != chrom_id):
        raise ValueError('the loci of chromosome %s do not all have its %d copies' % (chrom_id, len(copies)))
    return np.ascontiguousarray(table.T, np.int32)


def conformation_rmsd(pop, beads, edges=None, want_matrix=True, ctx=None, device=0):
    """igm_report_conformations on one group: beads (ncopy, nlocus) int32 (conformation_beads),
    conformation a = copy * nstruct + structure, M = ncopy * nstruct of them.

    Returns {'rmsd': (M, M) float32, the minimal RMSD after optimal rigid superposition of
    every two conformations, or None (want_matrix=False: every other entry has the same
    bytes without it), 'g': (M,) float64 sum of squared distances to the conformation's
    centre, 'row_sum' / 'row_n': (M,) float64 / int32, the sum and the number of the finite
    RMSDs to the other conformations, 'same': (nstruct, ncopy, ncopy) float32, the copies of
    one structure against each other, 'hist': (len(edges) - 1,) int64 over the pairs a < b
    (np.histogram on the float32 values) or None without edges, 'edges', 'nlocus'}.  A
    conformation with a non-finite coordinate has NaN in g, in its row and column, and
    counts nowhere."""
    xyz, _ = _population(pop)
    nbead, S = xyz.shape[0], xyz.shape[1]
    beads = np.ascontiguousarray(beads, np.int32)
    if beads.ndim != 2 or beads.shape[0] < 1 or beads.shape[1] < 1:
        raise ValueError('beads must be (ncopy, nlocus) with ncopy, nlocus >= 1')
    ncopy, nlocus = beads.shape
    M = ncopy * S
    e = _rmsd_edges(edges) if edges is not None else None
    c = ctx or _lib.context(device)
    out = {'rmsd': np.empty((M, M), np.float32) if want_matrix else None, 'g': np.empty(M, np.float64),
           'row_sum': np.empty(M, np.float64), 'row_n': np.empty(M, np.int32),
           'same': np.empty((S, ncopy, ncopy), np.float32),
           'hist': np.empty(len(e) - 1, np.int64) if e is not None else None, 'edges': e, 'nlocus': nlocus}
    rc = c.lib.igm_report_conformations(c.h, 0, xyz.ctypes.data, nbead, S, beads.ctypes.data, ncopy, nlocus,
                                        _lib.ptr(e), 0 if e is None else len(e), _lib.ptr(out['rmsd']),
                                        out['g'].ctypes.data, out['row_sum'].ctypes.data, out['row_n'].ctypes.data,
                                        out['same'].ctypes.data, _lib.ptr(out['hist']))
    c.check(rc, 'igm_report_conformations')
    return out


def conformation_summary(out, nstruct):
    """The numbers people take from conformation_rmsd's reductions, on the host and without
    the matrix: {'mean_rmsd': (M,) row_sum / row_n (NaN where row_n == 0), 'mean': the
    population mean pairwise RMSD sum(row_sum) / sum(row_n), 'mean_rg': the mean of
    sqrt(g / nlocus) over the conformations with a finite g, 'variability': mean / mean_rg,
    'medoid': (structure, copy) of the conformation with the smallest mean_rmsd, the lowest
    index on ties (the first conformation with a finite g when no mean is defined, (-1, -1)
    without one), 'medoid_mean_rmsd', and for ncopy > 1 (NaN otherwise) 'same_mean': the mean
    finite RMSD between copies of the same structure (from `same`), 'different_mean': between
    copies of different structures -- the total minus the same-structure pairs, as sums --
    and 'ratio' = same_mean / different_mean}."""
    g = np.asarray(out['g'], np.float64)
    row_sum, row_n = np.asarray(out['row_sum'], np.float64), np.asarray(out['row_n'], np.int64)
    M, S = len(g), int(nstruct)
    if S < 1 or M % S:
        raise ValueError('%d conformations are not a whole number of copies of %d structures' % (M, S))
    ncopy = M // S
    nan = float('nan')
    with np.errstate(invalid='ignore', divide='ignore'):
        mean_rmsd = np.where(row_n > 0, row_sum / row_n, np.nan)
    tot_sum, tot_n = float(row_sum.sum()), int(row_n.sum())          # every pair twice in both
    mean = tot_sum / tot_n if tot_n else nan
    fin = np.isfinite(g)
    mean_rg = float(np.sqrt(g[fin] / out['nlocus']).mean()) if fin.any() else nan
    res = {'mean_rmsd': mean_rmsd, 'mean': mean, 'mean_rg': mean_rg,
           'variability': mean / mean_rg if mean_rg > 0 else nan,
           'same_mean': nan, 'different_mean': nan, 'ratio': nan}
    if np.isfinite(mean_rmsd).any():
        a = int(np.nanargmin(mean_rmsd))
    else:
        a = int(np.argmax(fin)) if fin.any() else -1
    res['medoid'] = (a % S, a // S) if a >= 0 else (-1, -1)
    res['medoid_mean_rmsd'] = float(mean_rmsd[a]) if a >= 0 else nan
    if ncopy > 1:
        same = np.asarray(out['same'], np.float64).reshape(S, ncopy, ncopy)
        off = np.isfinite(same) & ~np.eye(ncopy, dtype=bool)[None]
        same_sum, same_n = float(same[off].sum()), int(off.sum())       # every pair twice here too
        diff_sum, diff_n = tot_sum - same_sum, tot_n - same_n
        res['same_mean'] = same_sum / same_n if same_n else nan
        res['different_mean'] = diff_sum / diff_n if diff_n else nan
        res['ratio'] = res['same_mean'] / res['different_mean'] if res['different_mean'] > 0 else nan
    return res


# ------------------------------------------------------------------ the Hi-C comparison
HIC_MASKS =('all', 'restrained', 'non_restrained')


def hic_edges():
    """(log_edges, lin_edges) of logloghist2d and density_histogram_2d as report_hic calls
    them (bins=(100, 100), ranges (1e-3, 1); report/plots.py:20-21, 89-90), the same on both
    axes: 100 logarithmic bins and -- np.linspace(x0, x1, bins) -- 99 linear ones."""
    return (np.logspace(np.log10(1e-3), np.log10(1), 100 + 1, base=10), np.linspace(1e-3, 1, 100))


def _sigma(v):
    """a sigma that is None, NaN or <= 0 is 'not given' (report_hic tests `if sigma:`)"""
    if v is None:
        return None
    v = float(v)
    return v if v > 0 else None


def _hcs(matrix):
    if isinstance(matrix, (str, os.PathLike)):
        from . import hss
        matrix = hss.read_hcs(os.fspath(matrix))
    return matrix


def hic_statistics(counts, nstruct, matrix, hap_chrom, intra_sigma=None, inter_sigma=None, log_edges=None,
                   lin_edges=None, nchrom=None, flags=0, ctx=None, device=0):
    """The raw igm_report_hic call: the sufficient statistics of the comparison between the
    haploid contact counts (nhap, nhap) int32 of evaluation.haploid_counts and the input
    matrix (the read_hcs dict: indptr, indices, data of the upper triangle).

    log_edges / lin_edges: None for no histogram, an edge array for both axes, or a pair
    (edges_x, edges_y).  With flags = IGM_DEVICE_PTRS, counts and the matrix's indices and
    data are device tensors.  Returns a dict of arrays over the nchrom + 1 populations (the
    chromosomes, then inter): n, dense_sums, sparse_ints, sparse_sumx, means, centred (the
    layouts of include/igm_hip.h), log_hist / lin_hist (ny, nx) int64 or None, nstruct and
    the sigmas used (None = not given)."""
    hap_chrom = np.ascontiguousarray(hap_chrom, np.int32)
    nhap = len(hap_chrom)
    indptr = np.ascontiguousarray(matrix['indptr'], np.int64)
    indices, data = matrix['indices'], matrix['data']
    if not (flags & _lib.IGM_DEVICE_PTRS):
        counts = np.ascontiguousarray(counts, np.int32)
        indices = np.ascontiguousarray(indices, np.int32)
        data = np.ascontiguousarray(data, np.float32)
        if len(indices) != len(data):
            raise ValueError('the matrix needs one value per column index')
    if tuple(counts.shape) != (nhap, nhap) or indptr.shape != (nhap + 1,):
        raise ValueError('counts must be (nhap, nhap) and indptr (nhap + 1,) for the %d entries of hap_chrom' % nhap)
    if indptr[-1] > len(indices):
        raise ValueError('indptr ends at %d, the matrix stores %d entries' % (indptr[-1], len(indices)))
    if nchrom is None:
        nchrom = int(hap_chrom.max()) + 1 if nhap else 0
    P = int(nchrom) + 1
    si, se = _sigma(intra_sigma), _sigma(inter_sigma)

    def edges(e):
        if e is None:
            return None, None, None
        ex, ey = e if isinstance(e, (tuple, list)) and len(e) == 2 and np.ndim(e[0]) == 1 else (e, e)
        ex, ey = np.ascontiguousarray(ex, np.float64), np.ascontiguousarray(ey, np.float64)
        return ex, ey, np.empty((len(ey) - 1, len(ex) - 1), np.int64)

    lgx, lgy, lgh = edges(log_edges)
    lix, liy, lih = edges(lin_edges)
    dense = np.empty((P, 2), np.int64)
    sparse = np.empty((P, 2, 3), np.int64)
    sumx = np.empty((P, 2), np.float64)
    means = np.empty((P, 3, 2), np.float64)
    cent = np.empty((P, 3, 2), np.float64)
    c = ctx or _lib.context(device)
    lnx, lny, inx, iny = (0 if e is None else len(e) - 1 for e in (lgx, lgy, lix, liy))
    rc = c.lib.igm_report_hic(c.h, int(flags), _lib.ptr(counts), nhap, int(nstruct), indptr.ctypes.data,
                              _lib.ptr(indices), _lib.ptr(data), hap_chrom.ctypes.data, int(nchrom),
                              0.0 if si is None else si, 0.0 if se is None else se,
                              _lib.ptr(lgx), lnx, _lib.ptr(lgy), lny, _lib.ptr(lgh),
                              _lib.ptr(lix), inx, _lib.ptr(liy), iny, _lib.ptr(lih),
                              dense.ctypes.data, sparse.ctypes.data, sumx.ctypes.data, means.ctypes.data,
                              cent.ctypes.data)
    c.check(rc, 'igm_report_hic')
    m = np.bincount(hap_chrom, minlength=int(nchrom)).astype(np.int64)
    n = np.concatenate([m * m, [(nhap * nhap - int((m * m).sum())) // 2]]).astype(np.int64)
    return {'n': n, 'dense_sums': dense, 'sparse_ints': sparse, 'sparse_sumx': sumx, 'means': means, 'centred': cent,
            'log_hist': lgh, 'lin_hist': lih, 'nstruct': int(nstruct), 'intra_sigma': si, 'inter_sigma': se}


def hic_correlations(stats):
    """Pearson r of every (population, mask) from the statistics of hic_statistics:
    {'intra': {mask: (nchrom,) float64}, 'inter': {mask: float}}, masks HIC_MASKS.

    r = cross / sqrt(var_x * var_y) with cross = centred[.., 0], var_x = centred[.., 1] +
    (n - n_stored) xbar^2 and var_y = (n sum c'^2 - (sum c')^2) / (n nstruct^2) computed
    exactly on the integers and rounded once.  A set with fewer than 2 entries or a
    constant side gives NaN (no warning); so does a mask whose sigma was not given."""
    from fractions import Fraction
    n_all, S = stats['n'], int(stats['nstruct'])
    P = len(n_all)
    r = np.full((P, 3), np.nan)
    for p in range(P):
        sig = stats['inter_sigma'] if p == P - 1 else stats['intra_sigma']
        d1, d2 = (int(v) for v in stats['dense_sums'][p])
        (w0, a0, b0), (w1, _, _) = ([int(v) for v in h] for h in stats['sparse_ints'][p])
        na = int(n_all[p])
        sets = ((na, d1, d2, w0 + w1), (w0, a0, b0, w0), (na - w0, d1 - a0, d2 - b0, w1))
        for m, (n, s1, s2, nst) in enumerate(sets):
            if n < 2 or (m > 0 and sig is None):
                continue
            var_y = float(Fraction(n * s2 - s1 * s1, n * S * S))
            xbar = float(stats['means'][p, m, 1])
            var_x = float(stats['centred'][p, m, 1]) + (n - nst) * (xbar * xbar)
            if not (var_y > 0 and var_x > 0):
                continue
            r[p, m] = max(-1.0, min(1.0, float(stats['centred'][p, m, 0]) / np.sqrt(var_x * var_y)))
    return {'intra': {k: r[:-1, m].copy() for m, k in enumerate(HIC_MASKS)},
            'inter': {k: float(r[-1, m]) for m, k in enumerate(HIC_MASKS)}}


def hic_comparison(pop, matrix, contact_range, intra_sigma=None, inter_sigma=None, radii=None, copy_ptr=None,
                   copy_idx=None, hap_chrom=None, ctx=None, device=0):
    """report_hic's numbers for a population: the contact counts at contact_range
    (evaluation.haploid_counts; the restraint's contact_range unchanged, as report_hic passes
    it to get_simulated_hic, hic.py:51 -- no 1 + EPS here), compared with the input matrix (a
    read_hcs dict or the path of a .hcs).  Returns {'intra': {mask: per-chromosome array},
    'inter': {mask: float}, 'log_hist', 'lin_hist' (int64, rows = output, columns = input),
    'log_edges', 'lin_edges', 'counts'}.  The chromosomes are the ids 0 .. max(hap_chrom)."""
    from . import evaluation
    xyz, store = _population(pop)
    radii = _pick(radii, store, 'radii')
    copy_ptr, copy_idx = _csr(_pick(copy_ptr, store, 'copy_ptr'), _pick(copy_idx, store, 'copy_idx'), xyz.shape[0],
                              'copy')
    hap_chrom = np.ascontiguousarray(_pick(hap_chrom, store, 'hap_chrom'), np.int32)
    matrix = _hcs(matrix)
    nhap = len(copy_ptr) - 1
    if hap_chrom.shape != (nhap,) or len(matrix['indptr']) != nhap + 1:
        raise ValueError('hap_chrom and the input matrix must cover the %d haploid loci of the population' % nhap)
    counts = evaluation.haploid_counts(xyz, radii, float(contact_range), copy_ptr, copy_idx, ctx=ctx, device=device)
    log_edges, lin_edges = hic_edges()
    stats = hic_statistics(counts, xyz.shape[1], matrix, hap_chrom, intra_sigma, inter_sigma, log_edges, lin_edges,
                           ctx=ctx, device=device)
    out = hic_correlations(stats)
    out.update({'log_hist': stats['log_hist'], 'lin_hist': stats['lin_hist'], 'log_edges': log_edges,
                'lin_edges': lin_edges, 'counts': counts})
    return out


def hic_correlation_texts(names, corr):
    """(intra text, inter text): matrix_comparison/{intra,inter}_correlations.txt in
    report_hic's formats (hic.py:88-94, 124-130); names: one per row of the intra arrays"""
    intra = '# chrom all imposed non_imposed\n'
    for k, c in enumerate(names):
        x, y, z = (corr['intra'][m][k] for m in HIC_MASKS)
        intra += f'{c:6s} {x:8.5f} {y:8.5f} {z:8.5f}\n'
    inter = '# all imposed non_imposed\n' + '{:8.5f} {:8.5f} {:8.5f}\n'.format(*(corr['inter'][m] for m in HIC_MASKS))
    return intra, inter


# ------------------------------------------------------------------ the igm-report driver
def _cfg_get(cfg, path, default=None):
    node = cfg
    for k in path.split('/'):
        if not isinstance(node, dict) or k not in node:
            return default
        node = node[k]
    return node


def parameters_from_config(cfg, basedir='.'):
    """get_parameters_from_igm_config (bin/igm-report:103-169) for the steps built here:
    {'semiaxes' or None, 'shape', 'damid': {'input_profile', 'contact_range'}, 'hic':
    {'input_matrix', 'contact_range', 'inter_sigma', 'intra_sigma'}}.  An exp_map nucleus
    has no semiaxes: the entry stays None instead of the reference's 5000.  The Hi-C sigmas
    come from runtime/Hi-C/{inter,intra}_sigma, else the old runtime/Hi-C/sigma, else the
    last entries of restraints/Hi-C/{inter,intra}_sigma_list, else of the old sigma_list."""
    out = {'semiaxes': None, 'shape': _cfg_get(cfg, 'model/restraints/envelope/nucleus_shape')}
    if _cfg_get(cfg, 'restraints/Hi-C', False):
        fpath = _cfg_get(cfg, 'restraints/Hi-C/input_matrix')
        if fpath and not os.path.isabs(fpath):
            fpath = os.path.abspath(os.path.join(basedir, fpath))
        hic = {'input_matrix': fpath, 'contact_range': _cfg_get(cfg, 'restraints/Hi-C/contact_range'),
               'inter_sigma': None, 'intra_sigma': None}
        if _cfg_get(cfg, 'runtime/Hi-C/inter_sigma', False):
            hic['inter_sigma'] = _cfg_get(cfg, 'runtime/Hi-C/inter_sigma')
            hic['intra_sigma'] = _cfg_get(cfg, 'runtime/Hi-C/intra_sigma')
        elif _cfg_get(cfg, 'runtime/Hi-C/sigma', False):
            hic['inter_sigma'] = hic['intra_sigma'] = _cfg_get(cfg, 'runtime/Hi-C/sigma')
        elif _cfg_get(cfg, 'restraints/Hi-C/inter_sigma_list', False):
            hic['inter_sigma'] = _cfg_get(cfg, 'restraints/Hi-C/inter_sigma_list')[-1]
            l2 = _cfg_get(cfg, 'restraints/Hi-C/intra_sigma_list', None)
            if l2:
                hic['intra_sigma'] = l2[-1]
        elif _cfg_get(cfg, 'restraints/Hi-C/sigma_list', False):
            hic['inter_sigma'] = hic['intra_sigma'] = _cfg_get(cfg, 'restraints/Hi-C/sigma_list')[-1]
        out['hic'] = hic
    if _cfg_get(cfg, 'restraints/DamID', False):
        fpath = _cfg_get(cfg, 'restraints/DamID/input_profile')
        if fpath and not os.path.isabs(fpath):
            fpath = os.path.abspath(os.path.join(basedir, fpath))
        out['damid'] = {'input_profile': fpath,
                        'contact_range': _cfg_get(cfg, 'restraints/DamID/contact_range', DEFAULT_DAMID_CONTACT_RANGE)}
    if out['shape'] == 'exp_map':
        return out
    if _cfg_get(cfg, 'model/restraints/envelope/nucleus_semiaxes', False):
        out['semiaxes'] = np.array(_cfg_get(cfg, 'model/restraints/envelope/nucleus_semiaxes'), np.float64)
    elif _cfg_get(cfg, 'model/restraints/envelope/nucleus_radius', False):
        out['semiaxes'] = np.array([_cfg_get(cfg, 'model/restraints/envelope/nucleus_radius')] * 3, np.float64)
    return out


def apply_hic_arguments(params, hic=None, hic_sigma=None, hic_inter_sigma=None, hic_intra_sigma=None,
                        hic_contact_range=None):
    """process_user_args (bin/igm-report:179-212) on the dict of parameters_from_config:
    --hic names the input matrix (and opens a Hi-C section when the configuration had
    none); --hic-sigma sets both sigmas, then --hic-inter-sigma / --hic-intra-sigma each
    its own, then --hic-contact-range; all but --hic are ignored without a Hi-C section."""
    params = dict(params)
    if hic is not None:
        params['hic'] = dict(params.get('hic') or {'contact_range': None, 'inter_sigma': None, 'intra_sigma': None})
        params['hic']['input_matrix'] = os.path.abspath(hic)
    if 'hic' not in params:
        return params
    params['hic'] = dict(params['hic'])
    if hic_sigma is not None:
        params['hic']['inter_sigma'] = params['hic']['intra_sigma'] = hic_sigma
    if hic_inter_sigma is not None:
        params['hic']['inter_sigma'] = hic_inter_sigma
    if hic_intra_sigma is not None:
        params['hic']['intra_sigma'] = hic_intra_sigma
    if hic_contact_range is not None:
        params['hic']['contact_range'] = hic_contact_range
    return params


def _hss_extras(path):
    """(envelope shape or None, envelope/params or None, genome chroms or None, config_data or None)"""
    from . import h5
    shape = params = chroms = config = None
    with h5.File(path) as f:
        top = f.keys('/')
        if 'envelope/' in top:
            names = f.keys('envelope')
            if 'shape' in names:
                shape = f.read('envelope/shape')
                shape = shape.decode() if isinstance(shape, bytes) else str(shape)
            if 'params' in names:
                params = np.atleast_1d(np.asarray(f.read('envelope/params'), np.float64))
        if 'genome/' in top and 'chroms' in f.keys('genome'):
            chroms = [c.decode() if isinstance(c, bytes) else str(c) for c in f.read('genome/chroms')]
        if 'config_data' in top:
            config = f.read('config_data')
    return shape, params, chroms, config


def named_maps(cfg, nstruct):
    """(volumes, struct_map) of an exp_map configuration that itself names its maps --
    model/restraints/envelope/volume_prefix and volumes_idx present as raw keys, not through
    the schema defaults ('' and [0]) -- else None.  The files are those of
    steps.envelope_section(cfg, range(nstruct))."""
    env = _cfg_get(cfg, 'model/restraints/envelope')
    if not isinstance(env, dict) or 'volume_prefix' not in env or 'volumes_idx' not in env:
        return None
    if env.get('nucleus_shape') != 'exp_map':
        return None
    from .steps import envelope_section
    sec = envelope_section(cfg, range(nstruct))
    return sec['volumes'], sec['struct_map']


def resolve_semiaxes(hss_envelope, cfg_params, explicit=None):
    """The semiaxes of the radial, shell and lamina numbers, or None when the nucleus is an
    exp_map and none were given.  Order: the caller's explicit semiaxes; envelope/params
    stored in the .hss (a scalar is a sphere; report_radials:101-107); the configuration's
    nucleus_semiaxes or nucleus_radius (bin/igm-report:120-127); 5000 on every axis.
    hss_envelope: (shape, params) read from the file."""
    if explicit is not None:
        return _semiaxes(explicit)
    shape, params = hss_envelope
    cfg_shape = (cfg_params or {}).get('shape')
    if shape == 'exp_map' or cfg_shape == 'exp_map':
        return None  # an imaged nucleus: no ellipsoid to measure against, never guessed
    if params is not None:
        return _semiaxes(params)
    if cfg_params and cfg_params.get('semiaxes') is not None:
        return _semiaxes(cfg_params['semiaxes'])
    return _semiaxes(DEFAULT_SEMIAXES)


def pearson(x, y):
    """(r,) or (r, p): Pearson r in plain NumPy, its two-sided p-value from scipy when
    importable (report_damid writes scipy's pair)"""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    xm, ym = x - x.mean(), y - y.mean()
    r = float((xm * ym).sum() / np.sqrt((xm * xm).sum() * (ym * ym).sum()))
    try:
        from scipy.stats import pearsonr
    except ImportError:
        return (r,)
    return (r, float(pearsonr(x, y)[1]))


def report_population(hss_path, cfg=None, out_dir=None, steps=STEPS, label='', semiaxes=None, ctx=None, device=0,
                      hic=None, hic_sigma=None, hic_inter_sigma=None, hic_intra_sigma=None, hic_contact_range=None,
                      neighbour_cutoff=DEFAULT_NEIGHBOUR_CUTOFF, min_sep=1, compaction_halfwidth=2, classes=None,
                      seeds=None, link_cutoff=DEFAULT_LINK_CUTOFF, min_body_size=DEFAULT_MIN_BODY_SIZE,
                      assoc_cutoff=DEFAULT_ASSOC_CUTOFF, tsa_decay=DEFAULT_TSA_DECAY, conformation_chroms=None,
                      conformation_loci=None, save_rmsd=False, rmsd_edges=None):
    """Write the numeric files of bin/igm-report for the population at hss_path into
    out_dir (default: QC_<label or file name> beside it) and return {relative name: path}.

    cfg: an IGM configuration (dict or JSON file); None looks for config_data in the .hss,
    then for igm-config.json beside it (bin/igm-report:236-262).  steps: any of STEPS, and
    'hic', 'bodies', the FEATURE_STEPS, 'seeded_bodies' and 'conformations' (not run by
    default).  radials, shells and damid need semiaxes
    (resolve_semiaxes).  On an exp_map nucleus without explicit ones they run in their map
    forms when the configuration names its maps (named_maps): the same file names hold the
    levels below the lamina, density_histo.txt is divided by the real shell volumes (nan for
    a bin without volume) and radials/lamina_depth.txt holds the mean signed depth per
    haploid locus; a configuration that names no maps raises ValueError.  bodies needs
    model/restraints/nucleolus and writes bodies/nucleolus_frequency.txt (contacts at
    restraints/nuclDamID/contact_range, else the DamID default) and
    bodies/nucleolus_distance.txt (the mean of -depth).  hic needs the Hi-C
    section of the configuration or the hic argument (the path of the input .hcs; the
    hic_* arguments are the command line's, apply_hic_arguments) and raises ValueError
    without one (the reference only logs).  It writes matrix_comparison/outmap.hcs,
    intra_correlations.txt, inter_correlations.txt and -- this project's addition, the
    reference only draws them -- the raw int64 histograms log_histogram2d.npy and
    linear_histogram2d.npy.  When a sigma is not given its imposed / non_imposed columns
    are nan (the reference then writes no intra rows and zeros in the inter row).

    FEATURE_STEPS (this project's, not run by default either): neighbours writes
    neighbours/icp.txt (inter_chromosomal_fraction at neighbour_cutoff and min_sep, one value
    per haploid locus), neighbours/mean_counts.txt (nhap x ncol: the census sums divided by
    nstruct, averaged over the copies) and, with classes -- one label per haploid locus, an
    array or a text file, -1 unlabelled, at most 8 classes; a wrong length or a label out of
    range raises ValueError before anything is written -- neighbours/trans_fraction.txt
    (trans_class_fraction, nhap x nclass).  compaction writes compaction/local_rg.txt (nhap x
    2: the mean and the standard deviation over copies and structures of local_compaction at
    compaction_halfwidth).

    seeded_bodies (not run by default) needs seeds -- one 0/1 flag per haploid locus, an
    array or a text file (seed_beads); without them it raises a ValueError that names
    --seeds, and a bad cutoff, decay or size raises before anything is written.  It writes
    seeded_bodies/count.txt (the bodies of every structure, seed_bodies at link_cutoff and
    min_body_size), seeded_bodies/centres.txt (rows of structure, body, size, x, y, z) and
    seeded_bodies/profiles.txt (nhap x 4: body_profiles of body_features at assoc_cutoff and
    tsa_decay).

    conformations (not run by default) compares the copies of every chromosome in
    conformation_chroms (ids as in the index; None: all of them) across the population by
    their minimal RMSD after superposition (conformation_rmsd), on the loci flagged in
    conformation_loci (one 0/1 flag per haploid locus, an array or a text file; None: all).
    It writes conformations/summary.txt (one row per chromosome: id, nlocus, ncopy, M, mean
    RMSD, mean Rg, variability, medoid structure, medoid copy, the medoid's mean RMSD, the
    same-structure mean, the different-structure mean, their ratio -- nan for a single
    copy; conformation_summary), conformations/<id>_mean_rmsd.txt (M values, conformation
    copy * nstruct + structure), conformations/histogram.txt (one row per bin of rmsd_edges,
    default rmsd_edges_of(): its lower and upper edge, then one count column per
    chromosome) and with save_rmsd conformations/<id>_rmsd.npy, the (M, M) float32 matrix.
    A chromosome id that is not in the index, bad loci or bad edges raise ValueError before
    anything is written."""
    from .steps import PopulationStore
    steps = tuple(steps.split(',')) if isinstance(steps, str) else tuple(steps)
    known = STEPS + OPTIONAL_STEPS + BODY_STEPS + FEATURE_STEPS + SEED_STEPS + CONFORMATION_STEPS
    unknown = [s for s in steps if s not in known]
    if unknown:
        raise ValueError('unknown report steps %s (known: %s)' % (unknown, ', '.join(known)))
    hss_path = os.path.realpath(hss_path)
    store = PopulationStore(hss_path)
    env_shape = env_params = chrom_names = stored = None
    if store.is_hss:
        env_shape, env_params, chrom_names, stored = _hss_extras(hss_path)
    basedir = os.path.dirname(hss_path)
    if isinstance(cfg, str):
        basedir = os.path.dirname(os.path.abspath(cfg))
        with open(cfg) as f:
            cfg = json.load(f)
    elif cfg is None:
        if stored:
            cfg = json.loads(stored)
        elif os.path.isfile(os.path.join(basedir, 'igm-config.json')):
            with open(os.path.join(basedir, 'igm-config.json')) as f:
                cfg = json.load(f)
    params = parameters_from_config(cfg, basedir) if cfg is not None else {'semiaxes': None, 'shape': None}
    params = apply_hic_arguments(params, hic, hic_sigma, hic_inter_sigma, hic_intra_sigma, hic_contact_range)
    if 'hic' in steps:
        hcfg = params.get('hic')
        if not hcfg or not hcfg.get('input_matrix'):
            raise ValueError('the hic step needs an input matrix: a restraints/Hi-C section in the configuration '
                             'or --hic')
        if hcfg.get('contact_range') is None:
            raise ValueError('the hic step needs a contact range: restraints/Hi-C/contact_range or '
                             '--hic-contact-range')
    sx = resolve_semiaxes((env_shape, env_params), params, semiaxes)
    needs = [s for s in steps if s in ('radials', 'shells', 'damid')]
    maps = None
    if sx is None and needs:
        maps = named_maps(cfg, store.nstruct)
        if maps is None:
            raise ValueError('the nucleus is an exp_map (no ellipsoid) and the configuration names no maps '
                             '(model/restraints/envelope/volume_prefix and volumes_idx): the steps %s need explicit '
                             'semiaxes' % ', '.join(needs))
        for v in maps[0]:
            map_depth_scale(v)  # a map without depth raises here, before anything is written
    bodies = None
    if 'bodies' in steps:
        if not isinstance(_cfg_get(cfg, 'model/restraints/nucleolus'), dict):
            raise ValueError('the bodies step needs model/restraints/nucleolus in the configuration')
        from .steps import nucleolus_section
        sec = nucleolus_section(cfg, range(store.nstruct))
        bodies = (sec['volumes'], sec['struct_map'])
        for v in bodies[0]:
            map_depth_scale(v)
    bead_classes, nclass = None, 0
    if 'neighbours' in steps:
        if not (np.isfinite(neighbour_cutoff) and neighbour_cutoff >= 0) or int(min_sep) < 1:
            raise ValueError('the neighbours step needs a finite cutoff >= 0 and min_sep >= 1')
        if classes is not None:
            bead_classes, nclass = haploid_classes(classes, store.copy_ptr, store.copy_idx)
    if 'compaction' in steps and int(compaction_halfwidth) < 0:
        raise ValueError('the compaction step needs a halfwidth >= 0')
    seed_idx = None
    if 'seeded_bodies' in steps:
        if seeds is None:
            raise ValueError('the seeded_bodies step needs the seed loci: --seeds FILE, one 0/1 flag per haploid '
                             'locus')
        for name, v in (('link cutoff', link_cutoff), ('association cutoff', assoc_cutoff), ('TSA decay', tsa_decay)):
            if not (np.isfinite(v) and v >= 0):
                raise ValueError('the seeded_bodies step needs a finite %s >= 0' % name)
        if int(min_body_size) < 1:
            raise ValueError('the seeded_bodies step needs a minimum body size >= 1')
        seed_idx = seed_beads(seeds, store.copy_ptr, store.copy_idx)
    groups, edges32 = [], None
    if 'conformations' in steps:
        edges32 = rmsd_edges_of() if rmsd_edges is None else _rmsd_edges(rmsd_edges)
        have = np.unique(store.chrom)
        want = have if conformation_chroms is None else np.atleast_1d(np.asarray(conformation_chroms))
        for cid in want:
            if cid not in have:
                raise ValueError('the conformations step: chromosome id %s is not in the index (ids: %s)'
                                 % (cid, ', '.join(str(i) for i in have)))
            groups.append((int(cid), conformation_beads(store.chrom, store.copy, store.copy_ptr, store.copy_idx, cid,
                                                        conformation_loci)))
    if out_dir is None:
        base = os.path.splitext(os.path.basename(hss_path))[0]
        out_dir = os.path.join(os.path.dirname(hss_path), 'QC_' + (label or base))
    out_dir = os.path.realpath(os.path.abspath(out_dir))
    tag = '-' + label if label else ''
    xyz = np.ascontiguousarray(store.coordinates(), np.float32)
    kw = {'ctx': ctx, 'device': device}
    written = {}

    def path(rel):
        p = os.path.join(out_dir, rel)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        written[rel] = p
        return p

    os.makedirs(out_dir, exist_ok=True)
    with open(path('label.txt'), 'w') as f:
        f.write(label)
    if 'rgs' in steps:
        ids, rgs = chromosome_rgs(xyz, store.chrom, store.copy, **kw)
        names = chrom_names if chrom_names is not None and len(chrom_names) >= len(ids) else \
            ['chr%d' % (i + 1) for i in ids]
        np.savez(path('radius_of_gyration/chromosomes%s.npz' % tag), **{c: a for c, a in zip(names, rgs)})
    if 'shells' in steps:
        if maps is None:
            smean, _, _ = shells(xyz, sx, **kw)
        else:
            smean, _, _ = map_shells(xyz, maps[0], maps[1], **kw)
        np.savetxt(path('shells/ave_radial%s.txt' % tag), np.average(smean, axis=0))
    if 'radials' in steps:
        if maps is None:
            radials = radial_levels(xyz, sx, store.copy_ptr, store.copy_idx, **kw)
            counts, edges = radial_density(xyz, sx, **kw)
            volumes = np.array([edges[i + 1]**3 - edges[i]**3 for i in range(len(counts))])
        else:  # an imaged nucleus: the level below the map's lamina and the real shell volumes
            radials, depth = map_levels(xyz, maps[0], maps[1], store.copy_ptr, store.copy_idx, **kw)
            np.savetxt(path('radials/lamina_depth%s.txt' % tag), depth)
            counts, edges, volumes = map_density(xyz, maps[0], maps[1], **kw)
            volumes = np.where(volumes > 0, volumes, np.nan)  # a bin without volume is nan
        np.savetxt(path('radials/radials%s.txt' % tag), radials)
        np.savetxt(path('radials/density_histo%s.txt' % tag), counts / volumes)
        ave = os.path.join(out_dir, 'shells/ave_radial%s.txt' % tag)
        if os.path.isfile(ave):  # normalised with respect to the last shell (report_radials:119-122)
            np.savetxt(path('radials/radials_norm%s.txt' % tag), radials / np.loadtxt(ave)[-1])
    if 'damid' in steps:
        dcfg = params.get('damid') or {}
        cr = dcfg.get('contact_range', DEFAULT_DAMID_CONTACT_RANGE)
        if maps is None:
            freq = lamina_frequency(xyz, store.radii, store.copy_ptr, store.copy_idx, sx, cr, **kw)
        else:
            freq = map_lamina_frequency(xyz, maps[0], maps[1], store.radii, store.copy_ptr, store.copy_idx, cr, **kw)
        np.savetxt(path('damid/output.txt'), freq)
        if dcfg.get('input_profile'):
            profile = np.loadtxt(dcfg['input_profile'], dtype='float32')
            np.savetxt(path('damid/input%s.txt' % tag), profile)
            np.savetxt(path('damid/pearsonr%s.txt' % tag), pearson(profile, freq))
    if 'bodies' in steps:  # the nucleolus: contacts towards the inside of the body, distance = -depth
        cr = _cfg_get(cfg, 'restraints/nuclDamID/contact_range', DEFAULT_DAMID_CONTACT_RANGE)
        np.savetxt(path('bodies/nucleolus_frequency%s.txt' % tag),
                   map_lamina_frequency(xyz, bodies[0], bodies[1], store.radii, store.copy_ptr, store.copy_idx, cr,
                                        side=-1, **kw))
        _, depth = map_levels(xyz, bodies[0], bodies[1], store.copy_ptr, store.copy_idx, **kw)
        np.savetxt(path('bodies/nucleolus_distance%s.txt' % tag), -depth)
    if 'distance_map' in steps:
        np.save(path('distance_map/average%s.npy' % tag),
                average_distance_map(xyz, store.copy_ptr, store.copy_idx, store.hap_chrom, **kw))
    if 'neighbours' in steps:
        res = neighbour_census(xyz, neighbour_cutoff, chain_numbers(store.chrom, store.copy), bead_classes, nclass,
                               int(min_sep), want_census=nclass > 0, **kw)
        np.savetxt(path('neighbours/icp%s.txt' % tag),
                   _fold_copies(icp_of(res['icp_sum'], res['icp_n']), store.copy_ptr, store.copy_idx))
        mean = res['sums'].astype(np.float64) / xyz.shape[1]
        np.savetxt(path('neighbours/mean_counts%s.txt' % tag),
                   np.stack([average_copies(mean[:, k], store.copy_ptr, store.copy_idx)
                             for k in range(mean.shape[1])], axis=1))
        if nclass:
            np.savetxt(path('neighbours/trans_fraction%s.txt' % tag),
                       trans_class_fraction(res['census'], store.copy_ptr, store.copy_idx))
    if 'compaction' in steps:
        lrg = local_compaction(xyz, store.chrom, store.copy, int(compaction_halfwidth), **kw)
        rows = [lrg[store.copy_idx[store.copy_ptr[h]:store.copy_ptr[h + 1]]].ravel()
                for h in range(len(store.copy_ptr) - 1)]
        np.savetxt(path('compaction/local_rg%s.txt' % tag), np.array([(r.mean(), r.std()) for r in rows]))
    if 'seeded_bodies' in steps:
        found = seed_bodies(xyz, seed_idx, link_cutoff, int(min_body_size), want_labels=False, **kw)
        nbody, size, centre = found['nbody'], found['size'], found['centre']
        np.savetxt(path('seeded_bodies/count%s.txt' % tag), nbody, fmt='%d')
        with open(path('seeded_bodies/centres%s.txt' % tag), 'w') as f:
            for s in range(len(nbody)):
                for k in range(nbody[s]):
                    f.write('%d %d %d %.17g %.17g %.17g\n' % ((s, k, size[s, k]) + tuple(centre[s, k])))
        feat = body_features(xyz, nbody, centre, assoc_cutoff, tsa_decay, **kw)
        np.savetxt(path('seeded_bodies/profiles%s.txt' % tag),
                   body_profiles(feat, nbody, store.copy_ptr, store.copy_idx))
    if 'conformations' in steps:
        rows, hists = [], []
        for cid, beads in groups:
            res = conformation_rmsd(xyz, beads, edges32, want_matrix=bool(save_rmsd), **kw)
            sm = conformation_summary(res, xyz.shape[1])
            rows.append((cid, beads.shape[1], beads.shape[0], len(res['g']), sm['mean'], sm['mean_rg'],
                         sm['variability'], sm['medoid'][0], sm['medoid'][1], sm['medoid_mean_rmsd'],
                         sm['same_mean'], sm['different_mean'], sm['ratio']))
            hists.append(res['hist'])
            np.savetxt(path('conformations/%d_mean_rmsd%s.txt' % (cid, tag)), sm['mean_rmsd'])
            if save_rmsd:
                np.save(path('conformations/%d_rmsd%s.npy' % (cid, tag)), res['rmsd'])
        with open(path('conformations/summary%s.txt' % tag), 'w') as f:
            f.write('# id nlocus ncopy M mean_rmsd mean_rg variability medoid_structure medoid_copy '
                    'medoid_mean_rmsd same_structure_mean different_structure_mean ratio\n')
            for r in rows:
                f.write('%d %d %d %d %.17g %.17g %.17g %d %d %.17g %.17g %.17g %.17g\n' % r)
        with open(path('conformations/histogram%s.txt' % tag), 'w') as f:
            f.write('# lower upper %s\n' % ' '.join(str(cid) for cid, _ in groups))
            for b in range(len(edges32) - 1):
                f.write('%.9g %.9g %s\n' % (edges32[b], edges32[b + 1], ' '.join(str(int(h[b])) for h in hists)))
    if 'hic' in steps:
        from . import hss
        hcfg = params['hic']
        res = hic_comparison(xyz, hcfg['input_matrix'], float(hcfg['contact_range']), hcfg.get('intra_sigma'),
                             hcfg.get('inter_sigma'), store.radii, store.copy_ptr, store.copy_idx, store.hap_chrom,
                             **kw)
        index, genome = hss.haploid_index(hss_path) if store.is_hss else (None, None)
        hss.write_hcs(path('matrix_comparison/outmap%s.hcs' % tag), res['counts'], nstruct=xyz.shape[1],
                      chrom=store.hap_chrom, index=index, genome=genome)
        ids = np.unique(store.hap_chrom)
        names = chrom_names if chrom_names is not None and len(chrom_names) >= len(ids) else \
            ['chr%d' % (i + 1) for i in ids]
        rows = {'intra': {m: res['intra'][m][ids] for m in HIC_MASKS}, 'inter': res['inter']}
        intra, inter = hic_correlation_texts(names[:len(ids)], rows)
        with open(path('matrix_comparison/intra_correlations%s.txt' % tag), 'w') as f:
            f.write(intra)
        with open(path('matrix_comparison/inter_correlations%s.txt' % tag), 'w') as f:
            f.write(inter)
        np.save(path('matrix_comparison/log_histogram2d%s.npy' % tag), res['log_hist'])
        np.save(path('matrix_comparison/linear_histogram2d%s.npy' % tag), res['lin_hist'])
    return written


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog='python -m igm_amd.report', description='Run population analysis pipeline')
    ap.add_argument('hss', help='Hss file for population')
    ap.add_argument('-c', '--config', help='Config file for IGM run (infers some parameters)')
    ap.add_argument('-l', '--label', help='Run label to be applied in filenames', default='')
    ap.add_argument('--semiaxes', nargs=3, type=float, help='Specify semiaxes of the envelope')
    ap.add_argument('--steps', default=','.join(STEPS),
                    help='comma separated list of steps to perform (default: %(default)s)')
    ap.add_argument('-o', '--out-dir', help='Output directory')
    ap.add_argument('--hic', help='Input matrix for HiC')
    ap.add_argument('--hic-sigma', type=float, help='Probability cutoff for HiC')
    ap.add_argument('--hic-inter-sigma', type=float, help='Inter-chromosomal probability cutoff for HiC')
    ap.add_argument('--hic-intra-sigma', type=float, help='Intra-chromosomal probability cutoff for HiC')
    ap.add_argument('--hic-contact-range', type=float, help='Probability cutoff for HiC')
    ap.add_argument('--neighbour-cutoff', type=float, default=DEFAULT_NEIGHBOUR_CUTOFF,
                    help='Neighbourhood radius of the neighbours step (default: %(default)s)')
    ap.add_argument('--min-sep', type=int, default=1,
                    help='Ignore cis neighbours closer than this on the bead index (default: %(default)s)')
    ap.add_argument('--compaction-halfwidth', type=int, default=2,
                    help='Beads on either side in the window of the compaction step (default: %(default)s)')
    ap.add_argument('--classes', help='Text file with one integer class label per haploid locus (-1: unlabelled)')
    ap.add_argument('--seeds', help='Text file with one 0/1 flag per haploid locus: the seed loci of the '
                                    'seeded_bodies step')
    ap.add_argument('--link-cutoff', type=float, default=DEFAULT_LINK_CUTOFF,
                    help='Seeds this close are linked into one body (default: %(default)s)')
    ap.add_argument('--min-body-size', type=int, default=DEFAULT_MIN_BODY_SIZE,
                    help='Seeds a component needs to count as a body (default: %(default)s)')
    ap.add_argument('--assoc-cutoff', type=float, default=DEFAULT_ASSOC_CUTOFF,
                    help='A bead this close to a body centre is associated with it (default: %(default)s)')
    ap.add_argument('--tsa-decay', type=float, default=DEFAULT_TSA_DECAY,
                    help='Decay of the predicted TSA-seq signal per length unit (default: %(default)s)')
    ap.add_argument('--conformation-chroms', help='Comma separated chromosome ids (as in the index) of the '
                                                  'conformations step (default: all)')
    ap.add_argument('--conformation-loci', help='Text file with one 0/1 flag per haploid locus: the loci the '
                                                'conformations step compares (default: all)')
    ap.add_argument('--save-rmsd', action='store_true',
                    help='Also write the full RMSD matrix of every chromosome of the conformations step')
    ap.add_argument('--rmsd-max', type=float, default=DEFAULT_RMSD_MAX,
                    help='Upper end of the RMSD histogram (default: %(default)s)')
    ap.add_argument('--rmsd-bins', type=int, default=DEFAULT_RMSD_BINS,
                    help='Bins of the RMSD histogram (default: %(default)s)')
    a = ap.parse_args(argv)
    if not os.path.isfile(a.hss):
        ap.error('Cannot find file %s' % a.hss)
    chroms = None
    if a.conformation_chroms is not None:
        try:
            chroms = [int(v) for v in a.conformation_chroms.split(',')]
        except ValueError:
            raise ValueError('--conformation-chroms takes comma separated integer ids, got %r'
                             % a.conformation_chroms)
    written = report_population(a.hss, cfg=a.config, out_dir=a.out_dir, steps=a.steps, label=a.label,
                                semiaxes=a.semiaxes, hic=a.hic, hic_sigma=a.hic_sigma,
                                hic_inter_sigma=a.hic_inter_sigma, hic_intra_sigma=a.hic_intra_sigma,
                                hic_contact_range=a.hic_contact_range, neighbour_cutoff=a.neighbour_cutoff,
                                min_sep=a.min_sep, compaction_halfwidth=a.compaction_halfwidth, classes=a.classes,
                                seeds=a.seeds, link_cutoff=a.link_cutoff, min_body_size=a.min_body_size,
                                assoc_cutoff=a.assoc_cutoff, tsa_decay=a.tsa_decay, conformation_chroms=chroms,
                                conformation_loci=a.conformation_loci, save_rmsd=a.save_rmsd,
                                rmsd_edges=rmsd_edges_of(a.rmsd_max, a.rmsd_bins))
    for rel in sorted(written):
        print(written[rel])
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
