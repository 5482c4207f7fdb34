"""Inputs that put the report on imaged nuclei on its edges, shared by test_report_map.py
(CPU: every input is the edge it claims) and test_report_map_gpu.py (the kernels against
the restatement report_map_ref.py).  Plain NumPy, seeded, nothing touches the GPU.

  maps        the three sphere maps of damid_edges.maps() (11, 13 and 11 voxels a side) and
              one NON-cubic box map, nvoxel (5, 7, 9) on grids (1.0, 0.5, 0.25): every grid
              step is a power of two, so voxel centres, half-steps and offsets are exact
  struct_map  2, 0, 1, 1, 0, 2, 0, 3 cyclically
  beads       KINDS below, dealt in rotation over (bead, structure)
  genome      damid_edges': loci with 1, 2, 3, 4, 0 and 2 copies behind a copy index that is
              neither contiguous nor ascending, every copy another radius
"""
import functools

import numpy as np

import damid_edges as D
import report_map_ref as M

f32, f64 = np.float32, np.float64
SMAP_PATTERN = (2, 0, 1, 1, 0, 2, 0, 3)
KINDS = ('centre', 'half', 'lamina', 'deepest', 'deep_off', 'outside_in_grid')
OFFSETS = (0.0, 0.5, 0.25, -0.25, -0.5)


def box_map():
    """nvoxel (5, 7, 9), grids (1.0, 0.5, 0.25), centred on 0: the voxels 1..3 x 1..5 x 1..7
    are inside, the EDT taken with the grid as sampling"""
    from scipy import ndimage
    n, g = np.array([5, 7, 9]), np.array([1.0, 0.5, 0.25])
    inside = np.zeros(n, bool)
    inside[1:4, 1:6, 1:8] = True
    er = ndimage.binary_erosion(inside, structure=ndimage.generate_binary_structure(3, 1), border_value=0)
    lamina = inside & ~er
    _, idx = ndimage.distance_transform_edt(~lamina, sampling=g, return_indices=True)
    mat = np.zeros(tuple(n) + (4,), np.int32)
    mat[..., 0], mat[..., 1], mat[..., 2] = idx[0], idx[1], idx[2]
    mat[..., 3] = inside
    return dict(body_idx=0, nvoxel=n.astype(np.int32), center=np.zeros(3, f32),
                origin=(-g * (n - 1) / 2.0).astype(f32), grid=g.astype(f32), matrice=mat)


@functools.lru_cache(maxsize=None)
def maps():
    return tuple(D.maps()) + (box_map(),)


@functools.lru_cache(maxsize=None)
def scales():
    return tuple(M.depth_scale(v) for v in maps())


def struct_map(S):
    return np.array([SMAP_PATTERN[s % len(SMAP_PATTERN)] for s in range(S)], np.int32)


def centre_of(vol, idx):
    n, o, g = M.geometry(vol)
    return o + np.asarray(idx, f64) * g


@functools.lru_cache(maxsize=None)
def landmarks(m):
    """of map m: (lamina voxels that are their own record, the deepest voxel, voxels in the
    grid with w == 0), as index arrays"""
    vol = maps()[m]
    mat = vol['matrice']
    n = M.geometry(vol)[0]
    idx = np.stack(np.meshgrid(*[np.arange(k) for k in n], indexing='ij'), axis=-1)
    own = (mat[..., 3] != 0) & np.all(mat[..., :3] == idx, axis=-1)
    g = M.geometry(vol)[2]
    t = (idx - mat[..., :3]).astype(f64) * g
    d = np.where(mat[..., 3] != 0, np.sqrt((t[..., 0]**2 + t[..., 2]**2) + t[..., 1]**2), -1.0)
    deepest = np.array(np.unravel_index(np.argmax(d), d.shape))
    return idx[own], deepest, idx[mat[..., 3] == 0]


def bead(kind, m, rng):
    """one bead (3,) float64 of the kind on map m"""
    vol = maps()[m]
    n, o, g = M.geometry(vol)
    lam, deep, out = landmarks(m)
    if kind == 'centre':       # a voxel centre, index -1 .. n: both out-of-grid sides
        return centre_of(vol, rng.integers(-1, n + 1))
    if kind == 'half':         # on half-steps k + 1/2, k even and odd, and quarter steps
        return centre_of(vol, rng.integers(-1, n + 1) + np.array(OFFSETS)[rng.integers(0, len(OFFSETS), 3)])
    if kind == 'lamina':       # depth 0, level exactly 1
        return centre_of(vol, lam[rng.integers(0, len(lam))])
    if kind == 'deepest':      # level 0
        return centre_of(vol, deep)
    if kind == 'deep_off':     # off-centre in the deepest voxel, away from its lamina voxel
        e = vol['matrice'][tuple(deep)][:3]
        return centre_of(vol, deep + 0.25 * np.sign(deep - e))
    if kind == 'outside_in_grid':
        return centre_of(vol, out[rng.integers(0, len(out))])
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def population(nbead, S, kinds=KINDS, seed=0):
    """(nbead, S, 3) f32 and the kind of every (bead, structure)"""
    rng = np.random.default_rng(1234 + 1000 * seed + 10 * nbead + S)
    sm = struct_map(S)
    xyz = np.zeros((nbead, S, 3))
    kind = np.empty((nbead, S), object)
    for s in range(S):
        for b in range(nbead):
            kind[b, s] = kinds[(b + s) % len(kinds)]
            xyz[b, s] = bead(kind[b, s], int(sm[s]), rng)
    out = xyz.astype(f32)
    assert np.array_equal(out.astype(f64), xyz)  # exact in float32
    out.setflags(write=False)
    return out, kind


# ---------------------------------------------------------------------------- a tiny run
RUN_IDX = (2, 0, 1, 1, 0, 2, 0)   # volumes_idx: structure s reads map RUN_IDX[s % 7]
RUN_S = 9
RUN_CR = 0.25


def write_run(tmp_path, name_maps=True, nucleolus=True):
    """A small exp_map run in tmp_path: the three sphere maps as nuc0.bin .. nuc2.bin, map 1 again
    as the nucleolus body nucl0.bin, and pop.hss -- two chromosomes, the first with two copies:
    5 + 3 haploid loci, 13 beads, RUN_S structures dealt over the maps through RUN_IDX -- whose
    stored configuration names the maps (or not).  Returns a dict with what was written."""
    import json
    from igm_amd import hss, volume as V
    vols = list(D.maps())
    for m, v in enumerate(vols):
        V.write_volume(str(tmp_path / ('nuc%d.bin' % m)), v)
    V.write_volume(str(tmp_path / 'nucl0.bin'), vols[1])
    smap = np.array([RUN_IDX[s % len(RUN_IDX)] for s in range(RUN_S)], np.int32)
    hap_chrom = np.array([0] * 5 + [1] * 3, np.int32)
    chrom = np.concatenate([hap_chrom, hap_chrom[:5]]).astype(np.int32)
    copy = np.array([0] * 8 + [1] * 5, np.int32)
    copy_ptr = np.array([0, 2, 4, 6, 8, 10, 11, 12, 13], np.int32)
    copy_idx = np.array([0, 8, 1, 9, 2, 10, 3, 11, 4, 12, 5, 6, 7], np.int32)
    rng = np.random.default_rng(77)
    xyz = np.zeros((13, RUN_S, 3))
    for s in range(RUN_S):
        for b in range(13):
            xyz[b, s] = bead(KINDS[(b + s) % len(KINDS)], int(smap[s]), rng)
    xyz = xyz.astype(f32)
    radii = np.linspace(0.125, 0.875, 13).astype(f32)
    env = {'nucleus_shape': 'exp_map', 'nucleus_kspring': 1.0}
    if name_maps:
        env.update({'volume_prefix': str(tmp_path / 'nuc'), 'volumes_idx': list(RUN_IDX)})
    cfg = {'model': {'restraints': {'envelope': env}},
           'restraints': {'DamID': {'contact_range': RUN_CR}, 'nuclDamID': {'contact_range': 0.125}}}
    if nucleolus:
        cfg['model']['restraints']['nucleolus'] = {'nucleus_shape': 'exp_map', 'nucleus_kspring': 1.0,
                                                   'volume_prefix': str(tmp_path / 'nucl'), 'volumes_idx': [0]}
    genome = {'assembly': 'test', 'chroms': np.array([b'chrA', b'chrB'], 'S10'),
              'lengths': np.array([5, 3], np.int32), 'origins': np.zeros(2, np.int32)}
    path = str(tmp_path / 'pop.hss')
    hss.write_hss(path, xyz, radii, hss.index_tree(chrom, copy, copy_ptr, copy_idx), genome=genome,
                  envelope={'shape': 'exp_map', 'volume': f64(1.0), 'params': f64(4000.0)},
                  config_data=json.dumps(cfg))
    return dict(path=path, xyz=xyz, radii=radii, copy_ptr=copy_ptr, copy_idx=copy_idx, vols=vols, smap=smap,
                body=[vols[1]], body_smap=np.zeros(RUN_S, np.int32), cfg=cfg)


def expected_files(run):
    """{relative name: array} of report_population(steps shells, radials, damid, bodies) on
    the run, from the restatement"""
    from igm_amd import report as RP
    cp, ci, S = run['copy_ptr'], run['copy_idx'], run['xyz'].shape[1]
    lev, dep = M.levels(run['xyz'], run['vols'], run['smap'])
    radials = RP.average_copies(M.mean_over_structures(lev), cp, ci)
    ave = np.average(M.shells_of_levels(lev, 5)[0], axis=0)
    edges = np.linspace(0, 1.1, 12)
    vol = M.population_volumes(run['vols'], run['smap'], S, edges)
    ncopy = np.diff(cp)
    thr = [RUN_CR * M.depth_scale(v) for v in run['vols']]
    freq = M.lamina_counts(run['xyz'], run['radii'], cp, ci, run['vols'], run['smap'], thr, 1).astype(f64) / S / ncopy
    bthr = [0.125 * M.depth_scale(v) for v in run['body']]
    bfreq = M.lamina_counts(run['xyz'], run['radii'], cp, ci, run['body'], run['body_smap'], bthr, -1).astype(
        f64) / S / ncopy
    _, bdep = M.levels(run['xyz'], run['body'], run['body_smap'])
    return {'shells/ave_radial.txt': ave, 'radials/radials.txt': radials, 'radials/radials_norm.txt': radials / ave[-1],
            'radials/lamina_depth.txt': RP.average_copies(M.mean_over_structures(dep), cp, ci),
            'radials/density_histo.txt': R_histogram(lev, edges) / np.where(vol > 0, vol, np.nan),
            'damid/output.txt': freq, 'bodies/nucleolus_frequency.txt': bfreq,
            'bodies/nucleolus_distance.txt': -RP.average_copies(M.mean_over_structures(bdep), cp, ci)}


def R_histogram(values, edges):
    import report_ref as R
    return R.histogram(values, edges)


# ---------------------------------------------------------------------------- lamina traps
TRAP_T = 0.125   # of a 0.5 grid step: scaled with the map's grid along y


@functools.lru_cache(maxsize=None)
def lamina_traps(S):
    """(xyz (12, S, 3) f32, T (nmap,) f64).  Every bead of structure s sits in the outermost
    lamina voxel (k, c, c) on the +x axis of its map -- which is its own record -- at the
    centre plus (0, t, 0): depth = t = T[map] exactly.  With the first-copy radius 0.5,
    depth - r == T - 0.5 and -depth - r == -T - 0.5 are exact doubles."""
    sm = struct_map(S)
    T = np.zeros(len(maps()))
    xyz = np.zeros((D.NBEAD, S, 3))
    for m, vol in enumerate(maps()):
        n, o, g = M.geometry(vol)
        c = (n - 1) // 2
        mat = vol['matrice']
        k = max(i for i in range(n[0]) if mat[i, c[1], c[2], 3] and tuple(mat[i, c[1], c[2], :3]) == (i, c[1], c[2]))
        p = centre_of(vol, (k, c[1], c[2]))
        T[m] = TRAP_T * g[1] / 0.5
        p[1] += T[m]
        xyz[:, sm == m] = p
    out = xyz.astype(f32)
    assert np.array_equal(out.astype(f64), xyz)
    out.setflags(write=False)
    return out, T
