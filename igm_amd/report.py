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
  report_population    -- the numeric files bin/igm-report leaves in its output directory
                          (names and formats of the reference); plots, images and the HTML
                          page stay with the reference

    python -m igm_amd.report HSS [-c CONFIG] [-l LABEL] [--semiaxes A B C] [--steps ...] [-o DIR]

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


# ------------------------------------------------------------------ the igm-report driver
def _cfg_get(cfg, path, default=None):
    node = cfg
    for k in path.split('/'):
        if not isinstance(node, dict) or k not in node:
            return default
        node = node[k]
    return node


def parameters_from_config(cfg, basedir='.'):
    """get_parameters_from_igm_config (bin/igm-report:103-128) for the steps built here:
    {'semiaxes' or None, 'shape', 'damid': {'input_profile', 'contact_range'}}.  An exp_map
    nucleus has no semiaxes: the entry stays None instead of the reference's 5000."""
    out = {'semiaxes': None, 'shape': _cfg_get(cfg, 'model/restraints/envelope/nucleus_shape')}
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


def report_population(hss_path, cfg=None, out_dir=None, steps=STEPS, label='', semiaxes=None, ctx=None, device=0):
    """Write the numeric files of bin/igm-report for the population at hss_path into
    out_dir (default: QC_<label or file name> beside it) and return {relative name: path}.

    cfg: an IGM configuration (dict or JSON file); None looks for config_data in the .hss,
    then for igm-config.json beside it (bin/igm-report:236-262).  steps: any of STEPS.
    radials, shells and damid need semiaxes (resolve_semiaxes) and raise ValueError on an
    exp_map nucleus without explicit ones."""
    from .steps import PopulationStore
    steps = tuple(steps.split(',')) if isinstance(steps, str) else tuple(steps)
    unknown = [s for s in steps if s not in STEPS]
    if unknown:
        raise ValueError('unknown report steps %s (known: %s)' % (unknown, ', '.join(STEPS)))
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
    sx = resolve_semiaxes((env_shape, env_params), params, semiaxes)
    needs = [s for s in steps if s in ('radials', 'shells', 'damid')]
    if sx is None and needs:
        raise ValueError('the nucleus is an exp_map (no ellipsoid): the steps %s need explicit semiaxes'
                         % ', '.join(needs))
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
        smean, _, _ = shells(xyz, sx, **kw)
        np.savetxt(path('shells/ave_radial%s.txt' % tag), np.average(smean, axis=0))
    if 'radials' in steps:
        radials = radial_levels(xyz, sx, store.copy_ptr, store.copy_idx, **kw)
        np.savetxt(path('radials/radials%s.txt' % tag), radials)
        counts, edges = radial_density(xyz, sx, **kw)
        volumes = np.array([edges[i + 1]**3 - edges[i]**3 for i in range(len(counts))])
        np.savetxt(path('radials/density_histo%s.txt' % tag), counts / volumes)
        ave = os.path.join(out_dir, 'shells/ave_radial%s.txt' % tag)
        if os.path.isfile(ave):  # normalised with respect to the last shell (report_radials:119-122)
            np.savetxt(path('radials/radials_norm%s.txt' % tag), radials / np.loadtxt(ave)[-1])
    if 'damid' in steps:
        dcfg = params.get('damid') or {}
        freq = lamina_frequency(xyz, store.radii, store.copy_ptr, store.copy_idx, sx,
                                dcfg.get('contact_range', DEFAULT_DAMID_CONTACT_RANGE), **kw)
        np.savetxt(path('damid/output.txt'), freq)
        if dcfg.get('input_profile'):
            profile = np.loadtxt(dcfg['input_profile'], dtype='float32')
            np.savetxt(path('damid/input%s.txt' % tag), profile)
            np.savetxt(path('damid/pearsonr%s.txt' % tag), pearson(profile, freq))
    if 'distance_map' in steps:
        np.save(path('distance_map/average%s.npy' % tag),
                average_distance_map(xyz, store.copy_ptr, store.copy_idx, store.hap_chrom, **kw))
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
    a = ap.parse_args(argv)
    if not os.path.isfile(a.hss):
        ap.error('Cannot find file %s' % a.hss)
    written = report_population(a.hss, cfg=a.config, out_dir=a.out_dir, steps=a.steps, label=a.label,
                                semiaxes=a.semiaxes)
    for rel in sorted(written):
        print(written[rel])
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
