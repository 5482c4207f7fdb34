#!/usr/bin/env python3
"""Generate tests/golden/report_golden.npz by running the REFERENCE's report functions
(bonimba87/igm, igm/report/*.py) on the demo population.

Run only where the reference tree is present (it is not on the GPU box):

    python tests/golden/make_golden_report.py

NumPy 2.x (the version is recorded in the file: report_damid's snormsq_ellipse divides in
float64 under NumPy 2 promotion, in float32 under NumPy 1.x) and matplotlib (the report
functions draw their figures while they compute; they go to a temporary directory).

The reference modules radials, shells, radius_of_gyration, damid, distance_map and utils
are loaded from their files under a bare `igm.report` package, so igm/__init__.py and its
dependencies are not needed; `alabtools` is a stub written to a temporary directory that
provides HssFile (a view of the arrays of demo_population.npz) and
plots.plot_by_chromosome.  No alabtools arithmetic is involved: the reference functions
only read coordinates, radii and the index through it.  Nothing from the reference is
written into the repository except the numbers below (fixtures = data).

Stored:
  semiaxes, contact_range, numpy_version
  radial_level     get_radial_level(coordinates, index, semiaxes)             (nhap,)
  rgs_values/ptr   radius_of_gyration/chromosomes.npz of report_radius_of_gyration's
                   get_chroms_rgs, one run per chromosome                     (float32 values)
  ave_radial       shells/ave_radial.txt of report_shells                     (5,)
  density_histo    radials/density_histo.txt of plot_radial_density          (11,)
  damid_output     damid/output.txt of report_damid at contact_range 0.05    (nhap,)
  dmap_loci, dmap  create_average_distance_map on the sub-population of those 120 haploid
                   loci (the ends of two autosomes, of the last autosome, chrX and chrY:
                   three chromosome boundaries inside), upper triangle, the rest zeroed
  max_rel_*        the largest relative difference between those numbers and the float64
                   restatement tests/report_ref.py, measured when the file was made
"""
import importlib.util
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('IGM_REFERENCE', '/root/reference')
SEMIAXES = (5488.0, 5499.5, 5390.0)
CONTACT_RANGE = 0.05

STUB_INIT = '''
import numpy as np

POPULATIONS = {}


class Index(object):
    def __init__(self, chrom, copy, copy_ptr, copy_idx):
        self.chrom, self.copy = chrom, copy
        self.copy_index = {h: copy_idx[copy_ptr[h]:copy_ptr[h + 1]] for h in range(len(copy_ptr) - 1)}

    def __len__(self):
        return len(self.chrom)

    def get_chromosomes(self):
        return np.unique(self.chrom)

    def get_chrom_copies(self, chrom):
        return np.unique(self.copy[self.chrom == chrom])

    def get_chrom_pos(self, chrom, copy):
        return np.flatnonzero((self.chrom == chrom) & (self.copy == copy))

    def get_haploid(self):
        return self


class HssFile(object):
    def __init__(self, fname, mode='r'):
        p = POPULATIONS[fname]
        self.coordinates, self.radii, self.index = p['coordinates'], p['radii'], p['index']
        self.nbead, self.nstruct = self.coordinates.shape[0], self.coordinates.shape[1]

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def get_bead_crd(self, i):
        return self.coordinates[i]
'''
STUB_PLOTS = '''
import matplotlib.pyplot as plt


def plot_by_chromosome(*a, **k):
    return plt.figure(), None
'''


def load_reference(tmp):
    stub = os.path.join(tmp, 'stubs', 'alabtools')
    os.makedirs(stub)
    with open(os.path.join(stub, '__init__.py'), 'w') as f:
        f.write(STUB_INIT)
    with open(os.path.join(stub, 'plots.py'), 'w') as f:
        f.write(STUB_PLOTS)
    sys.path.insert(0, os.path.dirname(stub))
    for name, path in (('igm', os.path.join(REF, 'igm')), ('igm.report', os.path.join(REF, 'igm', 'report'))):
        pkg = types.ModuleType(name)
        pkg.__path__ = [path]
        sys.modules[name] = pkg
    mods = {}
    for m in ('utils', 'radials', 'shells', 'radius_of_gyration', 'damid', 'distance_map'):
        spec = importlib.util.spec_from_file_location('igm.report.' + m, os.path.join(REF, 'igm', 'report', m + '.py'))
        mod = importlib.util.module_from_spec(spec)
        sys.modules['igm.report.' + m] = mod
        spec.loader.exec_module(mod)
        mods[m] = mod
    return mods


def sub_population(pop, loci):
    """The population of the haploid loci `loci` in the layout alabtools writes: beads
    0..n-1 are the first copies in locus order, the further copies follow."""
    import numpy as np
    cp, ci = pop['copy_ptr'], pop['copy_idx']
    beads, chrom, copy, rows = [], [], [], [[] for _ in loci]
    maxc = int(np.diff(cp).max())
    for k in range(maxc):
        for q, h in enumerate(loci):
            if cp[h + 1] - cp[h] > k:
                rows[q].append(len(beads))
                beads.append(ci[cp[h] + k])
                chrom.append(pop['hap_chrom'][h])
                copy.append(k)
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    idx = np.array([b for r in rows for b in r], np.int32)
    beads = np.array(beads)
    return {'coordinates': np.ascontiguousarray(pop['coordinates'][beads]), 'radii': pop['radii'][beads],
            'chrom': np.array(chrom, np.int32), 'copy': np.array(copy, np.int32), 'copy_ptr': ptr, 'copy_idx': idx}


def main():
    import matplotlib
    matplotlib.use('Agg')
    import numpy as np
    assert int(np.__version__.split('.')[0]) >= 2, 'report_golden.npz records the NumPy 2 evaluation'
    tmp = tempfile.mkdtemp(prefix='igm_report_golden_')
    ref = load_reference(tmp)
    import alabtools
    sys.path.insert(0, os.path.dirname(HERE))
    import report_ref as R

    pop = dict(np.load(os.path.join(HERE, 'demo_population.npz')))
    crd, cp, ci, hc = pop['coordinates'], pop['copy_ptr'], pop['copy_idx'], pop['hap_chrom']
    nhap = len(cp) - 1
    index = alabtools.Index(pop['chrom'], pop['copy'], cp, ci)
    alabtools.POPULATIONS['demo'] = {'coordinates': crd, 'radii': pop['radii'], 'index': index}
    sx = np.array(SEMIAXES)
    out = {'semiaxes': sx, 'contact_range': np.float64(CONTACT_RANGE), 'numpy_version': np.array(np.__version__)}

    os.chdir(tmp)
    for d in ('radials', 'shells', 'damid'):
        os.makedirs(d)
    out['radial_level'] = ref['radials'].get_radial_level(crd, index, sx)
    ref['radials'].plot_radial_density('demo', sx)
    out['density_histo'] = np.loadtxt('radials/density_histo.txt')
    ref['shells'].report_shells('demo', semiaxes=sx)
    out['ave_radial'] = np.loadtxt('shells/ave_radial.txt')
    rgs = ref['radius_of_gyration'].get_chroms_rgs(crd, index)
    out['rgs_values'] = np.concatenate(rgs)
    out['rgs_ptr'] = np.concatenate([[0], np.cumsum([len(r) for r in rgs])]).astype(np.int64)
    ref['damid'].report_damid('demo', None, CONTACT_RANGE, semiaxes=sx)
    out['damid_output'] = np.loadtxt('damid/output.txt')

    ends = {c: np.flatnonzero(hc == c) for c in (0, 1, 21, 22, 23)}
    loci = np.concatenate([ends[0][-30:], ends[1][:30], ends[21][-20:], ends[22][:20], ends[22][-10:], ends[23][:10]])
    sub = sub_population(pop, loci)
    assert np.array_equal(sub['chrom'][:len(loci)], hc[loci])  # index.chrom[i] is the haploid chromosome
    alabtools.POPULATIONS['sub'] = {'coordinates': sub['coordinates'], 'radii': sub['radii'],
                                    'index': alabtools.Index(sub['chrom'], sub['copy'], sub['copy_ptr'],
                                                             sub['copy_idx'])}
    dmap = np.triu(ref['distance_map'].create_average_distance_map('sub'), 1)
    out['dmap_loci'] = loci.astype(np.int32)
    out['dmap'] = dmap

    # the reference against the float64 restatement
    def rel(a, b):
        return float(np.max(np.abs(a - b) / np.abs(b)))

    lev = R.level_mean(crd, sx)
    mine = np.array([np.nanmean(lev[ci[cp[h]:cp[h + 1]]]) for h in range(nhap)])
    out['max_rel_radial_level'] = np.float64(rel(out['radial_level'], mine))
    _, _, chain_ptr, chain_idx = _chains(pop['chrom'], pop['copy'])
    out['max_rel_rg'] = np.float64(rel(out['rgs_values'].astype(np.float64), R.rg(crd, chain_ptr, chain_idx).ravel()))
    out['max_rel_ave_radial'] = np.float64(rel(out['ave_radial'], R.shells(crd, sx, 5)[0].mean(axis=0)))
    dref = R.distance_map(sub['coordinates'], sub['copy_ptr'], sub['copy_idx'], hc[loci])
    iu = np.triu_indices(len(loci), 1)
    out['max_rel_dmap'] = np.float64(rel(dmap[iu], dref[iu]))
    for k in ('max_rel_radial_level', 'max_rel_rg', 'max_rel_ave_radial', 'max_rel_dmap'):
        print(k, out[k])
    path = os.path.join(HERE, 'report_golden.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


def _chains(chrom, copy):
    import numpy as np
    ptr, idx, ids, cptr = [0], [], np.unique(chrom), [0]
    for c in ids:
        for k in np.unique(copy[chrom == c]):
            ii = np.flatnonzero((chrom == c) & (copy == k))
            idx.append(ii)
            ptr.append(ptr[-1] + len(ii))
        cptr.append(len(ptr) - 1)
    return ids, np.array(cptr), np.array(ptr, np.int32), np.concatenate(idx).astype(np.int32)


if __name__ == '__main__':
    main()
