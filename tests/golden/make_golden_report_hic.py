#!/usr/bin/env python3
"""Generate tests/golden/report_hic_golden.npz by running the REFERENCE's report_hic
(bonimba87/igm, igm/report/hic.py) and its histogram functions (igm/report/plots.py) on a
sub-matrix of the demo Hi-C input and the demo population.

Run only where the reference tree is present (it is not on the GPU box):

    python tests/golden/make_golden_report_hic.py

The reference modules hic, plots and utils are loaded from their files under a bare
`igm.report` package.  `alabtools` is a stub written to a temporary directory:

  Contactmatrix   a dense symmetric wrapper (the input in float32, as the .hcs stores it)
                  with .matrix.toarray(), .matrix.data, __getitem__(chrom name), toarray(),
                  getInterMask() and a no-op save()
  HssFile         exposing genome.chroms
  analysis.get_simulated_hic   returning the map tests/report_hic_ref.py builds from
                  demo_population.npz: contact counts / nstruct clipped to [0, 1], float64
  plots.plot_comparison, red   no-ops

What alabtools itself computes is therefore this project's statement (unpinned): the
symmetric-with-diagonal reading of toarray(), the clip, the '<=' of the contact test and
float64 for the simulated map (scipy's pearsonr then works in float64).  What report_hic
does with those matrices is the reference's own code: the masks, which entries go to which
pearsonr, the file formats, the histogram orientation and edges.  Nothing from the
reference is written into the repository except the numbers and strings below.

Stored:
  loci, hap_chrom, chrom_names   the chosen haploid loci of the demo population (the whole
                  chromosomes chr19 .. chr22, chrX, chrY: 221 loci) and their names
  indptr, indices, data          the sub-matrix of demo/WTC11_HiC_2Mb.hcs on those loci
  contact_range, intra_sigma, inter_sigma
  intra_text, inter_text         the two correlation files report_hic wrote with both sigmas
  inter_only_intra_text, inter_only_inter_text   the same with intra_sigma = None
  no_sigma_files                 the files report_hic wrote with both sigmas None (none: it
                  returns early)
  log_hist (100, 100), lin_hist (99, 99) int64   the interior (unpadded) of the q arrays of
                  logloghist2d and density_histogram_2d called as report_hic calls them but
                  with smooth=None
  log_edges, lin_edges           the edges those calls returned
  numpy_version, scipy_version
"""
import importlib.util
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('IGM_REFERENCE', '/root/reference')
CONTACT_RANGE = 2.0
INTRA_SIGMA = 0.05
INTER_SIGMA = 0.02
CHROMS = (18, 19, 20, 21, 22, 23)

STUB_INIT = '''
import numpy as np

MATRICES = {}      # name -> (dense symmetric matrix, hap_chrom ids, {chrom name: id})
GENOMES = {}       # hss name -> list of chromosome names


class _Matrix(object):
    def __init__(self, dense):
        self._dense = dense
        self.data = dense.ravel()  # a view: assignments through .data reach the matrix

    def toarray(self):
        return self._dense


class Contactmatrix(object):
    def __init__(self, src):
        dense, self._chrom, self._names = MATRICES[src] if isinstance(src, str) else src
        self.matrix = _Matrix(np.array(dense))

    def __getitem__(self, name):
        sel = np.flatnonzero(self._chrom == self._names[name])
        return Contactmatrix((self.matrix.toarray()[np.ix_(sel, sel)], self._chrom[sel], self._names))

    def toarray(self):
        return self.matrix.toarray()

    def getInterMask(self):
        return self._chrom[:, None] != self._chrom[None, :]

    def save(self, path):
        pass


class _Genome(object):
    def __init__(self, chroms):
        self.chroms = chroms


class HssFile(object):
    def __init__(self, fname, mode='r'):
        self.genome = _Genome(GENOMES[fname])

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False
'''
STUB_ANALYSIS = '''
from . import Contactmatrix, MATRICES


def get_simulated_hic(hssfname, contact_range):
    assert MATRICES[hssfname + ':range'] == contact_range
    return Contactmatrix(hssfname + ':out')
'''
STUB_PLOTS = '''
import matplotlib.pyplot as plt

red = None


def plot_comparison(*a, **k):
    return plt.figure()
'''


def load_reference(tmp):
    stub = os.path.join(tmp, 'stubs', 'alabtools')
    os.makedirs(stub)
    for name, text in (('__init__.py', STUB_INIT), ('analysis.py', STUB_ANALYSIS), ('plots.py', STUB_PLOTS)):
        with open(os.path.join(stub, name), 'w') as f:
            f.write(text)
    sys.path.insert(0, os.path.dirname(stub))
    for name, path in (('igm', os.path.join(REF, 'igm')), ('igm.report', os.path.join(REF, 'igm', 'report'))):
        pkg = types.ModuleType(name)
        pkg.__path__ = [path]
        sys.modules[name] = pkg
    mods = {}
    for m in ('utils', 'plots', 'hic'):
        spec = importlib.util.spec_from_file_location('igm.report.' + m, os.path.join(REF, 'igm', 'report', m + '.py'))
        mod = importlib.util.module_from_spec(spec)
        sys.modules['igm.report.' + m] = mod
        spec.loader.exec_module(mod)
        mods[m] = mod
    return mods


def read(path):
    return open(path).read() if os.path.exists(path) else None


def main():
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    import numpy as np
    import scipy
    tmp = tempfile.mkdtemp(prefix='igm_report_hic_golden_')
    ref = load_reference(tmp)
    import alabtools
    root = os.path.dirname(os.path.dirname(HERE))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.dirname(HERE))
    import report_hic_ref as R
    from igm_amd import hss

    pop = dict(np.load(os.path.join(HERE, 'demo_population.npz')))
    full = hss.read_hcs(os.path.join(REF, 'demo', 'WTC11_HiC_2Mb.hcs'))
    assert np.array_equal(full['chrom'], pop['hap_chrom'])
    loci = np.flatnonzero(np.isin(pop['hap_chrom'], CHROMS))
    hc = pop['hap_chrom'][loci].astype(np.int32)
    sub = R.sub_matrix(full, loci)
    spop = R.sub_population(pop, loci)
    nstruct = spop['coordinates'].shape[1]
    counts = R.contact_counts(spop['coordinates'], spop['radii'], CONTACT_RANGE, spop['copy_ptr'], spop['copy_idx'])
    x = R.dense_input(sub)
    y = R.probabilities(counts, nstruct)
    with hss.h5.File(os.path.join(REF, 'demo', 'WTC11_HiC_2Mb.hcs')) as f:
        all_names = [c.decode() if isinstance(c, bytes) else str(c) for c in f.read('genome/chroms')]
    names = [all_names[c] for c in CHROMS]
    name_id = {all_names[c]: c for c in CHROMS}

    # the finiteness condition on the inputs: no golden correlation is NaN
    for c in CHROMS:
        blk = x[np.ix_(hc == c, hc == c)]
        assert len(np.unique(blk[blk >= INTRA_SIGMA])) >= 2 and len(np.unique(blk[blk < INTRA_SIGMA])) >= 2, c
    inter = np.triu(hc[:, None] != hc[None, :])
    assert len(np.unique(x[inter & (x >= INTER_SIGMA)])) >= 2 and len(np.unique(x[inter & (x < INTER_SIGMA)])) >= 2

    alabtools.MATRICES['input'] = (x, hc, name_id)
    alabtools.MATRICES['demo:out'] = (y, hc, name_id)
    alabtools.MATRICES['demo:range'] = CONTACT_RANGE
    alabtools.GENOMES['demo'] = names

    out = {'loci': loci.astype(np.int32), 'hap_chrom': hc, 'chrom_names': np.array(names),
           'indptr': sub['indptr'], 'indices': sub['indices'], 'data': sub['data'],
           'contact_range': np.float64(CONTACT_RANGE), 'intra_sigma': np.float64(INTRA_SIGMA),
           'inter_sigma': np.float64(INTER_SIGMA), 'numpy_version': np.array(np.__version__),
           'scipy_version': np.array(scipy.__version__)}

    def run(tag, inter_sigma, intra_sigma):
        d = os.path.join(tmp, tag)
        os.makedirs(d)
        os.chdir(d)
        ref['hic'].report_hic('demo', 'input', inter_sigma, intra_sigma, CONTACT_RANGE)
        plt.close('all')
        files = sorted(os.listdir('matrix_comparison')) if os.path.isdir('matrix_comparison') else []
        return (read('matrix_comparison/intra_correlations.txt'), read('matrix_comparison/inter_correlations.txt'),
                [f for f in files if f.endswith('.txt')])

    out['intra_text'], out['inter_text'], _ = (np.array(v) if isinstance(v, str) else v
                                               for v in run('both', INTER_SIGMA, INTRA_SIGMA))
    a, b, _ = run('inter_only', INTER_SIGMA, None)
    out['inter_only_intra_text'], out['inter_only_inter_text'] = np.array(a), np.array(b)
    _, _, files = run('none', None, None)
    out['no_sigma_files'] = np.array(files, dtype='U64')
    assert 'nan' not in str(out['intra_text']) and 'nan' not in str(out['inter_text'])
    print(out['intra_text'], out['inter_text'], out['inter_only_intra_text'], out['inter_only_inter_text'], files,
          sep='\n')

    cm, om = alabtools.Contactmatrix('input'), alabtools.Contactmatrix('demo:out')
    os.chdir(tmp)
    for key, fn in (('log', ref['plots'].logloghist2d), ('lin', ref['plots'].density_histogram_2d)):
        _, _, q, e1, e2 = fn(cm.matrix.toarray().ravel(), om.matrix.toarray().ravel(), bins=(100, 100), outfile=None,
                             nlevels=10, sigma=min(INTRA_SIGMA, INTER_SIGMA), xlabel='INPUT', ylabel='OUTPUT',
                             smooth=None)
        plt.close('all')
        h = q[1:-1, 1:-1]
        assert np.array_equal(h, np.rint(h)) and np.array_equal(e1, e2)
        out[key + '_hist'] = h.astype(np.int64)
        out[key + '_edges'] = e1
        print(key, h.shape, int(h.sum()))
    path = os.path.join(HERE, 'report_hic_golden.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
