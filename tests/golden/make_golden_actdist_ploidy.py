#!/opt/conda/bin/python3.9
"""Golden vectors of the Hi-C A-step on a genome with one to four copies per locus, produced by
running the REFERENCE's own get_actdist (igm/steps/ActivationDistanceStep.py:336-485) and the
'%6d %6d %10.4f %.4f' text round trip of task()/reduce().  Build container only, like
make_golden.py:

    /opt/conda/bin/python3.9 tests/golden/make_golden_actdist_ploidy.py

The genome, populations and (pwish, plast) list are those of tests/astep_edges.py: loci with 1, 2,
3 and 4 copies on two chromosomes.  Every pair the reference defines is run: all inter pairs
(|ii| |jj| combinations, 1..16) and the intra pairs with |ii| <= |jj| (for |ii| > |jj| its d_sq
keeps uninitialised rows).  The existing goldens pin the combination and row order for diploids
only; this file pins 2x3, 3x4, 4x4 and the rest.

The cases are S = 1, 5, 64 and 65 at contact range 2.0, both it_corr values, and one more that
no other golden has: S = 65 at contact range 1.3 (contactRange * (ri + rj) is then not exact).

actdist_ploidy_golden.npz holds
  radii, copy_ptr, copy_idx, chrom     the genome
  pi, pj, pwish, plast                 the pair list (the same for every case)
  cases                                their names, 's<S>_cr<cr>_i<it_corr>'
  s<S>_xyz                             (32, S, 3) f32
  <case>_nrows, _ad64, _p64            per pair: row count, the reference's f64 ad and p (NaN: no rows)
  <case>_row, _col, _dist, _prob       the rows after the text round trip
The file is data only.  It is written with fixed zip time stamps, so the script regenerates it
byte for byte.
"""
import os
import sys
import zipfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden  # noqa: E402  (builds the reference environment)
import numpy as np  # noqa: E402
import astep_edges as E  # noqa: E402

assert np.__version__.startswith('1.')

S_GOLDEN = (1, 5, 64, 65)
CASES = [(S, 2.0) for S in S_GOLDEN] + [(65, 1.3)]


def save_npz(path, arrays):
    """np.savez_compressed with a fixed time stamp on every member"""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for key in arrays:
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, 'w') as fid:
                np.lib.format.write_array(fid, np.asanyarray(arrays[key]), allow_pickle=False)


def main():
    out = {'radii': E.RADII, 'copy_ptr': E.COPY_PTR, 'copy_idx': E.COPY_IDX, 'chrom': E.CHROM}
    ij = E.reference_pairs()
    pi = np.array([a for (a, _) in ij for _ in E.PW_PL], np.int32)
    pj = np.array([b for (_, b) in ij for _ in E.PW_PL], np.int32)
    pw = np.array([w for _ in ij for (w, _) in E.PW_PL], np.float64)
    pl = np.array([l for _ in ij for (_, l) in E.PW_PL], np.float64)
    out.update({'pi': pi, 'pj': pj, 'pwish': pw, 'plast': pl})
    names = []
    for S, cr in CASES:
        xyz, radii = E.population(S)
        out['s%d_xyz' % S] = np.array(xyz)
        hss = make_golden.DuckHss(xyz, radii, E.COPY_INDEX, E.CHROM)
        for it_corr in (0, 1):
            nrows, ad64, p64, rt = make_golden.run_pairs(hss, pi, pj, pw, pl, it_corr, cr=cr)
            tag = 's%d_cr%g_i%d' % (S, cr, it_corr)
            names.append(tag)
            out[tag + '_nrows'] = nrows
            out[tag + '_ad64'] = ad64
            out[tag + '_p64'] = p64
            for k in ('row', 'col', 'dist', 'prob'):
                out[tag + '_' + k] = rt[k]
            # every combination count came out, in the (k in ii, m in jj) / zip(ii, jj) order
            assert sorted(set(nrows.tolist())) == [0] + E.N_SET
            print(tag, len(pi), 'pairs', len(rt), 'rows', flush=True)
    out['cases'] = np.array(names)
    path = os.path.join(HERE, 'actdist_ploidy_golden.npz')
    save_npz(path, out)
    print('actdist_ploidy_golden.npz', os.path.getsize(path))


if __name__ == '__main__':
    main()
