#!/usr/bin/env python3
"""Times of the Hi-C report step.

    python scripts/report_hic_timing.py [--calls 5] [--nstruct 1000] [--skip-200kb]

Part 1, the demo population (1558 haploid loci, 100 structures) against the committed demo
Hi-C entries (tests/golden/demo_hic_pairs.npz, p >= 0.02): the contact map
(igm_contact_map_haploid), the comparison (igm_report_hic, both histograms) and the NumPy /
scipy dense restatement of the comparison (tests/report_hic_ref.py: dense x and y, masks,
pearsonr per population, two np.histogram2d) -- medians of `--calls` runs after one warm-up
call; GPU entries as HIP-event time of the kernels (igm_last_kernel_ms; for report_hic from
the first kernel to the last, the two host reads of the integer statistics in between
included) and as wall time of the Python call with host arrays (staging included).

Part 2, 200 kb x `--nstruct` on the synthetic population (igm_amd.synthetic.population_200kb)
with the synthetic sparse matrix (synthetic.hic_pairs_200kb at sigma 1e-3): the two GPU
parts only.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from igm_amd import _lib, evaluation as EV, report as RP, synthetic as syn  # noqa: E402


def csr(i, j, p, nhap):
    order = np.lexsort((j, i))
    indptr = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=nhap))]).astype(np.int64)
    return {'indptr': indptr, 'indices': np.ascontiguousarray(j[order], np.int32),
            'data': np.ascontiguousarray(p[order], np.float32)}


def timed(fn, calls, ctx=None, name=None):
    """(median wall ms, median kernel ms or None) of `calls` runs after one warm-up"""
    wall, kern = [], []
    for k in range(calls + 1):
        t0 = time.perf_counter()
        fn()
        dt = (time.perf_counter() - t0) * 1e3
        if k:
            wall.append(dt)
            if name:
                kern.append(ctx.kernel_ms(name))
    return float(np.median(wall)), float(np.median(kern)) if name else None


def gpu_parts(ctx, xyz, radii, cp, ci, hc, matrix, calls):
    S = xyz.shape[1]
    le, li = RP.hic_edges()
    counts = EV.haploid_counts(xyz, radii, 2.0, cp, ci, ctx=ctx)
    out = {}
    w, k = timed(lambda: EV.haploid_counts(xyz, radii, 2.0, cp, ci, ctx=ctx), calls, ctx, 'contact_map')
    out['contact_map'] = {'wall_ms': w, 'kernel_ms': k}
    w, k = timed(lambda: RP.hic_statistics(counts, S, matrix, hc, 0.05, 0.02, le, li, ctx=ctx), calls, ctx,
                 'report_hic')
    out['report_hic'] = {'wall_ms': w, 'kernel_ms': k}
    return counts, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--nstruct', type=int, default=1000)
    ap.add_argument('--skip-200kb', action='store_true')
    a = ap.parse_args()
    ctx = _lib.context(0)
    res = {'calls': a.calls}

    import report_hic_ref as R
    pop = np.load(os.path.join(ROOT, 'tests', 'golden', 'demo_population.npz'))
    pairs = np.load(os.path.join(ROOT, 'tests', 'golden', 'demo_hic_pairs.npz'))
    cp, ci, hc = pop['copy_ptr'], pop['copy_idx'], pop['hap_chrom']
    nhap = len(hc)
    matrix = csr(pairs['i'].astype(np.int64), pairs['j'].astype(np.int64), pairs['p'], nhap)
    xyz = np.ascontiguousarray(pop['coordinates'], np.float32)
    counts, demo = gpu_parts(ctx, xyz, pop['radii'], cp, ci, hc, matrix, a.calls)
    le, li = RP.hic_edges()

    def restatement():
        x, y = R.dense_input(matrix, nhap), R.probabilities(counts, xyz.shape[1])
        R.correlations(x, y, hc, 0.05, 0.02)
        R.histogram(x, y, le, le)
        R.histogram(x, y, li, li)

    demo['numpy_restatement'] = {'wall_ms': timed(restatement, a.calls)[0]}
    demo.update(nhap=nhap, nstruct=int(xyz.shape[1]), nnz=int(matrix['indptr'][-1]))
    res['demo'] = demo
    print('demo %s' % json.dumps(demo), file=sys.stderr, flush=True)

    if not a.skip_200kb:
        t0 = time.time()
        big = syn.population_200kb(a.nstruct)
        xyz = np.ascontiguousarray(np.asarray(big['xyz'], np.float32).transpose(1, 0, 2))  # bead-major
        nhap = len(big['hap_chrom'])
        i, j, p = syn.hic_pairs_200kb(1e-3)
        matrix = csr(i.astype(np.int64), j.astype(np.int64), p, nhap)
        print('200 kb inputs built in %.0f s' % (time.time() - t0), file=sys.stderr, flush=True)
        _, out = gpu_parts(ctx, xyz, big['radii'], big['copy_ptr'], big['copy_idx'], big['hap_chrom'], matrix,
                           min(a.calls, 3))
        out.update(nhap=nhap, nstruct=int(xyz.shape[1]), nnz=int(matrix['indptr'][-1]))
        res['200kb'] = out
    print(json.dumps(res))


if __name__ == '__main__':
    main()
