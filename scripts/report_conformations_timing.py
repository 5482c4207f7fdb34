#!/usr/bin/env python3
"""Kernel times of the pairwise conformation RMSD at the production shape.

    python scripts/report_conformations_timing.py [--nstruct 1000] [--calls 3]

Builds the synthetic 200 kb population (igm_amd.synthetic.population_200kb) and times
igm_report_conformations (report.conformation_rmsd with the default histogram edges, the
matrix not returned) on chromosome 1 alone -- with the matrix returned beside it -- and on
all chromosomes one after the other: one warm-up pass and the median of `--calls` timed
passes, as igm_last_kernel_ms -- HIP-event time of the three kernels of a call, staging the
population and copying the matrix back are not in it.  Beside them the wall clock of the
NumPy restatement (tests/report_conformations_ref.py) on one small group, 200 loci of 64
conformations, scaled by pairs x loci to chromosome 1 and to the genome: an EXTRAPOLATION,
nobody ran NumPy on the full shape.  There is no bar: these are the first times of this
kernel.  Prints one JSON line.
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

import report_conformations_ref as C  # noqa: E402
from igm_amd import _lib, report as RP, synthetic as syn  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nstruct', type=int, default=1000)
    ap.add_argument('--calls', type=int, default=3)
    a = ap.parse_args()
    t0 = time.time()
    pop = syn.population_200kb(a.nstruct)
    xyz = np.ascontiguousarray(np.asarray(pop['xyz'], np.float32).transpose(1, 0, 2))  # bead-major
    ids = np.unique(pop['chrom'])
    groups = [RP.conformation_beads(pop['chrom'], pop['copy'], pop['copy_ptr'], pop['copy_idx'], cid) for cid in ids]
    S = xyz.shape[1]
    edges = RP.rmsd_edges_of()
    ctx = _lib.context(0)
    print('population %s, %d chromosomes, built in %.1f s' % (xyz.shape, len(ids), time.time() - t0), file=sys.stderr,
          flush=True)

    def one(beads, want_matrix=False):
        out = RP.conformation_rmsd(xyz, beads, edges, want_matrix=want_matrix, ctx=ctx)
        return ctx.kernel_ms('report_conformations'), out

    runs = {'chr1': [], 'chr1_with_matrix': [], 'genome': []}
    per_chrom = None
    for k in range(a.calls + 1):  # the first pass warms up (workspace allocation, code load)
        t1 = one(groups[0])[0]
        t1m = one(groups[0], True)[0]
        each = [one(b)[0] for b in groups]
        if k:
            runs['chr1'].append(t1)
            runs['chr1_with_matrix'].append(t1m)
            runs['genome'].append(float(np.sum(each)))
            per_chrom = each
    ms = {name: float(np.median(v)) for name, v in runs.items()}
    for name in runs:
        print('%s %s' % (name, [round(t, 2) for t in runs[name]]), file=sys.stderr, flush=True)
    summary = RP.conformation_summary(one(groups[0])[1], S)

    def work(beads):
        M = beads.shape[0] * S
        return M * (M - 1) / 2.0, beads.shape[1]

    pair_loci = [p * n for p, n in (work(b) for b in groups)]
    # the restatement on 200 loci x 64 conformations of chromosome 1
    small = groups[0][:1, :200]
    sub = np.ascontiguousarray(xyz[:, :64])
    t0 = time.time()
    C.conformations(sub, small, edges)
    numpy_s = time.time() - t0
    per = numpy_s / (64 * 63 / 2.0 * small.shape[1])
    print(json.dumps({'nbead': int(xyz.shape[0]), 'nstruct': int(S), 'calls': a.calls,
                      'chr1': {'nlocus': int(groups[0].shape[1]), 'ncopy': int(groups[0].shape[0]),
                               'M': int(groups[0].shape[0] * S), 'pairs': work(groups[0])[0],
                               'mean_rmsd': summary['mean'], 'variability': summary['variability']},
                      'kernel_ms': ms, 'runs_ms': {k: [round(t, 2) for t in v] for k, v in runs.items()},
                      'per_chromosome_ms': [round(t, 2) for t in per_chrom],
                      'genome_pair_loci': float(np.sum(pair_loci)),
                      'genome_fp64_fma': 9.0 * float(np.sum(pair_loci)),
                      'numpy_small_group_s': numpy_s,
                      'numpy_extrapolated_s': {'chr1': per * pair_loci[0], 'genome': per * float(np.sum(pair_loci))},
                      'numpy_note': 'extrapolated from 200 loci x 64 conformations by pairs x loci, not measured'}))


if __name__ == '__main__':
    main()
