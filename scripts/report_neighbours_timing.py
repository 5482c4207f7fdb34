#!/usr/bin/env python3
"""Kernel time of the neighbour census at the production shape, against its yardstick.

    python scripts/report_neighbours_timing.py [--nstruct 1000] [--calls 3] [--cutoff 500]

Builds the synthetic 200 kb population (igm_amd.synthetic.population_200kb), deals two
class labels (and unlabelled beads) at random, and times igm_report_neighbours (nclass = 2,
the chains of report.chain_numbers, min_sep 1, sums and ICP without the census returned)
and igm_contact_map_haploid on the same population in the same run: one warm-up call and
the median of `--calls` timed calls each, as igm_last_kernel_ms -- HIP-event time of the
kernels alone, staging the population is not in it.  "report_neighbours" spans the bound
table, the census kernel and the per-bead sums.  The contact map does half the ordered
pair tests with one counter.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from igm_amd import _lib, evaluation as EV, report as RP, synthetic as syn  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nstruct', type=int, default=1000)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--cutoff', type=float, default=RP.DEFAULT_NEIGHBOUR_CUTOFF)
    a = ap.parse_args()
    t0 = time.time()
    pop = syn.population_200kb(a.nstruct)
    xyz = np.ascontiguousarray(np.asarray(pop['xyz'], np.float32).transpose(1, 0, 2))  # bead-major
    cp, ci = pop['copy_ptr'], pop['copy_idx']
    chain = RP.chain_numbers(pop['chrom'], pop['copy'])
    classes = np.random.default_rng(0).integers(-1, 2, xyz.shape[0]).astype(np.int32)
    ctx = _lib.context(0)
    print('population %s built in %.1f s' % (xyz.shape, time.time() - t0), file=sys.stderr, flush=True)

    last = {}

    def neighbours():
        last['res'] = RP.neighbour_census(xyz, a.cutoff, chain, classes, 2, want_census=False, ctx=ctx)

    calls = {'report_neighbours': neighbours,
             'contact_map': lambda: EV.haploid_counts(xyz, pop['radii'], 2.0, cp, ci, ctx=ctx)}
    ms, runs = {}, {}
    for name, fn in calls.items():
        times = []
        for k in range(a.calls + 1):
            fn()
            if k:  # the first call warms up (workspace allocation, code load)
                times.append(ctx.kernel_ms(name))
        ms[name], runs[name] = float(np.median(times)), [round(t, 2) for t in times]
        print('%s %s' % (name, runs[name]), file=sys.stderr, flush=True)
    n, S = xyz.shape[:2]
    print(json.dumps({'nbead': int(n), 'nstruct': int(S), 'nclass': 2, 'cutoff': a.cutoff, 'calls': a.calls,
                      'kernel_ms': ms, 'runs_ms': runs, 'ordered_pair_tests': float(n) * n * S,
                      'mean_neighbours': float(last['res']['sums'].sum()) / (n * S),
                      'neighbours_over_contact_map': ms['report_neighbours'] / ms['contact_map']}))


if __name__ == '__main__':
    main()
