#!/usr/bin/env python3
"""Kernel times of the seeded nuclear bodies at the production shape.

    python scripts/report_bodies_timing.py [--nstruct 1000] [--calls 3] [--fraction 0.1]

Builds the synthetic 200 kb population (igm_amd.synthetic.population_200kb), flags a random
tenth of the haploid loci as seeds (all copies: report.seed_beads) and times
igm_report_seed_bodies (report.seed_bodies at the default link cutoff and body size, labels
not returned) and igm_report_body_features on the bodies it found (report.body_features,
the per-bead sums without the nearest plane), with igm_report_neighbours (nclass = 0, sums
and ICP without the census returned) on the same population in the same run beside them for
scale: one warm-up call and the median of `--calls` timed calls each, as igm_last_kernel_ms
-- HIP-event time of the kernels alone, staging the population is not in it.  There is no
bar: these are the first times of these kernels.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from igm_amd import _lib, report as RP, synthetic as syn  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nstruct', type=int, default=1000)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--fraction', type=float, default=0.1)
    a = ap.parse_args()
    t0 = time.time()
    pop = syn.population_200kb(a.nstruct)
    xyz = np.ascontiguousarray(np.asarray(pop['xyz'], np.float32).transpose(1, 0, 2))  # bead-major
    cp, ci = pop['copy_ptr'], pop['copy_idx']
    flags = (np.random.default_rng(0).random(len(cp) - 1) < a.fraction).astype(np.int64)
    seeds = RP.seed_beads(flags, cp, ci)
    chain = RP.chain_numbers(pop['chrom'], pop['copy'])
    ctx = _lib.context(0)
    print('population %s, %d seeds, built in %.1f s' % (xyz.shape, len(seeds), time.time() - t0), file=sys.stderr,
          flush=True)

    last = {}

    def bodies():
        last['bodies'] = RP.seed_bodies(xyz, seeds, want_labels=False, ctx=ctx)

    def features():
        last['features'] = RP.body_features(xyz, last['bodies']['nbody'], last['bodies']['centre'], ctx=ctx)

    calls = {'report_seed_bodies': bodies, 'report_body_features': features,
             'report_neighbours': lambda: RP.neighbour_census(xyz, RP.DEFAULT_NEIGHBOUR_CUTOFF, chain,
                                                              want_census=False, ctx=ctx)}
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
    nbody, size = last['bodies']['nbody'], last['bodies']['size']
    print(json.dumps({'nbead': int(n), 'nstruct': int(S), 'nseed': int(len(seeds)), 'calls': a.calls,
                      'link_cutoff': RP.DEFAULT_LINK_CUTOFF, 'min_body_size': RP.DEFAULT_MIN_BODY_SIZE,
                      'kernel_ms': ms, 'runs_ms': runs, 'seed_pair_tests': float(len(seeds)) * (len(seeds) - 1) / 2 * S,
                      'bead_body_distances': float(n) * float(nbody.sum()),
                      'mean_bodies': float(nbody.mean()), 'max_bodies': int(nbody.max()),
                      'mean_body_size': float(size.sum()) / max(int(nbody.sum()), 1),
                      'mean_association': float(last['features']['assoc'].mean()) / S}))


if __name__ == '__main__':
    main()
