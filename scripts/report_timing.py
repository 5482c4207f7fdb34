#!/usr/bin/env python3
"""Kernel times of the population report at the production shape.

    python scripts/report_timing.py [--nstruct 1000] [--calls 3] [--resolution 200000]

Builds the synthetic 200 kb population (igm_amd.synthetic.population_200kb), makes one
warm-up call and `--calls` timed calls per entry point and prints one JSON line with the
median igm_last_kernel_ms of each: report_levels (levels + density + five shells),
report_rg, report_lamina, report_distance_map, and -- the yardstick, the same tile
traversal over the same population -- contact_map (igm_contact_map_haploid).  The times
are HIP-event times of the kernels alone: staging the population is not in them.
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
    ap.add_argument('--resolution', type=int, default=200000)
    a = ap.parse_args()
    t0 = time.time()
    if a.resolution == 200000:
        pop = syn.population_200kb(a.nstruct, semiaxes=syn.ELLIPSOID_D)
    else:
        pop = syn.population_2mb(a.nstruct)
    xyz = np.ascontiguousarray(np.asarray(pop['xyz'], np.float32).transpose(1, 0, 2))  # bead-major
    sx = np.asarray(syn.ELLIPSOID_D if a.resolution == 200000 else (5500.0,) * 3, np.float64)
    cp, ci, hc = pop['copy_ptr'], pop['copy_idx'], pop['hap_chrom']
    _, _, chain_ptr, chain_idx = RP.chains(pop['chrom'], pop['copy'])
    ctx = _lib.context(0)
    print('population %s built in %.1f s' % (xyz.shape, time.time() - t0), file=sys.stderr, flush=True)

    def levels():
        RP._levels(xyz, sx, ctx, 0, want_mean=True, density_edges=np.linspace(0, 1.1, 12), nshell=5,
                   shell_edges=np.linspace(0, 1.5, 151))

    calls = {
        'report_levels': levels,
        'report_rg': lambda: RP.chain_rgs(xyz, chain_ptr, chain_idx, ctx=ctx),
        'report_lamina': lambda: RP.lamina_counts(xyz, pop['radii'], cp, ci, sx, 0.05, ctx=ctx),
        'report_distance_map': lambda: RP.average_distance_map(xyz, cp, ci, hc, ctx=ctx),
        'contact_map': lambda: EV.haploid_counts(xyz, pop['radii'], 2.0, cp, ci, ctx=ctx),
    }
    ms = {}
    for name, fn in calls.items():
        times = []
        for k in range(a.calls + 1):
            fn()
            if k:  # the first call warms up (workspace allocation, code load)
                times.append(ctx.kernel_ms(name))
        ms[name] = float(np.median(times))
        print('%s %s' % (name, ['%.2f' % t for t in times]), file=sys.stderr, flush=True)
    print(json.dumps({'nbead': int(xyz.shape[0]), 'nstruct': int(xyz.shape[1]), 'nhap': int(len(cp) - 1),
                      'nchain': int(len(chain_ptr) - 1), 'calls': a.calls, 'kernel_ms': ms,
                      'distance_map_over_contact_map': ms['report_distance_map'] / ms['contact_map']}))


if __name__ == '__main__':
    main()
