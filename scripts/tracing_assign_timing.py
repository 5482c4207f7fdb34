#!/usr/bin/env python3
"""Time of the chromatin tracing A-step at the production shape.

    python scripts/tracing_assign_timing.py [--nstruct 1000] [--ntrace 10000] [--nspots 50]
                                            [--keep-best 50] [--calls 3] [--oracle-traces 100]

Builds the synthetic 200 kb population (igm_amd.synthetic.population_200kb), plants
`--ntrace` traces of `--nspots` spots on it (igm_amd.workloads.synthetic_traces, 20 nm noise),
makes one warm-up call of igm_amd.tracing.assign_costs and `--calls` timed ones, and prints one
JSON line: the median HIP-event times of the cost and the selection kernels
(igm_last_kernel_ms), the wall clock around the call (staging the population included), the
algorithmic traffic 12 B * spots * S * C of the cost kernel per second, the share of planted
slots the greedy assignment recovers, and the time of the fp64 NumPy oracle
(tests/tracing_assign.py) on the first `--oracle-traces` traces scaled linearly to all.
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

from igm_amd import _lib, synthetic as syn, tracing as T, workloads as W  # noqa: E402

HBM_TBS = 8.0  # MI355X peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nstruct', type=int, default=1000)
    ap.add_argument('--ntrace', type=int, default=10000)
    ap.add_argument('--nspots', type=int, default=50)
    ap.add_argument('--keep-best', type=int, default=50)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--oracle-traces', type=int, default=100)
    a = ap.parse_args()
    t0 = time.time()
    pop = syn.population_200kb(a.nstruct)
    xyz = np.ascontiguousarray(np.asarray(pop['xyz'], np.float32).transpose(1, 0, 2))  # bead-major
    print('population %s built in %.1f s' % (xyz.shape, time.time() - t0), file=sys.stderr, flush=True)
    t0 = time.time()
    tr, s, k = W.synthetic_traces(pop, xyz, a.ntrace, a.nspots, 20.0, 1)
    tr = T.check_traces(tr, pop['copy_ptr'], pop['hap_chrom'])
    print('%d traces planted in %.1f s' % (a.ntrace, time.time() - t0), file=sys.stderr, flush=True)
    ctx = _lib.context(0)
    cost, select, wall = [], [], []
    for c in range(a.calls + 1):
        t0 = time.time()
        cand, val = T.assign_costs(xyz, pop['copy_ptr'], pop['copy_idx'], tr, a.keep_best, ctx=ctx)
        if c:  # the first call warms up (workspace allocation, code load)
            wall.append(time.time() - t0)
            cost.append(ctx.kernel_ms('tracing_cost'))
            select.append(ctx.kernel_ms('tracing_select'))
        print('call %d: cost %.2f ms, select %.2f ms, wall %.2f s' % (
            c, ctx.kernel_ms('tracing_cost'), ctx.kernel_ms('tracing_select'), time.time() - t0), file=sys.stderr,
            flush=True)
    t0 = time.time()
    pick = T.greedy_assignment(cand, val, tr['chrom'])
    greedy_s = time.time() - t0
    C = int(tr['ncopy'].max())
    took = cand[np.arange(a.ntrace), np.maximum(pick, 0)]
    hit = (pick >= 0) & (took // C == s) & (took % C == k)
    nbytes = 12.0 * a.nspots * a.nstruct * float(np.sum(tr['ncopy']))
    out = {'nbead': int(xyz.shape[0]), 'nstruct': a.nstruct, 'ntrace': a.ntrace, 'nspots': a.nspots,
           'keep_best': a.keep_best, 'calls': a.calls, 'cost_ms': float(np.median(cost)),
           'select_ms': float(np.median(select)), 'wall_s': float(np.median(wall)), 'greedy_s': greedy_s,
           'algorithmic_GB': nbytes / 1e9, 'algorithmic_TBs': nbytes / (np.median(cost) * 1e-3) / 1e12,
           'fraction_of_hbm': nbytes / (np.median(cost) * 1e-3) / 1e12 / HBM_TBS,
           'recovered': float(np.mean(hit)), 'unassigned': int(np.count_nonzero(pick < 0))}
    if a.oracle_traces > 0:
        import tracing_assign as TA
        import types
        n = min(a.oracle_traces, a.ntrace)
        ix = types.SimpleNamespace(copy_ptr=pop['copy_ptr'], copy_idx=pop['copy_idx'])
        t0 = time.time()
        TA.oracle_rmsd(xyz, ix, T.slice_traces(tr, 0, n))
        dt = time.time() - t0
        out.update({'oracle_traces': n, 'oracle_s': dt, 'oracle_s_scaled': dt * a.ntrace / n})
    print(json.dumps(out))


if __name__ == '__main__':
    main()
