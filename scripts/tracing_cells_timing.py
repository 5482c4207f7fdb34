#!/usr/bin/env python3
"""Time of the joint placement of imaged cells at the production shape.

    python scripts/tracing_cells_timing.py [--nstruct 1000] [--ncell 200] [--nspots 50]
                                           [--keep-best 50] [--calls 3] [--oracle-cells 2]
                                           [--round-caps 0,1,2,4,8]

Builds the synthetic 200 kb population (igm_amd.synthetic.population_200kb), plants `--ncell`
cells on it (igm_amd.workloads.synthetic_cells: one window of `--nspots` spots on every
chromosome copy, 46 traces per cell, 20 nm noise), makes one warm-up call of
igm_amd.tracing.assign_cell_costs and `--calls` timed ones, and prints one JSON line: the median
HIP-event times of the three kernels (igm_last_kernel_ms), the wall clock around the call
(staging the population included), the algorithmic bytes of the sums kernel (12 B per bead read,
104 B per record written) and of the search kernel (104 B per record read: every trace once per
joint fit, every (trace, copy) once at the start and once per round), the share of planted cells
and labels recovered, the rounds histogram; from the same session igm_amd.tracing.assign_costs on
the same traces taken as independent ones, and the fp64 NumPy oracle (tests/tracing_cells.py) on
the first `--oracle-cells` cells scaled linearly to all.  `--round-caps` times the search kernel
again with its rounds cut short (IGM_TRACING_CELL_ROUNDS): cap 0 is the start and one joint fit,
the differences are the cost of a round.
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
REC = 13 * 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nstruct', type=int, default=1000)
    ap.add_argument('--ncell', type=int, default=200)
    ap.add_argument('--nspots', type=int, default=50)
    ap.add_argument('--keep-best', type=int, default=50)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--oracle-cells', type=int, default=2)
    ap.add_argument('--round-caps', default='', help='e.g. 0,1,2,4: the search kernel with IGM_TRACING_CELL_ROUNDS set')
    a = ap.parse_args()
    t0 = time.time()
    pop = syn.population_200kb(a.nstruct)
    xyz = np.ascontiguousarray(np.asarray(pop['xyz'], np.float32).transpose(1, 0, 2))  # bead-major
    print('population %s built in %.1f s' % (xyz.shape, time.time() - t0), file=sys.stderr, flush=True)
    t0 = time.time()
    tr, s, k = W.synthetic_cells(pop, xyz, a.ncell, a.nspots, 20.0, 1)
    tr = T.check_traces(tr, pop['copy_ptr'], pop['hap_chrom'])
    ntrace = len(tr['ncopy'])
    print('%d cells (%d traces) planted in %.1f s' % (a.ncell, ntrace, time.time() - t0), file=sys.stderr, flush=True)
    ctx = _lib.context(0)
    names = ('tracing_cell_sums', 'tracing_cell_search', 'tracing_cell_select')
    ms, wall = {q: [] for q in names}, []
    for c in range(a.calls + 1):
        t0 = time.time()
        bs, bv, bl, cost, label, rounds = T.assign_cell_costs(xyz, pop['copy_ptr'], pop['copy_idx'], tr, a.keep_best,
                                                              ctx=ctx, return_full=True)
        if c:  # the first call warms up (workspace allocation, code load)
            wall.append(time.time() - t0)
            for q in names:
                ms[q].append(ctx.kernel_ms(q))
        print('call %d: %s, wall %.2f s' % (c, ', '.join('%s %.2f ms' % (q, ctx.kernel_ms(q)) for q in names),
                                            time.time() - t0), file=sys.stderr, flush=True)
    pick = T.greedy_cell_assignment(bs, bv)
    cell = np.repeat(np.arange(a.ncell), np.diff(tr['cell_ptr']))
    hit = (pick >= 0) & (bs[np.arange(a.ncell), np.maximum(pick, 0)] == s)
    lab = bl[np.arange(ntrace), np.maximum(pick, 0)[cell]]
    nrec = float(np.sum(tr['ncopy'])) * a.nstruct  # records
    fits = rounds.astype(np.float64)  # joint fits per (cell, structure): one per round (+ 1 at the cap)
    per_cell = np.add.reduceat(tr['ncopy'].astype(np.float64), tr['cell_ptr'][:-1])
    search_bytes = REC * float(np.sum(fits * np.diff(tr['cell_ptr'])[:, None]) + np.sum((1.0 + fits) * per_cell[:, None]))
    sums_bytes = 12.0 * a.nspots * nrec + REC * nrec
    med = {q: float(np.median(v)) for q, v in ms.items()}
    out = {'nbead': int(xyz.shape[0]), 'nstruct': a.nstruct, 'ncell': a.ncell, 'ntrace': ntrace, 'nspots': a.nspots,
           'keep_best': a.keep_best, 'calls': a.calls, 'sums_ms': med[names[0]], 'search_ms': med[names[1]],
           'select_ms': med[names[2]], 'wall_s': float(np.median(wall)),
           'sums_GB': sums_bytes / 1e9, 'sums_TBs': sums_bytes / (med[names[0]] * 1e-3) / 1e12,
           'search_GB': search_bytes / 1e9, 'search_TBs': search_bytes / (med[names[1]] * 1e-3) / 1e12,
           'search_fraction_of_hbm': search_bytes / (med[names[1]] * 1e-3) / 1e12 / HBM_TBS,
           'eigen_solves': float(np.sum(per_cell) * a.nstruct + np.sum(fits)),
           'rounds_histogram': np.bincount(rounds.reshape(-1), minlength=17).tolist(),
           'cells_recovered': float(np.mean(hit)), 'labels_recovered': float(np.mean(lab[hit[cell]] == k[hit[cell]]))}
    for c in range(2):  # (a warm-up, then the timed call)
        T.assign_costs(xyz, pop['copy_ptr'], pop['copy_idx'], tr, a.keep_best, ctx=ctx)
    out.update({'independent_cost_ms': ctx.kernel_ms('tracing_cost'), 'independent_select_ms': ctx.kernel_ms('tracing_select')})
    for cap in [int(q) for q in a.round_caps.split(',') if q]:
        # the search cut short: cap 0 is the start and one joint fit, every further round adds one pass over
        # the records and one 4x4 eigen-solve per (cell, structure)
        os.environ['IGM_TRACING_CELL_ROUNDS'] = str(cap)
        t = []
        for c in range(3):
            T.assign_cell_costs(xyz, pop['copy_ptr'], pop['copy_idx'], tr, a.keep_best, ctx=ctx)
            t.append(ctx.kernel_ms('tracing_cell_search'))
        out['search_ms_rounds_cap_%d' % cap] = float(np.median(t[1:]))
    os.environ.pop('IGM_TRACING_CELL_ROUNDS', None)
    if a.oracle_cells > 0:
        import tracing_cells as TC
        import types
        n = min(a.oracle_cells, a.ncell)
        ix = types.SimpleNamespace(copy_ptr=pop['copy_ptr'], copy_idx=pop['copy_idx'], hap_chrom=pop['hap_chrom'])
        t0 = time.time()
        o = TC.cells_oracle(xyz, ix, T.slice_cells(tr, 0, n))
        dt = time.time() - t0
        err = np.abs(cost[:n].astype(np.float64) - o['cost'])
        out.update({'oracle_cells': n, 'oracle_s': dt, 'oracle_s_scaled': dt * a.ncell / n,
                    'oracle_max_rel_err': float((err / np.maximum(o['cost'], 1e-9)).max()),
                    'oracle_labels_equal': float(np.mean(label[:tr['cell_ptr'][n]] == o['label']))})
    print(json.dumps(out))


if __name__ == '__main__':
    main()
