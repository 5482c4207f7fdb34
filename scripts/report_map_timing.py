#!/usr/bin/env python3
"""Kernel times of the report on imaged nuclei at the production shape.

    python scripts/report_map_timing.py [--nstruct 1000] [--calls 3] [--maps 1 8]

Builds the synthetic 200 kb population (igm_amd.synthetic.population_200kb) and, for every
entry of --maps, that many 100 nm sphere maps (117^3 voxels each, their centres a few nm
apart so that every map is its own 25.6 MB table) assigned to the structures cyclically.
One warm-up call and `--calls` timed calls of igm_report_map_levels with all outputs (level
and depth means, the 11-bin density, 5 shells with 150-bin histograms) and of its first pass
alone (no shells), next to igm_report_levels with the same outputs on the same population,
and igm_report_map_lamina next to igm_report_lamina.  Prints one JSON line with the median igm_last_kernel_ms of
each: HIP-event times of the kernels alone, staging is not in them.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from igm_amd import _lib, report as RP, synthetic as syn, volume as V  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nstruct', type=int, default=1000)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--maps', type=int, nargs='+', default=[1, 8])
    a = ap.parse_args()
    t0 = time.time()
    pop = syn.population_200kb(a.nstruct, semiaxes=syn.ELLIPSOID_D)
    xyz = np.ascontiguousarray(np.asarray(pop['xyz'], np.float32).transpose(1, 0, 2))  # bead-major
    sx = np.asarray(syn.ELLIPSOID_D, np.float64)
    cp, ci = pop['copy_ptr'], pop['copy_idx']
    ctx = _lib.context(0)
    print('population %s built in %.1f s' % (xyz.shape, time.time() - t0), file=sys.stderr, flush=True)
    dedges, sedges = np.linspace(0, 1.1, 12), np.linspace(0, 1.5, 151)

    def timed(name, fn):
        times = []
        for k in range(a.calls + 1):
            fn()
            if k:  # the first call warms up (workspace allocation, code load)
                times.append(ctx.kernel_ms(name))
        print('%s %s' % (name, ['%.2f' % t for t in times]), file=sys.stderr, flush=True)
        return float(np.median(times))

    ms = {'report_levels': timed('report_levels', lambda: RP._levels(
        xyz, sx, ctx, 0, want_mean=True, density_edges=dedges, nshell=5, shell_edges=sedges)),
          # pass 1 alone (no shells: the level scratch is not written either)
          'report_levels_pass1': timed('report_levels', lambda: RP._levels(
              xyz, sx, ctx, 0, want_mean=True, density_edges=dedges)),
          'report_lamina': timed('report_lamina', lambda: RP.lamina_counts(xyz, pop['radii'], cp, ci, sx, 0.05,
                                                                           ctx=ctx))}
    for nmap in a.maps:
        t0 = time.time()
        vols = [V.sphere_map(5500.0, 100.0, 3, center=(7.0 * m, -3.0 * m, 5.0 * m)) for m in range(nmap)]
        smap = (np.arange(a.nstruct) % nmap).astype(np.int32)
        print('%d map(s) of %s voxels built in %.1f s' % (nmap, tuple(vols[0]['nvoxel']), time.time() - t0),
              file=sys.stderr, flush=True)
        ms['report_map_levels_%dmap' % nmap] = timed('report_map_levels', lambda: RP._map_levels(
            xyz, vols, smap, ctx, 0, want_mean=True, want_depth=True, density_edges=dedges, nshell=5,
            shell_edges=sedges))
        ms['report_map_levels_pass1_%dmap' % nmap] = timed('report_map_levels', lambda: RP._map_levels(
            xyz, vols, smap, ctx, 0, want_mean=True, want_depth=True, density_edges=dedges))
        ms['report_map_lamina_%dmap' % nmap] = timed('report_map_lamina', lambda: RP.map_lamina_counts(
            xyz, vols, smap, pop['radii'], cp, ci, 0.05, ctx=ctx))
    nb, S = xyz.shape[0], xyz.shape[1]
    print(json.dumps({'nbead': int(nb), 'nstruct': int(S), 'nhap': int(len(cp) - 1), 'calls': a.calls,
                      'kernel_ms': ms,
                      'map_levels_bytes': {'coordinates': 12 * nb * S, 'voxel_records': 16 * nb * S,
                                           'level_scratch_written': 8 * nb * S}}))


if __name__ == '__main__':
    main()
