"""What the native position anchor buys over the dummy-atom form.

The demo 2 Mb model (3008 beads + the centre dummy), 64 structures, 500 traced loci each,
the demo protocol x0.1.  Two ways to run the same restraints through igm_mstep_run:

  native   anchors=(ptr, igm_anchor): 3009 atoms, the LDS engine
  dummy    one IGM_ATOM_FIXED atom per traced locus + one bond, the existing API: 3509 atoms,
           past the LDS engine's 3072, hence the population engine

mstep.run on host arrays returns after the work is done (no IGM_ASYNC), so the wall time of
a call is the time of the run plus its PCIe copies, the same for both forms.  One warm-up of
each, then three repeats each, alternating.  Prints one JSON line.

    python scripts/tracing_native_vs_dummy.py [--nstruct 64] [--anchors 500] [--scale 0.1]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from igm_amd import model as M  # noqa: E402
from igm_amd import mstep, synthetic as syn, workloads as W  # noqa: E402
from igm_amd._lib import IGM_ATOM_FIXED, anchor_dtype, bond_dtype  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nstruct', type=int, default=64)
    ap.add_argument('--anchors', type=int, default=500)
    ap.add_argument('--scale', type=float, default=0.1)
    ap.add_argument('--repeats', type=int, default=3)
    a = ap.parse_args()
    S, n = a.nstruct, a.anchors
    pop = syn.population_2mb(S)
    atoms = M.Atoms(pop['radii'])
    nbead, natom = len(pop['radii']), atoms.n
    poly = M.polymer_bonds(pop['chrom'], pop['copy'], pop['radii'], 2.0, 1.0)
    prm = M.params_from_cfg({'optimization': {'optimizer_options': W.scaled_protocol(syn.DEMO_PROTOCOL, a.scale)}},
                            [((5500.0,) * 3, 1.0)])
    x = np.zeros((S, natom, 3), np.float32)
    x[:, :nbead] = pop['xyz']
    seeds = M.lammps_seeds(6535, np.arange(S), 1)
    # traced loci: n beads per structure, imaged 300 nm (sd) from where the territories put them
    rng = np.random.default_rng(0)
    anch = np.zeros(S * n, anchor_dtype)
    ptr = np.arange(S + 1, dtype=np.int64) * n
    for s in range(S):
        loci = np.sort(rng.choice(nbead, n, replace=False))
        t = x[s, loci] + rng.normal(0.0, 300.0, (n, 3))
        q = anch[s * n:(s + 1) * n]
        q['atom'], q['x'], q['y'], q['z'], q['r0'], q['k'] = loci, t[:, 0], t[:, 1], t[:, 2], 50.0, 1.0
    # the dummy-atom form
    radii2 = np.concatenate([atoms.radii, np.zeros(n, np.float32)])
    flags2 = np.concatenate([atoms.flags, np.full(n, IGM_ATOM_FIXED, np.uint32)])
    x2 = np.zeros((S, natom + n, 3), np.float32)
    x2[:, :natom] = x
    sb = np.zeros(S * n, bond_dtype)
    for s in range(S):
        q = anch[s * n:(s + 1) * n]
        x2[s, natom:] = np.stack([q['x'], q['y'], q['z']], 1)
        b = sb[s * n:(s + 1) * n]
        b['i'], b['j'], b['r0'], b['k'] = natom + np.arange(n), q['atom'], q['r0'], q['k']

    def native():
        return mstep.run(prm, x, atoms.radii, atoms.flags, poly, None, None, seeds, anchors=(ptr, anch))

    def dummy():
        return mstep.run(prm, x2, radii2, flags2, poly, ptr, sb, seeds)
    times = {'native': [], 'dummy': []}
    out = {}
    for rep in range(a.repeats + 1):  # rep 0: warm-up
        for name, fn in (('native', native), ('dummy', dummy)):
            t0 = time.perf_counter()
            xo, info = fn()
            dt = time.perf_counter() - t0
            if rep:
                times[name].append(dt)
            out[name] = (xo, info)
    far = {}
    for name, (xo, info) in out.items():  # the share of anchors left past 1.05 r0: the same restraint in both forms
        d = np.concatenate([np.linalg.norm(xo[s, anch['atom'][s * n:(s + 1) * n]] - np.stack(
            [anch['x'], anch['y'], anch['z']], 1)[s * n:(s + 1) * n], axis=1) for s in range(S)])
        far[name] = float(np.mean(d > 52.5))
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(json.dumps({'nstruct': S, 'anchors_per_structure': n, 'protocol_scale': a.scale,
                      'native_s': times['native'], 'dummy_s': times['dummy'], 'native_median_s': med['native'],
                      'dummy_median_s': med['dummy'], 'dummy_over_native': med['dummy'] / med['native'],
                      'violated_fraction': far}))


if __name__ == '__main__':
    main()
