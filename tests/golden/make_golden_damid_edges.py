#!/opt/conda/bin/python3.9
"""Golden vectors of the DamID A-step and of the DamID lamina selection beyond diploids, produced
by running the REFERENCE's own get_damid_actdist_I (igm/steps/DamidActivationDistanceStep.py:376-471)
with the '%6d %.5f %.5f' text round trip of task()/reduce(), and its snormsq_ellipsoid with the
membership decision of Damid._apply_envelope (igm/restraints/damid.py:43-61,112-126).  Build
container only, like make_golden.py:

    /opt/conda/bin/python3.9 tests/golden/make_golden_damid_edges.py

The inputs are those of tests/damid_edges.py (golden_cases(), select_traps()): a genome with 1, 2,
3 and 4 copies per locus behind a copy index that is neither contiguous nor ascending, radii that
differ between the copies of a locus, sphere and a three-axis ellipsoid, it_corr 0 and 1, S = 1, 5,
64 and 65, contact range 0.05 and 0.0, lattice populations, keys 0 / subnormal / inf / NaN, the
count threshold, order-index and decimal ties.  damid_golden.npz pins diploids on continuous
coordinates only.

damid_edges_golden.npz holds
  cases                              the A-step case names
  pop_s<S>                           the lattice population of damid_edges.population(S)
  <case>_loc, _dist, _prob           the rows after the text round trip
  <case>_p64, _ad64                  per listed locus: the reference's own p and activation distance
  select_sel                         (S, nrows) bool: Damid._apply_envelope's decision per structure
                                     and row on damid_edges.select_traps()
The file is data only.  It is written with fixed zip time stamps, so the script regenerates it
byte for byte.
"""
import contextlib
import io
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden  # noqa: E402  (builds the reference environment)
import numpy as np  # noqa: E402
import importlib  # noqa: E402
from make_golden_actdist_ploidy import save_npz  # noqa: E402
from make_golden_asteps import damid_roundtrip  # noqa: E402
import damid_edges as E  # noqa: E402

damid_mod = importlib.import_module('igm.steps.DamidActivationDistanceStep')
restraint_mod = importlib.import_module('igm.restraints.damid')
from igm.model.particle import Particle  # noqa: E402

assert np.__version__.startswith('1.')


def run_case(c):
    hss = make_golden.DuckHss(c['xyz'], c['radii'], c['copy_index'], None)
    rows, p64, ad64 = [], [], []
    # the rows task() writes for these loci (params are f32: setup() :211-217)
    params = np.array([(I, pe, pl) for I, pe, pl in zip(c['loci'], c['p_exp'], c['plast'])], dtype=np.float32)
    for I, p_exp, pl in params:
        with contextlib.redirect_stdout(io.StringIO()):
            r = damid_mod.get_damid_actdist_I(int(I), p_exp, pl, hss, c['it_corr'], contact_range=c['cr'],
                                              shape=c['shape'], nucleus_param=c['param'])
        rows += r
        ad64.append(float(r[0][1]))
        p64.append(float(r[0][2]))
    rt = damid_roundtrip(rows)
    return rt, np.array(p64), np.array(ad64)


def run_select():
    """Damid._apply_envelope's list comprehension (damid.py:119-126) per structure: the particle
    positions and radii as Particle holds them, d the float32 the activation distance file yields"""
    xyz, radii, rows, _ = E.select_traps()
    cutoff = 1 - 0.0
    a, b, c = E.SEL_ABC
    sel = np.zeros((xyz.shape[0], len(rows)), bool)
    for s in range(xyz.shape[0]):
        particles = [Particle(xyz[s, i], radii[i], Particle.NORMAL) for i in range(xyz.shape[1])]
        for q, (i, d) in enumerate(zip(rows['loc'], rows['dist'])):
            i = int(i)
            sel[s, q] = restraint_mod.snormsq_ellipsoid(particles[i].pos, np.array([a, b, c]) * cutoff,
                                                        particles[i].r) >= d**2
    return sel


def main():
    out = {}
    cases = E.golden_cases()
    for S in E.S_GOLDEN:
        out['pop_s%d' % S] = np.array(E.population(S))
    for name, c in cases.items():
        rt, p64, ad64 = run_case(c)
        out[name + '_loc'], out[name + '_dist'], out[name + '_prob'] = rt['loc'], rt['dist'], rt['prob']
        out[name + '_p64'], out[name + '_ad64'] = p64, ad64
        print(name, len(c['loci']), 'loci', len(rt), 'rows', flush=True)
    out['cases'] = np.array(list(cases))
    out['select_sel'] = run_select()
    path = os.path.join(HERE, 'damid_edges_golden.npz')
    save_npz(path, out)
    print('damid_edges_golden.npz', os.path.getsize(path))


if __name__ == '__main__':
    main()
