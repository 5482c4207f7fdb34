"""The fp64 oracle's force field against an independent reference (CPU).

oracle/mstep_ref.c is what every GPU force test compares the kernels with; it was written
from the same formulas as the kernels.  tests/small_models.brute_forces evaluates the
same force field in numpy fp64 over every pair (no cell lists, none of the oracle's code).
Both sides are fp64 and differ in summation order only, over at most ~3000 terms per atom
(the coincident pair energy: 32 640 equal terms), so the bounds are
max|dF| <= 1e-12 max|F| and energies to rtol 1e-12 (measured: 3e-16 and 5e-15)."""
import math

import numpy as np
import pytest

import oracle
import small_models as sm
from igm_amd import model as M

CPU_SIZES = (3, 64, 65, 257, 1024, 1025, 3073)


def _compare(natom, geometry, envelopes):
    atoms, poly, prm, ptr, sb, x = sm.case(natom, geometry, envelopes)
    fo, eo = oracle.mstep_forces(prm, x, atoms.radii, atoms.flags, poly, ptr, sb, sm.EVF, sm.ENVF)
    fb, eb, parts = sm.brute_batch(atoms, poly, ptr, sb, x, envelopes, sm.EVF, sm.ENVF, parts=True)
    print('natom %d %s nenv %d: max|dF| %.3g of max|F| %.3g' % (natom, geometry, len(envelopes),
                                                                np.abs(fo - fb).max(), np.abs(fb).max()))
    assert np.all(np.isfinite(fo)) and np.all(np.isfinite(fb))
    assert np.abs(fo - fb).max() <= 1e-12 * np.abs(fb).max()
    ne = 2 + len(envelopes)
    assert np.allclose(eo[:, 1:1 + ne], eb, rtol=1e-12, atol=0.0)
    assert np.allclose(eo[:, 0], eb.sum(axis=1), rtol=1e-12, atol=0.0)
    assert np.all(eo[:, 1 + ne:] == 0.0)
    return (atoms, poly, prm, ptr, sb, x), (fo, eo), (fb, eb, parts)


@pytest.mark.parametrize('envelopes', [sm.ENV_ONE, sm.ENV_TWO], ids=['env1', 'env2'])
@pytest.mark.parametrize('natom', CPU_SIZES)
def test_oracle_forces_match_brute_force(natom, envelopes):
    model, _, (fb, eb, _) = _compare(natom, 'random', envelopes)
    atoms = model[0]
    if len(envelopes) == 2 and natom >= 64:  # the per-structure flag rows differ, and so do the forces they give
        assert atoms.flags.ndim == 2 and not np.array_equal(atoms.flags[0], atoms.flags[2])
    if natom >= 64:
        assert np.all(eb[:, 1] > 0)  # stretched bonds


@pytest.mark.parametrize('envelopes', [sm.ENV_ONE, sm.ENV_TWO], ids=['env1', 'env2'])
@pytest.mark.parametrize('geometry', sm.GEOMETRIES)
def test_oracle_forces_degenerate_geometries(geometry, envelopes):
    natom = 257
    (atoms, poly, prm, ptr, sb, x), (fo, eo), (fb, eb, parts) = _compare(natom, geometry, envelopes)
    nbead = natom - 1
    if geometry == 'coincident':
        # closed form: every pair at r = 0 gives no force and E = A (1 + cos 0) = 2 A
        r = atoms.radii[:nbead].astype(np.float64)
        rc = r[:, None] + r[None, :]
        iu = np.triu_indices(nbead, 1)
        e2a = math.fsum(2.0 * sm.EVF * (rc[iu] / np.pi) ** 2)
        for s in range(len(x)):
            assert np.all(parts[s]['pair'] == 0.0)
            assert np.isclose(eo[s, 1], e2a, rtol=1e-12, atol=0.0) and np.isclose(eb[s, 0], e2a, rtol=1e-12, atol=0.0)
            # bonds of length 0 have no direction: energy, no force (LAMMPS bond_harmonic, r > 0 guard)
            assert np.all(parts[s]['bond'] == 0.0) and (s == 1 or eb[s, 1] > 0)
        assert np.all(fo[:, nbead] == 0.0)
    if geometry == 'origin' and len(envelopes) == 2:
        # k2 = 0 at the centre: the k < 0 envelope (active for 0 < k2 < 1) gives exactly no force
        for s in range(len(x)):
            assert sm.struct_flags(atoms, s)[0] & (M.IGM_ATOM_ENV0 << 1)
            assert np.all(x[s, 0] == 0.0) and np.all(parts[s]['env'][1][0] == 0.0)
            only_env1 = fo[s, 0] - parts[s]['pair'][0] - parts[s]['bond'][0] - parts[s]['env'][0][0]
            assert np.abs(only_env1).max() <= 1e-12 * np.abs(fb).max()
            assert eb[s, 3] > 0  # the other members feel it
    if geometry == 'one_cell':
        assert np.abs(x[:, :nbead] - x[:, :1]).max() <= 0.1 * min(sm.RADII)
    if geometry in ('outlier', 'plane_outlier'):
        assert np.abs(fb[:, sm.outlier_index(nbead)]).max() > 1e5  # the envelope pulls it back


def _headroom_cases():
    out = [(n, 'random') for n in sm.SIZES]
    out += [(n, g) for n in sm.GEOM_SIZES for g in sm.GEOMETRIES if not (g == 'random' and n in sm.SIZES)]
    return out


@pytest.mark.parametrize('natom,geometry', _headroom_cases())
def test_f32_bound_has_headroom_on_every_gpu_input(natom, geometry):
    """The GPU tests hold the f32 force path to ||err|| <= 1e-5 ||F_ref||.  The bound is
    relative to the net force, so every input the GPU tests use must leave an honest
    float32 evaluation (brute_forces in float32) at least 10x under it; 'coincident' (no
    net pair force) and 'one_cell' are held, per atom, to 1e-5 of the summed magnitudes of
    the atom's terms instead, and float32 numpy stays 10x under that as well."""
    env = sm.f32_envelopes(geometry)
    atoms, poly, prm, ptr, sb, x = sm.case(natom, geometry, env)
    f64, _, parts = sm.brute_batch(atoms, poly, ptr, sb, x, env, sm.EVF, sm.ENVF, parts=True)
    f32, _ = sm.brute_batch(atoms, poly, ptr, sb, x, env, sm.EVF, sm.ENVF, np.float32)
    err = np.linalg.norm(f32 - f64, axis=2)
    ref = np.linalg.norm(f64, axis=2)
    if geometry != 'coincident':
        h = 1e-5 * np.linalg.norm(ref) / np.linalg.norm(err)
        print('natom %d %s: f32 headroom %.0f' % (natom, geometry, h))
        assert h >= 10
    if geometry in ('outlier', 'plane_outlier'):  # also over the atoms the outlier's 1e6-scale forces do not reach
        keep = sm.outlier_rest(poly, ptr, sb, x)
        h = 1e-5 * np.linalg.norm(ref[keep]) / np.linalg.norm(err[keep])
        print('natom %d %s: f32 headroom over the rest %.0f' % (natom, geometry, h))
        assert h >= 10
    if geometry in ('coincident', 'one_cell'):
        bound = 1e-5 * sm.term_magnitudes(parts, geometry)
        assert np.all(err[bound == 0] == 0)
        h = (bound[bound > 0] / np.maximum(err[bound > 0], 1e-300)).min()
        print('natom %d %s: f32 per-atom headroom %.0f' % (natom, geometry, h))
        assert h >= 10
