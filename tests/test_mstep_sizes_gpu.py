"""The M-step engines at every model size and at degenerate geometries, through the C ABI.

Which kernels run depends on natom (lds_fits / prepare / IGM_DISPATCH_ALL in
igm_amd/csrc/mstep.hip; the table is in DESIGN.md):
    1 .. 1024      population (HBM) engine          2049 .. 3072   LDS kernels <1024, 3>
    1025 .. 2048   LDS kernels <1024, 2>            3073 .. 65535  population engine
(IGM_MSTEP_FORCE_GLOBAL forces the population engine at any size.)  The other GPU tests run
at ~3009 and 29 839 atoms only.  The inputs are tests/small_models.py's; the references are
the fp64 oracle and small_models.brute_forces (numpy fp64 over every pair), which
tests/test_small_models.py pins to each other on the CPU.

Tolerances (the project's own, as in test_mstep_gpu.py / test_mstep_paths_gpu.py):
    f64 forces (f32 on output)   max|d| <= 1e-6 max|F_ref| + 1e-6
    energies                     rtol 1e-9, atol 1e-9
    f32 forces                   ||err|| <= 1e-5 ||F_ref|| over the batch
    md segments                  max|dx| < 1e-3 max(1, moved), moved > 1
"""
import json
import os

import numpy as np
import pytest

import oracle
import small_models as sm
from igm_amd import _lib
from igm_amd import model as M
from igm_amd import synthetic as syn
from igm_amd._lib import IGM_MSTEP_FORCE_GLOBAL

pytestmark = pytest.mark.gpu

EVF, ENVF = sm.EVF, sm.ENVF


@pytest.fixture(scope='module')
def ms():
    from igm_amd import mstep
    return mstep


def _engine(prm, engine):
    """a copy of prm for the default engine of the size, or the population engine forced"""
    p = _lib.MStepParams.from_buffer_copy(prm)
    if engine == 'global':
        p.flags |= IGM_MSTEP_FORCE_GLOBAL
    return p


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_REFS = {}


def _reference(natom, geometry='random'):
    """(model, oracle (f, e), brute (f, e, parts)) of a force-test input, computed once"""
    key = (natom, geometry)
    if key not in _REFS:
        model = sm.case(natom, geometry)
        atoms, poly, prm, ptr, sb, x = model
        orc = oracle.mstep_forces(prm, x, atoms.radii, atoms.flags, poly, ptr, sb, EVF, ENVF)
        _REFS[key] = (model, orc, sm.brute_batch(atoms, poly, ptr, sb, x, sm.ENV_TWO, EVF, ENVF, parts=True))
    return _REFS[key]


def _check_f64(tag, fg, eg, fref, eref_cols):
    scale = np.abs(fref).max()
    print('%s: f64 max|dF| %.3g (bound %.3g), max rel dE %.3g' % (
        tag, np.abs(fg - fref).max(), 1e-6 * scale + 1e-6,
        np.abs(eg[:, :eref_cols.shape[1]] - eref_cols).max() / max(np.abs(eref_cols).max(), 1e-300)))
    assert np.all(np.isfinite(fg)) and np.all(np.isfinite(eg[:, :eref_cols.shape[1]]))
    assert np.abs(fg - fref).max() <= 1e-6 * scale + 1e-6  # f64 path, rounded to f32 on output
    assert np.allclose(eg[:, :eref_cols.shape[1]], eref_cols, rtol=1e-9, atol=1e-9)


def _check_f32(tag, fg, fref, keep=None):
    err = np.linalg.norm(fg - fref, axis=2)
    ref = np.linalg.norm(fref, axis=2)
    if keep is not None:
        err, ref = err[keep], ref[keep]
    print('%s: f32 ||err|| %.3g (bound %.3g)' % (tag, np.linalg.norm(err), 1e-5 * np.linalg.norm(ref)))
    assert np.all(np.isfinite(fg))
    assert np.linalg.norm(err) <= 1e-5 * np.linalg.norm(ref)


def _brute_energy_cols(eb):
    """{total, pair, bond, env0, env1} as the C ABI orders them"""
    return np.concatenate([eb.sum(axis=1, keepdims=True), eb], axis=1)


# ------------------------------------------------------------------ (a) size sweep, forces
def _sweep():
    out = []
    for n in sm.SIZES:
        out.append((n, 'default'))
        if n <= 3072:  # (3073 and up: the population engine is the default)
            out.append((n, 'global'))
    return out


@pytest.mark.parametrize('natom,engine', _sweep())
def test_gpu_forces_every_size(ms, natom, engine):
    """S = 3 (the middle structure without per-structure bonds: an empty CSR row, and with
    the polymer's <= 8 bond types the LDS-staged bond path), two envelopes through (S, N)
    flags.  f64 path against the oracle and against brute_forces; f32 path against the
    oracle.  natom = 3 is forces only: 2 beads have no thermal degrees of freedom left
    once the momentum is removed, so the dynamics tests start at 65."""
    (atoms, poly, prm, ptr, sb, x), (fo, eo), (fb, eb, _) = _reference(natom)
    p = _engine(prm, engine)
    tag = 'natom %d %s' % (natom, engine)
    fg, eg = ms.forces(p, x, atoms.radii, atoms.flags, poly, ptr, sb, EVF, ENVF)
    _check_f64(tag + ' vs oracle', fg, eg, fo, eo[:, :5])
    _check_f64(tag + ' vs brute', fg, eg, fb, _brute_energy_cols(eb))
    f32, _ = ms.forces(p, x, atoms.radii, atoms.flags, poly, ptr, sb, EVF, ENVF, f32=True)
    _check_f32(tag, f32, fo)


@pytest.mark.parametrize('natom,engine', [(257, 'default'), (1100, 'default'), (1100, 'global')])
def test_gpu_forces_without_bonds(ms, natom, engine):
    """No shared bonds and no per-structure CSR at all (shared_bonds empty, sbond_ptr None)."""
    atoms, poly, prm, ptr, sb, x = sm.case(natom)
    p = _engine(prm, engine)
    none = poly[:0]
    fo, eo = oracle.mstep_forces(prm, x, atoms.radii, atoms.flags, none, None, None, EVF, ENVF)
    fb, eb = sm.brute_batch(atoms, none, None, None, x, sm.ENV_TWO, EVF, ENVF)
    assert np.all(eo[:, 2] == 0.0) and np.all(eb[:, 1] == 0.0)
    tag = 'natom %d %s, no bonds' % (natom, engine)
    fg, eg = ms.forces(p, x, atoms.radii, atoms.flags, none, None, None, EVF, ENVF)
    _check_f64(tag + ' vs oracle', fg, eg, fo, eo[:, :5])
    _check_f64(tag + ' vs brute', fg, eg, fb, _brute_energy_cols(eb))
    assert np.all(eg[:, 2] == 0.0)
    f32, _ = ms.forces(p, x, atoms.radii, atoms.flags, none, None, None, EVF, ENVF, f32=True)
    _check_f32(tag, f32, fo)


# ------------------------------------------------------------------ (c) degenerate geometries
@pytest.mark.parametrize('natom,engine', [(257, 'default'), (1100, 'default'), (1100, 'global')])
@pytest.mark.parametrize('geometry', [g for g in sm.GEOMETRIES if g != 'random'])
def test_gpu_forces_degenerate_geometries(ms, geometry, natom, engine):
    """f64 and f32 forces against brute_forces (fp64) for coincident beads, a line, a plane,
    everything in one cell, a far outlier (one that inflates the cells; with a planar rest,
    one that leaves more cells than the grids hold unless the cell count is capped), a bead
    at the envelope centre, and a dense cloud (lists of ~150 entries at 257 atoms; at 1100,
    past the list capacity of either engine: the cell walks, with pairs at every r up to
    the cutoff).  The f32 bound is relative to the net force; where the
    outlier's 1e6-scale forces would hide everyone else, it is also applied to the atoms
    that share no bond with the outlier.  'coincident' has no net pair force (every pair
    term is exactly 0 at r = 0), so there the bound is absolute and per atom:
    err_i <= 1e-5 x (sum of the magnitudes of the bond and envelope terms on atom i, from
    brute_forces) -- an atom without such a term must come out exactly 0.  'one_cell' (beads
    a few nm apart, pair terms ~ evf r) passes the relative bound with CPU-side headroom
    (small_models docstring), and is held to the absolute form over all its terms as well."""
    (atoms, poly, prm, ptr, sb, x), _, (fb, eb, parts) = _reference(natom, geometry)
    p = _engine(prm, engine)
    tag = 'natom %d %s %s' % (natom, engine, geometry)
    fg, eg = ms.forces(p, x, atoms.radii, atoms.flags, poly, ptr, sb, EVF, ENVF)
    _check_f64(tag + ' vs brute', fg, eg, fb, _brute_energy_cols(eb))
    keep = sm.outlier_rest(poly, ptr, sb, x) if geometry in ('outlier', 'plane_outlier') else None
    if keep is not None:
        rest = np.abs(fb[keep]).max()
        print('%s: f64 max|dF| over the rest %.3g (bound %.3g)' % (tag, np.abs(fg - fb)[keep].max(),
                                                                    1e-6 * rest + 1e-6))
        assert np.abs(fg - fb)[keep].max() <= 1e-6 * rest + 1e-6
    # the f32 path ('line': the k > 0 envelope alone, small_models.f32_envelopes)
    env = sm.f32_envelopes(geometry)
    if env is not sm.ENV_TWO:
        atoms, poly, prm, ptr, sb, x = sm.case(natom, geometry, env)
        p = _engine(prm, engine)
        fb, eb, parts = sm.brute_batch(atoms, poly, ptr, sb, x, env, EVF, ENVF, parts=True)
    f32, _ = ms.forces(p, x, atoms.radii, atoms.flags, poly, ptr, sb, EVF, ENVF, f32=True)
    assert np.all(np.isfinite(f32))  # no NaN from rsq(0) or 1 / |x|
    if geometry != 'coincident':
        _check_f32(tag, f32, fb)
        if keep is not None:
            _check_f32(tag + ' (rest)', f32, fb, keep)
    if geometry in ('coincident', 'one_cell'):
        err = np.linalg.norm(f32 - fb, axis=2)
        bound = 1e-5 * sm.term_magnitudes(parts, geometry)
        print('%s: f32 per-atom worst err/bound %.3g, atoms with bound 0: %d' % (
            tag, (err[bound > 0] / bound[bound > 0]).max() if np.any(bound > 0) else 0.0, int((bound == 0).sum())))
        assert np.all(err <= bound)


# ------------------------------------------------------------------ (e) dynamics at the untested sizes
def _velocities(atoms, nstruct, seed0=11):
    fl = atoms.flags[0] if atoms.flags.ndim == 2 else atoms.flags  # (the FIXED bit is the same in every row)
    return np.stack([oracle.velocity_create(fl, 50.0, seed0 + s) for s in range(nstruct)]).astype(np.float32)


def _md_case(natom, nstruct, envelopes=sm.ENV_TWO):
    return sm.make(natom - 1, nstruct, 1000 + natom, envelopes=envelopes, empty_rows=(1,))


def _check_md(ms, tag, model, nsteps, engine='default', nthreads=4):
    atoms, poly, prm, ptr, sb, x = model
    v = _velocities(atoms, len(x))
    xg, vg = ms.md(_engine(prm, engine), x, v, atoms.radii, atoms.flags, poly, ptr, sb, EVF, ENVF, 50.0, 40.0, 1000.0,
                   nsteps)
    xo, vo = oracle.mstep_md(prm, x.astype(np.float64), v.astype(np.float64), atoms.radii, atoms.flags, poly, ptr, sb,
                             EVF, ENVF, 50.0, 40.0, 1000.0, nsteps, nthreads=nthreads)
    moved = np.abs(xo - x).max()
    print('%s: md %d steps moved %.3g, max|dx| %.3g' % (tag, nsteps, moved, np.abs(xg - xo).max()))
    assert moved > 1.0
    assert np.all(np.isfinite(xg)) and np.all(np.isfinite(vg))
    assert np.abs(xg - xo).max(axis=(1, 2)).max() < 1e-3 * max(1.0, moved)
    return xg, xo


DYN_SIZES = (65, 1024, 1100, 2048)


@pytest.mark.parametrize('natom', DYN_SIZES)
def test_gpu_md_segment_tracks_oracle_every_engine(ms, natom):
    """20 steps of nve/limit + temp/rescale from identical x, v against the fp64 oracle."""
    _check_md(ms, 'natom %d' % natom, _md_case(natom, 3), 20)


def _short_protocol(steps=(60, 80, 80, 60), relax=20):
    p = json.loads(json.dumps(syn.DEMO_PROTOCOL))
    p['custom_annealing_protocol']['mdsteps'] = list(steps)
    p['custom_annealing_protocol']['relax']['mdsteps'] = relax
    return p


@pytest.mark.parametrize('natom', DYN_SIZES)
def test_gpu_protocol_short_every_engine(ms, natom):
    """The demo protocol at mdsteps (60, 80, 80, 60), relax 20: bitwise equal on a rerun,
    finite, downhill.  At 65 and 1024 (population engine) also bitwise equal with 3 structure
    groups and without bond pruning, as the 200 kb model is held at 29 839."""
    atoms, poly, _, ptr, sb, x = _md_case(natom, 4)
    prm = M.params_from_cfg({'optimization': {'optimizer_options': _short_protocol()}}, sm.ENV_TWO)
    seeds = M.lammps_seeds(6535, list(range(4)), 3)

    def run():
        return ms.run(prm, x, atoms.radii, atoms.flags, poly, ptr, sb, seeds)
    x0, i0 = run()
    x1, i1 = run()
    assert np.array_equal(x0, x1) and i0.tobytes() == i1.tobytes()
    assert np.all(np.isfinite(x0)) and np.all(np.isfinite(i0['final_energy']))
    print('natom %d: E %s -> %s, rebuilds %s' % (natom, i0['einitial'].round(1).tolist(),
                                                 i0['final_energy'].round(1).tolist(), i0['nrebuild'].tolist()))
    # downhill; the 64 beads of structure 1 (polymer bonds only) anneal to exactly E = 0 on the
    # GPU as in the oracle, and CG has nothing left to lower there
    assert np.all((i0['final_energy'] < i0['einitial']) | (i0['einitial'] == 0.0))
    assert np.all(i0['final_energy'] <= i0['einitial']) and np.count_nonzero(i0['einitial'] > 0) >= 3
    if natom <= 1024:
        variants = {'3 groups': {'IGM_POP_GROUPS': '3'}, 'no bond pruning': {'IGM_POP_BOND_PRUNE': '0'}}
        bad = []
        for name, env in variants.items():
            xv, iv = _with_env(env, run)
            if not (np.array_equal(x0, xv) and i0.tobytes() == iv.tobytes()):
                bad.append(name)
        assert not bad, bad


@pytest.mark.parametrize('natom', DYN_SIZES)
def test_gpu_cg_matches_oracle_every_engine(ms, natom):
    """CG only (no annealing stages): same algorithm in f64 on both sides
    (as test_mstep_gpu.test_gpu_cg_matches_oracle)."""
    atoms, poly, prm, ptr, sb, x = _md_case(natom, 4)
    prm.nstages = 0
    seeds = M.lammps_seeds(6535, list(range(4)), 11)
    xg, ig = ms.run(prm, x, atoms.radii, atoms.flags, poly, ptr, sb, seeds)
    xo, io, _ = oracle.mstep_run(prm, x.copy(), atoms.radii, atoms.flags, poly, ptr, sb, seeds, nthreads=4)
    print('natom %d: cg iters gpu %s oracle %s' % (natom, ig['cg_iters'].tolist(), io['cg_iters'].tolist()))
    assert np.allclose(ig['einitial'], io['einitial'], rtol=1e-10)
    assert np.allclose(ig['final_energy'], io['final_energy'], rtol=1e-5)
    assert np.all(ig['final_energy'] < ig['einitial'])
    assert np.all(np.abs(ig['cg_iters'] - io['cg_iters']) <= max(5, 0.1 * io['cg_iters'].max()))


# ------------------------------------------------------------------ (d) more structures than the resident grid
# 1024-thread workgroups: at most 2 per CU, 256 CUs -> at most 512 resident (<1024, 3>: 256); the
# structures past the grid are served through work_counter.  The population engine runs every
# structure in its grids; 700 structures in 3 groups (IGM_POP_GROUPS=3) are 233 + 233 + 234.
@pytest.mark.parametrize('natom,nstruct,env', [(1100, 600, {}), (3009, 300, {}), (65, 700, {'IGM_POP_GROUPS': '3'})],
                         ids=['1100x600', '3009x300', '65x700-3groups'])
def test_gpu_more_structures_than_the_resident_grid(ms, natom, nstruct, env):
    """Every structure has its own coordinates and bonds, so an indexing slip shows: f64
    forces per structure against the oracle, then 5 md steps (the engines' own structure
    loops) against the oracle's."""
    model = sm.make(natom - 1, nstruct, 2000 + natom, envelopes=sm.ENV_ONE, empty_rows=(1, nstruct - 2))
    atoms, poly, prm, ptr, sb, x = model
    fo, eo = oracle.mstep_forces(prm, x, atoms.radii, atoms.flags, poly, ptr, sb, EVF, ENVF, nthreads=16)
    fg, eg = _with_env(env, lambda: ms.forces(prm, x, atoms.radii, atoms.flags, poly, ptr, sb, EVF, ENVF))
    scale = np.abs(fo).max(axis=(1, 2))
    worst = np.abs(fg - fo).max(axis=(1, 2))
    print('natom %d S %d: worst structure %d, max|dF| %.3g' % (natom, nstruct, int(np.argmax(worst / scale)),
                                                              worst.max()))
    assert np.all(worst <= 1e-6 * scale + 1e-6)  # per structure
    assert np.allclose(eg[:, :4], eo[:, :4], rtol=1e-9, atol=1e-9)
    _with_env(env, lambda: _check_md(ms, 'natom %d S %d' % (natom, nstruct), model, 5, nthreads=16))


# ------------------------------------------------------------------ (b) the top of the range
def _density_sigma(nbead):
    """sigma of normal() coordinates that gives nbead beads the 200 kb model's mean number
    of neighbours inside the largest contact distance (2 x 150 nm here: the mean bead-bead
    count inside R of a Gaussian cloud is N R^3 / (6 sqrt(pi) sigma^3))."""
    from scipy.spatial import cKDTree
    pop = syn.population_200kb(1)
    x200 = pop['xyz'][0]
    r200 = 2.0 * float(pop['radii'].max())
    target = (cKDTree(x200).query_ball_point(x200, r200, return_length=True) - 1).mean()
    R = 300.0
    return R * (nbead / (6.0 * np.sqrt(np.pi) * target)) ** (1.0 / 3.0), target, R


@pytest.fixture(scope='module')
def top_models():
    out = {}
    for natom in (32769, 65535):
        sigma, target, R = _density_sigma(natom - 1)
        # the default envelope scaled with the cloud, so the same share of beads lies outside it
        env = [(tuple(a * sigma / 700.0 for a in sm.ENV_ONE[0][0]), 1.0)]
        out[natom] = (sm.make(natom - 1, 1, natom, nbonds=4000, envelopes=env, sigma=sigma), sigma, target, R)
    return out


@pytest.mark.parametrize('natom', [32769, 65535])
def test_gpu_forces_top_of_the_range(ms, top_models, natom):
    """Slot ids, bond partners and sort keys that use the top bit of the u16 (and at 65 535
    the sort that keeps its ids in HBM: they no longer fit in LDS beside the cell counts), at
    the 200 kb model's list density.  Oracle only: O(N^2) numpy is not affordable here."""
    from scipy.spatial import cKDTree
    (atoms, poly, prm, ptr, sb, x), sigma, target, R = top_models[natom]
    got = (cKDTree(x[0, :-1]).query_ball_point(x[0, :-1], R, return_length=True) - 1).mean()
    print('natom %d: sigma %.0f, mean neighbours inside %.0f nm %.2f (200 kb model %.2f)' % (natom, sigma, R, got,
                                                                                           target))
    assert 0.7 * target < got < 1.4 * target
    fo, eo = oracle.mstep_forces(prm, x, atoms.radii, atoms.flags, poly, ptr, sb, EVF, ENVF)
    fg, eg = ms.forces(prm, x, atoms.radii, atoms.flags, poly, ptr, sb, EVF, ENVF)
    _check_f64('natom %d' % natom, fg, eg, fo, eo[:, :4])
    f32, _ = ms.forces(prm, x, atoms.radii, atoms.flags, poly, ptr, sb, EVF, ENVF, f32=True)
    _check_f32('natom %d' % natom, f32, fo)


def test_gpu_md_segment_at_65535(ms, top_models):
    """10 md steps at the largest model: sort, permute and fill with slot ids >= 32 768."""
    _check_md(ms, 'natom 65535', top_models[65535][0], 10, nthreads=16)


def test_gpu_natom_65536_is_rejected(ms):
    atoms, poly, prm, ptr, sb, x = sm.make(65535, 1, 5, nbonds=10, envelopes=sm.ENV_ONE)
    assert atoms.n == 65536
    with pytest.raises(RuntimeError, match=r'code %d\).*outside \[1, 65535\]' % _lib.IGM_E_UNSUPPORTED):
        ms.forces(prm, x, atoms.radii, atoms.flags, poly, ptr, sb, EVF, ENVF)
