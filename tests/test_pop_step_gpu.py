"""The MD step of the population engine at its block, build and clamp edges: what happens between
two list builds, and at a build in the middle of a run (pop_integrate_kernel's vote and bbox
partials, pop_sort_kernel's reduction, flag list and four instantiations, pop_permute_kernel's
reorder, pop_force_kernel's KE partials and flag clearing, pop_factor, pop_walk_pairs,
pop_finish_kernel, kick_limit).  The inputs and their CPU-side properties are tests/pop_step.py's;
tests/test_pop_step.py proves on the CPU that each is the edge it claims.

Everything runs through mstep.md (one 'run N' from explicit velocities) or mstep.run against
oracle.mstep_md / oracle.mstep_run, at the bounds of test_anneal_step_gpu.py: positions within
1e-3 max(1, moved), velocities rtol 1e-3, atol 1e-3 max|v|.  Every case that guards against a
wrong outcome first asserts, on the CPU, that the oracle lies at least 100 of those tolerances
away from it (pop_step.bullet_power, pop_step.apart).

Sizes: 257 (two blocks, the second of one slot), 1024, 1100 with IGM_MSTEP_FORCE_GLOBAL, 3073,
16 384 | 16 385 (sort <true, 16> | <true, 32>; 64 | 65 blocks: the partial sums' stride),
32 768 | 32 769 (<true, 32> | <true, 0>), 48 638 | 48 639 (ids in LDS | in HBM).  nve/limit also
on the LDS anneal kernel (1025, 3072), where it has no direct test either.

Measured on the MI355X (this file, one process): see DESIGN.md section 2.
"""
import os

import numpy as np
import pytest

import pop_step as ps
import small_models as sm
from igm_amd import model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ms():
    from igm_amd import mstep
    return mstep


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


def _check(tag, x, xg, vg, xo, vo):
    """the project's md bounds (test_anneal_step_gpu._check)"""
    moved = np.abs(xo - x).max()
    dx = np.abs(xg - xo).max()
    vtol = 1e-3 * np.abs(vo) + 1e-3 * np.abs(vo).max()
    print('%s: moved %.4g, max|dx| %.3g (bound %.3g), max|dv| %.3g, worst dv/tol %.3g' % (
        tag, moved, dx, 1e-3 * max(1.0, moved), np.abs(vg - vo).max(), (np.abs(vg - vo) / np.maximum(vtol, 1e-300)).max()
        if np.abs(vo).max() > 0 else 0.0))
    assert np.all(np.isfinite(xg)) and np.all(np.isfinite(vg))
    assert dx < 1e-3 * max(1.0, moved)
    assert np.allclose(vg, vo, rtol=1e-3, atol=1e-3 * np.abs(vo).max())
    return moved


def _bullets_md(ms, case):
    lat = case.lat
    p = ps.engine_params(case.prm, ps.engine_of(case.natom))
    return ms.md(p, case.x, case.v, lat.atoms.radii, lat.atoms.flags, lat.poly, None, None, 1.0, 1.0, 50.0, 50.0, ps.XMAX,
                 case.nsteps)


# ------------------------------------------------------------------ 1. the vote, the build and the reorder
@pytest.mark.parametrize('natom,where,axis,which,nsteps,start', ps.bullet_cases())
def test_gpu_bullet_vote_rebuilds_and_reorders(ms, natom, where, axis, which, nsteps, start):
    """One bullet: in slot 0, in the last slot or late in a middle block; atom id 0, natom // 2 or
    natom - 1 on a lattice whose ids are dealt at random; along x, y or z.  Only its block votes;
    the build that follows moves it (y, z: into another block) and the velocity it hands over must
    follow the atoms through inv / remap."""
    case = ps.bullet_case(natom, where, axis, which, nsteps, start)
    xo, vo = ps.bullet_power(case)
    xg, vg = _bullets_md(ms, case)
    _check('natom %d %s axis %d id %s' % (natom, where, axis, which), case.x, xg, vg, xo, vo)


@pytest.mark.parametrize('natom', [257, 1100])
def test_gpu_bullets_stay_in_their_structures(ms, natom):
    """S = 5, bullets in structures 1 and 3 (different blocks), 0, 2 and 4 at rest: each against
    the oracle, the resting ones bitwise unchanged, and the whole result bitwise the same with
    1, 2 (default) and 3 structure groups (5 is divisible by neither 2 nor 3).  S = 1: the group
    count clamps to 1."""
    case = ps.isolation_case(natom)
    xo, vo = ps.bullet_power(case, verbose=False)
    runs = {}
    for name, env in (('1 group', {'IGM_POP_GROUPS': '1'}), ('default', {}), ('3 groups', {'IGM_POP_GROUPS': '3'})):
        runs[name] = _with_env(env, lambda: _bullets_md(ms, case))
    xg, vg = runs['default']
    for s in range(5):
        _check('natom %d structure %d' % (natom, s), case.x[s], xg[s], vg[s], xo[s], vo[s])
    for s in (0, 2, 4):
        assert np.array_equal(xg[s], case.x[s]) and not vg[s].any()
    for name in ('1 group', '3 groups'):
        assert np.array_equal(runs[name][0], xg) and np.array_equal(runs[name][1], vg), name
    one = ps.isolation_case(natom, 1)
    x1o, v1o = ps.bullet_power(one, verbose=False)
    for env in ({}, {'IGM_POP_GROUPS': '3'}):
        x1, v1 = _with_env(env, lambda: _bullets_md(ms, one))
        _check('natom %d S = 1 %s' % (natom, env), one.x, x1, v1, x1o, v1o)


@pytest.mark.parametrize('natom', [257, 1100, 3073])
def test_gpu_two_bullets_build_upon_build(ms, natom):
    """Two bullets of one structure, in its first and last block, whose collisions are three steps
    apart: consecutive builds of one structure, a parity flip upon a parity flip."""
    case = ps.two_bullet_case(natom)
    xo, vo = ps.bullet_power(case)
    xg, vg = _bullets_md(ms, case)
    _check('natom %d two bullets' % natom, case.x, xg, vg, xo, vo)


# ------------------------------------------------------------------ 2. thermostat across blocks, per-structure dof
def _thermo_md(ms, natom, fixed, window, fraction, t0, t1):
    atoms, poly, prm, ptr, sb, x, v, flags = ps.thermo_inputs(natom, fixed)
    p = ps.engine_params(prm, ps.engine_of(natom), t_window=window, t_fraction=fraction)
    return ms.md(p, x, v, atoms.radii, flags, poly, ptr, sb, sm.EVF, sm.ENVF, t0, t1, ps.XMAX, ps.thermo_steps(natom))


@pytest.mark.parametrize('natom', ps.THERMO_SIZES)
def test_gpu_thermostat_inside_the_window_is_exactly_off(ms, natom):
    """|T - target| stays inside a window of 1e7: the factor is exactly 1 at every step, so the
    run is bitwise the run with an unbounded window.  (CPU: the oracle agrees, and the default
    window is left -- test_pop_step.test_thermostat_window_branch_matters, repeated here.)"""
    x = ps.thermo_inputs(natom)[5]
    xw, vw = ps.thermo_oracle(natom, False, 1.0e7, 1.0, 50.0, 50.0)
    xu, vu = ps.thermo_oracle(natom, False, 1.0e30, 1.0, 50.0, 50.0)
    xd, vd = ps.thermo_oracle(natom, False, 0.1, 1.0, 50.0, 50.0)
    assert np.array_equal(xw, xu) and np.array_equal(vw, vu)
    assert ps.apart(x, xd, vd, xu, vu)[1] >= 100.0
    xg, vg = _thermo_md(ms, natom, False, 1.0e7, 1.0, 50.0, 50.0)
    xh, vh = _thermo_md(ms, natom, False, 1.0e30, 1.0, 50.0, 50.0)
    assert np.array_equal(xg, xh) and np.array_equal(vg, vh)
    _check('natom %d inside the window' % natom, x, xg, vg, xw, vw)


@pytest.mark.parametrize('fraction', [1.0, 0.5])
@pytest.mark.parametrize('natom', ps.THERMO_SIZES)
def test_gpu_thermostat_fraction(ms, natom, fraction):
    """Constant target 50, window 0.1: rescaled all the way (1.0) or half way (0.5).  At 16 385
    the kinetic energy is the sum of 65 block partials, past pop_factor's stride of 64."""
    x, flags = ps.thermo_inputs(natom)[5], ps.thermo_inputs(natom)[7]
    xo, vo = ps.thermo_oracle(natom, False, 0.1, fraction, 50.0, 50.0)
    other = ps.thermo_oracle(natom, False, 0.1, 1.5 - fraction, 50.0, 50.0)
    assert ps.apart(x, xo, vo, other[0], other[1])[1] >= 100.0
    xg, vg = _thermo_md(ms, natom, False, 0.1, fraction, 50.0, 50.0)
    _check('natom %d fraction %g' % (natom, fraction), x, xg, vg, xo, vo)
    if fraction == 1.0:  # the last step's rescale put T at the target, or found it inside the window
        T = ps.temperature(vg, flags)
        print('final T', T)
        assert np.all(np.abs(T - 50.0) <= 0.1 + 1e-3 * 50.0)


@pytest.mark.parametrize('fixed', [False, True])
@pytest.mark.parametrize('natom', ps.THERMO_SIZES)
def test_gpu_thermostat_ramp_to_its_last_step(ms, natom, fixed):
    """t0 = 50 to t1 = 40: the last step's target is t1 itself.  With every 3rd bead FIXED the
    temperature counts the mobile atoms only: a dof of all atoms would leave the final T off 40
    by the ratio of the counts (50 %: 143 allowances, asserted)."""
    atoms, poly, prm, ptr, sb, x, v, flags = ps.thermo_inputs(natom, fixed)
    xo, vo = ps.thermo_oracle(natom, fixed, 0.1, 1.0, 50.0, 40.0)
    xg, vg = _thermo_md(ms, natom, fixed, 0.1, 1.0, 50.0, 40.0)
    _check('natom %d ramp%s' % (natom, ' with FIXED beads' if fixed else ''), x, xg, vg, xo, vo)
    held = flags & M.IGM_ATOM_FIXED != 0
    assert held.sum() == (1 + len(np.arange(3, natom - 1, ps.FIXED_EVERY)) if fixed else 1)
    assert np.array_equal(xg[:, held], x[:, held]) and not vg[:, held].any()
    nm, nall = int((~held).sum()), natom - 1
    if fixed:
        assert abs(40.0 * (3.0 * nall - 3.0) / (3.0 * nm - 3.0) - 40.0) > 100.0 * (0.1 + 1e-3 * 40.0)
    T = ps.temperature(vg, flags)
    print('final T', T, 'oracle', ps.temperature(vo, flags))
    assert np.all(np.abs(T - 40.0) <= 0.1 + 1e-3 * 40.0)


@pytest.mark.parametrize('natom', ps.THERMO_SIZES)
def test_gpu_thermostat_at_zero_temperature(ms, natom):
    """All velocities zero and no forces: T = 0, the factor is 1 (no 0 / 0), nothing moves."""
    lat = ps.Lattice(natom)
    x = lat.x()
    v = np.zeros_like(x)
    p = ps.engine_params(lat.prm, ps.engine_of(natom))
    xg, vg = ms.md(p, x, v, lat.atoms.radii, lat.atoms.flags, lat.poly, None, None, 1.0, 1.0, 50.0, 40.0, ps.XMAX, 20)
    assert np.all(np.isfinite(xg)) and np.all(np.isfinite(vg))
    assert np.array_equal(xg, x) and not vg.any()


@pytest.mark.parametrize('natom', ps.THERMO_SIZES)
def test_gpu_thermostat_per_structure_dof(ms, natom):
    """(S, N) flags whose FIXED sets differ per structure: none, every 7th, every 3rd bead.  The
    oracle honours per-structure dof (CPU: test_pop_step.test_oracle_honours_per_structure_dof);
    structure 0's dof on structure 2 would end 50 % above the target, 100 allowances and more."""
    atoms, poly, prm, ptr, sb, x, v, flags = ps.dof_inputs(natom)
    xo, vo = ps.dof_oracle(natom)
    mobile = (flags & M.IGM_ATOM_FIXED == 0).sum(axis=1)
    dof = 3.0 * mobile - 3.0
    allow = ps.dof_allowance(prm)
    assert np.all(np.abs(ps.temperature(vo, flags) - ps.DOF_TARGET) <= allow)
    assert abs(ps.DOF_TARGET * dof[0] / dof[2] - ps.DOF_TARGET) > 100.0 * allow
    p = ps.engine_params(prm, ps.engine_of(natom))
    xg, vg = ms.md(p, x, v, atoms.radii, flags, poly, ptr, sb, sm.EVF, sm.ENVF, 50.0, 50.0, ps.XMAX,
                   ps.thermo_steps(natom))
    T = ps.temperature(vg, flags)
    print('natom %d: mobile %s, final T %s' % (natom, mobile.tolist(), T.tolist()))
    assert np.all(np.abs(T - ps.DOF_TARGET) <= allow)
    for s in range(3):
        _check('natom %d structure %d' % (natom, s), x[s], xg[s], vg[s], xo[s], vo[s])
    held = flags & M.IGM_ATOM_FIXED != 0
    assert np.array_equal(xg[held], x[held]) and not vg[held].any()


def test_gpu_thermostat_counts_the_last_block(ms):
    """16 385 lattice beads: 80 % of the kinetic energy belongs to the one slot of block 64, the
    65th partial of pop_factor's sum.  (The random models end in their dummy atom, which is FIXED
    and last in slot order: their 65th partial is 0.)"""
    lat, x, v, hot, slow, tt = ps.last_block_case()
    xo, vo = ps.last_block_oracle()
    xw, vw = ps.last_block_without((hot,))
    ax, av = ps.apart(x, xo, vo, xw, vw)
    assert ax >= 100.0 and av >= 100.0
    p = ps.engine_params(lat.prm, t_window=ps.LAST_BLOCK_WINDOW)
    xg, vg = ms.md(p, x, v, lat.atoms.radii, lat.atoms.flags, lat.poly, None, None, 1.0, 1.0, tt, tt, ps.XMAX,
                   ps.LAST_BLOCK_STEPS)
    _check('natom 16385, the last block hot', x, xg, vg, xo, vo)


# ------------------------------------------------------------------ 3. nve/limit, both engines
@pytest.mark.parametrize('natom', ps.LIMIT_POP + ps.LIMIT_LDS)
def test_gpu_limit_without_forces(ms, natom):
    """Three beads at |v| = 160 under xmax = 10 (along an axis and two oblique directions), the
    rest of the lattice at rest: every step moves each of them exactly 10 along its direction."""
    lat, x, v, who, dirs = ps.limit_free_case(natom)
    xo, vo = ps.limit_free_oracle(natom)
    xu, vu = ps.limit_free_oracle(natom, ps.XMAX)
    ax, av = ps.apart(x, xo, vo, xu, vu)
    assert ax > 100.0 and av > 100.0
    p = ps.engine_params(lat.prm, ps.engine_of(natom) if natom in ps.LIMIT_POP else 'default', t_window=1.0e30)
    xg, vg = ms.md(p, x, v, lat.atoms.radii, lat.atoms.flags, lat.poly, None, None, 1.0, 1.0, 50.0, 50.0,
                   ps.LIMIT_XMAX_FREE, 20)
    _check('natom %d nve/limit, no forces' % natom, x, xg, vg, xo, vo)
    for a, u in zip(who, dirs):
        assert np.allclose(np.linalg.norm(vg[0, a]), ps.LIMIT_XMAX_FREE / ps.DT, rtol=1e-5)
        assert np.allclose(xg[0, a] - x[0, a], 200.0 * u, rtol=0, atol=0.2)


@pytest.mark.parametrize('natom', ps.LIMIT_POP + ps.LIMIT_LDS)
def test_gpu_limit_with_forces_and_thermostat(ms, natom):
    """The overlapping random model under xmax = 1, window 0.1, 20 steps: every mobile atom is
    clamped at step 1 (CPU: at least half), and the kinetic energy the thermostat sees is that of
    the clamped velocities -- the force kernel kicks and clamps before it squares."""
    atoms, poly, prm, ptr, sb, x, v, flags = ps.thermo_inputs(natom)
    assert ps.clamped_at_step_1(natom) >= 0.5
    xo, vo = ps.limit_forces_oracle(natom)
    xu, vu = ps.limit_forces_oracle(natom, ps.XMAX)
    ax, av = ps.apart(x, xo, vo, xu, vu)
    assert ax >= 100.0 and av >= 100.0
    p = ps.engine_params(prm, ps.engine_of(natom) if natom in ps.LIMIT_POP else 'default')
    xg, vg = ms.md(p, x, v, atoms.radii, flags, poly, ptr, sb, sm.EVF, sm.ENVF, 50.0, 50.0, ps.LIMIT_XMAX_FORCES, 20)
    _check('natom %d nve/limit with forces' % natom, x, xg, vg, xo, vo)
    assert np.linalg.norm(xg - x, axis=2).max() <= 20 * ps.LIMIT_XMAX_FORCES * (1 + 1e-4)


# ------------------------------------------------------------------ 4. the cell walk after motion
@pytest.mark.parametrize('natom', ps.WALK_SIZES)
def test_gpu_cell_walk_after_motion(ms, natom):
    """'dense' for 20 md steps: beads with more than 256 neighbours inside cut_list take their
    pair forces from pop_walk_pairs, which finds its cells from the build position xb and reads
    the current positions -- here they differ, and at least one rebuild lies in between."""
    atoms, poly, prm, ptr, sb, x, v = ps.walk_inputs(natom)
    xo, vo = ps.walk_oracle(natom)
    cut, skin = ps.list_cut(atoms, prm)
    bead = atoms.flags & M.IGM_ATOM_BEAD != 0
    for s in range(len(x)):
        assert ps.most_neighbours(x[s], bead, cut) > ps.LIST_CAP and ps.most_neighbours(xo[s], bead, cut) > ps.LIST_CAP
    assert np.all(np.abs(xo - x).max(axis=(1, 2)) > skin / 2)
    p = ps.engine_params(prm, ps.engine_of(natom))
    xg, vg = ms.md(p, x, v, atoms.radii, atoms.flags, poly, ptr, sb, sm.EVF, sm.ENVF, 50.0, 40.0, ps.XMAX, 20)
    _check('natom %d dense' % natom, x, xg, vg, xo, vo)


# ------------------------------------------------------------------ 5. segment parity and build counts through run()
@pytest.mark.parametrize('natom', ps.RUN_SIZES)
def test_gpu_run_segments_and_build_counts(ms, natom):
    """mdsteps (5, 6, 7, 4), relax 3: eight segments of odd and even lengths, so the flag parity
    runs on across them.  No pair ever interacts (CPU: nve/limit bounds every path), so the
    trajectory is not chaotic: positions at the md bound, and nrebuild within one build per
    segment of the oracle's -- which lies between 'never' and 'always' by more than that."""
    lat = ps.run_case(natom)
    info, x64 = ps.run_oracle(natom)
    total = sum(ps.RUN_STEPS) + 4 * ps.RUN_RELAX
    assert np.all(info['nrebuild'] >= 3) and np.all(info['nrebuild'] <= total // 2)
    assert info['nrebuild'].min() - ps.RUN_SEGMENTS > 2 and info['nrebuild'].max() + ps.RUN_SEGMENTS < total
    x = lat.x()
    p = ps.engine_params(lat.prm, ps.engine_of(natom))
    seeds = ps.run_seeds(lat.nstruct)
    xg, ig = ms.run(p, x, lat.atoms.radii, lat.atoms.flags, lat.poly, None, None, seeds)
    moved = np.abs(x64 - x).max()
    print('natom %d: moved %.4g, max|dx| %.3g, rebuilds %s (oracle %s)' % (
        natom, moved, np.abs(xg - x64).max(), ig['nrebuild'].tolist(), info['nrebuild'].tolist()))
    assert np.all(np.isfinite(xg)) and np.abs(xg - x64).max() < 1e-3 * max(1.0, moved)
    assert np.all(np.abs(ig['nrebuild'].astype(np.int64) - info['nrebuild']) <= ps.RUN_SEGMENTS)
    # the lattice structures in a batch with overlapping random ones: bitwise what they are alone
    xm = ps.run_mixed_x(lat)
    seeds5 = ps.run_seeds(len(xm))
    assert np.array_equal(seeds5[:lat.nstruct], seeds)
    xg5, ig5 = ms.run(p, xm, lat.atoms.radii, lat.atoms.flags, lat.poly, None, None, seeds5)
    assert np.all(np.isfinite(xg5)) and np.all(ig5['final_energy'][lat.nstruct:] < ig5['einitial'][lat.nstruct:])
    assert np.array_equal(xg5[:lat.nstruct], xg)
    assert ig5[:lat.nstruct].tobytes() == ig.tobytes()
