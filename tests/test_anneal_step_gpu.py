"""The two block-wide exchanges of an MD step of the LDS anneal kernel -- the displacement
vote (one word per wave, one barrier) and the kinetic-energy sum with fix temp/rescale
behind it -- at the kernel's smallest and edge sizes:

    1025 atoms   <1024, 2>, the smallest LDS size: only thread 0 owns a second atom
    2049 atoms   <1024, 3>: only thread 0 owns a third atom
    3072 atoms   <1024, 3> without padding: the last thread's third atom is atom 3071

Everything runs through mstep.md (one 'run 20' from explicit velocities) against
oracle.mstep_md, with the bound of test_mstep_gpu.test_gpu_md_segment_tracks_oracle:
positions within 1e-3 max(1, moved), velocities rtol 1e-3, atol 1e-3 max|v|.

Vote.  Beads of radius 100 at rest on a cubic lattice of spacing 400, skin 100: the list
cut is 2 x 100 + 100 = 300, so nothing is in any list and nothing interacts.  One bullet
bead starts 350 from its lattice neighbour and flies at it with |v| = 160: 40 per step at
dt = 0.25, past skin / 2 = 50 every second step, and it is the only thread whose vote is
ever 1 until the collision.  The target is outside the bullet's list at the setup build
(350 > 300); the pair overlaps (r < 200) from step 4 on.  With evf = 1 the barrier of the
soft pair potential, 2 (200 / pi)^2 = 8106, is above the collision's kinetic energy in the
centre-of-mass frame, 160^2 / 4 = 6400, so the bullet bounces: it hands its velocity to
the target.  A lost or mis-combined vote leaves the list of step 0 in place, and the
bullet flies free.  Each case first checks on the CPU that the oracle's bullet ends at
least 100 comparison tolerances away from free flight.

Thermostat.  Random models of tests/small_models.py (bonds, overlaps, one envelope), T = 50
velocities, 20 steps: a window that is never left (the factor is exactly 1: bitwise the run
with an unbounded window), fraction 1 and 0.5, a ramp to its last step, T = 0 with no
forces, and FIXED beads (dof below 3 N - 3).
"""
import numpy as np
import pytest

import oracle
import small_models as sm
from igm_amd import _lib
from igm_amd import model as M
from igm_amd._lib import bond_dtype

pytestmark = pytest.mark.gpu

NSTEPS = 20
DT = 0.25  # params.timestep of the demo protocol
XMAX = 1000.0
SIZES = (1025, 2049, 3072)
NO_ENVELOPE = [((1.0e6, 1.0e6, 1.0e6), 1.0)]  # k > 0 acts outside only: no bead ever gets there


@pytest.fixture(scope='module')
def ms():
    from igm_amd import mstep
    return mstep


def _prm(prm, **kw):
    p = _lib.MStepParams.from_buffer_copy(prm)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _check(tag, x, xg, vg, xo, vo):
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


# ------------------------------------------------------------------ lattice (no interactions)
SPACING, RADIUS, SKIN, SPEED, START = 400.0, 100.0, 100.0, 160.0, 350.0


def _lattice(natom):
    """natom beads (no dummy) at rest on a cubic lattice wider than the list cut, no bonds"""
    n = int(np.ceil(natom ** (1.0 / 3.0) - 1e-9))
    i = np.arange(natom)
    x = np.stack([i % n, (i // n) % n, i // (n * n)], axis=1).astype(np.float64) * SPACING
    x -= x.mean(axis=0).round()
    atoms = M.Atoms(np.full(natom, RADIUS, np.float32), n_static_dummies=0)
    prm = M.params_from_cfg({'optimization': {'optimizer_options': sm.DEMO_PROTOCOL}}, NO_ENVELOPE, skin=SKIN)
    assert prm.timestep == DT
    return n, atoms, prm, x.astype(np.float32)[None], np.zeros(0, bond_dtype)


def _bullets():
    out = []
    for natom in SIZES:
        for b in sorted({0, 1023, 1024, natom - 1}):
            out.append((natom, b))
    return out


_ORACLE = {}


def _bullet_case(natom, b):
    """model, x, v and the oracle's trajectory end of bullet b (computed once per case)"""
    if (natom, b) not in _ORACLE:
        n, atoms, prm, x, poly = _lattice(natom)
        prm = _prm(prm, t_window=1.0e30)  # no rescale: free flight is exact
        # the target: the +x lattice neighbour, or the -x one at the end of a row / of the atoms
        d = 1 if (b % n != n - 1 and b + 1 < natom) else -1
        assert 0 <= b + d < natom and (b + d) // n == b // n
        x = x.copy()
        x[0, b, 0] = x[0, b + d, 0] - d * START
        v = np.zeros_like(x)
        v[0, b, 0] = d * SPEED
        xo, vo = oracle.mstep_md(prm, x.astype(np.float64), v.astype(np.float64), atoms.radii, atoms.flags, poly, None,
                                 None, 1.0, 1.0, 50.0, 50.0, XMAX, NSTEPS)
        _ORACLE[(natom, b)] = (atoms, prm, poly, x, v, d, xo, vo)
    return _ORACLE[(natom, b)]


@pytest.mark.parametrize('natom,b', _bullets())
def test_gpu_vote_of_one_thread_rebuilds_the_list(ms, natom, b):
    """The bullet's owner: lane 0 of wave 0 (atom 0), lane 63 of wave 15 (1023), thread 0's
    second atom (1024) and the last atom (thread 0's second or third atom at 1025 and 2049,
    the last thread's third at 3072)."""
    atoms, prm, poly, x, v, d, xo, vo = _bullet_case(natom, b)
    # power, on the CPU: a stale list (free flight) is far outside the comparison's tolerance
    free_x = x[0, b, 0] + d * SPEED * DT * NSTEPS
    vtol = 2e-3 * np.abs(vo).max()  # >= rtol |v| + atol at every component
    xtol = 1e-3 * max(1.0, np.abs(xo - x).max())
    print('natom %d bullet %d (dir %+d): oracle v_x %.4g (free %.4g, tol %.3g), x %.5g (free %.5g, tol %.3g)' % (
        natom, b, d, vo[0, b, 0], d * SPEED, vtol, xo[0, b, 0], free_x, xtol))
    assert abs(vo[0, b, 0] - d * SPEED) >= 100.0 * vtol
    assert abs(xo[0, b, 0] - free_x) >= 100.0 * xtol
    assert abs(vo[0, b + d, 0]) >= 100.0 * vtol  # the target took the momentum
    xg, vg = ms.md(prm, x, v, atoms.radii, atoms.flags, poly, None, None, 1.0, 1.0, 50.0, 50.0, XMAX, NSTEPS)
    _check('natom %d bullet %d' % (natom, b), x, xg, vg, xo, vo)


@pytest.mark.parametrize('natom', SIZES)
def test_gpu_thermostat_at_zero_temperature(ms, natom):
    """All velocities zero and no forces: T = 0, the factor is 1 (no 0 / 0), nothing moves."""
    n, atoms, prm, x, poly = _lattice(natom)
    v = np.zeros_like(x)
    xg, vg = ms.md(prm, x, v, atoms.radii, atoms.flags, poly, None, None, 1.0, 1.0, 50.0, 40.0, XMAX, NSTEPS)
    assert np.all(np.isfinite(xg)) and np.all(np.isfinite(vg))
    assert np.array_equal(xg, x) and not vg.any()
    xo, vo = oracle.mstep_md(prm, x.astype(np.float64), v.astype(np.float64), atoms.radii, atoms.flags, poly, None, None,
                             1.0, 1.0, 50.0, 40.0, XMAX, NSTEPS)
    assert np.array_equal(xo, x.astype(np.float64)) and not vo.any()


# ------------------------------------------------------------------ thermostat, interacting models
_MODELS = {}


def _model(natom, fixed=False):
    """2 structures of a random model (one envelope: flags (N,)), T = 50 velocities"""
    if (natom, fixed) not in _MODELS:
        atoms, poly, prm, ptr, sb, x = sm.make(natom - 1, 2, 2000 + natom, envelopes=sm.ENV_ONE)
        if fixed:  # every 7th bead held: the mobile count, and with it dof, is not natom - 1
            atoms.flags[np.arange(3, natom - 1, 7)] |= np.uint32(M.IGM_ATOM_FIXED)
        v = np.stack([oracle.velocity_create(atoms.flags, 50.0, 21 + s) for s in range(2)]).astype(np.float32)
        assert not v[:, atoms.flags & M.IGM_ATOM_FIXED != 0].any()
        _MODELS[(natom, fixed)] = (atoms, poly, prm, ptr, sb, x, v)
    return _MODELS[(natom, fixed)]


_RUNS = {}


def _oracle_md(natom, fixed, window, fraction, t0, t1):
    key = (natom, fixed, window, fraction, t0, t1)
    if key not in _RUNS:
        atoms, poly, prm, ptr, sb, x, v = _model(natom, fixed)
        p = _prm(prm, t_window=window, t_fraction=fraction)
        _RUNS[key] = oracle.mstep_md(p, x.astype(np.float64), v.astype(np.float64), atoms.radii, atoms.flags, poly, ptr,
                                     sb, sm.EVF, sm.ENVF, t0, t1, XMAX, NSTEPS, nthreads=4)
    return _RUNS[key]


def _gpu_md(ms, natom, fixed, window, fraction, t0, t1):
    atoms, poly, prm, ptr, sb, x, v = _model(natom, fixed)
    p = _prm(prm, t_window=window, t_fraction=fraction)
    return ms.md(p, x, v, atoms.radii, atoms.flags, poly, ptr, sb, sm.EVF, sm.ENVF, t0, t1, XMAX, NSTEPS)


def _temperature(v, flags):
    """compute temp of group nonfixed: sum v^2 / (3 n_mobile - 3), per structure"""
    mobile = flags & M.IGM_ATOM_FIXED == 0
    return (np.asarray(v, np.float64)[:, mobile] ** 2).sum(axis=(1, 2)) / (3.0 * mobile.sum() - 3.0)


@pytest.mark.parametrize('natom', SIZES)
def test_gpu_thermostat_inside_the_window_is_exactly_off(ms, natom):
    """|T - target| stays inside the window: the factor is exactly 1 at every step, so the run
    is bitwise the run with an unbounded window.  On the CPU first: the oracle agrees that the
    window (1e7: the overlapping start heats the model to T ~ 6e5) is never left, and that the default window (0.1) is, so the branch matters."""
    xw, vw = _oracle_md(natom, False, 1.0e7, 1.0, 50.0, 50.0)
    xu, vu = _oracle_md(natom, False, 1.0e30, 1.0, 50.0, 50.0)
    xd, vd = _oracle_md(natom, False, 0.1, 1.0, 50.0, 50.0)
    assert np.array_equal(xw, xu) and np.array_equal(vw, vu)
    assert np.abs(vd - vu).max() > 0.2 * np.abs(vu).max()
    xg, vg = _gpu_md(ms, natom, False, 1.0e7, 1.0, 50.0, 50.0)
    xh, vh = _gpu_md(ms, natom, False, 1.0e30, 1.0, 50.0, 50.0)
    assert np.array_equal(xg, xh) and np.array_equal(vg, vh)
    _check('natom %d inside the window' % natom, _model(natom)[5], xg, vg, xw, vw)


@pytest.mark.parametrize('fraction', [1.0, 0.5])
@pytest.mark.parametrize('natom', SIZES)
def test_gpu_thermostat_fraction(ms, natom, fraction):
    """Constant target 50, window 0.1: rescaled all the way (1.0) or half way (0.5)."""
    xo, vo = _oracle_md(natom, False, 0.1, fraction, 50.0, 50.0)
    xg, vg = _gpu_md(ms, natom, False, 0.1, fraction, 50.0, 50.0)
    _check('natom %d fraction %g' % (natom, fraction), _model(natom)[5], xg, vg, xo, vo)
    if fraction == 1.0:  # the last step's rescale put T at the target, or found it inside the window
        T = _temperature(vg, _model(natom)[0].flags)
        print('final T', T)
        assert np.all(np.abs(T - 50.0) <= 0.1 + 1e-3 * 50.0)


@pytest.mark.parametrize('fixed', [False, True])
@pytest.mark.parametrize('natom', SIZES)
def test_gpu_thermostat_ramp_to_its_last_step(ms, natom, fixed):
    """t0 = 50 to t1 = 40 over the 20 steps: the target of step k is 50 - k / 2, and the last
    step's is t1 itself (delta = nsteps / nsteps).  With FIXED beads the temperature counts the
    mobile atoms only: a wrong dof would leave the final T off 40 by its ratio (14 %)."""
    atoms = _model(natom, fixed)[0]
    xo, vo = _oracle_md(natom, fixed, 0.1, 1.0, 50.0, 40.0)
    xg, vg = _gpu_md(ms, natom, fixed, 0.1, 1.0, 50.0, 40.0)
    _check('natom %d ramp%s' % (natom, ' with FIXED beads' if fixed else ''), _model(natom, fixed)[5], xg, vg, xo, vo)
    held = atoms.flags & M.IGM_ATOM_FIXED != 0
    assert held.sum() == (1 + len(np.arange(3, natom - 1, 7)) if fixed else 1)
    assert np.array_equal(xg[:, held], _model(natom, fixed)[5][:, held]) and not vg[:, held].any()
    T = _temperature(vg, atoms.flags)
    print('final T', T, 'oracle', _temperature(vo, atoms.flags))
    assert np.all(np.abs(T - 40.0) <= 0.1 + 1e-3 * 40.0)
