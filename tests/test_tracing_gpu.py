"""Position anchors (chromatin tracing) in the M-step engines, on the MI355X.

The independent reference is the reference's own formulation on the unchanged fp64 oracle
(tests/tracing.dummy_form: one IGM_ATOM_FIXED atom per anchor appended after all atoms, plus
a bond), and the numpy anchor term on top of small_models.brute_forces; tests/test_tracing.py
pins the two to each other on the CPU and holds every force input to the f32 headroom.

Engines by natom (tests/test_mstep_sizes_gpu.py): 1 .. 1024 the population engine, 1025 ..
3072 the LDS kernels, 3073 and up the population engine; 'global' = IGM_MSTEP_FORCE_GLOBAL.
Tolerances are the project's own:
    f64 forces   max|d| <= 1e-6 max|F_ref| + 1e-6        energies   rtol 1e-9
    f32 forces   ||err|| <= 1e-5 ||F_ref|| over the beads (coincident / one_cell: per atom,
                 err_i <= 1e-5 x the summed magnitudes of the atom's terms)
    md segment   max|dx| < 1e-3 max(1, moved)
"""
import json
import os

import numpy as np
import pytest

import oracle
import small_models as sm
import tracing as TR
from igm_amd import _lib
from igm_amd import assemble as A
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


def _reference(natom, geometry, envelopes):
    """(model, anchors, oracle (f, e) on the dummy-atom form, brute (f, e, parts) or None),
    computed once.  The numpy reference (O(N^2)) is kept to the 257-atom geometries."""
    key = (natom, geometry, len(envelopes))
    if key not in _REFS:
        model = sm.case(natom, geometry, envelopes)
        atoms, poly, prm, ptr, sb, x = model
        aptr, anch = TR.anchor_sets(x, natom, 1000 + natom)
        d = TR.dummy_form(atoms.radii, atoms.flags, poly, ptr, sb, x, aptr, anch)
        fo, eo = oracle.mstep_forces(prm, d[5], d[0], d[1], d[2], d[3], d[4], EVF, ENVF, nthreads=4)
        brute = None
        if natom <= 257:
            brute = TR.brute_batch(atoms, poly, ptr, sb, x, envelopes, EVF, ENVF, aptr, anch, parts=True)
        _REFS[key] = (model, (aptr, anch), (fo[:, :natom], eo), brute)
    return _REFS[key]


# ------------------------------------------------------------------ 1. forces
FORCE_CASES = [(n, 'random', 'default') for n in (3, 64, 65, 1025, 3072, 3073)] + \
              [(257, g, e) for g in sm.GEOMETRIES for e in ('default', 'global')]


@pytest.mark.parametrize('natom,geometry,engine', FORCE_CASES)
def test_gpu_anchor_forces(ms, natom, geometry, engine):
    """f64 path (forces and energies, the anchor energy in the bond column) and f32 path of
    both engines against the oracle on the dummy-atom form; at 257 atoms also against numpy."""
    (atoms, poly, prm, ptr, sb, x), (aptr, anch), (fo, eo), brute = _reference(natom, geometry, sm.ENV_TWO)
    p = _engine(prm, engine)
    nb = natom - 1
    tag = 'natom %d %s %s' % (natom, geometry, engine)
    fg, eg = ms.forces(p, x, atoms.radii, atoms.flags, poly, ptr, sb, EVF, ENVF, anchors=(aptr, anch))
    for name, (fr, er) in (('oracle', (fo, eo[:, :5])),) + \
            ((('brute', (brute[0], np.concatenate([brute[1].sum(axis=1, keepdims=True), brute[1]], axis=1))),)
             if brute is not None else ()):
        scale = np.abs(fr).max()
        print('%s vs %s: f64 max|dF| %.3g (bound %.3g), max rel dE %.3g' % (
            tag, name, np.abs(fg - fr).max(), 1e-6 * scale + 1e-6,
            (np.abs(eg[:, :5] - er) / np.maximum(np.abs(er), 1e-300)).max()))
        assert np.all(np.isfinite(fg)) and np.all(np.isfinite(eg[:, :5]))
        assert np.abs(fg - fr).max() <= 1e-6 * scale + 1e-6
        assert np.allclose(eg[:, :5], er, rtol=1e-9, atol=0.0)
    assert np.all(fg[:, nb] == 0.0)  # the fixed dummy: anchored in structure 2, energy but no force
    assert eg[2, 2] > eg[1, 2]
    # ---- the f32 path ('line': the k > 0 envelope alone, small_models.f32_envelopes)
    env = sm.f32_envelopes(geometry)
    if env is not sm.ENV_TWO:
        (atoms, poly, prm, ptr, sb, x), (aptr, anch), (fo, eo), brute = _reference(natom, geometry, env)
        p = _engine(prm, engine)
    f32, _ = ms.forces(p, x, atoms.radii, atoms.flags, poly, ptr, sb, EVF, ENVF, f32=True, anchors=(aptr, anch))
    assert np.all(np.isfinite(f32)) and np.all(f32[:, nb] == 0.0)  # no NaN at r = 0
    if geometry in ('coincident', 'one_cell'):
        err = np.linalg.norm(f32 - brute[0], axis=2)[:, :nb]
        bound = 1e-5 * sm.term_magnitudes(brute[2], geometry)[:, :nb]
        print('%s: f32 per-atom worst err/bound %.3g' % (tag, (err[bound > 0] / bound[bound > 0]).max()))
        assert np.all(err <= bound)
    else:
        err = np.linalg.norm(f32 - fo, axis=2)[:, :nb]
        ref = np.linalg.norm(fo, axis=2)[:, :nb]
        print('%s: f32 ||err|| %.3g (bound %.3g)' % (tag, np.linalg.norm(err), 1e-5 * np.linalg.norm(ref)))
        assert np.linalg.norm(err) <= 1e-5 * np.linalg.norm(ref)


# ------------------------------------------------------------------ 2. md segment
def _md_model(natom):
    model = sm.make(natom - 1, 3, 1000 + natom, envelopes=sm.ENV_TWO, empty_rows=(1,))
    return model, TR.anchor_sets(model[5], natom, 1000 + natom)


def _velocities(atoms, nstruct, seed0=11):
    fl = atoms.flags[0] if atoms.flags.ndim == 2 else atoms.flags
    return np.stack([oracle.velocity_create(fl, 50.0, seed0 + s) for s in range(nstruct)]).astype(np.float32)


@pytest.mark.parametrize('natom,engine', [(257, 'default'), (257, 'global'), (3072, 'default')])
def test_gpu_anchor_md_segment_tracks_oracle(ms, natom, engine):
    """20 steps of nve/limit + temp/rescale from identical x, v (bounds of
    test_gpu_md_segment_tracks_oracle)."""
    (atoms, poly, prm, ptr, sb, x), (aptr, anch) = _md_model(natom)
    v = _velocities(atoms, 3)
    xg, vg = ms.md(_engine(prm, engine), x, v, atoms.radii, atoms.flags, poly, ptr, sb, EVF, ENVF, 50.0, 40.0, 1000.0,
                   20, anchors=(aptr, anch))
    r2, f2, p2, ptr2, sb2, x2 = TR.dummy_form(atoms.radii, atoms.flags, poly, ptr, sb, x, aptr, anch)
    v2 = np.zeros(x2.shape, np.float64)
    v2[:, :natom] = v
    xo, vo = oracle.mstep_md(prm, x2.astype(np.float64), v2, r2, f2, p2, ptr2, sb2, EVF, ENVF, 50.0, 40.0, 1000.0, 20,
                             nthreads=4)
    xo, vo = xo[:, :natom], vo[:, :natom]
    xf, _ = oracle.mstep_md(prm, x.astype(np.float64), v.astype(np.float64), atoms.radii, atoms.flags, poly, ptr, sb,
                            EVF, ENVF, 50.0, 40.0, 1000.0, 20, nthreads=4)
    moved = np.abs(xo - x).max()
    print('natom %d %s: moved %.3g, max|dx| %.3g, anchors moved the oracle by %.3g' % (
        natom, engine, moved, np.abs(xg - xo).max(), np.abs(xo - xf).max()))
    assert moved > 1.0 and np.abs(xo - xf).max() > 1.0  # it moved, and the anchors matter
    assert np.all(np.isfinite(xg)) and np.all(np.isfinite(vg))
    assert np.abs(xg - xo).max() < 1e-3 * max(1.0, moved)
    assert np.allclose(vg, vo, rtol=1e-3, atol=1e-3 * np.abs(vo).max())


# ------------------------------------------------------------------ 3. anchors follow their atoms
def _short_protocol(steps=(300, 300, 300, 300), relax=100):
    p = json.loads(json.dumps(syn.DEMO_PROTOCOL))
    p['custom_annealing_protocol']['mdsteps'] = list(steps)
    p['custom_annealing_protocol']['relax']['mdsteps'] = relax
    return p


@pytest.fixture(scope='module')
def follow():
    """256 beads, no random bonds, the short protocol; anchors on every 4th bead of structure s
    at those beads' positions in structure (s + 1) % 3 of an anchor-free oracle run from
    seeds + 5 -- reachable targets far from where the atoms start and from where the sort puts
    them.  The oracle's anchored run (dummy-atom form) is the reference."""
    atoms, poly, prm, ptr, sb, x = sm.make(256, 3, 7, nbonds=0, protocol=_short_protocol())
    seeds = M.lammps_seeds(6535, [0, 1, 2], 3)
    xfree, _, _ = oracle.mstep_run(prm, x.copy(), atoms.radii, atoms.flags, poly, ptr, sb, seeds + 5, nthreads=3)
    beads = np.arange(0, 256, 4)
    aptr, anch = TR.make_anchors([(beads, xfree[(s + 1) % 3, beads]) for s in range(3)])
    start = np.concatenate([np.linalg.norm(TR.targets_of(anch[aptr[s]:aptr[s + 1]]) - x[s, beads], axis=1)
                            for s in range(3)])
    d = TR.dummy_form(atoms.radii, atoms.flags, poly, ptr, sb, x, aptr, anch)
    xo, io, _ = oracle.mstep_run(prm, d[5].copy(), d[0], d[1], d[2], d[3], d[4], seeds, nthreads=3)
    xf, _, _ = oracle.mstep_run(prm, x.copy(), atoms.radii, atoms.flags, poly, ptr, sb, seeds, nthreads=3)
    return (atoms, poly, prm, ptr, sb, x), seeds, (aptr, anch), start, (xo[:, :257], io), xf


def test_follow_case_is_what_it_claims(follow):
    """the oracle on this input: far starts, anchored run well inside the tolerance, the
    anchor-free run leaves the anchors violated"""
    model, seeds, (aptr, anch), start, (xo, io), xf = follow
    ro = np.concatenate([TR.anchor_ratios(xo[s], anch[aptr[s]:aptr[s + 1]]) for s in range(3)])
    rf = np.concatenate([TR.anchor_ratios(xf[s], anch[aptr[s]:aptr[s + 1]]) for s in range(3)])
    print('start distance min %.0f, oracle anchored max ratio %.4f, anchor-free violated %.2f, rebuilds %s' % (
        start.min(), ro.max(), np.mean(rf > 0.05), io['nrebuild'].tolist()))
    # every anchor starts at least 4 r0 from its target (sigma 700 coordinates: most start > 1000 away)
    assert start.min() > 4 * TR.R0 and np.median(start) > 1000.0 and ro.max() < 0.05 and np.mean(rf > 0.05) > 0.9


@pytest.mark.parametrize('engine,env', [('default', {}), ('global', {}), ('global', {'IGM_POP_BOND_PRUNE': '0'})],
                         ids=['default', 'global', 'global-noprune'])
def test_gpu_anchors_follow_their_atoms(ms, follow, engine, env):
    (atoms, poly, prm, ptr, sb, x), seeds, anchors, start, (xo, io), xf = follow
    p = _engine(prm, engine)

    def run():
        return ms.run(p, x, atoms.radii, atoms.flags, poly, ptr, sb, seeds, anchors=anchors)
    xg, ig = _with_env(env, run)
    xg2, ig2 = _with_env(env, run)
    assert np.array_equal(xg, xg2) and ig.tobytes() == ig2.tobytes()  # a rerun is bitwise equal
    rec = ms.anchor_violations(xg, 0.05, anchors)
    print('%s %s: rebuilds %s, violated_restr %s, n_violations %s, temp gpu %s oracle %s' % (
        engine, env, ig['nrebuild'].tolist(), rec[:, 101].tolist(), rec[:, 102].tolist(),
        ig['temp'].round(4).tolist(), io['temp'].round(4).tolist()))
    assert np.all(ig['nrebuild'] >= 2)
    assert np.array_equal(rec, TR.anchor_record(xg, anchors[0], anchors[1], 0.05))  # bin for bin
    assert np.all(rec[:, 103] == 64) and np.all(rec[:, 102] == 0)  # every anchor pulled its own atom home
    # thermo temp at the end of the protocol (test_gpu_full_protocol_short: < 0.2)
    assert np.all(ig['temp'] < 0.2) and np.all(np.abs(ig['temp'] - io['temp']) < 0.2)


# ------------------------------------------------------------------ 4. CG, energies, thermo temp
@pytest.mark.parametrize('engine', ['default', 'global'])
def test_gpu_anchor_cg_matches_oracle(ms, engine):
    (atoms, poly, prm, ptr, sb, x), (aptr, anch) = _md_model(257)
    p = _engine(prm, engine)
    p.nstages = 0
    seeds = M.lammps_seeds(6535, [0, 1, 2], 11)
    xg, ig = ms.run(p, x, atoms.radii, atoms.flags, poly, ptr, sb, seeds, anchors=(aptr, anch))
    d = TR.dummy_form(atoms.radii, atoms.flags, poly, ptr, sb, x, aptr, anch)
    po = _lib.MStepParams.from_buffer_copy(prm)
    po.nstages = 0
    xo, io, _ = oracle.mstep_run(po, d[5].copy(), d[0], d[1], d[2], d[3], d[4], seeds, nthreads=3)
    print('%s: einitial %s, final gpu %s oracle %s' % (engine, ig['einitial'].round(1).tolist(),
                                                      ig['final_energy'].round(3).tolist(),
                                                      io['final_energy'].round(3).tolist()))
    assert np.allclose(ig['einitial'], io['einitial'], rtol=1e-10)
    assert np.allclose(ig['final_energy'], io['final_energy'], rtol=1e-5)
    assert np.allclose(ig['bond_energy'], io['bond_energy'], rtol=1e-5)
    assert np.all(ig['final_energy'] < ig['einitial'])


@pytest.mark.parametrize('engine', ['default', 'global'])
def test_gpu_thermo_temp_counts_the_anchors(ms, engine):
    """info.temp is the thermo temperature of group all with every anchor counted as one more
    motionless atom.  One stage of 20 steps held at T = 50 and no CG iterations: the
    temperature of the beads is ~50, so info.temp is ~50 x dof_nonfixed / dof_all and the two
    conventions (anchors counted or not) differ by (natom + n_anchor) / natom -- 2x in
    structure 2, 1.26x in structure 0, nothing in structure 1.  (igm_mstep_md returns no
    temperature; the one-stage igm_mstep_run is the shortest call that does.)"""
    (atoms, poly, prm, ptr, sb, x), (aptr, anch) = _md_model(257)
    natom = 257

    def one_stage(q):
        q = _lib.MStepParams.from_buffer_copy(q)
        q.nstages, q.relax_steps, q.max_cg_iter = 1, 0, 0
        q.mdsteps[0], q.tstart[0], q.tstop[0], q.evfactor[0], q.envfactor[0] = 20, 50.0, 50.0, 1.0, 1.0
        return q
    seeds = M.lammps_seeds(6535, [0, 1, 2], 11)
    _, ig = ms.run(one_stage(_engine(prm, engine)), x, atoms.radii, atoms.flags, poly, ptr, sb, seeds,
                   anchors=(aptr, anch))
    _, i0 = ms.run(one_stage(_engine(prm, engine)), x, atoms.radii, atoms.flags, poly, ptr, sb, seeds)
    d = TR.dummy_form(atoms.radii, atoms.flags, poly, ptr, sb, x, aptr, anch)
    _, io, _ = oracle.mstep_run(one_stage(prm), d[5].copy(), d[0], d[1], d[2], d[3], d[4], seeds, nthreads=3)
    n = np.diff(aptr)
    m = int(n.max())  # the dummy form appends max(n) atoms to every structure
    want = io['temp'] * (3.0 * (natom + m) - 3.0) / (3.0 * (natom + n) - 3.0)
    print('%s: temp gpu %s, oracle (own atom count) %s, without anchors %s' % (
        engine, ig['temp'].round(3).tolist(), want.round(3).tolist(), i0['temp'].round(3).tolist()))
    assert np.all(want > 10.0)
    assert np.allclose(ig['temp'], want, rtol=2e-3)
    other = ig['temp'] * (3.0 * (natom + n) - 3.0) / (3.0 * natom - 3.0)  # the convention without anchors
    assert np.all(np.abs(other - want)[n > 0] > 0.2 * want[n > 0])


# ------------------------------------------------------------------ 5. staging
def test_gpu_anchor_staging(ms):
    (atoms, poly, prm, ptr, sb, x), (aptr, anch) = _md_model(65)
    p = _lib.MStepParams.from_buffer_copy(prm)
    p.nstages = 2
    for k in range(2):
        p.mdsteps[k] = 40
    p.relax_steps = 10
    seeds = M.lammps_seeds(6535, [0, 1, 2], 3)
    c = _lib.context(0)

    def run(anchors=None):
        xo, info = ms.run(p, x, atoms.radii, atoms.flags, poly, ptr, sb, seeds, anchors=anchors)
        f, e = ms.forces(p, xo, atoms.radii, atoms.flags, poly, ptr, sb, EVF, ENVF, anchors=anchors)
        return xo.tobytes() + info.tobytes() + f.tobytes() + e.tobytes()
    never = run()
    with_anchors = run((aptr, anch))
    assert with_anchors != never
    assert run() == never  # staged, then cleared
    assert run((np.zeros(4, np.int64), anch[:0])) == never  # every row empty
    # ---- errors, each leaving the context usable
    args = (p, x, atoms.radii, atoms.flags, poly, ptr, sb, EVF, ENVF)
    four = np.concatenate([aptr, aptr[-1:]])
    c.check(c.lib.igm_mstep_set_anchors(c.h, 4, four.ctypes.data, anch.ctypes.data), 'igm_mstep_set_anchors')
    try:
        with pytest.raises(RuntimeError, match=r'code %d\).*staged for 4 structures, batch has 3' % _lib.IGM_E_INVALID):
            ms.forces(*args)
        out = np.zeros((3, 104), np.int64)
        with pytest.raises(RuntimeError, match='staged for 4 structures, batch has 3'):
            c.check(c.lib.igm_mstep_anchor_violations(c.h, 0, 3, 65, x.ctypes.data, 0.05, out.ctypes.data),
                    'igm_mstep_anchor_violations')
    finally:
        c.lib.igm_mstep_set_anchors(c.h, 0, None, None)
    bad = anch.copy()
    bad['atom'][3] = 65
    with pytest.raises(RuntimeError, match=r'code %d\).*atom 65 >= natom 65' % _lib.IGM_E_INVALID):
        ms.forces(*args, anchors=(aptr, bad))
    for field, value, what in (('y', np.nan, 'non-finite target'), ('x', np.inf, 'non-finite target'),
                               ('r0', -1.0, 'r0 < 0'), ('k', np.nan, 'non-finite r0 or k')):
        bad = anch.copy()
        bad[field][5] = value
        with pytest.raises(RuntimeError, match=r'code %d\).*anchor 5 has a?n? ?%s' % (_lib.IGM_E_INVALID, what)):
            ms.forces(*args, anchors=(aptr, bad))
    down = aptr.copy()
    down[1], down[2] = down[2], down[1] - 1
    with pytest.raises(RuntimeError, match='not monotone'):
        ms.forces(*args, anchors=(down, anch))
    assert run() == never and run((aptr, anch)) == with_anchors


# ------------------------------------------------------------------ 6. the product path
def test_gpu_assemble_run_with_tracing(ms):
    """assemble.build + assemble.run on 4 demo structures with a tracing spec equals the
    direct mstep.run + anchor_violations; the record is the trailing class 'Tracing'."""
    import nuclear_bodies as NB
    from conftest import load_golden
    pop = load_golden('demo_population.npz')
    xyz = np.ascontiguousarray(pop['coordinates'][:, :4].transpose(1, 0, 2), np.float32)
    nbead = xyz.shape[1]
    rng = np.random.default_rng(21)
    locus = np.concatenate([np.sort(rng.choice(nbead, 40, replace=False)) for _ in range(3)])
    data = {'locus': locus, 'assignment': np.repeat([0, 1, 3], 40),
            'target': xyz[np.repeat([0, 1, 3], 40), locus] + rng.normal(0.0, 400.0, (120, 3))}
    spec = {'evfactor': 1.0, 'protocol': {'mdsteps': 40, 'tstart': 1, 'tstop': 1},
            'polymer': {'contact_range': 2.0, 'kspring': 1.0},
            'envelope': A.envelope_spec('sphere', radius=5500.0), 'tracing': {'data': data, 'tol': 100.0, 'k': 1.0}}
    ctx = _lib.context(0)
    b = A.build(xyz, np.arange(4), NB.index_of(pop), spec, ctx)
    assert b.names[-1] == 'Tracing' and len(b.names) == A.NCLASS + 2 and b.natom == nbead + 1  # no atoms added
    assert b.anchor_ptr.tolist() == [0, 40, 80, 80, 120]
    seeds = M.lammps_seeds(6535, np.arange(4), 1)
    xo, info, stats = A.run(b, seeds, 0.05, ctx)
    anchors = (b.anchor_ptr, b.anchors)
    xd, idd = ms.run(b.prm, b.x, b.radii, b.flags, b.poly, b.ptr, b.bonds, seeds, ctx=ctx, anchors=anchors)
    assert np.array_equal(xo, xd) and info.tobytes() == idd.tobytes()
    rec = ms.anchor_violations(xo, 0.05, anchors, ctx=ctx)
    assert stats.shape == (4, A.NCLASS + 2, 104) and np.array_equal(stats[:, -1], rec)
    assert rec[:, 103].tolist() == [40, 40, 0, 40]
    assert np.array_equal(rec, TR.anchor_record(xo, b.anchor_ptr, b.anchors, 0.05))
    xn, _ = ms.run(b.prm, b.x, b.radii, b.flags, b.poly, b.ptr, b.bonds, seeds, ctx=ctx)
    assert not np.array_equal(xn[0], xo[0])  # the anchors act
