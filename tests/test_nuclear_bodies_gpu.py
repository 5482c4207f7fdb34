"""DamID and nuclear bodies on imaged nuclei (exp_map) in the M-step, on the MI355X:
igm_volume_select and shape 3 of igm_damid_actdist bit-exact against the reference
goldens; the per-envelope map tables of igm_mstep_set_envelope_maps in the forces of both
engines (against a NumPy statement of the documented form and against the fp64 oracle
used one map at a time), in the violation records, in a short protocol and in one
igm-run iteration through the Step classes."""
import json

import numpy as np
import pytest

import mstep_fixtures as F
import nuclear_bodies as NB
import oracle
from conftest import load_golden
from igm_amd import _lib
from igm_amd import assemble as A
from igm_amd import model as M
from igm_amd import volume as V
from igm_amd._lib import (IGM_ATOM_BEAD, IGM_ATOM_ENV0, IGM_ATOM_FIXED, IGM_MSTEP_FORCE_GLOBAL, MStepParams,
                          damid_row_dtype)
from oracle import volume as OV

pytestmark = pytest.mark.gpu

NBEAD = 3008
SHORT = {'mdsteps': 10, 'tstart': 1, 'tstop': 1}


@pytest.fixture(scope='module')
def gold():
    return load_golden('nuclear_bodies_golden.npz')


@pytest.fixture(scope='module')
def maps():
    return NB.golden_maps()


@pytest.fixture
def ctx():
    c = _lib.context(0)
    yield c
    V.stage(c, [])  # clears the maps and every per-envelope table


def _rows(loc, dist):
    r = np.zeros(len(loc), damid_row_dtype)
    r['loc'], r['dist'] = loc, dist
    return r


def _engine(prm, engine):
    p = MStepParams.from_buffer_copy(prm)
    if engine == 'global':
        p.flags |= IGM_MSTEP_FORCE_GLOBAL
    return p


# ---------------------------------------------------------------- 1. igm_volume_select
def _want_flags(gold, pick, base, bit):
    """base | bit for the beads with a selected row; pick[s] = the golden map of structure s"""
    out = np.repeat(base[None], len(pick), 0) if base.ndim == 1 else base.copy()
    nsel = np.zeros(len(pick), np.int32)
    for s, m in enumerate(pick):
        sel = gold['sel_b%d' % m][s]
        out[s, gold['loc'][sel]] |= np.uint32(bit)
        nsel[s] = sel.sum()
    return out, nsel


def test_volume_select_equals_reference(gold, maps, ctx):
    from igm_amd import restraints as R
    base = np.full(NBEAD, IGM_ATOM_BEAD | IGM_ATOM_ENV0, np.uint32)
    rows = _rows(gold['loc'], gold['dist'])
    bit = IGM_ATOM_ENV0 << 2
    V.stage(ctx, [maps[0], maps[1]], struct_map=[0, 1, 0, 1])
    # S = 1 on each map (explicit pool index), S = 4 alternating (explicit, and the default table)
    for m in (0, 1):
        got, nsel = R.volume_envelope_flags(gold['pos'][:1], rows, [m], 2, base, ctx=ctx)
        want, wn = _want_flags(gold, [m], base, bit)
        assert np.array_equal(got, want) and np.array_equal(nsel, wn)
    want, wn = _want_flags(gold, [0, 1, 0, 1], base, bit)
    for smap in ([0, 1, 0, 1], None):
        got, nsel = R.volume_envelope_flags(gold['pos'], rows, smap, 2, base, ctx=ctx)
        assert np.array_equal(got, want) and np.array_equal(nsel, wn)
    assert 150 < wn.min() and wn.max() < 500
    # nrows = 0: the base flags, nothing selected
    got, nsel = R.volume_envelope_flags(gold['pos'], rows[:0], [0, 1, 0, 1], 2, base, ctx=ctx)
    assert np.array_equal(got, np.repeat(base[None], 4, 0)) and not nsel.any()
    # rows whose loc is outside [0, natom) are ignored
    junk = _rows([-1, NBEAD, 1 << 30, -(1 << 31)], [1e30] * 4)
    mixed = np.concatenate([junk[:2], rows[:300], junk[2:], rows[300:]])
    got, nsel = R.volume_envelope_flags(gold['pos'], mixed, [0, 1, 0, 1], 2, base, ctx=ctx)
    assert np.array_equal(got, want) and np.array_equal(nsel, wn)
    # the lamina selection (own nucleus map, default table) and the nuclear-body one compose on one array
    V.stage(ctx, [maps[0], maps[1]], struct_map=[0, 0, 0, 0])
    lam, _ = R.volume_envelope_flags(gold['pos'], rows, None, 3, base, ctx=ctx)
    both, nsel = R.volume_envelope_flags(gold['pos'], rows, [1, 1, 1, 1], 2, lam, ctx=ctx)
    w3, _ = _want_flags(gold, [0] * 4, base, IGM_ATOM_ENV0 << 3)
    w23, wn = _want_flags(gold, [1] * 4, w3, bit)
    assert np.array_equal(lam, w3) and np.array_equal(both, w23) and np.array_equal(nsel, wn)
    # a pool index outside the staged maps is refused, not read
    with pytest.raises(RuntimeError):
        R.volume_envelope_flags(gold['pos'], rows, [0, 1, 2, 0], 2, base, ctx=ctx)


def test_device_assembly_equals_cpu_assembly(gold, maps, ctx):
    pop = load_golden('demo_population.npz')
    spec = NB.four_envelope_spec(gold, maps)
    want = A.build(gold['pos'], np.arange(4), NB.index_of(pop), spec, None, select=NB.BodiesSelect())
    got = A.build(gold['pos'], np.arange(4), NB.index_of(pop), spec, ctx)
    assert np.array_equal(got.flags, want.flags) and got.names == want.names
    assert bytes(got.prm) == bytes(want.prm)


# ---------------------------------------------------------------- 2. shape 3 of igm_damid_actdist
@pytest.mark.parametrize('it_corr', [0, 1])
def test_nuclear_body_astep_equals_reference(gold, maps, ctx, it_corr):
    from igm_amd import damid
    pop = load_golden('demo_population.npz')
    r = damid.compute_damid_actdist(pop['coordinates'], pop['radii'], pop['copy_ptr'], pop['copy_idx'], gold['a_loci'],
                                    gold['a_pexp'], gold['a_plast'], it_corr, 0.95, 'exp_map_nucl', None, ctx=ctx,
                                    volumes=[maps[1], maps[2]], struct_map=gold['a_volumes_idx'])
    assert np.array_equal(r['loc'], gold['a%d_loc' % it_corr])
    assert np.array_equal(r['dist'].view(np.uint32), gold['a%d_dist' % it_corr].view(np.uint32))
    assert np.array_equal(r['prob'].view(np.uint32), gold['a%d_prob' % it_corr].view(np.uint32))


# ---------------------------------------------------------------- 3-5. four envelopes, two maps per structure
ENV_K = (1.0, 2.0, -0.5, -0.25)  # nucleus, nucleolus, nuclDamID, DamID
ENV_CR = (0.95, 0.95, 0.9, 0.8)  # the contact ranges of the violation scores
NUCLEOLUS = (1, 2, 1)            # pool index of the nucleolus envelopes per structure


@pytest.fixture(scope='module')
def case():
    """3 demo structures pushed partly outside the nucleus map; every bead in the nucleus
    and nucleolus envelopes, 600 random beads per structure in each of the lamina ones"""
    pop, _ = F.load()
    sids = [0, 1, 2]
    natom = NBEAD + 1
    x = F.struct_major(pop, sids, natom)
    x[:, :NBEAD] *= np.float32(1.25)
    radii = np.zeros(natom, np.float32)
    radii[:NBEAD] = pop['radii']
    flags = np.zeros((3, natom), np.uint32)
    flags[:, :NBEAD] = IGM_ATOM_BEAD | IGM_ATOM_ENV0 | (IGM_ATOM_ENV0 << 1)
    flags[:, NBEAD] = IGM_ATOM_FIXED
    rng = np.random.default_rng(5)
    for s in range(3):
        for e in (2, 3):
            flags[s, rng.choice(NBEAD, 600, replace=False)] |= np.uint32(IGM_ATOM_ENV0 << e)
    poly = M.polymer_bonds(pop['chrom'], pop['copy'], pop['radii'], 2.0, 1.0)
    prm = M.params_from_cfg({'optimization': {'optimizer_options': SHORT}}, [('volume', k) for k in ENV_K])
    return dict(x=x, radii=radii, flags=flags, poly=poly, prm=prm, sids=sids)


def _stage_four(ctx, maps):
    V.stage(ctx, maps, struct_map=[0, 0, 0])
    for e in (1, 2):
        V.set_envelope_maps(ctx, e, NUCLEOLUS)


def _map_of(maps, e, s):
    return maps[NUCLEOLUS[s]] if e in (1, 2) else maps[0]


def numpy_volume_forces(x, flags, maps, envf):
    """the form documented in include/igm_hip.h (Volumetric nuclear-body maps), float64"""
    S, N = x.shape[0], x.shape[1]
    f = np.zeros((S, N, 3))
    en = np.zeros((S, 4))
    for s in range(S):
        p = x[s].astype(np.float64)
        for e, k in enumerate(ENV_K):
            vol = _map_of(maps, e, s)
            o = vol['origin'].astype(np.float64) * envf
            g = vol['grid'].astype(np.float64) * envf
            v = np.clip(np.rint((p - o) / g).astype(np.int64), 0, np.asarray(vol['nvoxel']) - 1)
            r = vol['matrice'][v[:, 0], v[:, 1], v[:, 2]]
            outside_ok = (vol['body_idx'] == 0) == (k > 0)
            viol = (r[:, 3] == 0) if outside_ok else (r[:, 3] != 0)
            act = viol & ((flags[s] & (IGM_ATOM_ENV0 << e)) != 0)
            d = p - (o + g * r[:, :3])
            f[s][act] -= abs(k) * d[act]
            en[s, e] = 0.5 * abs(k) * np.sum(d[act] ** 2)
    return f, en


def oracle_forces_by_map(c, maps, envf):
    """the fp64 oracle holds one map per call: the nucleus-map envelopes with the pair and
    bond terms, then per nucleolus map its envelopes alone (evfactor 0, no bonds), summed"""
    S = len(c['sids'])
    remap = lambda fl, a, b: ((fl & np.uint32(0xf)) | np.where(fl & (IGM_ATOM_ENV0 << a), IGM_ATOM_ENV0, 0) |
                              np.where(fl & (IGM_ATOM_ENV0 << b), IGM_ATOM_ENV0 << 1, 0)).astype(np.uint32)
    prm = lambda a, b: M.params_from_cfg({'optimization': {'optimizer_options': SHORT}},
                                         [('volume', ENV_K[a]), ('volume', ENV_K[b])])
    try:
        oracle.set_volume(maps[0])
        f, e = oracle.mstep_forces(prm(0, 3), c['x'], c['radii'], remap(c['flags'], 0, 3), c['poly'], None, None, 1.0,
                                   envf)
        f = f.copy()
        en = np.zeros((S, 4))
        en[:, 0], en[:, 3] = e[:, 3], e[:, 4]
        for m in sorted(set(NUCLEOLUS)):
            ss = [s for s in range(S) if NUCLEOLUS[s] == m]
            oracle.set_volume(maps[m])
            f2, e2 = oracle.mstep_forces(prm(1, 2), c['x'][ss], c['radii'], remap(c['flags'][ss], 1, 2), None, None,
                                         None, 0.0, envf)
            f[ss] += f2
            en[ss, 1], en[ss, 2] = e2[:, 3], e2[:, 4]
    finally:
        oracle.set_volume(None)
    return f, en


def _check(fg, eg, fo, eo, f32):
    assert np.all(eo > 0)  # each of the four envelopes acts
    if f32:
        assert np.linalg.norm(fg - fo) <= 1e-5 * np.linalg.norm(fo)
    else:
        assert np.abs(fg - fo).max() <= 1e-6 * np.abs(fo).max() + 1e-6
        assert np.allclose(eg, eo, rtol=1e-9)


@pytest.fixture(scope='module')
def references(case, maps):
    """computed once: {envf: (numpy envelope forces, energies, oracle total forces, energies)}"""
    out = {}
    for envf in (1.0, 1.1):
        out[envf] = numpy_volume_forces(case['x'], case['flags'], maps, envf) + oracle_forces_by_map(case, maps, envf)
    return out


@pytest.mark.parametrize('engine', ['lds', 'global'])
@pytest.mark.parametrize('f32', [False, True])
@pytest.mark.parametrize('envf', [1.0, 1.1])
def test_forces_of_four_envelopes_on_two_maps(case, maps, references, ctx, envf, f32, engine):
    from igm_amd import mstep
    c = case
    fn, en, fo, eo = references[envf]
    assert np.allclose(en, eo, rtol=1e-9)  # the two references agree on the envelope energies
    _stage_four(ctx, maps)
    prm = _engine(c['prm'], engine)
    # (a) the envelopes alone against the documented form
    fg, eg = mstep.forces(prm, c['x'], c['radii'], c['flags'], None, None, None, 0.0, envf, f32=f32, ctx=ctx)
    _check(fg, eg[:, 3:7], fn, en, f32)
    # (b) everything against the oracle, one map at a time
    fg, eg = mstep.forces(prm, c['x'], c['radii'], c['flags'], c['poly'], None, None, 1.0, envf, f32=f32, ctx=ctx)
    _check(fg, eg[:, 3:7], fo, eo, f32)
    if engine == 'global':  # the population engine gathers in a fixed order
        fg2, eg2 = mstep.forces(prm, c['x'], c['radii'], c['flags'], c['poly'], None, None, 1.0, envf, f32=f32, ctx=ctx)
        assert fg2.tobytes() == fg.tobytes() and eg2.tobytes() == eg.tobytes()


@pytest.mark.parametrize('engine', ['lds', 'global'])
def test_tables_equal_to_the_default_change_nothing(case, maps, ctx, engine):
    """igm_mstep_run with no per-envelope table, and with every table set to the default
    one: the same bits"""
    from igm_amd import mstep
    c = case
    prm = _engine(M.params_from_cfg({'optimization': {'optimizer_options': {'mdsteps': 60, 'tstart': 50, 'tstop': 1}}},
                                    [('volume', k) for k in ENV_K]), engine)
    seeds = M.lammps_seeds(6535, c['sids'], 3)
    default = [0, 1, 0]
    V.stage(ctx, maps[:2], struct_map=default)
    x1, i1 = mstep.run(prm, c['x'], c['radii'], c['flags'], c['poly'], None, None, seeds, ctx=ctx)
    for e in range(4):
        V.set_envelope_maps(ctx, e, default)
    x2, i2 = mstep.run(prm, c['x'], c['radii'], c['flags'], c['poly'], None, None, seeds, ctx=ctx)
    assert np.all(np.isfinite(x1)) and not np.array_equal(x1, c['x'])
    assert x1.tobytes() == x2.tobytes() and i1.tobytes() == i2.tobytes()
    # ... and a table that differs does change the run; NULL restores the default
    V.set_envelope_maps(ctx, 1, [1, 0, 1])
    x3, _ = mstep.run(prm, c['x'], c['radii'], c['flags'], c['poly'], None, None, seeds, ctx=ctx)
    assert x3.tobytes() != x1.tobytes()
    for e in range(4):
        V.set_envelope_maps(ctx, e, None)
    x4, _ = mstep.run(prm, c['x'], c['radii'], c['flags'], c['poly'], None, None, seeds, ctx=ctx)
    assert x4.tobytes() == x1.tobytes()


def test_envelope_map_tables_are_validated(case, maps, ctx):
    from igm_amd import mstep
    c = case
    V.stage(ctx, maps, struct_map=[0, 0, 0])
    with pytest.raises(RuntimeError):
        V.set_envelope_maps(ctx, 1, [1, 3, 1])  # index outside the pool
    with pytest.raises(RuntimeError):
        V.set_envelope_maps(ctx, 4, [0, 0, 0])  # no such envelope
    V.set_envelope_maps(ctx, 1, [1, 2])  # shorter than the batch
    with pytest.raises(RuntimeError):
        mstep.forces(c['prm'], c['x'], c['radii'], c['flags'], None, None, None, 0.0, 1.0, ctx=ctx)
    V.stage(ctx, maps, struct_map=[0, 0, 0])  # staging clears the tables
    mstep.forces(c['prm'], c['x'], c['radii'], c['flags'], None, None, None, 0.0, 1.0, ctx=ctx)


def test_violation_records_of_four_envelopes(case, maps, ctx):
    from igm_amd import mstep
    c = case
    _stage_four(ctx, maps)
    stats = mstep.violations(c['prm'], c['x'], c['radii'], c['flags'], None, None, None, None, None, [0.0],
                             list(ENV_CR), 0.05, ctx=ctx)
    some = 0
    for s in range(3):
        for e, k in enumerate(ENV_K):
            members = np.nonzero(c['flags'][s] & (IGM_ATOM_ENV0 << e))[0]
            scores = OV.exp_envelope_scores(c['x'][s, members], _map_of(maps, e, s), k, ENV_CR[e])
            ref = oracle.violations(scores, 0.05)
            rec = stats[s, 1 + e]
            assert list(rec[:101]) == ref['counts'], (s, e)
            assert rec[101] == ref['violated_restr'] and rec[102] == ref['n_violations'] and rec[103] == len(members)
            some += ref['n_violations'] > 0
    assert some == 12  # every envelope of every structure has violations to count


# ---------------------------------------------------------------- 6. a short protocol
def test_nucleolus_body_excludes_short_protocol(maps, ctx):
    """A short protocol with the nucleus map and a per-structure nucleolus body: the share
    of beads inside the body falls to at most half.  The fp64 oracle, which holds one map,
    run on the nucleolus-only version of this input and protocol (structures 0 and 2 on b1,
    1 and 3 on n1) takes the share from 0.0166 to 0.0035 (a fifth), so the half holds."""
    from igm_amd import mstep
    from igm_amd.synthetic import DEMO_PROTOCOL
    pop, _ = F.load()
    sids = [0, 1, 2, 3]
    body = [1, 2, 1, 2]
    atoms = M.Atoms(pop['radii'], envelope_members=[np.arange(NBEAD), np.arange(NBEAD)])
    poly = M.polymer_bonds(pop['chrom'], pop['copy'], pop['radii'], 2.0, 1.0)
    x = F.struct_major(pop, sids, atoms.n)
    p = json.loads(json.dumps(DEMO_PROTOCOL))
    p['custom_annealing_protocol']['mdsteps'] = [200, 200, 200, 200]
    p['custom_annealing_protocol']['relax']['mdsteps'] = 50
    prm = M.params_from_cfg({'optimization': {'optimizer_options': p}}, [('volume', 1.0), ('volume', 1.0)])
    seeds = M.lammps_seeds(6535, sids, 11)
    V.stage(ctx, maps, struct_map=[0, 0, 0, 0])
    V.set_envelope_maps(ctx, 1, body)
    xo, info = mstep.run(prm, x, atoms.radii, atoms.flags, poly, None, None, seeds, ctx=ctx)
    xr, info_r = mstep.run(prm, x, atoms.radii, atoms.flags, poly, None, None, seeds, ctx=ctx)
    assert np.all(np.isfinite(xo)) and xo.tobytes() == xr.tobytes() and info.tobytes() == info_r.tobytes()
    assert inside_body(x, maps, body) > 0.01 and inside_body(xo, maps, body) <= 0.5 * inside_body(x, maps, body)


def inside_body(xx, maps, body):
    """share of the beads whose voxel is inside their structure's nucleolus body"""
    n = 0
    for s, m in enumerate(body):
        vol = maps[m]
        ix = np.rint((xx[s, :NBEAD] - vol['origin']) / vol['grid']).astype(int)
        ok = np.all((ix >= 0) & (ix < vol['nvoxel']), axis=1)
        ix = np.clip(ix, 0, vol['nvoxel'] - 1)
        n += np.count_nonzero(ok & (vol['matrice'][ix[:, 0], ix[:, 1], ix[:, 2], 3] != 0))
    return n / (len(body) * NBEAD)


# ---------------------------------------------------------------- 7. one igm-run iteration
def test_igm_run_iteration_with_hip_kernels(tmp_path):
    """exp_map + Hi-C + DamID + nucleolus + nuclDamID through the Step classes igm-run
    instantiates, optimization/kernel = 'hip', protocol x0.002"""
    import test_steps_de as TD
    from igm_amd import steps as ST
    tmp = str(tmp_path)
    cfg, _ = NB.bodies_config(tmp, S=3)
    cfg['optimization']['kernel'] = 'hip'
    store = ST.PopulationStore(cfg['optimization']['structure_output'])
    x0 = np.array(store.coordinates())
    try:
        ran = TD._iteration(cfg)
    finally:
        V.stage(_lib.context(0), [])
    assert [type(s).__name__ for s in ran] == ['NuclDamidActivationDistanceStep', 'ActivationDistanceStep',
                                               'DamidActivationDistanceStep', 'ModelingStep']
    db = ST.StepDB(cfg['parameters']['step_db'])
    assert all([r['status'] for r in db.get_history(s.uid)][-1] == 'completed' for s in ran)
    x1 = np.array(store.coordinates())
    assert np.all(np.isfinite(x1)) and not np.array_equal(x0, x1)
    summ = json.loads(store.read_summary())
    j = lambda f: tmp + '/' + f
    for key in ('ExpEnvelope[shape=exp_map,map=%s,k=1.0]' % j('nuc_0.bin'),
                'ExpEnvelope[shape=exp_map,map=%s,k=1.0]' % j('body_0.bin'),
                'ExpEnvelope[shape=exp_map,map=%s,k=1.0]' % j('body_1.bin'),
                'LaminaDamID[shape=exp_map,map=%s,k=-1.0, cr=0.95]' % j('body_0.bin'),
                'LaminaDamID[shape=exp_map,map=%s,k=-1.0, cr=0.95]' % j('body_1.bin'),
                'LaminaDamID[shape=exp_map,map=%s,k=-1.0, cr=0.95]' % j('nuc_0.bin'), 'interHiC', 'Polymer'):
        assert key in summ['byrestraint'], (key, sorted(summ['byrestraint']))
    for sec in ('DamID', 'nuclDamID'):
        assert len(ST.read_damid_rows(cfg['runtime'][sec]['damid_actdist_file'])) > 0
