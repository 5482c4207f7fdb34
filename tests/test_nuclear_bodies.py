"""DamID and nuclear bodies on imaged nuclei (exp_map) in the M-step, CPU side:
the NumPy restatement of tests/nuclear_bodies.py pinned to the reference goldens
(nuclear_bodies_golden.npz: GenDamid membership, the nuclear-body A-step rows), and on
that restatement as the selection backend: assemble.build's four envelopes, the
unchanged output for configurations without the new sections, the igm-run step order,
the nuclDamID threshold list in run_pipeline and the unsupported combinations."""
import copy
import json
import os

import numpy as np
import pytest

import nuclear_bodies as NB
from conftest import GOLDEN, load_golden
from igm_amd import assemble as A
from igm_amd import igm_run as RUN
from igm_amd import model as M
from igm_amd import steps as ST
from igm_amd._lib import IGM_ATOM_BEAD, IGM_ATOM_ENV0, IGM_ATOM_FIXED


@pytest.fixture(scope='module')
def gold():
    return load_golden('nuclear_bodies_golden.npz')


@pytest.fixture(scope='module')
def maps():
    return NB.golden_maps()


_rows = NB.golden_rows


# ---------------------------------------------------------------- the restatement, pinned
@pytest.mark.parametrize('m', [0, 1])
def test_restatement_membership_equals_reference(gold, maps, m):
    sel = NB.volume_select_rows(gold['pos'], _rows(gold), maps, [m] * 4)
    assert np.array_equal(sel, gold['sel_b%d' % m])
    # the golden is not trivial: both outcomes on both branches, for every structure
    for s in range(4):
        _, inside = NB.snormsq_exp(gold['pos'][s, gold['loc']], maps[m])
        for br in (True, False):
            got = sel[s][inside == br]
            assert len(got) >= 20 and 5 <= got.sum() <= len(got) - 5


def test_restatement_alternating_maps(gold, maps):
    sel = NB.volume_select_rows(gold['pos'], _rows(gold), maps, [0, 1, 0, 1])
    want = np.stack([gold['sel_b%d' % (s % 2)][s] for s in range(4)])
    assert np.array_equal(sel, want)


@pytest.mark.parametrize('it_corr', [0, 1])
def test_restatement_nuclear_body_astep_equals_reference(gold, maps, it_corr):
    pop = load_golden('demo_population.npz')
    r = NB.nucl_damid_actdist(pop['coordinates'], pop['copy_ptr'], pop['copy_idx'], gold['a_loci'], gold['a_pexp'],
                              gold['a_plast'], it_corr, 0.95, [maps[1], maps[2]], gold['a_volumes_idx'])
    assert np.array_equal(r['loc'], gold['a%d_loc' % it_corr])
    assert np.array_equal(r['dist'].view(np.uint32), gold['a%d_dist' % it_corr].view(np.uint32))
    assert np.array_equal(r['prob'].view(np.uint32), gold['a%d_prob' % it_corr].view(np.uint32))
    assert len(np.unique(r['dist'])) > 100


# ---------------------------------------------------------------- assemble.build
def test_build_four_envelopes_in_modelingstep_order(gold, maps):
    pop = load_golden('demo_population.npz')
    sel = NB.BodiesSelect()
    b = A.build(gold['pos'], np.arange(4), NB.index_of(pop), NB.four_envelope_spec(gold, maps), None, select=sel)
    nbead = 3008
    prm = b.prm
    assert prm.nenvelopes == 4 and list(prm.env_kind) == [M.IGM_ENV_VOLUME] * 4
    assert list(prm.env_k) == [1.0, 2.0, -0.5, -0.05]  # nucleus, nucleolus, nuclDamID, DamID
    assert np.array_equal(b.env_scale, [0.95, 0.95, 0.9, 0.05])
    # one pool, nucleus maps first; the nucleolus envelopes read pool entry 1, DamID the default table
    assert len(sel.pool) == 2 and sel.pool[0] is maps[0] and sel.pool[1] is maps[1]
    assert sorted(sel.tables) == [1, 2] and all(np.array_equal(t, [1, 1, 1, 1]) for t in sel.tables.values())
    assert np.array_equal(sel.struct_map, [0, 0, 0, 0])
    # names: the reference's repr()s
    want_damid = str(gold['repr_b0'])
    assert want_damid == 'LaminaDamID[shape=exp_map,map=MAPFILE,k=-0.05, cr=0.05]'
    for q in range(4):
        assert b.vstat_names(q)[A.NCLASS:] == [
            'ExpEnvelope[shape=exp_map,map=nuc_0.bin,k=1.0]',
            'ExpEnvelope[shape=exp_map,map=nucleolus_3.bin,k=2.0]',
            'LaminaDamID[shape=exp_map,map=nucleolus_3.bin,k=-0.5, cr=0.9]',
            want_damid.replace('MAPFILE', 'nuc_0.bin')]
    # flags: every bead in the nucleus and the nucleolus envelopes, the golden membership in the other two
    f = b.flags
    assert f.shape == (4, b.natom)
    every = IGM_ATOM_BEAD | IGM_ATOM_ENV0 | (IGM_ATOM_ENV0 << 1)
    assert np.all(f[:, :nbead] & every == every) and np.all(f[:, nbead] == IGM_ATOM_FIXED)
    for e, m in ((2, 1), (3, 0)):
        want = np.zeros((4, nbead), bool)
        for s in range(4):
            want[s, gold['loc'][gold['sel_b%d' % m][s]]] = True
        assert np.array_equal((f[:, :nbead] & (IGM_ATOM_ENV0 << e)) != 0, want), e
        assert 100 < want[0].sum() < 500


def test_build_exp_map_damid_alone_takes_the_second_slot(gold, maps):
    pop = load_golden('demo_population.npz')
    spec = NB.four_envelope_spec(gold, maps)
    del spec['nucleolus'], spec['nucldamid']
    spec['envelope'].update(volumes=[maps[0], maps[1]], files=['nuc_0.bin', 'nuc_1.bin'],
                            struct_map=np.array([0, 1, 0, 1], np.int32))
    sel = NB.BodiesSelect()
    b = A.build(gold['pos'], np.arange(4), NB.index_of(pop), spec, None, select=sel)
    assert b.prm.nenvelopes == 2 and list(b.prm.env_k)[:2] == [1.0, -0.05] and sel.tables == {}
    assert b.vstat_names(1)[A.NCLASS:] == ['ExpEnvelope[shape=exp_map,map=nuc_1.bin,k=1.0]',
                                           'LaminaDamID[shape=exp_map,map=nuc_1.bin,k=-0.05, cr=0.05]']
    for s in range(4):  # the structure's own nucleus map
        want = np.zeros(3008, bool)
        want[gold['loc'][gold['sel_b%d' % (s % 2)][s]]] = True
        assert np.array_equal((b.flags[s, :3008] & (IGM_ATOM_ENV0 << 1)) != 0, want)


@pytest.mark.parametrize('config', ['D', 'E'])
def test_build_without_the_new_sections_equals_the_previous_commit(tmp_path, config):
    """tests/golden/assemble_parent_digests.json: recorded with the commit before this
    feature, by this same function"""
    b, calls = NB.parent_case(str(tmp_path), config)
    with open(os.path.join(GOLDEN, 'assemble_parent_digests.json')) as f:
        want = json.load(f)[config]
    assert NB.batch_digest(b, strip=str(tmp_path)) == want
    assert set(calls) <= {'hic', 'damid', 'volumes'}  # the new backend methods are not touched


def test_build_rejects_what_the_reference_cannot_run(gold, maps):
    pop = load_golden('demo_population.npz')
    spec = NB.four_envelope_spec(gold, maps)
    spec['envelope'] = A.envelope_spec('sphere', radius=5500.0)
    with pytest.raises(NotImplementedError):
        A.build(gold['pos'], np.arange(4), NB.index_of(pop), spec, None, select=NB.BodiesSelect())
    spec = NB.four_envelope_spec(gold, maps)
    del spec['nucleolus']
    with pytest.raises(NotImplementedError):
        A.build(gold['pos'], np.arange(4), NB.index_of(pop), spec, None, select=NB.BodiesSelect())


# ---------------------------------------------------------------- igm-run
def test_iteration_steps_with_nucldamid_follow_igm_run():
    cfg = {'restraints': {'Hi-C': {}, 'FISH': {}, 'sprite': {}, 'DamID': {}, 'polymer': {}, 'nuclDamID': {}}}
    assert [s.__name__ for s in RUN.iteration_steps(cfg)] == [
        'PolymerAssignmentStep', 'NuclDamidActivationDistanceStep', 'ActivationDistanceStep', 'FishAssignmentStep',
        'SpriteAssignmentStep', 'DamidActivationDistanceStep', 'ModelingStep']
    assert issubclass(ST.NuclDamidActivationDistanceStep, ST.Step)
    with pytest.raises(NotImplementedError):
        RUN.iteration_steps({'restraints': {'tracing': {}, 'nuclDamID': {}}})


def test_run_pipeline_consumes_the_nucldamid_sigma_list(tmp_path):
    tmp = str(tmp_path)
    cfg, pop = NB.bodies_config(tmp)
    NB.register_cpu_kernels()
    cfg['optimization']['kernel'] = 'nuclear_bodies_test'
    cfg['restraints']['Hi-C']['intra_sigma_list'] = [1.0]
    cfg['restraints']['Hi-C']['inter_sigma_list'] = [1.0]
    cfg['restraints']['DamID']['sigma_list'] = [0.6]
    cfg['optimization'].update({'max_violations': 1.0, 'min_iterations': 1, 'max_iterations': 3})
    del NB.BUILT[:]
    seen = []

    def on_iteration(c, it, steps):
        seen.append((it, [s.__name__ for s in steps], c['runtime']['nuclDamID']['sigma'],
                     list(c['runtime']['nuclDamID']['sigma_list'])))

    assert RUN.run_pipeline(cfg, on_iteration=on_iteration) == 'completed'
    names = ['NuclDamidActivationDistanceStep', 'ActivationDistanceStep', 'DamidActivationDistanceStep', 'ModelingStep']
    # the nuclDamID list alone keeps the pipeline going for a second iteration
    assert seen == [(0, names, 0.6, [0.45]), (0, names, 0.45, [])]
    act = cfg['runtime']['nuclDamID']['damid_actdist_file']
    assert act == os.path.join(tmp, 'tmp', 'nucldamid_actdist', 'damid_actdist.hdf5')
    assert os.path.isfile(act + '.nuclDamID_0.4500.iter_-1')  # the first sigma's rows, kept as the swap file
    rows = ST.read_damid_rows(act)
    assert len(rows) > 0 and rows['loc'].max() < 3008
    # ModelingStep read both row files and both map sets: four envelopes, their vstat keys in the summary
    b = NB.BUILT[-1]
    assert b.prm.nenvelopes == 4 and [k > 0 for k in list(b.prm.env_k)] == [True, True, False, False]
    summ = json.loads(ST.PopulationStore(cfg['optimization']['structure_output']).read_summary())
    for key in ('ExpEnvelope[shape=exp_map,map=%s,k=1.0]' % os.path.join(tmp, 'nuc_0.bin'),
                'ExpEnvelope[shape=exp_map,map=%s,k=1.0]' % os.path.join(tmp, 'body_1.bin'),
                'LaminaDamID[shape=exp_map,map=%s,k=-1.0, cr=0.95]' % os.path.join(tmp, 'body_0.bin'),
                'LaminaDamID[shape=exp_map,map=%s,k=-1.0, cr=0.95]' % os.path.join(tmp, 'nuc_0.bin')):
        assert key in summ['byrestraint'], (key, sorted(summ['byrestraint']))


def test_modeling_spec_reads_the_new_sections_and_rejects_the_rest(tmp_path):
    tmp = str(tmp_path)
    cfg, _ = NB.bodies_config(tmp)
    for sec in ('DamID', 'nuclDamID'):  # rows as the A-steps would have left them
        path = os.path.join(tmp, sec + '_rows.npz')
        np.savez(path, loc=np.arange(5, dtype=np.int32), dist=np.ones(5, np.float32), prob=np.ones(5, np.float32))
        cfg['runtime'].setdefault(sec, {})['damid_actdist_file'] = path
    spec = ST.modeling_spec(cfg, [0, 1, 2])
    assert spec['nucleolus']['files'] == [os.path.join(tmp, 'body_0.bin'), os.path.join(tmp, 'body_1.bin')]
    assert list(spec['nucleolus']['struct_map']) == [0, 1, 0] and spec['nucleolus']['shape'] == 'exp_map'
    assert len(spec['nucldamid']['rows']) == 5 and spec['nucldamid']['contact_range'] == 0.95
    assert spec['damid']['repr_k'] == 1.0
    # any other nucleus shape: refused before a key of the sections is read (they are empty here)
    for shape in ({'nucleus_shape': 'sphere', 'nucleus_radius': 5500.0, 'nucleus_kspring': 1.0},
                  {'nucleus_shape': 'ellipsoid', 'nucleus_semiaxes': [5600.0, 5500.0, 5400.0], 'nucleus_kspring': 1.0}):
        for where, key in (('restraints', 'nuclDamID'), ('model', 'nucleolus')):
            c = copy.deepcopy(cfg)
            c['model']['restraints']['envelope'] = shape
            del c['model']['restraints']['nucleolus'], c['restraints']['nuclDamID']
            (c['restraints'] if where == 'restraints' else c['model']['restraints'])[key] = {}
            with pytest.raises(NotImplementedError):
                ST.modeling_spec(c, [0])
    c = copy.deepcopy(cfg)  # nuclDamID needs the nucleolus maps
    del c['model']['restraints']['nucleolus']
    with pytest.raises(NotImplementedError):
        ST.modeling_spec(c, [0])
    c = copy.deepcopy(cfg)
    c['restraints']['tracing'] = {}
    with pytest.raises(NotImplementedError):
        ST.modeling_spec(c, [0])
