"""Chromatin tracing on the CPU: the tests' own reference (the fp64 oracle on the reference's
dummy-atom formulation against the numpy anchor term), the f32 headroom of every GPU force
input, igm_amd.tracing (anchors_for, initial_coordinates, read_assignment), the assembly with
and without a tracing spec, and the Step layer: a config with a complete restraints/tracing
section through igm_run.run_pipeline from RandomInit to 'completed'."""
import copy
import json
import os

import numpy as np
import pytest

import oracle
import small_models as sm
import tracing as TR
from igm_amd import assemble as A
from igm_amd import h5
from igm_amd import igm_run as RUN
from igm_amd import steps as ST
from igm_amd import tracing as T
from igm_amd._lib import IGM_ATOM_FIXED, anchor_dtype

FORCE_CASES = [(n, 'random') for n in (3, 64, 65, 1025, 3072, 3073)] + [(257, g) for g in sm.GEOMETRIES]


def _case(natom, geometry, envelopes=None):
    model = sm.case(natom, geometry, envelopes)
    aptr, anch = TR.anchor_sets(model[5], natom, 1000 + natom)
    return model, aptr, anch


def test_anchor_sets_are_the_stated_ones():
    (atoms, poly, prm, ptr, sb, x), aptr, anch = _case(65, 'random')
    a0 = anch[aptr[0]:aptr[1]]
    assert aptr[1] == aptr[2] and aptr[3] - aptr[2] == 65  # structure 1: none; structure 2: every atom
    assert a0['atom'][0] == 0 and a0['atom'][1] == 63 and np.count_nonzero(a0['atom'] == 0) >= 2
    r = np.linalg.norm(TR.targets_of(a0).astype(np.float64) - x[0, a0['atom'].astype(int)], axis=1)
    assert r[-2] == 0.0 and abs(r[-1] - 10.0) < 1e-3
    assert np.all(anch['r0'] == 50.0) and np.all(anch['k'] == 1.0)
    assert atoms.flags[2, 64] & IGM_ATOM_FIXED and anch[aptr[2]:]['atom'][-1] == 64


@pytest.mark.parametrize('natom,geometry', [(3, 'random'), (65, 'random'), (257, 'random'), (257, 'coincident'),
                                            (257, 'origin'), (1025, 'random')])
def test_oracle_on_the_dummy_atom_form_equals_the_numpy_term(natom, geometry):
    """The reference of the GPU tests checked against itself: fp64 both sides, summation order
    only (bounds of test_small_models.py)."""
    (atoms, poly, prm, ptr, sb, x), aptr, anch = _case(natom, geometry)
    r2, f2, p2, ptr2, sb2, x2 = TR.dummy_form(atoms.radii, atoms.flags, poly, ptr, sb, x, aptr, anch)
    fo, eo = oracle.mstep_forces(prm, x2, r2, f2, p2, ptr2, sb2, sm.EVF, sm.ENVF)
    fb, eb, parts = TR.brute_batch(atoms, poly, ptr, sb, x, sm.ENV_TWO, sm.EVF, sm.ENVF, aptr, anch, parts=True)
    assert np.all(np.isfinite(fo)) and np.all(np.isfinite(fb))
    assert np.all(fo[:, natom - 1:] == 0.0)  # the dummy and the appended centroids are fixed
    assert np.abs(fo[:, :natom] - fb).max() <= 1e-12 * np.abs(fb).max()
    assert np.allclose(eo[:, 1:5], eb, rtol=1e-12, atol=0.0)
    assert np.all(fb[:, natom - 1] == 0.0) and eb[2, 1] > eb[1, 1]
    # the anchor on the atom itself: no force, no NaN; the one 10 nm away: inside the tolerance
    a0 = anch[aptr[0]:aptr[1]]
    fa, ea, _ = TR.anchor_forces(x[0], sm.struct_flags(atoms, 0), a0[-2:])
    assert np.all(fa == 0.0) and ea == 0.0


@pytest.mark.parametrize('natom,geometry', FORCE_CASES)
def test_f32_bound_has_headroom_with_anchors(natom, geometry):
    """As tests/test_small_models.py: every input of the GPU force tests leaves an honest
    float32 evaluation >= 10x under the 1e-5 bound (per atom for coincident / one_cell)."""
    env = sm.f32_envelopes(geometry)
    (atoms, poly, prm, ptr, sb, x), aptr, anch = _case(natom, geometry, env)
    f64, _, parts = TR.brute_batch(atoms, poly, ptr, sb, x, env, sm.EVF, sm.ENVF, aptr, anch, parts=True)
    f32, _ = TR.brute_batch(atoms, poly, ptr, sb, x, env, sm.EVF, sm.ENVF, aptr, anch, np.float32)
    nb = natom - 1
    err = np.linalg.norm(f32 - f64, axis=2)[:, :nb]
    ref = np.linalg.norm(f64, axis=2)[:, :nb]
    if geometry not in ('coincident', 'one_cell'):
        h = 1e-5 * np.linalg.norm(ref) / np.linalg.norm(err)
        print('natom %d %s: f32 headroom with anchors %.0f' % (natom, geometry, h))
        assert h >= 10
    else:
        bound = 1e-5 * sm.term_magnitudes(parts, geometry)[:, :nb]
        assert np.all(err[bound == 0] == 0)
        h = (bound[bound > 0] / np.maximum(err[bound > 0], 1e-300)).min()
        print('natom %d %s: f32 per-atom headroom with anchors %.0f' % (natom, geometry, h))
        assert h >= 10


# ------------------------------------------------------------------ igm_amd.tracing
def _data():
    return {'locus': np.array([5, 2, 9, 5, 7, 3]), 'assignment': np.array([1, 0, 1, 1, 3, 0]),
            'target': np.arange(18, dtype=np.float64).reshape(6, 3) + 0.1}


def test_anchors_for_order_and_empty_structures():
    ptr, a = T.anchors_for(_data(), [0, 1, 2, 3, 1], 75.0, 2.0, nbead=10)
    assert a.dtype == anchor_dtype and ptr.dtype == np.int64
    assert ptr.tolist() == [0, 2, 5, 5, 6, 9]  # structure 2: none
    assert a['atom'].tolist() == [2, 3, 5, 9, 5, 7, 5, 9, 5]  # file order; locus 5 twice in structure 1
    assert np.array_equal(a['x'][2:5], np.float32([0.1, 6.1, 9.1]))
    assert np.all(a['r0'] == 75.0) and np.all(a['k'] == 2.0)
    ptr, a = T.anchors_for(_data(), [2], 75.0, 2.0)
    assert ptr.tolist() == [0, 0] and len(a) == 0


def test_assignment_errors(tmp_path):
    d = _data()
    with pytest.raises(ValueError, match='outside'):
        T.anchors_for(d, [0], 50.0, 1.0, nbead=9)
    bad = dict(d, locus=np.array([5, 2, -1, 5, 7, 3]))
    with pytest.raises(ValueError, match='outside'):
        T.check_assignment(bad, 10)
    bad = dict(d, target=np.where(np.arange(18).reshape(6, 3) == 7, np.nan, d['target']))
    with pytest.raises(ValueError, match='non-finite'):
        T.check_assignment(bad)
    with pytest.raises(ValueError, match='do not match'):
        T.check_assignment(dict(d, assignment=d['assignment'][:5]))
    path = os.path.join(str(tmp_path), 'tracing.h5')
    h5.write(path, {'locus': d['locus'].astype(np.int32), 'target': d['target'], 'assignment': d['assignment']})
    back = T.read_assignment(path, nbead=10)
    assert all(np.array_equal(back[k], d[k]) for k in d)
    with pytest.raises(ValueError, match='outside'):
        T.read_assignment(path, nbead=9)


def test_initial_coordinates():
    rng = np.random.default_rng(4)
    crd = rng.normal(0, 1000.0, (12, 3))
    d = {'locus': np.array([2, 6, 7, 10, 4]), 'assignment': np.array([0, 0, 0, 1, 2]),
         'target': rng.normal(0, 500.0, (5, 3))}
    out = T.initial_coordinates(crd, d, 0)
    assert np.array_equal(out[[2, 6, 7]], d['target'][:3])  # targets hit exactly
    for m, q in enumerate((3, 4, 5)):  # interior loci on the segment 2 -> 6
        assert np.allclose(out[q], d['target'][0] + (m + 1) * (d['target'][1] - d['target'][0]) / 4, rtol=0, atol=1e-9)
    rest = [0, 1, 8, 9, 10, 11]
    assert np.array_equal(out[rest], crd[rest])  # adjacent loci 6, 7: nothing in between
    one = T.initial_coordinates(crd, d, 1)  # one traced locus: nothing to interpolate
    assert np.array_equal(one[10], d['target'][3]) and np.array_equal(np.delete(one, 10, 0), np.delete(crd, 10, 0))
    assert np.array_equal(T.initial_coordinates(crd, d, 5), crd)  # a structure without traced loci
    # noise: every bead, from the structure's own generator, reproducible
    n1 = T.initial_coordinates(crd, d, 0, np.random.RandomState(7), 25.0)
    n2 = T.initial_coordinates(crd, d, 0, np.random.RandomState(7), 25.0)
    assert np.array_equal(n1, n2)
    assert np.array_equal(n1 - out, (out + 25.0 * np.random.RandomState(7).randn(12, 3)) - out)
    assert np.all(n1 != out)
    # a descending pair of entries is not interpolated (pin_2 - pin_1 <= 1), as the reference
    dd = {'locus': np.array([8, 3]), 'assignment': np.array([0, 0]), 'target': d['target'][:2]}
    o = T.initial_coordinates(crd, dd, 0)
    assert np.array_equal(o[[4, 5, 6, 7]], crd[[4, 5, 6, 7]])


# ------------------------------------------------------------------ assembly and the Step layer
def _tracing_config(tmp, S=4):
    import test_steps_de as TD
    cfg, pop = TD._base(tmp, {'nucleus_shape': 'sphere', 'nucleus_radius': 5500.0, 'nucleus_kspring': 1.0}, S=S)
    nbead = len(pop['radii'])
    rng = np.random.default_rng(12)
    locus = np.concatenate([np.sort(rng.choice(nbead, 6, replace=False)) for _ in range(S - 1)])
    assignment = np.repeat(np.arange(S - 1), 6)  # the last structure has no traced locus
    target = rng.normal(0.0, 1500.0, (len(locus), 3))
    path = os.path.join(tmp, 'tracing_assignment.h5')
    h5.write(path, {'locus': locus.astype(np.int64), 'target': target, 'assignment': assignment.astype(np.int64)})
    cfg['restraints']['tracing'] = {'assignment_file': path, 'kspring': 1.0, 'tol_list': [200, 100]}
    return cfg, pop, {'locus': locus, 'target': target, 'assignment': assignment}


def test_batch_without_tracing_is_unchanged_and_with_it_gains_one_class(tmp_path):
    import cpu_kernels as CK
    cfg, pop, d = _tracing_config(str(tmp_path))
    cfg['runtime'] = {'tracing': {'tol': 200}}
    store = ST.PopulationStore(cfg['optimization']['structure_output'])
    sids = np.arange(4)
    spec = ST.modeling_spec(cfg, sids)
    assert spec['tracing']['tol'] == 200.0 and spec['tracing']['k'] == 1.0
    plain = copy.deepcopy(cfg)
    del plain['restraints']['tracing']
    b0 = A.build(ST.batch_coordinates(store, sids), sids, store, ST.modeling_spec(plain, sids), None,
                 select=CK.OracleSelect())
    b1 = A.build(ST.batch_coordinates(store, sids), sids, store, spec, None, select=CK.OracleSelect())
    assert b0.anchors is None and b0.anchor_ptr is None and 'Tracing' not in b0.names
    assert b1.names == b0.names + ['Tracing'] and len(b0.names) == A.NCLASS + 1
    assert np.array_equal(b0.class_cr, b1.class_cr) and bytes(b0.prm) == bytes(b1.prm)
    assert b1.natom == b0.natom and np.array_equal(b0.x, b1.x) and np.array_equal(b0.flags, b1.flags)
    assert b1.anchor_ptr.tolist() == [0, 6, 12, 18, 18]
    assert np.array_equal(b1.anchors['atom'], d['locus']) and np.all(b1.anchors['r0'] == 200.0)
    assert np.array_equal(TR.targets_of(b1.anchors), d['target'].astype(np.float32))


def test_tracing_section_without_assignment_file_still_raises(tmp_path):
    with pytest.raises(NotImplementedError, match='no assignment step'):
        RUN.iteration_steps({'restraints': {'tracing': {'kspring': 1.0, 'tol_list': [1]}}})
    with pytest.raises(NotImplementedError, match='no assignment step'):
        ST.modeling_spec({'restraints': {'tracing': {}}}, [0])  # before any other key is read


def test_run_pipeline_with_tracing_completes(tmp_path):
    """RandomInit (traced loci at their targets) + RelaxInit (tolerance 50) + two A/M
    iterations through tol_list [200, 100]; the summary carries 'Tracing'."""
    tmp = str(tmp_path)
    cfg, pop, d = _tracing_config(tmp)
    TR.register_cpu_kernels()
    del TR.SEEN[:]
    cfg['optimization']['kernel'] = 'tracing_test'
    cfg['model']['starting_coordinates'] = ''
    cfg['restraints']['Hi-C']['intra_sigma_list'] = [1.0]
    cfg['restraints']['Hi-C']['inter_sigma_list'] = [1.0]
    cfg['optimization'].update({'max_violations': 1.0, 'min_iterations': 1, 'max_iterations': 3,
                                'violation_tolerance': 0.05})
    seen = []

    def on_iteration(c, it, steps):
        seen.append((it, [s.__name__ for s in steps], c['runtime']['tracing']['tol'],
                     list(c['runtime']['tracing']['tol_list'])))
    assert RUN.run_pipeline(cfg, on_iteration=on_iteration) == 'completed'
    assert os.path.isfile(os.path.join(tmp, 'completed'))
    names = ['ActivationDistanceStep', 'ModelingStep']  # no step of its own
    assert seen == [(0, names, 200, [100]), (0, names, 100, [])]
    assert [s for s in TR.SEEN if s[0] == 'relax'] == [('relax', 50.0)] * 2  # two batches of RelaxInit
    assert [s[1:] for s in TR.SEEN if s[0] == 'mstep'] == [(200.0, 200.0)] * 2 + [(100.0, 100.0)] * 2
    assert cfg['restraints']['tracing']['tol_list'] == [200, 100]  # the config's list is copied, not consumed
    store = ST.PopulationStore(cfg['optimization']['structure_output'])
    summ = json.loads(store.read_summary())
    assert 'Tracing' in summ['byrestraint'], sorted(summ['byrestraint'])
    assert summ['byrestraint']['Tracing']['n_imposed'] == len(d['locus'])


def test_random_init_puts_traced_loci_at_their_targets(tmp_path):
    """RandomInit.task: territories from the structure's RandomState, then the tracing block
    (targets, interpolation), then init_noise from the same generator."""
    from igm_amd import init
    cfg, pop, d = _tracing_config(str(tmp_path))
    ST.RandomInit(cfg).run()
    x = np.array(ST.PopulationStore(cfg['optimization']['structure_output']).coordinates())
    assert np.array_equal(x[d['locus'], d['assignment']], d['target'].astype(np.float32))
    plain = init.generate_territories(pop['chrom_sizes'], 7000.0, np.random.RandomState(3)).astype(np.float32)
    assert np.array_equal(x[:, 3], plain)  # the structure without traced loci: the territories alone
    want = T.initial_coordinates(init.generate_territories(pop['chrom_sizes'], 7000.0, np.random.RandomState(1)),
                                 d, 1).astype(np.float32)
    assert np.array_equal(x[:, 1], want) and not np.array_equal(x[:, 1], plain)
    cfg['model']['init_noise'] = 30.0
    cfg['parameters']['step_db'] = os.path.join(str(tmp_path), 'stepdb2.sqlite')
    ST.RandomInit(cfg).run()
    xn = np.array(ST.PopulationStore(cfg['optimization']['structure_output']).coordinates())
    rng = np.random.RandomState(1)
    terr = init.generate_territories(pop['chrom_sizes'], 7000.0, rng)
    assert np.array_equal(xn[:, 1], T.initial_coordinates(terr, d, 1, rng, 30.0).astype(np.float32))
    assert 5.0 < np.abs(xn[:, 1] - x[:, 1]).mean() < 60.0
