"""The chromatin tracing A-step on the CPU: the trace file's validation, the greedy assignment,
the Kabsch targets, the assignment file's round trip into the M-step's reader, the resolution of
the assignment file, the step's place in an iteration, and the Step layer from RandomInit to
'completed' on the CPU kernels (the fp64 oracle of tests/tracing_assign.py as 'tracing_assign'),
restart included.  The GPU's side is tests/test_tracing_assign_gpu.py."""
import copy
import json
import os

import numpy as np
import pytest

import tracing_assign as TA
from igm_amd import h5
from igm_amd import igm_run as RUN
from igm_amd import steps as ST
from igm_amd import tracing as T
from igm_amd import workloads as W


# ------------------------------------------------------------------ read_traces
def _file(tmp_path, **over):
    ix, xyz = TA.model(2)
    rng = np.random.default_rng(0)
    tr = TA.traces_of([([0, 3, 4, 7], rng.normal(0, 100, (4, 3))), ([12, 13, 20], rng.normal(0, 100, (3, 3))),
                       ([21, 22, 30, 34], rng.normal(0, 100, (4, 3)))])
    tr.update(over)
    path = os.path.join(str(tmp_path), 'traces.h5')
    h5.write(path, {'trace_ptr': np.asarray(tr['trace_ptr'], np.int64), 'locus': np.asarray(tr['locus'], np.int32),
                    'position': np.asarray(tr['position'])})
    return path, ix, tr


def test_read_traces_round_trip(tmp_path):
    path, ix, tr = _file(tmp_path)
    got = T.read_traces(path, ix)
    assert got['trace_ptr'].tolist() == [0, 4, 7, 11] and got['trace_ptr'].dtype == np.int64
    assert np.array_equal(got['locus'], tr['locus']) and got['locus'].dtype == np.int32
    assert np.array_equal(got['position'], tr['position']) and got['position'].dtype == np.float32
    assert got['chrom'].tolist() == [0, 1, 2] and got['ncopy'].tolist() == [2, 2, 1]
    path, ix, tr = _file(tmp_path, position=np.arange(33, dtype=np.float64).reshape(11, 3))  # float64 on file
    assert np.array_equal(T.read_traces(path, ix)['position'], np.arange(33, dtype=np.float32).reshape(11, 3))
    sub = T.slice_traces(got, 1, 3)
    assert sub['trace_ptr'].tolist() == [0, 3, 7] and sub['locus'].tolist() == [12, 13, 20, 21, 22, 30, 34]
    assert sub['ncopy'].tolist() == [2, 1]


@pytest.mark.parametrize('what,over,match', [
    ('ptr', {'trace_ptr': [0, 7, 4, 11]}, 'not monotone at trace 1'),
    ('short', {'trace_ptr': [0, 4, 6, 11]}, 'trace 1 has 2 spots'),
    ('range', {'locus': [0, 3, 4, 7, 12, 13, 20, 21, 22, 30, 35]}, 'trace 2: locus 35 is outside'),
    ('negative', {'locus': [-1, 3, 4, 7, 12, 13, 20, 21, 22, 30, 34]}, 'trace 0: locus -1 is outside'),
    ('order', {'locus': [0, 3, 3, 7, 12, 13, 20, 21, 22, 30, 34]}, 'trace 0: loci are not strictly increasing'),
    ('chrom', {'locus': [0, 3, 4, 7, 11, 13, 20, 21, 22, 30, 34]}, 'trace 1 has loci of more than one chromosome'),
])
def test_read_traces_rejects(tmp_path, what, over, match):
    path, ix, _ = _file(tmp_path, **{k: np.asarray(v) for k, v in over.items()})
    with pytest.raises(ValueError, match=match):
        T.read_traces(path, ix)


@pytest.mark.parametrize('bad', [np.nan, np.inf])
def test_read_traces_rejects_a_non_finite_position(tmp_path, bad):
    pos = np.random.default_rng(1).normal(0, 100, (11, 3))
    pos[8, 1] = bad
    path, ix, _ = _file(tmp_path, position=pos)
    with pytest.raises(ValueError, match='trace 2 has a non-finite position'):
        T.read_traces(path, ix)


# ------------------------------------------------------------------ greedy_assignment
def test_greedy_three_traces_two_slots():
    """traces 0 and 2 want slot 7 first; trace 2 is cheaper and takes it, trace 0 falls back to
    slot 3, which leaves trace 1 (slots 3, 7) with nothing"""
    cand = np.array([[7, 3], [3, 7], [7, 3]])
    rmsd = np.array([[2.0, 5.0], [4.0, 6.0], [1.0, 9.0]], np.float32)
    pick = T.greedy_assignment(cand, rmsd, np.zeros(3, int))
    assert pick.tolist() == [1, -1, 0]
    assert np.array_equal(pick, T.greedy_assignment(cand, rmsd, np.zeros(3, int)))  # a rerun
    # the same candidates on different chromosomes are different slots
    assert T.greedy_assignment(cand, rmsd, np.array([0, 1, 2])).tolist() == [0, 0, 0]


def test_greedy_ties_go_to_the_lower_trace_and_a_slot_is_taken_once():
    cand = np.array([[4, 5, 6], [4, 5, 6], [4, 5, 6], [4, 5, 6]])
    rmsd = np.array([[1.0, 2.0, 3.0]] * 4, np.float32)
    pick = T.greedy_assignment(cand, rmsd, np.array([9, 9, 9, 9]))
    assert pick.tolist() == [0, 1, 2, -1]
    took = cand[np.arange(4), np.maximum(pick, 0)][pick >= 0]
    assert len(set(took.tolist())) == len(took)
    # order by the best cost, not by the trace id
    rmsd[3, 0] = 0.5
    assert T.greedy_assignment(cand, rmsd, np.array([9, 9, 9, 9])).tolist() == [1, 2, -1, 0]
    assert T.greedy_assignment(np.zeros((0, 3), int), np.zeros((0, 3), np.float32), np.zeros(0, int)).tolist() == []


# ------------------------------------------------------------------ aligned_targets, write_assignment
def _exact_and_mirror():
    ix, xyz = TA.model(3, seed=5)
    loci = np.arange(12, 21)  # chromosome B, 9 loci
    x = xyz[TA.beads_of(ix, loci, 1), 2].astype(np.float64)
    p = x @ TA.PERM.T + np.array([1024.0, -512.0, 256.0])
    mirror = p * np.array([-1.0, 1.0, 1.0])
    other = xyz[TA.beads_of(ix, [21, 25, 26], 0), 0].astype(np.float64) + 5.0
    tr = TA.traces_of([(loci, p), (loci, mirror), ([21, 25, 26], other)])
    assert np.array_equal(tr['position'][:9].astype(np.float64), p)  # exact in float32
    return ix, xyz, T.check_traces(tr, ix.copy_ptr, ix.hap_chrom), x


def test_aligned_targets_exact_and_mirrored():
    ix, xyz, tr, x = _exact_and_mirror()
    target, rmsd, rot = T.aligned_targets(xyz, ix.copy_ptr, ix.copy_idx, tr, [2, 2, -1], [1, 1, -1])
    assert np.abs(target[:9] - x).max() <= 1e-6 and rmsd[0] <= 1e-6
    assert np.allclose(np.linalg.det(rot[:2]), 1.0, rtol=0, atol=1e-12)  # on the mirrored trace too
    assert np.allclose(rot[0], TA.PERM.T, rtol=0, atol=1e-9)
    assert rmsd[1] > 10.0  # a reflection is not a rigid motion
    assert np.isclose(rmsd[1], np.sqrt(np.mean(np.sum((target[9:18] - x) ** 2, axis=1))), rtol=1e-12)
    ref, _ = TA.oracle_rmsd(xyz, ix, tr)
    assert abs(rmsd[1] - ref[1, 2, 1]) <= 1e-9 * ref[1, 2, 1]
    assert np.all(np.isnan(target[18:])) and np.isnan(rmsd[2]) and np.all(np.isnan(rot[2]))


def test_write_assignment_round_trips_into_the_m_step_reader(tmp_path):
    ix, xyz, tr, x = _exact_and_mirror()
    structure, cp = np.array([2, -1, 0]), np.array([1, -1, 0])
    target, rmsd, _ = T.aligned_targets(xyz, ix.copy_ptr, ix.copy_idx, tr, structure, cp)
    path = os.path.join(str(tmp_path), 'a.h5')
    T.write_assignment(path, tr, ix.copy_ptr, ix.copy_idx, structure, cp, target, rmsd)
    d = T.read_assignment(path, nbead=ix.nbead)
    assert d['locus'].tolist() == TA.beads_of(ix, np.arange(12, 21), 1).tolist() + TA.beads_of(ix, [21, 25, 26], 0).tolist()
    assert d['assignment'].tolist() == [2] * 9 + [0] * 3 and d['target'].dtype == np.float64
    assert np.array_equal(d['target'], np.concatenate([target[:9], target[18:]]))
    with h5.File(path) as f:
        assert sorted(f.keys()) == sorted(['locus', 'target', 'assignment', 'trace', 'trace_structure', 'trace_copy',
                                           'trace_rmsd'])
        assert np.asarray(f.read('trace')).tolist() == [0] * 9 + [2] * 3
        assert np.asarray(f.read('trace_structure')).tolist() == [2, -1, 0]
        assert np.asarray(f.read('trace_copy')).tolist() == [1, -1, 0]
        r = np.asarray(f.read('trace_rmsd'))
        assert np.isnan(r[1]) and r[0] == rmsd[0] and r[2] == rmsd[2]
    ptr, a = T.anchors_for(d, [0, 1, 2], 75.0, 1.0, nbead=ix.nbead)
    assert ptr.tolist() == [0, 3, 3, 12]
    assert np.array_equal(a['atom'][3:], TA.beads_of(ix, np.arange(12, 21), 1))
    assert np.array_equal(a['x'][3:], target[:9, 0].astype(np.float32))


# ------------------------------------------------------------------ resolution and the step list
def test_assignment_file_resolution_order():
    cfg = {'restraints': {'tracing': {'assignment_file': 'given.h5', 'input_file': 'traces.h5'}},
           'runtime': {'tracing': {'assignment_file': 'made.h5'}}}
    assert ST.tracing_assignment_file(cfg) == 'made.h5' and ST.tracing_assigned(cfg)
    cfg['runtime'] = {}
    assert ST.tracing_assignment_file(cfg) == 'given.h5' and ST.tracing_assigned(cfg)
    del cfg['restraints']['tracing']['assignment_file']
    assert not ST.tracing_assigned(cfg)
    with pytest.raises(RuntimeError, match='has not been assigned yet'):
        ST.tracing_assignment_file(cfg)
    with pytest.raises(NotImplementedError, match='no assignment step'):  # the text of the parent commit
        ST.tracing_assignment_file({'restraints': {'tracing': {'kspring': 1.0}}})
    assert not ST.tracing_assigned({'restraints': {}})


def test_iteration_steps_adds_the_step_for_input_file_alone():
    R = {'polymer': {}, 'nuclDamID': {}, 'Hi-C': {}, 'FISH': {}, 'sprite': {}, 'DamID': {},
         'tracing': {'input_file': 'traces.h5', 'tol_list': [1]}}
    names = [s.__name__ for s in RUN.iteration_steps({'restraints': R})]
    assert names == ['PolymerAssignmentStep', 'NuclDamidActivationDistanceStep', 'TracingAssignmentStep',
                     'ActivationDistanceStep', 'FishAssignmentStep', 'SpriteAssignmentStep',
                     'DamidActivationDistanceStep', 'ModelingStep']
    plain = [n for n in names if n != 'TracingAssignmentStep']
    R['tracing'] = {'assignment_file': 'given.h5', 'tol_list': [1]}
    assert [s.__name__ for s in RUN.iteration_steps({'restraints': R})] == plain
    R['tracing'] = {'assignment_file': 'given.h5', 'input_file': 'traces.h5', 'tol_list': [1]}
    assert [s.__name__ for s in RUN.iteration_steps({'restraints': R})] == plain  # the given file is used
    del R['tracing']
    assert [s.__name__ for s in RUN.iteration_steps({'restraints': R})] == plain
    assert 'tracing_assign' in ST.KERNELS['hip']


# ------------------------------------------------------------------ the Step layer
def _config(tmp, S=4, ntrace=6, nspots=5):
    """the sphere config of tests/test_tracing.py with imaged traces instead of an assignment"""
    import test_steps_de as TD
    cfg, pop = TD._base(tmp, {'nucleus_shape': 'sphere', 'nucleus_radius': 5500.0, 'nucleus_kspring': 1.0}, S=S)
    store = ST.PopulationStore(cfg['optimization']['structure_output'])
    tr, s, k = W.synthetic_traces(store, np.asarray(store.coordinates()), ntrace, nspots, 1.0, 3)
    path = os.path.join(tmp, 'traces.h5')
    h5.write(path, {'trace_ptr': tr['trace_ptr'], 'locus': tr['locus'], 'position': tr['position']})
    cfg['restraints']['tracing'] = {'input_file': path, 'kspring': 1.0, 'tol_list': [200, 100]}
    cfg['restraints']['Hi-C']['intra_sigma_list'] = [1.0]
    cfg['restraints']['Hi-C']['inter_sigma_list'] = [1.0]
    cfg['optimization'].update({'max_violations': 1.0, 'min_iterations': 1, 'max_iterations': 3,
                                'violation_tolerance': 0.05})
    return cfg, pop, tr, s, k


def test_modeling_spec_and_steps_with_assignment_file_are_the_parent_commits(tmp_path):
    """with assignment_file nothing changes: the step list has no tracing step and the spec's
    tracing entry is the file's content, tol and k, as before"""
    import test_tracing as TT
    cfg, pop, d = TT._tracing_config(str(tmp_path))
    cfg['runtime'] = {'tracing': {'tol': 200}}
    assert [s.__name__ for s in RUN.iteration_steps(cfg)] == ['ActivationDistanceStep', 'ModelingStep']
    spec = ST.modeling_spec(cfg, np.arange(4))
    assert sorted(spec) == ['envelope', 'evfactor', 'hic', 'polymer', 'protocol', 'tracing']
    assert spec['tracing']['tol'] == 200.0 and spec['tracing']['k'] == 1.0
    assert all(np.array_equal(spec['tracing']['data'][k], d[k]) for k in d)
    assert 'assignment_file' not in cfg['runtime']['tracing']


def test_random_init_with_input_file_alone_is_the_run_without_tracing(tmp_path):
    out = []
    for sub, keep in (('a', True), ('b', False)):
        d = tmp_path / sub
        d.mkdir()
        cfg, _, _, _, _ = _config(str(d))
        if not keep:
            del cfg['restraints']['tracing']
        cfg['model']['init_noise'] = 30.0
        ST.RandomInit(cfg).run()
        out.append(np.array(ST.PopulationStore(cfg['optimization']['structure_output']).coordinates()))
    assert out[0].tobytes() == out[1].tobytes()


def test_run_pipeline_on_input_file_alone_completes_and_restarts(tmp_path):
    tmp = str(tmp_path)
    cfg, pop, tr, planted_s, planted_k = _config(tmp)
    TA.register_cpu_kernels()
    cfg['optimization']['kernel'] = 'tracing_assign_test'
    cfg['model']['starting_coordinates'] = ''
    fresh = copy.deepcopy(cfg)
    seen = []

    def on_iteration(c, it, steps):
        f = c['runtime']['tracing']['assignment_file']
        d = T.read_assignment(f, nbead=len(pop['radii']))
        with h5.File(f) as g:
            ts = np.asarray(g.read('trace_structure'))
        seen.append((it, [s.__name__ for s in steps], c['runtime']['tracing']['tol'], len(d['locus']), ts.tolist(),
                     sorted(os.listdir(os.path.dirname(f)))))
        summ = json.loads(ST.PopulationStore(c['optimization']['structure_output']).read_summary())
        assert summ['byrestraint']['Tracing']['n_imposed'] == len(d['locus'])
    del TA.CALLS[:]
    assert RUN.run_pipeline(cfg, on_iteration=on_iteration) == 'completed'
    names = ['TracingAssignmentStep', 'ActivationDistanceStep', 'ModelingStep']
    assert [s[:3] for s in seen] == [(0, names, 200), (0, names, 100)]
    T_ = len(tr['trace_ptr']) - 1
    assert TA.CALLS == [T_, T_]
    for s in seen:  # 6 traces on 4 x 6 slots: every trace placed, one slot each
        assert s[3] == len(tr['locus']) and min(s[4]) >= 0
    assert seen[0][5] == ['tracing_assignment.h5']
    assert seen[1][5] == ['tracing_assignment.h5', 'tracing_assignment.h5.tol_100.0000.iter_0']  # the earlier one rotated
    path = cfg['runtime']['tracing']['assignment_file']
    assert path == os.path.join(tmp, 'tmp', 'tracing', 'tracing_assignment.h5')
    assert cfg['runtime']['tracing']['n_unassigned'] == 0
    assert cfg['restraints']['tracing']['tol_list'] == [200, 100]
    # a restart on the same StepDB: every step is skipped, the file is found again
    del TA.CALLS[:]
    before = os.path.getmtime(path)
    assert RUN.run_pipeline(fresh) == 'completed'
    assert TA.CALLS == [] and os.path.getmtime(path) == before
    assert fresh['runtime']['tracing']['assignment_file'] == path and os.path.isfile(path)
    assert len(T.read_assignment(ST.tracing_assignment_file(fresh))['locus']) == len(tr['locus'])


def test_planted_traces_are_recovered_by_the_oracle():
    """the inputs of the GPU recovery test: the fp64 oracle alone recovers every planted slot"""
    ix, xyz = TA.model(8, seed=11)
    tr, s, k = W.synthetic_traces(ix, xyz, 40, 8, 1.0, 7)
    tr = T.check_traces(tr, ix.copy_ptr, ix.hap_chrom)
    assert len(set(zip(s.tolist(), tr['chrom'].tolist(), k.tolist()))) == 40  # one trace on every slot
    full, _ = TA.oracle_rmsd(xyz, ix, tr)
    cand, val = TA.select(full.astype(np.float32), 8)
    pick = T.greedy_assignment(cand, val, tr['chrom'])
    took = cand[np.arange(40), pick]
    assert np.all(pick >= 0) and np.array_equal(took // 2, s) and np.array_equal(took % 2, k)
