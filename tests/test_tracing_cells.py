"""The joint placement of the traces of an imaged cell on the CPU: the fp64 oracle of
tests/tracing_cells.py against the brute force over all labellings, the cell_ptr validation, the
one-cell-per-structure greedy, the joint Kabsch targets, the assignment file's round trip, and
TracingAssignmentStep on a cell_ptr file with the oracle as the 'tracing_assign_cells' kernel.
The GPU's side is tests/test_tracing_cells_gpu.py."""
import os

import numpy as np
import pytest

import tracing_assign as TA
import tracing_cells as TC
from igm_amd import h5
from igm_amd import steps as ST
from igm_amd import tracing as T
from igm_amd import workloads as W


# ------------------------------------------------------------------ the oracle itself
@pytest.fixture(scope='module')
def proto():
    """the prototype's inputs: six chromosomes of 8-14 loci (one single-copy, one with a
    homologue not imaged), 24 random-walk structures, 18 planted cells with 0, 30 and 150 nm
    noise; the oracle's search and the brute force on every (cell, structure)"""
    ix, xyz = TC.genome(24, seed=1)
    tr, s, k = TC.planted(ix, xyz)
    sums = [TC.cell_sums(xyz, ix, tr, c) for c in range(18)]
    return {'ix': ix, 'xyz': xyz, 'tr': tr, 's': s, 'k': k, 'oracle': TC.cells_oracle(xyz, ix, tr),
            'brute': np.array([TC.brute(r)[0] for r in sums])}


def test_the_inputs_are_the_prototypes(proto):
    tr, ix = proto['tr'], proto['ix']
    assert len(tr['cell_ptr']) == 19 and np.all(np.diff(tr['cell_ptr']) == 10)  # 5 x 2 + 1 - 1 traces per cell
    assert len(set(proto['s'].tolist())) == 18
    chrom = tr['chrom'][:10].tolist()
    assert sorted(chrom) == [0, 0, 1, 1, 2, 3, 3, 4, 4, 5]
    assert np.all(proto['k'][tr['chrom'] == 5] == 0)


def test_search_is_never_below_the_brute_force(proto):
    o, b = proto['oracle'], proto['brute']
    floor = TA.noise_floor(o['scale'])
    print('search / brute: max %.3f, equal in %.0f %%' % ((o['cost'] / np.maximum(b, floor)).max(),
                                                          100.0 * np.mean(np.abs(o['cost'] - b) <= 1e-9 * b + floor)))
    assert np.all(o['cost'] >= b - floor)


def test_search_recovers_every_planted_cell(proto):
    o, b, tr, s, k = (proto[q] for q in ('oracle', 'brute', 'tr', 's', 'k'))
    c = np.arange(18)
    floor = TA.noise_floor(o['scale'][c, s])
    assert np.all(np.abs(o['cost'][c, s] - b[c, s]) <= 1e-9 * b[c, s] + floor)  # the optimum where it matters
    assert np.array_equal(np.argmin(o['cost'], axis=1), s)
    cell = np.repeat(c, np.diff(tr['cell_ptr']))
    assert np.array_equal(o['label'][np.arange(len(k)), s[cell]], k)
    assert np.all(o['fixed']) and o['rounds'].max() <= 8 and o['rounds'].min() >= 1
    noise = np.resize([0.0, 30.0, 150.0], 18)
    print('planted cost / (noise sqrt 3):', (o['cost'][c, s][noise > 0] / (noise[noise > 0] * np.sqrt(3.0))).round(2))
    assert np.all(o['cost'][c, s] <= 2.0 * noise * np.sqrt(3.0) + floor)
    assert np.sort(o['cost'], axis=1)[:, 1].min() > 1000.0  # the runner-up is another structure altogether


def test_cost_sequence_never_increases(proto):
    o = proto['oracle']
    for (c, s), seq in o['costs'].items():
        assert len(seq) == o['rounds'][c, s]  # one fit per round (the last round moved nothing)
        assert np.all(np.diff(seq) <= TA.noise_floor(o['scale'][c, s])), (c, s, seq)


def test_one_trace_cells_are_the_independent_cost():
    """a cell of one trace: the cell's frame is the trace's, so the cost is min_k of the per-trace
    cost of tests/tracing_assign.py and the label its argmin; on a tie the lower copy"""
    ix, xyz = TC.genome(9, seed=4)
    xyz[ix.copy_idx[ix.copy_ptr[:12] + 1], 5] = xyz[ix.copy_idx[ix.copy_ptr[:12]], 5]  # structure 5: A's copies coincide
    tr, s, k = TC.planted(ix, xyz, ncell=3, seed=8)
    tr = T.check_traces(dict(tr, cell_ptr=np.arange(len(tr['ncopy']) + 1)), ix.copy_ptr, ix.hap_chrom)
    ref, scale = TA.oracle_rmsd(xyz, ix, tr)
    o = TC.cells_oracle(xyz, ix, tr)
    want = ref.min(axis=2)
    assert np.all(np.abs(o['cost'] - want) <= 1e-9 * want + TA.noise_floor(o['scale']))
    clear = np.abs(ref[:, :, 0] - np.where(np.isfinite(ref[:, :, -1]), ref[:, :, -1], np.inf)) > 1e-6
    assert np.array_equal(o['label'][clear], np.argmin(ref, axis=2)[clear]) and clear.mean() > 0.8
    assert np.all(o['label'][tr['chrom'] == 0, 5] == 0)  # the tie
    assert np.all(o['rounds'] == 1) and np.all(o['fixed'])


# ------------------------------------------------------------------ check_traces
def _cells(**over):
    ix, xyz = TC.genome(2)
    rng = np.random.default_rng(0)
    loci = [[0, 3, 4, 7], [1, 2, 5], [12, 13, 20], [21, 22, 30, 34], [0, 1, 2], [21, 25, 26]]
    tr = TA.traces_of([(l, rng.normal(0, 100, (len(l), 3))) for l in loci])
    tr['cell_ptr'] = np.array([0, 4, 6])
    tr.update(over)
    return ix, tr


def test_check_traces_takes_cell_ptr(tmp_path):
    ix, tr = _cells()
    got = T.check_traces(tr, ix.copy_ptr, ix.hap_chrom)
    assert got['cell_ptr'].tolist() == [0, 4, 6] and got['cell_ptr'].dtype == np.int64
    assert T.check_traces({k: v for k, v in tr.items() if k != 'cell_ptr'}, ix.copy_ptr, ix.hap_chrom)['cell_ptr'] is None
    path = os.path.join(str(tmp_path), 'cells.h5')
    h5.write(path, {k: np.asarray(v) for k, v in tr.items()})
    assert T.read_traces(path, ix)['cell_ptr'].tolist() == [0, 4, 6]
    h5.write(path, {k: np.asarray(v) for k, v in tr.items() if k != 'cell_ptr'})
    assert T.read_traces(path, ix)['cell_ptr'] is None
    sub = T.slice_cells(got, 1, 2)
    assert sub['cell_ptr'].tolist() == [0, 2] and sub['trace_ptr'].tolist() == [0, 3, 6]
    assert sub['locus'].tolist() == [0, 1, 2, 21, 25, 26]


@pytest.mark.parametrize('what,cell_ptr,match', [
    ('start', [1, 4, 6], 'cell_ptr must start at 0'),
    ('monotone', [0, 5, 4, 6], 'cell_ptr is not monotone at cell 1'),
    ('empty', [0, 4, 4, 6], 'cell 1 has no trace'),
    ('short', [0, 4, 5], 'cell_ptr ends at 5, the file has 6 traces'),
    ('long', [0, 4, 7], 'cell_ptr ends at 7, the file has 6 traces'),
    ('three of a diploid chromosome', [0, 5, 6], 'cell 0 has 3 traces of chromosome 0, which has 2 copies'),
    ('two of a single-copy chromosome', [0, 3, 6], 'cell 1 has 2 traces of chromosome 2, which has 1 copies'),
])
def test_check_traces_rejects(what, cell_ptr, match):
    ix, tr = _cells(cell_ptr=np.asarray(cell_ptr))
    with pytest.raises(ValueError, match=match):
        T.check_traces(tr, ix.copy_ptr, ix.hap_chrom)


def test_per_trace_rules_still_hold_with_cells():
    ix, tr = _cells(trace_ptr=np.array([0, 4, 7, 10, 14, 16, 20]))
    with pytest.raises(ValueError, match='trace 4 has 2 spots'):
        T.check_traces(tr, ix.copy_ptr, ix.hap_chrom)


# ------------------------------------------------------------------ greedy_cell_assignment
def test_greedy_cells_collisions_exhaustion_and_ties():
    cand = np.array([[7, 3], [3, 7], [7, 3]])
    cost = np.array([[2.0, 5.0], [4.0, 6.0], [1.0, 9.0]], np.float32)
    # cell 2 is cheapest and takes 7, cell 0 falls back to 3, cell 1 (3, 7) is left with nothing
    assert T.greedy_cell_assignment(cand, cost).tolist() == [1, -1, 0]
    same = np.array([[4, 5, 6]] * 4)
    cost = np.array([[1.0, 2.0, 3.0]] * 4, np.float32)
    pick = T.greedy_cell_assignment(same, cost)
    assert pick.tolist() == [0, 1, 2, -1]  # ties go to the lower cell, a structure is taken once
    cost[3, 0] = 0.5
    assert T.greedy_cell_assignment(same, cost).tolist() == [1, 2, -1, 0]  # by the best cost, not by the cell id
    assert T.greedy_cell_assignment(np.zeros((0, 3), int), np.zeros((0, 3), np.float32)).tolist() == []


# ------------------------------------------------------------------ aligned_cell_targets, write_assignment
def _exact_cell_and_mirror():
    """cell 0: every homologue of structure 2 turned by an axis permutation and shifted by whole
    nm (exact in float32); cell 1: its mirror image; cell 2: unassigned"""
    ix, xyz = TC.genome(3, seed=5)
    loci = [np.arange(0, 12), np.arange(0, 12), np.arange(12, 21), np.arange(21, 35)]
    copy = np.array([1, 0, 1, 0])
    x = [xyz[TA.beads_of(ix, l, k), 2].astype(np.float64) for l, k in zip(loci, copy)]
    p = [q @ TA.PERM.T + np.array([1024.0, -512.0, 256.0]) for q in x]
    items = ([(l, q) for l, q in zip(loci, p)] + [(l, q * np.array([-1.0, 1.0, 1.0])) for l, q in zip(loci, p)] +
             [([21, 25, 26], x[3][[0, 4, 5]] + 5.0)])
    tr = TA.traces_of(items)
    tr['cell_ptr'] = np.array([0, 4, 8, 9])
    assert np.array_equal(tr['position'][:12].astype(np.float64), p[0])
    return ix, xyz, T.check_traces(tr, ix.copy_ptr, ix.hap_chrom), np.concatenate(x), copy


def test_aligned_cell_targets_exact_and_mirrored():
    ix, xyz, tr, x, copy = _exact_cell_and_mirror()
    labels = np.concatenate([copy, copy, [0]])
    target, cell_rmsd, trace_rmsd, rot = T.aligned_cell_targets(xyz, ix.copy_ptr, ix.copy_idx, tr, [2, 2, -1], labels)
    n = len(x)
    assert np.abs(target[:n] - x).max() <= 1e-6 and cell_rmsd[0] <= 1e-6 and np.all(trace_rmsd[:4] <= 1e-6)
    assert np.allclose(rot[0], TA.PERM.T, rtol=0, atol=1e-9)
    assert np.allclose(np.linalg.det(rot[:2]), 1.0, rtol=0, atol=1e-12)  # on the mirrored cell too
    assert cell_rmsd[1] > 10.0  # a reflection is not a rigid motion
    # against an SVD on the concatenated points, written out here
    p = tr['position'][n:2 * n].astype(np.float64)
    pc, xc = p - p.mean(axis=0), x - x.mean(axis=0)
    U, sv, Vt = np.linalg.svd(xc.T @ pc)
    d = np.sign(np.linalg.det(U) * np.linalg.det(Vt))
    want = np.sqrt(max(0.0, np.sum(pc * pc) + np.sum(xc * xc) - 2.0 * (sv[0] + sv[1] + d * sv[2])) / n)
    assert abs(cell_rmsd[1] - want) <= 1e-9 * want
    assert np.isclose(cell_rmsd[1], np.sqrt(np.mean(np.sum((target[n:2 * n] - x) ** 2, axis=1))), rtol=1e-12)
    nt = np.diff(tr['trace_ptr'])[4:8]
    assert np.isclose(np.sum(trace_rmsd[4:8] ** 2 * nt), cell_rmsd[1] ** 2 * n, rtol=1e-12)  # the traces' shares
    # and the joint cost of the oracle at that labelling is the same number
    r = TC.cell_sums(xyz, ix, tr, 1)
    assert abs(TC.joint(r, copy, 2)[0] - want) <= 1e-9 * want
    assert np.all(np.isnan(target[2 * n:])) and np.isnan(cell_rmsd[2]) and np.isnan(trace_rmsd[8])


def test_write_assignment_round_trips_with_cells(tmp_path):
    ix, xyz, tr, x, copy = _exact_cell_and_mirror()
    cell_structure = np.array([2, -1, 0])
    structure = np.repeat(cell_structure, np.diff(tr['cell_ptr']))
    labels = np.where(structure >= 0, np.concatenate([copy, copy, [0]]), -1)
    target, cell_rmsd, trace_rmsd, _ = T.aligned_cell_targets(xyz, ix.copy_ptr, ix.copy_idx, tr, cell_structure, labels)
    path = os.path.join(str(tmp_path), 'a.h5')
    T.write_assignment(path, tr, ix.copy_ptr, ix.copy_idx, structure, labels, target, trace_rmsd,
                       cell_structure=cell_structure, cell_rmsd=cell_rmsd)
    d = T.read_assignment(path, nbead=ix.nbead)
    n = len(x)
    assert d['assignment'].tolist() == [2] * n + [0] * 3 and len(d['locus']) == n + 3
    assert d['locus'][:12].tolist() == TA.beads_of(ix, np.arange(12), 1).tolist()
    assert np.array_equal(d['target'], np.concatenate([target[:n], target[2 * n:]]))
    with h5.File(path) as f:
        assert sorted(f.keys()) == sorted(['locus', 'target', 'assignment', 'trace', 'trace_structure', 'trace_copy',
                                           'trace_rmsd', 'trace_cell', 'cell_structure', 'cell_rmsd'])
        assert np.asarray(f.read('trace_cell')).tolist() == [0] * 4 + [1] * 4 + [2]
        assert np.asarray(f.read('cell_structure')).tolist() == [2, -1, 0]
        assert np.asarray(f.read('trace_copy')).tolist() == copy.tolist() + [-1] * 4 + [0]
        cr, trr = np.asarray(f.read('cell_rmsd')), np.asarray(f.read('trace_rmsd'))
        assert cr[0] == cell_rmsd[0] and np.isnan(cr[1]) and cr[2] == cell_rmsd[2]
        assert np.array_equal(trr[:4], trace_rmsd[:4]) and np.all(np.isnan(trr[4:8]))
    ptr, a = T.anchors_for(d, [0, 1, 2], 75.0, 1.0, nbead=ix.nbead)
    assert ptr.tolist() == [0, 3, 3, n + 3]


# ------------------------------------------------------------------ the Step layer
def _step_config(tmp, cells=True, S=6, ncell=4, nspots=5):
    """the config of tests/test_tracing_assign.py with imaged cells planted on the demo population"""
    import test_steps_de as TD
    cfg, pop = TD._base(tmp, {'nucleus_shape': 'sphere', 'nucleus_radius': 5500.0, 'nucleus_kspring': 1.0}, S=S)
    store = ST.PopulationStore(cfg['optimization']['structure_output'])
    tr, s, k = W.synthetic_cells(store, np.asarray(store.coordinates()), ncell, nspots, 1.0, 3)
    path = os.path.join(tmp, 'traces.h5')
    h5.write(path, {q: tr[q] for q in ('trace_ptr', 'locus', 'position') + (('cell_ptr',) if cells else ())})
    cfg['restraints']['tracing'] = {'input_file': path, 'kspring': 1.0, 'tol_list': [200, 100], 'keep_best': 4}
    cfg['optimization']['kernel_opts']['hip']['tracing_cell_batch'] = 3  # two batches
    return cfg, store, tr, s, k


def test_step_places_planted_cells(tmp_path):
    cfg, store, tr, s, k = _step_config(str(tmp_path))
    TC.register_cpu_kernels()
    cfg['optimization']['kernel'] = 'tracing_cells_test'
    del TC.CALLS[:]
    ST.TracingAssignmentStep(cfg).run()
    assert TC.CALLS == [3, 1]
    path = cfg['runtime']['tracing']['assignment_file']
    assert cfg['runtime']['tracing']['n_unassigned'] == 0 and cfg['runtime']['tracing']['n_cells_unassigned'] == 0
    with h5.File(path) as f:
        got = {q: np.asarray(f.read(q)) for q in ('cell_structure', 'trace_copy', 'trace_structure', 'trace_cell',
                                                  'cell_rmsd', 'trace_rmsd')}
    assert np.array_equal(got['cell_structure'], s) and np.array_equal(got['trace_copy'], k)
    assert len(set(got['cell_structure'].tolist())) == 4  # no structure takes more than one cell
    assert np.array_equal(got['trace_structure'], s[got['trace_cell']])
    assert np.all(got['cell_rmsd'] < 3.0) and np.all(got['trace_rmsd'] < 4.0)  # 1 nm noise: sqrt 3 nm
    d = T.read_assignment(path, nbead=store.nbead)
    assert len(d['locus']) == len(tr['locus'])
    ptr, a = T.anchors_for(d, np.arange(6), 200.0, 1.0, nbead=store.nbead)
    assert np.array_equal(np.diff(ptr), np.bincount(s, minlength=6) * 46 * 5)
    first = int(s[0])  # the anchors of cell 0's structure sit on its beads, up to the 1 nm noise
    sl = slice(int(ptr[first]), int(ptr[first + 1]))
    xb = np.asarray(store.coordinates())[a['atom'][sl], first]
    assert np.abs(np.stack([a['x'][sl], a['y'][sl], a['z'][sl]], axis=1) - xb).max() < 10.0


def test_step_without_cell_ptr_writes_todays_file(tmp_path):
    """the same traces without the dataset: every line of the per-trace path, and its file byte
    for byte (built here from the per-trace functions the step calls)"""
    a, b = tmp_path / 'a', tmp_path / 'b'
    a.mkdir()
    b.mkdir()
    cfg, store, tr, s, k = _step_config(str(a), cells=False)
    TC.register_cpu_kernels()
    cfg['optimization']['kernel'] = 'tracing_cells_test'
    del TC.CALLS[:], TA.CALLS[:]
    ST.TracingAssignmentStep(cfg).run()
    assert TC.CALLS == [] and TA.CALLS == [len(tr['trace_ptr']) - 1]
    assert 'n_cells_unassigned' not in cfg['runtime']['tracing']
    traces = T.check_traces({q: tr[q] for q in ('trace_ptr', 'locus', 'position')}, store.copy_ptr, store.hap_chrom)
    cand, val = TA.cpu_tracing(store, traces, 4, 0)
    pick = T.greedy_assignment(cand, val, traces['chrom'])
    took = np.where(pick >= 0, cand[np.arange(len(pick)), np.maximum(pick, 0)], -1)
    structure, copy = np.where(took >= 0, took // 2, -1), np.where(took >= 0, took % 2, -1)
    target, fit, _ = T.aligned_targets(store.coordinates(), store.copy_ptr, store.copy_idx, traces, structure, copy)
    want = os.path.join(str(b), 'want.h5')
    T.write_assignment(want, traces, store.copy_ptr, store.copy_idx, structure, copy, target, fit)
    with open(cfg['runtime']['tracing']['assignment_file'], 'rb') as f, open(want, 'rb') as g:
        assert f.read() == g.read()
    with h5.File(want) as f:
        assert sorted(f.keys()) == sorted(['locus', 'target', 'assignment', 'trace', 'trace_structure', 'trace_copy',
                                           'trace_rmsd'])
