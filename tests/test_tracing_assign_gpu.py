"""The chromatin tracing A-step on the GPU, through the C ABI (igm_tracing_assign): the cost
matrix against the fp64 Kabsch oracle of tests/tracing_assign.py, exact and mirrored traces, the
keep_best selection (LDS sort and counting fallback) against a stable argsort of the library's
own matrix, the errors, the recovery of planted traces, and run_pipeline on the hip kernels.

The bound of every comparison with the oracle (tracing_assign.bound):
    |rmsd_gpu - rmsd_ref| <= 1e-6 rmsd_ref + sqrt(1e-12 (Ga + Gb) / n)
the f32 rounding of the output, and about 4500 fp64 ulps of the sums that cancel in
Ga + Gb - 2 lambda.
"""
import json
import os

import numpy as np
import pytest

import tracing_assign as TA
from igm_amd import _lib, h5
from igm_amd import igm_run as RUN
from igm_amd import steps as ST
from igm_amd import tracing as T
from igm_amd import workloads as W

pytestmark = pytest.mark.gpu

CHUNK = 8            # IGM_TRACING_CHUNK of the parity cases: a 9-spot trace takes two chunks
SORT_LIMIT = 8192    # candidates the LDS sort takes; above it the counting pass runs


@pytest.fixture(scope='module')
def ctx():
    return _lib.context(0)


def _rigid(rng, x, shift=3000.0):
    return (x - x.mean(axis=0)) @ W.random_rotation(rng).T + rng.normal(0.0, shift, 3)


def _parity_traces(ix, xyz, seed):
    """3 spots; one spot more than the LDS chunk; a collinear trace; two coincident spots; noisy
    copies of the model on every chromosome (A, B diploid, C single-copy)"""
    rng = np.random.default_rng(seed)
    S = xyz.shape[1]
    cut = lambda loci, k, s: xyz[TA.beads_of(ix, loci, k), s].astype(np.float64)
    items = [([2, 5, 6], _rigid(rng, cut([2, 5, 6], 1, S - 1)) + rng.normal(0, 20.0, (3, 3))),
             (np.arange(0, CHUNK + 1), _rigid(rng, cut(np.arange(0, CHUNK + 1), 0, 0)) + rng.normal(0, 30.0, (CHUNK + 1, 3))),
             (np.arange(21, 21 + CHUNK + 1), _rigid(rng, cut(np.arange(21, 21 + CHUNK + 1), 0, S // 2))),
             ([12, 14, 15, 19], np.outer([0.0, 1.0, 2.5, 7.0], [60.0, -20.0, 35.0]) + 400.0),  # collinear
             ([22, 23, 27, 30, 33], None),  # two coincident spots (below)
             (np.arange(21, 35), rng.normal(0.0, 300.0, (14, 3)))]  # unrelated to the model
    p = _rigid(rng, cut([22, 23, 27, 30, 33], 0, 0))
    p[3] = p[1]
    items[4] = (items[4][0], p)
    return T.check_traces(TA.traces_of(items), ix.copy_ptr, ix.hap_chrom)


@pytest.mark.parametrize('S', [1, 65, 257])
def test_cost_matrix_equals_the_oracle(ctx, monkeypatch, S):
    monkeypatch.setenv('IGM_TRACING_CHUNK', str(CHUNK))
    ix, xyz = TA.model(S, seed=S)
    tr = _parity_traces(ix, xyz, 100 + S)
    ref, scale = TA.oracle_rmsd(xyz, ix, tr)
    cand, val, full = T.assign_costs(xyz, ix.copy_ptr, ix.copy_idx, tr, 1, ctx=ctx, return_full=True)
    assert full.shape == ref.shape == (6, S, 2) and full.dtype == np.float32
    assert np.array_equal(np.isinf(full), np.isinf(ref))  # +inf exactly where k >= C_t
    assert np.all(np.isinf(full[[2, 4, 5], :, 1])) and np.all(np.isfinite(full[[0, 1, 3]]))
    ok = np.isfinite(ref)
    err, lim = np.abs(full.astype(np.float64)[ok] - ref[ok]), TA.bound(ref[ok], scale[ok])
    print('S %d: max |gpu - ref| / bound = %.3g, max rel %.3g' % (S, (err / lim).max(), (err / ref[ok]).max()))
    assert np.all(err <= lim)
    assert ctx.kernel_ms('tracing_assign') > 0.0 and ctx.kernel_ms('tracing_cost') > 0.0
    assert ctx.kernel_ms('tracing_select') > 0.0


def test_long_trace_at_the_default_chunk(ctx, monkeypatch):
    """129 and 300 spots: two and three of the default 128-spot chunks"""
    monkeypatch.delenv('IGM_TRACING_CHUNK', raising=False)
    ix, xyz = TA.chain_model(300, 70, seed=2)
    rng = np.random.default_rng(3)
    items = [(np.arange(50, 179), _rigid(rng, xyz[50:179, 69].astype(np.float64)) + rng.normal(0, 25.0, (129, 3))),
             (np.arange(300), _rigid(rng, xyz[:, 3].astype(np.float64)) + rng.normal(0, 25.0, (300, 3)))]
    tr = T.check_traces(TA.traces_of(items), ix.copy_ptr, ix.hap_chrom)
    ref, scale = TA.oracle_rmsd(xyz, ix, tr)
    cand, val, full = T.assign_costs(xyz, ix.copy_ptr, ix.copy_idx, tr, 2, ctx=ctx, return_full=True)
    err = np.abs(full.astype(np.float64) - ref)
    print('max |gpu - ref| / bound = %.3g' % (err / TA.bound(ref, scale)).max())
    assert np.all(err <= TA.bound(ref, scale))
    assert cand[:, 0].tolist() == [69, 3]


def test_exact_and_mirrored_trace(ctx, monkeypatch):
    """A trace cut from a structure's own beads, turned and shifted without rounding (model
    coordinates are multiples of 1/64 nm, the rotation an axis permutation, the shift whole nm):
    its true rmsd is 0, so the GPU's is within the cancellation term and never NaN.  Its mirror
    image must not score 0."""
    monkeypatch.setenv('IGM_TRACING_CHUNK', str(CHUNK))
    ix, xyz = TA.model(65, seed=5)
    loci = np.arange(12, 21)
    x = xyz[TA.beads_of(ix, loci, 1), 40].astype(np.float64)
    p = x @ TA.PERM.T + np.array([1024.0, -512.0, 256.0])
    tr = TA.traces_of([(loci, p), (loci, p * np.array([-1.0, 1.0, 1.0]))])
    assert np.array_equal(tr['position'][:9].astype(np.float64), p)
    tr = T.check_traces(tr, ix.copy_ptr, ix.hap_chrom)
    ref, scale = TA.oracle_rmsd(xyz, ix, tr)
    cand, val, full = T.assign_costs(xyz, ix.copy_ptr, ix.copy_idx, tr, 3, ctx=ctx, return_full=True)
    assert not np.any(np.isnan(full))
    print('exact: gpu %.3g, oracle %.3g, floor %.3g; mirrored: gpu %.6f, oracle %.6f' % (
        full[0, 40, 1], ref[0, 40, 1], TA.noise_floor(scale[0, 40, 1]), full[1, 40, 1], ref[1, 40, 1]))
    assert 0.0 <= full[0, 40, 1] <= TA.noise_floor(scale[0, 40, 1])
    assert cand[0, 0] == 40 * 2 + 1 and val[0, 0] == full[0, 40, 1]
    assert ref[1, 40, 1] > 1000.0 * TA.noise_floor(scale[1, 40, 1])  # the oracle's value is above the noise
    assert full[1, 40, 1] > 10.0
    assert np.all(np.abs(full.astype(np.float64) - ref) <= TA.bound(ref, scale))


@pytest.mark.parametrize('S,diploid_only', [(1, False), (65, False), (65, True), (257, True)])
def test_selection_is_a_stable_argsort_of_the_librarys_matrix(ctx, monkeypatch, S, diploid_only):
    monkeypatch.setenv('IGM_TRACING_CHUNK', str(CHUNK))
    ix, xyz = TA.model(S, seed=20 + S)
    if S > 1:
        xyz[:, S - 1] = xyz[:, 0]  # two identical structures: every cost of a trace ties once
        xyz[:, 7] = xyz[:, 0]
    tr = _parity_traces(ix, xyz, 200 + S)
    if diploid_only:
        tr = T.check_traces(TA.traces_of([(tr['locus'][a:b], tr['position'][a:b]) for a, b in
                                          zip(tr['trace_ptr'][:-1], tr['trace_ptr'][1:]) if tr['locus'][a] < 21]),
                            ix.copy_ptr, ix.hap_chrom)
    most = S * int(tr['ncopy'].min())  # keep_best = S * C_t of the trace with the fewest candidates
    for kb in sorted({1, min(50, most), most}):
        cand, val, full = T.assign_costs(xyz, ix.copy_ptr, ix.copy_idx, tr, kb, ctx=ctx, return_full=True)
        want_c, want_v = TA.select(full, kb)
        assert cand.shape == (len(tr['ncopy']), kb)
        assert np.array_equal(cand, want_c) and np.array_equal(val, want_v)
        if S > 1:
            assert np.array_equal(full[:, 0], full[:, S - 1]) and np.array_equal(full[:, 0], full[:, 7])
    if S > 1 and most >= 2 * S:  # the whole row is ranked: the tied structures sit side by side, lower first
        pos = {int(c): r for r, c in enumerate(cand[0])}
        assert pos[7 * 2] == pos[0] + 1 and pos[(S - 1) * 2] == pos[0] + 2


def test_selection_past_the_lds_limit_counts(ctx):
    """1 trace of 3 spots on 8 beads: S * C one above the LDS sort's limit takes the counting
    pass; the same rule, ties included"""
    S = SORT_LIMIT + 1
    ix, xyz = TA.chain_model(8, S, seed=9)
    xyz[:, 5000] = xyz[:, 17]
    xyz[:, S - 1] = xyz[:, 17]
    rng = np.random.default_rng(4)
    tr = T.check_traces(TA.traces_of([([1, 4, 6], _rigid(rng, xyz[[1, 4, 6], 17].astype(np.float64)))]),
                        ix.copy_ptr, ix.hap_chrom)
    for kb in (1, 50, S):
        cand, val, full = T.assign_costs(xyz, ix.copy_ptr, ix.copy_idx, tr, kb, ctx=ctx, return_full=True)
        want_c, want_v = TA.select(full, kb)
        assert np.array_equal(cand, want_c) and np.array_equal(val, want_v)
    assert cand[0, :3].tolist() == [17, 5000, S - 1]
    # and one below the limit the sort gives the same ranking of the same structures
    c2, v2 = T.assign_costs(xyz[:, :SORT_LIMIT], ix.copy_ptr, ix.copy_idx, tr, 50, ctx=ctx)
    keep = cand[0][cand[0] < SORT_LIMIT][:50]
    assert np.array_equal(c2[0], keep)


def _raw(ctx, ix, xyz, ptr, locus, pos, kb):
    xyz = np.ascontiguousarray(xyz, np.float32)
    ptr, locus, pos = np.asarray(ptr, np.int64), np.asarray(locus, np.int32), np.ascontiguousarray(pos, np.float32)
    T_ = len(ptr) - 1
    bc, bv = np.zeros((T_, max(kb, 1)), np.int32), np.zeros((T_, max(kb, 1)), np.float32)
    rc = ctx.lib.igm_tracing_assign(ctx.h, 0, xyz.ctypes.data, xyz.shape[0], xyz.shape[1], ix.copy_ptr.ctypes.data,
                                    ix.copy_idx.ctypes.data, len(ix.copy_ptr) - 1, T_, ptr.ctypes.data,
                                    locus.ctypes.data, pos.ctypes.data, kb, None, bc.ctypes.data, bv.ctypes.data)
    return rc, ctx.lib.igm_last_error(ctx.h).decode()


def test_errors(ctx):
    """every malformed input returns IGM_E_INVALID with a message; the validation is on the
    host, before any launch"""
    ix, xyz = TA.model(4)
    pos = np.random.default_rng(0).normal(0, 100, (7, 3))
    good = ([0, 4, 7], [0, 3, 4, 7, 21, 22, 30], pos, 4)
    assert _raw(ctx, ix, xyz, *good)[0] == _lib.IGM_OK
    bad_pos = pos.copy()
    bad_pos[5, 2] = np.nan
    cases = {
        'trace_ptr not monotone': ([0, 7, 4], good[1], pos, 4),
        'fewer than 3 spots': ([0, 5, 7], good[1], pos, 4),
        'locus past nhap': (good[0], [0, 3, 4, 7, 21, 22, 35], pos, 4),
        'negative locus': (good[0], [-1, 3, 4, 7, 21, 22, 30], pos, 4),
        'loci not increasing': (good[0], [0, 3, 3, 7, 21, 22, 30], pos, 4),
        'two chromosomes': (good[0], [0, 3, 4, 21, 22, 23, 30], pos, 4),
        'non-finite position': (good[0], good[1], bad_pos, 4),
        'keep_best 0': (good[0], good[1], pos, 0),
        'keep_best over S * C_t': (good[0], good[1], pos, 5),  # the single-copy trace has 4 candidates
    }
    for what, args in cases.items():
        rc, msg = _raw(ctx, ix, xyz, *args)
        assert rc == _lib.IGM_E_INVALID and msg.startswith('igm_tracing_assign:'), (what, rc, msg)
    assert _raw(ctx, ix, xyz, good[0], good[1], pos, 8)[0] == _lib.IGM_E_INVALID
    assert _raw(ctx, ix, xyz, [0, 4], good[1][:4], pos[:4], 8)[0] == _lib.IGM_OK  # a diploid trace alone: 8
    with pytest.raises(RuntimeError, match='keep_best'):
        T.assign_costs(xyz, ix.copy_ptr, ix.copy_idx, {'trace_ptr': good[0], 'locus': good[1], 'position': pos}, 5,
                       ctx=ctx)


def test_planted_traces_are_recovered(ctx, monkeypatch):
    """8 structures, one trace planted on every (structure, chromosome, copy) slot with 1 nm
    noise (the inputs of test_tracing_assign.test_planted_traces_are_recovered_by_the_oracle,
    where the oracle alone recovers them): the greedy assignment on the GPU's candidates
    recovers every planted slot, and the superposition of each winner has the cost the GPU gave."""
    monkeypatch.delenv('IGM_TRACING_CHUNK', raising=False)
    ix, xyz = TA.model(8, seed=11)
    tr, s, k = W.synthetic_traces(ix, xyz, 40, 8, 1.0, 7)
    tr = T.check_traces(tr, ix.copy_ptr, ix.hap_chrom)
    ref, scale = TA.oracle_rmsd(xyz, ix, tr)
    oc, ov = TA.select(ref.astype(np.float32), 8)
    op = T.greedy_assignment(oc, ov, tr['chrom'])
    took = oc[np.arange(40), op]
    assert np.all(op >= 0) and np.array_equal(took // 2, s) and np.array_equal(took % 2, k)  # the oracle first
    cand, val = T.assign_costs(xyz, ix.copy_ptr, ix.copy_idx, tr, 8, ctx=ctx)
    pick = T.greedy_assignment(cand, val, tr['chrom'])
    assert np.all(pick >= 0)
    took = cand[np.arange(40), pick]
    assert np.array_equal(took // 2, s) and np.array_equal(took % 2, k)
    target, fit, rot = T.aligned_targets(xyz, ix.copy_ptr, ix.copy_idx, tr, took // 2, took % 2)
    won = val[np.arange(40), pick].astype(np.float64)
    lim = TA.bound(fit, scale[np.arange(40), s, k])
    print('max |aligned - best_rmsd| / bound = %.3g; rmsd %.3f .. %.3f' % ((np.abs(won - fit) / lim).max(), fit.min(),
                                                                           fit.max()))
    assert np.all(np.abs(won - fit) <= lim)
    assert np.allclose(np.linalg.det(rot), 1.0, rtol=0, atol=1e-12)


def test_run_pipeline_with_hip_kernels(tmp_path):
    """input_file only, tol_list of two values, optimization/kernel = 'hip', from the demo
    population: every iteration leaves a valid assignment file, the earlier one rotated, and the
    M-step's summary carries 'Tracing' with one restraint per assigned spot."""
    import test_tracing_assign as TT
    tmp = str(tmp_path)
    cfg, pop, tr, planted_s, planted_k = TT._config(tmp)
    cfg['optimization']['kernel'] = 'hip'
    seen = []

    def on_iteration(c, it, steps):
        f = c['runtime']['tracing']['assignment_file']
        d = T.read_assignment(f, nbead=len(pop['radii']))
        with h5.File(f) as g:
            ts, tc = np.asarray(g.read('trace_structure')), np.asarray(g.read('trace_copy'))
        summ = json.loads(ST.PopulationStore(c['optimization']['structure_output']).read_summary())
        seen.append(([s.__name__ for s in steps], c['runtime']['tracing']['tol'], len(d['locus']), ts.tolist(),
                     tc.tolist(), sorted(os.listdir(os.path.dirname(f))),
                     summ['byrestraint']['Tracing']['n_imposed']))
    assert RUN.run_pipeline(cfg, on_iteration=on_iteration) == 'completed'
    names = ['TracingAssignmentStep', 'ActivationDistanceStep', 'ModelingStep']
    assert [(s[0], s[1]) for s in seen] == [(names, 200), (names, 100)]
    # the traces were planted on the starting population with 1 nm noise: the first assignment finds them
    assert seen[0][3] == planted_s.tolist() and seen[0][4] == planted_k.tolist()
    for s in seen:
        assert s[2] == len(tr['locus']) == s[6] and min(s[3]) >= 0
    assert seen[0][5] == ['tracing_assignment.h5']
    assert seen[1][5] == ['tracing_assignment.h5', 'tracing_assignment.h5.tol_100.0000.iter_0']
    assert cfg['runtime']['tracing']['n_unassigned'] == 0
