"""The joint placement of the traces of an imaged cell on the GPU, through the C ABI
(igm_tracing_assign_cells): cost, labelling and rounds against the fp64 oracle of
tests/tracing_cells.py, the selection against a stable argsort of the library's own costs, block
and wave edges, ties, every cell shape, batching, the errors, a rerun, and TracingAssignmentStep
on the hip kernel.

The bound of every cost (tracing_assign.bound, as for the per-trace A-step):
    |cost_gpu - cost_ref| <= 1e-6 cost_ref + sqrt(1e-12 (Ga + Gb) / n).
Labels and rounds are compared wherever every choice of the oracle's search had a decision margin
above 1e-9 (tracing_cells.choose): below it the order of two labelling sums is rounding.
"""
import os

import numpy as np
import pytest

import tracing_assign as TA
import tracing_cells as TC
from igm_amd import _lib, h5
from igm_amd import steps as ST
from igm_amd import tracing as T
from igm_amd import workloads as W

pytestmark = pytest.mark.gpu

MARGIN = 1e-9
REC = 13 * 8  # bytes of a (trace, copy, structure) record


@pytest.fixture(scope='module')
def ctx():
    return _lib.context(0)


@pytest.fixture(scope='module')
def proto():
    """the inputs of tests/test_tracing_cells.py::proto and their oracle"""
    ix, xyz = TC.genome(24, seed=1)
    tr, s, k = TC.planted(ix, xyz)
    return ix, xyz, tr, s, k, TC.cells_oracle(xyz, ix, tr)


def _run(ctx, ix, xyz, tr, kb=1, **kw):
    return T.assign_cell_costs(xyz, ix.copy_ptr, ix.copy_idx, tr, kb, ctx=ctx, return_full=True, **kw)


def _against_oracle(what, out, o, tr, every_margin=False):
    """cost within the bound everywhere; label and rounds equal where the margins allow"""
    bs, bv, bl, cost, label, rounds = out
    err, lim = np.abs(cost.astype(np.float64) - o['cost']), TA.bound(o['cost'], o['scale'])
    ok = o['margin'] > MARGIN
    print('%s: max |gpu - ref| / bound = %.3g; %d of %d pairs compared on labels, smallest margin %.3g' % (
        what, (err / lim).max(), ok.sum(), ok.size, o['margin'].min()))
    assert cost.dtype == np.float32 and not np.any(np.isnan(cost))
    assert np.all(err <= lim)
    if every_margin:
        assert np.all(ok)
    okt = ok[np.repeat(np.arange(len(ok)), np.diff(tr['cell_ptr']))]
    assert np.array_equal(label[okt], o['label'][okt])
    assert np.array_equal(rounds[ok], o['rounds'][ok])
    return ok


def _selection_holds(out, tr, kb):
    bs, bv, bl, cost, label, rounds = out
    ws, wv, wl = TC.select(cost, label, tr['cell_ptr'], kb)
    assert bs.shape == (len(cost), kb) and bl.shape == (len(label), kb)
    assert np.array_equal(bs, ws) and np.array_equal(bv, wv) and np.array_equal(bl, wl)


# ------------------------------------------------------------------ the prototype's inputs
def test_costs_labels_and_rounds_equal_the_oracle(ctx, proto):
    ix, xyz, tr, s, k, o = proto
    out = _run(ctx, ix, xyz, tr, 5)
    _against_oracle('prototype', out, o, tr, every_margin=True)
    bs, bv, bl, cost, label, rounds = out
    assert np.array_equal(bs[:, 0], s) and np.array_equal(bl[:, 0], k)  # every planted cell and labelling
    assert rounds.max() <= 8 and rounds.min() >= 1
    total = ctx.kernel_ms('tracing_cells')
    parts = [ctx.kernel_ms(q) for q in ('tracing_cell_sums', 'tracing_cell_search', 'tracing_cell_select')]
    assert min(parts) > 0.0 and abs(total - sum(parts)) <= 1e-9 * total


@pytest.mark.parametrize('kb', [1, 5, 24])
def test_selection_is_a_stable_argsort_of_the_librarys_costs(ctx, proto, kb):
    ix, xyz, tr, s, k, o = proto
    _selection_holds(_run(ctx, ix, xyz, tr, kb), tr, kb)


def test_batching_does_not_change_a_bit(ctx, proto):
    """18 cells of 10 traces, 2 copies at most: a scratch of exactly one cell's records makes 18
    batches; one byte less is refused and the context goes on working"""
    ix, xyz, tr, s, k, o = proto
    one = 10 * 2 * REC * 24
    whole = _run(ctx, ix, xyz, tr, 5)
    for scratch in (one, 3 * one + 7):
        split = _run(ctx, ix, xyz, tr, 5, scratch_bytes=scratch)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(whole, split))
    assert ctx.kernel_ms('tracing_cells') > 0.0
    with pytest.raises(RuntimeError, match=r'code -5.*cell 0 needs %d bytes' % one):
        _run(ctx, ix, xyz, tr, 5, scratch_bytes=one - 1)
    again = _run(ctx, ix, xyz, tr, 5)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(whole, again))  # a rerun is bitwise equal


# ------------------------------------------------------------------ block and wave edges, ties
@pytest.mark.parametrize('S', [1, 63, 64, 65, 255, 256, 257])
def test_block_and_wave_edges(ctx, S):
    ix, xyz = TC.genome(S, seed=S)
    tr, s, k = TC.planted(ix, xyz, ncell=1, noise=(30.0,), seed=S)
    out = _run(ctx, ix, xyz, tr, S)
    _against_oracle('S %d' % S, out, TC.cells_oracle(xyz, ix, tr), tr)
    _selection_holds(out, tr, S)
    assert out[0][0, 0] == s[0] and np.array_equal(out[2][:, 0], k)


def test_identical_structures_tie_to_the_lower(ctx):
    ix, xyz = TC.genome(65, seed=2)
    xyz[:, 64] = xyz[:, 9]
    xyz[:, 3] = xyz[:, 9]
    tr, s, k = TC.planted(ix, xyz, ncell=2, noise=(30.0,), seed=6)
    bs, bv, bl, cost, label, rounds = out = _run(ctx, ix, xyz, tr, 65)
    for q in (cost, rounds, label):
        assert np.array_equal(q[:, 3], q[:, 9]) and np.array_equal(q[:, 64], q[:, 9])
    _selection_holds(out, tr, 65)
    for c in range(2):
        pos = {int(v): r for r, v in enumerate(bs[c])}
        assert pos[9] == pos[3] + 1 and pos[64] == pos[3] + 2


# ------------------------------------------------------------------ cell shapes
def test_one_trace_cells_are_the_per_trace_a_step(ctx):
    """cells of one trace: cost within the bound of min_k of igm_tracing_assign's matrix, the
    label its argmin"""
    ix, xyz = TC.genome(9, seed=4)
    tr, s, k = TC.planted(ix, xyz, ncell=3, seed=8)
    tr = T.check_traces(dict(tr, cell_ptr=np.arange(len(tr['ncopy']) + 1)), ix.copy_ptr, ix.hap_chrom)
    _, _, full = T.assign_costs(xyz, ix.copy_ptr, ix.copy_idx, tr, 1, ctx=ctx, return_full=True)
    bs, bv, bl, cost, label, rounds = _run(ctx, ix, xyz, tr, 1)
    ref, scale = TA.oracle_rmsd(xyz, ix, tr)
    want = full.min(axis=2).astype(np.float64)
    lim = TA.bound(want, np.take_along_axis(scale, np.argmin(ref, axis=2)[:, :, None], axis=2)[:, :, 0])
    assert np.all(np.abs(cost - want) <= lim)
    gap = np.abs(np.diff(np.sort(np.where(np.isfinite(ref), ref, np.inf), axis=2)[:, :, :2], axis=2))[:, :, 0]
    clear = ~(gap <= 2.0 * lim)  # (single-copy: inf or NaN gap, clear)
    assert np.array_equal(label[clear], np.argmin(full, axis=2)[clear]) and clear.mean() > 0.8
    assert np.all(rounds == 1)


def _copies_genome(S, seed):
    # 3 and 4 copies, a single-copy and a diploid chromosome
    return TC.genome(S, seed=seed, chroms=((0, 10, 3), (1, 9, 4), (2, 8, 1), (3, 8, 2)))


@pytest.mark.parametrize('full_house', [True, False])
def test_three_and_four_copies(ctx, full_house):
    """full house: 3 of 3 and 4 of 4 homologues imaged (6 and 24 labellings); otherwise 2 of 3
    and 3 of 4 (6 and 24 again), and one of the diploid chromosome's two"""
    ix, xyz = _copies_genome(7, 12)
    tr, s, k = W.synthetic_cells(ix, xyz, 5, 6, [0.0, 20.0, 20.0, 100.0, 100.0], 4)
    if not full_house:
        chrom = ix.hap_chrom[tr['locus'][tr['trace_ptr'][:-1]]]
        keep = ~(((chrom == 0) & (k == 1)) | ((chrom == 1) & (k == 2)) | ((chrom == 3) & (k == 0)))
        tr, k = TC.drop(tr, keep), k[keep]
    tr = T.check_traces(tr, ix.copy_ptr, ix.hap_chrom)
    assert np.diff(tr['cell_ptr']).tolist() == [10 if full_house else 7] * 5
    out = _run(ctx, ix, xyz, tr, 7)
    ok = _against_oracle('copies %s' % full_house, out, TC.cells_oracle(xyz, ix, tr), tr)
    _selection_holds(out, tr, 7)
    assert ok[np.arange(5), s].all()
    assert np.array_equal(out[0][:, 0], s) and np.array_equal(out[2][:, 0], k)


def test_a_cell_of_128_traces_and_the_refusal_at_129(ctx):
    ix, xyz = TC.genome(3, seed=7, chroms=tuple((c, 3, 4) for c in range(33)))
    tr, s, k = W.synthetic_cells(ix, xyz, 1, 3, 25.0, 9)
    assert len(k) == 132
    big = T.check_traces(TC.drop(tr, np.arange(132) < 128), ix.copy_ptr, ix.hap_chrom)
    out = _run(ctx, ix, xyz, big, 3)
    ok = _against_oracle('128 traces', out, TC.cells_oracle(xyz, ix, big), big)
    assert ok[0, s[0]] and out[0][0, 0] == s[0] and np.array_equal(out[2][:, 0], k[:128])
    over = T.check_traces(TC.drop(tr, np.arange(132) < 129), ix.copy_ptr, ix.hap_chrom)
    with pytest.raises(RuntimeError, match='code -5.*cell 0 has 129 traces'):
        _run(ctx, ix, xyz, over, 3)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(out, _run(ctx, ix, xyz, big, 3)))  # the context lives


def test_more_than_four_copies_is_refused(ctx):
    ix, xyz = TC.genome(2, seed=1, chroms=((0, 4, 5),))
    tr = T.check_traces(W.synthetic_cells(ix, xyz, 1, 4, 1.0, 0)[0], ix.copy_ptr, ix.hap_chrom)
    with pytest.raises(RuntimeError, match='code -5.*5 copies'):
        _run(ctx, ix, xyz, tr, 1)


def test_a_trace_longer_than_the_lds_chunk(ctx, monkeypatch):
    """129 spots: two of the default 128-spot chunks"""
    monkeypatch.delenv('IGM_TRACING_CHUNK', raising=False)
    ix, xyz = TC.genome(5, seed=3, chroms=((0, 129, 2), (1, 129, 1)))
    tr, s, k = W.synthetic_cells(ix, xyz, 2, 129, 25.0, 2)
    tr = T.check_traces(tr, ix.copy_ptr, ix.hap_chrom)
    out = _run(ctx, ix, xyz, tr, 2)
    _against_oracle('129 spots', out, TC.cells_oracle(xyz, ix, tr), tr)
    assert np.array_equal(out[0][:, 0], s) and np.array_equal(out[2][:, 0], k)


# ------------------------------------------------------------------ errors
def _raw(ctx, ix, xyz, tr, kb, cell_ptr=None, chrom=None, scratch=0):
    xyz = np.ascontiguousarray(xyz, np.float32)
    ptr, locus = np.asarray(tr['trace_ptr'], np.int64), np.asarray(tr['locus'], np.int32)
    pos = np.ascontiguousarray(tr['position'], np.float32)
    cp = np.asarray(tr['cell_ptr'] if cell_ptr is None else cell_ptr, np.int64)
    chrom = np.asarray(tr['chrom'] if chrom is None else chrom, np.int32)
    T_, nc = len(ptr) - 1, len(cp) - 1
    bs, bv = np.zeros((max(nc, 1), max(kb, 1)), np.int32), np.zeros((max(nc, 1), max(kb, 1)), np.float32)
    bl = np.zeros((T_, max(kb, 1)), np.uint8)
    rc = ctx.lib.igm_tracing_assign_cells(ctx.h, 0, xyz.ctypes.data, xyz.shape[0], xyz.shape[1], ix.copy_ptr.ctypes.data,
                                          ix.copy_idx.ctypes.data, len(ix.copy_ptr) - 1, T_, ptr.ctypes.data,
                                          locus.ctypes.data, pos.ctypes.data, chrom.ctypes.data, nc, cp.ctypes.data, kb,
                                          scratch, None, None, None, bs.ctypes.data, bv.ctypes.data, bl.ctypes.data)
    return rc, ctx.lib.igm_last_error(ctx.h).decode(), bs


def test_errors_leave_the_context_usable(ctx):
    ix, xyz = TC.genome(4, seed=3)
    tr, s, k = TC.planted(ix, xyz, ncell=2, noise=(10.0,), seed=1)  # 2 cells of 10 traces
    rc, _, good = _raw(ctx, ix, xyz, tr, 2)
    assert rc == _lib.IGM_OK and good[:, 0].tolist() == s.tolist()
    one_chrom = np.zeros(20, np.int32)  # every trace called chromosome 0: three of a diploid one
    cases = {
        'cell_ptr[0]': dict(cell_ptr=[1, 10, 20]),
        'cell_ptr not monotone': dict(cell_ptr=[0, 12, 10, 20]),
        'an empty cell': dict(cell_ptr=[0, 10, 10, 20]),
        'cell_ptr short of T': dict(cell_ptr=[0, 10, 19]),
        'cell_ptr past T': dict(cell_ptr=[0, 10, 21]),
        'too many traces of a chromosome': dict(chrom=one_chrom),
        'two cells merged': dict(cell_ptr=[0, 20]),
        'keep_best 0': dict(kb=0),
        'keep_best over S': dict(kb=5),
    }
    for what, kw in cases.items():
        rc, msg, _ = _raw(ctx, ix, xyz, tr, kw.pop('kb', 2), **kw)
        assert rc == _lib.IGM_E_INVALID and msg.startswith('igm_tracing_assign_cells:'), (what, rc, msg)
        rc, _, bs = _raw(ctx, ix, xyz, tr, 2)
        assert rc == _lib.IGM_OK and np.array_equal(bs, good), what
    rc, msg, _ = _raw(ctx, ix, xyz, tr, 2, scratch=10 * 2 * REC * 4 - 1)
    assert rc == _lib.IGM_E_UNSUPPORTED and 'scratch' in msg
    assert _raw(ctx, ix, xyz, tr, 2, scratch=-1)[0] == _lib.IGM_E_INVALID
    assert np.array_equal(_raw(ctx, ix, xyz, tr, 2)[2], good)
    bad = dict(tr, trace_ptr=np.concatenate([tr['trace_ptr'][:-1], [tr['trace_ptr'][-1] - 6]]))  # the last trace: 2 spots
    rc, msg, _ = _raw(ctx, ix, xyz, bad, 2)
    assert rc == _lib.IGM_E_INVALID and 'fewer than 3' in msg


# ------------------------------------------------------------------ the Step layer
def test_step_with_the_hip_kernel(tmp_path):
    """S = 24, 12 cells of 46 traces planted on the demo population with 30 nm noise, two batches
    of cells: every planted cell gets its structure and its labelling"""
    import test_steps_de as TD
    tmp = str(tmp_path)
    cfg, pop = TD._base(tmp, {'nucleus_shape': 'sphere', 'nucleus_radius': 5500.0, 'nucleus_kspring': 1.0}, S=24)
    store = ST.PopulationStore(cfg['optimization']['structure_output'])
    tr, s, k = W.synthetic_cells(store, np.asarray(store.coordinates()), 12, 8, 30.0, 5)
    path = os.path.join(tmp, 'cells.h5')
    h5.write(path, {q: tr[q] for q in ('trace_ptr', 'locus', 'position', 'cell_ptr')})
    cfg['restraints']['tracing'] = {'input_file': path, 'kspring': 1.0, 'tol_list': [200], 'keep_best': 50}
    cfg['optimization']['kernel'] = 'hip'
    cfg['optimization']['kernel_opts']['hip']['tracing_cell_batch'] = 8
    ST.TracingAssignmentStep(cfg).run()
    rt = cfg['runtime']['tracing']
    assert rt['n_unassigned'] == 0 and rt['n_cells_unassigned'] == 0
    with h5.File(rt['assignment_file']) as f:
        cs, tc, cr = (np.asarray(f.read(q)) for q in ('cell_structure', 'trace_copy', 'cell_rmsd'))
    assert np.array_equal(cs, s) and np.array_equal(tc, k)
    print('cell rmsd %.1f .. %.1f nm (noise sqrt 3 = %.1f)' % (cr.min(), cr.max(), 30.0 * np.sqrt(3.0)))
    assert np.all(cr < 2.0 * 30.0 * np.sqrt(3.0))
    d = T.read_assignment(rt['assignment_file'], nbead=store.nbead)
    assert len(d['locus']) == len(tr['locus']) == 12 * 46 * 8
