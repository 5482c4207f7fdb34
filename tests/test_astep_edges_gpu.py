"""The Hi-C A-step kernels (igm_amd/csrc/actdist.hip) bit for bit against the CPU oracle on the
inputs of tests/astep_edges.py: every selection width and both sides of every width boundary,
loci with one to four copies, the f32 contact threshold one ulp off, the '%.4f' decimal ties,
round-half-even of the order index, the refusal past 65536 keys, the row capacity, the
device-pointer callers and igm_astep_update_plast.  test_astep_edges.py proves on the CPU that
the inputs are those edges and that the oracle equals the reference on this genome."""
import ctypes
import functools

import numpy as np
import pytest

import astep_edges as E
import oracle
from conftest import load_golden, make_pairs

pytestmark = pytest.mark.gpu

CR2_S = (64, 65, 4096, 4097, 16384)    # the populations that also run contact range 1.3


@pytest.fixture(scope='module')
def astep():
    from igm_amd import astep as a
    return a


@pytest.fixture(scope='module')
def ctx():
    from igm_amd import _lib
    return _lib.context(0)


@functools.lru_cache(maxsize=None)
def case(S):
    """(xyz, radii, the pairs within 65536 keys, their n)"""
    xyz, radii = E.population(S)
    p, n, ok = E.pairs(S)
    return xyz, radii, np.ascontiguousarray(p[ok]), n[ok]


@functools.lru_cache(maxsize=None)
def oracle_case(S, cr, it_corr):
    xyz, radii, p, _ = case(S)
    return oracle.actdist(*E.genome_args(xyz), p, cr, it_corr, nthreads=16)


def same_per_pair(res, ores):
    assert np.array_equal(res['nrows'], ores['nrows'])
    assert np.array_equal(res['o'], ores['o'])
    for k in ('pnow', 'p', 'ad'):
        assert np.array_equal(res[k], ores[k], equal_nan=True), k


def same(rows, res, orows, ores):
    same_per_pair(res, ores)
    assert rows.tobytes() == orows.tobytes()


def no_combination_pairs_are_empty(p, res):
    bad = (p['i'] < 0) | (p['j'] >= E.NHAP) | (p['i'] == p['j'])
    assert bad.any()
    assert np.all(res['nrows'][bad] == 0) and np.all(res['o'][bad] == -1)
    assert np.all(np.isnan(res['ad'][bad]) & np.isnan(res['p'][bad]) & np.isnan(res['pnow'][bad]))


# ---------------------------------------------------------------------------- widths and ploidy
@pytest.mark.parametrize('it_corr', [0, 1])
@pytest.mark.parametrize('S', E.S_LIST)
def test_gpu_every_width(astep, S, it_corr):
    xyz, radii, p, n = case(S)
    assert len(p) % 64 and len(p) % 256
    rows, res = astep.compute_actdist(*E.genome_args(xyz), p, 2.0, it_corr, return_per_pair=True)
    same(rows, res, *oracle_case(S, 2.0, it_corr))
    no_combination_pairs_are_empty(p, res)
    has = res['nrows'] > 0
    assert np.array_equal(res['nrows'][has], n[has])


@pytest.mark.parametrize('it_corr', [0, 1])
@pytest.mark.parametrize('S', CR2_S)
def test_gpu_every_width_second_contact_range(astep, S, it_corr):
    xyz, radii, p, n = case(S)
    rows, res = astep.compute_actdist(*E.genome_args(xyz), p, 1.3, it_corr, return_per_pair=True)
    same(rows, res, *oracle_case(S, 1.3, it_corr))
    # the contact range matters on this population
    assert not np.array_equal(res['pnow'], oracle_case(S, 2.0, it_corr)[1]['pnow'], equal_nan=True)


def test_gpu_ploidy_goldens(astep):
    """the reference's own output for 1x1 up to 4x4 combinations, bit for bit"""
    gp = load_golden('actdist_ploidy_golden.npz')
    pairs = make_pairs(gp['pi'], gp['pj'], gp['pwish'], gp['plast'])
    for tag in gp['cases']:
        s, cr, it = str(tag).split('_')
        rows, res = astep.compute_actdist(gp[s + '_xyz'], gp['radii'], gp['copy_ptr'], gp['copy_idx'], gp['chrom'],
                                          pairs, float(cr[2:]), int(it[1:]), return_per_pair=True)
        assert np.array_equal(res['nrows'], gp[tag + '_nrows'])
        assert np.array_equal(res['ad'], gp[tag + '_ad64'], equal_nan=True)
        has = res['nrows'] > 0
        assert np.array_equal(res['p'][has], gp[tag + '_p64'][has])
        for k in ('row', 'col'):
            assert np.array_equal(rows[k], gp[tag + '_' + k])
        for k in ('dist', 'prob'):
            assert np.array_equal(rows[k].view(np.uint32), gp[tag + '_' + k].view(np.uint32))


@pytest.mark.parametrize('npairs', [1, 63, 64, 65, 257])
def test_gpu_pair_counts(astep, npairs):
    """the last partial wave of the classification and of the selection kernels"""
    xyz, radii, p, _ = case(65)
    p = np.ascontiguousarray(p[:npairs])
    for it_corr in (0, 1):
        rows, res = astep.compute_actdist(*E.genome_args(xyz), p, 2.0, it_corr, return_per_pair=True)
        same(rows, res, *oracle.actdist(*E.genome_args(xyz), p, 2.0, it_corr))


# ---------------------------------------------------------------------------- rounding edges
@pytest.mark.parametrize('S', [8, 64, 300])
def test_gpu_threshold_traps(astep, S):
    for cr in E.TRAP_CRS:
        c = E.trap_case(cr, S)
        args = (c['xyz'], c['radii'], c['copy_ptr'], c['copy_idx'], c['chrom'], c['pairs'], cr)
        for it_corr in (0, 1):
            rows, res = astep.compute_actdist(*args, it_corr, return_per_pair=True)
            assert np.array_equal(res['pnow'], c['expect_pnow'])
            same(rows, res, *oracle.actdist(*args, it_corr))


def test_gpu_decimal_ties(astep):
    c = E.decimal_ties()
    args = (c['xyz'], c['radii'], c['copy_ptr'], c['copy_idx'], c['chrom'], c['pairs'], 2.0, 0)
    rows, res = astep.compute_actdist(*args, return_per_pair=True)
    orows, ores = oracle.actdist(*args)
    same(rows, res, orows, ores)
    has = res['nrows'] > 0
    assert np.array_equal(res['ad'][has], c['a'][has] / 32.0) and np.array_equal(res['p'], c['pairs']['pwish'])
    dist = np.array([np.float32(float('%10.4f' % x)) for x in res['ad'][has]])
    prob = np.array([np.float32(float('%.4f' % x)) for x in res['p'][has]])
    assert np.array_equal(rows['dist'].view(np.uint32), dist.view(np.uint32))
    assert np.array_equal(rows['prob'].view(np.uint32), prob.view(np.uint32))


@pytest.mark.parametrize('S', [4, 64])
def test_gpu_order_ties(astep, S):
    xyz, p, ks = E.order_ties(S)
    rows, res = astep.compute_actdist(*E.genome_args(xyz), p, 2.0, 0, return_per_pair=True)
    assert np.array_equal(res['o'], [k + (k % 2) for k in ks])
    same(rows, res, *oracle.actdist(*E.genome_args(xyz), p, 2.0, 0))


# ---------------------------------------------------------------------------- refusal
@pytest.mark.parametrize('S,ij', [(4097, (3, 7)), (7282, (2, 6)), (16385, (1, 5))])
def test_gpu_refuses_past_65536_keys(astep, ctx, S, ij):
    xyz, radii, p, _ = case(S)
    valid = np.ascontiguousarray(p[::6])
    assert E.ncomb(*ij) * S > E.MAX_KEYS
    assert max(E.ncomb(int(a), int(b)) for a, b in zip(valid['i'], valid['j'])) * S <= E.MAX_KEYS
    refused = make_pairs([ij[0]], [ij[1]], [0.5], [0.0])
    mixed = np.concatenate([valid[:70], refused, valid[70:]])
    with pytest.raises(RuntimeError) as err:
        astep.compute_actdist(*E.genome_args(xyz), mixed, 2.0, 1, ctx=ctx)
    assert 'code -5' in str(err.value) and 'too large' in str(err.value)     # IGM_E_UNSUPPORTED
    rows, res = astep.compute_actdist(*E.genome_args(xyz), valid, 2.0, 1, return_per_pair=True, ctx=ctx)
    same(rows, res, *oracle.actdist(*E.genome_args(xyz), valid, 2.0, 1, nthreads=16))


# ---------------------------------------------------------------------------- row capacity
def call_host(ctx, astep, xyz, p, cr, it_corr, cap, fill=0):
    from igm_amd._lib import result_dtype
    res = np.full(max(len(p), 1), fill, np.uint8).repeat(result_dtype.itemsize).view(result_dtype)
    rows = np.zeros(max(cap, 1), astep.row_dtype)
    nout = ctypes.c_int64(-7)
    rc = ctx.lib.igm_astep_actdist(ctx.h, 0, xyz.ctypes.data, xyz.shape[0], xyz.shape[1], E.RADII.ctypes.data,
                                   E.COPY_PTR.ctypes.data, E.COPY_IDX.ctypes.data, E.NHAP, E.CHROM.ctypes.data,
                                   p.ctypes.data if len(p) else None, len(p), float(cr), int(it_corr),
                                   res.ctypes.data, rows.ctypes.data, cap, ctypes.byref(nout))
    return rc, nout.value, rows, res[:len(p)]


def test_gpu_row_capacity(astep, ctx):
    from igm_amd import _lib
    xyz, radii, p, _ = case(65)
    orows, ores = oracle_case(65, 2.0, 1)
    total = len(orows)
    assert total == int(ores['nrows'].sum()) > 4
    rc, nout, rows, res = call_host(ctx, astep, xyz, p, 2.0, 1, total - 1, fill=0xAB)
    assert rc == _lib.IGM_E_OVERFLOW and nout == total
    assert b'exceed capacity' in ctx.lib.igm_last_error(ctx.h)
    same_per_pair(res, ores)               # per_pair is filled although no row is
    rc, nout, rows, res = call_host(ctx, astep, xyz, p, 2.0, 1, total)
    assert rc == _lib.IGM_OK and nout == total
    same(rows[:total], res, orows, ores)
    rc, nout, rows, res = call_host(ctx, astep, xyz, p[:0], 2.0, 1, 0)
    assert rc == _lib.IGM_OK and nout == 0
    # a list without a single row: every pair p <= 0
    none = make_pairs(p['i'][:70], p['j'][:70], np.zeros(70), np.zeros(70))
    rc, nout, rows, res = call_host(ctx, astep, xyz, none, 2.0, 0, 0)
    assert rc == _lib.IGM_OK and nout == 0 and np.all(res['nrows'] == 0)


# ---------------------------------------------------------------------------- device pointers
def to_dev(a):
    import torch
    a = np.array(a)
    return torch.from_numpy(a.view(np.uint8) if a.dtype.names else a).to('cuda:0')


def run_device(astep, xyz, p, cr, it_corr, pairs_t=None):
    import torch
    from igm_amd._lib import result_dtype
    pairs_t = to_dev(p) if pairs_t is None else pairs_t
    g = [to_dev(a) for a in E.genome_args(xyz)]
    rows_t, n, res_t = astep.compute_actdist(*g, pairs_t, cr, it_corr, return_per_pair=True)
    torch.cuda.synchronize()
    rows = rows_t[:n * astep.row_dtype.itemsize].cpu().numpy().view(astep.row_dtype)
    return rows, res_t.cpu().numpy().view(result_dtype), pairs_t, res_t


@pytest.mark.parametrize('heavy', [False, True], ids=['all', 'above4'])
def test_gpu_device_pointer_path(astep, heavy):
    """Inputs resident in HBM: the rows and per-pair results of the host path.  'above4' keeps the
    pairs with more than four combinations (up to 16 rows a pair), which a row buffer sized for
    diploids (four rows a pair) cannot hold."""
    xyz, radii, p, n = case(64)
    if heavy:
        p = np.ascontiguousarray(p[n > 4])
    hrows, hres = astep.compute_actdist(*E.genome_args(xyz), p, 2.0, 1, return_per_pair=True)
    if heavy:
        assert len(hrows) > 4 * len(p)
    rows, res, _, _ = run_device(astep, xyz, p, 2.0, 1)
    same(rows, res, hrows, hres)
    same(rows, res, *oracle.actdist(*E.genome_args(xyz), p, 2.0, 1))


# ---------------------------------------------------------------------------- update_plast
def update_plast_device(ctx, pairs_t, npairs, res_t):
    import torch
    from igm_amd import _lib
    ctx.set_stream(torch.cuda.current_stream(pairs_t.device).cuda_stream)
    try:
        rc = ctx.lib.igm_astep_update_plast(ctx.h, _lib.IGM_DEVICE_PTRS, _lib.ptr(pairs_t), npairs, _lib.ptr(res_t))
        ctx.check(rc, 'igm_astep_update_plast')
    finally:
        ctx.set_stream(None)
    torch.cuda.synchronize()


@pytest.mark.parametrize('S', [5, 64, 1025])
def test_gpu_update_plast(astep, ctx, S):
    """plast of the next iteration: ActivationDistanceStep.setup reads it back from the rows
    (astep.plast_from_rows); pairs without rows get exactly 0."""
    from igm_amd import _lib
    xyz, _ = E.population(S)
    p, _ = E.unique_pairs()
    rows, res = astep.compute_actdist(*E.genome_args(xyz), p, 2.0, 1, return_per_pair=True)
    same(rows, res, *oracle.actdist(*E.genome_args(xyz), p, 2.0, 1))
    want = astep.plast_from_rows(rows, E.NHAP, p['i'], p['j'])
    has = res['nrows'] > 0
    assert has.any() and (~has).any() and np.all(want[~has] == 0.0)
    assert np.array_equal(want[has], rows['prob'][np.cumsum(res['nrows'])[has] - res['nrows'][has]].astype(np.float64))
    assert np.any(want[has] != res['p'][has])                 # the text round trip is part of it
    host = p.copy()
    host['plast'] = -3.0
    rc = ctx.lib.igm_astep_update_plast(ctx.h, 0, host.ctypes.data, len(host), res.ctypes.data)
    ctx.check(rc, 'igm_astep_update_plast')
    dev_p = p.copy()
    dev_p['plast'] = -3.0
    pairs_t = to_dev(dev_p)
    update_plast_device(ctx, pairs_t, len(p), to_dev(res))
    dev = pairs_t.cpu().numpy().view(_lib.pair_dtype)
    for got in (host, dev):
        assert np.array_equal(got['plast'].view(np.uint64), want.view(np.uint64))
        for k in ('i', 'j', 'pwish'):
            assert np.array_equal(got[k], p[k])
    assert ctx.lib.igm_astep_update_plast(ctx.h, 0, None, 0, None) == _lib.IGM_OK


@pytest.mark.parametrize('S', [64, 1025])
def test_gpu_two_chained_iterations(astep, ctx, S):
    """A-step, update_plast, A-step, all on device pointers, against the oracle fed
    plast_from_rows of its own first rows"""
    xyz, _ = E.population(S)
    p, _ = E.unique_pairs()
    orows1, ores1 = oracle.actdist(*E.genome_args(xyz), p, 2.0, 1)
    p2 = p.copy()
    p2['plast'] = astep.plast_from_rows(orows1, E.NHAP, p['i'], p['j'])
    orows2, ores2 = oracle.actdist(*E.genome_args(xyz), p2, 2.0, 1)
    assert orows1.tobytes() != orows2.tobytes()
    rows1, res1, pairs_t, res_t = run_device(astep, xyz, p, 2.0, 1)
    same(rows1, res1, orows1, ores1)
    update_plast_device(ctx, pairs_t, len(p), res_t)
    rows2, res2, _, _ = run_device(astep, xyz, None, 2.0, 1, pairs_t=pairs_t)
    same(rows2, res2, orows2, ores2)


def test_gpu_am_iteration_astep_beyond_diploid():
    """AMIteration.astep (the loop bench.py measures) on the 1..4-copy genome: its row buffer
    holds up to 16 rows a pair, and its second A-step runs on the plast of the first."""
    import torch
    from igm_amd import model as M
    from igm_amd import astep as A
    from igm_amd._lib import MStepParams, bond_dtype, row_dtype
    from igm_amd.pipeline import AMIteration
    S = 64
    xyz, _ = E.population(S)
    p, n = E.unique_pairs()
    p = np.ascontiguousarray(p[n > 4])
    atoms = M.Atoms(E.RADII)
    x = np.zeros((S, atoms.n, 3), np.float32)
    x[:, :E.NBEAD] = xyz.transpose(1, 0, 2)
    chrom = np.concatenate([E.CHROM, [-1]]).astype(np.int32)
    it = AMIteration(torch.device('cuda', 0), x, atoms, chrom, E.COPY_PTR, E.COPY_IDX, p, MStepParams(),
                     np.zeros(0, bond_dtype))
    orows, _ = oracle.actdist(*E.genome_args(xyz), p, 2.0, 1)
    assert len(orows) > 4 * len(p)
    for _ in range(2):
        nrows = it.astep()
        torch.cuda.synchronize()
        rows = it.rows[:nrows * row_dtype.itemsize].cpu().numpy().view(row_dtype)
        assert rows.tobytes() == orows.tobytes()
        p = p.copy()
        p['plast'] = A.plast_from_rows(orows, E.NHAP, p['i'], p['j'])
        orows, _ = oracle.actdist(*E.genome_args(xyz), p, 2.0, 1)
