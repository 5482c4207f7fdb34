"""The DamID kernels bit for bit against the CPU restatements on the inputs of tests/damid_edges.py:
igm_damid_actdist (damid_kernel, damid_exp_kernel<false> and <true> of igm_amd/csrc/asteps.hip)
and the lamina selections igm_damid_select and igm_volume_select (igm_amd/csrc/restraints.hip).
Every comparison is an equality: integer rows, the uint32 bits of dist and prob, flags and counts.
test_damid_edges.py proves on the CPU that the inputs are the edges they claim and that the
restatements equal the reference's own output on them.

Coordinates that are NaN or inf are left out for the exp_map A-steps and igm_volume_select: the
integer conversion of the voxel is undefined for them in the reference too."""
import ctypes
import functools

import numpy as np
import pytest

import damid_edges as E
from conftest import load_golden
from igm_amd._lib import (IGM_DEVICE_PTRS, IGM_E_INVALID, IGM_E_OVERFLOW, IGM_OK, damid_row_dtype, result_dtype)
from test_restraints_gpu import select_restatement

pytestmark = pytest.mark.gpu

f32 = np.float32


@pytest.fixture(scope='module')
def damid():
    from igm_amd import damid as d
    return d


@pytest.fixture(scope='module')
def R():
    from igm_amd import restraints as r
    return r


@pytest.fixture(scope='module')
def ctx():
    from igm_amd import _lib, volume as V
    c = _lib.context(0)
    yield c
    V.stage(c, [])         # clears the maps


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_per_locus(res, ores):
    assert np.array_equal(res['o'], ores['o']) and np.array_equal(res['nrows'], ores['nrows'])
    for k in ('p', 'pnow'):
        assert np.array_equal(res[k], ores[k]), k
    assert np.array_equal(res['ad'], ores['ad'], equal_nan=True)


def same_rows(rows, orows):
    assert np.array_equal(rows['loc'], orows['loc'])
    for k in ('dist', 'prob'):
        assert np.array_equal(bits(rows[k]), bits(orows[k])), k


def check(damid, c):
    rows, res = damid.compute_damid_actdist(*E.args(c), return_per_locus=True)
    orows, ores = E.expected(c)
    same_per_locus(res, ores)
    same_rows(rows, orows)
    return rows, res


# ---------------------------------------------------------------------------- igm_damid_actdist
@pytest.mark.parametrize('shape', ['sphere', 'ellipsoid'])
@pytest.mark.parametrize('S', E.S_LIST)
def test_gpu_ploidy_and_radius(damid, S, shape):
    """1 to 4 copies with their own radii around the wave, the 256-thread stride and four strides;
    every cleanProbability branch, it_corr 2 as 0, the clamp and the tiny p"""
    for cr in (0.05, 0.0):
        for it_corr in (0, 1, 2):
            check(damid, E.ploidy_case(S, shape, cr, it_corr))


def test_gpu_reference_goldens(damid):
    """the reference's own rows for every golden case, without the oracle in between"""
    g = load_golden('damid_edges_golden.npz')
    for name, c in E.golden_cases().items():
        rows, res = damid.compute_damid_actdist(*E.args(c), return_per_locus=True)
        assert np.array_equal(rows['loc'], g[name + '_loc']), name
        assert np.array_equal(bits(rows['dist']), bits(g[name + '_dist'])), name
        assert np.array_equal(bits(rows['prob']), bits(g[name + '_prob'])), name
        assert np.array_equal(res['p'], g[name + '_p64']), name
        has = res['o'] >= 0
        assert np.array_equal(res['ad'][has], g[name + '_ad64'][has], equal_nan=True), name


@pytest.mark.parametrize('S', E.S_LIST)
def test_gpu_radix_ties_and_buckets(damid, S):
    rows, res = check(damid, E.radix_case(S))
    t = np.array([E.T_KEY], np.uint32).view(f32)[0]
    assert np.all(res['ad'] == np.sqrt(np.float64(t)))


@pytest.mark.parametrize('it_corr', [0, 1, 2])
def test_gpu_special_keys_and_count_threshold(damid, it_corr):
    rows, res = check(damid, E.special_case(it_corr))
    assert np.array_equal(bits(rows['dist'][:3]), bits([np.nan, np.nan, np.inf]))
    assert np.all(res['pnow'][:9] == 3 / 8) and np.all(res['pnow'][9:] == 5 / 8)


def test_gpu_order_index_half_to_even(damid):
    for S in (4, 5):
        check(damid, E.order_case(S))


def test_gpu_decimal_ties(damid):
    c = E.decimal_case()
    rows, res = check(damid, c)
    odd = (2 * c['loci'] + 1) / 64.0
    assert np.array_equal(res['ad'], odd) and np.array_equal(res['p'], odd)


@pytest.mark.parametrize('cr', [0.05, 0.0])
def test_gpu_ellipsoid_one_axis_at_a_time(damid, cr):
    for it_corr in (0, 1):
        check(damid, E.axes_case(cr, it_corr))


@pytest.mark.parametrize('n', [1, 255, 256, 257])
def test_gpu_locus_counts(damid, n):
    check(damid, E.nloci_case(n))


def test_gpu_locus_without_copies(damid):
    """tested against the library contract: the reference would raise on an empty copy list"""
    c = E.zero_copy_case()
    rows, res = damid.compute_damid_actdist(*E.args(c), return_per_locus=True)
    keep = c['loci'] != 4
    full = dict(c, loci=c['loci'][keep], p_exp=c['p_exp'][keep], plast=c['plast'][keep])
    orows, ores = E.expected(full)
    same_rows(rows, orows)                       # the offsets after the empty locus are right
    same_per_locus(res[keep], ores)
    assert np.all(res['nrows'][~keep] == 0) and np.all(res['o'][~keep] == -1)
    assert res['nrows'].tolist() == [2, 0, 4, 0, 1]
    only = dict(c, loci=c['loci'][~keep], p_exp=c['p_exp'][~keep], plast=c['plast'][~keep])
    rows, res = damid.compute_damid_actdist(*E.args(only), return_per_locus=True)
    assert len(rows) == 0 and np.all(res['nrows'] == 0) and np.all(res['o'] == -1)


def call_actdist(ctx, c, cap, flags=0, dev=None, per_locus=True, fill=0):
    """igm_damid_actdist itself; dev: the arrays already on the device (to_dev)"""
    from igm_amd import damid as D
    par = D._nucleus_param(c['shape'], c['param'])
    n = len(c['loci'])
    a = dev or [c[k] for k in ('xyz', 'radii', 'copy_ptr', 'copy_idx', 'loci', 'p_exp', 'plast')]
    p = [x.data_ptr() if dev else x.ctypes.data for x in a]
    res = np.full(max(n, 1) * result_dtype.itemsize, fill, np.uint8).view(result_dtype)
    rows = np.zeros(max(cap, 1), damid_row_dtype)
    nout = ctypes.c_int64(-7)
    out = [res, rows]
    if dev:
        out = [to_dev(res), to_dev(rows)]
    rc = ctx.lib.igm_damid_actdist(ctx.h, flags, p[0], c['xyz'].shape[0], c['xyz'].shape[1], p[1], p[2], p[3],
                                   len(c['copy_ptr']) - 1, p[4], p[5], p[6], n, c['it_corr'], c['cr'],
                                   D.SHAPES[c['shape']], par.ctypes.data,
                                   (out[0].data_ptr() if dev else res.ctypes.data) if per_locus else None,
                                   out[1].data_ptr() if dev else rows.ctypes.data, cap, ctypes.byref(nout))
    if dev:
        res = out[0].cpu().numpy().view(result_dtype)
        rows = out[1].cpu().numpy().view(damid_row_dtype)
    return rc, nout.value, rows, res[:n]


def test_gpu_row_capacity(ctx):
    c = E.ploidy_case(65, 'sphere', 0.05, 1)
    orows, ores = E.expected(c)
    total = len(orows)
    assert total == int(ores['nrows'].sum()) > 4
    rc, nout, rows, res = call_actdist(ctx, c, total - 1)
    assert rc == IGM_E_OVERFLOW and nout == total
    assert b'exceed capacity' in ctx.lib.igm_last_error(ctx.h)
    rc, nout, rows, res = call_actdist(ctx, c, total, fill=0xAB)    # the context is usable afterwards
    assert rc == IGM_OK and nout == total
    same_per_locus(res, ores)
    same_rows(rows[:total], orows)


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to('cuda:0')


@pytest.mark.parametrize('per_locus', [True, False], ids=['per_locus', 'null'])
def test_gpu_device_pointers(ctx, per_locus):
    import torch
    c = E.ploidy_case(257, 'ellipsoid', 0.05, 1)
    orows, ores = E.expected(c)
    dev = [to_dev(c[k]) for k in ('xyz', 'radii', 'copy_ptr', 'copy_idx', 'loci', 'p_exp', 'plast')]
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        rc, nout, rows, res = call_actdist(ctx, c, len(orows), IGM_DEVICE_PTRS, dev, per_locus, fill=0xAB)
    finally:
        ctx.set_stream(None)
    torch.cuda.synchronize()
    assert rc == IGM_OK and nout == len(orows)
    same_rows(rows[:nout], orows)
    if per_locus:
        same_per_locus(res, ores)
    else:
        assert np.all(res.view(np.uint8) == 0xAB)      # untouched


def test_gpu_refuses_loci_outside_the_genome(damid, ctx):
    c = E.ploidy_case(5, 'sphere', 0.05, 1)
    for bad in (-1, E.NHAP):
        loci = c['loci'].copy()
        loci[70] = bad
        rc, nout, rows, res = call_actdist(ctx, dict(c, loci=loci), 1000)
        assert rc == IGM_E_INVALID and b'locus index outside' in ctx.lib.igm_last_error(ctx.h)
    check(damid, c)


# ---------------------------------------------------------------------------- igm_damid_select
def select_want(xyz, radii, rows, abc, cr, bit, base):
    return E.select_expected(select_restatement, xyz, radii, rows, abc, cr, bit, base)


def test_gpu_select_threshold_traps(R):
    xyz, radii, rows, want = E.select_traps()
    g = load_golden('damid_edges_golden.npz')
    for env in (0, 1, 3):
        bit = E.env_bit(env)
        base = E.base_pattern(len(radii), bit)
        base[:] &= ~np.uint32(bit)
        flags, nsel = R.damid_envelope_flags(xyz, radii, rows, E.SEL_ABC, 0.0, env, base)
        assert np.array_equal((flags & np.uint32(bit)) != 0, g['select_sel'])      # a bead a row: the reference
        assert np.array_equal(flags & ~np.uint32(bit), np.repeat(base[None], len(xyz), 0))
        assert np.array_equal(nsel, g['select_sel'].sum(1))
        wflags, wn = select_want(xyz, radii, rows, E.SEL_ABC, 0.0, bit, base)
        assert np.array_equal(flags, wflags) and np.array_equal(nsel, wn)
    assert np.array_equal(g['select_sel'][0], want)


def test_gpu_select_rows_naming_one_bead(R):
    """n_selected counts rows, the flag is set once"""
    xyz, radii, rows, want = E.select_traps()
    for k in (2, 3):
        r = rows[:k].copy()
        r['loc'] = 0                       # d, the f32 above, the f32 below, all of bead 0
        flags, nsel = R.damid_envelope_flags(xyz, radii, r, E.SEL_ABC, 0.0, 1, np.zeros(len(radii), np.uint32))
        assert nsel.tolist() == [k - 1, k, 0]
        assert flags[:, 0].tolist() == [0x20, 0x20, 0] and not flags[:, 1:].any()


@pytest.mark.parametrize('mode', E.HIT_MODES)
@pytest.mark.parametrize('n', E.ROW_COUNTS)
def test_gpu_select_row_edges(R, n, mode):
    S, natom = 3, 257
    xyz, radii = E.select_population(S, natom), np.full(natom, 0.5, f32)
    bit = E.env_bit(3)
    base = E.base_pattern(natom, bit)
    rows = E.select_rows(n, natom, mode)
    flags, nsel = R.damid_envelope_flags(xyz, radii, rows, E.SEL_ABC, 0.0, 3, base)
    wflags, wn = select_want(xyz, radii, rows, E.SEL_ABC, 0.0, bit, base)
    assert np.array_equal(flags, wflags) and np.array_equal(nsel, wn)
    assert n == 0 or wn.sum() > 0
    junk = E.with_junk(rows, natom)          # loc = -1 and loc = natom change nothing
    flags, nsel = R.damid_envelope_flags(xyz, radii, junk, E.SEL_ABC, 0.0, 3, base)
    assert np.array_equal(flags, wflags) and np.array_equal(nsel, wn)


@pytest.mark.parametrize('S,natom', [(1, 257), (3, 255), (70, 1), (70, 257)])
def test_gpu_select_shapes_and_bits(R, S, natom):
    xyz, radii = E.select_population(S, natom), np.linspace(0.25, 0.75, natom).astype(f32)
    rows = E.select_rows(65, natom, 'two_thirds')
    for env, cr in ((0, 0.05), (1, 0.0), (3, 0.05)):
        bit = E.env_bit(env)
        base = E.base_pattern(natom, bit)
        flags, nsel = R.damid_envelope_flags(xyz, radii, rows, E.SEL_ABC, cr, env, base)
        wflags, wn = select_want(xyz, radii, rows, E.SEL_ABC, cr, bit, base)
        assert np.array_equal(flags, wflags) and np.array_equal(nsel, wn)
        assert np.array_equal(flags & ~np.uint32(bit), np.repeat((base & ~np.uint32(bit))[None], S, 0))


def call_select(ctx, xyz, radii, rows, abc, cr, bit, base, nsel=True, device=False):
    """igm_damid_select itself: n_selected NULL, device pointers"""
    import torch
    S, N = xyz.shape[0], xyz.shape[1]
    abc = np.array(abc, np.float64)
    out = np.zeros((S, N), np.uint32)
    ns = np.full(S, -7, np.int32)
    a = [np.ascontiguousarray(xyz, f32), radii, rows, base, out, ns]
    if device:
        a = [to_dev(x) for x in a]
        p = [x.data_ptr() for x in a]
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    else:
        p = [x.ctypes.data for x in a]
    try:
        rc = ctx.lib.igm_damid_select(ctx.h, IGM_DEVICE_PTRS if device else 0, S, N, p[0], p[1], p[2], len(rows),
                                      abc.ctypes.data, cr, bit, p[3], p[4], p[5] if nsel else None)
    finally:
        if device:
            ctx.set_stream(None)
    assert rc == IGM_OK
    if device:
        torch.cuda.synchronize()
        out = a[4].cpu().numpy().view(np.uint32).reshape(S, N)
        ns = a[5].cpu().numpy().view(np.int32)
    return out, ns


@pytest.mark.parametrize('device', [False, True], ids=['host', 'device'])
def test_gpu_select_null_count_and_device_pointers(ctx, device):
    S, natom = 3, 255
    xyz, radii = E.select_population(S, natom), np.full(natom, 0.5, f32)
    rows = E.with_junk(E.select_rows(257, natom, 'two_thirds'), natom)
    bit = E.env_bit(2)
    base = E.base_pattern(natom, bit)
    wflags, wn = select_want(xyz, radii, rows, E.SEL_ABC, 0.0, bit, base)
    out, ns = call_select(ctx, xyz, radii, rows, E.SEL_ABC, 0.0, bit, base, True, device)
    assert np.array_equal(out, wflags) and np.array_equal(ns, wn)
    out, ns = call_select(ctx, xyz, radii, rows, E.SEL_ABC, 0.0, bit, base, False, device)
    assert np.array_equal(out, wflags) and np.all(ns == -7)


# ---------------------------------------------------------------------------- exp_map A-steps
@functools.lru_cache(maxsize=None)
def exp_want(S, kind, nucl, cr, it_corr):
    return E.exp_expected(S, kind, nucl, cr, it_corr)


@pytest.mark.parametrize('nucl', [False, True], ids=['exp_map', 'exp_map_nucl'])
@pytest.mark.parametrize('kind', ['centre', 'off'])
@pytest.mark.parametrize('S', E.EXP_S)
def test_gpu_exp_map_forms(damid, ctx, S, kind, nucl):
    """voxel rounding on half-steps and faces, a map per structure, ties at every byte of the
    8-pass select, the count threshold on keys equal to the contact range"""
    loci, pe, pl = E.exp_listing()
    for cr, it_corr in ((E.EXP_CR[0], 1), (E.EXP_CR[1], 1), (E.EXP_CR[0], 0)):
        rows = damid.compute_damid_actdist(E.exp_population(S, kind), E.RADII, E.COPY_PTR, E.COPY_IDX, loci, pe, pl,
                                           it_corr, cr, 'exp_map_nucl' if nucl else 'exp_map', ctx=ctx,
                                           volumes=list(E.maps()), struct_map=E.struct_map(S))
        same_rows(rows, exp_want(S, kind, nucl, cr, it_corr))


# ---------------------------------------------------------------------------- igm_volume_select
def stage(ctx, smap=None):
    from igm_amd import volume as V
    V.stage(ctx, list(E.maps()), smap)


def test_gpu_volume_threshold_traps(R, ctx):
    xyz, T = E.volume_traps()
    stage(ctx)
    base = np.zeros(T.shape[1], np.uint32)
    for s in range(3):
        rows = E.volume_trap_rows(T[s])
        flags, nsel = R.volume_envelope_flags(xyz[s:s + 1], rows, [s], 2, base, ctx=ctx)
        wflags, wn = E.volume_expected(xyz[s:s + 1], rows, [s], E.env_bit(2), base)
        assert np.array_equal(flags, wflags) and np.array_equal(nsel, wn) and nsel[0] == T.shape[1]
        exact = rows[0::3]                    # v == d^2 alone: not selected
        flags, nsel = R.volume_envelope_flags(xyz[s:s + 1], exact, [s], 2, base, ctx=ctx)
        assert not flags.any() and nsel[0] == 0
    # all three structures at once on the rows of structure 0
    rows = E.volume_trap_rows(T[0])
    flags, nsel = R.volume_envelope_flags(xyz, rows, [0, 1, 2], 2, base, ctx=ctx)
    wflags, wn = E.volume_expected(xyz, rows, [0, 1, 2], E.env_bit(2), base)
    assert np.array_equal(flags, wflags) and np.array_equal(nsel, wn)


def volume_rows(n, natom, mode, S):
    """select_rows with dist = 1 replaced by a distance that some beads are within and some not"""
    r = E.select_rows(n, natom, mode)
    r['dist'] = np.where(r['dist'] == 1.0, f32(1.5), f32(0.0))      # v < 0 never holds
    return r


@pytest.mark.parametrize('mode', E.HIT_MODES)
@pytest.mark.parametrize('n', E.ROW_COUNTS)
def test_gpu_volume_row_edges(R, ctx, n, mode):
    S = 5
    x = np.ascontiguousarray(E.exp_population(S, 'off').transpose(1, 0, 2))      # (S, 12, 3)
    smap = E.struct_map(S)
    stage(ctx, smap)
    rows = volume_rows(n, E.NBEAD, mode, S)       # 12 beads: many rows name the same bead
    bit = E.env_bit(1)
    base = E.base_pattern(E.NBEAD, bit)
    wflags, wn = E.volume_expected(x, rows, smap, bit, base)
    assert n == 0 or wn.sum() > 0
    for given in (smap, None):                    # struct_map given, and NULL with the staged one
        flags, nsel = R.volume_envelope_flags(x, rows, given, 1, base, ctx=ctx)
        assert np.array_equal(flags, wflags) and np.array_equal(nsel, wn)
    junk = E.with_junk(rows, E.NBEAD)
    junk['dist'][(junk['loc'] < 0) | (junk['loc'] >= E.NBEAD)] = 1e30           # would select any bead
    flags, nsel = R.volume_envelope_flags(x, junk, None, 1, base, ctx=ctx)
    assert np.array_equal(flags, wflags) and np.array_equal(nsel, wn)


def call_volume_select(ctx, x, rows, smap, bit, base, nsel=True, device=False):
    """igm_volume_select itself: the return code, n_selected NULL, device pointers"""
    import torch
    S, N = x.shape[0], x.shape[1]
    out = np.zeros((S, N), np.uint32)
    ns = np.full(S, -7, np.int32)
    a = [np.ascontiguousarray(x, f32), rows, np.zeros(1, np.int32) if smap is None else np.array(smap, np.int32),
         np.ascontiguousarray(base, np.uint32), out, ns]
    if device:
        a = [to_dev(v) for v in a]
        p = [v.data_ptr() for v in a]
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    else:
        p = [v.ctypes.data for v in a]
    try:
        rc = ctx.lib.igm_volume_select(ctx.h, IGM_DEVICE_PTRS if device else 0, S, N, p[0], p[1], len(rows),
                                       None if smap is None else p[2], bit, p[3], int(np.ndim(base) == 2), p[4],
                                       p[5] if nsel else None)
    finally:
        if device:
            ctx.set_stream(None)
    if device:
        torch.cuda.synchronize()
        out = a[4].cpu().numpy().view(np.uint32).reshape(S, N)
        ns = a[5].cpu().numpy().view(np.int32)
    return rc, out, ns


@pytest.mark.parametrize('S', [1, 3, 70])
def test_gpu_volume_select_maps_and_base(R, ctx, S):
    x = np.ascontiguousarray(E.exp_population(max(S, 64), 'off').transpose(1, 0, 2))[:S]
    smap = E.struct_map(S)
    rows = volume_rows(65, E.NBEAD, 'two_thirds', S)
    bit = E.env_bit(3)
    base = E.base_pattern(E.NBEAD, bit)
    # nothing staged per structure: map 0 for everyone
    stage(ctx, None)
    flags, nsel = R.volume_envelope_flags(x, rows, None, 3, base, ctx=ctx)
    w0, n0 = E.volume_expected(x, rows, np.zeros(S, np.int32), bit, base)
    assert np.array_equal(flags, w0) and np.array_equal(nsel, n0)
    flags, nsel = R.volume_envelope_flags(x, rows, smap, 3, base, ctx=ctx)
    wflags, wn = E.volume_expected(x, rows, smap, bit, base)
    assert np.array_equal(flags, wflags) and np.array_equal(nsel, wn)
    assert S == 1 or not np.array_equal(wflags, w0)                 # the map of a structure matters
    # base_per_struct 1: the result of an earlier selection
    base2 = wflags | np.uint32(E.env_bit(0)) * (np.arange(S * E.NBEAD).reshape(S, E.NBEAD) % 3 == 0).astype(np.uint32)
    flags, nsel = R.volume_envelope_flags(x, rows, smap, 2, base2, ctx=ctx)
    w2, n2 = E.volume_expected(x, rows, smap, E.env_bit(2), base2)
    assert np.array_equal(flags, w2) and np.array_equal(nsel, n2)
    # a map index equal to nmap, and -1: refused, and the context is usable afterwards
    for bad in (3, -1):
        wrong = smap.copy()
        wrong[S // 2] = bad
        rc, _, _ = call_volume_select(ctx, x, rows, wrong, bit, base)
        assert rc == IGM_E_INVALID and b'map index outside' in ctx.lib.igm_last_error(ctx.h)
    for device in (False, True):
        rc, out, ns = call_volume_select(ctx, x, rows, smap, bit, base, True, device)
        assert rc == IGM_OK and np.array_equal(out, wflags) and np.array_equal(ns, wn)
        rc, out, ns = call_volume_select(ctx, x, rows, smap, bit, base, False, device)
        assert rc == IGM_OK and np.array_equal(out, wflags) and np.all(ns == -7)
