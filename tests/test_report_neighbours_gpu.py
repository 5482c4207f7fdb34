"""The neighbour census kernel (igm_report_neighbours) and the report steps on it, on the
MI355X, against the NumPy oracle tests/report_neighbours_ref.py.

Everything the census returns is an exact integer or, icp_sum, a float64 sum with a fixed
order that the oracle restates: every comparison is an equality.  Every call is made twice
and must return the same bytes; the outputs start from a fill that no result equals, so
an entry that was never written shows.  Only local_compaction carries a bar, the one of
tests/test_report_gpu.py for Rg: 2 (3 n) 2^-53 relative plus n 2^-52 max|x| absolute for a
window of n beads.

Shapes: the kernel owns 32 beads per workgroup and 8 per wave, streams partners in tiles
of 32 (two at a time in the unrolled loop) and structures in chunks of 64; the bead and
structure counts below sit on both sides of each of those."""
import itertools

import numpy as np
import pytest

import asteps_edges as E
import report_neighbours_ref as N
from conftest import load_golden
from igm_amd import _lib, report as RP

pytestmark = pytest.mark.gpu

f32 = np.float32
OUTS = ('census', 'sums', 'icp_sum', 'icp_n')
FILL = {'census': -7, 'sums': -7, 'icp_sum': -7.0, 'icp_n': -7}
DTYPE = {'census': np.int32, 'sums': np.int64, 'icp_sum': np.float64, 'icp_n': np.int32}


@pytest.fixture(scope='module')
def ctx():
    return _lib.context(0)


def call(ctx, xyz, chain, cls=None, nclass=0, min_sep=1, cutoff=500.0, radii=None, contact_range=0.0, outs=OUTS):
    """igm_report_neighbours on host arrays, twice: (rc, {name: array or None})"""
    xyz = np.ascontiguousarray(xyz, f32)
    n, S = xyz.shape[:2]
    chain = np.ascontiguousarray(chain, np.int32)
    cls = None if cls is None else np.ascontiguousarray(cls, np.int32)
    radii = None if radii is None else np.ascontiguousarray(radii, f32)
    shape = {'census': (n, S, nclass + 2), 'sums': (n, nclass + 2), 'icp_sum': (n,), 'icp_n': (n,)}
    runs = []
    for _ in range(2):
        o = {k: np.full(shape[k], FILL[k], DTYPE[k]) if k in outs else None for k in OUTS}
        rc = ctx.lib.igm_report_neighbours(ctx.h, 0, xyz.ctypes.data, n, S, chain.ctypes.data, _lib.ptr(cls), nclass,
                                           min_sep, cutoff, _lib.ptr(radii), contact_range,
                                           *(_lib.ptr(o[k]) for k in OUTS))
        runs.append((rc, o))
    assert runs[0][0] == runs[1][0]
    for k in OUTS:
        a, b = runs[0][1][k], runs[1][1][k]
        assert (a is None and b is None) or a.tobytes() == b.tobytes(), 'rerun differs in %s' % k
    return runs[0]


def check(ctx, xyz, chain, cls=None, nclass=0, min_sep=1, cutoff=500.0, radii=None, contact_range=0.0):
    """all four outputs equal the oracle's; returns them"""
    rc, got = call(ctx, xyz, chain, cls, nclass, min_sep, cutoff, radii, contact_range)
    assert rc == 0, ctx.lib.igm_last_error(ctx.h).decode()
    want = N.results(xyz, chain, cls, nclass, min_sep, cutoff, radii, contact_range if radii is not None else None)
    for k in OUTS:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
    assert np.array_equal(got['sums'], got['census'].sum(axis=1, dtype=np.int64))
    return got


def population(n, S, seed, scale=600.0):
    """positions on the scale of the default cutoff, so that hits and misses both occur"""
    rng = np.random.default_rng(seed)
    xyz = (rng.standard_normal((n, S, 3)) * scale).astype(f32)
    chain = rng.integers(0, 4, n).astype(np.int32)       # four chains scattered over the index
    cls = rng.integers(-1, 2, n).astype(np.int32)        # two classes and unlabelled beads
    return xyz, chain, cls


# ------------------------------------------------------------------ shapes
NBEAD = (1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 129, 257)
NSTRUCT = (1, 2, 63, 64, 65, 130)


@pytest.mark.parametrize('n,S', list(itertools.product(NBEAD, NSTRUCT)))
def test_shapes(ctx, n, S):
    xyz, chain, cls = population(n, S, 1000 * n + S)
    got = check(ctx, xyz, chain, cls, 2, min_sep=2)
    if n >= 31:
        assert got['census'][..., 0].any() and got['census'][..., 1:].any()


def test_many_partner_tiles(ctx):
    """1025 beads: 33 workgroups of beads, and class segments of several partner tiles each"""
    xyz, chain, cls = population(1025, 3, 5, scale=1500.0)
    got = check(ctx, xyz, chain, cls, 2, min_sep=3)
    assert got['sums'].min(axis=0).tolist() != got['sums'].max(axis=0).tolist()
    assert ctx.kernel_ms('report_neighbours') > 0


# ------------------------------------------------------------------ the distance test at its edges
@pytest.mark.parametrize('cr,offaxis', list(itertools.product(E.TIE_CRS, (False, True))))
def test_near_ties_radii_form(ctx, cr, offaxis):
    """every pair within +-2 ulp of its radii bound (twelve distinct radii)"""
    xyz, radii = E.near_tie_case(cr, offaxis)
    got = check(ctx, xyz, np.arange(12) % 2, radii=radii, contact_range=cr)
    if not offaxis:  # on an axis the norm is exact: a neighbour iff the distance is not above the bound
        for p, (i, j) in enumerate(E.TIE_PAIRS):
            hits = got['census'][i, 5 * p:5 * p + 5].sum(axis=1)
            assert hits.tolist() == [1, 1, 1, 0, 0], (i, j)


@pytest.mark.parametrize('cutoff', [500.0, 0.1, 3.0, 2.0 ** -60, 1e15])
def test_near_ties_cutoff_form(ctx, cutoff):
    """a pair at the cutoff moved by -2 .. 2 ulp, on the axes and along the oblique directions"""
    cut = f32(cutoff)
    dirs = [np.eye(3)[a] * sgn for a in range(3) for sgn in (1.0, -1.0)] + list(E.TIE_DIRS)
    xyz = np.zeros((2, len(dirs) * len(E.TIE_K), 3), f32)
    for q, d in enumerate(dirs):
        for k in E.TIE_K:
            xyz[1, len(E.TIE_K) * q + k + 2] = (np.float64(E.ulps(cut, k)) * d).astype(f32)
    got = check(ctx, xyz, [0, 1], cutoff=float(cut))
    assert got['census'][0, :30, 1].tolist() == [1, 1, 1, 0, 0] * 6  # the six axis directions are exact


def test_cutoff_zero(ctx):
    """only coincident beads are neighbours: lattice beads that coincide in some structures"""
    xyz, _ = E.zero_threshold_case()
    got = check(ctx, xyz, np.arange(12) // 4, cutoff=0.0)
    assert 0 < got['census'].sum() < 12 * 11 * 24
    got = check(ctx, xyz, np.arange(12) // 4, radii=E.TIE_RADII, contact_range=0.0)
    assert got['census'].sum() > 0
    distinct = np.arange(36, dtype=f32).reshape(12, 1, 3)
    assert not check(ctx, distinct, np.zeros(12), cutoff=0.0)['census'].any()


@pytest.mark.parametrize('kind', ['overflow', 'big_threshold', 'nonfinite', 'tiny_radii'])
def test_ends_of_float32(ctx, kind):
    """squared norms that overflow or vanish, bounds whose square does, NaN and +-inf coordinates"""
    xyz, radii, cr = E.extreme_case(kind)
    chain = np.arange(10) % 3
    check(ctx, xyz, chain, radii=radii, contact_range=cr)
    for cutoff in (0.0, 1e-30, 100.0, 4e20, float(np.finfo(f32).max)):
        got = check(ctx, xyz, chain, cutoff=cutoff)
    if kind == 'nonfinite':  # bead 5 has a NaN in every fourth structure: nobody's neighbour there
        s = np.arange(40) % 4 == 0
        assert not got['census'][5, s].any() and got['census'][5, ~s].any()


# ------------------------------------------------------------------ classes and chains
@pytest.mark.parametrize('nclass', [0, 1, 2, 8])
def test_classes(ctx, nclass):
    xyz, chain, _ = population(70, 5, 77 + nclass)
    rng = np.random.default_rng(nclass)
    if nclass == 0:
        check(ctx, xyz, chain)                                  # cls NULL
        check(ctx, xyz, chain, np.full(70, -1), 0)               # cls given, all unlabelled
        return
    check(ctx, xyz, chain, np.full(70, -1), nclass)              # all beads unlabelled
    dealt = rng.integers(-1, nclass, 70)
    got = check(ctx, xyz, chain, dealt, nclass)                  # labels dealt at random
    assert got['census'][..., 1:1 + nclass].any()
    absent = np.where(dealt == nclass - 1, -1, dealt)            # the last class has no bead
    got = check(ctx, xyz, chain, absent, nclass)
    assert not got['census'][..., nclass].any()
    first = np.where(dealt == 0, -1, dealt)                      # the first class has none
    assert not check(ctx, xyz, chain, first, nclass)['census'][..., 1].any()
    check(ctx, xyz, chain, np.zeros(70), nclass)                 # everybody in class 0


def test_chains(ctx):
    xyz, _, cls = population(67, 4, 21)
    idx = np.arange(67)
    for chain in (idx, idx % 3, idx // 10, np.zeros(67), -idx * 1000 + 5):
        for min_sep in (1, 2, 3, 10, 23, 66, 67, 1000):
            check(ctx, xyz, chain, cls, 2, min_sep=min_sep)
    alone = check(ctx, xyz, idx, min_sep=5)                      # chains of length 1: nothing is cis
    assert not alone['census'][..., 0].any() and np.all(alone['icp_sum'] == alone['icp_n'])


# ------------------------------------------------------------------ the radii form
def radii_case(ndistinct, n=90, S=9, seed=0):
    rng = np.random.default_rng(100 + ndistinct + seed)
    vals = (10.0 ** rng.uniform(1.5, 2.5, ndistinct)).astype(f32)
    radii = vals[rng.permutation(np.arange(n) % ndistinct)]
    xyz = (rng.standard_normal((n, S, 3)) * 250.0).astype(f32)
    return xyz, radii


@pytest.mark.parametrize('ndistinct', [1, 2, 16])
def test_radii_form(ctx, ndistinct):
    xyz, radii = radii_case(ndistinct)
    chain = np.arange(90) % 5
    got = check(ctx, xyz, chain, np.arange(90) % 3 - 1, 2, min_sep=6, cutoff=-1.0, radii=radii, contact_range=1.3)
    assert got['census'].any() and len(np.unique(radii)) == ndistinct
    check(ctx, xyz, chain, radii=radii, contact_range=0.7, cutoff=float('nan'))  # cutoff is ignored


def test_seventeen_radii_are_refused(ctx):
    xyz, radii = radii_case(17)
    rc, got = call(ctx, xyz, np.zeros(90), radii=radii, contact_range=1.0)
    assert rc == _lib.IGM_E_UNSUPPORTED and 'radii' in ctx.lib.igm_last_error(ctx.h).decode()
    for k in OUTS:
        assert np.all(got[k] == FILL[k])
    xyz, radii = radii_case(16)
    check(ctx, xyz, np.zeros(90), radii=radii, contact_range=1.0)  # the context stays usable


@pytest.mark.parametrize('n,S', [(65, 33), (129, 7)])
def test_identity_with_the_contact_map(ctx, n, S):
    """min_sep = 1: for every bead the census summed over structures and columns is the
    row of igm_contact_map's counts on the same input without its diagonal"""
    xyz, radii = radii_case(16, n, S, seed=n)
    cr = 1.1
    rc, got = call(ctx, xyz, np.arange(n) % 4, np.arange(n) % 3 - 1, 2, radii=radii, contact_range=cr)
    assert rc == 0
    counts = np.full((n, n), -7, np.int32)
    ctx.check(ctx.lib.igm_contact_map(ctx.h, 0, xyz.ctypes.data, n, S, radii.ctypes.data, cr, counts.ctypes.data),
              'igm_contact_map')
    np.fill_diagonal(counts, 0)
    assert counts.sum() > 0
    assert np.array_equal(got['sums'].sum(axis=1), counts.sum(axis=1, dtype=np.int64))


# ------------------------------------------------------------------ the outputs and the refusals
def test_every_null_combination(ctx):
    xyz, chain, cls = population(70, 66, 8)
    _, full = call(ctx, xyz, chain, cls, 2, min_sep=2)
    for r in range(1, 4):
        for outs in itertools.combinations(OUTS, r):
            rc, got = call(ctx, xyz, chain, cls, 2, min_sep=2, outs=outs)
            assert rc == 0, outs
            for k in OUTS:
                assert (got[k] is None) if k not in outs else got[k].tobytes() == full[k].tobytes(), (outs, k)


def test_refusals_leave_the_outputs_and_the_context(ctx):
    xyz, chain, cls = population(20, 3, 9)
    inv = _lib.IGM_E_INVALID
    bad = [dict(outs=()),                                          # all four outputs NULL
           dict(nclass=9, cls=cls), dict(nclass=-1), dict(nclass=2),   # nclass outside [0, 8]; classes without cls
           dict(nclass=2, cls=np.where(np.arange(20) == 7, 2, cls)),   # a label outside [-1, nclass)
           dict(nclass=2, cls=np.where(np.arange(20) == 19, -2, cls)),
           dict(min_sep=0), dict(min_sep=-4),
           dict(cutoff=-1.0), dict(cutoff=float('nan')), dict(cutoff=float('inf')),
           dict(radii=np.ones(20), contact_range=-0.5), dict(radii=np.ones(20), contact_range=float('nan')),
           dict(radii=np.ones(20), contact_range=float('inf'))]
    for kw in bad:
        rc, got = call(ctx, xyz, chain, **kw)
        assert rc == inv and ctx.lib.igm_last_error(ctx.h).decode().startswith('igm_report_neighbours'), kw
        for k in OUTS:
            assert got[k] is None or np.all(got[k] == FILL[k]), kw
        check(ctx, xyz, chain, cls, 2)                             # usable after every refusal
    sums = np.full((20, 2), -7, np.int64)
    args = (20, 3, chain.ctypes.data, None, 0, 1, 500.0, None, 0.0, None, sums.ctypes.data, None, None)
    assert ctx.lib.igm_report_neighbours(ctx.h, 0, None, *args) == inv                            # xyz NULL
    assert ctx.lib.igm_report_neighbours(ctx.h, 0, xyz.ctypes.data, 20, 3, None, *args[3:]) == inv   # chain NULL
    assert ctx.lib.igm_report_neighbours(ctx.h, 0, xyz.ctypes.data, 0, 3, *args[2:]) == inv
    assert ctx.lib.igm_report_neighbours(ctx.h, 0, xyz.ctypes.data, 20, 0, *args[2:]) == inv
    assert np.all(sums == -7)
    big = np.zeros((65536, 1, 3), f32)
    rc, got = call(ctx, big, np.zeros(65536), outs=('icp_n',))
    assert rc == _lib.IGM_E_UNSUPPORTED and np.all(got['icp_n'] == -7)
    check(ctx, xyz, chain, cls, 2)


def test_device_pointers(ctx):
    """IGM_DEVICE_PTRS: xyz and census are device memory, everything else stays on the host"""
    import torch
    xyz, chain, cls = population(70, 66, 10)
    _, host = call(ctx, xyz, chain, cls, 2, min_sep=2)
    dx = torch.from_numpy(xyz).cuda()
    F = _lib.IGM_DEVICE_PTRS
    for with_census in (True, False):
        for _ in range(2):
            cen = torch.full((70, 66, 4), -7, dtype=torch.int32, device='cuda') if with_census else None
            sums, isum, icn = np.full((70, 4), -7, np.int64), np.full(70, -7.0), np.full(70, -7, np.int32)
            rc = ctx.lib.igm_report_neighbours(ctx.h, F, dx.data_ptr(), 70, 66, chain.ctypes.data, cls.ctypes.data, 2,
                                               2, 500.0, None, 0.0, None if cen is None else cen.data_ptr(),
                                               sums.ctypes.data, isum.ctypes.data, icn.ctypes.data)
            ctx.check(rc, 'igm_report_neighbours')
            if with_census:
                assert cen.cpu().numpy().tobytes() == host['census'].tobytes()
            for got, k in ((sums, 'sums'), (isum, 'icp_sum'), (icn, 'icp_n')):
                assert got.tobytes() == host[k].tobytes(), k
    cen = torch.full((70, 66, 4), -7, dtype=torch.int32, device='cuda')   # the census alone
    ctx.check(ctx.lib.igm_report_neighbours(ctx.h, F, dx.data_ptr(), 70, 66, chain.ctypes.data, cls.ctypes.data, 2, 2,
                                            500.0, None, 0.0, cen.data_ptr(), None, None, None),
              'igm_report_neighbours')
    assert cen.cpu().numpy().tobytes() == host['census'].tobytes()


# ------------------------------------------------------------------ the Python layer and the report steps
def test_python_functions(ctx):
    xyz, _, _ = population(60, 5, 12)
    chrom = np.repeat([0, 1, 2], 20).astype(np.int32)
    copy = np.tile(np.repeat([0, 1], 10), 3).astype(np.int32)
    chain = RP.chain_numbers(chrom, copy)
    copy_ptr = np.arange(0, 61, 2).astype(np.int32)
    copy_idx = np.array([b + 10 * k for c in range(3) for b in range(20 * c, 20 * c + 10) for k in (0, 1)], np.int32)
    cls = (np.arange(60) % 4 - 1).astype(np.int32)
    res = RP.neighbour_census(xyz, 450.0, chain, cls, min_sep=2, ctx=ctx)
    want = N.results(xyz, chain, cls, 3, 2, 450.0)
    for k in OUTS:
        assert res[k].tobytes() == want[k].tobytes(), k
    lean = RP.neighbour_census(xyz, 450.0, chain, cls, min_sep=2, want_census=False, ctx=ctx)
    assert lean['census'] is None and lean['sums'].tobytes() == want['sums'].tobytes()
    with pytest.raises(ValueError):
        RP.neighbour_census(xyz, 450.0, ctx=ctx)                   # host arrays need a chain
    icp = RP.inter_chromosomal_fraction(xyz, 450.0, chain, 2, copy_ptr=copy_ptr, copy_idx=copy_idx, ctx=ctx)
    plain = N.census(xyz, chain, None, 0, 2, 450.0)
    assert np.array_equal(icp, N.icp_per_locus(plain, copy_ptr, copy_idx), equal_nan=True)
    r = np.where(np.arange(60) % 2, 100.0, 150.0).astype(f32)
    res = RP.neighbour_census(xyz, chain=chain, radii=r, contact_range=1.5, ctx=ctx)
    assert res['census'].tobytes() == N.census(xyz, chain, radii=r, contact_range=1.5).tobytes()
    with pytest.raises(RuntimeError, match='distinct radii'):
        RP.neighbour_census(xyz, chain=chain, radii=np.arange(60), contact_range=1.5, ctx=ctx)


def rg_bar(want, ptr, xmax):
    """the bar of tests/test_report_gpu.py for Rg, per window of n beads"""
    n = np.diff(ptr).astype(np.float64)[:, None]
    return 2 * 3 * n * 2.0 ** -53 * want + n * 2.0 ** -52 * xmax


def test_local_compaction(ctx):
    rng = np.random.default_rng(3)
    chrom = np.array([0] * 9 + [1] * 1 + [2] * 30 + [0] * 9 + [2] * 30, np.int32)   # a one-bead chain among them
    copy = np.array([0] * 40 + [1] * 39, np.int32)
    xyz = (rng.standard_normal((79, 67, 3)) * 3000).astype(f32)
    for h in (0, 2, 40):
        a, b = (RP.local_compaction(xyz, chrom, copy, h, ctx=ctx) for _ in range(2))
        assert a.tobytes() == b.tobytes() and a.shape == (79, 67)
        want, ptr = N.local_rg(xyz, chrom, copy, h)
        assert np.all(np.abs(a - want) <= rg_bar(want, ptr, np.abs(xyz).max()))
        assert np.all(a[9] == 0) and (h == 0) == (not a.any())


def test_report_steps_on_the_demo_population(ctx, tmp_path):
    """--steps neighbours,compaction through main() on the demo population (its first three
    structures: the O(N^2) oracle takes a third of a second per structure), every file against
    the oracle"""
    from igm_amd.steps import PopulationStore
    pop = load_golden('demo_population.npz')
    xyz = np.ascontiguousarray(pop['coordinates'][:, :3])
    cp, ci = pop['copy_ptr'], pop['copy_idx']
    nhap = len(cp) - 1
    p = str(tmp_path / 'demo.hss')
    PopulationStore.create(p, xyz, pop['radii'], pop['chrom'], pop['copy'], cp, ci)
    labels = np.random.default_rng(0).integers(-1, 2, nhap)
    np.savetxt(tmp_path / 'classes.txt', labels, fmt='%d')
    out = tmp_path / 'qc'
    assert RP.main([p, '--steps', 'neighbours,compaction', '--classes', str(tmp_path / 'classes.txt'), '--min-sep',
                    '2', '--neighbour-cutoff', '900', '--compaction-halfwidth', '3', '-l', 'run', '-o', str(out)]) == 0
    made = sorted(str(f.relative_to(out)) for f in out.rglob('*') if f.is_file())
    assert made == ['compaction/local_rg-run.txt', 'label.txt', 'neighbours/icp-run.txt',
                    'neighbours/mean_counts-run.txt', 'neighbours/trans_fraction-run.txt']
    bead_cls = np.empty(len(ci), np.int32)
    bead_cls[ci] = np.repeat(labels, np.diff(cp))
    cen = N.census(xyz, pop['chrom'].astype(np.int64) * 64 + pop['copy'], bead_cls, 2, 2, 900.0)
    assert cen[..., 0].any() and cen[..., 1].any() and cen[..., 2].any() and cen[..., 3].any()
    same = lambda name, want: np.array_equal(np.loadtxt(out / name), want, equal_nan=True)  # noqa: E731
    assert same('neighbours/icp-run.txt', N.icp_per_locus(cen, cp, ci))
    assert same('neighbours/mean_counts-run.txt', N.mean_counts(cen, cp, ci))
    assert same('neighbours/trans_fraction-run.txt', N.trans_fraction(cen, cp, ci))
    # the mean and the standard deviation move by no more than the largest error of an Rg
    # (|std(a) - std(b)| <= |a - b|_2 / sqrt(n) <= max |a - b|), plus the rounding of the two
    # reductions themselves
    want, ptr = N.local_rg(xyz, pop['chrom'], pop['copy'], 3)
    tol = rg_bar(want, ptr, np.abs(xyz).max()).max() + 64 * 2.0 ** -53 * want.max()
    rows = np.array([(want[ci[cp[h]:cp[h + 1]]].mean(), want[ci[cp[h]:cp[h + 1]]].std()) for h in range(nhap)])
    got = np.loadtxt(out / 'compaction/local_rg-run.txt')
    assert got.shape == (nhap, 2) and np.all(np.abs(got - rows) <= tol)
    # without classes, at a radius barely above the bead diameter (561) and with the chain neighbours ignored:
    # no trans_fraction file, one trans column, and loci without any neighbour, which are NaN
    out = tmp_path / 'qc2'
    written = RP.report_population(p, steps='neighbours', out_dir=str(out), neighbour_cutoff=580.0, min_sep=2,
                                   ctx=ctx)
    assert sorted(written) == ['label.txt', 'neighbours/icp.txt', 'neighbours/mean_counts.txt']
    cen = N.census(xyz, pop['chrom'].astype(np.int64) * 64 + pop['copy'], cutoff=580.0, min_sep=2)
    want = N.icp_per_locus(cen, cp, ci)
    assert np.isnan(want).any() and not np.isnan(want).all()
    assert same('neighbours/icp.txt', want)
    assert same('neighbours/mean_counts.txt', N.mean_counts(cen, cp, ci)) and cen.shape[2] == 2
