"""Population report kernels on the MI355X (igm_report_levels / _rg / _lamina /
_distance_map), through the C ABI.

Against the reference's own numbers on the demo population (report_golden.npz) and against
the float64 restatement tests/report_ref.py on the smallest shapes at which each kernel can
go wrong.  Bars: integer outputs are equal; per-element values are bit-equal by
construction, so a float64 output differs from the restatement only by the order of a sum
of n non-negative terms, at most 2 n 2^-53 relative (n = nstruct for means over the
structures, the shell size for shell means); Rg sums 3 n signed squares, 2 (3 n) 2^-53
relative plus n 2^-52 max|x| absolute, because centring coincident beads leaves rounding
noise; the reference's float32 sums (Rg, distance means) are within 32 * 2^-24.
Every call is made twice and must return the same bytes."""

import numpy as np
import pytest

import report_ref as R
from conftest import load_golden
from igm_amd import _lib, report as RP

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
F32_SUM_BAR = 32 * 2.0 ** -24


@pytest.fixture(scope='module')
def ctx():
    return _lib.context(0)


@pytest.fixture(scope='module')
def pop():
    return load_golden('demo_population.npz')


@pytest.fixture(scope='module')
def gold():
    return load_golden('report_golden.npz')


def _p(a):
    return None if a is None else a.ctypes.data


def call_levels(ctx, xyz, sx, mean=False, dedges=None, nshell=0, sedges=None, want=('smean', 'shist')):
    """igm_report_levels on host arrays, twice: (rc, mean, density, shell_mean, shell_hist)"""
    xyz = np.ascontiguousarray(xyz, np.float32)
    n, S = xyz.shape[:2]
    sx = np.ascontiguousarray(sx, np.float64)
    outs = []
    for _ in range(2):
        m = np.full(n, -7.0) if mean else None
        de = None if dedges is None else np.ascontiguousarray(dedges, np.float64)
        d = None if de is None else np.full(len(de) - 1, -7, np.int64)
        se = None if sedges is None else np.ascontiguousarray(sedges, np.float64)
        sm = np.full((S, max(nshell, 1)), -7.0) if nshell and 'smean' in want else None
        sh = np.full((max(nshell, 1), len(se) - 1), -7, np.int64) if se is not None and 'shist' in want else None
        rc = ctx.lib.igm_report_levels(ctx.h, 0, xyz.ctypes.data, n, S, sx.ctypes.data, _p(m), _p(de),
                                       0 if de is None else len(de) - 1, _p(d), nshell, _p(sm), _p(se),
                                       0 if se is None else len(se) - 1, _p(sh))
        outs.append((rc, m, d, sm, sh))
    for a, b in zip(outs[0][1:], outs[1][1:]):
        assert (a is None and b is None) or a.tobytes() == b.tobytes(), 'rerun differs'
    assert outs[0][0] == outs[1][0]
    return outs[0]


def twice(fn):
    a, b = fn(), fn()
    assert a.tobytes() == b.tobytes(), 'rerun differs'
    return a


def rel_close(got, want, bar):
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    print('max rel err %.3g (bar %.3g)' % (np.max(err / np.maximum(np.abs(want[ok]), 1e-300), initial=0.0), bar))
    assert np.all(err <= bar * np.abs(want[ok]))


def rg_close(rg, want, chain_ptr, xmax):
    """2 (3 n) 2^-53 relative plus n 2^-52 max|x| absolute, n the chain's length"""
    n = np.diff(chain_ptr).astype(np.float64)[:, None]
    err = np.abs(rg - want)
    print('max rg err %.3g' % err.max())
    assert np.all(err <= 2 * 3 * n * U53 * want + n * 2.0 ** -52 * xmax)


def synthetic(chrom_loci, copies, S, seed, scale=3000.0):
    """A population in the layout alabtools writes: first copies in locus order, then the
    second copies, ...; copies[h] is the copy count of haploid locus h."""
    hap_chrom = np.repeat(np.arange(len(chrom_loci)), chrom_loci).astype(np.int32)
    copies = np.asarray(copies)
    assert len(copies) == len(hap_chrom)
    rows, chrom, copy = [[] for _ in copies], [], []
    for k in range(copies.max()):
        for h in np.flatnonzero(copies > k):
            rows[h].append(len(chrom))
            chrom.append(hap_chrom[h])
            copy.append(k)
    ptr = np.concatenate([[0], np.cumsum(copies)]).astype(np.int32)
    idx = np.array([b for r in rows for b in r], np.int32)
    rng = np.random.default_rng(seed)
    xyz = (rng.standard_normal((len(chrom), S, 3)) * scale).astype(np.float32)
    radii = rng.uniform(100, 300, len(chrom)).astype(np.float32)
    return {'xyz': xyz, 'radii': radii, 'chrom': np.array(chrom, np.int32), 'copy': np.array(copy, np.int32),
            'copy_ptr': ptr, 'copy_idx': idx, 'hap_chrom': hap_chrom}


# ------------------------------------------------------------------ the demo population
def test_demo_levels_bit_equal_and_means(ctx, pop, gold):
    crd, sx = pop['coordinates'], gold['semiaxes']
    # one structure at a time the mean is the level itself: bit-equal to the NumPy expression
    for s in (0, 57, 99):
        rc, mean, _, _, _ = call_levels(ctx, crd[:, s:s + 1], sx, mean=True)
        assert rc == 0 and mean.tobytes() == R.levels(crd[:, s:s + 1], sx)[:, 0].tobytes()
    rc, mean, _, _, _ = call_levels(ctx, crd, sx, mean=True)
    assert rc == 0
    rel_close(mean, R.level_mean(crd, sx), 2 * 100 * U53)
    got = RP.average_copies(mean, pop['copy_ptr'], pop['copy_idx'])
    rel_close(got, gold['radial_level'], 2 * 100 * U53)
    assert np.array_equal(got, RP.radial_levels(crd, sx, pop['copy_ptr'], pop['copy_idx'], ctx=ctx))


def test_demo_density_and_shells(ctx, pop, gold):
    crd, sx = pop['coordinates'], gold['semiaxes']
    dedges, sedges = np.linspace(0, 1.1, 12), np.linspace(0, 1.5, 151)
    rc, _, dens, smean, shist = call_levels(ctx, crd, sx, dedges=dedges, nshell=5, sedges=sedges)
    assert rc == 0
    volumes = np.array([dedges[i + 1]**3 - dedges[i]**3 for i in range(11)])
    assert (dens / volumes).tobytes() == gold['density_histo'].tobytes()
    want_mean, want_hist = R.shells(crd, sx, 5, sedges)
    assert np.array_equal(shist, want_hist) and shist.sum() == crd.shape[0] * crd.shape[1]
    rel_close(smean, want_mean, 2 * 602 * U53)
    rel_close(np.average(smean, axis=0), gold['ave_radial'], 2 * 602 * U53 + 2 * 100 * U53)
    assert ctx.kernel_ms('report_levels') > 0


def test_demo_rg(ctx, pop, gold):
    crd = pop['coordinates']
    ids, chrom_ptr, chain_ptr, chain_idx = RP.chains(pop['chrom'], pop['copy'])
    rg = twice(lambda: RP.chain_rgs(crd, chain_ptr, chain_idx, ctx=ctx))
    assert rg.shape == (46, 100)
    rel_close(rg.ravel(), gold['rgs_values'].astype(np.float64), F32_SUM_BAR)
    want = R.rg(crd, chain_ptr, chain_idx)
    rg_close(rg, want, chain_ptr, np.abs(crd).max())
    names, per_chrom = RP.chromosome_rgs(crd, pop['chrom'], pop['copy'], ctx=ctx)
    assert np.array_equal(np.concatenate(per_chrom), rg.ravel()) and len(names) == 24


def test_demo_lamina(ctx, pop, gold):
    crd, cp, ci = pop['coordinates'], pop['copy_ptr'], pop['copy_idx']
    cr = float(gold['contact_range'])
    freq = twice(lambda: RP.lamina_frequency(crd, pop['radii'], cp, ci, gold['semiaxes'], cr, ctx=ctx))
    assert freq.tobytes() == gold['damid_output'].tobytes()
    counts, _ = RP.lamina_counts(crd, pop['radii'], cp, ci, gold['semiaxes'], cr, ctx=ctx)
    den = R.lamina_denoms(gold['semiaxes'], cr, pop['radii'], cp, ci)
    assert np.array_equal(counts, R.lamina_counts(crd, cp, ci, den)) and counts.sum() > 0


def test_demo_distance_map(ctx, pop, gold):
    """all 1558 loci: 24 full tiles and a 22-wide edge, 100 structures = 3 chunks of 32 + 4"""
    crd, cp, ci, hc = pop['coordinates'], pop['copy_ptr'], pop['copy_idx'], pop['hap_chrom']
    d = twice(lambda: RP.average_distance_map(crd, cp, ci, hc, ctx=ctx))
    assert d.shape == (1558, 1558) and np.array_equal(d, d.T) and not d.diagonal().any()
    assert np.all(np.isfinite(d))
    loci = gold['dmap_loci']
    iu = np.triu_indices(len(loci), 1)
    rel_close(d[np.ix_(loci, loci)][iu], gold['dmap'][iu], F32_SUM_BAR)
    rng = np.random.default_rng(11)
    a, b = rng.integers(0, 1558, 2000), rng.integers(0, 1558, 2000)
    want = np.array([R.distance_entry(crd, cp, ci, hc, i, j) for i, j in zip(a, b)])
    rel_close(d[a, b], want, 2 * 100 * U53)
    assert ctx.kernel_ms('report_distance_map') > 0


def test_demo_command_line(pop, gold, tmp_path):
    """python -m igm_amd.report's main() on a demo .hss writes the reference's files"""
    from igm_amd.steps import PopulationStore
    p = str(tmp_path / 'demo.hss')
    PopulationStore.create(p, pop['coordinates'], pop['radii'], pop['chrom'], pop['copy'], pop['copy_ptr'],
                           pop['copy_idx'])
    sx = [str(v) for v in gold['semiaxes']]
    assert RP.main([p, '--semiaxes'] + sx + ['-o', str(tmp_path / 'qc')]) == 0
    out = tmp_path / 'qc'
    for n in ('radius_of_gyration/chromosomes.npz', 'shells/ave_radial.txt', 'radials/radials.txt',
              'radials/density_histo.txt', 'radials/radials_norm.txt', 'damid/output.txt',
              'distance_map/average.npy'):
        assert (out / n).is_file(), n
    assert np.loadtxt(out / 'damid/output.txt').tobytes() == gold['damid_output'].tobytes()
    assert np.loadtxt(out / 'radials/density_histo.txt').tobytes() == gold['density_histo'].tobytes()
    rel_close(np.loadtxt(out / 'radials/radials.txt'), gold['radial_level'], 2 * 100 * U53)
    assert len(np.load(out / 'radius_of_gyration/chromosomes.npz').files) == 24


# ------------------------------------------------------------------ synthetic smallest shapes
@pytest.mark.parametrize('S', [1, 33, 64])
def test_chunk_edges_every_entry_point(ctx, S):
    """nstruct 1, 33 and 64: a structure chunk of the level tile (32) and of the distance
    tile (32) that is partial, full + 1, and exactly full"""
    p = synthetic([40, 31], [2] * 40 + [1] * 31, S, seed=S)
    xyz, sx = p['xyz'], (5000.0, 4000.0, 3500.0)
    dedges, sedges = np.linspace(0, 1.1, 12), np.linspace(0, 1.5, 151)
    rc, mean, dens, smean, shist = call_levels(ctx, xyz, sx, mean=True, dedges=dedges, nshell=5, sedges=sedges)
    assert rc == 0
    rel_close(mean, R.level_mean(xyz, sx), 2 * S * U53)
    assert np.array_equal(dens, R.histogram(R.levels(xyz, sx), dedges))
    wm, wh = R.shells(xyz, sx, 5, sedges)
    rel_close(smean, wm, 2 * 23 * U53)
    assert np.array_equal(shist, wh)
    _, _, cptr, cidx = RP.chains(p['chrom'], p['copy'])
    rg = twice(lambda: RP.chain_rgs(xyz, cptr, cidx, ctx=ctx))
    want = R.rg(xyz, cptr, cidx)
    rg_close(rg, want, cptr, np.abs(xyz).max())
    den = R.lamina_denoms(sx, 0.05, p['radii'], p['copy_ptr'], p['copy_idx'])
    cnt, _ = RP.lamina_counts(xyz, p['radii'], p['copy_ptr'], p['copy_idx'], sx, 0.05, ctx=ctx)
    assert np.array_equal(cnt, R.lamina_counts(xyz, p['copy_ptr'], p['copy_idx'], den))
    d = twice(lambda: RP.average_distance_map(xyz, p['copy_ptr'], p['copy_idx'], p['hap_chrom'], ctx=ctx))
    rel_close(d, R.distance_map(xyz, p['copy_ptr'], p['copy_idx'], p['hap_chrom']), 2 * S * U53)


@pytest.mark.parametrize('nhap', [65, 130])
def test_distance_map_tile_edges_and_mixed_copies(ctx, nhap):
    """a tile edge (64 + 1, 2 * 64 + 2) with copy counts 1, 2 and 3 mixed inside one
    chromosome and across chromosomes: the zip truncation on one chromosome (the k-th with
    the k-th copy up to the smaller count), every copy pair across chromosomes, the masked
    passes of missing copies"""
    rng = np.random.default_rng(nhap)
    sizes = [nhap // 2, nhap - nhap // 2 - 7, 7]
    copies = rng.integers(1, 4, nhap)
    copies[-7:] = 1
    copies[:3] = (3, 1, 2)
    p = synthetic(sizes, copies, 5, seed=nhap)
    d = twice(lambda: RP.average_distance_map(p['xyz'], p['copy_ptr'], p['copy_idx'], p['hap_chrom'], ctx=ctx))
    want = R.distance_map(p['xyz'], p['copy_ptr'], p['copy_idx'], p['hap_chrom'])
    rel_close(d, want, 2 * 5 * U53)
    assert np.array_equal(d, d.T) and not d.diagonal().any()
    # the reference's quirk: on one chromosome only the k-th with the k-th copy counts
    a, b = 0, 2  # 3 and 2 copies on chromosome 0
    ca, cb = p['copy_idx'][p['copy_ptr'][a]:], p['copy_idx'][p['copy_ptr'][b]:]
    two = (R.pair_mean(p['xyz'], ca[0], cb[0]) + R.pair_mean(p['xyz'], ca[1], cb[1])) / 2
    assert abs(d[a, b] - two) <= 2 * 5 * U53 * two


def test_distance_map_locus_without_copies(ctx):
    p = synthetic([4], [1, 2, 1, 1], 3, seed=1)
    ptr = np.array([0, 1, 1, 3, 4], np.int32)  # locus 1 has no copy
    idx = np.array([0, 1, 2, 3], np.int32)
    d = RP.average_distance_map(p['xyz'], ptr, idx, np.zeros(4, np.int32), ctx=ctx)
    assert np.isnan(d[1, [0, 2, 3]]).all() and np.isnan(d[[0, 2, 3], 1]).all() and d[1, 1] == 0
    assert np.isfinite(d[0, 2]) and d[0, 2] == d[2, 0]


def test_empty_shells_are_nan(ctx):
    """nbead 3 with nshell 5: the shells [0,0) and [1,1) are empty"""
    xyz = np.random.default_rng(2).uniform(-1, 1, (3, 4, 3)).astype(np.float32)
    edges = np.linspace(0, 2, 21)
    rc, _, _, smean, shist = call_levels(ctx, xyz, (1.0, 1.0, 1.0), nshell=5, sedges=edges)
    assert rc == 0
    wm, wh = R.shells(xyz, (1.0, 1.0, 1.0), 5, edges)
    assert np.isnan(smean[:, [0, 2]]).all() and np.array_equal(np.isnan(smean), np.isnan(wm))
    assert np.array_equal(smean[:, [1, 3, 4]], wm[:, [1, 3, 4]])  # one level per shell: the level itself
    assert np.array_equal(shist, wh) and shist[[0, 2]].sum() == 0


def test_all_levels_tied(ctx):
    """every bead at one point: each shell boundary falls inside one run of equal levels"""
    xyz = np.tile(np.array([300.0, -400.0, 1200.0], np.float32), (103, 3, 1))
    edges = np.linspace(0, 1.5, 151)
    rc, mean, _, smean, shist = call_levels(ctx, xyz, (5000.0,) * 3, mean=True, nshell=5, sedges=edges)
    assert rc == 0
    lev = R.levels(xyz, (5000.0,) * 3)[0, 0]
    rel_close(smean, np.full((3, 5), lev), 2 * 21 * U53)
    sizes = np.diff(R.shell_bounds(103, 5))
    k = np.searchsorted(edges, lev, side='right') - 1
    assert np.array_equal(shist[:, k], 3 * sizes) and shist.sum() == 3 * 103
    # partial ties: two values, the boundary ranks fall inside the runs
    xyz2 = xyz.copy()
    xyz2[40:] *= 2
    rc, _, _, smean, shist = call_levels(ctx, xyz2, (5000.0,) * 3, nshell=5, sedges=edges)
    wm, wh = R.shells(xyz2, (5000.0,) * 3, 5, edges)
    rel_close(smean, wm, 2 * 21 * U53)
    assert np.array_equal(shist, wh)


def test_levels_on_histogram_edges(ctx):
    """levels exactly on an edge and one step either side, at 0, at the last edge and beyond;
    edges one float64 ulp off a level.  With unit semiaxes and points on the x axis the level
    is |x| exactly."""
    f = np.float32
    vals = np.array([0.0, np.nextafter(f(0), f(1)), 0.25, np.nextafter(f(0.25), f(0)), np.nextafter(f(0.25), f(1)),
                     0.5, np.nextafter(f(0.5), f(0)), 0.75, 1.0, np.nextafter(f(1), f(0)), np.nextafter(f(1), f(2)),
                     1.5, -0.5, -1.0], np.float32)
    xyz = np.zeros((len(vals), 2, 3), np.float32)
    xyz[:, 0, 0] = vals
    xyz[:, 1, 0] = vals[::-1]
    edges = np.array([0.0, np.nextafter(0.25, 1.0), 0.5, np.nextafter(0.75, 0.0), 1.0])
    rc, _, dens, smean, shist = call_levels(ctx, xyz, (1.0, 1.0, 1.0), dedges=edges, nshell=2, sedges=edges)
    assert rc == 0
    lev = R.levels(xyz, (1.0, 1.0, 1.0))
    assert np.array_equal(lev[:, 0], np.abs(vals).astype(np.float64))
    want = np.histogram(lev.ravel(), bins=edges)[0]
    assert np.array_equal(dens, want) and np.array_equal(dens, R.histogram(lev, edges))
    assert dens.sum() == 2 * (len(vals) - 2)  # the two levels beyond the last edge are dropped
    assert np.array_equal(shist, R.shells(xyz, (1.0, 1.0, 1.0), 2, edges)[1])
    # first edge above 0: the zero levels are dropped too
    rc, _, dens, _, _ = call_levels(ctx, xyz, (1.0, 1.0, 1.0), dedges=edges[1:])
    assert np.array_equal(dens, np.histogram(lev.ravel(), bins=edges[1:])[0])


def test_lamina_at_one(ctx):
    """values exactly 1 and one ulp either side: the denominators are given directly"""
    x = np.float32(1234.567)
    xx = np.float64(x * x)
    xyz = np.zeros((3, 2, 3), np.float32)
    xyz[:, :, 0] = x
    den = np.array([[xx, 1.0, 1.0], [np.nextafter(xx, np.inf), 1.0, 1.0], [np.nextafter(xx, 0.0), 1.0, 1.0]])
    ptr, idx = np.arange(4, dtype=np.int32), np.arange(3, dtype=np.int32)
    out = np.full(3, -1, np.int64)
    rc = ctx.lib.igm_report_lamina(ctx.h, 0, xyz.ctypes.data, 3, 2, ptr.ctypes.data, idx.ctypes.data, 3,
                                   den.ctypes.data, out.ctypes.data)
    assert rc == 0 and out.tolist() == [2, 0, 2]
    assert np.array_equal(out, R.lamina_counts(xyz, ptr, idx, den))


def test_rg_degenerate_chains(ctx):
    """a chain of one bead (Rg 0), a chain of coincident beads (rounding noise only), a chain
    whose beads lie on both sides of bead 64 and out of order"""
    rng = np.random.default_rng(5)
    xyz = (rng.standard_normal((150, 3, 3)) * 3000).astype(np.float32)
    xyz[100:120] = xyz[100]
    chain_idx = np.concatenate([[7], np.arange(100, 120), np.arange(30, 100)[::-1], np.arange(120, 150)]).astype(np.int32)
    chain_ptr = np.array([0, 1, 21, 91, 121], np.int32)
    rg = twice(lambda: RP.chain_rgs(xyz, chain_ptr, chain_idx, ctx=ctx))
    want = R.rg(xyz, chain_ptr, chain_idx)
    assert np.all(rg[0] == 0)
    assert np.all(rg[1] <= 20 * 2.0 ** -52 * np.abs(xyz).max())
    rg_close(rg, want, chain_ptr, np.abs(xyz).max())
    assert np.all(rg[2:] > 100)


@pytest.mark.parametrize('nbead,S', [(20001, 3), (65535, 2)])
def test_large_structures(ctx, nbead, S):
    """more levels than fit LDS (every select pass streams them from memory), up to the
    size limit"""
    rng = np.random.default_rng(nbead)
    xyz = (rng.standard_normal((nbead, S, 3)) * 2500).astype(np.float32)
    xyz[::7] = xyz[0]  # runs of equal levels across the boundaries too
    sx = (5000.0, 4500.0, 4000.0)
    dedges, sedges = np.linspace(0, 1.1, 12), np.linspace(0, 1.5, 151)
    rc, mean, dens, smean, shist = call_levels(ctx, xyz, sx, mean=True, dedges=dedges, nshell=5, sedges=sedges)
    assert rc == 0
    rel_close(mean, R.level_mean(xyz, sx), 2 * S * U53)
    assert np.array_equal(dens, R.histogram(R.levels(xyz, sx), dedges))
    wm, wh = R.shells(xyz, sx, 5, sedges)
    rel_close(smean, wm, 2 * (nbead // 5 + 1) * U53)
    assert np.array_equal(shist, wh)


def test_many_shells_and_bins(ctx):
    """more shells than one select group (8) and more bins than the LDS histograms hold"""
    xyz = (np.random.default_rng(9).standard_normal((500, 2, 3)) * 2500).astype(np.float32)
    sx = (5000.0,) * 3
    dedges, sedges = np.linspace(0, 1.1, 1501), np.linspace(0, 1.5, 301)
    rc, _, dens, smean, shist = call_levels(ctx, xyz, sx, dedges=dedges, nshell=21, sedges=sedges)
    assert rc == 0
    assert np.array_equal(dens, R.histogram(R.levels(xyz, sx), dedges))
    wm, wh = R.shells(xyz, sx, 21, sedges)
    rel_close(smean, wm, 2 * 24 * U53)
    assert np.array_equal(shist, wh)


def test_nullable_outputs(ctx):
    xyz = (np.random.default_rng(4).standard_normal((70, 9, 3)) * 2500).astype(np.float32)
    sx = (5000.0, 4000.0, 3000.0)
    dedges, sedges = np.linspace(0, 1.1, 12), np.linspace(0, 1.5, 151)
    rc, mean, dens, smean, shist = call_levels(ctx, xyz, sx, mean=True, dedges=dedges, nshell=5, sedges=sedges)
    assert rc == 0
    assert call_levels(ctx, xyz, sx, mean=True)[1].tobytes() == mean.tobytes()
    assert call_levels(ctx, xyz, sx, dedges=dedges)[2].tobytes() == dens.tobytes()
    only_mean = call_levels(ctx, xyz, sx, nshell=5, want=('smean',))
    assert only_mean[3].tobytes() == smean.tobytes() and only_mean[4] is None
    only_hist = call_levels(ctx, xyz, sx, nshell=5, sedges=sedges, want=('shist',))
    assert only_hist[4].tobytes() == shist.tobytes() and only_hist[3] is None
    assert call_levels(ctx, xyz, sx)[0] == 0  # nothing asked: nothing to do


def test_device_pointers(ctx):
    """IGM_DEVICE_PTRS: xyz and the outputs are device memory, the small inputs stay on the host"""
    import torch
    p = synthetic([40, 30], [2] * 40 + [1] * 30, 37, seed=3)
    xyz, sx = p['xyz'], np.array([5000.0, 4000.0, 3000.0])
    dedges, sedges = np.linspace(0, 1.1, 12), np.linspace(0, 1.5, 151)
    n, S, nhap = xyz.shape[0], xyz.shape[1], 70
    dx = torch.from_numpy(xyz).cuda()
    f64 = dict(dtype=torch.float64, device='cuda')
    i64 = dict(dtype=torch.int64, device='cuda')
    mean, dens = torch.empty(n, **f64), torch.empty(11, **i64)
    smean, shist = torch.empty((S, 5), **f64), torch.empty((5, 150), **i64)
    F = _lib.IGM_DEVICE_PTRS
    rc = ctx.lib.igm_report_levels(ctx.h, F, dx.data_ptr(), n, S, sx.ctypes.data, mean.data_ptr(),
                                   dedges.ctypes.data, 11, dens.data_ptr(), 5, smean.data_ptr(), sedges.ctypes.data,
                                   150, shist.data_ptr())
    ctx.check(rc, 'igm_report_levels')
    host = call_levels(ctx, xyz, sx, mean=True, dedges=dedges, nshell=5, sedges=sedges)
    for dev, h in zip((mean, dens, smean, shist), host[1:]):
        assert dev.cpu().numpy().tobytes() == h.tobytes()
    _, _, cptr, cidx = RP.chains(p['chrom'], p['copy'])
    rg = torch.empty((len(cptr) - 1, S), **f64)
    ctx.check(ctx.lib.igm_report_rg(ctx.h, F, dx.data_ptr(), n, S, cptr.ctypes.data, cidx.ctypes.data, len(cptr) - 1,
                                    rg.data_ptr()), 'igm_report_rg')
    assert rg.cpu().numpy().tobytes() == RP.chain_rgs(xyz, cptr, cidx, ctx=ctx).tobytes()
    den = RP.lamina_denominators(sx, 0.05, p['radii'], p['copy_ptr'], p['copy_idx'])
    cnt = torch.empty(nhap, **i64)
    ctx.check(ctx.lib.igm_report_lamina(ctx.h, F, dx.data_ptr(), n, S, p['copy_ptr'].ctypes.data,
                                        p['copy_idx'].ctypes.data, nhap, den.ctypes.data, cnt.data_ptr()),
              'igm_report_lamina')
    want, _ = RP.lamina_counts(xyz, p['radii'], p['copy_ptr'], p['copy_idx'], sx, 0.05, ctx=ctx)
    assert np.array_equal(cnt.cpu().numpy(), want)
    dmap = torch.empty((nhap, nhap), **f64)
    ctx.check(ctx.lib.igm_report_distance_map(ctx.h, F, dx.data_ptr(), n, S, p['copy_ptr'].ctypes.data,
                                              p['copy_idx'].ctypes.data, p['hap_chrom'].ctypes.data, nhap,
                                              dmap.data_ptr()), 'igm_report_distance_map')
    want = RP.average_distance_map(xyz, p['copy_ptr'], p['copy_idx'], p['hap_chrom'], ctx=ctx)
    assert dmap.cpu().numpy().tobytes() == want.tobytes()


def test_invalid_arguments(ctx):
    """IGM_E_INVALID with a message, and nothing launched: the outputs keep their fill"""
    xyz = np.ones((6, 2, 3), np.float32)
    good = np.linspace(0, 1, 5)

    def message():
        return ctx.lib.igm_last_error(ctx.h).decode()

    for sx in ((1.0, 0.0, 1.0), (1.0, -2.0, 1.0), (np.nan, 1.0, 1.0), (np.inf, 1.0, 1.0)):
        rc, mean, _, _, _ = call_levels(ctx, xyz, sx, mean=True)
        assert rc == _lib.IGM_E_INVALID and 'semiaxes' in message() and np.all(mean == -7.0)
    for bad in (np.array([0.0, 0.5, 0.4, 0.8, 1.0]), np.array([0.0, 0.5, np.nan, 0.8, 1.0])):
        rc, _, dens, _, _ = call_levels(ctx, xyz, (1.0,) * 3, dedges=bad)
        assert rc == _lib.IGM_E_INVALID and 'density_edges' in message() and np.all(dens == -7)
        rc, _, _, smean, shist = call_levels(ctx, xyz, (1.0,) * 3, nshell=2, sedges=bad)
        assert rc == _lib.IGM_E_INVALID and 'shell_edges' in message() and np.all(shist == -7)
    sm = np.full((2, 1), -7.0)
    sx = np.ones(3)
    for nshell in (0, -3):
        rc = ctx.lib.igm_report_levels(ctx.h, 0, xyz.ctypes.data, 6, 2, sx.ctypes.data, None, None, 0, None, nshell,
                                       sm.ctypes.data, good.ctypes.data, 4, None)
        assert rc == _lib.IGM_E_INVALID and 'nshell' in message() and np.all(sm == -7.0)
    big = np.zeros((65536, 1, 3), np.float32)
    assert call_levels(ctx, big, (1.0,) * 3, mean=True)[0] == _lib.IGM_E_UNSUPPORTED
    # CSR: a first entry that is not 0, a decreasing pointer, an index out of range
    out = np.full((2, 2), -7.0)
    for ptr, idx in (([1, 2, 3], [0, 1, 2]), ([0, 3, 2], [0, 1, 2]), ([0, 1, 3], [0, 1, 6]), ([0, 1, 3], [0, -1, 2])):
        ptr, idx = np.array(ptr, np.int32), np.array(idx, np.int32)
        rc = ctx.lib.igm_report_rg(ctx.h, 0, xyz.ctypes.data, 6, 2, ptr.ctypes.data, idx.ctypes.data, 2,
                                   out.ctypes.data)
        assert rc == _lib.IGM_E_INVALID and 'chain' in message() and np.all(out == -7.0)
        cnt = np.full(2, -7, np.int64)
        den = np.ones((2, 3))
        rc = ctx.lib.igm_report_lamina(ctx.h, 0, xyz.ctypes.data, 6, 2, ptr.ctypes.data, idx.ctypes.data, 2,
                                       den.ctypes.data, cnt.ctypes.data)
        assert rc == _lib.IGM_E_INVALID and 'copy' in message() and np.all(cnt == -7)
        hc = np.zeros(2, np.int32)
        rc = ctx.lib.igm_report_distance_map(ctx.h, 0, xyz.ctypes.data, 6, 2, ptr.ctypes.data, idx.ctypes.data,
                                             hc.ctypes.data, 2, out.ctypes.data)
        assert rc == _lib.IGM_E_INVALID and 'copy' in message() and np.all(out == -7.0)
    ptr, idx = np.array([0, 1, 3], np.int32), np.array([0, 1, 2], np.int32)
    den = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, 1.0]])
    cnt = np.full(2, -7, np.int64)
    rc = ctx.lib.igm_report_lamina(ctx.h, 0, xyz.ctypes.data, 6, 2, ptr.ctypes.data, idx.ctypes.data, 2,
                                   den.ctypes.data, cnt.ctypes.data)
    assert rc == _lib.IGM_E_INVALID and 'inv_denoms' in message() and np.all(cnt == -7)
    assert ctx.lib.igm_report_rg(ctx.h, 0, None, 6, 2, ptr.ctypes.data, idx.ctypes.data, 2, out.ctypes.data) == \
        _lib.IGM_E_INVALID and message()
    assert ctx.lib.igm_report_rg(ctx.h, 0, xyz.ctypes.data, 6, 0, ptr.ctypes.data, idx.ctypes.data, 2,
                                 out.ctypes.data) == _lib.IGM_E_INVALID
    # the context still works after the errors
    assert np.all(RP.chain_rgs(xyz, ptr, idx, ctx=ctx) == 0)
