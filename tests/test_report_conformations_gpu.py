"""The pairwise conformation RMSD (igm_report_conformations) and the conformations report
step on the MI355X, against the NumPy restatement tests/report_conformations_ref.py.

Every call is made twice from outputs pre-filled with -7, which no result equals (an RMSD,
a g, a sum and a count are >= 0 or NaN), and the two runs must be bytewise equal.

The matrix is checked within the project's bar for this superposition core
(tests/tracing_assign.py: bound), |gpu - ref| <= 1e-6 ref + sqrt(1e-12 (g_a + g_b) / nlocus):
the float32 rounding plus the float64 cancellation in g_a + g_b - 2 lambda; it holds while
nlocus <= 9000 and the cases here stop at 300.  The worst ratio to the bar is printed.
Exact: the matrix is bitwise symmetric with a zero diagonal; same, hist and row_n equal the
values recomputed on the host from the returned float32 matrix; row_sum is within
(M + 1) 2^-53 relative of the sequential float64 sum of that matrix's row (non-negative
terms: the rounding of M additions on each side); g within 4 nlocus 2^-53 relative of the
restatement; every reduction without the matrix has the bytes of the same reduction with it.

Shapes.  The pair kernel owns tiles of 64 x 64 conformations (512 threads, 2 x 4 pairs each)
and stages 8 loci at a time; the preparation kernel cuts the loci in 16 runs.  M sits on
both sides of one and two tile widths (63, 64, 65, 127, 128, 129, reached with 3, 2, 1, 1, 2
and 3 copies, so that a copy boundary falls inside a tile and nstruct is 21, 32, 65, 127, 64,
43), and M = 1 and 2; nlocus is 1, 2, 3, then 7, 8, 9 and 15, 16, 17 around one and two
chunks and the 16 runs, and IGM_CONFORMATION_CHUNK = 3 puts 2, 3, 4, 6 and 7 around a
smaller chunk; 390 conformations of 300 loci is the largest call.  The bead table
interleaves the copies and descends with the locus."""
import numpy as np
import pytest

import report_conformations_ref as C
from igm_amd import _lib, report as RP

pytestmark = pytest.mark.gpu

f32 = np.float32
OUTS = ('rmsd', 'g', 'row_sum', 'row_n', 'same', 'hist')
DTYPE = {'rmsd': f32, 'g': np.float64, 'row_sum': np.float64, 'row_n': np.int32, 'same': f32, 'hist': np.int64}
FILL = -7
PERM = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
EDGES = np.concatenate([np.linspace(0.0, 1500.0, 31), [4000.0]]).astype(f32)


@pytest.fixture(scope='module')
def ctx():
    return _lib.context(0)


def call(ctx, xyz, bead, edges=EDGES, outs=OUTS, over=()):
    """igm_report_conformations on host arrays, twice: (rc, {name: array or None}); over replaces
    arguments of the C call by name"""
    xyz = np.ascontiguousarray(xyz, f32)
    bead = np.ascontiguousarray(bead, np.int32)
    nbead, S = xyz.shape[:2]
    ncopy, nlocus = bead.shape
    M = ncopy * S
    edges = None if edges is None else np.ascontiguousarray(edges, f32)
    nbin = max(len(edges) - 1, 1) if edges is not None else 1
    shape = {'rmsd': (M, M), 'g': (M,), 'row_sum': (M,), 'row_n': (M,), 'same': (S, ncopy, ncopy), 'hist': (nbin,)}
    a = dict(xyz=xyz.ctypes.data, nbead=nbead, nstruct=S, bead=bead.ctypes.data, ncopy=ncopy, nlocus=nlocus,
             edges=_lib.ptr(edges), nedge=0 if edges is None else len(edges))
    a.update(dict(over))
    runs = []
    for _ in range(2):
        o = {k: np.full(shape[k], FILL, DTYPE[k]) if k in outs else None for k in OUTS}
        rc = ctx.lib.igm_report_conformations(ctx.h, 0, a['xyz'], a['nbead'], a['nstruct'], a['bead'], a['ncopy'],
                                              a['nlocus'], a['edges'], a['nedge'], *(_lib.ptr(o[k]) for k in OUTS))
        runs.append((rc, o))
    assert runs[0][0] == runs[1][0]
    for k in OUTS:
        p, q = runs[0][1][k], runs[1][1][k]
        assert (p is None and q is None) or p.tobytes() == q.tobytes(), 'rerun differs in %s' % k
    return runs[0]


def bead_table(ncopy, nlocus, pad=3):
    """copies interleaved, descending with the locus, `pad` beads in front that nobody uses"""
    k, i = np.arange(ncopy)[:, None], np.arange(nlocus)[None, :]
    return (pad + (nlocus - 1 - i) * ncopy + k).astype(np.int32), pad + ncopy * nlocus + 2


def population(ncopy, S, nlocus, seed, special=True):
    """(xyz, bead, planted): random walks at nucleus scale, 1e5 from the origin, on multiples
    of 1/64 (exact in float32, and so are the images made from them); planted {name: (a, b)}
    where conformation b is an exact duplicate / rigid image / mirror image of a, and the
    collinear, collapsed, NaN and inf conformations"""
    rng = np.random.default_rng(seed)
    M = ncopy * S
    step = rng.normal(size=(M, nlocus, 3))
    step = 100.0 * step / np.linalg.norm(step, axis=2, keepdims=True)
    step[:, 0] = rng.uniform(-3000.0, 3000.0, (M, 3))
    conf = np.round((1e5 + np.cumsum(step, axis=1)) * 64.0) / 64.0
    planted = {}
    if special and M >= 60:
        # far apart, so that pairs cross tiles and copies; M - 1 sits in the last, partial tile
        planted = {'duplicate': (0, M - 1), 'rigid': (1, M // 2), 'mirror': (2, M // 3), 'collinear': M // 4,
                   'collapsed': M // 5, 'collapsed2': M - 2, 'nan': M // 6, 'inf': M // 8 + 1}
        conf[M - 1] = conf[0]
        conf[M // 2] = conf[1] @ PERM.T + np.array([3000.0, -3000.0, 3000.0])
        conf[M // 3] = conf[2] * np.array([1.0, 1.0, -1.0]) + np.array([0.0, 0.0, 2e5])
        conf[M // 4] = conf[M // 4, 0] + np.arange(nlocus)[:, None] * np.array([50.0, 25.0, -12.5])
        conf[M // 5] = conf[M // 5, 0]
        conf[M - 2] = conf[M - 2, 0]
    bead, nbead = bead_table(ncopy, nlocus)
    xyz = rng.uniform(9e4, 1.1e5, (nbead, S, 3))                # the unused beads hold something too
    for k in range(ncopy):
        xyz[bead[k]] = conf[k * S:(k + 1) * S].transpose(1, 0, 2)
    xyz = xyz.astype(f32)
    assert np.array_equal(C.gather(xyz, bead), conf)
    if planted:
        a = planted['nan']
        xyz[bead[a // S, nlocus // 2], a % S, 1] = np.nan
        a = planted['inf']
        xyz[bead[a // S, 0], a % S, 2] = -np.inf
    return xyz, bead, planted


def check(ctx, xyz, bead, edges=EDGES, label=''):
    """the full contract of one call; returns (outputs, restatement)"""
    S, nlocus = xyz.shape[1], bead.shape[1]
    rc, got = call(ctx, xyz, bead, edges)
    assert rc == 0, ctx.lib.igm_last_error(ctx.h).decode()
    want = C.conformations(xyz, bead, edges)
    r, M = got['rmsd'], len(got['g'])
    # the matrix: symmetric to the bit, zero (or NaN) diagonal, NaN exactly where the restatement has it
    assert r.tobytes() == np.ascontiguousarray(r.T).tobytes()
    bad = np.isnan(want['g'])
    assert np.array_equal(np.isnan(got['g']), bad) and np.array_equal(np.isnan(r), np.isnan(want['rmsd']))
    assert not r.diagonal()[~bad].any() and not np.signbit(r.diagonal()[~bad]).any()
    ok = ~np.isnan(want['rmsd'])
    bar = C.bound(want['rmsd'], np.where(bad, 0.0, want['g']), nlocus)
    diff = np.abs(r.astype(np.float64) - want['rmsd'].astype(np.float64))
    ratio = np.max(diff[ok] / np.maximum(bar[ok], 1e-300), initial=0.0)
    print('%s M %d nlocus %d: worst |gpu - ref| / bar %.3g (largest difference %.3g)'
          % (label, M, nlocus, ratio, np.max(diff[ok], initial=0.0)))
    assert np.all(diff[ok] <= bar[ok])
    # g
    gg, gw = got['g'][~bad], want['g'][~bad]
    assert np.all(np.abs(gg - gw) <= 4 * nlocus * 2.0 ** -53 * gw)
    # the reductions, from the returned matrix
    mine = C.reductions(r, S, edges)
    assert np.array_equal(got['row_n'], mine['row_n'])
    assert np.array_equal(got['same'], mine['same'], equal_nan=True)
    assert np.array_equal(got['hist'], mine['hist'])
    assert np.all(np.abs(got['row_sum'] - mine['row_sum']) <= (M + 1) * 2.0 ** -53 * mine['row_sum'])
    assert not got['row_sum'][bad].any() and not got['row_n'][bad].any()
    # without the matrix: the same bytes, all together and one at a time
    rc, lean = call(ctx, xyz, bead, edges, outs=OUTS[1:])
    assert rc == 0 and all(lean[k].tobytes() == got[k].tobytes() for k in OUTS[1:])
    return got, want


@pytest.mark.parametrize('ncopy,S', [(3, 21), (2, 32), (1, 65), (1, 127), (2, 64), (3, 43)])
def test_tile_edges(ctx, ncopy, S):
    nlocus = {21: 9, 32: 17, 65: 8, 127: 3, 64: 16, 43: 40}[S]
    xyz, bead, planted = population(ncopy, S, nlocus, seed=S)
    got, _ = check(ctx, xyz, bead, label='tile edges')
    r, g = got['rmsd'], got['g']
    for name in ('duplicate', 'rigid'):
        a, b = planted[name]
        assert r[a, b] <= np.sqrt(1e-12 * (g[a] + g[b]) / nlocus), name
    a, b = planted['mirror']
    assert r[a, b] > 10.0 or nlocus <= 3                   # three points are their own mirror image
    a = planted['collapsed']
    assert g[a] == 0.0 and r[a, planted['collapsed2']] == 0.0
    others = np.isfinite(g) & (g > 0)
    # (0 + g_b - 0) / n exactly, then one float64 square root and the float32 rounding: one float32 ulp
    assert np.all(np.abs(r[a, others] - np.sqrt(g[others] / nlocus)) <= 2.0 ** -23 * r[a, others])


@pytest.mark.parametrize('ncopy,S', [(1, 1), (2, 1), (1, 2)])
def test_one_and_two_conformations(ctx, ncopy, S):
    xyz, bead, _ = population(ncopy, S, 11, seed=5)
    got, _ = check(ctx, xyz, bead, label='tiny')
    if ncopy * S == 1:
        assert got['row_n'].tolist() == [0] and got['row_sum'].tolist() == [0.0] and got['rmsd'].tolist() == [[0.0]]
        assert not got['hist'].any() and got['same'].tolist() == [[[0.0]]]
    else:
        assert got['row_n'].tolist() == [1, 1] and got['row_sum'].tolist() == [float(got['rmsd'][0, 1])] * 2
        assert got['hist'].sum() == 1


@pytest.mark.parametrize('nlocus', [1, 2, 3, 7, 8, 9, 15, 16, 17])
def test_locus_counts(ctx, nlocus):
    xyz, bead, _ = population(2, 35, nlocus, seed=nlocus)
    got, _ = check(ctx, xyz, bead, label='loci')
    if nlocus == 1:
        assert not got['g'][np.isfinite(got['g'])].any() and not got['rmsd'][np.isfinite(got['rmsd'])].any()


@pytest.mark.parametrize('nlocus', [2, 3, 4, 6, 7])
def test_small_chunk(ctx, nlocus, monkeypatch):
    xyz, bead, _ = population(2, 35, nlocus, seed=nlocus)
    _, full = call(ctx, xyz, bead)
    monkeypatch.setenv('IGM_CONFORMATION_CHUNK', '3')
    got, _ = check(ctx, xyz, bead, label='chunk 3')
    assert all(got[k].tobytes() == full[k].tobytes() for k in OUTS)     # the chunking does not reorder a sum


def test_largest_call(ctx):
    xyz, bead, planted = population(3, 130, 300, seed=0)
    got, want = check(ctx, xyz, bead, label='largest')
    a, b = planted['mirror']
    assert got['rmsd'][a, b] > 100.0
    assert np.max(got['hist']) > 0 and got['hist'].sum() < 390 * 389 // 2    # some pairs lie past the last edge


def test_values_on_histogram_edges(ctx):
    """two loci at (0, 0, 0) and (2 v, 0, 0) against a collapsed pair at the origin: g = 2 v^2
    exactly, the covariance is zero, and rmsd = sqrt(v^2) = v to the bit.  v is every edge and
    its float32 neighbours: the bins are [e_i, e_i+1), the last one closed, nothing outside."""
    edges = np.array([0.5, 1.0, 3.0, 50.0, 50.25], f32)
    vs = [f32(0.0)]
    for e in edges:
        vs += [np.nextafter(e, f32(-np.inf)), e, np.nextafter(e, f32(np.inf))]
    vs = np.array(vs, f32)
    n = len(vs) + 1                                        # conformation 0 is the collapsed pair
    xyz = np.zeros((2, n, 3), f32)                         # one copy, n structures, two beads
    xyz[1, 1:, 0] = 2 * vs
    bead = np.array([[0, 1]], np.int32)
    got, _ = check(ctx, xyz, bead, edges, label='edges')
    assert got['rmsd'][0, 1:].tobytes() == vs.tobytes()
    first = np.histogram(vs, bins=edges)[0]
    assert first.tolist() == [3, 3, 3, 4]                  # an edge opens its bin; both ends of the last bin count
    rc, alone = call(ctx, xyz[:, :2], bead, edges)          # the collapsed pair and v = 0 only: rmsd 0 < e_0
    assert rc == 0 and not alone['hist'].any() and alone['rmsd'].tolist() == [[0.0, 0.0], [0.0, 0.0]]
    rc, zero = call(ctx, xyz[:, :2], bead, np.array([0.0, 1.0], f32))
    assert rc == 0 and zero['hist'].tolist() == [1]


def test_refusals(ctx):
    xyz, bead, _ = population(2, 9, 5, seed=3, special=False)
    nbead = xyz.shape[0]
    inv, uns = _lib.IGM_E_INVALID, _lib.IGM_E_UNSUPPORTED
    check(ctx, xyz, bead)
    low, high = bead.copy(), bead.copy()
    low[1, 2] = -1
    high[0, 4] = nbead
    flat, down, nan_e = EDGES.copy(), EDGES.copy(), EDGES.copy()
    flat[4] = flat[3]
    down[7] = down[5]
    nan_e[-1] = np.nan
    many = np.arange(4098, dtype=f32)
    wide = np.zeros((2049, 1), np.int32)                   # 2049 copies x 512 structures > 2^20 conformations
    big = np.zeros((1, 512, 3), f32)
    cases = [(inv, dict(xyz=None)), (inv, dict(bead=None)), (inv, dict(nbead=0)), (inv, dict(nstruct=0)),
             (inv, dict(ncopy=0)), (inv, dict(nlocus=0)), (inv, dict(nbead=-4)), (inv, dict(nlocus=-1)),
             (inv, dict(bead=low.ctypes.data)), (inv, dict(bead=high.ctypes.data)),
             (inv, dict(edges=None)), (inv, dict(nedge=1)), (inv, dict(nedge=0)), (inv, dict(edges=flat.ctypes.data)),
             (inv, dict(edges=down.ctypes.data)), (inv, dict(edges=nan_e.ctypes.data)),
             (uns, dict(edges=many.ctypes.data, nedge=4098))]
    for code, kw in cases:
        rc, got = call(ctx, xyz, bead, over=kw)
        assert rc == code and ctx.lib.igm_last_error(ctx.h).decode().startswith('igm_report_conformations'), kw
        assert all(np.all(got[k] == FILL) for k in OUTS), kw
        check(ctx, xyz, bead)                              # usable and correct after every refusal
    rc, got = call(ctx, xyz, bead, outs=())
    assert rc == inv
    rc, got = call(ctx, big, wide, outs=('g', 'row_n'))
    assert rc == uns and np.all(got['g'] == FILL) and np.all(got['row_n'] == FILL)
    rc, got = call(ctx, xyz, bead, edges=None, outs=OUTS[:5])     # no histogram: no edges needed
    assert rc == 0 and got['hist'] is None
    check(ctx, xyz, bead)


def test_device_pointers(ctx):
    """IGM_DEVICE_PTRS: xyz and rmsd are device memory, everything else stays on the host"""
    import torch
    xyz, bead, _ = population(2, 70, 12, seed=8)
    _, host = call(ctx, xyz, bead)
    nbead, S = xyz.shape[:2]
    M = 2 * S
    dx = torch.from_numpy(xyz).cuda()
    for with_matrix in (True, False):
        for _ in range(2):
            dr = torch.full((M, M), float(FILL), dtype=torch.float32, device='cuda') if with_matrix else None
            o = {k: np.full(host[k].shape, FILL, DTYPE[k]) for k in OUTS[1:]}
            ctx.check(ctx.lib.igm_report_conformations(ctx.h, _lib.IGM_DEVICE_PTRS, dx.data_ptr(), nbead, S,
                                                       bead.ctypes.data, 2, 12, EDGES.ctypes.data, len(EDGES),
                                                       None if dr is None else dr.data_ptr(),
                                                       *(o[k].ctypes.data for k in OUTS[1:])),
                      'igm_report_conformations')
            if with_matrix:
                assert dr.cpu().numpy().tobytes() == host['rmsd'].tobytes()
            for k in OUTS[1:]:
                assert o[k].tobytes() == host[k].tobytes(), k
    assert ctx.kernel_ms('report_conformations') > 0


# ------------------------------------------------------------------ the Python layer and the report step
def test_python_functions(ctx):
    xyz, bead, _ = population(2, 33, 10, seed=4)
    res = RP.conformation_rmsd(xyz, bead, EDGES, ctx=ctx)
    _, raw = call(ctx, xyz, bead)
    assert all(res[k].tobytes() == raw[k].tobytes() for k in OUTS) and res['nlocus'] == 10
    lean = RP.conformation_rmsd(xyz, bead, want_matrix=False, ctx=ctx)
    assert lean['rmsd'] is None and lean['hist'] is None and lean['row_sum'].tobytes() == raw['row_sum'].tobytes()
    sm = RP.conformation_summary(lean, 33)
    ref = C.summary(raw['rmsd'], raw['g'], 33, 10)
    assert sm['medoid'] == ref['medoid']
    for k in ('mean', 'mean_rg', 'variability', 'medoid_mean_rmsd', 'same_mean', 'different_mean', 'ratio'):
        assert sm[k] == pytest.approx(ref[k], rel=1e-12), k
    assert np.allclose(sm['mean_rmsd'], ref['mean_rmsd'], rtol=1e-12, atol=0, equal_nan=True)
    with pytest.raises(ValueError):
        RP.conformation_rmsd(xyz, bead[0], ctx=ctx)
    with pytest.raises(RuntimeError, match='outside'):
        RP.conformation_rmsd(xyz, bead + 1000, ctx=ctx)


def test_report_step(ctx, tmp_path):
    """a small population without an .hss behind it: chromosome 0 in two copies (9 loci),
    chromosome 1 in one (5 loci), 7 structures; every file against the restatement"""
    from igm_amd.steps import PopulationStore
    n0, n1, S = 9, 5, 7
    chrom = np.array([0] * n0 + [1] * n1 + [0] * n0, np.int32)
    copy = np.array([0] * (n0 + n1) + [1] * n0, np.int32)
    cp = np.concatenate([np.arange(0, 2 * n0 + 1, 2), 2 * n0 + 1 + np.arange(n1)]).astype(np.int32)
    ci = np.concatenate([np.stack([np.arange(n0), n0 + n1 + np.arange(n0)], axis=1).ravel(),
                         n0 + np.arange(n1)]).astype(np.int32)
    rng = np.random.default_rng(12)
    xyz = np.cumsum(rng.normal(0, 80.0, (len(chrom), S, 3)), axis=0).astype(f32)
    p = str(tmp_path / 'small')
    PopulationStore.create(p, xyz, np.full(len(chrom), 10.0, f32), chrom, copy, cp, ci)
    out = tmp_path / 'qc'
    edges = RP.rmsd_edges_of(600.0, 12)
    RP.report_population(p, steps='conformations', out_dir=str(out), label='run', save_rmsd=True, rmsd_edges=edges,
                         ctx=ctx)
    made = sorted(str(f.relative_to(out)) for f in out.rglob('*') if f.is_file())
    assert made == ['conformations/0_mean_rmsd-run.txt', 'conformations/0_rmsd-run.npy',
                    'conformations/1_mean_rmsd-run.txt', 'conformations/1_rmsd-run.npy',
                    'conformations/histogram-run.txt', 'conformations/summary-run.txt', 'label.txt']
    assert np.array_equal(edges, np.linspace(0, 600, 13).astype(f32))
    rows = np.loadtxt(out / 'conformations/summary-run.txt')
    hist = np.loadtxt(out / 'conformations/histogram-run.txt')
    assert rows.shape == (2, 13) and hist.shape == (12, 4)
    assert np.array_equal(hist[:, 0], edges[:-1]) and np.array_equal(hist[:, 1], edges[1:])
    for j, (cid, nlocus, ncopy) in enumerate(((0, n0, 2), (1, n1, 1))):
        bead = RP.conformation_beads(chrom, copy, cp, ci, cid)
        assert bead.shape == (ncopy, nlocus)
        want = C.conformations(xyz, bead, edges)
        r = np.load(out / ('conformations/%d_rmsd-run.npy' % cid))
        assert r.dtype == f32 and np.all(np.abs(r - want['rmsd']) <= C.bound(want['rmsd'], want['g'], nlocus))
        ref = C.summary(r, want['g'], S, nlocus)
        assert rows[j, :4].tolist() == [cid, nlocus, ncopy, ncopy * S]
        assert rows[j, 7:9].tolist() == list(ref['medoid'])
        got = rows[j, [4, 5, 6, 9, 10, 11, 12]]
        exp = np.array([ref[k] for k in ('mean', 'mean_rg', 'variability', 'medoid_mean_rmsd', 'same_mean',
                                         'different_mean', 'ratio')])
        assert np.allclose(got, exp, rtol=1e-12, atol=0, equal_nan=True) and np.isnan(got[4:]).all() == (ncopy == 1)
        assert np.allclose(np.loadtxt(out / ('conformations/%d_mean_rmsd-run.txt' % cid)), ref['mean_rmsd'],
                           rtol=1e-12, atol=0)
        assert np.array_equal(hist[:, 2 + j], C.reductions(r, S, edges)['hist'])
    # one chromosome, a domain of it, no matrix, no label, through report_population
    out = tmp_path / 'qc2'
    loci = np.zeros(n0 + n1, int)
    loci[2:6] = 1
    written = RP.report_population(p, steps='conformations', out_dir=str(out), conformation_chroms=[0],
                                   conformation_loci=loci, rmsd_edges=edges, ctx=ctx)
    assert sorted(written) == ['conformations/0_mean_rmsd.txt', 'conformations/histogram.txt',
                               'conformations/summary.txt', 'label.txt']
    row = np.loadtxt(out / 'conformations/summary.txt')
    bead = RP.conformation_beads(chrom, copy, cp, ci, 0, loci)
    want = C.conformations(xyz, bead, edges)
    ref = C.summary(want['rmsd'], want['g'], S, 4)
    assert row[:4].tolist() == [0, 4, 2, 14] and row[4] == pytest.approx(ref['mean'], rel=1e-5)
    assert np.loadtxt(out / 'conformations/histogram.txt')[:, 2].sum() == 14 * 13 // 2
