"""The seeded nuclear bodies (igm_report_seed_bodies, igm_report_body_features) and the
seeded_bodies report step on the MI355X, against the NumPy oracle tests/report_bodies_ref.py.

Every call is made twice and must return the same bytes; the outputs start from a fill that
no result equals, so an entry that was never written shows.  Labels, nbody, size, centre,
nearest, dist_sum, dist_sqsum and assoc are compared by equality (a NaN equals a NaN: the
payload of a NaN that arithmetic produced is the processor's).

tsa_sum carries a relative bar of 2 (K + S + 2) 2^-53 with K = nbody.max() and S = nstruct:
one ulp per exp on each side -- the bound both math libraries document for exp in double
precision -- and the rounding of each of the at most K + S positive additions on each side;
every term is positive, so the relative errors do not amplify.  decay * d stays below 700 in
the cases under this bar.  Where a body is so far away that decay * d > 746 its term is
exactly 0 on both sides; that case is built so that every other term is exactly 0 or 1 and
tsa_sum is compared by equality.

Shapes.  The component kernel runs one workgroup of 1024 threads (16 waves of 64) per
structure; its pair pass cuts the seeds into tiles of 256 rows (4 per lane) by 128 columns,
and its per-seed phases take 1024 seeds at a time: the seed counts below sit on both sides
of 64, 128, 256 and 1024, and the chains reach the 8192 that fit in LDS.  The feature kernel
owns 32 beads per workgroup and 8 per wave and walks the structures in chunks of 64."""
import itertools

import numpy as np
import pytest

import asteps_edges as E
import report_bodies_ref as B
from conftest import load_golden
from igm_amd import _lib, report as RP

pytestmark = pytest.mark.gpu

f32 = np.float32
BOUTS = ('label', 'nbody', 'size', 'centre')
FOUTS = ('nearest', 'dist_sum', 'dist_sqsum', 'assoc', 'tsa_sum')
FILL = {'label': -7, 'nbody': -7, 'size': -7, 'centre': -7.0, 'nearest': -7.0, 'dist_sum': -7.0, 'dist_sqsum': -7.0,
        'assoc': -7, 'tsa_sum': -7.0}
DTYPE = {'label': np.int32, 'nbody': np.int32, 'size': np.int32, 'centre': np.float64, 'nearest': np.float64,
         'dist_sum': np.float64, 'dist_sqsum': np.float64, 'assoc': np.int64, 'tsa_sum': np.float64}


@pytest.fixture(scope='module')
def ctx():
    return _lib.context(0)


def same_twice(runs, names):
    assert runs[0][0] == runs[1][0]
    for k in names:
        a, b = runs[0][1][k], runs[1][1][k]
        assert (a is None and b is None) or a.tobytes() == b.tobytes(), 'rerun differs in %s' % k
    return runs[0]


def bodies(ctx, xyz, seeds, cutoff=500.0, min_size=3, max_bodies=None, outs=BOUTS):
    """igm_report_seed_bodies on host arrays, twice: (rc, {name: array or None})"""
    xyz = np.ascontiguousarray(xyz, f32)
    nbead, S = xyz.shape[:2]
    seeds = np.ascontiguousarray(seeds, np.int32)
    n = len(seeds)
    if max_bodies is None:
        max_bodies = max(n // min_size, 1) if min_size >= 1 else 1
    room = max(max_bodies, 0)
    shape = {'label': (S, n), 'nbody': (S,), 'size': (S, room), 'centre': (S, room, 3)}
    runs = []
    for _ in range(2):
        o = {k: np.full(shape[k], FILL[k], DTYPE[k]) if k in outs else None for k in BOUTS}
        rc = ctx.lib.igm_report_seed_bodies(ctx.h, 0, xyz.ctypes.data, nbead, S, seeds.ctypes.data, n, cutoff, min_size,
                                            max_bodies, *(_lib.ptr(o[k]) for k in BOUTS))
        runs.append((rc, o))
    return same_twice(runs, BOUTS)


def equal(got, want):
    return (got.dtype == want.dtype and got.shape == want.shape
            and np.array_equal(got, want, equal_nan=got.dtype.kind == 'f'))


def check_bodies(ctx, xyz, seeds, cutoff=500.0, min_size=3, want=None):
    """all four outputs equal the oracle's; returns them"""
    rc, got = bodies(ctx, xyz, seeds, cutoff, min_size)
    assert rc == 0, ctx.lib.igm_last_error(ctx.h).decode()
    if want is None:
        want = B.seed_bodies(xyz, seeds, cutoff, min_size, max_bodies=got['size'].shape[1])
    for k in BOUTS:
        assert equal(got[k], want[k]), k
    return got


def features(ctx, xyz, nbody, centre, assoc_cutoff=500.0, decay=0.004, outs=FOUTS):
    """igm_report_body_features on host arrays, twice: (rc, {name: array or None})"""
    xyz = np.ascontiguousarray(xyz, f32)
    n, S = xyz.shape[:2]
    nbody = np.ascontiguousarray(nbody, np.int32)
    centre = np.ascontiguousarray(centre, np.float64)
    shape = {'nearest': (n, S)}
    runs = []
    for _ in range(2):
        o = {k: np.full(shape.get(k, (n,)), FILL[k], DTYPE[k]) if k in outs else None for k in FOUTS}
        rc = ctx.lib.igm_report_body_features(ctx.h, 0, xyz.ctypes.data, n, S, nbody.ctypes.data, centre.ctypes.data,
                                              centre.shape[1], assoc_cutoff, decay, *(_lib.ptr(o[k]) for k in FOUTS))
        runs.append((rc, o))
    return same_twice(runs, FOUTS)


def tsa_bar(want, nbody):
    return 2.0 * (int(np.max(nbody)) + len(nbody) + 2) * 2.0 ** -53 * np.abs(want)


def check_features(ctx, xyz, nbody, centre, assoc_cutoff=500.0, decay=0.004, exact_tsa=False, in_reach=True):
    xyz, centre = np.asarray(xyz, f32), np.asarray(centre, np.float64)
    rc, got = features(ctx, xyz, nbody, centre, assoc_cutoff, decay)
    assert rc == 0, ctx.lib.igm_last_error(ctx.h).decode()
    want = B.body_features(xyz, nbody, centre, assoc_cutoff, decay)
    for k in FOUTS[:4]:
        assert equal(got[k], want[k]), k
    g, w = got['tsa_sum'], want['tsa_sum']
    assert np.array_equal(np.isnan(g), np.isnan(w))
    ok = ~np.isnan(w)
    print('tsa_sum: largest relative difference %.3g, bar %.3g'
          % (np.max(np.abs(g[ok] - w[ok]) / np.maximum(w[ok], 1e-300), initial=0.0),
             2.0 * (int(np.max(nbody)) + len(nbody) + 2) * 2.0 ** -53))
    if exact_tsa:
        assert np.array_equal(g[ok], w[ok])
    else:
        if in_reach:  # decay * d <= 700 for every bead and body: sqrt(3) (max |x| + max |c|) bounds d
            fx, fc = np.abs(xyz[np.isfinite(xyz)]).astype(np.float64), np.abs(centre[np.isfinite(centre)])
            assert decay * np.sqrt(3.0) * (fx.max(initial=0.0) + fc.max(initial=0.0)) <= 700.0
        assert np.all(np.abs(g[ok] - w[ok]) <= tsa_bar(w[ok], nbody))
    return got


def gas(n, S, seed, z=2.5, r=500.0):
    """n seeds among n + n // 2 + 3 beads thrown into a box in which a seed has z others
    within r on average: just below the percolation of the link graph, so components of
    every size occur.  Returns xyz and the ascending seed indices."""
    rng = np.random.default_rng(seed)
    nbead = n + n // 2 + 3
    side = (n * 4.0 / 3.0 * np.pi * r ** 3 / z) ** (1.0 / 3.0)
    xyz = rng.uniform(0.0, side, (nbead, S, 3)).astype(f32)
    return xyz, np.sort(rng.choice(nbead, n, replace=False)).astype(np.int32)


# ------------------------------------------------------------------ shapes
NSEED = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513, 1023, 1024, 1025)
NSTRUCT = (1, 2, 63, 64, 65, 130)
NBEAD = (1, 9, 31, 32, 33, 65, 257)


@pytest.mark.parametrize('n', NSEED)
def test_seed_counts(ctx, n):
    xyz, seeds = gas(n, 3, n)
    got = check_bodies(ctx, xyz, seeds)
    if n >= 257:  # the gas has a big component and singletons in every structure
        for lab in got['label']:
            sizes = B.component_sizes(lab)
            assert sizes.max() >= 10 and np.count_nonzero(sizes == 1) >= 10
    check_bodies(ctx, xyz, seeds, min_size=1)


@pytest.mark.parametrize('S', NSTRUCT)
def test_structure_counts(ctx, S):
    xyz, seeds = gas(65, S, 900 + S)
    got = check_bodies(ctx, xyz, seeds, min_size=2)
    assert got['nbody'].min() >= 1 and ctx.kernel_ms('report_seed_bodies') > 0


def random_bodies(S, K, seed, scale=3000.0):
    """nbody dealt over [0, K] with both ends present where S allows, centres of the beads' scale"""
    rng = np.random.default_rng(seed)
    nbody = rng.integers(0, K + 1, S).astype(np.int32)
    nbody[rng.integers(0, S)] = K
    if S > 1:
        nbody[(int(np.argmax(nbody == K)) + 1) % S] = 0
    centre = rng.uniform(-scale, scale, (S, K, 3))
    centre[np.arange(K)[None, :] >= nbody[:, None]] = np.nan   # never read
    return nbody, centre


@pytest.mark.parametrize('n,S', list(itertools.product(NBEAD, NSTRUCT)))
def test_feature_shapes(ctx, n, S):
    rng = np.random.default_rng(77 * n + S)
    xyz = rng.uniform(-3000.0, 3000.0, (n, S, 3)).astype(f32)
    nbody, centre = random_bodies(S, 5, n + 1000 * S)
    got = check_features(ctx, xyz, nbody, centre, assoc_cutoff=1500.0)
    if n * S >= 64:
        assert 0 < got['assoc'].sum() < n * np.count_nonzero(nbody)
    assert ctx.kernel_ms('report_body_features') > 0


def test_bodies_then_features(ctx):
    """the two calls chained, as the report step chains them"""
    xyz, seeds = gas(257, 67, 4)
    got = check_bodies(ctx, xyz, seeds)
    K = int(got['nbody'].max())
    check_features(ctx, xyz, got['nbody'], got['centre'][:, :K])
    check_features(ctx, xyz, got['nbody'], got['centre'])          # a wider max_bodies changes nothing


# ------------------------------------------------------------------ chains
def chain(n, gap, seed, cutoff=500.0):
    """A zigzag chain of n seeds in two halves: consecutive seeds are 0.994 cutoff apart in
    the xy plane (seeds two apart 1.6 cutoff), and the second half lies above the first by
    `gap` along z, its first seed straight above the last of the first half -- that one
    link is exactly `gap` long.  The ranks are dealt at random along the chain.  Returns xyz
    (n, 1, 3), and the position along the chain of every rank."""
    m = n // 2
    k = np.arange(n)
    j = np.where(k < m, k, k - 1)
    pts = np.stack([j * (0.8 * cutoff), (j % 2) * (0.59 * cutoff), np.where(k < m, 0.0, np.float64(gap))], axis=1)
    pos = np.random.default_rng(seed).permutation(n)
    return pts[pos].astype(f32)[:, None, :], pos


def centre_of(xyz, members):
    acc = np.zeros(3, np.float64)
    for m in members:                                     # ascending rank
        acc = acc + xyz[m, 0].astype(np.float64)
    return acc / np.float64(len(members))


@pytest.mark.parametrize('n', [4096, 8192])
def test_chain_is_one_body(ctx, n):
    """diameter n - 1: one body with label 0, whatever the order of the hooks"""
    xyz, _ = chain(n, f32(500.0), n)
    rc, got = bodies(ctx, xyz, np.arange(n), min_size=n)
    assert rc == 0 and got['nbody'].tolist() == [1] and got['size'].tolist() == [[n]]
    assert not got['label'].any()
    assert np.array_equal(got['centre'][0, 0], centre_of(xyz, range(n)))
    if n == 4096:
        want = B.seed_bodies(xyz, np.arange(n), 500.0, n, max_bodies=1)
        assert all(equal(got[k], want[k]) for k in BOUTS)


@pytest.mark.parametrize('n', [4096, 8192])
def test_chain_cut_by_one_ulp(ctx, n):
    """the middle link one float32 ulp past the cutoff: two bodies, labelled by their smallest ranks"""
    xyz, pos = chain(n, np.nextafter(f32(500.0), f32(np.inf)), n)
    rc, got = bodies(ctx, xyz, np.arange(n), min_size=2)
    assert rc == 0 and got['nbody'].tolist() == [2]
    first = pos < n // 2                                  # per rank: in the first half of the chain
    la, lb = int(np.argmax(first)), int(np.argmax(~first))
    assert np.array_equal(got['label'][0], np.where(first, la, lb))
    order = [first, ~first] if la < lb else [~first, first]
    assert got['size'][0, :2].tolist() == [int(o.sum()) for o in order] and not got['size'][0, 2:].any()
    for k, o in enumerate(order):
        assert np.array_equal(got['centre'][0, k], centre_of(xyz, np.nonzero(o)[0]))
    assert np.isnan(got['centre'][0, 2:]).all()


@pytest.mark.parametrize('kind', ['coincident', 'apart'])
def test_all_or_nothing(ctx, kind):
    """8192 seeds that are all linked to one another, and 8192 without any link"""
    n = 8192
    xyz = np.zeros((n, 1, 3), f32)
    if kind == 'coincident':
        xyz[:] = (3.5, -2.25, 7.0)
        for cutoff in (0.0, 500.0):
            rc, got = bodies(ctx, xyz, np.arange(n), cutoff, min_size=1)
            assert rc == 0 and got['nbody'].tolist() == [1] and got['size'][0, 0] == n and not got['label'].any()
            assert got['centre'][0, 0].tolist() == [3.5, -2.25, 7.0]
            assert not got['size'][0, 1:].any() and np.isnan(got['centre'][0, 1:]).all()
        return
    xyz[:, 0, 0] = np.arange(n) * 501.0
    xyz[:, 0, 1] = np.arange(n) % 7
    rc, got = bodies(ctx, xyz, np.arange(n), min_size=1)
    assert rc == 0 and got['nbody'].tolist() == [n] and np.all(got['size'] == 1)
    assert np.array_equal(got['label'][0], np.arange(n))
    assert np.array_equal(got['centre'][0], xyz[:, 0].astype(np.float64))
    rc, got = bodies(ctx, xyz, np.arange(n), min_size=2)
    assert rc == 0 and got['nbody'].tolist() == [0] and not got['size'].any() and np.isnan(got['centre']).all()


# ------------------------------------------------------------------ the link test at its edges
@pytest.mark.parametrize('cutoff', [500.0, 0.1, 3.0, 2.0 ** -60, 1e15])
def test_near_ties(ctx, cutoff):
    """two seeds at the cutoff moved by -2 .. 2 ulp, on the axes and along the oblique directions"""
    cut = f32(cutoff)
    dirs = [np.eye(3)[a] * sgn for a in range(3) for sgn in (1.0, -1.0)] + list(E.TIE_DIRS)
    xyz = np.zeros((2, len(dirs) * len(E.TIE_K), 3), f32)
    for q, d in enumerate(dirs):
        for k in E.TIE_K:
            xyz[1, len(E.TIE_K) * q + k + 2] = (np.float64(E.ulps(cut, k)) * d).astype(f32)
    got = check_bodies(ctx, xyz, [0, 1], float(cut), min_size=2)
    assert got['nbody'][:30].tolist() == [1, 1, 1, 0, 0] * 6      # the six axis directions are exact


@pytest.mark.parametrize('cr,offaxis', list(itertools.product(E.TIE_CRS, (False, True))))
def test_near_tie_population(ctx, cr, offaxis):
    """asteps_edges.near_tie_case: every pair of twelve seeds within 2 ulp of its own bound in
    five structures; at that pair's bound as the cutoff those five decide on the last bit"""
    xyz, radii = E.near_tie_case(cr, offaxis)
    for p in (0, 7, 23, 40, 65):
        i, j = E.TIE_PAIRS[p]
        cut = float(E.threshold(radii[i], radii[j], cr))
        got = check_bodies(ctx, xyz, np.arange(12), cut, min_size=2)
        if not offaxis:
            assert got['nbody'][5 * p:5 * p + 5].tolist() == [1, 1, 1, 0, 0]


@pytest.mark.parametrize('kind', ['overflow', 'big_threshold', 'nonfinite', 'tiny_radii'])
def test_ends_of_float32(ctx, kind):
    """squared norms that overflow or vanish, a cutoff whose square does, NaN and +-inf seeds"""
    xyz, _, _ = E.extreme_case(kind)
    for cutoff in (0.0, 1e-30, 100.0, 4e20, float(np.finfo(f32).max)):
        got = check_bodies(ctx, xyz, np.arange(10), cutoff, min_size=1)
        check_bodies(ctx, xyz, np.array([1, 2, 5, 6, 7, 9]), cutoff, min_size=2)
    if kind == 'nonfinite':  # seed 5 has a NaN in every fourth structure: alone there, at any cutoff
        s = np.arange(40) % 4 == 0
        assert np.all(got['label'][s, 5] == 5) and np.all(got['label'][~s, 5] == 0)


def test_cutoff_zero(ctx):
    """only coincident seeds are linked: lattice seeds that coincide in some structures"""
    xyz, _ = E.zero_threshold_case()
    got = check_bodies(ctx, xyz, np.arange(12), 0.0, min_size=2)
    assert 0 < got['nbody'].sum() and np.any(got['label'] == np.arange(12))


# ------------------------------------------------------------------ min_size and the order of the bodies
def clusters(sizes, S, seed, shuffle=True):
    """tight clusters (spread 10) of the given sizes, 10000 apart, the ranks shuffled
    differently in every structure; returns xyz (n, S, 3) and cluster_of[s][rank]"""
    rng = np.random.default_rng(seed)
    which = np.repeat(np.arange(len(sizes)), sizes)
    xyz = np.empty((len(which), S, 3), f32)
    cluster_of = np.empty((S, len(which)), np.int64)
    for s in range(S):
        w = rng.permutation(which) if shuffle else which
        cluster_of[s] = w
        xyz[:, s] = (w[:, None] * 10000.0 + rng.uniform(0.0, 10.0, (len(w), 3))).astype(f32)
    return xyz, cluster_of


@pytest.mark.parametrize('min_size', [1, 2, 3, 4, 5, 6, 7])
def test_min_size(ctx, min_size):
    """components of 1 .. 6 seeds: those of exactly min_size - 1 are dropped, those of min_size kept"""
    sizes = [1, 2, 3, 4, 5, 6, 1, 3, 5]
    xyz, _ = clusters(sizes, 5, min_size)
    got = check_bodies(ctx, xyz, np.arange(sum(sizes)), 100.0, min_size)
    kept = sorted(v for v in sizes if v >= min_size)
    assert np.all(got['nbody'] == len(kept))
    for s in range(5):
        assert sorted(got['size'][s, :len(kept)].tolist()) == kept


def test_bodies_come_out_in_label_order(ctx):
    sizes = [4, 3, 9, 3, 5, 1, 2, 6]
    xyz, cluster_of = clusters(sizes, 9, 3)
    got = check_bodies(ctx, xyz, np.arange(sum(sizes)), 100.0, 3)
    orders = set()
    for s in range(9):
        first = [int(np.argmax(cluster_of[s] == c)) for c in range(len(sizes))]     # the label of cluster c
        assert np.array_equal(got['label'][s], np.array(first)[cluster_of[s]])
        kept = sorted((first[c], sizes[c]) for c in range(len(sizes)) if sizes[c] >= 3)
        assert got['size'][s, :len(kept)].tolist() == [v for _, v in kept]
        orders.add(tuple(v for _, v in kept))
    assert len(orders) > 1                                # the shuffles put the bodies in different orders


# ------------------------------------------------------------------ capacity
def test_overflow_returns_the_true_counts(ctx):
    xyz, seeds = gas(257, 5, 11)
    rc, full = bodies(ctx, xyz, seeds)
    assert rc == 0
    most = int(full['nbody'].max())
    assert most >= 2 and full['nbody'].min() < most
    rc, got = bodies(ctx, xyz, seeds, max_bodies=most - 1)
    assert rc == _lib.IGM_E_OVERFLOW and 'max_bodies' in ctx.lib.igm_last_error(ctx.h).decode()
    assert np.array_equal(got['nbody'], full['nbody'])
    for k in ('label', 'size', 'centre'):
        assert np.all(got[k] == FILL[k]), k
    rc, got = bodies(ctx, xyz, seeds, max_bodies=most)            # exactly enough
    assert rc == 0 and np.array_equal(got['size'], full['size'][:, :most])
    assert equal(got['centre'], full['centre'][:, :most])
    rc, got = bodies(ctx, xyz, seeds, max_bodies=0, outs=('label', 'nbody'))   # counts and labels need no room
    assert rc == _lib.IGM_E_OVERFLOW and np.array_equal(got['nbody'], full['nbody']) and np.all(got['label'] == -7)


def test_seed_capacity(ctx):
    """8193 seeds are refused, 8192 run"""
    xyz = np.zeros((8193, 1, 3), f32)
    xyz[:, 0, 2] = np.arange(8193) * 300.0                # a straight chain at cutoff 500
    rc, got = bodies(ctx, xyz, np.arange(8193))
    assert rc == _lib.IGM_E_UNSUPPORTED and '8192' in ctx.lib.igm_last_error(ctx.h).decode()
    for k in BOUTS:
        assert np.all(got[k] == FILL[k]), k
    rc, got = bodies(ctx, xyz, np.arange(8192))
    assert rc == 0 and got['nbody'].tolist() == [1] and got['size'][0, 0] == 8192 and not got['label'].any()


# ------------------------------------------------------------------ the features at their edges
def test_crafted_centres(ctx):
    """a bead at the same distance from two bodies, a bead on a centre, a bead at the
    association cutoff +-1 ulp, a NaN and an inf bead.  Bead 5 is 1e30 away from everything:
    decay * d is about 7e27, far past 746, and each of its terms is exactly 0 on both sides."""
    S = 4
    centre = np.zeros((S, 3, 3))
    centre[:, 0] = (0.0, 0.0, 0.0)
    centre[:, 1] = (6.0, 8.0, 0.0)
    centre[:, 2] = (0.0, 0.0, 500.0)
    nbody = np.array([3, 2, 0, 1], np.int32)
    xyz = np.zeros((6, S, 3), f32)
    xyz[0] = (3.0, 4.0, 0.0)                              # 5 from body 0 and from body 1
    xyz[1] = (6.0, 8.0, 0.0)                              # on body 1, 10 from body 0
    xyz[2] = (0.0, -500.0, 0.0)                           # exactly 500 from body 0
    xyz[3] = (np.nan, 1.0, 1.0)
    xyz[4, ::2] = (np.inf, 0.0, 0.0)
    xyz[5] = (1e30, -1e30, 1e30)                          # finite, the float64 norm is too
    up, down = np.nextafter(500.0, np.inf), np.nextafter(500.0, 0.0)
    for cutoff, hits in ((500.0, 3), (up, 3), (down, 0)):
        got = check_features(ctx, xyz, nbody, centre, cutoff, decay=0.004 if cutoff == 500.0 else 0.0, in_reach=False)
        assert got['assoc'][2] == hits
        assert got['nearest'][0].tolist()[:2] == [5.0, 5.0] and got['nearest'][1].tolist()[:2] == [0.0, 0.0]
        assert got['nearest'][1, 3] == 10.0 and np.isnan(got['nearest'][:, 2]).all()
        assert np.isnan(got['dist_sum'][3]) and np.isnan(got['tsa_sum'][3]) and got['assoc'][3] == 0
        assert np.isnan(got['dist_sum'][4]) and got['assoc'][4] == 2   # on body 0 in structures 1 and 3, inf in 0
    assert got['tsa_sum'][:3].tolist() == [6.0, 6.0, 6.0]             # decay 0: the body count


def test_structures_without_bodies(ctx):
    """structures with and without bodies interleaved across the 64-structure chunk edges"""
    rng = np.random.default_rng(5)
    S, n = 130, 37
    xyz = rng.uniform(-2000.0, 2000.0, (n, S, 3)).astype(f32)
    for pattern in (np.arange(S) % 2, (np.arange(S) + 1) % 2, (np.arange(S) >= 63) & (np.arange(S) < 65),
                    (np.arange(S) < 63) | (np.arange(S) >= 65), np.zeros(S), np.arange(S) == 129):
        nbody = np.asarray(pattern, np.int32) * 3
        centre = rng.uniform(-2000.0, 2000.0, (S, 3, 3))
        got = check_features(ctx, xyz, nbody, centre, assoc_cutoff=1500.0)
        assert np.array_equal(np.isnan(got['nearest']).all(axis=0), nbody == 0)
        if not nbody.any():
            assert not got['dist_sum'].any() and not got['tsa_sum'].any() and not got['assoc'].any()


def test_every_lane_its_own_body_count(ctx):
    """nbody differs in every lane of a wave, 0 and max_bodies included; at decay 0 t(p, s)
    is the body count exactly"""
    rng = np.random.default_rng(6)
    S, n, K = 70, 20, 63
    nbody = ((np.arange(S) * 37) % 64).astype(np.int32)       # a permutation of 0 .. 63 in the first wave
    assert sorted(nbody[:64].tolist()) == list(range(64))
    xyz = rng.uniform(-2000.0, 2000.0, (n, S, 3)).astype(f32)
    centre = rng.uniform(-2000.0, 2000.0, (S, K, 3))
    check_features(ctx, xyz, nbody, centre, assoc_cutoff=300.0)
    got = check_features(ctx, xyz, nbody, centre, assoc_cutoff=300.0, decay=0.0, exact_tsa=True)
    assert np.all(got['tsa_sum'] == nbody.sum())


def test_a_body_out_of_reach_adds_exactly_nothing(ctx):
    """decay * d > 746 underflows exp to 0 on both sides.  Every other term is exactly 1 (a
    bead on the near centre) or exactly 0 (a bead 1e6 away from it too), so tsa_sum is
    compared by equality; on random beads the sums with and without the far body must be
    the same bytes."""
    rng = np.random.default_rng(8)
    S, n = 67, 21
    near = rng.uniform(-2000.0, 2000.0, (S, 3)).astype(f32).astype(np.float64)
    centre = np.stack([near, near + (0.0, 1e6, 0.0)], axis=1)
    nbody = np.full(S, 2, np.int32)
    on = rng.random((n, S)) < 0.5
    xyz = np.where(on[..., None], near[None].astype(f32), (near[None] - (1e6, 0.0, 0.0)).astype(f32))
    got = check_features(ctx, xyz, nbody, centre, decay=0.004, exact_tsa=True)
    assert np.array_equal(got['tsa_sum'], on.sum(axis=1).astype(np.float64)) and got['tsa_sum'].any()
    xyz = (near[None] + rng.uniform(-800.0, 800.0, (n, S, 3))).astype(f32)
    _, both = features(ctx, xyz, nbody, centre, decay=0.004)
    _, alone = features(ctx, xyz, np.ones(S, np.int32), centre, decay=0.004)
    assert both['tsa_sum'].tobytes() == alone['tsa_sum'].tobytes() and np.all(both['tsa_sum'] > 0)


# ------------------------------------------------------------------ the interface
def test_every_null_combination(ctx):
    xyz, seeds = gas(70, 66, 8)
    _, full = bodies(ctx, xyz, seeds)
    for r in range(0, 4):
        for extra in itertools.combinations(('label', 'size', 'centre'), r):
            outs = ('nbody',) + extra
            rc, got = bodies(ctx, xyz, seeds, outs=outs)
            assert rc == 0, outs
            for k in BOUTS:
                assert (got[k] is None) if k not in outs else equal(got[k], full[k]), (outs, k)
    K = int(full['nbody'].max())
    _, feat = features(ctx, xyz, full['nbody'], full['centre'][:, :K])
    for r in range(1, 5):
        for outs in itertools.combinations(FOUTS, r):
            rc, got = features(ctx, xyz, full['nbody'], full['centre'][:, :K], outs=outs)
            assert rc == 0, outs
            for k in FOUTS:
                assert (got[k] is None) if k not in outs else got[k].tobytes() == feat[k].tobytes(), (outs, k)


def test_seed_bodies_refusals(ctx):
    xyz, seeds = gas(20, 3, 9)
    nbead = xyz.shape[0]
    inv = _lib.IGM_E_INVALID
    dup, swapped, low, high = seeds.copy(), seeds.copy(), seeds.copy(), seeds.copy()
    dup[5] = dup[4]
    swapped[[3, 4]] = swapped[[4, 3]]
    low[0] = -1
    high[-1] = nbead
    bad = [dict(seeds=dup), dict(seeds=swapped), dict(seeds=low), dict(seeds=high),
           dict(cutoff=-1.0), dict(cutoff=float('nan')), dict(cutoff=float('inf')),
           dict(min_size=0), dict(min_size=-3), dict(max_bodies=-1), dict(max_bodies=0),
           dict(max_bodies=0, outs=('nbody', 'size')), dict(max_bodies=0, outs=('nbody', 'centre'))]
    for kw in bad:
        kw = dict(kw)
        rc, got = bodies(ctx, xyz, kw.pop('seeds', seeds), **kw)
        assert rc == inv and ctx.lib.igm_last_error(ctx.h).decode().startswith('igm_report_seed_bodies'), kw
        for k in BOUTS:
            assert got[k] is None or np.all(got[k] == FILL[k]), kw
        check_bodies(ctx, xyz, seeds)                              # usable after every refusal
    nb = np.full(3, -7, np.int32)
    args = [ctx.h, 0, xyz.ctypes.data, nbead, 3, seeds.ctypes.data, 20, 500.0, 3, 6, None, nb.ctypes.data, None, None]

    def with_(i, v):
        a = list(args)
        a[i] = v
        return ctx.lib.igm_report_seed_bodies(*a)

    for i, v in ((2, None), (5, None), (11, None), (3, 0), (4, 0), (6, 0), (3, -1)):
        assert with_(i, v) == inv, i
    assert np.all(nb == -7)
    assert ctx.lib.igm_report_seed_bodies(*args) == 0 and np.all(nb >= 0)


def test_body_features_refusals(ctx):
    rng = np.random.default_rng(10)
    xyz = rng.uniform(-2000.0, 2000.0, (20, 3, 3)).astype(f32)
    nbody, centre = np.array([2, 0, 1], np.int32), rng.uniform(-2000.0, 2000.0, (3, 2, 3))
    centre[1] = np.nan                                             # unread: structure 1 has no body
    centre[2, 1] = np.inf                                          # unread too
    check_features(ctx, xyz, nbody, centre)
    inv = _lib.IGM_E_INVALID
    nan_c, inf_c = centre.copy(), centre.copy()
    nan_c[0, 1, 2] = np.nan
    inf_c[2, 0, 0] = -np.inf
    bad = [dict(outs=()), dict(nbody=np.array([2, 0, 3], np.int32)), dict(nbody=np.array([2, -1, 1], np.int32)),
           dict(centre=nan_c), dict(centre=inf_c),
           dict(assoc_cutoff=-1.0), dict(assoc_cutoff=float('nan')), dict(assoc_cutoff=float('inf')),
           dict(decay=-0.5), dict(decay=float('nan')), dict(decay=float('inf'))]
    for kw in bad:
        kw = dict(kw)
        rc, got = features(ctx, xyz, kw.pop('nbody', nbody), kw.pop('centre', centre), **kw)
        assert rc == inv and ctx.lib.igm_last_error(ctx.h).decode().startswith('igm_report_body_features'), kw
        for k in FOUTS:
            assert got[k] is None or np.all(got[k] == FILL[k]), kw
        check_features(ctx, xyz, nbody, centre)                    # usable after every refusal
    ds = np.full(20, -7.0)
    args = [ctx.h, 0, xyz.ctypes.data, 20, 3, nbody.ctypes.data, centre.ctypes.data, 2, 500.0, 0.004, None,
            ds.ctypes.data, None, None, None]

    def with_(i, v):
        a = list(args)
        a[i] = v
        return ctx.lib.igm_report_body_features(*a)

    for i, v in ((2, None), (5, None), (6, None), (3, 0), (4, 0), (7, 0), (7, 1)):   # max_bodies 1 < nbody[0]
        assert with_(i, v) == inv, i
    assert np.all(ds == -7.0)
    assert ctx.lib.igm_report_body_features(*args) == 0 and np.all(ds >= 0)


def test_device_pointers(ctx):
    """IGM_DEVICE_PTRS: xyz and nearest are device memory, everything else stays on the host"""
    import torch
    xyz, seeds = gas(70, 66, 12)
    _, host = bodies(ctx, xyz, seeds)
    K = int(host['nbody'].max())
    centre = np.ascontiguousarray(host['centre'][:, :K])
    _, feat = features(ctx, xyz, host['nbody'], centre)
    nbead, S, n = xyz.shape[0], 66, 70
    dx = torch.from_numpy(xyz).cuda()
    F = _lib.IGM_DEVICE_PTRS
    for _ in range(2):
        o = {k: np.full(host[k].shape, FILL[k], DTYPE[k]) for k in BOUTS}
        ctx.check(ctx.lib.igm_report_seed_bodies(ctx.h, F, dx.data_ptr(), nbead, S, seeds.ctypes.data, n, 500.0, 3,
                                                 host['size'].shape[1], *(o[k].ctypes.data for k in BOUTS)),
                  'igm_report_seed_bodies')
        for k in BOUTS:
            assert o[k].tobytes() == host[k].tobytes(), k
    for with_nearest in (True, False):
        for _ in range(2):
            near = torch.full((nbead, S), -7.0, dtype=torch.float64, device='cuda') if with_nearest else None
            o = {k: np.full(nbead, FILL[k], DTYPE[k]) for k in FOUTS[1:]}
            ctx.check(ctx.lib.igm_report_body_features(ctx.h, F, dx.data_ptr(), nbead, S, host['nbody'].ctypes.data,
                                                       centre.ctypes.data, K, 500.0, 0.004,
                                                       None if near is None else near.data_ptr(),
                                                       *(o[k].ctypes.data for k in FOUTS[1:])),
                      'igm_report_body_features')
            if with_nearest:
                assert near.cpu().numpy().tobytes() == feat['nearest'].tobytes()
            for k in FOUTS[1:]:
                assert o[k].tobytes() == feat[k].tobytes(), k
    near = torch.full((nbead, S), -7.0, dtype=torch.float64, device='cuda')      # nearest alone
    ctx.check(ctx.lib.igm_report_body_features(ctx.h, F, dx.data_ptr(), nbead, S, host['nbody'].ctypes.data,
                                               centre.ctypes.data, K, 500.0, 0.004, near.data_ptr(), None, None, None,
                                               None), 'igm_report_body_features')
    assert near.cpu().numpy().tobytes() == feat['nearest'].tobytes()


# ------------------------------------------------------------------ the Python layer and the report step
def test_python_functions(ctx):
    xyz, seeds = gas(129, 5, 13)
    want = B.seed_bodies(xyz, seeds, 450.0, 2)
    res = RP.seed_bodies(xyz, seeds, 450.0, 2, ctx=ctx)
    assert sorted(res) == sorted(BOUTS) and all(equal(res[k], want[k]) for k in BOUTS)
    assert res['size'].shape[1] == res['nbody'].max()              # trimmed
    lean = RP.seed_bodies(xyz, seeds, 450.0, 2, want_labels=False, ctx=ctx)
    assert lean['label'] is None and equal(lean['centre'], want['centre'])
    none = RP.seed_bodies(xyz, seeds, 1.0, 2, ctx=ctx)               # no body anywhere
    assert not none['nbody'].any() and none['size'].shape == (5, 0) and none['centre'].shape == (5, 0, 3)
    feat = RP.body_features(xyz, none['nbody'], none['centre'], ctx=ctx)
    assert feat['nearest'] is None and not feat['dist_sum'].any() and not feat['tsa_sum'].any()
    feat = RP.body_features(xyz, res['nbody'], res['centre'], 700.0, 0.002, want_nearest=True, ctx=ctx)
    ref = B.body_features(xyz, want['nbody'], want['centre'], 700.0, 0.002)
    assert all(equal(feat[k], ref[k]) for k in FOUTS[:4])
    assert np.all(np.abs(feat['tsa_sum'] - ref['tsa_sum']) <= tsa_bar(ref['tsa_sum'], want['nbody']))
    with pytest.raises(RuntimeError, match='exceed 8192'):
        RP.seed_bodies(np.zeros((8193, 1, 3), f32), np.arange(8193), ctx=ctx)
    with pytest.raises(ValueError):
        RP.body_features(xyz, res['nbody'][:-1], res['centre'], ctx=ctx)


def test_report_step_on_the_demo_population(ctx, tmp_path):
    """--steps seeded_bodies through main() on the demo population (its first three
    structures), every file against the oracle.  The TSA column carries tsa_sum's bar with
    two roundings more, the division by nstruct and the mean over the copies."""
    from igm_amd.steps import PopulationStore
    pop = load_golden('demo_population.npz')
    xyz = np.ascontiguousarray(pop['coordinates'][:, :3])
    cp, ci = pop['copy_ptr'], pop['copy_idx']
    nhap = len(cp) - 1
    p = str(tmp_path / 'demo.hss')
    PopulationStore.create(p, xyz, pop['radii'], pop['chrom'], pop['copy'], cp, ci)
    flags = np.random.default_rng(0).random(nhap) < 0.1
    np.savetxt(tmp_path / 'seeds.txt', flags.astype(int), fmt='%d')
    out = tmp_path / 'qc'
    assert RP.main([p, '--steps', 'seeded_bodies', '--seeds', str(tmp_path / 'seeds.txt'), '--link-cutoff', '900',
                    '--min-body-size', '3', '-l', 'run', '-o', str(out)]) == 0
    made = sorted(str(f.relative_to(out)) for f in out.rglob('*') if f.is_file())
    assert made == ['label.txt', 'seeded_bodies/centres-run.txt', 'seeded_bodies/count-run.txt',
                    'seeded_bodies/profiles-run.txt']
    seeds = RP.seed_beads(flags.astype(int), cp, ci)
    assert len(seeds) == 308
    want = B.seed_bodies(xyz, seeds, 900.0, 3)
    assert want['nbody'].tolist() == [30, 33, 35]
    assert [int(np.count_nonzero(B.component_sizes(lab) == 1)) for lab in want['label']] == [88, 80, 89]
    assert np.loadtxt(out / 'seeded_bodies/count-run.txt', dtype=np.int64).tolist() == [30, 33, 35]
    rows = np.loadtxt(out / 'seeded_bodies/centres-run.txt')
    assert rows.shape == (98, 6)
    at = 0
    for s in range(3):
        for k in range(want['nbody'][s]):
            assert rows[at, :3].tolist() == [s, k, want['size'][s, k]]
            assert rows[at, 3:].tolist() == want['centre'][s, k].tolist()      # %.17g reads back exactly
            at += 1
    ref = B.profiles(B.body_features(xyz, want['nbody'], want['centre']), want['nbody'], cp, ci)
    got = np.loadtxt(out / 'seeded_bodies/profiles-run.txt')
    assert got.shape == (nhap, 4) and np.array_equal(got[:, :3], ref[:, :3])
    assert 0 < got[:, 2].mean() < 1 and got[:, 1].max() > 0
    assert np.all(np.abs(got[:, 3] - ref[:, 3]) <= 2.0 * (35 + 3 + 4) * 2.0 ** -53 * ref[:, 3]) and got[:, 3].min() > 0
    # the other parameters and a run without a label, through report_population
    out = tmp_path / 'qc2'
    written = RP.report_population(p, steps='seeded_bodies', out_dir=str(out), seeds=flags.astype(int),
                                   link_cutoff=700.0, min_body_size=2, assoc_cutoff=900.0, tsa_decay=0.001, ctx=ctx)
    assert sorted(written) == ['label.txt', 'seeded_bodies/centres.txt', 'seeded_bodies/count.txt',
                               'seeded_bodies/profiles.txt']
    want = B.seed_bodies(xyz, seeds, 700.0, 2)
    assert np.loadtxt(out / 'seeded_bodies/count.txt', dtype=np.int64).tolist() == want['nbody'].tolist()
    ref = B.profiles(B.body_features(xyz, want['nbody'], want['centre'], 900.0, 0.001), want['nbody'], cp, ci)
    got = np.loadtxt(out / 'seeded_bodies/profiles.txt')
    assert np.array_equal(got[:, :3], ref[:, :3])
    assert np.all(np.abs(got[:, 3] - ref[:, 3]) <= 2.0 * (int(want['nbody'].max()) + 3 + 4) * 2.0 ** -53 * ref[:, 3])
