"""The report on imaged nuclei on the MI355X (igm_report_map_levels / igm_report_map_lamina),
through the C ABI, against the restatement tests/report_map_ref.py on the inputs of
tests/report_map_cases.py.

Bars: integers and per-element values are equal (per-element: a call on one structure returns
the level and the depth themselves); a mean over n non-negative terms is within 2 n 2^-53
relative, the bar of test_report_gpu.py; the mean signed depth sums terms of both signs, so
its bar is 2 n 2^-53 of the mean ABSOLUTE depth.  level_mean and depth_mean also equal the
restatement summed in structure order, the order the header states, bit for bit.
Every call is made twice and must return the same bytes."""

import functools

import numpy as np
import pytest

import damid_edges as D
import report_map_cases as C
import report_map_ref as M
from igm_amd import _lib, report as RP, volume as V

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
DEDGES, SEDGES = np.linspace(0, 1.1, 12), np.linspace(0, 1.5, 151)
SIZES = (1, 31, 32, 33, 65)
INVALID, UNSUPPORTED = _lib.IGM_E_INVALID, _lib.IGM_E_UNSUPPORTED


@pytest.fixture(scope='module')
def ctx():
    """a context of this module's own: staging maps leaves the process-wide one alone"""
    c = _lib.Context(0)
    yield c
    c.close()


def _p(a):
    return None if a is None else a.ctypes.data


def stage(ctx, smap=None, vols=None):
    V.stage(ctx, list(C.maps() if vols is None else vols), smap)


def unstage(ctx):
    ctx.check(ctx.lib.igm_mstep_set_volumes(ctx.h, 0, None, None, 0), 'igm_mstep_set_volumes')


def call_levels(ctx, xyz, smap=None, scale=None, mean=False, depth=False, dedges=None, nshell=0, sedges=None,
                want=('smean', 'shist')):
    """igm_report_map_levels on host arrays, twice: (rc, mean, depth, density, shell_mean, shell_hist)"""
    xyz = np.ascontiguousarray(xyz, np.float32)
    n, S = xyz.shape[:2]
    scale = np.ascontiguousarray(C.scales() if scale is None else scale, np.float64)
    smap = None if smap is None else np.ascontiguousarray(smap, np.int32)
    outs = []
    for _ in range(2):
        m = np.full(n, -7.0) if mean else None
        dp = np.full(n, -7.0) if depth else None
        de = None if dedges is None else np.ascontiguousarray(dedges, np.float64)
        d = None if de is None else np.full(len(de) - 1, -7, np.int64)
        se = None if sedges is None else np.ascontiguousarray(sedges, np.float64)
        sm = np.full((S, max(nshell, 1)), -7.0) if nshell and 'smean' in want else None
        sh = np.full((max(nshell, 1), len(se) - 1), -7, np.int64) if se is not None and 'shist' in want else None
        rc = ctx.lib.igm_report_map_levels(ctx.h, 0, xyz.ctypes.data, n, S, _p(smap), scale.ctypes.data, _p(m), _p(dp),
                                           _p(de), 0 if de is None else len(de) - 1, _p(d), nshell, _p(sm), _p(se),
                                           0 if se is None else len(se) - 1, _p(sh))
        outs.append((rc, m, dp, d, sm, sh))
    for a, b in zip(outs[0][1:], outs[1][1:]):
        assert (a is None and b is None) or a.tobytes() == b.tobytes(), 'rerun differs'
    assert outs[0][0] == outs[1][0]
    return outs[0]


def call_lamina(ctx, xyz, thr, side, smap=None, radii=D.RADII, ptr=D.COPY_PTR, idx=D.COPY_IDX):
    """igm_report_map_lamina, twice: (rc, counts)"""
    xyz = np.ascontiguousarray(xyz, np.float32)
    thr = np.ascontiguousarray(thr, np.float64)
    radii = np.ascontiguousarray(radii, np.float32)
    smap = None if smap is None else np.ascontiguousarray(smap, np.int32)
    nhap = len(ptr) - 1
    outs = []
    for _ in range(2):
        cnt = np.full(nhap, -7, np.int64)
        rc = ctx.lib.igm_report_map_lamina(ctx.h, 0, xyz.ctypes.data, xyz.shape[0], xyz.shape[1], ptr.ctypes.data,
                                           idx.ctypes.data, nhap, radii.ctypes.data, _p(smap), thr.ctypes.data,
                                           int(side), cnt.ctypes.data)
        outs.append((rc, cnt))
    assert outs[0][0] == outs[1][0] and outs[0][1].tobytes() == outs[1][1].tobytes(), 'rerun differs'
    return outs[0]


@functools.lru_cache(maxsize=None)
def ref(nbead, S, kinds=C.KINDS):
    """(xyz, level, depth) of the shared population: computed once, read only"""
    xyz, _ = C.population(nbead, S, kinds)
    lev, dep = M.levels(xyz, C.maps(), C.struct_map(S), C.scales())
    lev.setflags(write=False)
    dep.setflags(write=False)
    return xyz, lev, dep


def rel_close(got, want, bar, scale=None):
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    ref_ = np.abs(want) if scale is None else np.asarray(scale)
    err = np.abs(got[ok] - want[ok])
    print('max err / scale %.3g (bar %.3g)' % (np.max(err / np.maximum(ref_[ok], 1e-300), initial=0.0), bar))
    assert np.all(err <= bar * ref_[ok])


def check_all(out, lev, dep, nshell=5, dedges=DEDGES, sedges=SEDGES):
    rc, mean, depth, dens, smean, shist = out
    n, S = lev.shape
    assert rc == 0
    import report_ref as R
    if mean is not None:
        rel_close(mean, lev.sum(axis=1) / S, 2 * S * U53)
        assert mean.tobytes() == M.mean_over_structures(lev).tobytes()
        assert not np.any(np.signbit(mean))
    if depth is not None:
        rel_close(depth, dep.sum(axis=1) / S, 2 * S * U53, scale=np.abs(dep).sum(axis=1) / S)
        assert depth.tobytes() == M.mean_over_structures(dep).tobytes()
    if dens is not None:
        assert np.array_equal(dens, R.histogram(lev, dedges))
    if smean is not None or shist is not None:
        want_mean, want_hist = M.shells_of_levels(lev, nshell, sedges)
        if smean is not None:
            rel_close(smean, want_mean, 2 * n * U53)
        if shist is not None:
            assert np.array_equal(shist, want_hist)
            assert shist.sum() == R.histogram(lev, sedges).sum()


# ------------------------------------------------------------------ levels
@pytest.mark.parametrize('S', SIZES)
@pytest.mark.parametrize('nbead', SIZES)
def test_tile_edges(ctx, nbead, S):
    """nbead and nstruct on both sides of the 32 x 32 tile, all outputs together, the staged table"""
    xyz, lev, dep = ref(nbead, S)
    stage(ctx, C.struct_map(S))
    out = call_levels(ctx, xyz, mean=True, depth=True, dedges=DEDGES, nshell=5, sedges=SEDGES)
    check_all(out, lev, dep)
    if S == 1:  # the mean of one structure is the value itself
        assert out[1].tobytes() == lev[:, 0].tobytes() and out[2].tobytes() == dep[:, 0].tobytes()


def test_every_level_and_depth_bit_equal(ctx):
    """one structure a call, its map named by struct_map: level_mean and depth_mean are the level and
    the depth of every bead -- voxel centres from -1 to n, half-steps, the lamina (depth 0, level 1),
    the deepest voxel (level 0), off-centre in it (clamped, sign bit clear), w = 0 in the grid"""
    xyz, lev, dep = ref(65, 65)
    _, kind = C.population(65, 65)
    sm = C.struct_map(65)
    stage(ctx)
    got_l, got_d = np.empty_like(lev), np.empty_like(dep)
    for s in range(65):
        rc, m, d, _, _, _ = call_levels(ctx, xyz[:, s:s + 1], smap=sm[s:s + 1], mean=True, depth=True)
        assert rc == 0
        got_l[:, s], got_d[:, s] = m, d
    for k in C.KINDS:
        sel = kind == k
        assert got_d[sel].tobytes() == dep[sel].tobytes(), k
        assert got_l[sel].tobytes() == lev[sel].tobytes(), k
    assert np.all(got_l[kind == 'lamina'] == 1.0) and np.all(got_d[kind == 'lamina'] == 0.0)
    assert np.all(got_l[kind == 'deepest'] == 0.0)
    assert np.all(got_l[kind == 'deep_off'] == 0.0) and not np.any(np.signbit(got_l))
    assert np.all(got_d[kind == 'outside_in_grid'] <= 0.0)


@pytest.mark.parametrize('nbins', (11, 1024, 1025))
def test_density_bins(ctx, nbins):
    """the density in LDS (up to 1024 bins) and in global atomics"""
    import report_ref as R
    xyz, lev, _ = ref(33, 33)
    stage(ctx, C.struct_map(33))
    edges = np.linspace(0, 2.5, nbins + 1)
    rc, _, _, dens, _, _ = call_levels(ctx, xyz, dedges=edges)
    assert rc == 0 and np.array_equal(dens, R.histogram(lev, edges)) and dens.sum() > 0


def test_shells_with_ties_and_empty_shells(ctx):
    """lattice beads: many levels tie on a shell boundary; nbead < nshell: empty shells are NaN"""
    xyz, lev, dep = ref(33, 8, ('centre',))
    stage(ctx, C.struct_map(8))
    check_all(call_levels(ctx, xyz, nshell=5, sedges=SEDGES), lev, dep)
    xyz, lev, dep = ref(3, 8)
    out = call_levels(ctx, xyz, nshell=5, sedges=SEDGES)
    check_all(out, lev, dep)
    assert np.isnan(out[4]).any() and np.isfinite(out[4]).any()


def test_each_output_alone(ctx):
    xyz, lev, dep = ref(33, 33)
    stage(ctx, C.struct_map(33))
    full = call_levels(ctx, xyz, mean=True, depth=True, dedges=DEDGES, nshell=5, sedges=SEDGES)
    check_all(full, lev, dep)
    alone = [call_levels(ctx, xyz, mean=True), call_levels(ctx, xyz, depth=True),
             call_levels(ctx, xyz, dedges=DEDGES), call_levels(ctx, xyz, nshell=5, want=('smean',)),
             call_levels(ctx, xyz, nshell=5, sedges=SEDGES, want=('shist',))]
    for k, out in enumerate(alone, start=1):
        assert out[0] == 0 and out[k].tobytes() == full[k].tobytes()
        assert all(o is None for j, o in enumerate(out[1:], start=1) if j != k)
    assert call_levels(ctx, xyz)[0] == 0  # nothing asked: nothing to do


def test_struct_map_sources(ctx):
    """given; NULL with a staged table; NULL with none staged (map 0); entries nmap and -1 refused"""
    xyz, lev, dep = ref(33, 33)
    sm = C.struct_map(33)
    stage(ctx)
    given = call_levels(ctx, xyz, smap=sm, mean=True, depth=True, dedges=DEDGES, nshell=5, sedges=SEDGES)
    check_all(given, lev, dep)
    lev0, dep0 = M.levels(xyz, C.maps(), None, C.scales())
    check_all(call_levels(ctx, xyz, mean=True, depth=True, dedges=DEDGES), lev0, dep0)
    assert not np.array_equal(lev0, lev)
    # a given struct_map wins over a staged one
    stage(ctx, np.zeros(33, np.int32))
    check_all(call_levels(ctx, xyz, smap=sm, mean=True, depth=True), lev, dep)
    stage(ctx, sm)
    staged = call_levels(ctx, xyz, mean=True, depth=True, dedges=DEDGES, nshell=5, sedges=SEDGES)
    for a, b in zip(given[1:], staged[1:]):
        assert a.tobytes() == b.tobytes()
    for bad in (len(C.maps()), -1):
        for where in (0, 32):
            smb = sm.copy()
            smb[where] = bad
            out = call_levels(ctx, xyz, smap=smb, mean=True)
            assert out[0] == INVALID and np.all(out[1] == -7.0)
            assert b'struct_map' in ctx.lib.igm_last_error(ctx.h)
            assert call_lamina(ctx, ref(12, 33)[0], [0.1] * 4, 1, smap=smb)[0] == INVALID
        check_all(call_levels(ctx, xyz, mean=True, depth=True), lev, dep)   # the context is still usable
    # a staged table shorter than the call
    stage(ctx, C.struct_map(8))
    assert call_levels(ctx, xyz, mean=True)[0] == INVALID


def test_refused_scales_thresholds_and_sides(ctx):
    xyz, lev, dep = ref(12, 33)
    stage(ctx, C.struct_map(33))
    for bad in (0.0, -1.0, np.nan, np.inf):
        sc = np.array(C.scales())
        sc[2] = bad
        out = call_levels(ctx, xyz, scale=sc, mean=True)
        assert out[0] == INVALID and np.all(out[1] == -7.0)
    thr = 0.25 * np.array(C.scales())
    for bad in (np.nan, np.inf, -np.inf):
        t = thr.copy()
        t[3] = bad
        rc, cnt = call_lamina(ctx, xyz, t, 1)
        assert rc == INVALID and np.all(cnt == -7)
    for side in (0, 2, -2):
        assert call_lamina(ctx, xyz, thr, side)[0] == INVALID
    check_all(call_levels(ctx, xyz, mean=True, depth=True), lev, dep)
    assert call_lamina(ctx, xyz, thr, 1)[0] == 0


def test_no_maps_staged(ctx):
    xyz, lev, dep = ref(12, 33)
    unstage(ctx)
    out = call_levels(ctx, xyz, mean=True)
    assert out[0] == INVALID and np.all(out[1] == -7.0)
    rc, cnt = call_lamina(ctx, xyz, [0.1] * 4, 1)
    assert rc == INVALID and np.all(cnt == -7)
    stage(ctx, C.struct_map(33))
    check_all(call_levels(ctx, xyz, mean=True, depth=True), lev, dep)


def test_limits_are_those_of_report_levels(ctx):
    stage(ctx)
    xyz = np.zeros((6, 2, 3), np.float32)
    rc = call_levels(ctx, xyz, nshell=257, want=('smean',))[0]
    assert rc == UNSUPPORTED
    sc = np.ascontiguousarray(C.scales())
    rc = ctx.lib.igm_report_map_levels(ctx.h, 0, xyz.ctypes.data, 65536, 1, None, sc.ctypes.data, None, None, None, 0,
                                       None, 0, None, None, 0, None)
    assert rc == UNSUPPORTED   # refused before anything is read
    assert call_levels(ctx, xyz, nshell=0, sedges=SEDGES, want=('shist',))[0] == INVALID


def test_device_pointers(ctx):
    """IGM_DEVICE_PTRS: xyz and the outputs are device memory, the small inputs stay on the host"""
    import torch
    xyz, lev, dep = ref(33, 33)
    sm = C.struct_map(33)
    stage(ctx, sm)
    n, S = 33, 33
    dx = torch.from_numpy(np.array(xyz)).cuda()
    f64 = dict(dtype=torch.float64, device='cuda')
    i64 = dict(dtype=torch.int64, device='cuda')
    mean, depth, dens = torch.empty(n, **f64), torch.empty(n, **f64), torch.empty(11, **i64)
    smean, shist = torch.empty((S, 5), **f64), torch.empty((5, 150), **i64)
    sc = np.ascontiguousarray(C.scales())
    F = _lib.IGM_DEVICE_PTRS
    rc = ctx.lib.igm_report_map_levels(ctx.h, F, dx.data_ptr(), n, S, None, sc.ctypes.data, mean.data_ptr(),
                                       depth.data_ptr(), DEDGES.ctypes.data, 11, dens.data_ptr(), 5, smean.data_ptr(),
                                       SEDGES.ctypes.data, 150, shist.data_ptr())
    ctx.check(rc, 'igm_report_map_levels')
    host = call_levels(ctx, xyz, mean=True, depth=True, dedges=DEDGES, nshell=5, sedges=SEDGES)
    for dev, h in zip((mean, depth, dens, smean, shist), host[1:]):
        assert dev.cpu().numpy().tobytes() == h.tobytes()
    x12 = ref(12, 33)[0]
    dx = torch.from_numpy(np.array(x12)).cuda()
    cnt = torch.empty(D.NHAP, **i64)
    thr = 0.25 * sc
    rc = ctx.lib.igm_report_map_lamina(ctx.h, F, dx.data_ptr(), 12, S, D.COPY_PTR.ctypes.data, D.COPY_IDX.ctypes.data,
                                       D.NHAP, D.RADII.ctypes.data, None, thr.ctypes.data, 1, cnt.data_ptr())
    ctx.check(rc, 'igm_report_map_lamina')
    assert np.array_equal(cnt.cpu().numpy(), call_lamina(ctx, x12, thr, 1)[1])


# ------------------------------------------------------------------ lamina
@pytest.mark.parametrize('S', (1, 63, 64, 65, 255, 256, 257))
def test_lamina_counts(ctx, S):
    """loci of 1, 2, 3, 4 and 0 copies behind an unsorted copy index, every copy another radius;
    structures on both sides of the wave and of the workgroup; both sides; both struct_map sources"""
    xyz = ref(12, S)[0]
    sm, vols = C.struct_map(S), C.maps()
    thr = 0.25 * np.array(C.scales())
    stage(ctx, sm)
    for side in (1, -1):
        want = M.lamina_counts(xyz, D.RADII, D.COPY_PTR, D.COPY_IDX, vols, sm, thr, side)
        rc, cnt = call_lamina(ctx, xyz, thr, side)
        assert rc == 0 and np.array_equal(cnt, want)
        rc, cnt = call_lamina(ctx, xyz, thr, side, smap=sm)
        assert rc == 0 and np.array_equal(cnt, want)
        assert cnt[4] == 0                       # the locus without copies
        if S >= 63:
            assert 0 < cnt.sum() < 12 * S
            own = M.lamina_counts(xyz, D.RADII, D.COPY_PTR, D.COPY_IDX, vols, sm, thr, side, own_radius=True)
            assert not np.array_equal(own, want)  # only the first copy's radius may enter


def test_lamina_threshold_is_closed(ctx):
    """depth - r == thr exactly is a contact; the double below thr is not; the first copy's radius
    decides for every copy; a body map reads the other side"""
    S = 9
    xyz, T = C.lamina_traps(S)
    sm, vols = C.struct_map(S), C.maps()
    stage(ctx, sm)
    full = np.diff(D.COPY_PTR).astype(np.int64) * S
    for side in (1, -1):
        thr = side * T - 0.5
        for t in (thr, np.nextafter(thr, -np.inf), np.nextafter(thr, np.inf)):
            want = M.lamina_counts(xyz, D.RADII, D.COPY_PTR, D.COPY_IDX, vols, sm, t, side)
            rc, cnt = call_lamina(ctx, xyz, t, side)
            assert rc == 0 and np.array_equal(cnt, want)
        assert np.array_equal(call_lamina(ctx, xyz, thr, side)[1], full)
        below = call_lamina(ctx, xyz, np.nextafter(thr, -np.inf), side)[1]
        assert np.all(below[:4] == 0) and below[5] == full[5]
    # the nucleus threshold read on the body side and the other way round
    assert np.all(call_lamina(ctx, xyz, -T - 0.5, 1)[1][:4] == 0)
    assert np.array_equal(call_lamina(ctx, xyz, T - 0.5, -1)[1], full)


# ------------------------------------------------------------------ report_population
def test_report_population_on_the_gpu(ctx, tmp_path):
    """The tiny run of test_report_map.py through the kernels: every file equals the restatement's.
    The two files that hold shell means (shells/ave_radial.txt, and radials_norm.txt divided by its
    last entry) are held to the bar of a shell mean, 2 n 2^-53 relative plus the same for the
    average over the structures: the order of a shell's sum is the kernel's own."""
    run = C.write_run(tmp_path)
    steps = ('shells', 'radials', 'damid', 'bodies')
    written = RP.report_population(run['path'], steps=steps, out_dir=str(tmp_path / 'qc'), ctx=ctx)
    want = C.expected_files(run)
    assert set(written) == set(want) | {'label.txt'}
    bar = 2 * 13 * U53 + 2 * C.RUN_S * U53
    for name, a in want.items():
        got = np.loadtxt(tmp_path / 'qc' / name)
        if name in ('shells/ave_radial.txt', 'radials/radials_norm.txt'):
            rel_close(got, a, bar + 2 * U53)   # and the one division of radials_norm
        else:
            assert np.array_equal(got, a, equal_nan=True), name
    radials = np.loadtxt(tmp_path / 'qc' / 'radials/radials.txt')
    ave = np.loadtxt(tmp_path / 'qc' / 'shells/ave_radial.txt')
    assert np.array_equal(np.loadtxt(tmp_path / 'qc' / 'radials/radials_norm.txt'), radials / ave[-1])
