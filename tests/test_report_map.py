"""The report on imaged nuclei without a GPU: every input of report_map_cases.py is the edge
it claims, the definition (report_map_ref.py) reduces to the ellipsoid forms on voxelised
spheres, and report_population writes the restatement's numbers when its two native calls
are answered by the restatement."""

import numpy as np
import pytest

import damid_edges as D
import report_map_cases as C
import report_map_ref as M
from igm_amd import report as RP, volume as V

f32, f64 = np.float32, np.float64


# ------------------------------------------------------------------ 1. the inputs are the edges
def test_maps_and_scales():
    vols = C.maps()
    assert [tuple(v['nvoxel']) for v in vols] == [(11, 11, 11), (13, 13, 13), (11, 11, 11), (5, 7, 9)]
    assert tuple(vols[3]['grid']) == (1.0, 0.5, 0.25)
    for v, s in zip(vols, C.scales()):
        assert s > 0 and RP.map_depth_scale(v) == s  # the host function and the restatement agree bit for bit
    assert C.scales()[3] == 0.75
    assert sorted(set(C.struct_map(65))) == [0, 1, 2, 3] and tuple(C.struct_map(8)) == C.SMAP_PATTERN


def test_population_holds_every_kind_on_every_map():
    xyz, kind = C.population(65, 65)
    sm = C.struct_map(65)
    lev, dep = M.levels(xyz, C.maps(), sm, C.scales())
    raw, _ = M.levels(xyz, C.maps(), sm, C.scales(), no_level_clamp=True)
    for m in range(4):
        col = sm == m
        for k in C.KINDS:
            assert np.any(kind[:, col] == k), (m, k)
        k_ = kind[:, col]
        assert np.all(dep[:, col][k_ == 'lamina'] == 0.0) and np.all(lev[:, col][k_ == 'lamina'] == 1.0)
        assert np.all(lev[:, col][k_ == 'deepest'] == 0.0)
        assert np.all(dep[:, col][k_ == 'deepest'] == C.scales()[m])
        # the clamp case does have a negative raw level, and the clamped one is +0.0
        assert np.all(raw[:, col][k_ == 'deep_off'] < 0.0)
        assert np.all(lev[:, col][k_ == 'deep_off'] == 0.0) and not np.any(np.signbit(lev[:, col][k_ == 'deep_off']))
        out = k_ == 'outside_in_grid'
        _, _, in_grid = M.voxel(xyz[:, col][out], C.maps()[m])
        assert in_grid.all() and np.all(dep[:, col][out] <= 0.0) and np.all(lev[:, col][out] >= 1.0)
    assert not np.any(np.signbit(lev))
    # both out-of-grid sides of every axis occur
    for m in range(4):
        u, _, _ = M.voxel(xyz[:, sm == m], C.maps()[m])
        n = M.geometry(C.maps()[m])[0]
        for d in range(3):
            assert np.any(u[..., d] == -1) and np.any(u[..., d] == n[d])


MISTAKES = ('half_up', 'swap_stride', 'no_voxel_clamp', 'ignore_w')


def test_every_mistake_changes_a_depth():
    """the half-step beads round differently under floor(x + 0.5); the box map tells n[1] from
    n[2]; the out-of-grid beads tell the clamp; the in-grid w = 0 beads tell the flag"""
    xyz, kind = C.population(65, 65)
    sm = C.struct_map(65)
    _, dep = M.levels(xyz, C.maps(), sm, C.scales())
    changed = {}
    for mk in MISTAKES:
        _, bad = M.levels(xyz, C.maps(), sm, C.scales(), **{mk: True})
        changed[mk] = bad != dep
        assert changed[mk].any(), mk
    # half steps k + 1/2 with k even and odd are present, and only 'half' beads move
    u_even = u_odd = False
    for m in range(4):
        n, o, g = M.geometry(C.maps()[m])
        q = (xyz[:, sm == m].astype(f64) - o) / g
        fr = q - np.floor(q)
        k = np.floor(q)[fr == 0.5]
        u_even |= bool(np.any(k % 2 == 0))
        u_odd |= bool(np.any(k % 2 == 1))
    assert u_even and u_odd
    assert set(kind[changed['half_up']]) == {'half'}
    assert np.all(sm[np.nonzero(changed['swap_stride'])[1]] == 3)   # every committed map is cubic
    _, _, in_grid = zip(*[M.voxel(xyz[:, s], C.maps()[sm[s]]) for s in range(65)])
    in_grid = np.stack(in_grid, 1)
    # the flag decides only in the grid, on voxels with w = 0; every 'outside_in_grid' bead off the
    # lamina's own record is one (on a voxel centre with depth 0 the sign shows nothing)
    assert np.all(in_grid[changed['ignore_w']]) and np.all(dep[changed['ignore_w']] < 0)
    assert np.array_equal(changed['ignore_w'][kind == 'outside_in_grid'], dep[kind == 'outside_in_grid'] < 0)
    assert np.any(kind[changed['ignore_w']] == 'outside_in_grid')
    assert not np.any(in_grid[changed['no_voxel_clamp']])


def test_shell_lattice_has_ties_on_boundaries():
    xyz, _ = C.population(33, 8, kinds=('centre',))
    lev, _ = M.levels(xyz, C.maps(), C.struct_map(8), C.scales())
    bds = [int(k * 33 / 5) for k in range(1, 5)]
    ties = 0
    for s in range(8):
        r = np.sort(lev[:, s])
        ties += sum(r[b - 1] == r[b] for b in bds)
    assert ties >= 4


def test_lamina_traps_sit_on_the_threshold():
    S = 9
    xyz, T = C.lamina_traps(S)
    sm, vols = C.struct_map(S), C.maps()
    _, dep = M.levels(xyz, vols, sm, C.scales())
    assert np.array_equal(dep, np.broadcast_to(T[sm], dep.shape))
    full = np.diff(D.COPY_PTR).astype(np.int64) * S
    first_half = np.array([D.RADII[D.COPY_IDX[D.COPY_PTR[h]]] == 0.5 if full[h] else False for h in range(D.NHAP)])
    for side in (1, -1):
        thr = side * T - 0.5
        assert np.array_equal((side * dep[0] - 0.5), thr[sm])   # depth - r == thr exactly
        on = M.lamina_counts(xyz, D.RADII, D.COPY_PTR, D.COPY_IDX, vols, sm, thr, side)
        below = M.lamina_counts(xyz, D.RADII, D.COPY_PTR, D.COPY_IDX, vols, sm, np.nextafter(thr, -np.inf), side)
        above = M.lamina_counts(xyz, D.RADII, D.COPY_PTR, D.COPY_IDX, vols, sm, np.nextafter(thr, np.inf), side)
        assert np.array_equal(on, full) and np.array_equal(above, full)
        assert np.array_equal(below, np.where(first_half, 0, full))     # locus 5: r = 0.75 stays in contact
        strict = M.lamina_counts(xyz, D.RADII, D.COPY_PTR, D.COPY_IDX, vols, sm, thr, side, strict=True)
        assert np.array_equal(strict, below)
        own = M.lamina_counts(xyz, D.RADII, D.COPY_PTR, D.COPY_IDX, vols, sm, thr, side, own_radius=True)
        # a copy with a smaller radius of its own leaves the contact: beads 10 (0.25) and 4 (0.375)
        assert own[1] == full[1] - S and own[5] == full[5] - S and own[0] == full[0]
    thr = -T - 0.5
    flipped = M.lamina_counts(xyz, D.RADII, D.COPY_PTR, D.COPY_IDX, vols, sm, thr, -1, ignore_side=True)
    assert np.all(flipped[:4] == 0) and np.all(full[:4] > 0)            # read as a nucleus map: no contact
    assert full[4] == 0                                                 # a locus without copies


# ------------------------------------------------------------------ 2. reduces to the ellipsoid
SPHERES = [(2.0, 0.5, 1), (1.25, 0.25, 1), (3.0, 1.0, 2), (5.0, 0.5, 3), (5500.0, 100.0, 3)]
SHIFT = (0.13, -0.4, 0.27)


@pytest.mark.parametrize('R,grid,margin', SPHERES)
@pytest.mark.parametrize('shifted', (False, True))
def test_depth_is_the_distance_to_the_sphere(R, grid, margin, shifted):
    c = tuple(grid * t for t in SHIFT) if shifted else (0.0, 0.0, 0.0)
    vol = V.sphere_map(R, grid, margin, center=c)
    rng = np.random.default_rng(int(R * 100) + shifted)
    x = (np.asarray(vol['center'], f64) + rng.uniform(-1.3 * R, 1.3 * R, (200000, 3))).astype(f32)
    d = M.depth(x, vol)
    dist = np.sqrt(((x.astype(f64) - np.asarray(c, f64))**2).sum(axis=1))
    err = np.abs(d - (R - dist)).max() / grid
    print('R %g grid %g shifted %d: max |depth - (R - |x - c|)| = %.3f grid' % (R, grid, shifted, err))
    assert err <= 2.5
    if grid == 100.0:
        lev = M.level_of_depth(d, M.depth_scale(vol))
        lerr = np.abs(lev - dist / R).max()
        print('level against |x - c| / R: %.4f' % lerr)
        assert lerr <= 0.05


# ------------------------------------------------------------------ 3. report_population
@pytest.fixture
def cpu_map_report(monkeypatch):
    """igm_amd.report with its two native map calls answered by the restatement"""
    import report_ref as R

    def map_levels(xyz, volumes, struct_map, ctx, device, want_mean=False, want_depth=False, density_edges=None,
                   nshell=0, shell_edges=None):
        lev, dep = M.levels(xyz, volumes, struct_map)
        smean, shist = M.shells_of_levels(lev, nshell, shell_edges) if nshell else (None, None)
        return (M.mean_over_structures(lev) if want_mean else None, M.mean_over_structures(dep) if want_depth else None,
                R.histogram(lev, density_edges) if density_edges is not None else None, smean, shist)

    def map_lamina_counts(pop, volumes, struct_map=None, radii=None, copy_ptr=None, copy_idx=None,
                          contact_range=0.05, side=1, **kw):
        thr = [contact_range * M.depth_scale(v) for v in volumes]
        return M.lamina_counts(pop, radii, copy_ptr, copy_idx, volumes, struct_map, thr, side), np.diff(copy_ptr)

    def levels(xyz, semiaxes, ctx, device, want_mean=False, density_edges=None, nshell=0, shell_edges=None):
        sx = RP._semiaxes(semiaxes)
        return (R.level_mean(xyz, sx) if want_mean else None,
                R.histogram(R.levels(xyz, sx), density_edges) if density_edges is not None else None, None, None)

    monkeypatch.setattr(RP, '_map_levels', map_levels)
    monkeypatch.setattr(RP, 'map_lamina_counts', map_lamina_counts)
    monkeypatch.setattr(RP, '_levels', levels)
    return RP


STEPS = ('shells', 'radials', 'damid', 'bodies')


def test_report_population_on_named_maps(cpu_map_report, tmp_path):
    run = C.write_run(tmp_path)
    assert np.array_equal(run['smap'], [2, 0, 1, 1, 0, 2, 0, 2, 0])   # cyclic through the 7 entries
    written = cpu_map_report.report_population(run['path'], steps=STEPS, out_dir=str(tmp_path / 'qc'))
    want = C.expected_files(run)
    assert set(written) == set(want) | {'label.txt'}
    for name, a in want.items():
        got = np.loadtxt(tmp_path / 'qc' / name)
        assert np.array_equal(got, a, equal_nan=True), name
    dens = want['radials/density_histo.txt']
    assert np.isfinite(dens).any() and np.nansum(dens) > 0
    assert np.any(want['damid/output.txt'] > 0) and np.any(want['damid/output.txt'] < 1)
    assert np.any(want['bodies/nucleolus_frequency.txt'] > 0)


def test_explicit_semiaxes_still_select_the_ellipsoid(cpu_map_report, tmp_path):
    import report_ref as R
    run = C.write_run(tmp_path)
    written = cpu_map_report.report_population(run['path'], steps=('radials',), out_dir=str(tmp_path / 'qc'),
                                               semiaxes=(3.0, 2.0, 4.0))
    assert set(written) == {'label.txt', 'radials/radials.txt', 'radials/density_histo.txt'}
    want = RP.average_copies(R.level_mean(run['xyz'], (3.0, 2.0, 4.0)), run['copy_ptr'], run['copy_idx'])
    assert np.array_equal(np.loadtxt(tmp_path / 'qc' / 'radials/radials.txt'), want)


def test_configuration_without_map_names_still_raises(cpu_map_report, tmp_path):
    run = C.write_run(tmp_path, name_maps=False, nucleolus=False)
    for step in ('radials', 'shells', 'damid'):
        with pytest.raises(ValueError, match='exp_map'):
            cpu_map_report.report_population(run['path'], steps=(step,), out_dir=str(tmp_path / 'qc'))
    with pytest.raises(ValueError, match='nucleolus'):
        cpu_map_report.report_population(run['path'], steps=('bodies',), out_dir=str(tmp_path / 'qc'))
    assert not (tmp_path / 'qc').exists()
    assert RP.named_maps(run['cfg'], 9) is None


def test_depth_scale_errors():
    vol = dict(C.maps()[3])
    empty = dict(vol, matrice=np.zeros_like(vol['matrice']))
    with pytest.raises(ValueError, match='inside'):
        RP.map_depth_scale(empty)
    mat = np.zeros_like(vol['matrice'])
    mat[2, 3, 4] = (2, 3, 4, 1)       # one inside voxel that is its own lamina voxel: scale 0
    with pytest.raises(ValueError, match='depth scale'):
        RP.map_depth_scale(dict(vol, matrice=mat))


def test_shell_volumes_are_the_host_functions():
    edges = np.linspace(0, 1.1, 12)
    for v in C.maps():
        a, b = RP.map_shell_volumes(v, edges), M.shell_volumes(v, edges)
        assert np.array_equal(a, b)
        g = M.geometry(v)[2]
        assert a.sum() == np.count_nonzero(v['matrice'][..., 3]) * g[0] * g[1] * g[2]
