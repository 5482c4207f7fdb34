"""The pairwise conformation RMSD without a GPU: the NumPy restatement
tests/report_conformations_ref.py on cases whose answers are known in closed form or by brute
force, the host-side functions of igm_amd.report (conformation_beads, conformation_summary,
rmsd_edges_of) and the refusals and flags of the conformations report step."""
import numpy as np
import pytest

import report_conformations_ref as C
from igm_amd import report as RP

f32 = np.float32
PERM = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])   # a proper rotation, exact in float32


def pop_of(confs):
    """(nbead, 1, 3) float32 and the bead table of conformations given as (ncopy, nlocus, 3):
    one structure, copy k holds conformation k"""
    confs = np.asarray(confs, np.float64)
    ncopy, n = confs.shape[:2]
    return confs.reshape(ncopy * n, 1, 3).astype(f32), np.arange(ncopy * n, dtype=np.int32).reshape(ncopy, n)


def walk(n, seed, offset=1e5):
    """multiples of 1/64 around `offset`: exact in float32, and so are its whole-number shifts"""
    rng = np.random.default_rng(seed)
    return np.round((offset + np.cumsum(rng.normal(0, 60.0, (n, 3)), axis=0)) * 64.0) / 64.0


# ------------------------------------------------------------------ the restatement
def test_rigid_image_is_at_the_noise_floor():
    a = walk(40, 0)
    b = a @ PERM.T + np.array([3000.0, -3000.0, 3000.0])
    xyz, bead = pop_of([a, b, walk(40, 1)])
    assert np.array_equal(xyz[bead[1], 0].astype(np.float64), b)            # the image is exact
    r, g = C.rmsd_matrix(xyz, bead)
    floor = np.sqrt(1e-12 * (g[0] + g[1]) / 40)
    print('rigid image: rmsd %.3g, floor %.3g, unrelated walk %.3g' % (r[0, 1], floor, r[0, 2]))
    assert r[0, 1] <= floor and r[0, 2] > 100.0 and abs(g[0] - g[1]) <= 1e-12 * g[0]
    assert np.array_equal(r, r.T) and not r.diagonal().any()


def rotations(step_deg):
    """every rotation Rz(a) Ry(b) Rz(c) on a grid of step_deg: (n, 3, 3)"""
    ang = np.deg2rad(np.arange(0.0, 360.0, step_deg))
    half = np.deg2rad(np.arange(0.0, 180.0 + step_deg / 2, step_deg))

    def rz(t):
        m = np.zeros((len(t), 3, 3))
        m[:, 0, 0] = m[:, 1, 1] = np.cos(t)
        m[:, 0, 1], m[:, 1, 0] = -np.sin(t), np.sin(t)
        m[:, 2, 2] = 1.0
        return m

    def ry(t):
        m = np.zeros((len(t), 3, 3))
        m[:, 0, 0] = m[:, 2, 2] = np.cos(t)
        m[:, 0, 2], m[:, 2, 0] = np.sin(t), -np.sin(t)
        m[:, 1, 1] = 1.0
        return m

    return np.einsum('aij,bjk,ckl->abcil', rz(ang), ry(half), rz(ang)).reshape(-1, 3, 3)


def test_mirror_image_against_brute_force():
    """a mirror image is no match: its RMSD is the minimum over proper rotations only.  The
    grid of 4 degrees has a rotation within 3.5 degrees (0.061 rad) of the optimum, where the
    mean squared deviation exceeds its minimum by at most 0.061^2 (g_a + g_b) / (2 n): the
    brute-force value lies in [exact, sqrt(exact^2 + that)]."""
    a = np.array([[0.0, 0.0, 0.0], [300.0, 0.0, 0.0], [0.0, 200.0, 0.0], [50.0, 60.0, 250.0]])
    b = a * np.array([1.0, 1.0, -1.0])
    xyz, bead = pop_of([a, b])
    r, g = C.rmsd_matrix(xyz, bead)
    pa, pb = a - a.mean(axis=0), b - b.mean(axis=0)
    turned = np.einsum('rij,nj->rni', rotations(4.0), pb)
    brute = np.sqrt(((turned - pa[None]) ** 2).sum(axis=(1, 2)).min() / 4)
    slack = 0.061 ** 2 * (g[0] + g[1]) / (2 * 4)
    print('mirror image: rmsd %.6g, brute force %.6g, upper end %.6g' % (r[0, 1], brute, np.sqrt(r[0, 1] ** 2 + slack)))
    assert r[0, 1] > 50.0
    assert r[0, 1] * (1 - 1e-6) <= brute <= np.sqrt(float(r[0, 1]) ** 2 + slack)
    # with reflections allowed the two would coincide
    assert np.linalg.svd(pa.T @ pb)[1].sum() * 2 == pytest.approx(g[0] + g[1], rel=1e-12)


def test_two_loci_one_locus_and_a_collapsed_conformation():
    seg = lambda l, d: np.array([[0.0, 0.0, 0.0], np.asarray(d, np.float64) * l])      # noqa: E731
    xyz, bead = pop_of([seg(10.0, (1, 0, 0)), seg(4.0, (0, 1, 0)), seg(7.5, (0, 0, -1)), seg(0.0, (1, 0, 0))])
    r, g = C.rmsd_matrix(xyz, bead)
    lengths = np.array([10.0, 4.0, 7.5, 0.0])
    assert np.allclose(r, np.abs(lengths[:, None] - lengths[None, :]) / 2, rtol=1e-6, atol=1e-6)
    assert np.allclose(g, lengths ** 2 / 2)
    xyz, bead = pop_of([[[1.0, 2.0, 3.0]], [[-50.0, 0.0, 9.0]]])                        # nlocus = 1
    r, g = C.rmsd_matrix(xyz, bead)
    assert not r.any() and not g.any()
    w = walk(25, 3, offset=0.0)
    xyz, bead = pop_of([np.tile([[40.0, -8.0, 2.0]], (25, 1)), w])                      # all beads coincident
    r, g = C.rmsd_matrix(xyz, bead)
    assert g[0] == 0.0 and r[0, 1] == f32(np.sqrt(g[1] / 25))


def test_nan_rules_and_reductions():
    confs = np.stack([walk(6, s, offset=0.0) for s in range(6)])            # 2 copies x 3 structures
    xyz = np.zeros((12, 3, 3), f32)
    bead = np.arange(12, dtype=np.int32).reshape(2, 6)
    for k in range(2):
        for s in range(3):
            xyz[bead[k], s] = confs[k * 3 + s]
    xyz[bead[1, 2], 1, 0] = np.nan                                          # conformation 1 * 3 + 1 = 4
    edges = np.array([0.0, 100.0, 200.0, 400.0], f32)
    out = C.conformations(xyz, bead, edges)
    r = out['rmsd']
    assert np.isnan(out['g'][4]) and np.isnan(r[4]).all() and np.isnan(r[:, 4]).all()
    assert np.isfinite(np.delete(np.delete(r, 4, 0), 4, 1)).all()
    assert out['row_n'].tolist() == [4, 4, 4, 4, 0, 4] and out['row_sum'][4] == 0.0
    assert out['row_sum'][0] == float(np.float64(r[0, 1]) + np.float64(r[0, 2]) + np.float64(r[0, 3])
                                      + np.float64(r[0, 5]))
    assert out['same'].shape == (3, 2, 2) and out['same'][0, 0, 1] == r[0, 3] and out['same'][2, 1, 0] == r[5, 2]
    assert np.isnan(out['same'][1]).sum() == 3 and out['same'][1, 0, 0] == 0.0
    assert out['hist'].sum() <= 10 and out['hist'].dtype == np.int64


# ------------------------------------------------------------------ the host-side functions
# five haploid loci: chromosome 0 (loci 0-2, two copies), chromosome 1 (loci 3-4, one copy: an X);
# the beads of the second copy come first and in descending order
CHROM = np.array([0, 0, 0, 0, 0, 0, 1, 1], np.int32)
COPY = np.array([1, 1, 1, 0, 0, 0, 0, 0], np.int32)
COPY_PTR = np.array([0, 2, 4, 6, 7, 8], np.int32)
COPY_IDX = np.array([2, 3, 1, 4, 5, 0, 6, 7], np.int32)       # locus 0: beads 2 (copy 1), 3 (copy 0); ...


def test_conformation_beads(tmp_path):
    got = RP.conformation_beads(CHROM, COPY, COPY_PTR, COPY_IDX, 0)
    assert got.dtype == np.int32 and got.flags['C_CONTIGUOUS'] and got.tolist() == [[3, 4, 5], [2, 1, 0]]
    assert RP.conformation_beads(CHROM, COPY, COPY_PTR, COPY_IDX, 1).tolist() == [[6, 7]]   # a single copy
    assert RP.conformation_beads(CHROM, COPY, COPY_PTR, COPY_IDX, 0, [1, 0, 1, 1, 1]).tolist() == [[3, 5], [2, 0]]
    f = tmp_path / 'loci.txt'
    f.write_text('0\n1\n0\n0\n1\n')
    assert RP.conformation_beads(CHROM, COPY, COPY_PTR, COPY_IDX, 0, str(f)).tolist() == [[4], [1]]
    assert RP.conformation_beads(CHROM, COPY, COPY_PTR, COPY_IDX, 1, str(f)).tolist() == [[7]]
    # three copies, the beads of a locus in no particular order
    chrom, copy = np.zeros(6, np.int32), np.array([0, 1, 2, 2, 0, 1], np.int32)
    got = RP.conformation_beads(chrom, copy, np.array([0, 3, 6]), np.array([2, 0, 1, 5, 3, 4]), 0)
    assert got.tolist() == [[0, 4], [1, 5], [2, 3]]
    for bad in ([1, 0, 1], [1, 0, 1, 1, 1, 0], [0, 2, 0, 0, 0], [0, -1, 0, 0, 0], [0, 0, 0, 1, 1]):
        with pytest.raises(ValueError):
            RP.conformation_beads(CHROM, COPY, COPY_PTR, COPY_IDX, 0, bad)
    with pytest.raises(ValueError, match='no loci'):
        RP.conformation_beads(CHROM, COPY, COPY_PTR, COPY_IDX, 5)
    with pytest.raises(ValueError, match='copies'):                         # a locus that lost a copy
        RP.conformation_beads(CHROM, COPY, np.array([0, 2, 4, 5, 6, 7]), np.array([2, 3, 1, 4, 0, 6, 7]), 0)


def hand_made(r, nstruct, g, nlocus):
    out = C.reductions(np.asarray(r, f32), nstruct)
    out.update(g=np.asarray(g, np.float64), nlocus=nlocus)
    return out


def test_conformation_summary_by_hand():
    # two copies x two structures: a = (0, 0), (0, 1), (1, 0), (1, 1) by (copy, structure)
    r = np.array([[0, 4, 1, 6], [4, 0, 5, 2], [1, 5, 0, 3], [6, 2, 3, 0]], f32)
    sm = RP.conformation_summary(hand_made(r, 2, [8.0, 18.0, 32.0, 50.0], 2), 2)
    assert sm['mean_rmsd'].tolist() == [11 / 3, 11 / 3, 3.0, 11 / 3]
    assert sm['mean'] == 3.5 and sm['mean_rg'] == (2 + 3 + 4 + 5) / 4 and sm['variability'] == 1.0
    assert sm['medoid'] == (0, 1) and sm['medoid_mean_rmsd'] == 3.0          # (structure, copy) of a = 2
    assert sm['same_mean'] == 1.5 and sm['different_mean'] == 4.5 and sm['ratio'] == 1.5 / 4.5
    want = C.summary(r, np.array([8.0, 18.0, 32.0, 50.0]), 2, 2)
    assert all(sm[k] == want[k] for k in ('mean', 'mean_rg', 'variability', 'medoid', 'same_mean', 'different_mean'))
    # a tie goes to the lowest index
    tie = np.array([[0, 2, 2], [2, 0, 2], [2, 2, 0]], f32)
    sm = RP.conformation_summary(hand_made(tie, 3, [1.0, 1.0, 1.0], 1), 3)
    assert sm['medoid'] == (0, 0) and sm['mean'] == 2.0
    assert all(np.isnan(sm[k]) for k in ('same_mean', 'different_mean', 'ratio'))        # a single copy
    sm = RP.conformation_summary(hand_made(tie, 1, [1.0, 1.0, 1.0], 1), 1)                  # three copies of one cell
    assert sm['same_mean'] == 2.0 and np.isnan(sm['different_mean']) and np.isnan(sm['ratio'])
    # a conformation with a NaN counts nowhere; the medoid is among the others
    r = np.array([[np.nan] * 4, [np.nan, 0, 5, 2], [np.nan, 5, 0, 3], [np.nan, 2, 3, 0]], f32)
    sm = RP.conformation_summary(hand_made(r, 2, [np.nan, 18.0, 32.0, 50.0], 2), 2)
    assert np.isnan(sm['mean_rmsd'][0]) and sm['medoid'] == (1, 1) and sm['medoid_mean_rmsd'] == 2.5
    assert sm['mean'] == 10 / 3 and sm['mean_rg'] == 4.0 and sm['same_mean'] == 2.0 and sm['different_mean'] == 4.0
    # M = 1: nothing to average, the conformation is its own medoid
    sm = RP.conformation_summary(hand_made(np.zeros((1, 1), f32), 1, [9.0], 1), 1)
    assert np.isnan(sm['mean']) and np.isnan(sm['variability']) and sm['mean_rg'] == 3.0 and sm['medoid'] == (0, 0)
    with pytest.raises(ValueError):
        RP.conformation_summary(hand_made(tie, 3, [1.0, 1.0, 1.0], 1), 2)


def test_defaults_edges_and_the_library():
    from igm_amd import _lib
    assert RP.CONFORMATION_STEPS == ('conformations',) and 'conformations' not in RP.STEPS
    e = RP.rmsd_edges_of()
    assert e.dtype == f32 and np.array_equal(e, np.linspace(0, 10000, 201).astype(f32))
    assert np.array_equal(RP.rmsd_edges_of(300.0, 3), np.array([0, 100, 200, 300], f32))
    for bad in ((0.0, 10), (-5.0, 10), (np.inf, 10), (np.nan, 10), (100.0, 0), (100.0, -1), (100.0, 2.5),
                (100.0, 4097), (1e-44, 8)):
        with pytest.raises(ValueError):
            RP.rmsd_edges_of(*bad)
    assert hasattr(_lib.load(), 'igm_report_conformations')
    assert len(_lib.SIGNATURES['igm_report_conformations'][1]) == 16


# ------------------------------------------------------------------ the step's refusals and flags
@pytest.fixture()
def tiny_store(tmp_path):
    from igm_amd.steps import PopulationStore
    p = str(tmp_path / 'tiny.hss')
    xyz = np.random.default_rng(1).normal(0, 100, (8, 3, 3)).astype(f32)
    PopulationStore.create(p, xyz, np.full(8, 10.0, f32), CHROM, COPY, COPY_PTR, COPY_IDX)
    return p


def test_unknown_step_message_names_the_step(tiny_store, tmp_path):
    with pytest.raises(ValueError, match='conformations'):
        RP.report_population(tiny_store, steps='conformation', out_dir=str(tmp_path / 'qc'))
    assert not (tmp_path / 'qc').exists()


def test_bad_arguments_raise_before_anything_is_written(tiny_store, tmp_path):
    out = tmp_path / 'qc'
    loci = tmp_path / 'loci.txt'
    loci.write_text('1\n1\n')
    for kw in ({'conformation_chroms': [0, 7]}, {'conformation_chroms': [-1]}, {'conformation_loci': [1, 0, 1]},
               {'conformation_loci': [0, 0, 0, 1, 1]},                      # chromosome 0 is left without loci
               {'conformation_loci': [1, 2, 1, 1, 1]}, {'conformation_loci': str(loci)},
               {'rmsd_edges': [0.0]}, {'rmsd_edges': [0.0, 1.0, 1.0]}, {'rmsd_edges': [0.0, np.nan]},
               {'rmsd_edges': np.arange(4098.0)}):
        with pytest.raises(ValueError):
            RP.report_population(tiny_store, steps='conformations', out_dir=str(out), **kw)
    for argv in (['--conformation-chroms', '0,7'], ['--conformation-chroms', 'chr1'], ['--rmsd-bins', '0'],
                 ['--rmsd-max', '0'], ['--rmsd-max', 'nan'], ['--rmsd-bins', '5000'], ['--conformation-loci', str(loci)]):
        with pytest.raises(ValueError):
            RP.main([tiny_store, '--steps', 'conformations', '-o', str(out)] + argv)
    assert not out.exists()


def test_flags_reach_the_step(tiny_store, tmp_path, monkeypatch):
    """main() hands the five flags on; the step's GPU call is replaced by a recorder"""
    seen = {}

    def fake(hss, **kw):
        seen.update(kw)
        return {}

    monkeypatch.setattr(RP, 'report_population', fake)
    loci = tmp_path / 'loci.txt'
    assert RP.main([tiny_store, '--steps', 'conformations', '--conformation-chroms', '1,0', '--conformation-loci',
                    str(loci), '--save-rmsd', '--rmsd-max', '800', '--rmsd-bins', '4']) == 0
    assert seen['steps'] == 'conformations' and seen['conformation_chroms'] == [1, 0]
    assert seen['conformation_loci'] == str(loci) and seen['save_rmsd'] is True
    assert np.array_equal(seen['rmsd_edges'], np.array([0, 200, 400, 600, 800], f32))
    assert RP.main([tiny_store]) == 0
    assert seen['conformation_chroms'] is None and seen['conformation_loci'] is None and seen['save_rmsd'] is False
    assert np.array_equal(seen['rmsd_edges'], RP.rmsd_edges_of())
