"""The neighbourhood features without a GPU: the NumPy oracle (report_neighbours_ref.py)
against cases counted by hand, the host-side folds of igm_amd/report.py on crafted
censuses, the wiring of the new report steps, and the window CSR of local_compaction."""
import warnings

import numpy as np
import pytest

import report_neighbours_ref as N
from igm_amd import report as RP

f32 = np.float32


def pop_of(rows):
    """(nbead, 1, 3) float32 from one position per bead"""
    return np.asarray(rows, f32)[:, None, :]


# ------------------------------------------------------------------ the oracle, by hand
def test_three_collinear_beads():
    xyz = pop_of([(0, 0, 0), (300, 0, 0), (700, 0, 0)])  # 0-1 300, 1-2 400, 0-2 700 apart
    one = N.results(xyz, [5, 5, 5], cutoff=500.0)
    assert one['census'][:, 0].tolist() == [[1, 0], [2, 0], [1, 0]]
    two = N.results(xyz, [0, 0, 1], cutoff=500.0)
    assert two['census'][:, 0].tolist() == [[1, 0], [1, 1], [0, 1]]
    assert two['sums'].tolist() == [[1, 0], [1, 1], [0, 1]]
    assert two['icp_sum'].tolist() == [0.0, 0.5, 1.0] and two['icp_n'].tolist() == [1, 1, 1]
    far = N.results(xyz, [0, 0, 1], cutoff=100.0)
    assert not far['census'].any() and far['icp_n'].tolist() == [0, 0, 0] and far['icp_sum'].tolist() == [0.0] * 3


def test_pair_exactly_at_the_bound():
    above = np.nextafter(f32(500.0), f32(np.inf))
    xyz = np.zeros((2, 3, 3), f32)
    xyz[1, :, 1] = (np.nextafter(f32(500.0), f32(0)), 500.0, above)
    cen = N.census(xyz, [0, 1], cutoff=500.0)
    assert cen[0, :, 1].tolist() == [1, 1, 0] and cen[1, :, 1].tolist() == [1, 1, 0]
    # the radii form: fl32(fl32(0.1) * fl32(2500 + 2500)) is the bound, whatever 0.1 * 5000 is in float64
    bound = f32(f32(0.1) * f32(5000.0))
    xyz[1, :, 1] = (bound, np.nextafter(bound, f32(np.inf)), np.nextafter(bound, f32(0)))
    cen = N.census(xyz, [0, 1], radii=[2500.0, 2500.0], contact_range=0.1)
    assert cen[0, :, 1].tolist() == [1, 0, 1]


def test_coincident_beads_at_cutoff_zero():
    xyz = pop_of([(1, 2, 3), (1, 2, 3), (1, 2, 3.5)])
    cen = N.census(xyz, [0, 1, 2], cutoff=0.0)
    assert cen[:, 0].tolist() == [[0, 1], [0, 1], [0, 0]]


def test_nan_and_inf_have_no_neighbours():
    xyz = pop_of([(0, 0, 0), (np.nan, 0, 0), (np.inf, 0, 0), (1, 0, 0), (np.inf, 0, 0)])
    cen = N.census(xyz, [0, 1, 2, 3, 4], cutoff=f32(3e38))
    assert cen[:, 0, 1].tolist() == [1, 0, 0, 1, 0]


def test_homologous_copy_is_trans():
    chain = RP.chain_numbers(chrom=[0, 0, 0, 0], copy=[0, 0, 1, 1])
    assert chain.tolist() == [0, 0, 1, 1]
    xyz = pop_of([(0, 0, 0), (5000, 0, 0), (100, 0, 0), (9000, 0, 0)])  # bead 0 beside its homologue 2 only
    res = N.results(xyz, chain, cutoff=500.0)
    assert res['census'][:, 0].tolist() == [[0, 1], [0, 0], [0, 1], [0, 0]]
    assert res['icp_sum'].tolist() == [1.0, 0.0, 1.0, 0.0] and res['icp_n'].tolist() == [1, 0, 1, 0]
    # chains that are not contiguous in the index keep their numbers
    assert RP.chain_numbers([1, 0, 1, 0, 1], [0, 0, 0, 1, 1]).tolist() == [2, 0, 2, 1, 3]


def test_min_sep_across_a_chain_boundary():
    xyz = np.zeros((6, 1, 3), f32)  # six coincident beads: everybody is within the cutoff
    chain = [0, 0, 0, 1, 1, 1]
    want = {1: [[2, 3]] * 6,                                          # only i itself is ignored
            2: [[1, 3], [0, 3], [1, 3], [1, 3], [0, 3], [1, 3]],      # the neighbours on the chain too
            3: [[0, 3]] * 6}                                          # beyond the chain length: no cis left
    for min_sep, rows in want.items():
        cen = N.census(xyz, chain, min_sep=min_sep, cutoff=1.0)
        assert cen[:, 0].tolist() == rows, min_sep  # bead 3 is at |i - j| = 1 of bead 2 and trans: never ignored


def test_unlabelled_column():
    xyz = np.zeros((4, 1, 3), f32)
    cen = N.census(xyz, [0, 1, 2, 3], cls=[-1, 0, 1, -1], nclass=2, cutoff=1.0)
    # columns: cis, class 0, class 1, unlabelled
    assert cen[:, 0].tolist() == [[0, 1, 1, 1], [0, 0, 1, 2], [0, 1, 0, 2], [0, 1, 1, 1]]
    absent = N.census(xyz, [0, 0, 2, 3], cls=[1, 1, 1, -1], nclass=2, cutoff=1.0)  # class 0 has no bead
    assert absent[:, 0].tolist() == [[1, 0, 1, 1], [1, 0, 1, 1], [0, 0, 2, 1], [0, 0, 3, 0]]


def test_icp_sum_is_sequential():
    """thirds do not add up the same pairwise and one after the other"""
    rng = np.random.default_rng(0)
    cen = rng.integers(0, 7, (3, 1000, 3)).astype(np.int32)
    s, n = N.icp(cen)
    for b in range(3):
        acc, cnt = 0.0, 0
        for row in cen[b]:
            if row.sum() > 0:
                acc += float(row[1] + row[2]) / float(row.sum())
                cnt += 1
        assert s[b] == acc and n[b] == cnt


# ------------------------------------------------------------------ the host-side folds
COPY_PTR = np.array([0, 2, 3], np.int32)
COPY_IDX = np.array([0, 2, 1], np.int32)   # locus 0 = beads 0 and 2, locus 1 = bead 1


def test_trans_class_fraction_by_hand():
    cen = np.zeros((3, 2, 4), np.int32)
    cen[0, 0] = (9, 1, 3, 5)    # 1/4, 3/4; cis and unlabelled partners do not count
    cen[0, 1] = (2, 0, 0, 7)    # no labelled trans partner: skipped
    cen[2, 0] = (0, 2, 2, 0)    # 1/2, 1/2
    cen[2, 1] = (0, 4, 0, 0)    # 1, 0
    cen[1, :] = (3, 0, 0, 1)    # locus 1: nothing labelled anywhere
    got = RP.trans_class_fraction(cen, COPY_PTR, COPY_IDX)
    assert got.shape == (2, 2)
    assert got[0].tolist() == [0.5, 0.5] and np.all(np.isnan(got[1]))
    assert np.array_equal(got, N.trans_fraction(cen, COPY_PTR, COPY_IDX), equal_nan=True)
    assert RP.trans_class_fraction(cen[:, :, :2], COPY_PTR, COPY_IDX).shape == (2, 0)  # nclass = 0


def test_icp_fold_and_nan_rules():
    per_bead = RP.icp_of(np.array([1.0, 0.0, 0.5]), np.array([4, 0, 1], np.int32))
    assert per_bead[0] == 0.25 and np.isnan(per_bead[1]) and per_bead[2] == 0.5
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        got = RP._fold_copies(per_bead, COPY_PTR, COPY_IDX)  # locus 1 is all NaN
        skip = RP._fold_copies(per_bead, np.array([0, 2, 3], np.int32), np.array([0, 1, 2], np.int32))
    assert got[0] == 0.375 and np.isnan(got[1])
    assert skip.tolist() == [0.25, 0.5]  # a NaN copy is left out of its locus's mean
    assert np.array_equal(got, N.fold_mean(per_bead, COPY_PTR, COPY_IDX), equal_nan=True)


def test_haploid_classes(tmp_path):
    bead, nclass = RP.haploid_classes([1, -1], COPY_PTR, COPY_IDX)
    assert bead.tolist() == [1, -1, 1] and bead.dtype == np.int32 and nclass == 2
    assert RP.haploid_classes([-1, -1], COPY_PTR, COPY_IDX)[1] == 0
    f = tmp_path / 'classes.txt'
    f.write_text('0\n7\n')
    bead, nclass = RP.haploid_classes(str(f), COPY_PTR, COPY_IDX)
    assert bead.tolist() == [0, 7, 0] and nclass == 8
    for bad in ([0], [0, 1, 1], [0, 9], [0, 8], [-2, 0]):
        with pytest.raises(ValueError):
            RP.haploid_classes(bad, COPY_PTR, COPY_IDX)


# ------------------------------------------------------------------ the step wiring
def test_steps_defaults_unchanged():
    assert RP.STEPS == ('rgs', 'shells', 'radials', 'damid', 'distance_map')
    assert RP.OPTIONAL_STEPS == ('hic',)
    assert RP.FEATURE_STEPS == ('neighbours', 'compaction')
    assert not set(RP.FEATURE_STEPS) & set(RP.STEPS)
    assert RP.DEFAULT_NEIGHBOUR_CUTOFF == 500.0


@pytest.fixture()
def tiny_store(tmp_path):
    from igm_amd.steps import PopulationStore
    p = str(tmp_path / 'tiny.hss')
    xyz = np.random.default_rng(1).normal(0, 100, (3, 2, 3)).astype(f32)
    PopulationStore.create(p, xyz, np.full(3, 10.0, f32), np.zeros(3, np.int32), np.array([0, 0, 1], np.int32),
                           np.array([0, 2, 3], np.int32), np.array([0, 2, 1], np.int32))
    return p


def test_unknown_steps_still_raise(tiny_store, tmp_path):
    with pytest.raises(ValueError, match='unknown report steps'):
        RP.report_population(tiny_store, steps='neighbours,neighbors', out_dir=str(tmp_path / 'qc'))
    assert not (tmp_path / 'qc').exists()


@pytest.mark.parametrize('labels', ['0\n1\n0\n', '0\n', '0\n9\n'])
def test_bad_classes_file_raises_before_anything_is_written(tiny_store, tmp_path, labels):
    f = tmp_path / 'classes.txt'
    f.write_text(labels)
    out = tmp_path / 'qc'
    with pytest.raises(ValueError):
        RP.report_population(tiny_store, steps=('neighbours', 'compaction'), out_dir=str(out), classes=str(f))
    assert not out.exists()
    with pytest.raises(ValueError):
        RP.main([tiny_store, '--steps', 'neighbours', '--classes', str(f), '-o', str(out)])
    assert not out.exists()


def test_bad_neighbour_parameters_raise_before_anything_is_written(tiny_store, tmp_path):
    out = tmp_path / 'qc'
    for kw in ({'neighbour_cutoff': -1.0}, {'neighbour_cutoff': np.inf}, {'min_sep': 0}):
        with pytest.raises(ValueError):
            RP.report_population(tiny_store, steps='neighbours', out_dir=str(out), **kw)
    with pytest.raises(ValueError):
        RP.report_population(tiny_store, steps='compaction', out_dir=str(out), compaction_halfwidth=-1)
    assert not out.exists()


# ------------------------------------------------------------------ the windows of local_compaction
def test_compaction_windows_clip_at_chain_ends():
    # chain (0, 0) = beads 0 2 4 6 8, chain (0, 1) = 1 3 5, chain (1, 0) = bead 7 alone
    chrom = [0, 0, 0, 0, 0, 0, 0, 1, 0]
    copy = [0, 1, 0, 1, 0, 1, 0, 0, 0]
    ptr, idx = RP.compaction_windows(chrom, copy, halfwidth=2)
    rows = [idx[ptr[b]:ptr[b + 1]].tolist() for b in range(9)]
    assert rows == [[0, 2, 4], [1, 3, 5], [0, 2, 4, 6], [1, 3, 5], [0, 2, 4, 6, 8], [1, 3, 5], [2, 4, 6, 8], [7],
                    [4, 6, 8]]
    assert ptr.dtype == np.int32 and idx.dtype == np.int32
    for h in (0, 1, 2, 7):
        p, i = RP.compaction_windows(chrom, copy, h)
        q, j = N.windows(chrom, copy, h)
        assert np.array_equal(p, q) and np.array_equal(i, j)
    p0, i0 = RP.compaction_windows(chrom, copy, 0)
    assert i0.tolist() == list(range(9))  # halfwidth 0: every bead alone


def test_local_rg_oracle_of_a_one_bead_chain_and_a_straight_fibre():
    chrom, copy = [0, 0, 0, 0, 1], [0, 0, 0, 0, 0]
    xyz = pop_of([(0, 0, 0), (10, 0, 0), (20, 0, 0), (30, 0, 0), (7, 7, 7)])
    rg, ptr = N.local_rg(xyz, chrom, copy, 1)
    # windows of 2 beads at the ends (Rg 5), of 3 inside (sqrt(200 / 3)), and the lone bead (0)
    assert np.diff(ptr).tolist() == [2, 3, 3, 2, 1]
    assert np.allclose(rg[:, 0], [5.0, np.sqrt(200 / 3), np.sqrt(200 / 3), 5.0, 0.0], rtol=1e-15, atol=0)
