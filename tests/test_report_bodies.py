"""The seeded nuclear bodies without a GPU: the NumPy oracle tests/report_bodies_ref.py on
hand-made cases whose answers are written out, the host-side functions of igm_amd.report
(seed_beads, body_profiles) and the refusals of the seeded_bodies report step."""
import numpy as np
import pytest

import report_bodies_ref as B
from igm_amd import report as RP

f32 = np.float32
COPY_PTR = np.array([0, 2, 3, 5], np.int32)          # three loci: two copies, one, two
COPY_IDX = np.array([0, 3, 1, 2, 4], np.int32)


def pop_of(points):
    """(n, 1, 3): one structure"""
    return np.asarray(points, f32)[:, None, :]


# ------------------------------------------------------------------ the oracle, by hand
TRIANGLES = [(0, 0, 0), (10, 0, 0), (1, 0, 0), (100, 0, 0), (10, 1, 0), (0, 1, 0), (11, 0, 0)]


def test_two_triangles_and_a_stray_seed():
    """ranks 0, 2, 5 and 1, 4, 6 form two right triangles with legs 1 (the hypotenuse is
    not a link at cutoff 1, the legs are); rank 3 is alone"""
    res = B.seed_bodies(pop_of(TRIANGLES), np.arange(7), cutoff=1.0, min_size=3)
    assert res['label'].tolist() == [[0, 1, 0, 3, 1, 0, 1]]
    assert res['nbody'].tolist() == [2] and res['size'].tolist() == [[3, 3]]
    third = np.float64(1.0) / 3.0
    assert np.array_equal(res['centre'][0], [[third, third, 0.0], [np.float64(31.0) / 3.0, third, 0.0]])
    one = B.seed_bodies(pop_of(TRIANGLES), np.arange(7), cutoff=1.0, min_size=1)
    assert one['nbody'].tolist() == [3] and one['size'].tolist() == [[3, 3, 1]]   # ascending label: 0, 1, 3
    assert one['centre'][0, 2].tolist() == [100.0, 0.0, 0.0]
    four = B.seed_bodies(pop_of(TRIANGLES), np.arange(7), cutoff=1.0, min_size=4, max_bodies=2)
    assert four['nbody'].tolist() == [0] and not four['size'].any() and np.isnan(four['centre']).all()
    wide = B.seed_bodies(pop_of(TRIANGLES), np.arange(7), cutoff=1.5, min_size=3)  # the hypotenuse links too
    assert wide['label'].tolist() == res['label'].tolist()
    far = B.seed_bodies(pop_of(TRIANGLES), np.arange(7), cutoff=10.0, min_size=3)  # the triangles merge
    assert far['label'].tolist() == [[0, 0, 0, 3, 0, 0, 0]] and far['size'].tolist() == [[6]]


def test_seeds_among_other_beads():
    """only the seeds take part, and their rank is their place in seed_idx"""
    pts = [(50, 50, 50)] * 3 + TRIANGLES + [(0.5, 0, 0)]   # the last bead would bridge nothing: not a seed
    res = B.seed_bodies(pop_of(pts), np.arange(3, 10), cutoff=1.0, min_size=3)
    assert res['label'].tolist() == [[0, 1, 0, 3, 1, 0, 1]]


def test_chain():
    """a chain of five at spacing 0.9, ranks dealt out of order: one component at cutoff 1,
    none at 0.8; without its middle seed two pairs"""
    order = [3, 0, 4, 1, 2]                                # rank r sits at position order[r] of the chain
    pts = [(0.9 * k, 0, 0) for k in order]
    res = B.seed_bodies(pop_of(pts), np.arange(5), cutoff=1.0, min_size=2)
    assert res['label'].tolist() == [[0] * 5] and res['size'].tolist() == [[5]]
    acc = np.float64(0.0)
    for k in order:
        acc = acc + np.float64(f32(0.9 * k))               # rank order
    assert res['centre'][0, 0].tolist() == [acc / 5.0, 0.0, 0.0]
    none = B.seed_bodies(pop_of(pts), np.arange(5), cutoff=0.8, min_size=1)
    assert none['label'].tolist() == [[0, 1, 2, 3, 4]] and none['nbody'].tolist() == [5]
    cut = B.seed_bodies(pop_of(pts), np.array([0, 1, 2, 3]), cutoff=1.0, min_size=2)   # position 2 is rank 4
    assert cut['label'].tolist() == [[0, 1, 0, 1]] and cut['size'].tolist() == [[2, 2]]


def test_coincident_seeds():
    """cutoff 0 links exactly the coincident seeds; a NaN seed is linked to nobody, not even
    to a seed with the same bits"""
    pts = [(1, 2, 3), (4, 4, 4), (1, 2, 3), (np.nan, 0, 0), (4, 4, 4), (1, 2, 3), (np.nan, 0, 0)]
    res = B.seed_bodies(pop_of(pts), np.arange(7), cutoff=0.0, min_size=2)
    assert res['label'].tolist() == [[0, 1, 0, 3, 1, 0, 6]]
    assert res['size'].tolist() == [[3, 2]]
    assert res['centre'][0].tolist() == [[1.0, 2.0, 3.0], [4.0, 4.0, 4.0]]
    lone = B.seed_bodies(pop_of(pts), np.arange(7), cutoff=0.0, min_size=1)
    assert lone['nbody'].tolist() == [4] and np.isnan(lone['centre'][0, 2, 0])


def test_features_by_hand():
    """two structures, the second without a body; 3-4-5 triangles give exact distances"""
    xyz = np.zeros((3, 2, 3), f32)
    xyz[0, 0] = (3, 4, 0)                                  # 5 from the body at the origin, 5 from the other
    xyz[1, 0] = (0, 0, 0)                                  # on the first centre
    xyz[2, 0] = (np.nan, 0, 0)
    centre = np.array([[[0, 0, 0], [6, 8, 0]], [[np.nan] * 3] * 2], np.float64)
    res = B.body_features(xyz, [2, 0], centre, assoc_cutoff=5.0, decay=0.5)
    assert res['nearest'][0].tolist()[0] == 5.0 and np.isnan(res['nearest'][:, 1]).all()
    assert res['nearest'][1, 0] == 0.0 and np.isnan(res['nearest'][2, 0])
    assert res['dist_sum'].tolist()[:2] == [5.0, 0.0] and np.isnan(res['dist_sum'][2])
    assert res['dist_sqsum'].tolist()[:2] == [25.0, 0.0]
    assert res['assoc'].tolist() == [1, 1, 0]
    assert res['tsa_sum'][0] == np.exp(-2.5) + np.exp(-2.5) and res['tsa_sum'][1] == 1.0 + np.exp(-5.0)
    assert np.isnan(res['tsa_sum'][2])
    tight = B.body_features(xyz, [2, 0], centre, assoc_cutoff=np.nextafter(5.0, 0.0), decay=0.0)
    assert tight['assoc'].tolist() == [0, 1, 0] and tight['tsa_sum'].tolist()[:2] == [2.0, 2.0]


# ------------------------------------------------------------------ the host-side functions
def test_seed_beads(tmp_path):
    got = RP.seed_beads([1, 0, 1], COPY_PTR, COPY_IDX)
    assert got.tolist() == [0, 2, 3, 4] and got.dtype == np.int32   # all copies, ascending
    assert RP.seed_beads([0, 1, 0], COPY_PTR, COPY_IDX).tolist() == [1]
    f = tmp_path / 'seeds.txt'
    f.write_text('0\n1\n1\n')
    assert RP.seed_beads(str(f), COPY_PTR, COPY_IDX).tolist() == [1, 2, 4]
    for bad in ([1, 0], [1, 0, 1, 0], [0, 2, 0], [-1, 1, 0], [0, 0, 0]):
        with pytest.raises(ValueError):
            RP.seed_beads(bad, COPY_PTR, COPY_IDX)


def test_body_profiles_by_hand():
    feat = {'dist_sum': np.array([10.0, 4.0, 6.0, 30.0, np.nan]),
            'dist_sqsum': np.array([68.0, 8.0, 18.0, 450.0, np.nan]),
            'assoc': np.array([1, 2, 0, 0, 0], np.int64),
            'tsa_sum': np.array([3.0, 1.5, 0.0, 6.0, np.nan])}
    nbody = np.array([2, 0, 1])                            # two of the three structures have a body
    got = RP.body_profiles(feat, nbody, COPY_PTR, COPY_IDX)
    # beads: mean 5, 2, 3, 15, nan; variance 34 - 25 = 9, 4 - 4 = 0, 9 - 9 = 0, 225 - 225 = 0
    want = np.array([[(5.0 + 15.0) / 2, (3.0 + 0.0) / 2, (0.5 + 0.0) / 2, (1.0 + 2.0) / 2],
                     [2.0, 0.0, 1.0, 0.5],
                     [3.0, 0.0, 0.0, 0.0]])                # the NaN copy is left out of its locus
    assert got.shape == (3, 4) and np.array_equal(got, want)
    assert np.array_equal(got, B.profiles(feat, nbody, COPY_PTR, COPY_IDX))
    # rounding may leave the variance a hair below zero: the standard deviation is then 0
    feat['dist_sqsum'][1] = np.nextafter(8.0, 0.0)
    assert RP.body_profiles(feat, nbody, COPY_PTR, COPY_IDX)[1, 1] == 0.0
    # no structure has a body: NaN, except the TSA column, which is 0
    none = {'dist_sum': np.zeros(5), 'dist_sqsum': np.zeros(5), 'assoc': np.zeros(5, np.int64),
            'tsa_sum': np.zeros(5)}
    got = RP.body_profiles(none, np.zeros(3, np.int32), COPY_PTR, COPY_IDX)
    assert np.isnan(got[:, :3]).all() and not got[:, 3].any()
    assert np.array_equal(got, B.profiles(none, np.zeros(3, np.int32), COPY_PTR, COPY_IDX), equal_nan=True)


def test_defaults_and_the_library():
    """the step is optional, the four defaults are the documented ones, and the library
    exports the two entry points"""
    from igm_amd import _lib
    assert RP.SEED_STEPS == ('seeded_bodies',) and 'seeded_bodies' not in RP.STEPS
    assert (RP.DEFAULT_LINK_CUTOFF, RP.DEFAULT_MIN_BODY_SIZE, RP.DEFAULT_ASSOC_CUTOFF, RP.DEFAULT_TSA_DECAY) == \
        (500.0, 3, 500.0, 0.004)
    lib = _lib.load()
    assert hasattr(lib, 'igm_report_seed_bodies') and hasattr(lib, 'igm_report_body_features')


# ------------------------------------------------------------------ the step's refusals
@pytest.fixture()
def tiny_store(tmp_path):
    from igm_amd.steps import PopulationStore
    p = str(tmp_path / 'tiny.hss')
    xyz = np.random.default_rng(1).normal(0, 100, (3, 2, 3)).astype(f32)
    PopulationStore.create(p, xyz, np.full(3, 10.0, f32), np.zeros(3, np.int32), np.array([0, 0, 1], np.int32),
                           np.array([0, 2, 3], np.int32), np.array([0, 2, 1], np.int32))
    return p


def test_step_without_seeds_names_the_flag(tiny_store, tmp_path):
    out = tmp_path / 'qc'
    with pytest.raises(ValueError, match='--seeds'):
        RP.report_population(tiny_store, steps='seeded_bodies', out_dir=str(out))
    with pytest.raises(ValueError, match='--seeds'):
        RP.main([tiny_store, '--steps', 'seeded_bodies', '-o', str(out)])
    assert not out.exists()


@pytest.mark.parametrize('flags', ['1\n0\n1\n', '1\n', '0\n2\n', '0\n0\n'])
def test_bad_seed_file_raises_before_anything_is_written(tiny_store, tmp_path, flags):
    f = tmp_path / 'seeds.txt'
    f.write_text(flags)
    out = tmp_path / 'qc'
    with pytest.raises(ValueError):
        RP.report_population(tiny_store, steps='seeded_bodies', out_dir=str(out), seeds=str(f))
    with pytest.raises(ValueError):
        RP.main([tiny_store, '--steps', 'seeded_bodies', '--seeds', str(f), '-o', str(out)])
    assert not out.exists()


def test_bad_parameters_raise_before_anything_is_written(tiny_store, tmp_path):
    out = tmp_path / 'qc'
    for kw in ({'link_cutoff': -1.0}, {'link_cutoff': np.inf}, {'min_body_size': 0}, {'assoc_cutoff': np.nan},
               {'assoc_cutoff': -2.0}, {'tsa_decay': -0.1}, {'tsa_decay': np.inf}):
        with pytest.raises(ValueError, match='seeded_bodies'):
            RP.report_population(tiny_store, steps='seeded_bodies', out_dir=str(out), seeds=[1, 1], **kw)
    assert not out.exists()
