"""The NumPy restatement of the violation record (tests/violations_ref.py) against the reference:
bit-equal ratios and equal records on the edge golden (make_golden_violations.py) and on the
demo structures (violations_golden.npz), and every one-line mistake the restatement can make on
purpose changes the record of the edge golden's inputs."""
import numpy as np
import pytest

import mstep_fixtures as F
import violations_ref as VR
from conftest import load_golden


@pytest.fixture(scope='module')
def edges():
    return load_golden('violations_edges_golden.npz')


def bond_case(g, c, wrong=None):
    return VR.bond_ratios(g[c + '_pos'], g[c + '_radii'], g[c + '_i'], g[c + '_j'], g[c + '_r0'], g[c + '_k'],
                          g[c + '_lower'], float(g[c + '_cr']), wrong=wrong)


def env_case(g, c, wrong=None):
    return VR.envelope_ratios(g[c + '_pos'], g[c + '_radii'], g[c + '_abc'], float(g[c + '_k']),
                              float(g[c + '_scale']), wrong=wrong)


def all_records(g, wrong=None):
    tol = float(g['tol'])
    out = {c: VR.record(bond_case(g, c, wrong), tol, wrong) for c in g['bond_cases']}
    out.update({c: VR.record(env_case(g, c, wrong), tol, wrong) for c in g['env_cases']})
    return out


def test_golden_holds_the_edges(edges):
    """what make_golden_violations.py asserts when it writes the file, checked on the file"""
    g = edges
    assert len(g['bond_cases']) == 10 and len(g['env_cases']) == 4
    natoms = sum(len(g[c + '_pos']) for c in list(g['bond_cases']) + list(g['env_cases']))
    assert natoms < 15000
    v = g['up100_ratios']
    assert np.array_equal(v, np.arange(251) / 100.0)
    rec = g['up100_rec']
    assert rec[99] == 2 and rec[100] == 150 and rec[102] == 245 and rec[103] == 251  # 0.99 and 1.0; tol itself is no violation
    plain = np.minimum((v[:101] * 100).astype(int), 99)
    truth = np.repeat(np.arange(100), rec[:100])
    assert set(np.nonzero(plain != truth)[0]) >= {29, 58, 35, 41, 47, 69, 70, 82, 83, 94, 95}
    assert g['lo100_ratios'][100] == 1.0 and np.all(g['lo100_ratios'][101:] == 0)
    assert np.all(g['zero_d_ratios'] == 0) and g['zero_d_rec'][0] == 8 and g['zero_d_rec'][103] == 8
    for c in g['env_cases']:
        rec = g[c + '_rec']
        assert np.count_nonzero(rec[:100]) >= 20
        assert (rec[100] >= 20) == (float(g[c + '_k']) > 0)


def test_restatement_equals_edge_golden(edges):
    g = edges
    for c in g['bond_cases']:
        assert bond_case(g, c).tobytes() == g[c + '_ratios'].tobytes(), c
    for c in g['env_cases']:
        assert env_case(g, c).tobytes() == g[c + '_ratios'].tobytes(), c
    for c, rec in all_records(g).items():
        assert np.array_equal(rec, g[c + '_rec']), c


def test_restatement_equals_demo_golden():
    """the ratios of the ten demo structures (make_golden.py G6), every class, bit for bit"""
    pop, g3 = F.load()
    viol = load_golden('violations_golden.npz')
    atoms, poly, prm, chrom = F.demo_model(pop)
    for s in range(10):
        x = F.struct_major(pop, [s], atoms.n)[0]
        hic, cls = F.hic_bonds_from_golden(g3, atoms.radii, s)
        parts = {'Polymer': poly, 'interHiC': hic[cls == 1], 'intraHiC': hic[cls == 2]}
        for name, b in parts.items():
            v = VR.bond_ratios(x, atoms.radii, b['i'], b['j'], b['r0'], b['k'], False, 2.0)
            assert v.tobytes() == viol['vs_%s_%d' % (name, s)].tobytes(), (name, s)
        v = VR.envelope_ratios(x[:atoms.nbead], atoms.radii[:atoms.nbead], (5500.0,) * 3, 1.0, 550.0)
        assert v.tobytes() == viol['vs_Envelope_%d' % s].tobytes(), s
        assert VR.default_scale((5500.0,) * 3) == 0.1 * np.mean([5500.0] * 3)


@pytest.mark.parametrize('wrong', VR.WRONG)
def test_wrong_variant_changes_the_golden_record(edges, wrong):
    """the golden's inputs catch each mistake: some case's record differs from the reference's"""
    g = edges
    bad = all_records(g, wrong)
    differ = [c for c, rec in bad.items() if not np.array_equal(rec, g[c + '_rec'])]
    assert differ, wrong
    expect = {'int_bin': 'up100', 'ge_tol': 'up100', 'ge_one': 'up100', 'swap_bounds': 'lo100',
              'no_zero_guard': 'zero_d', 'r0_for_radii': 'radii_cr105', 'pos_k_form': 'ell_k-1',
              'mean_semiaxis': 'ell_k+1'}
    assert expect[wrong] in differ, (wrong, differ)


def test_model_record_assembles_classes_and_envelopes(edges):
    """model_record on one structure that holds two golden bond cases as two classes and one
    golden envelope: the rows are the golden records"""
    from igm_amd._lib import IGM_ATOM_ENV0, LOWER_BOUND_BIT, bond_dtype
    g = edges
    n1, n2, n3 = len(g['lo100_pos']), len(g['radii_cr105_pos']), len(g['ell_k+1_pos'])
    x = np.concatenate([g['lo100_pos'], g['radii_cr105_pos'], g['ell_k+1_pos']])
    radii = np.concatenate([g['lo100_radii'], g['radii_cr105_radii'], g['ell_k+1_radii']])
    flags = np.zeros(len(x), np.uint32)
    flags[n1 + n2:] = IGM_ATOM_ENV0
    b = np.zeros(len(g['lo100_i']) + len(g['radii_cr105_i']), bond_dtype)
    m = len(g['lo100_i'])
    b['i'][:m], b['j'][:m] = g['lo100_i'], g['lo100_j'].astype(np.uint32) | LOWER_BOUND_BIT
    b['i'][m:], b['j'][m:] = g['radii_cr105_i'] + n1, g['radii_cr105_j'] + n1
    b['r0'] = np.concatenate([g['lo100_r0'], g['radii_cr105_r0']])
    b['k'] = np.concatenate([g['lo100_k'], g['radii_cr105_k']])
    cls = np.concatenate([np.zeros(m, np.int32), np.ones(len(b) - m, np.int32)])
    rec = VR.model_record(x, radii, flags, b, cls, [0.0, 1.05], [(g['ell_k+1_abc'], 1.0)], 0.05,
                          env_scale=[float(g['ell_k+1_scale'])])
    assert np.array_equal(rec[0], g['lo100_rec']) and np.array_equal(rec[1], g['radii_cr105_rec'])
    assert np.array_equal(rec[2], g['ell_k+1_rec']) and n3 == 2000
