"""The constructed bond sets of tests/bond_tables.py on the CPU: what the GPU test relies on.

For every (set, natom) that tests/test_bond_tables_gpu.py uses, as tests/test_small_models.py
does for the size sweep: the fp64 oracle and brute_forces agree (forces 1e-12 max|F|,
energies rtol 1e-12), an honest float32 evaluation stays 10x under the GPU test's f32
bound, and every property the set was built for holds."""
import numpy as np
import pytest

import bond_tables as bt
import oracle
import small_models as sm
from igm_amd import model as M


def test_rest_cap_is_the_carve():
    """the docstring's hand derivation, the Python carve and the edges the set straddles"""
    assert bt.rest_cap_py(2048) == bt.REST_CAP[2048] == 36688
    assert bt.rest_cap_py(3072) == bt.REST_CAP[3072] == 17232
    for natom, npad in ((1100, 2048), (2100, 3072)):
        edge = bt.REST_EDGE[natom]
        assert ((2 * edge + 7) & ~7) <= bt.REST_CAP[npad] < ((2 * (edge + 1) + 7) & ~7)
        assert bt.REST_CAP[npad] < 0xFFFF  # the other clause never binds
    assert (bt.REST_EDGE[1100], bt.REST_EDGE[2100]) == (18344, 8616)


@pytest.mark.parametrize('name,natom', bt.all_cases())
def test_oracle_matches_brute_force_and_f32_has_headroom(name, natom):
    c = bt.case(name, natom)
    radii, flags, shared, ptr, sb = c.args()
    fo, eo = oracle.mstep_forces(c.prm, c.x, radii, flags, shared, ptr, sb, sm.EVF, sm.ENVF, nthreads=4)
    fb, eb, parts = bt.brute(c, parts=True)
    print('%s %d: max|dF| %.3g of max|F| %.3g' % (name, natom, np.abs(fo - fb).max(), np.abs(fb).max()))
    assert np.all(np.isfinite(fo)) and np.all(np.isfinite(fb))
    assert np.abs(fo - fb).max() <= 1e-12 * np.abs(fb).max()
    assert np.allclose(eo[:, 1:5], eb, rtol=1e-12, atol=0.0)
    assert np.allclose(eo[:, 0], eb.sum(axis=1), rtol=1e-12, atol=0.0)
    f32, _ = bt.brute(c, np.float32)
    h = 1e-5 * np.linalg.norm(fb) / np.linalg.norm(f32 - fb)
    print('%s %d: f32 headroom %.0f' % (name, natom, h))
    assert h >= 10
    # the GPU test's own bound on the atoms of the highest-type bond: per atom, 1e-5 of the
    # summed magnitudes of the atom's terms
    worst = np.inf
    for s, pair in enumerate(c.hi):
        for a in pair:
            if not (sm.struct_flags(c.atoms, s)[a] & M.IGM_ATOM_FIXED):
                mag = parts[s]['mag'][a] + parts[s]['mag_pair'][a]
                worst = min(worst, 1e-5 * mag / max(np.linalg.norm(f32[s, a] - fb[s, a]), 1e-300))
    print('%s %d: f32 per-atom headroom on the top-type bond %.0f' % (name, natom, worst))
    assert worst >= 10


@pytest.mark.parametrize('counts', [(4097, 4097, 4097), (8, 8, 9000)])
def test_refusal_inputs_have_their_type_counts(counts):
    c = bt.types_counts(257, counts)
    assert [len(np.unique(bt.keys(c.bonds(s)))) for s in range(3)] == list(counts)


@pytest.mark.parametrize('name,natom', bt.all_cases())
def test_constructed_properties(name, natom):
    c = bt.case(name, natom)
    fb, _, parts = bt.brute(c, parts=True)
    assert len(c.x) == len(c.ntype) == len(c.hi) == len(c.lo)
    for s in range(len(c.x)):
        b = c.bonds(s)
        i, j, low = bt.partners(b)
        assert np.all(i != j) and i.max() < natom and j.max() < natom
        ukeys = np.unique(bt.keys(b))
        assert len(ukeys) == c.ntype[s], (s, len(ukeys))
        act, r = bt.active(c.x[s], b), bt.lengths(c.x[s], b)
        for which, pair, key, lower in (('hi', c.hi[s], ukeys[-1], True), ('lo', c.lo[s], ukeys[0], False)):
            rows = np.flatnonzero((bt.keys(b) == key) & (((i == pair[0]) & (j == pair[1])) | ((i == pair[1]) & (j == pair[0]))))
            assert len(rows) >= 1, (which, s)
            assert np.all(low[rows] == lower) and np.all(act[rows]), (which, s)
            if lower:
                assert np.all(r[rows] < b['r0'][rows])
            if not name.startswith('degrees'):
                assert np.count_nonzero(bt.keys(b) == key) == 1  # the type's only bond
                # the bond's own force on its two atoms (its only other bonds there may cancel part of it)
                g = 2.0 * float(b['k'][rows[0]]) * abs(r[rows[0]] - float(b['r0'][rows[0]]))
                assert g > 1.0
            for a in pair:
                if not (sm.struct_flags(c.atoms, s)[a] & M.IGM_ATOM_FIXED):
                    assert np.linalg.norm(parts[s]['bond'][a]) > 0.0
        assert b['r0'].max() == bt.R_HI and b['r0'].min() == bt.R_LO
        deg = bt.degrees(b, natom)
        if name.startswith('degrees'):
            assert sorted(c.named.values()) == [0, 1, 3, 4, 5, 31, 32, 33, 64]
            assert (c.named[0], c.named[63], c.named[64], c.named[natom - 2], c.named[natom - 1]) == (33, 32, 31, 64, 0)
            for atom, d in c.named.items():
                assert deg[atom] == d, (atom, deg[atom])
                order = bt.entry_order(b, atom)
                assert len(order) == d and np.all(act[order[17:]])  # so every entry from 30 on
                if d >= 31:
                    assert np.count_nonzero(~act[order[:17]]) >= 3  # the idle MID bonds (and maybe a slack polymer bond), inside the mask
        if name.startswith('hub_'):
            (hub, d), = c.named.items()
            assert hub == (natom - 1 if name == 'hub_dummy' else (natom - 1) // 2)
            assert deg[hub] == d and d == min(600, natom - 4) + bt.degrees(c.shared, natom)[hub]
            mine = (i == hub) | (j == hub)
            assert np.count_nonzero(low & mine) > 100 and np.count_nonzero(~low & mine) > 100
            assert np.count_nonzero(i == hub) > 100 and np.count_nonzero(j == hub) > 100
            assert deg.max() == d
        if name == 'duplicates':
            def count(p, q):
                return np.count_nonzero((i == p) & (j == q))
            a, bb = c.named['both']
            assert count(a, bb) == 2 and np.count_nonzero((c.shared['i'] == a) & (c.shared['j'] == bb)) == 1
            assert count(*c.named['triple']) == 3
            e, f = c.named['swapped']
            assert count(e, f) == 1 and count(f, e) == 1
        if name == 'rest_cap':
            assert len(b) == c.named['total'] - 2 + s and deg.sum() == 2 * len(b)
        if name.startswith('types') and c.ntype[s] >= 512:
            k = bt.keys(bt.mk([0] * 5, [1] * 5, [bt.DUAL[0], bt.DUAL[0], np.nextafter(bt.DUAL[0], np.float32(1e4)),
                                                bt.DUAL[0], np.float32(310.0)],
                              [bt.DUAL[1], np.nextafter(bt.DUAL[1], np.float32(2)), bt.DUAL[1], np.float32(0.9), bt.DUAL[1]]))
            assert len(np.unique(k)) == 5 and np.all(np.isin(k, ukeys))
        if c.ntype[s] >= 8 and not name.startswith(('degrees', 'hub', 'dup', 'rest')):
            dual = bt.keys(b) == bt.keys(bt.mk([0], [1], *bt.DUAL))[0]
            assert np.count_nonzero(dual & low) >= 1 and np.count_nonzero(dual & ~low) >= 1
    if name == 'mixed512_513_3':
        assert c.shared is None and c.ntype == [512, 513, 3]
    if name == 'shared_only':
        assert c.ptr is None and c.sb is None
    if name == 'mixed8_9_8':
        assert c.ntype == [8, 9, 8]
