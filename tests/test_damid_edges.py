"""CPU half of the DamID edge tests: every input of tests/damid_edges.py is the edge it claims, and
the restatements the GPU half compares the kernels with equal the reference's own output
(tests/golden/damid_edges_golden.npz, the reference run on these very inputs)."""
import functools

import numpy as np
import pytest

import damid_edges as E
import nuclear_bodies as NB
from conftest import load_golden

f32 = np.float32


@pytest.fixture(scope='module')
def gold():
    return load_golden('damid_edges_golden.npz')


@functools.lru_cache(maxsize=None)
def expected(name):
    return E.expected(E.golden_cases()[name])


def bits(a):
    return np.asarray(a, f32).view(np.uint32)


# ---------------------------------------------------------------------------- the reference golden
def test_golden_inputs_are_the_builders(gold):
    assert list(gold['cases']) == list(E.golden_cases())
    for S in E.S_GOLDEN:
        assert np.array_equal(gold['pop_s%d' % S], E.population(S))


@pytest.mark.parametrize('name', list(E.golden_cases()))
def test_oracle_equals_the_reference(gold, name):
    """oracle.asteps.damid_actdist on 1 to 4 copies, both shapes, both it_corr, two contact ranges"""
    rows, res = expected(name)
    assert np.array_equal(rows['loc'], gold[name + '_loc'])
    assert np.array_equal(bits(rows['dist']), bits(gold[name + '_dist']))
    assert np.array_equal(bits(rows['prob']), bits(gold[name + '_prob']))
    assert np.array_equal(res['p'], gold[name + '_p64'])
    has = res['o'] >= 0
    assert np.array_equal(res['ad'][has], gold[name + '_ad64'][has], equal_nan=True)
    assert np.all(gold[name + '_ad64'][~has] == 2)


@pytest.mark.parametrize('name', list(E.golden_cases()))
def test_variant_without_a_mistake_is_the_oracle(name):
    rows, res = expected(name)
    vrows, vres = E.variant(E.golden_cases()[name])
    assert rows.tobytes() == vrows.tobytes()
    for k in ('p', 'pnow', 'ad'):
        assert np.array_equal(res[k], vres[k], equal_nan=True)
    assert np.array_equal(res['o'], vres['o']) and np.array_equal(res['nrows'], vres['nrows'])


def test_select_restatement_equals_the_reference(gold):
    from test_restraints_gpu import select_restatement
    xyz, radii, rows, want = E.select_traps()
    sel = np.zeros(gold['select_sel'].shape, bool)
    for s in range(xyz.shape[0]):
        for q in range(len(rows)):
            sel[s, q] = select_restatement(xyz[s], radii, rows[q:q + 1], E.SEL_ABC, 0.0)[rows['loc'][q]]
    assert np.array_equal(sel, gold['select_sel'])
    assert np.array_equal(sel[0], want) and sel[1].all() and not sel[2].any()


# ---------------------------------------------------------------------------- genome and radius
def test_genome_is_the_edge():
    assert sorted(E.NCOPY.tolist()) == [0, 1, 2, 2, 3, 4]
    assert sorted(E.COPY_IDX.tolist()) == list(range(E.NBEAD))
    assert np.any(np.diff(E.COPY_IDX) < 0) and np.any(np.abs(np.diff(E.COPY_IDX)) > 1)
    for I in (1, 2, 3, 5):
        ii = E.COPY_INDEX[I]
        assert ii != sorted(ii) or I == 1
        assert len(set(E.RADII[ii].tolist())) == len(ii)           # every copy another radius
    assert E.COPY_INDEX[5][0] > E.COPY_INDEX[5][1]
    for I in (0, 1, 2, 3):                                         # divisor exactly 1 at contact range 0
        assert f32((E.SPHERE - float(E.RADII[E.COPY_INDEX[I][0]])) ** 2) == 1.0
    a, b, c = E.ELLIPSOID
    assert min(a, b, c) * 1.5 < sorted((a, b, c))[1] and sorted((a, b, c))[1] * 1.5 < max(a, b, c)


@pytest.mark.parametrize('S', E.S_LIST)
def test_each_copys_own_radius_changes_rows(S):
    for shape in ('sphere', 'ellipsoid'):
        c = E.ploidy_case(S, shape, 0.05, 0)
        rows, res = E.variant(c)
        wrong, _ = E.variant(c, own_radius=True)
        changed = set()
        for q, I in enumerate(c['loci']):
            sl = E.rows_of(c, res, q)
            if rows[sl].tobytes() != wrong[sl].tobytes():
                changed.add(int(I))
        assert {1, 2, 3} <= changed and 0 not in changed, (S, shape, changed)


# ---------------------------------------------------------------------------- radix select
def select_trace(u, m):
    """buckets of the 4-pass 8-bit radix select for ascending rank m over the bit patterns u:
    [(bucket, rank within the bucket, bucket size)] per pass"""
    out, cand = [], np.asarray(u, np.uint32)
    for shift in (24, 16, 8, 0):
        byte = (cand >> np.uint32(shift)) & np.uint32(255)
        hist = np.bincount(byte, minlength=256)
        b = 0
        while m >= hist[b]:
            m -= hist[b]
            b += 1
        out.append((b, m, int(hist[b])))
        cand = cand[byte == b]
    return out, int(cand[0])


@pytest.mark.parametrize('S', E.S_LIST)
def test_radix_case_is_the_edge(S):
    c = E.radix_case(S)
    _, res = E.expected(c)
    proven = 0
    for q, I in enumerate(c['loci']):
        u = E.keys(c, int(I)).view(np.uint32)
        n = len(u)
        m = n - 1 - int(res['o'][q])                    # the ascending rank the kernel selects
        trace, sel = select_trace(u, m)
        assert sel == E.T_KEY == int(np.sort(u)[m])
        assert f32(np.sqrt(np.float64(np.array([sel], np.uint32).view(f32)[0]))) == f32(res['ad'][q])
        other = u[u != sel]
        ok = (np.count_nonzero(u == sel) > 1
              and all(np.any((other >> np.uint32(sh)) == (sel >> sh)) for sh in (24, 16, 8))
              and any(b == 255 for b, _, _ in trace) and any(b == 0 for b, _, _ in trace)
              and 0 < trace[3][1] < trace[3][2] - 1)
        proven += ok
    assert proven >= 1
    if S > 1:
        assert proven == 3


def test_special_keys_are_selected_each():
    for it in (0, 1, 2):
        c = E.special_case(it)
        rows, res = E.expected(c)
        k = E.keys(c, 0)
        assert np.array_equal(k.view(np.uint32)[:6], bits([0.0, 2.0 ** -140, 0.25, 1.0, 9.0, np.inf]))
        assert 0 < k[1] < np.finfo(f32).tiny                         # an f32 subnormal
        assert np.isnan(k[6]) and np.isnan(k[7]) and k.view(np.uint32)[7] >> 31 == 1
        assert res['o'][:9].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 7]
        assert np.all(np.isnan(res['ad'][:2])) and np.all(np.isnan(rows['dist'][:2]))   # NaN sorts first
        assert np.array_equal(bits(rows['dist'][:2]), bits([np.nan, np.nan]))          # the text 'nan'
        assert res['ad'][2:9].tolist() == [np.inf, 3.0, 1.0, 0.5, 2.0 ** -70, 0.0, 0.0]
        assert np.isinf(rows['dist'][2]) and rows['dist'][6] == 0.0
        assert np.all(res['pnow'][:9] == 0.375)
        assert np.array_equal(res['p'][:9], c['p_exp'][:9].astype(np.float64))         # pnow == plast: p = p_exp


def test_count_threshold_is_in_the_data():
    c = E.special_case(1)
    k = E.keys(c, 1)
    one = f32(1.0)
    assert np.count_nonzero(k == one) == 2
    assert np.count_nonzero(k == np.nextafter(one, f32(0))) == 2
    assert np.count_nonzero(k == np.nextafter(one, f32(2))) == 2
    _, res = E.variant(c)
    _, wrong = E.variant(c, count_gt=True)
    assert np.all(res['pnow'][9:] == 5 / 8) and np.all(wrong['pnow'][9:] == 3 / 8)
    assert not np.array_equal(res['p'][9:11], wrong['p'][9:11])
    # the radix populations hold 1.0 itself at every size (pnow is recorded whatever it_corr is)
    for S in E.S_LIST[1:]:
        c = E.radix_case(S)
        _, res = E.variant(c)
        _, wrong = E.variant(c, count_gt=True)
        assert np.any(res['pnow'] != wrong['pnow'])


# ---------------------------------------------------------------------------- cleanProbability
@pytest.mark.parametrize('S', (64, 65, 1025))
def test_clean_probability_branches(S):
    c = E.ploidy_case(S, 'sphere', 0.0, 1)
    rows, res = E.expected(c)
    pl = c['plast'].astype(np.float64)
    for v in (0.0, float(f32(0.99)), 1.0, 1.5):
        assert np.any(pl == v)
    same = pl == res['pnow']
    if S == 64:
        assert same.any() and np.all(same[4 * 6:5 * 6] | (res['pnow'] != f32(res['pnow']))[4 * 6:5 * 6])
        assert np.array_equal(res['p'][same & (pl > 0)], c['p_exp'][same & (pl > 0)].astype(np.float64))
    none = res['p'] == 0
    assert none.any() and np.all(res['o'][none] == -1)
    first = np.cumsum(res['nrows']) - res['nrows']
    assert np.all(rows['dist'][first[none]] == 2.0) and np.all(rows['prob'][first[none]] == 0.0)
    # it_corr 0: the tiny p, the clamp, and it_corr 2 the same as 0
    c0 = E.ploidy_case(S, 'sphere', 0.0, 0)
    rows0, res0 = E.expected(c0)
    tiny = c0['p_exp'] == f32(1e-7)
    assert np.all(res0['o'][tiny] == 0) and np.all(rows0['prob'][first[tiny]] == 0.0)
    for q in np.where(tiny)[0]:
        assert res0['ad'][q] == np.sqrt(np.float64(E.keys(c0, int(c0['loci'][q])).max()))
    nS = res0['nrows'] * S
    for v in (1.0, 1.5):
        assert np.all(res0['o'][c0['p_exp'] == f32(v)] == nS[c0['p_exp'] == f32(v)] - 1)
    c2 = E.ploidy_case(S, 'sphere', 0.0, 2)
    rows2, res2 = E.expected(c2)
    assert rows2.tobytes() == rows0.tobytes() and res2.tobytes() == res0.tobytes()
    assert rows.tobytes() != rows0.tobytes()


# ---------------------------------------------------------------------------- order index and decimals
def test_order_index_ties_are_in_the_data():
    seen = set()
    for S in (4, 5):
        c = E.order_case(S)
        rows, res = E.variant(c)
        wrong, wres = E.variant(c, half_up=True)
        for q, I in enumerate(c['loci']):
            n = int(res['nrows'][q]) * S
            x = n * float(c['p_exp'][q])
            if x % 1 == 0.5:
                k = int(x)
                assert res['o'][q] == k + (k % 2) and wres['o'][q] == k + 1
                sl = E.rows_of(c, res, q)
                if k % 2 == 0:
                    assert rows[sl].tobytes() != wrong[sl].tobytes()       # another key
                    seen.add((n, 'even'))
                else:
                    seen.add((n, 'odd'))
    assert {(4, 'even'), (12, 'even'), (20, 'even')} <= seen and {(4, 'odd'), (12, 'odd'), (20, 'odd')} <= seen


def test_decimal_ties_are_in_the_data():
    c = E.decimal_case()
    rows, res = E.variant(c)
    wrong, _ = E.variant(c, dec_half_up=True)
    odd = 2 * c['loci'] + 1
    assert np.array_equal(res['ad'], odd / 64.0) and np.array_equal(res['p'], odd / 64.0)
    differs = bits(rows['dist']) != bits(wrong['dist'])
    for v in (1, 5, 9, 13, 37):
        assert differs[v // 2]
    for v in (3, 7, 11, 99):
        assert not differs[v // 2]
    assert np.array_equal(differs, bits(rows['prob']) != bits(wrong['prob']))
    # the ploidy cases carry the same ties in prob
    c = E.ploidy_case(5, 'sphere', 0.05, 0)
    rows, _ = E.variant(c)
    wrong, _ = E.variant(c, dec_half_up=True)
    assert np.any(bits(rows['prob']) != bits(wrong['prob']))


def test_every_semiaxis_decides_a_locus_alone():
    a, b, cc = E.ELLIPSOID
    for cr in (0.05, 0.0):
        c = E.axes_case(cr)
        rows, res = E.variant(c)
        for perm, same_locus in (((a, cc, b), 1), ((cc, b, a), 2), ((b, a, cc), 3)):
            wrong, _ = E.variant(c, param=perm)
            for q, I in enumerate(c['loci']):
                sl = E.rows_of(c, res, q)
                if int(I) == same_locus:
                    assert rows[sl].tobytes() == wrong[sl].tobytes()
            changed = {int(I) for q, I in enumerate(c['loci'])
                       if rows[E.rows_of(c, res, q)].tobytes() != wrong[E.rows_of(c, res, q)].tobytes()}
            assert {1, 2, 3} - {same_locus} <= changed


def test_list_shapes():
    for n in (1, 255, 256, 257):
        c = E.nloci_case(n)
        assert len(c['loci']) == n and (n == 1 or np.all(np.diff(c['loci'][:64]) < 0))
        rows, res = E.expected(c)
        assert len(rows) == n
    c = E.zero_copy_case()
    assert [len(E.copies(c, int(I))) for I in c['loci']] == [2, 0, 4, 0, 1]
    c = E.ploidy_case(5, 'sphere', 0.05, 1)
    assert c['loci'][:6].tolist() == E.LOCI_ORDER and E.LOCI_ORDER.count(1) == 2


# ---------------------------------------------------------------------------- igm_damid_select
def test_select_traps_are_on_the_threshold():
    xyz, radii, rows, want = E.select_traps()
    A = np.array(E.SEL_ABC) - 0.5
    assert np.array_equal(A, E.SEL_AXES)
    x = xyz[0].astype(np.float64)
    v = ((x[:, 0] ** 2 / A[0] ** 2) + (x[:, 1] ** 2 / A[1] ** 2)) + x[:, 2] ** 2 / A[2] ** 2
    d = rows['dist'].astype(np.float64)
    n = 9 * len(E.TRAP_D)
    assert np.all(np.square(xyz[0, :n]).astype(np.float64) == x[:n] ** 2)    # the f32 squares are exact
    assert np.all(v[:n:3] == d[:n:3] ** 2) and np.all(v[1:n:3] < d[1:n:3] ** 2) and np.all(v[2:n:3] > d[2:n:3] ** 2)
    assert want[:n].tolist() == [True, False, True] * (n // 3)
    # the f32 square of d against the f64 square
    dn, up = rows['dist'][n], rows['dist'][n + 1]
    vn, vu = [np.float64(np.square(xyz[0, n + k, 1])) for k in (0, 1)]
    assert vn == np.float64(f32(dn * dn)) < np.float64(dn) ** 2 and not want[n]
    assert vu == np.float64(f32(up * up)) > np.float64(up) ** 2 and want[n + 1]


def test_select_rows_are_the_edge():
    assert E.ROW_COUNTS == (0, 1, 63, 64, 65, 255, 256, 257, 513)
    for n in E.ROW_COUNTS[1:]:
        r = E.select_rows(n, 257, 'last_wave')
        can = r['dist'] == 1.0
        assert can.any() and np.all(np.where(can)[0] >= 64 * ((n - 1) // 64))
        r = E.select_rows(n, 257, 'lanes_0_63')
        assert set((np.where(r['dist'] == 1.0)[0] % 64).tolist()) <= {0, 63}
    r = E.select_rows(513, 257, 'two_thirds')
    hit_beads = r['loc'][r['dist'] == 1.0]
    counts = np.bincount(hit_beads)
    assert counts.max() >= 2                                      # two rows name one bead
    for S, natom in ((1, 257), (3, 255), (70, 1)):
        x = E.select_population(S, natom).astype(np.float64)
        A = np.array(E.SEL_AXES)
        v = (x ** 2 / A ** 2).sum(-1)
        assert (np.any(v >= 1) and np.any(v < 1)) or natom == 1
    j = E.with_junk(E.select_rows(65, 257, 'two_thirds'), 257)
    assert len(j) == 69 and sorted(j['loc'][[0, 33, 34, 68]].tolist()) == [-1, -1, 257, 257]
    assert E.env_bit(3) == 0x80 and E.env_bit(0) == 0x10
    b = E.base_pattern(257, E.env_bit(3))
    assert np.any(b & 0x80) and np.any(~b & 0x80) and np.any(b & ~np.uint32(0x80))


# ---------------------------------------------------------------------------- exp_map
def test_maps_differ_and_are_assigned_unsorted():
    M = E.maps()
    assert [int(m['nvoxel'][0]) for m in M] == [11, 13, 11]
    assert len({float(m['grid'][0]) for m in M}) == 3 and len({tuple(m['center'].tolist()) for m in M}) == 3
    sm = E.struct_map(65)
    assert set(sm.tolist()) == {0, 1, 2} and np.any(np.diff(sm) < 0) and np.any(np.diff(sm) > 0)


@pytest.mark.parametrize('S', E.EXP_S[1:])
def test_voxel_rounding_edges_are_in_the_data(S):
    M, sm = E.maps(), E.struct_map(S)
    x = E.exp_population(S, 'off')
    seen, halves = set(), set()
    for s in range(S):
        m = M[sm[s]]
        n = int(m['nvoxel'][0])
        v, u = E.voxel_index(x[:, s], m)
        for name, val in (('0', 0), ('n-1', n - 1), ('-1', -1), ('n', n)):
            if np.any(v == val):
                seen.add(name)
        half = (u % 1) == 0.5
        k = np.floor(u[half]).astype(np.int64)
        assert np.all(v[half] == k + (k % 2))                     # half to even
        halves |= {('even' if kk % 2 == 0 else 'odd') for kk in k.tolist()}
        assert np.all(np.floor(u[half] + 0.5)[k % 2 == 0] != v[half][k % 2 == 0])    # half-up differs
    assert seen == {'0', 'n-1', '-1', 'n'} and halves == {'even', 'odd'}
    xc = E.exp_population(S, 'centre')
    for s in range(S):
        v, u = E.voxel_index(xc[:, s], M[sm[s]])
        assert np.all(u == v)


@pytest.mark.parametrize('S', E.EXP_S)
def test_exp_forms_and_thresholds(S):
    M, sm = E.maps(), E.struct_map(S)
    lam = nucl = None
    for kind in ('centre', 'off'):
        x = E.exp_population(S, kind)
        kl = np.stack([NB.snormsq_exp(x[:, s], M[sm[s]], False)[0] for s in range(S)])
        kn = np.stack([NB.snormsq_exp(x[:, s], M[sm[s]], True)[0] for s in range(S)])
        inside = np.stack([NB.snormsq_exp(x[:, s], M[sm[s]], True)[1] for s in range(S)])
        assert np.array_equal(kl[~inside], kn[~inside])                       # outside the grid they agree
        if kind == 'centre':
            assert np.array_equal(kl, kn)
            lam, nucl = kl, kn
        elif S > 1:
            assert np.any(kl[inside] != kn[inside])                           # exchanged forms would show
    if S > 1:
        assert np.any(nucl == E.EXP_CR[0]) and np.any(nucl == 0.0) and not np.any(nucl == E.EXP_CR[1])
        assert len(np.unique(nucl)) < nucl.size // 2                          # heavy ties
        # the map of a structure matters: map 0 for everyone gives other keys
        x = E.exp_population(S, 'centre')
        k0 = np.stack([NB.snormsq_exp(x[:, s], M[0], True)[0] for s in range(S)])
        assert np.any(k0 != nucl)


def test_volume_traps_are_on_the_threshold():
    xyz, T = E.volume_traps()
    M = list(E.maps())
    for s in range(3):
        v, inside = NB.snormsq_exp(xyz[s], M[s])
        assert inside.all() and np.array_equal(v, T[s].astype(np.float64) ** 2)
        rows = E.volume_trap_rows(T[s])
        sel = NB.volume_select_rows(xyz[s:s + 1], rows, M, [s])[0]
        assert sel.tolist() == [False, True, False] * T.shape[1]
    t = T[0, -1]
    assert np.float64(f32(t * t)) > np.float64(t) ** 2        # the f32 square of d would select it
