"""The A-step edge builder (tests/astep_edges.py) and the CPU oracle on it: the oracle against
the reference's own output for loci with one to four copies, and proof that every input the GPU
tests rely on really is the edge it claims to be.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import astep_edges as E
import oracle
from conftest import load_golden, make_pairs


@pytest.fixture(scope='module')
def gp():
    return load_golden('actdist_ploidy_golden.npz')


def case_params(tag):
    s, cr, it = tag.split('_')
    return int(s[1:]), float(cr[2:]), int(it[1:])


# ---------------------------------------------------------------------------- ploidy goldens
def test_golden_holds_the_builder_genome(gp):
    assert np.array_equal(gp['radii'], E.RADII) and gp['radii'].dtype == np.float32
    assert np.array_equal(gp['copy_ptr'], E.COPY_PTR)
    assert np.array_equal(gp['copy_idx'], E.COPY_IDX)
    assert np.array_equal(gp['chrom'], E.CHROM)
    ij = E.reference_pairs()
    assert len(ij) == 44 and len(gp['pi']) == 44 * len(E.PW_PL)
    assert [(int(a), int(b)) for a, b in zip(gp['pi'][::len(E.PW_PL)], gp['pj'][::len(E.PW_PL)])] == ij
    assert np.array_equal(gp['pwish'][:len(E.PW_PL)], [w for w, _ in E.PW_PL])
    assert np.array_equal(gp['plast'][:len(E.PW_PL)], [l for _, l in E.PW_PL])
    assert len(gp['cases']) == 10


@pytest.mark.parametrize('tag', ['s%d_cr%s_i%d' % (S, cr, it) for S, cr in
                                 ((1, '2'), (5, '2'), (64, '2'), (65, '2'), (65, '1.3')) for it in (0, 1)])
def test_oracle_equals_reference_ploidy(gp, tag):
    """nrows, f64 ad and p, and the rows byte for byte: combination order and row order of 1x1 up
    to 4x4 (2x3, 3x4 and 4x4 among them) as the reference emits them."""
    assert tag in gp['cases']
    S, cr, it_corr = case_params(tag)
    pairs = make_pairs(gp['pi'], gp['pj'], gp['pwish'], gp['plast'])
    rows, res = oracle.actdist(gp['s%d_xyz' % S], gp['radii'], gp['copy_ptr'], gp['copy_idx'], gp['chrom'], pairs,
                               cr, it_corr, nthreads=4)
    assert np.array_equal(res['nrows'], gp[tag + '_nrows'])
    assert np.array_equal(res['ad'], gp[tag + '_ad64'], equal_nan=True)
    has = res['nrows'] > 0
    assert np.array_equal(res['p'][has], gp[tag + '_p64'][has])
    g = np.zeros(len(gp[tag + '_row']), oracle.row_dtype)
    for k in ('row', 'col', 'dist', 'prob'):
        g[k] = gp[tag + '_' + k]
    assert rows.tobytes() == g.tobytes()
    n = np.array([E.ncomb(a, b) for a, b in zip(gp['pi'], gp['pj'])])
    assert np.array_equal(res['nrows'][has], n[has]) and set(n[has]) == set(E.N_SET)


# ---------------------------------------------------------------------------- widths
def test_width_list_reaches_every_kernel_and_boundary():
    reach = {}
    for S in E.S_LIST:
        for n in E.N_SET:
            reach.setdefault(E.expected_width(n, S), []).append((n * ((S + 63) // 64), n * S))
    for v in (1, 2, 4, 8, 16, 32, 64):
        needs = {need for need, _ in reach[('wave', v)]}
        assert v // 2 + 1 in needs and v in needs, (v, sorted(needs))
        assert all(v // 2 < need <= v for need in needs)
    keys = {v: {k for _, k in reach[('block', v)]} for v in (8, 16, 32, 64)}
    assert 65 in {need for need, _ in reach[('block', 8)]}    # need 64 is ('wave', 64), 65 is not
    assert 8192 in keys[8] and 8193 in keys[16]
    assert 16384 in keys[16] and 16385 in keys[32]
    assert 32768 in keys[32] and 32770 in keys[64]
    assert 65536 in keys[64] and E.expected_width(16, 4096) == E.expected_width(4, 16384) == ('block', 64)
    assert 65538 in {k for _, k in reach[('refused', 0)]} and E.expected_width(9, 7282) == ('refused', 0)
    assert E.expected_width(9, 7281) == ('block', 64)
    assert min(k for _, k in reach[('refused', 0)]) > E.MAX_KEYS
    assert max(k for v in keys for k in keys[v]) == E.MAX_KEYS
    assert E.expected_width(0, 64) == ('none', 0)
    # the refusal tests: the valid pairs with the most combinations at these S and the one refused
    for S, n in ((4097, 16), (7282, 9), (16385, 4)):
        assert E.expected_width(n, S) == ('refused', 0)


def test_pair_list_shape():
    p, n, ok = E.pairs(65)
    assert len(p) == 804 and len(p) % 64 and len(p) % 256
    assert set(n) == set(E.N_SET) | {0} and ok.all()
    # every 64-pair wave of the classification holds at least six different widths
    for lo in range(0, len(p) - 63, 64):
        assert len({E.expected_width(int(k), 65) for k in n[lo:lo + 64]}) >= 6
    # the invalid pairs and i == j are in, with no combination
    bad = (p['i'] < 0) | (p['j'] >= E.NHAP) | (p['i'] == p['j'])
    assert bad.sum() == 11 * len(E.PW_PL) and np.all(n[bad] == 0) and np.all(n[~bad] > 0)
    # n > 4, and inter pairs with na != nb, both > 1 (c / nb against c % nb)
    na, nb = E.NCOPY[p['i'][~bad]], E.NCOPY[p['j'][~bad]]
    inter = E.HAP_CHROM[p['i'][~bad]] != E.HAP_CHROM[p['j'][~bad]]
    assert np.any(inter & (na != nb) & (na > 1) & (nb > 1))
    # intra pairs in both directions, na < nb and na > nb
    assert np.any(~inter & (na < nb)) and np.any(~inter & (na > nb))
    _, _, ok = E.pairs(16385)
    assert not ok.all() and np.array_equal(ok, n * 16385 <= 65536)
    u, un = E.unique_pairs()
    assert len(u) == 56 and len({(a, b) for a, b in zip(u['i'], u['j'])}) == 56 and np.all(un > 0)


def test_radii_differ_between_copies():
    for h in range(E.NHAP):
        r = E.RADII[E.COPY_INDEX[h]]
        assert len(set(r.tolist())) == len(r)
    # contact range 2: rcutsq on the lattice of squared distances for some pairs
    on = [E.rcutsq_f64(E.RADII0[i], E.RADII0[j], 2.0) for i in range(8) for j in range(8) if i != j]
    assert {4.0, 9.0, 16.0} <= set(on)


# S = 1 and 2 are left out: a pair has at most 16 or 32 keys there, too few for ties to be the rule
@pytest.mark.parametrize('S', [S for S in E.S_LIST if S >= 63])
def test_lattice_ties_at_the_selected_order_statistic(S):
    """At every population size the GPU width tests use, for a majority of the pairs (every
    seventh is looked at) the selected squared distance occurs more than once among the pair's
    keys (the bisection is decided among equal keys), d2 == rcutsq occurs, and few ad values are
    unique.  The pairs beyond 65536 keys are dropped, as in the GPU tests."""
    xyz, radii = E.population(S)
    p, n, ok = E.pairs(S)
    p = np.ascontiguousarray(p[ok])
    rows, res = oracle.actdist(*E.genome_args(xyz), p, 2.0, 0, nthreads=8)
    has = np.where(res['nrows'] > 0)[0]
    tied = 0
    on_cut = 0
    for q in has[::7]:
        i, j = int(p['i'][q]), int(p['j'][q])
        ii, jj = E.COPY_INDEX[i], E.COPY_INDEX[j]
        comb = list(zip(ii, jj)) if E.HAP_CHROM[i] == E.HAP_CHROM[j] else [(a, b) for a in ii for b in jj]
        d2 = np.concatenate([((xyz[a] - xyz[b]) ** 2).sum(1) for a, b in comb])
        tied += np.count_nonzero(d2 == np.float32(res['ad'][q] ** 2)) > 1
        on_cut += np.count_nonzero(d2 == E.rcutsq_f64(radii[i], radii[j], 2.0)) > 0
    assert tied > len(has[::7]) // 2
    assert on_cut > 0
    assert len(np.unique(res['ad'][has])) < 80 < len(has)


# ---------------------------------------------------------------------------- threshold traps
def test_every_trap_is_a_trap():
    traps = E.threshold_traps()
    assert len(traps) >= 8 and {t[2] for t in traps} == set(E.TRAP_CRS)
    for ri, rj, cr, x, xb in traps:
        r2 = E.rcutsq_f64(ri, rj, cr)
        d2 = np.float32(x * x)
        assert x.dtype == np.float32 and d2.dtype == np.float32
        assert float(d2) > r2 and np.float32(r2) == d2          # beyond the cutoff, equal after f32 rounding
        db = np.float32(xb * xb)
        assert xb < x and float(db) <= r2                       # the next separation below counts
        assert float(np.float32(np.float32(2) * x) ** 2) > r2


@pytest.mark.parametrize('S', [8, 64, 300])
@pytest.mark.parametrize('cr', E.TRAP_CRS)
def test_oracle_counts_exactly_the_neighbours(cr, S):
    c = E.trap_case(cr, S)
    for it_corr in (0, 1):
        rows, res = oracle.actdist(c['xyz'], c['radii'], c['copy_ptr'], c['copy_idx'], c['chrom'], c['pairs'], cr,
                                   it_corr)
        assert np.array_equal(res['pnow'], c['expect_pnow'])
        assert np.all(res['pnow'] > 0) and np.all(res['pnow'] < 0.5)


# ---------------------------------------------------------------------------- decimal ties
def test_decimal_tie_inputs_are_exact():
    for odd in range(1, 34, 2):
        assert Fraction(odd / 32.0) * 10000 % 1 == Fraction(1, 2)
    v = E.prob_tie_values()
    assert len(v) == 17 + 6 * len(E.TIE_K)
    for q, k in enumerate(E.TIE_K):
        lo, mid, hi = v[17 + 6 * q + 3:17 + 6 * q + 6]
        tie = Fraction(2 * k + 1, 20000)
        assert Fraction(lo) < tie < Fraction(hi) and lo < mid < hi    # the neighbours straddle the tie
        assert (Fraction(mid) == tie) == (k == 312)                   # 312.5/1e4 is 1/32; no other is dyadic
        lo, mid, hi = v[17 + 6 * q:17 + 6 * q + 3]
        assert Fraction(lo) < Fraction(k, 10000) < Fraction(hi) and lo < mid < hi
    for a in E.dist_tie_values():
        assert a % 2 == 1 and a < 4096
        x = np.float32(a / 32.0)
        d2 = np.float32(x * x)
        assert float(x) == a / 32.0 and Fraction(float(d2)) == Fraction(a * a, 1024)
        assert np.sqrt(np.float64(d2)) == a / 32.0
        assert Fraction(a, 32) * 10000 % 1 == Fraction(1, 2)
    A = E.dist_tie_values()
    assert max(A) // 32 == 127 and {(a * 625 - 1) // 2 % 2 for a in A} == {0, 1}


def test_oracle_decimal_ties_equal_python_formatting():
    c = E.decimal_ties()
    rows, res = oracle.actdist(c['xyz'], c['radii'], c['copy_ptr'], c['copy_idx'], c['chrom'], c['pairs'], 2.0, 0)
    has = res['nrows'] > 0
    assert np.array_equal(res['p'], c['pairs']['pwish'])
    assert np.array_equal(res['ad'][has], c['a'][has] / 32.0)
    assert set(c['a'][has]) == set(E.dist_tie_values())             # every distance tie emits a row
    assert has.sum() == len(rows) and np.all(res['nrows'][has] == 1)
    assert np.count_nonzero(~has) == 2
    dist = np.array([np.float32(float('%10.4f' % x)) for x in res['ad'][has]])
    prob = np.array([np.float32(float('%.4f' % x)) for x in res['p'][has]])
    assert np.array_equal(rows['dist'].view(np.uint32), dist.view(np.uint32))
    assert np.array_equal(rows['prob'].view(np.uint32), prob.view(np.uint32))
    # the ties go to the even digit: 1/32 -> 0.0312, 3/32 -> 0.0938
    assert '%.4f' % (1 / 32.0) == '0.0312' and '%.4f' % (3 / 32.0) == '0.0938'


@pytest.mark.parametrize('S', [4, 64])
def test_oracle_order_ties_round_half_even(S):
    xyz, p, ks = E.order_ties(S)
    rows, res = oracle.actdist(*E.genome_args(xyz), p, 2.0, 0)
    assert np.array_equal(res['o'], [k + (k % 2) for k in ks])       # Python round(k + 0.5)
    assert np.all(res['nrows'] == 4)
    # a wrong o would pick another distance: the sorted distances around it differ
    for q, k in enumerate(ks):
        _, other = oracle.actdist(*E.genome_args(xyz), make_pairs([p['i'][q]], [p['j'][q]],
                                                                  [(k + 1 - (k % 2) + 0.25) / (4.0 * S)], [0.0]), 2.0, 0)
        assert other['o'][0] != res['o'][q] and other['ad'][0] != res['ad'][q]
