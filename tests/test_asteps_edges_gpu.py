"""The FISH, polymer, SPRITE and contact-map kernels (igm_amd/csrc/asteps.hip) bit for bit against
the CPU oracles on the inputs of tests/asteps_edges.py: one, two and three copies behind an
interleaved copy index, both sides of every LDS / HBM switch, every output combination, unsorted
and repeated bin values with uniforms on the cdf entries, the 64-bead tile and 32-structure chunk
edges, distances a few ulp around the contact threshold, the ends of float32, and SPRITE
structures without a combination below INF.  Every comparison is array_equal on integers or on
float32 bit patterns.  test_asteps_edges.py proves on the CPU that the inputs are those edges."""
import functools

import numpy as np
import pytest

import asteps_edges as E
from asteps_edges import bits
from oracle import asteps as OA

pytestmark = pytest.mark.gpu


def same_f32(got, want):
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


# ---------------------------------------------------------------------------- FISH
def fish_items(kind):
    return E.FISH_PROBES if kind == 'probe' else E.FISH_PAIRS


@functools.lru_cache(maxsize=None)
def fish_oracle(S, kind):
    items = fish_items(kind)
    tmin, tmax = E.fish_targets(len(items), S, 1), E.fish_targets(len(items), S, 2)
    fn = OA.fish_radial if kind == 'probe' else OA.fish_pair
    omin, omax, dmin, dmax = fn(E.fish_population(S), E.FISH_COPY_PTR, E.FISH_COPY_IDX, items, tmin, tmax)
    return tmin, tmax, omin, omax, dmin.astype(np.float32), dmax.astype(np.float32)


@pytest.mark.parametrize('kind', ['probe', 'pair'])
@pytest.mark.parametrize('S', E.FISH_S)
def test_gpu_fish_copy_counts_at_every_width(S, kind):
    """probes of 1, 2 and 3 copies and the 4 x 4 pairs of them (a locus with itself included) at
    every width class of the rank sort; 4097 is the first population in HBM"""
    from igm_amd import fish
    tmin, tmax, omin, omax, dmin, dmax = fish_oracle(S, kind)
    got = fish.assign(E.fish_population(S), E.FISH_COPY_PTR, E.FISH_COPY_IDX, kind, fish_items(kind), tmin, tmax,
                      return_dists=True)
    assert same_f32(got[2], dmin) and same_f32(got[3], dmax)
    assert same_f32(got[0], omin) and same_f32(got[1], omax)


@pytest.mark.parametrize('which', ['min', 'max', 'both'])
@pytest.mark.parametrize('kind', ['probe', 'pair'])
@pytest.mark.parametrize('S', E.FISH_OUTPUT_S)
def test_gpu_fish_output_combinations(S, kind, which):
    from igm_amd import fish
    tmin, tmax, omin, omax, dmin, dmax = fish_oracle(S, kind)
    args = (E.fish_population(S), E.FISH_COPY_PTR, E.FISH_COPY_IDX, kind, fish_items(kind))
    if which == 'min':
        gmin, gmax = fish.assign(*args, tmin, None)
        assert gmax is None and same_f32(gmin, omin)
    elif which == 'max':
        gmin, gmax = fish.assign(*args, None, tmax)
        assert gmin is None and same_f32(gmax, omax)
    else:
        gmin, gmax, gdmin, gdmax = fish.assign(*args, tmin, tmax, return_dists=True)
        assert same_f32(gmin, omin) and same_f32(gmax, omax) and same_f32(gdmin, dmin) and same_f32(gdmax, dmax)
        # distances alone, no target at all
        n0, n1, gdmin, gdmax = fish.assign(*args, None, None, return_dists=True)
        assert n0 is None and n1 is None and same_f32(gdmin, dmin) and same_f32(gdmax, dmax)


@pytest.mark.parametrize('S', [300, 4097])
def test_gpu_fish_refuses_loci_outside_the_genome(S):
    from igm_amd import fish
    xyz = E.fish_population(S)
    t = E.fish_targets(2, S, 1)
    for kind, items in (('probe', [1, E.FISH_NHAP]), ('probe', [-1, 2]), ('pair', [(0, 1), (2, E.FISH_NHAP)]),
                        ('pair', [(-1, 0), (1, 1)])):
        with pytest.raises(RuntimeError, match='outside'):
            fish.assign(xyz, E.FISH_COPY_PTR, E.FISH_COPY_IDX, kind, np.array(items, np.int32), t, t)


# ---------------------------------------------------------------------------- polymer
def polymer_both(S, edges, prob, loci=E.POLY_LOCI, **kw):
    """(kernel output, distances, oracle output): both sides draw the same prescribed uniforms"""
    from igm_amd import polymer as PL
    xyz = E.polymer_population(S)
    rows = E.polymer_uniforms(prob, len(loci), S)
    _, nn, dist = PL.assign(xyz, edges, prob, E.Uniforms(rows), loci=loci, return_dists=True, **kw)
    want = OA.polymer_assign(xyz, loci, edges, prob, E.Uniforms(rows))
    d = np.linalg.norm(xyz[loci] - xyz[np.asarray(loci) + 1], axis=2).astype(np.float32)
    assert same_f32(dist, d)
    return nn, want, rows


@pytest.mark.parametrize('nbins,zeros', [(nb, z) for nb in E.POLY_NBINS for z in (False, True) if nb > 1 or not z])
def test_gpu_polymer_unsorted_edges_zero_bins_and_cdf_uniforms(nbins, zeros):
    edges, prob = E.polymer_distribution(nbins, zeros)
    nn, want, rows = polymer_both(E.POLY_S, edges, prob)
    assert nn.tobytes() == want.tobytes()
    # the expected bins written out: cdf.searchsorted(u, side='right'), values sorted, taken by rank
    cdf = E.cdf_of(prob)
    xyz = E.polymer_population(E.POLY_S)
    for q, i in enumerate(E.POLY_LOCI):
        drawn = np.sort(edges[cdf.searchsorted(rows[q], side='right')])
        d = np.linalg.norm(xyz[i] - xyz[i + 1], axis=1)
        rank = np.argsort(np.argsort(d, kind='stable'), kind='stable')
        assert same_f32(nn[q], drawn[rank].astype(np.float32))


@pytest.mark.parametrize('k', range(len(E.POLY_EXTRA)))
def test_gpu_polymer_hand_written_distributions(k):
    edges, prob = E.POLY_EXTRA[k]
    nn, want, _ = polymer_both(E.POLY_S, edges, prob)
    assert nn.tobytes() == want.tobytes()
    assert set(np.unique(nn)) <= set(edges[prob > 0].astype(np.float32))


@pytest.mark.parametrize('zeros', [False, True])
@pytest.mark.parametrize('S', E.POLY_BIG_S)
def test_gpu_polymer_either_side_of_the_lds_switch(S, zeros):
    """lds = ((S + nbins + 2 npad + S + 1) & ~1) * 4 + 20 nbins of igm_polymer_assign with 40 bins:
    132 032 bytes at S = 8192 (npad 8192), 197 576 at 8193 (npad 16384), around the 162 816 of one
    CU -- the last population ranked in LDS and the first in HBM"""
    assert E.polymer_lds(8192, E.POLY_BIG_NBINS) <= E.SORT_LDS_MAX < E.polymer_lds(8193, E.POLY_BIG_NBINS)
    edges, prob = E.polymer_distribution(E.POLY_BIG_NBINS, zeros)
    nn, want, _ = polymer_both(S, edges, prob)
    assert nn.tobytes() == want.tobytes()


@pytest.mark.parametrize('S', (E.POLY_S, 8193))
def test_gpu_polymer_repeated_locus_follows_the_draw_order(S):
    """one locus three times: three rows, each from its own S uniforms in the order drawn, whether
    the loci go in one launch or two"""
    from igm_amd import polymer as PL
    edges, prob = E.polymer_distribution(E.POLY_BIG_NBINS, True)
    loci = np.array([2, 2, 2], np.int32)
    nn, want, rows = polymer_both(S, edges, prob, loci=loci)
    assert nn.tobytes() == want.tobytes()
    assert len({nn[q].tobytes() for q in range(3)}) == 3
    nn2, _, _ = polymer_both(S, edges, prob, loci=loci, chunk=2)
    assert nn2.tobytes() == want.tobytes()
    for q in range(3):
        _, one = PL.assign(E.polymer_population(S), edges, prob, E.Uniforms([rows[q]]), loci=loci[:1])
        assert one[0].tobytes() == want[q].tobytes()


# ---------------------------------------------------------------------------- contact map
def oracle_counts(xyz, r, cr):
    with np.errstate(all='ignore'):
        return OA.contact_counts(xyz, r, cr)


def map_equals_oracle(xyz, r, cr, tables):
    """igm_contact_map against the oracle, and igm_contact_map_haploid against the oracle's counts
    summed over the copies, for every copy table given.  Returns the oracle's counts."""
    from igm_amd import evaluation as EV
    want = oracle_counts(xyz, r, cr)
    got = EV.contact_counts(xyz, r, cr)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    for cp, ci in tables:
        hap = EV.haploid_counts(xyz, r, cr, cp, ci)
        hwant = EV.sum_copies(want.astype(np.int64), cp, ci).astype(np.int64)
        assert hap.shape == hwant.shape and np.array_equal(hap.astype(np.int64), hwant)
    return want


@pytest.mark.parametrize('S', E.MAP_S)
@pytest.mark.parametrize('nbead', E.MAP_NBEAD)
def test_gpu_map_tile_and_chunk_edges(nbead, S):
    xyz, r = E.map_case(nbead, S)
    map_equals_oracle(xyz, r, 2.0, [E.ragged_copies(nbead), E.single_locus(nbead)])


@pytest.mark.parametrize('offaxis', [False, True])
@pytest.mark.parametrize('cr', E.TIE_CRS)
def test_gpu_map_near_ties_for_every_pair(cr, offaxis):
    xyz, r = E.near_tie_case(cr, offaxis)
    want = map_equals_oracle(xyz, r, cr, [E.ragged_copies(12)])
    assert all(0 < want[i, j] < xyz.shape[1] for i, j in E.TIE_PAIRS)


def test_gpu_map_zero_threshold():
    xyz, r = E.zero_threshold_case()
    map_equals_oracle(xyz, r, 0.0, [E.ragged_copies(12)])


@pytest.mark.parametrize('kind', ['overflow', 'big_threshold', 'nonfinite', 'tiny_radii'])
def test_gpu_map_extremes(kind):
    xyz, r, cr = E.extreme_case(kind)
    map_equals_oracle(xyz, r, cr, [E.ragged_copies(len(r))])


@pytest.mark.parametrize('nbead,S', [(9, 5), (129, 33), (129, 64)])
def test_gpu_haploid_counts_against_the_oracle(nbead, S):
    """ragged copy tables (1, 2 and 3 copies, interleaved; at 129 beads the copies of a locus share
    a tile or sit in two or three) and a genome of one locus, the counts from the oracle"""
    from igm_amd import evaluation as EV
    xyz, r = E.map_case(nbead, S)
    want = map_equals_oracle(xyz, r, 2.0 * (1 + EV.EPS), [E.ragged_copies(nbead), E.single_locus(nbead)])
    one = EV.haploid_counts(xyz, r, 2.0 * (1 + EV.EPS), *E.single_locus(nbead))
    assert one.shape == (1, 1) and int(one[0, 0]) == int(want.astype(np.int64).sum())


# ---------------------------------------------------------------------------- SPRITE
@functools.lru_cache(maxsize=None)
def sprite_case(which):
    g = {'small': E.SMALL, 'wide': E.WIDE}[which]
    clusters = {'small': E.SMALL_CLUSTERS, 'wide': E.WIDE_CLUSTERS}[which]
    xyz = E.sprite_population(which)
    want = [OA.sprite_cluster_rg2(xyz, g['hap_chrom'], g['copy_ptr'], g['copy_idx'], cl, reps, structs=E.SPRITE_STRUCTS)
            for cl, reps in clusters]
    return g, clusters, xyz, want


@pytest.mark.parametrize('tables', [None, '0'], ids=['tables', 'index'])
@pytest.mark.parametrize('which', ['small', 'wide'])
def test_gpu_sprite_copy_counts_register_edges_and_all_inf(which, tables, monkeypatch):
    """'small': clusters of 1, 2 and 3 copies, radix 3-2-3, 2-1 and 3-1 combination indices, one
    segment; 'wide': 6 and 7 representatives, 10 and 11 segments.  In SPRITE_INF_STRUCTS no
    combination is below INF.  With IGM_SPRITE_TABLES unset (flat tables where the copies allow)
    and 0 (the per-bead index path for every cluster)."""
    from igm_amd import sprite
    if tables is None:
        monkeypatch.delenv('IGM_SPRITE_TABLES', raising=False)
    else:
        monkeypatch.setenv('IGM_SPRITE_TABLES', tables)
    g, clusters, xyz, want = sprite_case(which)
    t = E.sprite_tables(g, clusters)
    kb = E.SPRITE_S - 1
    bi, bv, bs, rg2 = sprite.rg2_select(xyz, g['copy_ptr'], g['copy_idx'], t, kb, return_rg2=True)
    structs = list(E.SPRITE_STRUCTS)
    for c, (rg, sel) in enumerate(want):
        assert np.array_equal(bits(rg2[c][structs]), bits(rg[structs])), (c, clusters[c])
        assert np.array_equal(bi[c], OA.keep_best(rg2[c], kb)), c
        assert np.array_equal(bits(bv[c]), bits(rg2[c][bi[c]])), c
        g0, g1 = int(t['seg_ptr'][c]), int(t['seg_ptr'][c + 1])
        got = bs[g0 * kb:g1 * kb].reshape(kb, g1 - g0)
        rank_of = {int(s): k for k, s in enumerate(bi[c])}
        seen = [s for s in structs if s in rank_of]
        assert len(seen) >= len(structs) - 1            # keep_best = S - 1 leaves one structure out
        for s in seen:
            assert np.array_equal(got[rank_of[s]], sel[s]), (c, clusters[c], s)
        if len(clusters[c][0]) > 1:
            assert np.all(rg2[c][list(E.SPRITE_INF_STRUCTS)] == E.SPRITE_INF)


@pytest.mark.parametrize('S', E.KEEP_S)
def test_gpu_sprite_keep_best_either_side_of_the_lds_switch(S):
    """keep_best_lds = 8 S + 8 npad: sorted in LDS up to S = 8192, ranks counted from 8193; 16384
    is the largest population accepted.  Lattice ties: the kept order is a stable argsort."""
    from igm_amd import sprite
    g = E.KEEP
    xyz = E.keep_population(S)
    t = sprite.cluster_tables([np.array(c) for c in E.KEEP_CLUSTERS], g['hap_chrom'], g['copy_ptr'])
    cols = [E.rg2_columns(xyz[cl]) for cl in E.KEEP_CLUSTERS]
    for kb in E.keep_cases(S):
        bi, bv, bs, rg2 = sprite.rg2_select(xyz, g['copy_ptr'], g['copy_idx'], t, kb, return_rg2=True)
        for c, cl in enumerate(E.KEEP_CLUSTERS):
            assert np.array_equal(bits(rg2[c]), bits(cols[c])), (kb, c)
            order = np.argsort(cols[c], kind='stable')[:kb]
            assert np.array_equal(bi[c], order), (kb, c)
            assert np.array_equal(bits(bv[c]), bits(cols[c][order])), (kb, c)
            g0, g1 = int(t['seg_ptr'][c]), int(t['seg_ptr'][c + 1])
            assert np.array_equal(bs[g0 * kb:g1 * kb].reshape(kb, g1 - g0), np.tile(np.sort(cl), (kb, 1)))


def test_gpu_sprite_refuses_past_its_limits():
    from igm_amd import sprite
    g = E.KEEP
    t = sprite.cluster_tables([np.array(c) for c in E.KEEP_CLUSTERS], g['hap_chrom'], g['copy_ptr'])
    with pytest.raises(RuntimeError, match='exceed'):
        sprite.rg2_select(np.zeros((6, E.SPRITE_MAX_S + 1, 3), np.float32), g['copy_ptr'], g['copy_idx'], t, 5)
    xyz = E.keep_population(8193)
    with pytest.raises(RuntimeError, match='keep_best'):
        sprite.rg2_select(xyz, g['copy_ptr'], g['copy_idx'], t, 8193)
    bi, _, _ = sprite.rg2_select(xyz, g['copy_ptr'], g['copy_idx'], t, 8192)
    assert bi.shape == (len(E.KEEP_CLUSTERS), 8192)
