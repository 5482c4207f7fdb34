"""Inputs that put the FISH, polymer, SPRITE and contact-map kernels of
igm_amd/csrc/asteps.hip on every branch they have: loci with one, two and three copies behind an
interleaved copy index, both sides of every LDS / HBM switch, unsorted and repeated bin values,
uniforms that land on a cdf entry, bead tiles and structure chunks one short of and one past
their width, contact distances a few ulp around the threshold, and SPRITE structures in which
no copy combination is below INF.  Shared by test_asteps_edges.py (CPU: the builders and the
oracles on their own) and test_asteps_edges_gpu.py (the kernels against the oracles).

Everything here is plain NumPy and deterministic; nothing touches the GPU.
"""
import functools

import numpy as np

f32 = np.float32
i32 = lambda a: np.ascontiguousarray(a, np.int32)

# ---------------------------------------------------------------------------- kernel dispatch
SORT_LDS_MAX = 160 * 1024 - 1024      # kSortLdsMax: one CU's LDS less the static part


def pow2_at_least(n):
    p = 1
    while p < n:
        p <<= 1
    return p


def fish_lds(S):
    """fish_lds: min and max columns, two rank columns (16 S), keys and indices of both (16 npad)"""
    return 4 * (4 * S + 4 * pow2_at_least(S))


def keep_best_lds(S):
    """keep_best_lds: the column and the ranks (8 S), the sort's keys and indices (8 npad)"""
    return 4 * (2 * S + 2 * pow2_at_least(S))


def polymer_lds(S, nbins):
    """the `lds` expression of igm_polymer_assign: distances, counts, sort scratch and ranks as
    floats (rounded to an even count), then cdf and values (double) and positions (int) per bin"""
    return ((S + nbins + 2 * pow2_at_least(S) + S + 1) & ~1) * 4 + nbins * (2 * 8 + 4)


def lattice(shape, sigma, seed):
    """integer-lattice coordinates: most norms tie, so ranks are decided by structure order"""
    xyz = np.round(np.random.default_rng(seed).normal(0.0, sigma, shape)).astype(f32)
    xyz.setflags(write=False)
    return xyz


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---------------------------------------------------------------------------- FISH
# loci 0..3 with 1, 2, 3, 3 copies on 9 beads; the copies of a locus are neither adjacent nor
# ascending in copy_idx
FISH_NCOPY = (1, 2, 3, 3)
FISH_COPY_PTR = i32([0, 1, 3, 6, 9])
FISH_COPY_IDX = i32([0, 4, 1, 7, 2, 5, 3, 8, 6])
FISH_NHAP = 4
FISH_PROBES = i32([2, 0, 3, 1])
FISH_PAIRS = i32([(a, b) for a in range(4) for b in range(4)])      # every (na, nb), a == b included
FISH_S = (1, 2, 255, 256, 257, 4096, 4097)                           # every width class of the rank sort
FISH_OUTPUT_S = (300, 4097)


@functools.lru_cache(maxsize=None)
def fish_population(S):
    return lattice((9, S, 3), 2.0, 4000 + S)


@functools.lru_cache(maxsize=None)
def fish_targets(n, S, seed):
    t = np.sort(np.random.default_rng(seed).random((n, S)), axis=1).astype(f32)
    t.setflags(write=False)
    return t


# ---------------------------------------------------------------------------- polymer
class Uniforms(object):
    """RandomState stand-in that replays prescribed uniforms, one row of S per locus.
    random_sample is what igm_amd.polymer.assign draws; choice is RandomState.choice(a, size, p=p)
    as NumPy's legacy generator computes it from the same uniforms (cdf = p.cumsum(); cdf /=
    cdf[-1]; cdf.searchsorted(u, side='right')), which is what oracle.asteps.polymer_assign
    calls."""

    def __init__(self, rows):
        self.rows = [np.asarray(r, np.float64) for r in rows]
        self.at = 0

    def _take(self, n, S):
        out = self.rows[self.at:self.at + n]
        assert len(out) == n and all(len(r) == S for r in out), 'draws exhausted'
        self.at += n
        return np.stack(out)

    def random_sample(self, size):
        n, S = size
        return self._take(n, S)

    def choice(self, a, size, p):
        cdf = np.asarray(p, np.float64).cumsum()
        cdf /= cdf[-1]
        return np.asarray(a)[cdf.searchsorted(self._take(1, size)[0], side='right')]


POLY_NBINS = (1, 2, 63, 64, 65, 129)       # around the 64-lane chunks of the prefix over the bins
POLY_S = 37
POLY_BIG_S = (8192, 8193)                  # polymer_lds(S, 40): the last LDS and the first HBM population
POLY_BIG_NBINS = 40
POLY_LOCI = i32([0, 3, 2, 2, 2, 4])        # locus 2 three times


def zero_bins(nbins):
    """bins of probability zero: the first, the last, one in the middle and a run of several"""
    if nbins == 1:
        return []
    if nbins == 2:
        return [0]
    mid = nbins // 2
    z = {0, nbins - 1, mid}
    if nbins >= 16:
        z |= set(range(mid + 2, mid + 7))
    return sorted(z)


@functools.lru_cache(maxsize=None)
def polymer_distribution(nbins, zeros):
    """(edges, prob): bin values that no float32 holds, unsorted, each third value twice in
    positions that are not adjacent in value or bin order; `zeros` puts zero_bins(nbins) at
    probability 0."""
    rng = np.random.default_rng(100 + nbins)
    nv = nbins if nbins < 4 else (2 * nbins) // 3
    vals = 1.0 + 0.1 * np.arange(nv) + 1e-9
    edges = vals[np.arange(nbins) % nv][rng.permutation(nbins)]
    if nbins == 2:
        edges = np.sort(edges)[::-1].copy()
    p = rng.random(nbins) + 0.05
    if zeros:
        p[zero_bins(nbins)] = 0.0
    p /= p.sum()
    edges.setflags(write=False)
    p.setflags(write=False)
    return edges, p


# hand-written distributions: the last bin empty, all mass in one middle bin, equal edges
POLY_EXTRA = (
    (np.array([7.3, 2.1]), np.array([1.0, 0.0])),
    (np.array([3.3, 1.1, 2.2, 1.1]), np.array([0.0, 0.0, 1.0, 0.0])),
    (np.array([5.7, 5.7, 5.7]), np.array([0.25, 0.5, 0.25])),
    (np.array([9.1, 0.3, 4.7, 0.3, 9.1]), np.array([0.125, 0.25, 0.25, 0.25, 0.125])),   # cdf exact in binary
)


def cdf_of(prob):
    cdf = np.asarray(prob, np.float64).cumsum()
    cdf /= cdf[-1]
    return cdf


def special_uniforms(prob):
    """uniforms on and beside cdf entries: for several bins k (the first, one before the last, a
    zero-probability bin and the start of the zero run when there are any) cdf[k] exactly and its
    two neighbours, then 0.0 and the largest double below 1"""
    cdf = cdf_of(prob)
    nb = len(cdf)
    ks = {0, nb // 3, nb // 2, nb // 2 + 2, nb - 2}
    u = []
    for k in sorted(k for k in ks if 0 <= k < nb):
        u += [cdf[k], np.nextafter(cdf[k], 0.0), np.nextafter(cdf[k], 1.0)]
    u += [0.0, 1.0 - 2.0 ** -53]
    return np.array(sorted(set(v for v in u if 0.0 <= v < 1.0)))


def polymer_uniforms(prob, nloci, S, seed=0):
    """nloci rows of S uniforms: the special values first (rotated by row, so a special meets a
    different structure, hence a different distance rank, in every row) and random draws after"""
    rng = np.random.default_rng(900 + seed + 17 * len(prob) + S)
    sp = special_uniforms(prob)
    rows = []
    for q in range(nloci):
        u = rng.random(S)
        n = min(len(sp), S)
        u[:n] = sp[:n]
        rows.append(np.roll(u, 5 * q))
    return rows


def expected_bins(prob, u):
    """the bin of every uniform, written out: the number of cdf entries <= u"""
    cdf = cdf_of(prob)
    return np.array([sum(1 for c in cdf if c <= v) for v in u], np.int64)


@functools.lru_cache(maxsize=None)
def polymer_population(S):
    return lattice((6, S, 3), 3.0, 7000 + S)


# ---------------------------------------------------------------------------- contact map
MAP_NBEAD = (63, 64, 65, 129)      # the 64-bead tile
MAP_S = (1, 31, 32, 33, 65)        # the 32-structure chunk


@functools.lru_cache(maxsize=None)
def map_case(nbead, S):
    """radii over six decades; every bead scattered on the scale of its own radius, so contacts
    and misses both occur among small and among large beads"""
    rng = np.random.default_rng(50000 + 131 * nbead + S)
    r = (10.0 ** rng.uniform(-3.0, 3.0, nbead)).astype(f32)
    xyz = (rng.standard_normal((nbead, S, 3)) * (1.5 * r[:, None, None])).astype(f32)
    xyz.setflags(write=False)
    return xyz, r


# twelve different radii; 0.5 + 1.5 is a power of two, and so is the threshold at contact range 2
TIE_RADII = np.array([0.5, 1.5, 37.25, 51.7, 0.013, 129.9, 2.2, 3.3, 1000.1, 7.77, 64.5, 0.3], f32)
TIE_K = (-2, -1, 0, 1, 2)
TIE_CRS = (2.0, 2.1)
TIE_PAIRS = [(i, j) for i in range(12) for j in range(i + 1, 12)]
# unit vectors with three non-zero components, exact and inexact in binary
TIE_DIRS = (np.array([1.0, 2.0, 2.0]) / 3.0, np.array([2.0, 3.0, 6.0]) / 7.0, np.array([-4.0, 4.0, 7.0]) / 9.0,
            np.array([1.0, -1.0, 1.0]) / np.sqrt(3.0))


def threshold(ri, rj, cr):
    """fl32(cr * fl32(ri + rj)), the Hi-C restraint's r0 (restraints/hic.py)"""
    return f32(f32(cr) * f32(f32(ri) + f32(rj)))


def ulps(x, k):
    x = f32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, f32(np.inf) if k > 0 else f32(-np.inf))
    return x


@functools.lru_cache(maxsize=None)
def near_tie_case(cr, offaxis):
    """Structure 5 p + (k + 2) holds pair p = (i, j) at the threshold distance moved by k ulps:
    i at the origin, j on a coordinate axis (the squared norm is one exact product) or, offaxis,
    along a direction with three components (three products and two sums round).  The other ten
    beads are parked 1e6 apart.  Returns xyz (12, 330, 3) and the radii."""
    S = len(TIE_PAIRS) * len(TIE_K)
    xyz = np.zeros((12, S, 3), f32)
    for b in range(12):
        xyz[b] = (1e6 * (b + 1), -1e6, 5e5)
    for p, (i, j) in enumerate(TIE_PAIRS):
        t = threshold(TIE_RADII[i], TIE_RADII[j], cr)
        for k in TIE_K:
            s = len(TIE_K) * p + (k + 2)
            d = ulps(t, k)
            xyz[i, s] = 0.0
            if offaxis:
                xyz[j, s] = (np.float64(d) * TIE_DIRS[p % len(TIE_DIRS)]).astype(f32)
            else:
                xyz[j, s] = 0.0
                xyz[j, s, p % 3] = d if p % 2 else -d
    xyz.setflags(write=False)
    return xyz, TIE_RADII


@functools.lru_cache(maxsize=None)
def zero_threshold_case():
    """contact range 0: every threshold is 0 and only coincident beads touch; coordinates on
    {-1, 0, 1}^3, so beads coincide in some structures and not in others"""
    return lattice((12, 24, 3), 0.6, 31), TIE_RADII


@functools.lru_cache(maxsize=None)
def extreme_case(kind):
    """(xyz, radii, contact_range) of the populations at the ends of float32"""
    rng = np.random.default_rng({'overflow': 1, 'big_threshold': 2, 'nonfinite': 3, 'tiny_radii': 4}[kind])
    nb, S = 10, 40
    r = np.full(nb, 100.0, f32)
    if kind == 'overflow':          # |x| = 1e20: d2 is 0 or +inf
        xyz = rng.choice(np.array([-1e20, 0.0, 1e20]), (nb, S, 3)).astype(f32)
    elif kind == 'big_threshold':   # the bound's square overflows: every finite d2 is a contact, +inf is not
        r = np.full(nb, 1e20, f32)
        xyz = rng.uniform(-1.2e19, 1.2e19, (nb, S, 3)).astype(f32)
    elif kind == 'nonfinite':
        xyz = (rng.standard_normal((nb, S, 3)) * 150.0).astype(f32)
        s = np.arange(S)
        xyz[2, s % 3 == 0] = np.inf
        xyz[6, s % 6 == 0, 0] = np.inf          # with bead 2: inf - inf
        xyz[7, s % 5 == 0, 1] = -np.inf
        xyz[5, s % 4 == 0, 2] = np.nan
    elif kind == 'tiny_radii':      # threshold 4e-30, its square below the smallest subnormal
        r = np.full(nb, 1e-30, f32)
        xyz = rng.choice(np.array([0.0, 1e-20, 1.0]), (nb, S, 3), p=[0.6, 0.2, 0.2]).astype(f32)
    else:
        raise KeyError(kind)
    xyz.setflags(write=False)
    return xyz, r, 2.0


def ragged_copies(nbead):
    """(copy_ptr, copy_idx) with 1, 2, 3, 1, 2, 3, ... copies per locus over nbead beads, laid out
    as a .hss lays them out: every locus' copy 0 first, then the copies 1, then the copies 2 -- so
    the copies of a locus are far apart in bead order.  At nbead = 129 (64 loci) copy 0 is in the
    first 64-bead tile, copies 1 and 2 of most 3-copy loci share the second, and the last locus'
    copy 2 is alone in the third."""
    ncopy = []
    while sum(ncopy) < nbead:
        ncopy.append(min((1, 2, 3)[len(ncopy) % 3], nbead - sum(ncopy)))
    nhap = len(ncopy)
    beads = [[] for _ in range(nhap)]
    b = 0
    for k in range(3):
        for h in range(nhap):
            if ncopy[h] > k:
                beads[h].append(b)
                b += 1
    assert b == nbead
    return i32(np.concatenate([[0], np.cumsum(ncopy)])), i32(np.concatenate(beads))


def single_locus(nbead):
    """nhap = 1: every bead is a copy of the one locus, in a shuffled order"""
    return i32([0, nbead]), i32(np.random.default_rng(nbead).permutation(nbead))


def tiles_of(copy_ptr, copy_idx, h):
    return [int(b) // 64 for b in copy_idx[copy_ptr[h]:copy_ptr[h + 1]]]


# ---------------------------------------------------------------------------- SPRITE
SPRITE_INF = f32(1e8)
REG_REPS = 6        # kRegReps
REG_BEADS = 10      # kRegBeads
SPRITE_MAX_S = 16384


class Recorded(object):
    """np.random stand-in that replays the representative drawn for every chromosome"""

    def __init__(self, values):
        self.values = [int(v) for v in values]

    def choice(self, x):
        v = self.values.pop(0)
        assert v in x
        return v


def genome(nloci, ncopy):
    """chromosome c has nloci[c] loci of ncopy[c] copies each; beads in .hss order (all copies 0,
    then all copies 1, ...), so a locus' copies are interleaved with everybody else's.
    Returns dict(hap_chrom, copy_ptr, copy_idx, nbead)."""
    hap_chrom = np.repeat(np.arange(len(nloci)), nloci)
    nc = np.repeat(ncopy, nloci)
    beads = [[] for _ in hap_chrom]
    b = 0
    for k in range(max(ncopy)):
        for h in range(len(hap_chrom)):
            if nc[h] > k:
                beads[h].append(b)
                b += 1
    return dict(hap_chrom=hap_chrom.astype(np.int64), copy_ptr=i32(np.concatenate([[0], np.cumsum(nc)])),
                copy_idx=i32(np.concatenate(beads)), nbead=b)


# 14 loci on four chromosomes: loci 0-3 with 3 copies, 4-7 with 2, 8-10 with 3, 11-13 with 1
SMALL = genome([4, 4, 3, 3], [3, 2, 3, 1])
# (cluster, representatives in chromosome order -- none for a single chromosome)
SMALL_CLUSTERS = (
    ([0, 1, 2, 3], []),                 # one chromosome, 3 copies: the general path's copy loop
    ([10, 8], []),
    ([1, 2, 5, 6, 9], [2, 5, 9]),       # radix 3, 2, 3 in one combination index
    ([3, 4, 7, 8], [3, 7, 8]),
    ([5, 11, 12], [5, 12]),             # a 1-copy representative with 1-copy segments, beside a 2-copy one
    ([0, 13], [0, 13]),                 # radix 3, 1
    ([11, 12, 13], []),                 # one copy only
    ([4, 5, 6, 7], []),                 # 2 copies: the flat tables
    ([6], []),                          # one segment: Rg^2 = 0 for every copy
    ([9], []),
    ([4, 12], [4, 12]),
    ([12, 6, 2], [2, 6, 12]),           # radix 3, 2, 1, given unsorted
)
# 25 loci, two copies each: chromosome 0 with 11 loci, chromosomes 1..7 with two (11 + 2 (c - 1), + 1)
WIDE = genome([11, 2, 2, 2, 2, 2, 2, 2], [2] * 8)
WIDE_CLUSTERS = (
    (list(range(10)), []),                                              # kRegBeads segments
    (list(range(11)), []),                                              # one more
    ([11, 12, 13, 14, 15, 17, 19, 21], [12, 13, 15, 17, 19, 21]),       # kRegReps representatives
    ([11, 13, 15, 17, 19, 21, 23, 24], [11, 13, 15, 17, 19, 21, 24]),   # one more: 128 combinations
    (list(range(8)) + [11, 13], [3, 11, 13]),                           # 10 segments behind representatives
    (list(range(9)) + [11, 13], [8, 11, 13]),                           # 11
)
SPRITE_S = 300                                        # two 256-thread blocks, the second partial
SPRITE_INF_STRUCTS = (2, 255, 257, 299)               # every combination at or above INF
SPRITE_STRUCTS = (0, 1, 2, 130, 254, 255, 256, 257, 298, 299)


@functools.lru_cache(maxsize=None)
def sprite_population(which):
    """Coordinates of scale 100; in SPRITE_INF_STRUCTS every locus is moved 1e5 h along x, so two
    different loci are at least ~1e5 apart and every Rg^2 of two or more is above 2e9 > INF."""
    g = {'small': SMALL, 'wide': WIDE}[which]
    rng = np.random.default_rng(len(which))
    xyz = (rng.standard_normal((g['nbead'], SPRITE_S, 3)) * 100.0).astype(f32)
    for h in range(len(g['hap_chrom'])):
        for b in g['copy_idx'][g['copy_ptr'][h]:g['copy_ptr'][h + 1]]:
            xyz[b, list(SPRITE_INF_STRUCTS), 0] += f32(1e5 * h)
    xyz.setflags(write=False)
    return xyz


def sprite_tables(g, clusters, max_chrom=8):
    from igm_amd import sprite
    reps = [r for _, rr in clusters for r in rr]
    rec = Recorded(reps)
    t = sprite.cluster_tables([np.array(c) for c, _ in clusters], g['hap_chrom'], g['copy_ptr'],
                              max_chrom_in_cluster=max_chrom, rng=rec)
    assert not rec.values and len(t['kept']) == len(clusters)
    return t


def rg2_columns(pts):
    """gyration_radius_sq for a whole population at once: pts (n, S, 3) float32, the float32 sums
    in the order of oracle.asteps.rg2_f32, read through get_rg2s_cpp (not below INF: INF)"""
    n = f32(len(pts))
    m = np.zeros(pts.shape[1:], f32)
    for p in pts:
        m = m + p
    m = m / n
    rg = np.zeros(pts.shape[1], f32)
    for p in pts:
        d = p - m
        rg = rg + ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    rg = rg / n
    return np.where(rg < SPRITE_INF, rg, SPRITE_INF).astype(f32)


# keep_best: six single-copy loci on one chromosome, lattice coordinates
KEEP_S = (8192, 8193, 16384)       # keep_best_lds: the last sorted population, the first counted, the largest
KEEP_CLUSTERS = ([0, 1, 2], [2, 3, 4, 5], [1, 5], [3])       # the last: Rg^2 = 0 everywhere
KEEP = genome([6], [1])


@functools.lru_cache(maxsize=None)
def keep_population(S):
    return lattice((6, S, 3), 1.0, 8000 + S)


def keep_cases(S):
    return [1, 50] + ([S - 1] if S == 8193 else [])
