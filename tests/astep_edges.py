"""Inputs that put the Hi-C A-step (igm_amd/csrc/actdist.hip) on every selection width,
every combination count of a genome with one to four copies per locus, and the rounding
edges of its contract (the f32 contact threshold, CPython's '%.4f', round-half-even of the
order index).  Shared by test_astep_edges.py (CPU: the builder and the oracle),
test_astep_edges_gpu.py (the kernels against the oracle) and
golden/make_golden_actdist_ploidy.py (the reference itself on this genome).

Everything here is plain NumPy and deterministic; nothing touches the GPU.
"""
import functools
from fractions import Fraction

import numpy as np

# ---------------------------------------------------------------------------- genome
NHAP = 8
NBEAD = 32
NCOPY = np.array([1, 2, 3, 4, 1, 2, 3, 4], np.int32)          # loci 0..3 chromosome 0, 4..7 chromosome 1
HAP_CHROM = np.array([0, 0, 0, 0, 1, 1, 1, 1], np.int32)
# copy k of locus h is bead h + 8 k: copy 0 is the haploid index, as in a real .hss
COPY_PTR = np.concatenate([[0], np.cumsum(NCOPY)]).astype(np.int32)
COPY_IDX = np.array([h + NHAP * k for h in range(NHAP) for k in range(NCOPY[h])], np.int32)
CHROM = np.tile(HAP_CHROM, NBEAD // NHAP)                     # per bead; the A-step reads chrom[locus]
COPY_INDEX = {h: [h + NHAP * k for k in range(int(NCOPY[h]))] for h in range(NHAP)}

# radii of copy 0: with contact range 2, (2 (ri + rj))^2 is 4, 6.25, 9, 12.25, 16, 20.25: several on
# the integer lattice of squared distances, so d2 == rcutsq is in the data.  The other copies carry
# other radii: only copy 0's may enter rcutsq (ActivationDistanceStep.py:393).
RADII0 = np.array([0.5, 0.75, 1.0, 0.75, 0.5, 1.25, 0.75, 1.0], np.float32)
RADII = np.array([RADII0[b % NHAP] + 0.375 * (b // NHAP) for b in range(NBEAD)], np.float32)

PW_PL = [(0.5, 0.0), (0.25, 0.1), (1.0, 1.0), (0.3, 1.5), (0.05, 0.9), (0.7, 0.2),
         (1e-9, 0.0),          # p > 0, o = 0, prob prints 0.0000
         (0.0, 0.0),           # no rows
         (1.5, 0.0), (1e6, 0.0),  # o clamps to nS - 1
         (5e-324, 0.0),
         (0.03125, 0.5)]

S_LIST = [1, 2, 63, 64, 65, 128, 129, 256, 257, 448, 449, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097,
          7281, 7282, 8192, 8193, 16384, 16385]
N_SET = [1, 2, 3, 4, 6, 8, 9, 12, 16]
MAX_KEYS = 65536


def ncomb(i, j):
    """Distance combinations of the pair: 0 invalid or i == j, min(|ii|, |jj|) intra (copies
    zipped), |ii| |jj| inter."""
    if i < 0 or j < 0 or i >= NHAP or j >= NHAP or i == j:
        return 0
    na, nb = int(NCOPY[i]), int(NCOPY[j])
    return min(na, nb) if HAP_CHROM[i] == HAP_CHROM[j] else na * nb


def expected_width(n, S):
    """The selection kernel the documented dispatch picks: ('none', 0) without a combination,
    ('wave', v) one wavefront with v keys per lane for need = n ceil(S / 64) <= v in 1..64,
    ('block', v) a 1024-thread workgroup with v keys per thread for n S <= 1024 v in 8..64,
    ('refused', 0) past 65536 keys."""
    if n <= 0:
        return ('none', 0)
    need = n * ((S + 63) // 64)
    keys = n * S
    for v in (1, 2, 4, 8, 16, 32, 64):
        if need <= v:
            return ('wave', v)
    for v in (8, 16, 32, 64):
        if keys <= 1024 * v:
            return ('block', v)
    return ('refused', 0)


@functools.lru_cache(maxsize=None)
def population(S, seed=0):
    """(xyz (32, S, 3) f32, radii): integer-lattice coordinates, so most squared distances tie
    and the order statistic is decided among equal keys.  Treat both as read-only."""
    rng = np.random.default_rng(1000 + 7919 * seed + S)
    xyz = np.round(rng.normal(0.0, 3.0, (NBEAD, S, 3))).astype(np.float32)
    xyz.setflags(write=False)
    return xyz, RADII


def base_pairs():
    """The 64 ordered (i, j), i == j included, and three invalid pairs."""
    ij = [(i, j) for i in range(NHAP) for j in range(NHAP)]
    ij += [(-1, 3), (2, NHAP), (5, NHAP + 5)]
    return ij


def pairs(S):
    """(pairs, n, ok): the 67 base pairs crossed with PW_PL, 804 pairs (a multiple of neither 64
    nor 256).  Consecutive pairs walk the base pairs with a stride coprime to 67, so every 64-pair
    wave of the classification holds every width that the combination counts reach at that S (six
    classes or more, never all eleven kernels at one S).  n: the combinations of each pair (0 for the
    invalid ones); ok: n S within the 65536 keys the selection kernels hold."""
    from conftest import make_pairs
    ij = base_pairs()
    order = (np.arange(len(ij)) * 29) % len(ij)
    pi, pj, pw, pl = [], [], [], []
    for k, (w, l) in enumerate(PW_PL):
        for t in np.roll(order, 5 * k):
            pi.append(ij[t][0])
            pj.append(ij[t][1])
            pw.append(w)
            pl.append(l)
    n = np.array([ncomb(a, b) for a, b in zip(pi, pj)], np.int64)
    p = make_pairs(np.array(pi, np.int32), np.array(pj, np.int32), np.array(pw, np.float64),
                   np.array(pl, np.float64))
    assert len(p) % 64 and len(p) % 256
    return p, n, n * S <= MAX_KEYS


def unique_pairs():
    """The 56 ordered pairs with i != j, once each, PW_PL cycled over them: the pair list of
    igm_astep_update_plast, whose plast is looked up by (i, j) in the rows."""
    from conftest import make_pairs
    ij = [(i, j) for i in range(NHAP) for j in range(NHAP) if i != j]
    pw = [PW_PL[(5 * q) % len(PW_PL)][0] for q in range(len(ij))]
    pl = [PW_PL[(5 * q) % len(PW_PL)][1] for q in range(len(ij))]
    p = make_pairs(np.array([a for a, _ in ij], np.int32), np.array([b for _, b in ij], np.int32),
                   np.array(pw, np.float64), np.array(pl, np.float64))
    return p, np.array([ncomb(a, b) for a, b in ij], np.int64)


def reference_pairs():
    """Every (i, j) the reference defines: all inter pairs and the intra pairs with
    |ii| <= |jj| (its d_sq has |ii| rows and fills min(|ii|, |jj|) of them)."""
    return [(i, j) for i in range(NHAP) for j in range(NHAP)
            if i != j and (HAP_CHROM[i] != HAP_CHROM[j] or NCOPY[i] <= NCOPY[j])]


# ---------------------------------------------------------------------------- threshold traps
TRAP_CRS = (1.0, 1.3, 2.0, 2.5)


def rcutsq_f64(ri, rj, cr):
    """np.square(contactRange * (ri + rj)) with f32 radii and a Python float contact range
    (NumPy 1.x: the f32 sum, then f64)."""
    rc = float(cr) * float(np.float32(ri) + np.float32(rj))
    return rc * rc


def _square_root_f32(f):
    """an f32 x with fl32(x * x) == f, or None"""
    x = np.float32(np.sqrt(np.float64(f)))
    for _ in range(3):
        x = np.nextafter(x, np.float32(0))
    for _ in range(7):
        if np.float32(x * x) == f:
            return x
        x = np.nextafter(x, np.float32(np.inf))
    return None


@functools.lru_cache(maxsize=None)
def threshold_traps(seed=0, per_cr=3):
    """[(ri, rj, cr, x, x_below)]: radii and a contact range whose f64 rcutsq rounds UP to f32,
    with an f32 separation x whose squared distance is exactly float32(rcutsq) -- beyond the
    cutoff, yet counted by a kernel that compares d2 <= (float)rcutsq -- and the next f32
    separation below, whose squared distance is within the cutoff.  per_cr for every contact range
    of TRAP_CRS (12 with the defaults)."""
    rng = np.random.default_rng(4242 + seed)
    out = []
    for cr in TRAP_CRS:
        got = 0
        for _ in range(2000):
            if got == per_cr:
                break
            ri, rj = rng.uniform(0.3, 3.0, 2).astype(np.float32)
            r2 = rcutsq_f64(ri, rj, cr)
            f = np.float32(r2)
            if not float(f) > r2:
                continue
            x = _square_root_f32(f)
            if x is None:
                continue
            xb = np.nextafter(x, np.float32(0))
            out.append((ri, rj, float(cr), x, xb))
            got += 1
        assert got == per_cr, 'trap search exhausted for cr=%g' % cr
    return tuple(out)


def trap_case(cr, S, seed=0):
    """The traps of one contact range as a population of single-copy loci: pair t is loci 2t (at
    the origin, radius ri) and 2t + 1 (radius rj) at (x, 0, 0) in the structures s % 3 == 0 (the
    trap), at (x_below, 0, 0) for s % 3 == 1 (must count) and at (2 x, 0, 0) otherwise.
    Returns dict(xyz, radii, copy_ptr, copy_idx, chrom, pairs, traps, expect_pnow)."""
    from conftest import make_pairs
    traps = [t for t in threshold_traps(seed) if t[2] == cr]
    T = len(traps)
    xyz = np.zeros((2 * T, S, 3), np.float32)
    radii = np.zeros(2 * T, np.float32)
    s = np.arange(S)
    for t, (ri, rj, _, x, xb) in enumerate(traps):
        radii[2 * t], radii[2 * t + 1] = ri, rj
        xyz[2 * t + 1, :, 0] = np.where(s % 3 == 0, x, np.where(s % 3 == 1, xb, np.float32(2) * x))
    pw = [PW_PL[q % 6][0] for q in range(T)]
    pl = [PW_PL[q % 6][1] for q in range(T)]
    p = make_pairs(np.arange(0, 2 * T, 2, dtype=np.int32), np.arange(1, 2 * T, 2, dtype=np.int32),
                   np.array(pw), np.array(pl))
    return dict(xyz=xyz, radii=radii, copy_ptr=np.arange(2 * T + 1, dtype=np.int32),
                copy_idx=np.arange(2 * T, dtype=np.int32), chrom=(np.arange(2 * T, dtype=np.int32) // 2) % 2,
                pairs=p, traps=traps, expect_pnow=np.full(T, np.count_nonzero(s % 3 == 1) / S))


# ---------------------------------------------------------------------------- decimal ties
TIE_K = (0, 1, 2, 5, 312, 4999, 5000, 9999)


def prob_tie_values():
    """pwish values on and around the '%.4f' ties: odd/32 (the only dyadic exact ties at four
    decimals) and, for k of TIE_K, the doubles nearest k/1e4 and (k + 0.5)/1e4 with both
    neighbours."""
    v = [odd / 32.0 for odd in range(1, 34, 2)]
    for k in TIE_K:
        for c in (k / 1e4, (k + 0.5) / 1e4):
            v += [float(np.nextafter(c, -np.inf)), c, float(np.nextafter(c, np.inf))]
    return v


def dist_tie_values():
    """odd a < 4096: a/32 has a square exact in f32, so ad = a/32, a tie of '%10.4f' (a 312.5);
    integer parts up to 127, both parities of the digit the tie rounds to"""
    return [a for a in range(1, 4096, 62)] + [4095, 4093, 33, 35]


def decimal_ties():
    """Single-copy pair t: loci 2t and 2t + 1 separated by (a_t/32, 0, 0) in all S = 4 structures;
    its pwish walks prob_tie_values() (run with it_corr = 0, so p == pwish).  Returns the same
    dict as trap_case, plus 'a'."""
    from conftest import make_pairs
    S = 4
    A = dist_tie_values()
    P = prob_tie_values()
    T = max(len(A), len(P))
    xyz = np.zeros((2 * T, S, 3), np.float32)
    a = np.array([A[t % len(A)] for t in range(T)], np.int64)
    for t in range(T):
        xyz[2 * t:2 * t + 2, :, 1] = t
        xyz[2 * t:2 * t + 2, :, 2] = -t
        xyz[2 * t + 1, :, 0] = np.float32(a[t] / 32.0)
    # a no-row pwish (0, -5e-324) would hide its pair's distance: those pairs come again below
    pw = np.array([P[t % len(P)] for t in range(T)], np.float64)
    again = np.where(~(pw > 0))[0]
    i = np.concatenate([np.arange(0, 2 * T, 2), 2 * again]).astype(np.int32)
    j = i + 1
    pw = np.concatenate([pw, np.full(len(again), 0.40625)])
    p = make_pairs(i, j, pw, np.zeros(len(i)))
    return dict(xyz=xyz, radii=np.full(2 * T, 0.5, np.float32), copy_ptr=np.arange(2 * T + 1, dtype=np.int32),
                copy_idx=np.arange(2 * T, dtype=np.int32), chrom=np.zeros(2 * T, np.int32), pairs=p,
                a=np.concatenate([a, a[again]]))


def order_ties(S):
    """n S p == k + 1/2 exactly: pairs of the genome with n = 4 (2x2, 1x4, 4x1) at S = 64 (or any
    S with 4 S a power of two), p = (k + 0.5)/(4 S) for even and odd k.  Coordinates are not on
    the lattice here: a wrong o picks another distance."""
    from conftest import make_pairs
    nS = 4 * S
    assert nS & (nS - 1) == 0
    rng = np.random.default_rng(77 + S)
    xyz = rng.normal(0.0, 3.0, (NBEAD, S, 3)).astype(np.float32)
    ks = [k for k in (0, 1, 2, 3, 4, 5, 6, 7, 100, 101, nS - 3, nS - 2) if k < nS - 1]
    ij = [(1, 5), (0, 7), (3, 4), (5, 1)]
    pi = [ij[q % 4][0] for q in range(len(ks))]
    pj = [ij[q % 4][1] for q in range(len(ks))]
    pw = np.array([(k + 0.5) / nS for k in ks], np.float64)
    assert all(Fraction(float(w)) * nS == Fraction(2 * k + 1, 2) for w, k in zip(pw, ks))
    return xyz, make_pairs(np.array(pi, np.int32), np.array(pj, np.int32), pw, np.zeros(len(ks))), np.array(ks)


def genome_args(xyz, radii=RADII):
    """positional arguments of compute_actdist / oracle.actdist up to the pair list"""
    return xyz, radii, COPY_PTR, COPY_IDX, CHROM
