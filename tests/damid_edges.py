"""Inputs that put the DamID kernels on their edges: the A-step of igm_amd/csrc/asteps.hip
(damid_kernel, damid_exp_kernel<false> and <true>) and the lamina selections of
igm_amd/csrc/restraints.hip (damid_select_kernel, volume_select_kernel).  Shared by
test_damid_edges.py (CPU: every input is the edge it claims, the restatements equal the
reference), test_damid_edges_gpu.py (the kernels against the restatements) and
golden/make_golden_damid_edges.py (the reference itself on these inputs).

  genome      loci with 1, 2, 3, 4, 0 and 2 copies behind a copy index that is neither
              contiguous nor ascending; the radii differ between the copies of a locus and only
              the first copy's may enter the divisor (DamidActivationDistanceStep.py:421)
  lattices    coordinates j/64 (squared norms tie), (1 + j/4096, k/4096, l/4096) (keys that share
              their upper 8, 16 and 24 bits), j/8192 (the f32 below 1.0); with the sphere 1.5, the
              first-copy radius 0.5 and contact range 0 the divisor is exactly 1
  A-step      ploidy, radix ties, 0 / subnormal / inf / NaN keys, the count threshold, the
              cleanProbability branches, half-to-even order indices, decimal ties of '%.5f',
              one-axis ellipsoid beads, list shapes
  selection   beads exactly on v == d^2 for each axis, the f32 against the f64 square of d, row
              counts around the wave and the block, duplicate and out-of-range rows
  exp_map     three small sphere maps of different size, centre and grid, assigned per structure
              in an unsorted pattern; beads on voxel centres, on voxel half-steps and one voxel
              inside and outside every face

Coordinates that are NaN or inf are left out for the exp_map A-steps and igm_volume_select: the
integer conversion of the voxel is undefined for them in the reference too.

Everything here is plain NumPy and deterministic; nothing touches the GPU.  A case is a dict
(see case()); variant() restates the A-step with one deliberate mistake switched on, which is
how the CPU test shows that an input tells the mistake from the contract.
"""
import decimal
import functools

import numpy as np

from igm_amd._lib import IGM_ATOM_ENV0, damid_row_dtype, result_dtype
from oracle import asteps as OA

f32 = np.float32

# ---------------------------------------------------------------------------- genome
NHAP = 6
NCOPY = np.array([1, 2, 3, 4, 0, 2], np.int32)
COPY_INDEX = {0: [7], 1: [3, 10], 2: [11, 0, 5], 3: [2, 9, 1, 6], 5: [8, 4]}   # what the reference reads
COPY_PTR = np.concatenate([[0], np.cumsum(NCOPY)]).astype(np.int32)
COPY_IDX = np.array([b for h in range(NHAP) for b in COPY_INDEX.get(h, [])], np.int32)
NBEAD = 12
# first copies (beads 7, 3, 11, 2) 0.5 and (bead 8) 0.75; every other copy another radius
RADII = np.array([0.625, 0.75, 0.5, 0.5, 0.375, 0.875, 1.0, 0.5, 0.75, 0.625, 0.25, 0.5], f32)
SPHERE = 1.5                      # 1.5 - 0.5 = 1: the divisor is exactly 1 at contact range 0
ELLIPSOID = (2.5, 1.5, 4.5)       # minus 0.5: 2, 1, 4
LOCI_ORDER = [3, 1, 0, 5, 2, 1]   # not sorted, locus 1 twice
S_LIST = (1, 2, 63, 64, 65, 255, 256, 257, 1025)
S_GOLDEN = (1, 5, 64, 65)

PNOW = 'pnow'                     # plast = the locus's own pnow: cleanProbability(pnow, plast) = 0
# (p_exp, plast)
PE_PL = [(0.5, 0.0), (0.25, 0.99), (0.75, 1.0), (0.3, 1.5), (0.6, PNOW), (0.9, 0.2), (0.05, 0.9),
         (0.01, 0.0),               # it_corr 1: below pnow, p = 0, dist = 2, o = -1
         (1e-7, 0.0),               # it_corr 0: o = 0, the largest key, prob prints 0.00000
         (1.0, 0.0), (1.5, 0.0),    # o clamps to nS - 1
         (1 / 64, 0.0), (5 / 64, 0.0), (3 / 64, 0.0), (37 / 64, 0.0), (99 / 64, 0.0),   # six decimals ending in 5
         (1 / 8, 0.0), (3 / 8, 0.0), (5 / 8, 0.0)]


def copies(c, I):
    return [int(b) for b in c['copy_idx'][c['copy_ptr'][I]:c['copy_ptr'][I + 1]]]


def case(xyz, loci, p_exp, plast, it_corr, cr, shape, radii=RADII, copy_ptr=COPY_PTR, copy_idx=COPY_IDX,
         copy_index=None):
    xyz = np.ascontiguousarray(xyz, f32)
    xyz.setflags(write=False)
    return dict(xyz=xyz, radii=radii, copy_ptr=copy_ptr, copy_idx=copy_idx, loci=np.array(loci, np.int32),
                p_exp=np.array(p_exp, f32), plast=np.array(plast, f32), it_corr=int(it_corr), cr=float(cr),
                shape=shape, param=SPHERE if shape == 'sphere' else ELLIPSOID,
                copy_index=COPY_INDEX if copy_index is None else copy_index)


def args(c):
    """the arguments of igm_amd.damid.compute_damid_actdist"""
    return (c['xyz'], c['radii'], c['copy_ptr'], c['copy_idx'], c['loci'], c['p_exp'], c['plast'], c['it_corr'],
            c['cr'], c['shape'], c['param'])


def expected(c):
    """(rows, per locus) of oracle.asteps.damid_actdist; the oracle indexes p_exp and plast by the
    haploid locus, a case lists them per entry, so the oracle runs entry by entry"""
    nhap = len(c['copy_ptr']) - 1
    rows, res = [], []
    for q, I in enumerate(c['loci']):
        a, b = OA.damid_actdist(c['xyz'], c['radii'], c['copy_ptr'], c['copy_idx'], [int(I)],
                                np.full(nhap, c['p_exp'][q], f32), np.full(nhap, c['plast'][q], f32), c['it_corr'],
                                c['cr'], c['shape'], c['param'], return_per_locus=True)
        rows.append(a.astype(damid_row_dtype))
        res.append(b)
    if not rows:
        return np.zeros(0, damid_row_dtype), np.zeros(0, result_dtype)
    return np.concatenate(rows), np.concatenate(res).astype(result_dtype)


def keys(c, I, own_radius=False, param=None):
    """the f32 keys of locus I in copy-major order, as the oracle forms them"""
    ii = copies(c, I)
    par = c['param'] if param is None else param
    return np.concatenate([OA.damid_d2(c['xyz'][b], c['radii'][b if own_radius else ii[0]], c['cr'], c['shape'], par)
                           for b in ii]).astype(f32)


def descending(k):
    """d_sq[::-1].sort(): NaN first"""
    return np.sort(np.asarray(k, np.float64))[::-1]


def _dec_half_up(x):
    if not np.isfinite(x):
        return '%.5f' % x
    return str(decimal.Decimal(float(x)).quantize(decimal.Decimal('0.00001'), rounding=decimal.ROUND_HALF_UP))


def variant(c, own_radius=False, count_gt=False, half_up=False, dec_half_up=False, param=None):
    """The A-step restated with one mistake switched on (none: the contract, which
    test_damid_edges.py holds equal to expected()): each copy's own radius, > for >= 1 in the
    count, floor(x + 0.5) for the order index, half-up decimals in the text."""
    rows = []
    res = np.zeros(len(c['loci']), result_dtype)
    for q, I in enumerate(c['loci']):
        d = descending(keys(c, int(I), own_radius, param))
        n = len(d)
        pnow = float(np.count_nonzero(d > 1.0 if count_gt else d >= 1.0)) / n
        pe, pl = c['p_exp'][q], c['plast'][q]
        p = OA._clean(pe, OA._clean(pnow, pl)) if c['it_corr'] == 1 else float(pe)
        ad, o = 2, -1
        if p > 0:
            x = np.float64(n) * p
            o = min(n - 1, int(np.floor(x + 0.5) if half_up else np.round(x)))
            ad = float(np.sqrt(d[o]))
        res[q] = (ad if o >= 0 else np.nan, p, pnow, o, len(copies(c, int(I))))
        fmt = _dec_half_up if dec_half_up else (lambda v: '%.5f' % v)
        for b in copies(c, int(I)):
            rows.append((b, f32(float(fmt(ad))), f32(float(fmt(p)))))
    out = np.zeros(len(rows), damid_row_dtype)
    if rows:
        out['loc'], out['dist'], out['prob'] = zip(*rows)
    return out, res


def rows_of(c, res, q):
    """slice of the rows that entry q wrote"""
    off = int(np.sum(res['nrows'][:q]))
    return slice(off, off + int(res['nrows'][q]))


# ---------------------------------------------------------------------------- populations
@functools.lru_cache(maxsize=None)
def population(S):
    """(12, S, 3) f32 on the lattice j/64, |j| <= 60: squared norms are multiples of 1/4096 and tie"""
    rng = np.random.default_rng(4000 + S)
    xyz = (rng.integers(-60, 61, (NBEAD, S, 3)) / 64.0).astype(f32)
    xyz.setflags(write=False)
    return xyz


def _listing(loci, pe_pl, c0):
    """loci x (p_exp, plast); PNOW becomes f32(pnow) of the locus on the case c0"""
    L, pe, pl = [], [], []
    for (a, b) in pe_pl:
        for I in loci:
            if b is PNOW:
                k = keys(c0, I)
                b_ = f32(np.count_nonzero(k >= 1.0) / len(k))
            else:
                b_ = b
            L.append(I)
            pe.append(a)
            pl.append(b_)
    return L, pe, pl


@functools.lru_cache(maxsize=None)
def ploidy_case(S, shape, cr, it_corr):
    c0 = case(population(S), [], [], [], it_corr, cr, shape)
    return case(population(S), *_listing(LOCI_ORDER, PE_PL, c0), it_corr, cr, shape)


# (j, k, l): the bead (1 + j/4096, k/4096, l/4096); with divisor 1 its key has the bits named
T_KEY = 0x3f80ff00
RADIX_POOL = [(11, 141, 143), (11, 141, 143), (11, 141, 143),   # T 0x3f80ff00: bucket 255 then bucket 0
              (12, 119, 134),                                   # 0x3f80ff02: the upper 24 bits of T
              (13, 22, 153),                                    # 0x3f80fefe: the upper 16 bits of T
              (11, 126, 158),                                   # 0x3f810000: the upper 8 bits of T
              (0, 0, 0),                                        # 0x3f800000: 1.0
              (63, 159, 159)]                                   # 0x3f845a80


@functools.lru_cache(maxsize=None)
def radix_case(S):
    """Loci 1, 2, 3 hold the pool above in rotation over (copy, structure); p_exp picks the middle
    one of the keys equal to T: ties, shared prefixes, bucket 255 and bucket 0 in one select."""
    xyz = population(S).copy()
    c0 = dict(copy_ptr=COPY_PTR, copy_idx=COPY_IDX)
    for I in (1, 2, 3):
        for ci, b in enumerate(copies(c0, I)):
            for s in range(S):
                j, k, l = RADIX_POOL[(ci * S + s) % len(RADIX_POOL)]
                xyz[b, s] = (1 + j / 4096.0, k / 4096.0, l / 4096.0)
    c = case(xyz, [], [], [], 0, 0.0, 'sphere')
    loci, pe = [3, 2, 1], []
    for I in loci:
        u = keys(c, I).view(np.uint32)
        n, less, nt = len(u), int(np.count_nonzero(u < T_KEY)), int(np.count_nonzero(u == T_KEY))
        o = n - 1 - (less + nt // 2)          # descending index of the middle T
        p = f32(o / n) if o > 0 else f32(0.25 / n)
        assert int(np.round(np.float64(n) * float(p))) == o
        pe.append(p)
    return case(xyz, loci, pe, [0.0] * 3, 0, 0.0, 'sphere')


# a second, two-locus genome of single copies for the special keys: S = 8
SP_PTR = np.array([0, 1, 2], np.int32)
SP_IDX = np.array([1, 0], np.int32)
SP_RADII = np.array([0.5, 0.5], f32)
NEG_NAN = np.array([0xffc00000], np.uint32).view(f32)[0]
BELOW_ONE = (8178 / 8192.0, 476 / 8192.0, 51 / 8192.0)      # the squares sum to the f32 below 1.0
ABOVE_ONE = (1.0, 5 / 16384.0, 0.0)                         # ... to the f32 above 1.0
SPECIAL_X = [0.0, 2.0 ** -70, 0.5, 1.0, 3.0, np.inf, np.nan, NEG_NAN]


@functools.lru_cache(maxsize=None)
def special_case(it_corr):
    """Locus 0 (bead 1): keys 0, the f32 subnormal 2^-140, 0.25, 1, 9, +inf, NaN and NaN with the
    sign bit; descending that is NaN, NaN, inf, 9, 1, 0.25, 2^-140, 0 and p_exp = o/8 selects
    each.  pnow = 3/8 = plast, so it_corr 1 leaves p = p_exp.
    Locus 1 (bead 0): keys 1.0, the f32 below and the f32 above, twice, 0.25 and 4: five of the
    eight are >= 1, three are > 1."""
    xyz = np.zeros((2, 8, 3), f32)
    xyz[1, :, 0] = np.array(SPECIAL_X, f32)
    xyz[1, 7, 0] = NEG_NAN
    xyz[0] = np.array([(1.0, 0.0, 0.0), BELOW_ONE, ABOVE_ONE, (1.0, 0.0, 0.0), BELOW_ONE, ABOVE_ONE,
                       (0.5, 0.0, 0.0), (2.0, 0.0, 0.0)], f32)
    pe = [1e-7] + [o / 8.0 for o in range(1, 8)] + [1.0]
    loci = [0] * len(pe) + [1, 1, 1]
    return case(xyz, loci, pe + [0.9, 0.9, 0.5], [0.375] * len(pe) + [0.0, 0.625, 0.0], it_corr, 0.0, 'sphere',
                radii=SP_RADII, copy_ptr=SP_PTR, copy_idx=SP_IDX, copy_index={0: [1], 1: [0]})


ORDER_P = (1 / 8, 3 / 8, 5 / 8)


@functools.lru_cache(maxsize=None)
def order_case(S):
    """nS p = k + 1/2 exactly: S = 4 gives nS = 4, 8, 12, 16 and S = 5 gives 5, 10, 15, 20"""
    loci = [I for p in ORDER_P for I in (0, 1, 2, 3, 5)]
    pe = [p for p in ORDER_P for _ in range(5)]
    return case(population(S), loci, pe, [0.0] * len(loci), 0, 0.0, 'sphere')


# a third genome: 64 single-copy loci, one structure, bead h at ((2 h + 1)/64, 0, 0)
DEC_N = 64
DEC_PTR = np.arange(DEC_N + 1, dtype=np.int32)
DEC_IDX = np.arange(DEC_N, dtype=np.int32)[::-1].copy()     # locus h is bead 63 - h
DEC_RADII = np.full(DEC_N, 0.5, f32)
DEC_INDEX = {h: [DEC_N - 1 - h] for h in range(DEC_N)}


def _dec_xyz():
    xyz = np.zeros((DEC_N, 1, 3), f32)
    for h in range(DEC_N):
        xyz[DEC_N - 1 - h, 0, 0] = (2 * h + 1) / 64.0
    return xyz


@functools.lru_cache(maxsize=None)
def decimal_case():
    """ad = odd/64 and p = odd/64 exactly: six decimals ending in 5, a tie of '%.5f'"""
    odd = [(2 * h + 1) / 64.0 for h in range(DEC_N)]
    return case(_dec_xyz(), range(DEC_N), odd, [0.0] * DEC_N, 0, 0.0, 'sphere', radii=DEC_RADII, copy_ptr=DEC_PTR,
                copy_idx=DEC_IDX, copy_index=DEC_INDEX)


@functools.lru_cache(maxsize=None)
def nloci_case(n):
    """n loci in one call, descending and repeating: the edges of check_loci_kernel,
    damid_nrows_kernel and the scan"""
    loci = [(DEC_N - 1 - i) % DEC_N for i in range(n)]
    pe = [PE_PL[i % len(PE_PL)][0] for i in range(n)]
    return case(_dec_xyz(), loci, pe, [0.0] * n, 2, 0.0, 'sphere', radii=DEC_RADII, copy_ptr=DEC_PTR,
                copy_idx=DEC_IDX, copy_index=DEC_INDEX)


AXIS_OF = {1: 0, 2: 1, 3: 2}      # the beads of locus 1 lie on x, of locus 2 on y, of locus 3 on z


@functools.lru_cache(maxsize=None)
def axes_case(cr, it_corr=1):
    """every copy of a locus on one axis, so D0, D1 and D2 each decide a locus alone"""
    S = 65
    xyz = population(S).copy()
    c0 = dict(copy_ptr=COPY_PTR, copy_idx=COPY_IDX)
    for I, ax in AXIS_OF.items():
        for b in copies(c0, I):
            keep = xyz[b, :, ax].copy() * (ax + 1)     # further out on the longer axes
            xyz[b] = 0.0
            xyz[b, :, ax] = keep
    c1 = case(xyz, [], [], [], it_corr, cr, 'ellipsoid')
    return case(xyz, *_listing([3, 2, 1, 0], PE_PL[:8], c1), it_corr, cr, 'ellipsoid')


def zero_copy_case():
    """locus 4 has no copy: no rows, nrows 0, o -1, and the offsets after it are right"""
    loci = [1, 4, 3, 4, 0]
    return case(population(5), loci, [0.5, 0.5, 0.25, 0.75, 0.125], [0.0] * 5, 0, 0.05, 'sphere')


def golden_cases():
    """name -> case: what the reference itself is run on (make_golden_damid_edges.py)"""
    out = {}
    for S in S_GOLDEN:
        for shape in ('sphere', 'ellipsoid'):
            for cr in (0.05, 0.0):
                for it in (0, 1):
                    out['ploidy_s%d_%s_cr%g_i%d' % (S, shape, cr, it)] = ploidy_case(S, shape, cr, it)
        out['radix_s%d' % S] = radix_case(S)
    for it in (0, 1):
        out['special_i%d' % it] = special_case(it)
    out['order_s4'], out['order_s5'] = order_case(4), order_case(5)
    out['decimal'] = decimal_case()
    for cr in (0.05, 0.0):
        out['axes_cr%g' % cr] = axes_case(cr)
    return out


# ---------------------------------------------------------------------------- igm_damid_select
SEL_ABC = (2.5, 1.5, 4.5)
SEL_AXES = (2.0, 1.0, 4.0)          # abc - r at contact range 0, r = 0.5
TRAP_D = [0.75, 1.5, 0.3125, 1.0 + 2.0 ** -11, 4095 / 4096.0]   # at most 12 significant bits
SQ_DOWN = f32(1.0 + 3 * 2.0 ** -23)   # f32(d d) < d d: v = f32(d d) is below the f64 square
SQ_UP = f32(1.0 + 2.0 ** -12 + 2.0 ** -23)      # f32(d d) > d d
SCALE = (1.0, 2.0, 0.5)             # structure s holds the beads scaled by SCALE[s % 3]


def _rows(loc, dist):
    r = np.zeros(len(loc), damid_row_dtype)
    r['loc'], r['dist'] = loc, dist
    r['prob'] = 0.5
    return r


@functools.lru_cache(maxsize=None)
def select_traps(S=3):
    """(xyz (S, N, 3), radii, rows, want (N,) bool for structure 0).  For every axis and every d of
    TRAP_D three beads at d * (abc - r) on that axis: the rows name them with dist = d (v == d^2,
    selected), the f32 above d (not selected) and the f32 below (selected).  Then two beads at
    (0, d, 0) (b - r = 1): v = f32(d d) exactly; for SQ_DOWN that is below the f64 square (not
    selected, the f32 square would select), for SQ_UP above."""
    pos, dist, want = [], [], []
    for ax in range(3):
        for d in TRAP_D:
            p = [0.0, 0.0, 0.0]
            p[ax] = d * SEL_AXES[ax]
            for dd, w in ((f32(d), True), (np.nextafter(f32(d), f32(np.inf)), False),
                          (np.nextafter(f32(d), f32(-np.inf)), True)):
                pos.append(p)
                dist.append(dd)
                want.append(w)
    for d, w in ((SQ_DOWN, False), (SQ_UP, True)):
        pos.append([0.0, float(d), 0.0])
        dist.append(d)
        want.append(w)
    pos = np.array(pos, f32)
    xyz = np.stack([pos * f32(SCALE[s % 3]) for s in range(S)])
    return xyz, np.full(len(pos), 0.5, f32), _rows(np.arange(len(pos)), np.array(dist, f32)), np.array(want)


ROW_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 513)
HIT_MODES = ('two_thirds', 'last_wave', 'lanes_0_63')
NEVER = f32(1e30)


@functools.lru_cache(maxsize=None)
def select_population(S, natom):
    """(S, natom, 3) on j/64 with every bead inside and outside v = 1 somewhere"""
    rng = np.random.default_rng(7000 + 1000 * S + natom)
    xyz = (rng.integers(-160, 161, (S, natom, 3)) / 64.0).astype(f32)
    xyz.setflags(write=False)
    return xyz


def select_rows(n, natom, mode):
    """n rows; row q names bead 7 q mod natom (beads repeat once n > natom).  The rows that can
    hit carry dist = 1 (selected where v >= 1, so it depends on the structure), the others 1e30:
    'two_thirds' two rows of three, 'last_wave' only rows of the last partial wave, 'lanes_0_63' only
    lanes 0 and 63 of every wave."""
    q = np.arange(n)
    if mode == 'two_thirds':
        can = q % 3 != 1
    elif mode == 'last_wave':
        can = q >= 64 * ((n - 1) // 64)
    else:
        can = (q % 64 == 0) | (q % 64 == 63)
    return _rows((7 * q) % natom, np.where(can, f32(1.0), NEVER).astype(f32))


def with_junk(rows, natom):
    """the rows with loc = -1 and loc = natom put in front, in the middle and at the end"""
    junk = _rows([-1, natom, -1, natom], [0.0] * 4)     # dist 0 would select any bead
    h = len(rows) // 2
    return np.concatenate([junk[:1], rows[:h], junk[1:3], rows[h:], junk[3:]])


def select_expected(select_restatement, xyz, radii, rows, abc, cr, bit, base):
    """(flags (S, N), n_selected (S,)) from the per-bead restatement run row by row: n_selected
    counts rows, the flag is set once"""
    S, N = xyz.shape[0], xyz.shape[1]
    out = np.repeat(np.asarray(base, np.uint32)[None], S, 0)
    nsel = np.zeros(S, np.int32)
    for s in range(S):
        for q in range(len(rows)):
            loc = int(rows['loc'][q])
            if 0 <= loc < N and select_restatement(xyz[s], radii, rows[q:q + 1], abc, cr)[loc]:
                out[s, loc] |= np.uint32(bit)
                nsel[s] += 1
    return out, nsel


def base_pattern(natom, bit):
    """base flags that already hold other bits, and the envelope bit itself on every fifth bead"""
    rng = np.random.default_rng(99 + natom)
    b = rng.integers(0, 1 << 32, natom, dtype=np.uint64).astype(np.uint32) & ~np.uint32(bit)
    b[::5] |= np.uint32(bit)
    return b


def env_bit(index):
    return int(IGM_ATOM_ENV0 << index)


# ---------------------------------------------------------------------------- exp_map
@functools.lru_cache(maxsize=None)
def maps():
    """three sphere maps of 11, 13 and 11 voxels a side; every grid step is a power of two, so a
    voxel centre, a half-step and a bead's offset from them are exact in f32 and f64"""
    from igm_amd import volume as V
    return (V.sphere_map(2.0, 0.5, margin=1),
            V.sphere_map(1.25, 0.25, margin=1, body_idx=1, center=(0.5, -0.25, 1.0)),
            V.sphere_map(3.0, 1.0, margin=2, center=(-1.0, 0.0, 2.0)))


SMAP_PATTERN = (2, 0, 1, 1, 0, 2, 0)


def struct_map(S):
    return np.array([SMAP_PATTERN[s % len(SMAP_PATTERN)] for s in range(S)], np.int32)


def voxel_index(x, vol):
    """np.round((x - origin) / grid) in float64, and the unrounded value"""
    o, g = (np.asarray(vol[k], f32).astype(np.float64) for k in ('origin', 'grid'))
    u = (np.asarray(x, f32).astype(np.float64) - o) / g
    return np.round(u).astype(np.int64), u


OFFSETS = (0.0, 0.5, 0.25, -0.25, -0.5)


@functools.lru_cache(maxsize=None)
def exp_population(S, kind):
    """(12, S, 3) f32.  Structure s lives on its own map: 'centre' puts every bead on a voxel
    centre with index -1 .. n (one voxel outside each face included); 'off' adds 0, 1/2, 1/4, -1/4
    or -1/2 of a grid step per axis, so beads sit exactly on voxel half-steps, k + 1/2 with k even
    and odd."""
    rng = np.random.default_rng(9000 + 10 * S + (kind == 'off'))
    sm, M = struct_map(S), maps()
    xyz = np.zeros((NBEAD, S, 3))
    for s in range(S):
        m = M[sm[s]]
        n = int(m['nvoxel'][0])
        idx = rng.integers(-1, n + 1, (NBEAD, 3)).astype(np.float64)
        if kind == 'off':
            idx = idx + np.array(OFFSETS)[rng.integers(0, len(OFFSETS), (NBEAD, 3))]
        xyz[:, s] = m['origin'].astype(np.float64) + idx * m['grid'].astype(np.float64)
    out = xyz.astype(f32)
    assert np.array_equal(out.astype(np.float64), xyz)
    out.setflags(write=False)
    return out


EXP_S = (1, 64, 65, 257)
EXP_CR = (0.25, 0.3)               # a squared distance: some keys equal 0.25, none equals 0.3
EXP_PE_PL = [(0.5, 0.0), (0.25, 0.99), (0.75, 1.0), (0.3, 1.5), (0.01, 0.0), (1e-7, 0.0), (1.5, 0.0),
             (5 / 64, 0.0), (37 / 64, 0.0), (1 / 8, 0.0), (3 / 8, 0.0), (5 / 8, 0.0)]
EXP_LOCI = [3, 1, 0, 5, 2]


def exp_listing():
    loci = [I for _ in EXP_PE_PL for I in EXP_LOCI]
    pe = np.array([a for (a, _) in EXP_PE_PL for _ in EXP_LOCI], f32)
    pl = np.array([b for (_, b) in EXP_PE_PL for _ in EXP_LOCI], f32)
    return loci, pe, pl


def exp_keys(S, kind, nucl, I):
    """the f64 keys of locus I on its structures' maps, copy-major"""
    import nuclear_bodies as NB
    x, sm, M = exp_population(S, kind), struct_map(S), maps()
    c0 = dict(copy_ptr=COPY_PTR, copy_idx=COPY_IDX)
    return np.array([NB.snormsq_exp(x[b, s], M[sm[s]], nucl)[0] for b in copies(c0, I) for s in range(S)])


def exp_expected(S, kind, nucl, cr, it_corr):
    """rows of oracle.asteps.damid_actdist_exp (exp_map) or nuclear_bodies.nucl_damid_actdist"""
    import nuclear_bodies as NB
    loci, pe, pl = exp_listing()
    fn = NB.nucl_damid_actdist if nucl else OA.damid_actdist_exp
    return fn(exp_population(S, kind), COPY_PTR, COPY_IDX, loci, pe, pl, it_corr, cr, list(maps()),
              struct_map(S)).astype(damid_row_dtype)


# ---- igm_volume_select
VS_T = [f32(0.125), f32(0.2), f32(-0.1875), f32(0.0999)]     # offsets from a voxel centre on a 0.5 grid, |t| < 1/4


def _sq_up_offset():
    """an f32 t in (0.2, 0.25) whose f32 square rounds up: t^2 in f64 is below f32(t t)"""
    t = f32(0.2)
    while not np.float64(f32(t * t)) > np.float64(t) * np.float64(t):
        t = np.nextafter(t, f32(1.0))
    return t


@functools.lru_cache(maxsize=None)
def volume_traps():
    """(xyz (3, N, 3) f32, T (3, N) f32): structure s lies on map s.  The outermost lamina voxel
    (k, c, c) on the +x axis through the centre voxel c is its own nearest lamina voxel, so a bead
    at its centre plus (0, t, 0) has v = T^2 exactly, T the f32 |y - centre|.  The last bead of
    structure 0 (map centre 0, so T = t) carries a t whose f32 square rounds up."""
    M = maps()
    ts = VS_T + [_sq_up_offset()]
    xyz = np.zeros((3, len(ts), 3), f32)
    T = np.zeros((3, len(ts)), f32)
    for s, m in enumerate(M):
        n = int(m['nvoxel'][0])
        c = (n - 1) // 2
        lam = m['matrice']
        k = max(i for i in range(n) if lam[i, c, c, 3] and tuple(lam[i, c, c, :3]) == (i, c, c))
        g, o = m['grid'].astype(np.float64), m['origin'].astype(np.float64)
        centre = o + np.array([k, c, c]) * g
        for b, t in enumerate(ts):
            p = centre.copy()
            p[1] += np.float64(t) * g[1] / 0.5
            xyz[s, b] = p.astype(f32)
            te = abs(np.float64(xyz[s, b, 1]) - centre[1])
            assert np.float64(f32(te)) == te and np.array_equal(xyz[s, b, ::2].astype(np.float64), centre[::2])
            T[s, b] = te
    return xyz, T


def volume_trap_rows(t):
    """three rows a bead: dist = T (v == d^2: not selected, the test is <), the f32 above T
    (selected) and the f32 below (not selected)"""
    t = np.asarray(t, f32)
    dist = np.stack([t, np.nextafter(t, f32(np.inf)), np.nextafter(t, f32(0.0))], 1).ravel()
    return _rows(np.repeat(np.arange(len(t)), 3), dist)


def volume_expected(xyz, rows, smap, bit, base):
    """(flags, n_selected) of nuclear_bodies.volume_select / volume_select_rows"""
    import nuclear_bodies as NB
    N = xyz.shape[1]
    ok = (rows['loc'] >= 0) & (rows['loc'] < N)
    index = {1 << (4 + e): e for e in range(4)}[bit]
    flags = NB.volume_select(xyz, rows[ok], list(maps()), smap, index, base)
    nsel = NB.volume_select_rows(xyz, rows[ok], list(maps()), smap).sum(1).astype(np.int32)
    return flags, nsel
