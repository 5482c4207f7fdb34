"""Constructed bond sets at the edges of the M-step bond tables.

Every M-step engine reads a structure's bonds through the device table that prepare()
builds (adj_degree_kernel / adj_slices_kernel / adj_fill_kernel in igm_amd/csrc/mstep.hip):
distinct (r0, k) pairs ranked by bit pattern, every bond packed as
j | type << 16 | lower << 31 into a sliced ELLPACK, each atom's entries sorted.  The sets
here sit on the limits under which the engines re-pack or stage that table.  They build
on small_models.make(): its atoms, radii, polymer, the two envelopes, 'random' geometry,
S = 3 (rest_cap: S = 5, one structure per count), seed = natom.  The per-structure bonds
are replaced; distances come from the structure's own coordinates.

Rules of every set, checked by tests/test_bond_tables.py on the CPU:
  * the one bond of the highest-ranked type (r0 = R_HI = 8192 nm, the largest r0: keys
    order by the r0 bits, then the k bits) is a lower bound with r < r0, so it is active;
  * the one bond of the lowest-ranked type (r0 = 10 nm, upper) is active as well;
  * no bond has i == j;
  * the number of distinct (r0, k) of a structure is exactly what the set says.
The polymer of make() has 5 types (r0 = 2 (r_i + r_j) over radii {100, 150, 200}, k = 1).

Sets (case(name, natom)); natom 257 runs on the population engine, 1100 on the LDS
kernels <1024, 2>, 2100 on <1024, 3>:
  types8 / types9 / types512 / types513 / types4096
        exactly n distinct types in every structure.  After LO and HI the added types are,
        in this order: DUAL (300, 0.7), used once as an upper and once as a lower bound
        (one type); one ulp above it in k; one ulp above it in r0; (300, 0.9) (k alone
        differs); (310, 0.7) (r0 alone differs); then a grid.  types8 stops after DUAL and
        types9 after the ulp in k; the larger sets hold all of them.
  mixed8_9_8, mixed512_513_3
        the per-structure decisions inside one call, and tbase.  mixed512_513_3 passes no
        shared array at all (shared_bonds None: the polymer rides in the rows); its third
        structure has LO, HI and the polymer bonds of one type only.
  degrees8, degrees9
        atoms of degree 0 (the dummy), 1, 3, 4, 5, 31, 32, 33 and 64, polymer bonds
        counted: 33 at atom 0, 32 at atom 63 and 31 at atom 64 (a slice boundary), 64 at
        the last bead.  An atom's entries sort as uppers by type rank, then lowers: LO
        bonds, its polymer bonds, three idle MID bonds (upper, r0 = 7168 > r: what the
        pruning masks drop), then HI-type lower bounds -- every entry from index 17 on, so
        every entry from index 30 on, is active.  8 types (LDS-staged); degrees9 adds one
        type, so the LDS engine reads the same bonds from HBM.  (Only here HI and LO have many
        bonds; the recorded ones are two of the degree-64 atom's.)
  hub_dummy, hub_bead
        min(600, nbead - 3) beads bonded to one atom: the dummy (non-bead, FIXED, last atom,
        last and partial slice) or bead nbead // 2.  Alternating upper / lower bounds of
        one type, LO and HI among them; 8 types.
  duplicates
        one bond three times; one pair as (i, j) and as (j, i); one bond in the shared
        array and in the row.  8 types.
  shared_only
        sbond_ptr None: polymer, LO, HI and DUAL bonds in the shared array (R_HI and 10 nm
        keep HI and LO active in every structure's coordinates).
  rest_cap
        5 structures whose total bond counts are edge - 2 .. edge + 2 at 8 types, where
        edge is the last count the LDS anneal kernel stages (below).  natom 1100, 2100.

The LDS staging capacity, from carve_md_lds (kLdsBytes = 160 KB - 1 KB = 162 816,
kCellCap 4096, kLdsListSlots 8, kLdsBondTypes 8, kMaxWaves 16; every take is aligned to 16 B
and every size below is a multiple of 16):
    carve_red     3 x 16 x 8 doubles 3072 + wsum 64 + misc 64 + gp 32 + gn 32   =  3 264
    npad = 2048   pos 32 768, cell (4096 + 8) x 2 = 8208, nnb 4096, sorted 4096,
                  boff (2048 + 8) x 2 = 4112, btab 128, lell 8 x 2048 x 2 = 32 768
                  -> 89 440 carved, 73 376 B left: rest_cap = 36 688 u16 entries
    npad = 3072   pos 49 152, cell 8208, nnb 6144, sorted 6144, boff 6160, btab 128,
                  lell 49 152 -> 128 352 carved, 34 464 B left: rest_cap = 17 232
A bond is two entries and the kernel asks (2 nb + 7) & ~7 <= rest_cap; both capacities are
multiples of 8, so the last staged counts are 18 344 and 8616 bonds (rest_cap_py() redoes
the carve; the CPU test holds it to these figures).  The other clause, nbent < 0xFFFF,
cannot bind at these sizes: nbent <= rest_cap <= 36 688 < 65 535 wherever the capacity
clause holds, and block_scan saturates at 0xFFFF, so it only matters for an npad whose
rest_cap reaches 65 535 -- none of the LDS configurations.  It is not tested.

CPU-side f32 headroom (small_models.f32_headroom form, 1e-5 ||F64|| / ||F32 - F64|| over
the batch, numpy float32) is asserted >= 10 for every (set, natom) the GPU tests use.
brute() is small_models.brute_batch with the forces of FIXED atoms zeroed (fix setforce:
the hub_dummy bonds pull on the dummy, which neither the oracle nor the engines move).
"""
import numpy as np

import small_models as sm
from igm_amd import model as M
from igm_amd._lib import LOWER_BOUND_BIT, bond_dtype

R_HI, K_HI = np.float32(8192.0), np.float32(0.01)
R_LO, K_LO = np.float32(10.0), np.float32(0.01)
R_MID, K_MID = np.float32(7168.0), np.float32(0.02)
R_HUB, K_HUB = np.float32(700.0), np.float32(0.02)
DUAL = (np.float32(300.0), np.float32(0.7))
REST_EDGE = {1100: 18344, 2100: 8616}  # last staged bond count (npad 2048, 3072)
REST_CAP = {2048: 36688, 3072: 17232}
SIZES = (257, 1100, 2100)
TYPE_COUNTS = (8, 9, 512, 513, 4096)
NAMES = tuple('types%d' % n for n in TYPE_COUNTS) + (
    'mixed8_9_8', 'mixed512_513_3', 'degrees8', 'degrees9', 'hub_dummy', 'hub_bead', 'duplicates', 'shared_only',
    'rest_cap')


def sizes_of(name):
    return (1100, 2100) if name == 'rest_cap' else SIZES


def rest_cap_py(npad, lds_bytes=160 * 1024 - 1024, cellcap=4096, kl=8, btypes=8, waves=16):
    """carve_md_lds in Python: the u16 entries left after the carve"""
    o = 0
    for nbytes in (waves * 8 * 8,) * 3 + (waves * 4, 16 * 4, 8 * 4, 8 * 4, npad * 16, (cellcap + 8) * 2, npad * 2,
                                          npad * 2, (npad + 8) * 2, btypes * 16, kl * npad * 2):
        o = ((o + 15) & ~15) + nbytes
    o = (o + 15) & ~15
    return max(lds_bytes - o, 0) // 2


class Case(object):
    """shared / ptr / sb as the C ABI takes them (shared or ptr + sb may be None);
    hi[s], lo[s]: (i, j) of the structure's highest- and lowest-type bond; ntype[s]: its
    distinct (r0, k); named: {atom: degree} constructed in every structure."""

    def __init__(self, name, natom, atoms, prm, shared, ptr, sb, x, hi, lo, ntype, named=None):
        self.name, self.natom, self.atoms, self.prm = name, natom, atoms, prm
        self.shared, self.ptr, self.sb, self.x = shared, ptr, sb, x
        self.hi, self.lo, self.ntype, self.named = hi, lo, ntype, named or {}

    def bonds(self, s):
        sh = self.shared if self.shared is not None else np.zeros(0, bond_dtype)
        return sm.struct_bonds(sh, self.ptr, self.sb, s)

    def args(self):
        """(radii, flags, shared, ptr, sb) as mstep.forces / oracle.mstep_forces take them"""
        return self.atoms.radii, self.atoms.flags, self.shared, self.ptr, self.sb


def mk(i, j, r0, k, lower=False):
    i = np.atleast_1d(np.asarray(i, np.int64))
    b = np.zeros(len(i), bond_dtype)
    b['i'] = i
    b['j'] = np.asarray(j, np.int64).astype(np.uint32) | np.where(np.broadcast_to(lower, i.shape), LOWER_BOUND_BIT,
                                                                   np.uint32(0)).astype(np.uint32)
    b['r0'] = r0
    b['k'] = k
    return b


# ------------------------------------------------------------------ the table, as adj_fill_kernel builds it
def keys(b):
    """the 64-bit type key: r0 bits, then k bits"""
    return (b['r0'].view(np.uint32).astype(np.uint64) << np.uint64(32)) | b['k'].view(np.uint32).astype(np.uint64)


def partners(b):
    return b['i'].astype(np.int64), (b['j'] & np.uint32(0x7fffffff)).astype(np.int64), (b['j'] >> np.uint32(31)) != 0


def degrees(b, natom):
    i, j, _ = partners(b)
    return np.bincount(i, minlength=natom) + np.bincount(j, minlength=natom)


def entry_order(b, atom):
    """indices into b of the atom's entries, in the table's order (partner | rank << 16 | lower << 31)"""
    i, j, low = partners(b)
    rank = np.searchsorted(np.unique(keys(b)), keys(b))
    rows = np.concatenate([np.flatnonzero(i == atom), np.flatnonzero(j == atom)])
    other = np.concatenate([j[i == atom], i[j == atom]])
    packed = other | (rank[rows] << 16) | (low[rows].astype(np.int64) << 31)
    return rows[np.argsort(packed, kind='stable')]


def lengths(x_s, b):
    i, j, _ = partners(b)
    return np.linalg.norm(x_s[i].astype(np.float64) - x_s[j].astype(np.float64), axis=1)


def active(x_s, b):
    r = lengths(x_s, b)
    return np.where(partners(b)[2], r < b['r0'], r > b['r0']) & (r > 0)


def brute(c, dtype=np.float64, parts=False, envelopes=sm.ENV_TWO):
    """small_models.brute_batch of the case, FIXED atoms' forces zeroed (fix setforce)"""
    sh = c.shared if c.shared is not None else np.zeros(0, bond_dtype)
    out = sm.brute_batch(c.atoms, sh, c.ptr, c.sb, c.x, envelopes, sm.EVF, sm.ENVF, dtype, parts)
    fixed = (c.atoms.flags if c.atoms.flags.ndim == 1 else c.atoms.flags[0]) & M.IGM_ATOM_FIXED != 0
    out[0][:, fixed] = 0.0
    return out


# ------------------------------------------------------------------ pieces
def _pairs(rng, nbead, n):
    i = rng.integers(0, nbead, n)
    return i, (i + 1 + rng.integers(0, nbead - 1, n)) % nbead  # j != i


def _filler_types(have, n):
    """n (r0, k) float32 pairs outside `have` (a set of keys), in the documented order"""
    r, k = DUAL
    cand = [(r, k), (r, np.nextafter(k, np.float32(2))), (np.nextafter(r, np.float32(1e4)), k), (r, np.float32(0.9)),
            (np.float32(310.0), k)]
    out, q = [], 0
    while len(out) < n:
        if len(out) < len(cand):
            t = cand[len(out)]
        else:
            t = (np.float32(100.5 + 0.171875 * q), np.float32(0.5 + 0.0625 * (q % 8)))
            q += 1
        key = int(keys(mk([0], [1], t[0], t[1]))[0])
        if key in have:
            assert len(out) >= len(cand), 'a documented type collides'
            continue
        have.add(key)
        out.append(t)
    return out


def _hi_lo(x_s, rng, nbead, pair_hi=None, pair_lo=None):
    """the HI and LO bonds of a structure: [HI lower, LO upper], both active"""
    (a, b), (c, d) = pair_hi or _one_pair(rng, nbead), pair_lo or _one_pair(rng, nbead)
    out = np.concatenate([mk([a], [b], R_HI, K_HI, True), mk([c], [d], R_LO, K_LO)])
    assert np.all(active(x_s, out)), 'HI / LO bond not active'
    return out, (a, b), (c, d)


def _one_pair(rng, nbead):
    i, j = _pairs(rng, nbead, 1)
    return int(i[0]), int(j[0])


def _typed_row(x_s, rng, nbead, have_bonds, n):
    """bonds that bring a structure holding have_bonds to exactly n distinct types"""
    have = set(int(k) for k in np.unique(keys(have_bonds)))
    need = n - len(have)
    assert need >= 2
    hl, hi, lo = _hi_lo(x_s, rng, nbead)
    types = _filler_types(have, need - 2)
    i, j = _pairs(rng, nbead, len(types))
    fill = mk(i, j, [t[0] for t in types], [t[1] for t in types], np.arange(len(types)) % 3 == 1)
    extra = [hl, fill]
    if types:  # DUAL a second time, as a lower bound
        a, b = _one_pair(rng, nbead)
        extra.append(mk([a], [b], DUAL[0], DUAL[1], True))
    return np.concatenate(extra), hi, lo


def _base(natom, nstruct=3):
    atoms, poly, prm, _, _, x = sm.make(natom - 1, nstruct, natom, envelopes=sm.ENV_TWO, nbonds=0)
    return atoms, poly, prm, x, np.random.default_rng(7000 + natom)


def _case(name, natom, atoms, prm, shared, rows, x, hi, lo, ntype, named=None):
    ptr, sb = M.concat_bonds(rows) if rows is not None else (None, None)
    return Case(name, natom, atoms, prm, shared, ptr, sb, x, hi, lo, ntype, named)


# ------------------------------------------------------------------ the sets
def _types(name, natom, counts, own_polymer=False):
    atoms, poly, prm, x, rng = _base(natom)
    nbead = natom - 1
    rows, his, los = [], [], []
    for s, n in enumerate(counts):
        mine = poly
        if n < 5:  # fewer types than the polymer has: keep its bonds of the commonest type only
            u, cnt = np.unique(keys(poly), return_counts=True)
            mine = poly[keys(poly) == u[np.argmax(cnt)]]
        row, hi, lo = _typed_row(x[s], rng, nbead, mine, n)
        rows.append(np.concatenate([mine, row]) if own_polymer else row)
        his.append(hi)
        los.append(lo)
    return _case(name, natom, atoms, prm, None if own_polymer else poly, rows, x, his, los, list(counts))


def _degree_named(nbead):
    """{atom: degree}: atom 0, the slice boundary 63 | 64, the last bead; the last bead of
    the second chromosome keeps its one polymer bond; the dummy (nbead) has none"""
    end1 = 2 * ((nbead + 3) // 4) - 1
    return {0: 33, 63: 32, 64: 31, nbead - 1: 64, nbead: 0, end1: 1, 100: 3, 130: 4, 160: 5}


def _degrees(name, natom, ntype):
    atoms, poly, prm, x, rng = _base(natom)
    nbead = natom - 1
    named = _degree_named(nbead)
    assert len(named) == 9
    polydeg = degrees(poly, natom)
    pool = np.array([a for a in range(170, nbead - 1) if a not in named and a + 1 not in named and a - 1 not in named])
    rows, his, los = [], [], []
    for s in range(len(x)):
        row, hi, lo = [], None, None
        for atom, deg in named.items():
            extra = deg - int(polydeg[atom])
            assert extra >= 0
            if extra == 0:
                continue
            other = rng.choice(pool, extra, replace=False)
            nmid = 3 if deg >= 31 else 0
            nlo = min(12, (extra - nmid) // 2)
            kinds = [(R_LO, K_LO, False)] * nlo + [(R_MID, K_MID, False)] * nmid
            kinds += [(R_HI, K_HI, True)] * (extra - len(kinds))
            b = mk(np.full(extra, atom), other, [t[0] for t in kinds], [t[1] for t in kinds], [t[2] for t in kinds])
            row.append(b)
            if deg == 64:
                hi = (atom, int(other[-1]))
                lo = (atom, int(other[0]))
        if ntype == 9:
            a, b = int(pool[0]), int(pool[len(pool) // 2])
            row.append(mk([a], [b], np.float32(450.0), K_MID))
        row = np.concatenate(row)
        act, mid, ninth = active(x[s], row), row['r0'] == R_MID, row['r0'] == np.float32(450.0)
        assert np.all(act[~mid & ~ninth]) and not np.any(act[mid])
        rows.append(row)
        his.append(hi)
        los.append(lo)
    return _case(name, natom, atoms, prm, poly, rows, x, his, los, [ntype] * len(x), named)


def _hub(name, natom, hub_is_dummy):
    atoms, poly, prm, x, rng = _base(natom)
    nbead = natom - 1
    hub = nbead if hub_is_dummy else nbead // 2
    n = min(600, nbead - 3)
    rows, his, los = [], [], []
    for s in range(len(x)):
        other = rng.choice(np.setdiff1d(np.arange(nbead), [hub]), n, replace=False)
        # the hub as i for one half and as j for the other
        b = mk(np.where(np.arange(n) % 4 < 2, hub, other), np.where(np.arange(n) % 4 < 2, other, hub), R_HUB, K_HUB,
               np.arange(n) % 2 == 1)
        b['r0'][0], b['k'][0], b['j'][0] = R_HI, K_HI, b['j'][0] | LOWER_BOUND_BIT
        b['r0'][1], b['k'][1], b['j'][1] = R_LO, K_LO, b['j'][1] & np.uint32(0x7fffffff)
        assert np.all(active(x[s], b[:2]))
        rows.append(b)
        his.append((hub, int(other[0])))
        los.append((hub, int(other[1])))
    named = {hub: n + int(degrees(poly, natom)[hub])}
    return _case(name, natom, atoms, prm, poly, rows, x, his, los, [8] * len(x), named)


def _duplicates(name, natom):
    atoms, poly, prm, x, rng = _base(natom)
    nbead = natom - 1
    (a, b), (c, d), (e, f) = [_one_pair(rng, nbead) for _ in range(3)]
    both = mk([a], [b], R_HUB, K_HUB)  # in the shared array and in every row
    rows, his, los = [], [], []
    for s in range(len(x)):
        hl, hi, lo = _hi_lo(x[s], rng, nbead)
        rows.append(np.concatenate([hl, both, mk([c] * 3, [d] * 3, R_HUB, K_HUB, True), mk([e, f], [f, e], R_HUB, K_HUB)]))
        his.append(hi)
        los.append(lo)
    return _case(name, natom, atoms, prm, np.concatenate([poly, both]), rows, x, his, los, [8] * len(x),
                 {'both': (a, b), 'triple': (c, d), 'swapped': (e, f)})


def _shared_only(name, natom):
    atoms, poly, prm, x, rng = _base(natom)
    nbead = natom - 1
    hi, lo = _one_pair(rng, nbead), _one_pair(rng, nbead)
    for s in range(len(x)):
        hl, _, _ = _hi_lo(x[s], rng, nbead, hi, lo)
    (a, b), (c, d) = _one_pair(rng, nbead), _one_pair(rng, nbead)
    shared = np.concatenate([poly, hl, mk([a], [b], *DUAL), mk([c], [d], DUAL[0], DUAL[1], True)])
    return _case(name, natom, atoms, prm, shared, None, x, [hi] * len(x), [lo] * len(x), [8] * len(x))


def _rest_cap(name, natom):
    atoms, poly, prm, x, rng = _base(natom, 5)
    nbead = natom - 1
    rows, his, los = [], [], []
    for s in range(5):
        total = REST_EDGE[natom] - 2 + s
        hl, hi, lo = _hi_lo(x[s], rng, nbead)
        n = total - len(poly) - 2
        i, j = _pairs(rng, nbead, n)
        rows.append(np.concatenate([hl, mk(i, j, R_HUB, K_HUB, np.arange(n) % 3 == 0)]))
        his.append(hi)
        los.append(lo)
    return _case(name, natom, atoms, prm, poly, rows, x, his, los, [8] * 5, {'total': REST_EDGE[natom]})


_CACHE = {}


def case(name, natom):
    """the Case of a set at a model size, built once (treat it as read-only)"""
    key = (name, natom)
    if key not in _CACHE:
        if name.startswith('types'):
            c = _types(name, natom, [int(name[5:])] * 3)
        elif name == 'mixed8_9_8':
            c = _types(name, natom, [8, 9, 8])
        elif name == 'mixed512_513_3':
            c = _types(name, natom, [512, 513, 3], own_polymer=True)
        elif name.startswith('degrees'):
            c = _degrees(name, natom, int(name[7:]))
        elif name.startswith('hub_'):
            c = _hub(name, natom, name == 'hub_dummy')
        elif name == 'duplicates':
            c = _duplicates(name, natom)
        elif name == 'shared_only':
            c = _shared_only(name, natom)
        elif name == 'rest_cap':
            c = _rest_cap(name, natom)
        else:
            raise ValueError('unknown set %r' % name)
        _CACHE[key] = c
    return _CACHE[key]


def types_counts(natom, counts):
    """an uncached types set with the given number of distinct types per structure (the
    refusal tests: 4097 and 9000 are past what prepare() accepts)"""
    return _types('types', natom, list(counts))


def all_cases():
    return [(name, natom) for name in NAMES for natom in sizes_of(name)]
