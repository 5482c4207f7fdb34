"""Inputs for the MD step of the population engine (igm_amd/csrc/mstep.hip: pop_integrate_kernel,
pop_sort_kernel, pop_permute_kernel, pop_fill_kernel, pop_force_kernel, pop_finish_kernel), and
their CPU-side properties.  tests/test_pop_step.py proves on the CPU that every input is the edge
it claims; tests/test_pop_step_gpu.py runs them through mstep.md / mstep.run against the oracle.

Engines by natom: 1 .. 1024 and 3073 .. 65 535 take the population engine; 1025 .. 3072 the LDS
kernels, unless IGM_MSTEP_FORCE_GLOBAL is set (engine 'global': 1100 here).

Constants of mstep.hip restated here (the CPU test holds the derived edges to the figures):
    kPopBS 256          slots per block of the kernels over every slot; nbs = ceil(N / 256)
    kPopSortNT 1024     threads of a sort workgroup; <true, 16> up to 16 384, <true, 32> up to 32 768
    kPopCellCap 32768   cells of a structure's grid
    kLdsBytes 162 816   160 KB - 1 KB.  pop_sort_lds = 4 ((ccap + 3) / 2) + 2 N with u16 ids in
                        LDS: 65 540 + 2 N <= 162 816 up to N = 48 638, <false, 0> from 48 639 on
    kPopListCap 256     Verlet-list entries of a slot; more: the cell walk (pop_walk_pairs)
    64                  stride of the partial sums over a structure's nbs blocks (pop_factor, the
                        bbox loop of pop_sort_kernel): nbs 64 at N = 16 384, 65 at 16 385

Lattice.  Beads of radius 100 at rest on a cubic lattice, no dummy, no bonds, no envelope that
acts, explicit skin: the list cut is 2 x 100 + skin, below the spacing, so nothing is in any list.
The atoms are dealt onto the sites by a random permutation (every radius is the same, so the
physics do not see it): atom id and slot are uncorrelated, and every list build permutes.

Slot order.  After a build the slots of a structure are in cell order, x fastest, ascending atom
ids inside a cell.  slots_of() restates pop_grid_of / pop_cell_xyz in float32 NumPy.

Bullet.  One bead starts START = 350 from a lattice neighbour (outside the list cut of 300) and
flies at it with |v| = 160: 40 per step, past skin / 2 = 50 every second step.  The pair overlaps
(r < 200) from step 4 on; with evf = 1 the barrier 2 (200 / pi)^2 = 8106 is above the collision's
kinetic energy in the centre-of-mass frame, 160^2 / 4 = 6400, so the bullet hands its velocity to
the target.  Only a list rebuilt from the bullet's vote shows the pair: a lost vote, a stale
counter or a flag on the wrong structure leaves the bullet in free flight.
    sites   'low'  the lattice's lowest corner: slot 0, first block, lane 0
            'last' the highest occupied site: the last slot, last block
            'mid'  a site near the middle in one of the last lanes of its block (MID_SITE), so a
                   flight along y (its slot moves by about a row) or z (a layer) takes it into
                   the next block
    ids     0, natom // 2, natom - 1
    axes    x (the slot shifts by a few at most), y, z
A flight leaves the block where slot arithmetic allows it: always from 'mid' (natom >= 1024),
from 'last' where the last block is smaller than a row (257, 16 385, 32 769) -- block_change()
says which, and the CPU test asserts it for those.  natom 257 has two blocks, the second of one
slot: only 'last' can change block there.

Thermostat.  The cases of test_anneal_step_gpu.py on model(): small_models.make at 257, 1024,
3073 and 16 385 atoms (65 partials; 10 steps there).  These models end in their FIXED dummy, the
last slot, so last_block_case() puts 80 % of a lattice's kinetic energy into the 65th partial.
dof_inputs(): (S, N) flags that hold no bead, every 7th, every 3rd.

nve/limit.  limit_free_case(): three beads at |v| = 160 leave the lattice's low faces under
xmax = 10; limit_forces_oracle(): model() under xmax = 1 with the thermostat on.  Both also at
1025 and 3072, on the LDS anneal kernel.

Cell walk.  walk_inputs(): 'dense' at 1024 and 1100, 20 steps: lists past kPopListCap before and
after the beads have moved.

run().  run_case(): lattice structures 1300 apart, skin 50, under run_protocol() -- mdsteps
(5, 6, 7, 4), relax 3, T 400 .. 200, max_velocity 15 (relax: 10), so nve/limit bounds every path
and no pair ever interacts; run_mixed_x() adds overlapping random structures to the batch.
"""
import json

import numpy as np

import oracle
import small_models as sm
from igm_amd import _lib
from igm_amd import model as M
from igm_amd._lib import IGM_MSTEP_FORCE_GLOBAL, bond_dtype

# ------------------------------------------------------------------ constants of mstep.hip, restated
POP_BS = 256
SORT_NT = 1024
CELL_CAP = 32768
CELL_CAP_BIG = 32768
LDS_BYTES = 160 * 1024 - 1024
LIST_CAP = 256
PARTIAL_STRIDE = 64

DT = 0.25  # params.timestep of the demo protocol
NO_ENVELOPE = [((1.0e6, 1.0e6, 1.0e6), 1.0)]  # k > 0 acts outside only: no bead ever gets there
SPACING, RADIUS, SKIN, SPEED, START = 400.0, 100.0, 100.0, 160.0, 350.0
XMAX = 1000.0


def nbs(natom):
    return (natom + POP_BS - 1) // POP_BS


def sort_lds(ids_lds, natom, ccap):
    """pop_sort_lds: LDS bytes of pop_sort_kernel<IDS_LDS> over grids of at most ccap cells"""
    return 4 * ((ccap + 3) // 2) + (2 * natom if ids_lds else 0)


def sort_cells(natom):
    """pop_sort_cells: the grid cap of a run"""
    if sort_lds(True, natom, CELL_CAP) <= LDS_BYTES:
        return CELL_CAP
    room = (LDS_BYTES - 2 * natom) // 2 - 4
    if room >= CELL_CAP_BIG:
        return room & ~63
    return CELL_CAP


def sort_variant(natom):
    """the pop_sort_kernel instantiation run_anneal_pop picks: (IDS_LDS, APT)"""
    if sort_lds(True, natom, sort_cells(natom)) > LDS_BYTES:
        return (False, 0)
    if natom <= 16 * SORT_NT:
        return (True, 16)
    if natom <= 32 * SORT_NT:
        return (True, 32)
    return (True, 0)


def engine_params(prm, engine='default', **kw):
    """a copy of prm, fields set; engine 'global' forces the population engine"""
    p = _lib.MStepParams.from_buffer_copy(prm)
    for k, v in kw.items():
        setattr(p, k, v)
    if engine == 'global':
        p.flags |= IGM_MSTEP_FORCE_GLOBAL
    return p


def engine_of(natom):
    """the engine name under which a size runs on the population engine"""
    return 'default' if natom <= 1024 or natom >= 3073 else 'global'


# ------------------------------------------------------------------ the slot order of a build
def _grid_cap(a, b, c, cap):
    for _ in range(2):
        if a * b * c > cap:
            ma = a >= b and a >= c
            mb = (not ma) and b >= c
            o = b * c if ma else (a * c if mb else a * b)
            q = cap // o if o < cap else 1
            a, b, c = (q if ma else a), (q if mb else b), (c if (ma or mb) else q)
    return a, b, c


def grid_of(x, cut, ccap):
    """pop_grid_of in float32: (lo, inv, nb) of the bead positions x (N, 3)"""
    f = np.float32
    x = np.asarray(x, f)
    lo, hi = x.min(axis=0), x.max(axis=0)
    ext = (hi - lo).astype(f)
    vol = f(1.0)
    for d in range(3):
        vol = f(vol * max(ext[d], f(cut)))
    cs = f(cut)
    if f(vol / f(cs * cs * cs)) > f(ccap):
        cs = f(f(np.cbrt(f(vol / f(ccap)))) * f(1.0001))
    nb = [max(1, int(np.floor(f(ext[d] / cs)))) for d in range(3)]
    nb = _grid_cap(nb[0], nb[1], nb[2], ccap)
    inv = np.array([f(nb[d]) / ext[d] if ext[d] > 0 else f(0) for d in range(3)], f)
    return lo, inv, np.array(nb)


def slots_of(x, cut, ccap=CELL_CAP):
    """slot of every atom after a list build at positions x (N, 3), all beads: cells x fastest
    (pop_cell_xyz: clamped), ascending atom ids inside a cell.  Returns (slot (N,), nb)."""
    x = np.asarray(x, np.float32)
    lo, inv, nb = grid_of(x, cut, ccap)
    c = ((x - lo).astype(np.float32) * inv).astype(np.float32).astype(np.int64)
    c = np.clip(c, 0, nb - 1)
    cell = (c[:, 2] * nb[1] + c[:, 1]) * nb[0] + c[:, 0]
    order = np.lexsort((np.arange(len(x)), cell))
    slot = np.empty(len(x), np.int64)
    slot[order] = np.arange(len(x))
    return slot, nb


# ------------------------------------------------------------------ lattice
class Lattice(object):
    """natom beads at rest; site(k) = (k % n, (k // n) % n, k // n^2) * spacing; atom_at[k] is
    the atom on site k (a random permutation, seed = natom)"""

    def __init__(self, natom, nstruct=1, spacing=SPACING, skin=SKIN, protocol=None, permute=True):
        self.natom, self.spacing, self.skin = natom, spacing, skin
        self.n = n = int(np.ceil(natom ** (1.0 / 3.0) - 1e-9))
        k = np.arange(natom)
        site = np.stack([k % n, (k // n) % n, k // (n * n)], axis=1).astype(np.float64) * spacing
        site -= site.mean(axis=0).round()
        self.site = site.astype(np.float32)
        rng = np.random.default_rng(natom)
        self.atom_at = rng.permutation(natom) if permute else k.copy()
        self.atoms = M.Atoms(np.full(natom, RADIUS, np.float32), n_static_dummies=0)
        self.prm = M.params_from_cfg({'optimization': {'optimizer_options': protocol or sm.DEMO_PROTOCOL}},
                                     NO_ENVELOPE, skin=skin)
        assert self.prm.timestep == DT
        self.poly = np.zeros(0, bond_dtype)
        self.nstruct = nstruct
        self.cut = 2.0 * RADIUS + skin

    def put(self, atom, k):
        """atom `atom` onto site k (it trades places with the site's atom)"""
        j = int(np.flatnonzero(self.atom_at == atom)[0])
        self.atom_at[j], self.atom_at[k] = self.atom_at[k], self.atom_at[j]

    def x(self):
        """(S, N, 3) float32 positions in atom order"""
        x = np.empty((self.natom, 3), np.float32)
        x[self.atom_at] = self.site
        return np.repeat(x[None], self.nstruct, axis=0)

    def neighbour(self, k, axis, d):
        """the site next to k along axis (d = +-1), or -1 if it is not occupied"""
        n = self.n
        c = [k % n, (k // n) % n, k // (n * n)]
        c[axis] += d
        if not 0 <= c[axis] < n:
            return -1
        j = c[0] + n * (c[1] + n * c[2])
        return j if j < self.natom else -1

    def args(self):
        return self.atoms.radii, self.atoms.flags, self.poly, None, None


# 'mid': the site nearest the middle, of lane 254 or the nearest lane below it, with +x, +y and +z
# neighbours, from which the y flight (and below 4096 atoms, where it is run, the z flight) ends in
# another block than it began -- whether a flight of ~150 crosses a cell boundary depends on how
# the grid falls on the lattice.  Found by a search with the oracle; the CPU test asserts the
# change of block for each.  (257: the top layer; the bullet flies down and stays in block 0.)
MID_SITE = {257: 254, 1024: 510, 1100: 510, 3073: 1273, 16384: 8446, 16385: 8446, 32768: 16638, 32769: 16382,
            48638: 24563, 48639: 24563}


def bullet_site(natom, where, axis=0, atom=None):
    """the lattice site of a bullet.  Up to 16 385 atoms every site has a cell of its own and the
    slot of the setup build is the site.  From 32 768 on some cells hold two sites or more (there
    are more atoms than cells, or the capped cell side equals the spacing), ordered by atom id:
    'last' is then the highest site from which the bullet, with its id, gets the last slot."""
    if where == 'low':
        return 0
    if where == 'mid':
        return MID_SITE[natom]
    if natom < 32768:
        return natom - 1
    k = last_slot_site(natom, axis, natom - 1 if atom is None else atom)
    if k is None:
        raise ValueError('no site gives atom %r the last slot of %d along axis %d' % (atom, natom, axis))
    return k


def last_slot_site(natom, axis, atom):
    """the site among those of the last cells from which a bullet of this id, started along
    axis, holds the last slot; None if there is none (a start 50 below a site that lies on a cell
    boundary is in the cell below)"""
    def find():
        lat = Lattice(natom, permute=False)
        slot0, _ = slots_of(lat.x()[0], lat.cut, sort_cells(natom))  # (site order inside a cell)
        for k in np.argsort(-slot0)[:32].tolist():  # the sites of the last cells
            if lat.neighbour(k, axis, 1) < 0 and lat.neighbour(k, axis, -1) < 0:
                continue
            b = Bullets(natom, [[(k, axis, atom, START)]])
            slot, _ = slots_of(b.x[0], b.lat.cut, sort_cells(natom))
            if slot[atom] == natom - 1:
                return k
        return None
    return cached(('last_slot_site', natom, axis, atom), find)


IDS = ('first', 'middle', 'last')


def atom_id(natom, which):
    return {'first': 0, 'middle': natom // 2, 'last': natom - 1}[which]


class Bullets(object):
    """A lattice batch with bullets: per structure a list of (site, axis, atom id, start)."""

    def __init__(self, natom, per_struct, nsteps=20):
        self.natom, self.nsteps = natom, nsteps
        self.lat = lat = Lattice(natom, len(per_struct))
        # one assignment of atoms to sites for the whole batch: the bullets' ids on their sites
        for bl in per_struct:
            for (k, axis, a, start) in bl:
                lat.put(a, k)
        for bl in per_struct:
            for (k, axis, a, start) in bl:
                assert lat.atom_at[k] == a, 'two bullets want one atom or one site'
        self.x = lat.x()
        self.v = np.zeros_like(self.x)
        self.prm = engine_params(lat.prm, t_window=1.0e30)  # no rescale: free flight is exact
        self.bullets = []  # (structure, atom, target atom, axis, d, start)
        for s, bl in enumerate(per_struct):
            for (k, axis, a, start) in bl:
                d = 1 if lat.neighbour(k, axis, 1) >= 0 else -1
                t = lat.neighbour(k, axis, d)
                assert t >= 0
                ta = int(lat.atom_at[t])
                self.x[s, a] = self.x[s, ta]
                self.x[s, a, axis] -= np.float32(d * start)
                self.v[s, a, axis] = d * SPEED
                self.bullets.append((s, a, ta, axis, d, start))

    def free_flight(self, s, a, axis, d):
        return float(self.x[s, a, axis]) + d * SPEED * DT * self.nsteps


def flight_axis(natom, where, axis):
    """the axis itself, or the next one (cyclically) along which the site has a neighbour: the
    last site of 1024 = 11^3 - 307 atoms starts a row, so its x flight becomes a y flight"""
    for a in (axis, (axis + 1) % 3, (axis + 2) % 3):
        if where == 'last' and natom >= 32768:  # (32 769: along x, inside the last cell)
            if last_slot_site(natom, a, natom - 1) is not None:
                return a
            continue
        lat, k = Lattice(natom, permute=False), bullet_site(natom, where)
        if lat.neighbour(k, a, 1) >= 0 or lat.neighbour(k, a, -1) >= 0:
            return a
    raise ValueError('no flight from %r of %d' % (where, natom))


def bullet_cases():
    """(natom, where, axis, which id, nsteps, start): all nine (site, axis) pairs with the ids
    dealt as a Latin square at the four small sizes; at the six sort / stride edges the three
    pairs of its diagonal (low x with the first id, mid y with the middle one, last z with the last
    one: where cells hold several sites, ordered by id, these keep slot 0 and the last slot)"""
    out = []
    for natom in (257, 1024, 1100, 3073):
        for wi, where in enumerate(('low', 'mid', 'last')):
            for axis in range(3):
                out.append((natom, where, flight_axis(natom, where, axis), IDS[(wi + axis) % 3], 20, START))
    for natom in (16384, 16385, 32768, 32769, 48638, 48639):
        for wi, where in enumerate(('low', 'mid', 'last')):
            out.append((natom, where, flight_axis(natom, where, wi), IDS[wi], 20, START))
    return out


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def bullet_case(natom, where, axis, which, nsteps=20, start=START):
    return cached(('bullet', natom, where, axis, which, nsteps, start),
                  lambda: Bullets(natom, [[(bullet_site(natom, where, axis, atom_id(natom, which)), axis, atom_id(natom, which),
                                            start)]], nsteps))


def isolation_case(natom, nstruct=5):
    """S = 5: structures 1 and 3 carry a bullet each, in different blocks (low along y with id
    last; last along z with id first); 0, 2 and 4 are at rest.  S = 1: the first of them."""
    def make():
        b1 = [(bullet_site(natom, 'low'), 1, atom_id(natom, 'last'), START)]
        b3 = [(bullet_site(natom, 'last'), flight_axis(natom, 'last', 2), atom_id(natom, 'first'), START)]
        per = [[], b1, [], b3, []] if nstruct == 5 else [b1]
        return Bullets(natom, per)
    return cached(('isolation', natom, nstruct), make)


def two_bullet_case(natom):
    """two bullets in one structure, in different blocks ('low' along x, 'last' along y); the
    second starts 120 = 3 steps further out (470 from its target, 330 from the site behind it:
    outside every list), so its collision and the builds it causes come three steps later"""
    def make():
        return Bullets(natom, [[(bullet_site(natom, 'low'), 0, atom_id(natom, 'middle'), START),
                                (bullet_site(natom, 'last'), flight_axis(natom, 'last', 1), atom_id(natom, 'first'),
                                 START + 120.0)]])
    return cached(('two', natom), make)


def block_change(case, xo):
    """per bullet: (block before, block after) from the slot order at the start and at the
    oracle's final positions xo"""
    out = []
    for (s, a, ta, axis, d, start) in case.bullets:
        s0, _ = slots_of(case.x[s], case.lat.cut, sort_cells(case.natom))
        s1, _ = slots_of(xo[s], case.lat.cut, sort_cells(case.natom))
        out.append((int(s0[a]) // POP_BS, int(s1[a]) // POP_BS))
    return out


def must_change_block(natom, where, axis):
    """the (site, axis) pairs whose flight leaves the bullet's block by slot arithmetic"""
    if axis == 0:
        return False
    if where == 'mid':
        return natom >= 1024
    if where == 'last':
        n = int(np.ceil(natom ** (1.0 / 3.0) - 1e-9))
        return (natom - 1) % POP_BS < n - 1  # fewer slots before it in its block than a row holds
    return False


# ------------------------------------------------------------------ random models (thermostat, clamp, walk)
THERMO_SIZES = (257, 1024, 3073, 16385)


def thermo_steps(natom):
    return 10 if natom > 4096 else 20


def model(natom, nstruct=2, geometry='random'):
    """a random model of small_models.make (bonds, overlaps, one envelope); past 1024 atoms the
    cloud and its envelope grow with natom^(1/3), so the density stays that of 1024"""
    def make():
        g = max(1.0, (natom / 1024.0) ** (1.0 / 3.0))
        env = [(tuple(a * g for a in sm.ENV_ONE[0][0]), 1.0)]
        return sm.make(natom - 1, nstruct, 2000 + natom, geometry, envelopes=env, sigma=700.0 * g)
    return cached(('model', natom, nstruct, geometry), make)


def fixed_flags(flags, every, first=3):
    fl = flags.copy()
    fl[np.arange(first, len(fl) - 1, every)] |= np.uint32(M.IGM_ATOM_FIXED)
    return fl


def dof_flags(flags):
    """(3, N) flags whose FIXED sets differ per structure: none, every 7th, every 3rd bead"""
    return np.stack([flags, fixed_flags(flags, 7), fixed_flags(flags, 3)])


def temperature(v, flags):
    """compute temp of group nonfixed, per structure: sum v^2 / (3 n_mobile - 3); flags (N,) or (S, N)"""
    v = np.asarray(v, np.float64)
    fl = np.broadcast_to(flags, v.shape[:2])
    mobile = fl & M.IGM_ATOM_FIXED == 0
    return ((v ** 2).sum(axis=2) * mobile).sum(axis=1) / (3.0 * mobile.sum(axis=1) - 3.0)


# ------------------------------------------------------------------ nve/limit
LIMIT_POP = (257, 1024, 3073)
LIMIT_LDS = (1025, 3072)
LIMIT_DIRS = np.array([[0.0, -1.0, 0.0], [-1.0, 0.0, -1.0], [-2.0, -1.0, 0.0]])


def limit_free_case(natom):
    """the lattice at rest and three beads on its low faces, flying outwards with |v| = 160:
    along -y from site (2, 0, 0), along (-1, 0, -1) from (0, 2, 0), along (-2, -1, 0) from
    (0, 0, 2).  Nothing is ever in range, so the velocity only meets the clamp."""
    def make():
        lat = Lattice(natom)
        n = lat.n
        sites = [2, 2 * n, 2 * n * n]
        x = lat.x()
        v = np.zeros_like(x)
        dirs = LIMIT_DIRS / np.linalg.norm(LIMIT_DIRS, axis=1)[:, None]
        who = [int(lat.atom_at[k]) for k in sites]
        for a, u in zip(who, dirs):
            v[0, a] = (SPEED * u).astype(np.float32)
        return lat, x, v, who, dirs
    return cached(('limit_free', natom), make)


# ------------------------------------------------------------------ run(): segments and build counts
RUN_SPACING, RUN_SKIN, RUN_XMAX = 1300.0, 50.0, 15.0
RUN_STEPS, RUN_RELAX = (5, 6, 7, 4), 3


def run_protocol():
    p = json.loads(json.dumps(sm.DEMO_PROTOCOL))
    c = p['custom_annealing_protocol']
    c['mdsteps'] = list(RUN_STEPS)
    c['tstarts'], c['tstops'] = [400.0, 350.0, 300.0, 250.0], [350.0, 300.0, 250.0, 200.0]
    c['evfactors'], c['envelope_factors'] = [1.0] * 4, [1.0] * 4
    c['relax'] = {'mdsteps': RUN_RELAX, 'temperature': 300.0, 'max_velocity': 10.0}
    p['max_velocity'] = RUN_XMAX
    return p


def run_path_bound():
    """the longest path nve/limit lets a bead travel over the protocol"""
    return sum(RUN_STEPS) * RUN_XMAX + len(RUN_STEPS) * RUN_RELAX * 10.0


def run_case(natom, nstruct=3):
    """lattice structures of spacing 1300, skin 50, under run_protocol(): a bead travels at most
    450, two neighbours stay 400 > 2 r + skin = 250 apart -- no pair ever interacts; at 7 to 13 a
    step a bead passes skin / 2 = 25 every two or three steps"""
    return cached(('run', natom, nstruct), lambda: Lattice(natom, nstruct, RUN_SPACING, RUN_SKIN, run_protocol()))


def run_mixed_x(lat, nrandom=2, seed=5):
    """the lattice structures followed by nrandom overlapping random ones (the lattice's atoms
    at normal(0, 700 (N / 1024)^(1/3)) coordinates)"""
    rng = np.random.default_rng(seed + lat.natom)
    sig = 700.0 * max(1.0, (lat.natom / 1024.0) ** (1.0 / 3.0))
    xr = rng.normal(0.0, sig, (nrandom, lat.natom, 3)).astype(np.float32)
    return np.concatenate([lat.x(), xr])


# ------------------------------------------------------------------ the oracle's runs, and what they prove
def xtol(x0, xo):
    """the position bound of the md comparisons: 1e-3 max(1, moved)"""
    return 1e-3 * max(1.0, float(np.abs(xo - x0).max()))


def vtol(vo):
    """at least rtol |v| + atol of the velocity comparison (rtol 1e-3, atol 1e-3 max|v|) at every component"""
    return 2e-3 * float(np.abs(vo).max())


def apart(x0, xo, vo, xw, vw):
    """how far a wrong outcome (xw, vw) lies from the oracle's (xo, vo): (positions, velocities)
    in units of the comparison's tolerances"""
    return (float(np.abs(xw - xo).max()) / xtol(x0, xo), float(np.abs(vw - vo).max()) / max(vtol(vo), 1e-300))


def oracle_md(prm, x, v, atoms, poly, ptr, sb, evf, envf, t0, t1, xmax, nsteps, flags=None):
    return oracle.mstep_md(prm, np.asarray(x, np.float64), np.asarray(v, np.float64), atoms.radii,
                           atoms.flags if flags is None else flags, poly, ptr, sb, evf, envf, t0, t1, xmax, nsteps,
                           nthreads=4)


def bullet_oracle(case):
    """the oracle's (x, v) after the case's steps, computed once"""
    if not hasattr(case, '_oracle'):
        case._oracle = oracle_md(case.prm, case.x, case.v, case.lat.atoms, case.lat.poly, None, None, 1.0, 1.0, 50.0,
                                 50.0, XMAX, case.nsteps)
    return case._oracle


def bullet_power(case, verbose=True):
    """every bullet of the case ends at least 100 tolerances from free flight, in position and in
    velocity, and its target took the momentum -- a stale list cannot pass the comparison"""
    xo, vo = bullet_oracle(case)
    for (s, a, ta, axis, d, start) in case.bullets:
        free_x = case.free_flight(s, a, axis, d)
        vt, xt = vtol(vo[s]), xtol(case.x[s], xo[s])
        if verbose:
            print('natom %d structure %d bullet %d -> %d (axis %d, dir %+d): oracle v %.4g (free %.4g, tol %.3g), '
                  'x %.5g (free %.5g, tol %.3g)' % (case.natom, s, a, ta, axis, d, vo[s, a, axis], d * SPEED, vt,
                                                    xo[s, a, axis], free_x, xt))
        assert abs(vo[s, a, axis] - d * SPEED) >= 100.0 * vt
        assert abs(xo[s, a, axis] - free_x) >= 100.0 * xt
        assert abs(vo[s, ta, axis]) >= 100.0 * vt
    return xo, vo


# thermostat
FIXED_EVERY = 3


def thermo_inputs(natom, fixed=False):
    """model(natom) with T = 50 velocities; fixed: every 3rd bead held (the anneal step's case
    holds every 7th: a dof of all atoms is then 48 allowances off the target, here 143)"""
    def make():
        atoms, poly, prm, ptr, sb, x = model(natom)
        flags = fixed_flags(atoms.flags, FIXED_EVERY) if fixed else atoms.flags
        v = np.stack([oracle.velocity_create(flags, 50.0, 21 + s) for s in range(len(x))]).astype(np.float32)
        assert not v[:, flags & M.IGM_ATOM_FIXED != 0].any()
        return atoms, poly, prm, ptr, sb, x, v, flags
    return cached(('thermo_inputs', natom, fixed), make)


def thermo_oracle(natom, fixed, window, fraction, t0, t1):
    def make():
        atoms, poly, prm, ptr, sb, x, v, flags = thermo_inputs(natom, fixed)
        p = engine_params(prm, t_window=window, t_fraction=fraction)
        return oracle_md(p, x, v, atoms, poly, ptr, sb, sm.EVF, sm.ENVF, t0, t1, XMAX, thermo_steps(natom), flags)
    return cached(('thermo_oracle', natom, fixed, window, fraction, t0, t1), make)


def dof_inputs(natom):
    """S = 3 with (S, N) flags: no bead, every 7th, every 3rd held; T = 50 velocities of each"""
    def make():
        atoms, poly, prm, ptr, sb, x = model(natom, 3)
        flags = dof_flags(atoms.flags)
        v = np.stack([oracle.velocity_create(flags[s], 50.0, 31 + s) for s in range(3)]).astype(np.float32)
        return atoms, poly, prm, ptr, sb, x, v, flags
    return cached(('dof_inputs', natom), make)


def dof_oracle(natom):
    def make():
        atoms, poly, prm, ptr, sb, x, v, flags = dof_inputs(natom)
        return oracle_md(prm, x, v, atoms, poly, ptr, sb, sm.EVF, sm.ENVF, 50.0, 50.0, XMAX, thermo_steps(natom), flags)
    return cached(('dof_oracle', natom), make)


DOF_TARGET = 50.0


def dof_allowance(prm):
    """the final temperature of a fraction-1 rescale: within window + 1e-3 T of the target"""
    return prm.t_window + 1e-3 * DOF_TARGET


# nve/limit
LIMIT_XMAX_FREE, LIMIT_XMAX_FORCES = 10.0, 1.0


def limit_free_oracle(natom, xmax=LIMIT_XMAX_FREE):
    def make():
        lat, x, v, who, dirs = limit_free_case(natom)
        p = engine_params(lat.prm, t_window=1.0e30)
        return oracle_md(p, x, v, lat.atoms, lat.poly, None, None, 1.0, 1.0, 50.0, 50.0, xmax, 20)
    return cached(('limit_free_oracle', natom, xmax), make)


def limit_forces_oracle(natom, xmax=LIMIT_XMAX_FORCES):
    """the overlapping random model, thermostat on (window 0.1, target 50), 20 steps"""
    def make():
        atoms, poly, prm, ptr, sb, x, v, flags = thermo_inputs(natom)
        return oracle_md(prm, x, v, atoms, poly, ptr, sb, sm.EVF, sm.ENVF, 50.0, 50.0, xmax, 20)
    return cached(('limit_forces_oracle', natom, xmax), make)


def clamped_at_step_1(natom, xmax=LIMIT_XMAX_FORCES):
    """share of the mobile atoms whose first half-kick, v + dt / 2 f(x0), exceeds xmax / dt"""
    atoms, poly, prm, ptr, sb, x, v, flags = thermo_inputs(natom)
    f, _ = oracle.mstep_forces(prm, x, atoms.radii, flags, poly, ptr, sb, sm.EVF, sm.ENVF, nthreads=4)
    mobile = flags & M.IGM_ATOM_FIXED == 0
    f[:, ~mobile] = 0.0
    vh = v.astype(np.float64) + 0.5 * DT * f
    return float((np.linalg.norm(vh, axis=2)[:, mobile] > xmax / DT).mean())


# the cell walk after motion
WALK_SIZES = (1024, 1100)


def walk_inputs(natom):
    def make():
        atoms, poly, prm, ptr, sb, x = model(natom, 2, 'dense')
        v = np.stack([oracle.velocity_create(atoms.flags, 50.0, 41 + s) for s in range(len(x))]).astype(np.float32)
        return atoms, poly, prm, ptr, sb, x, v
    return cached(('walk_inputs', natom), make)


def walk_oracle(natom):
    def make():
        atoms, poly, prm, ptr, sb, x, v = walk_inputs(natom)
        return oracle_md(prm, x, v, atoms, poly, ptr, sb, sm.EVF, sm.ENVF, 50.0, 40.0, XMAX, 20)
    return cached(('walk_oracle', natom), make)


def list_cut(atoms, prm):
    """cut_list = 2 rmax + skin; skin = rmax when the params give none"""
    rmax = float(atoms.radii[atoms.flags & M.IGM_ATOM_BEAD != 0].max())
    skin = prm.skin if prm.skin > 0 else rmax
    return 2.0 * rmax + skin, skin


def most_neighbours(x_s, bead, cut):
    """the largest number of beads inside cut of one bead of a structure"""
    from scipy.spatial import cKDTree
    p = np.asarray(x_s, np.float64)[bead]
    return int(cKDTree(p).query_ball_point(p, cut, return_length=True).max()) - 1


# run()
RUN_SIZES = (257, 3073)
RUN_SEGMENTS = 2 * len(RUN_STEPS)


def run_seeds(nstruct):
    return M.lammps_seeds(6535, list(range(nstruct)), 3)


def run_oracle(natom, nstruct=3):
    """(info, x64) of oracle.mstep_run over the lattice structures"""
    def make():
        lat = run_case(natom, nstruct)
        _, info, x64 = oracle.mstep_run(lat.prm, lat.x(), lat.atoms.radii, lat.atoms.flags, lat.poly, None, None,
                                        run_seeds(nstruct), nthreads=4)
        return info, x64
    return cached(('run_oracle', natom, nstruct), make)


# the kinetic energy of the last block
LAST_BLOCK_NATOM, LAST_BLOCK_STEPS, LAST_BLOCK_WINDOW = 16385, 10, 1.0e-5


def last_block_case():
    """16 385 lattice beads, 65 blocks, the last of one slot.  The bead in that slot flies outwards
    (+z) at |v| = 4 and the bead in slot 0 (-z) at 2; everybody else rests: 80 % of the kinetic
    energy is the 65th partial.  Target T / 4, window 1e-5: the first rescale halves both
    velocities and the later ones find T on target.  Nobody passes skin / 2, so no build moves a
    slot.  Returns (lattice, x, v, hot atom, slow atom, t_target)."""
    def make():
        lat = Lattice(LAST_BLOCK_NATOM)
        x = lat.x()
        v = np.zeros_like(x)
        hot, slow = int(lat.atom_at[LAST_BLOCK_NATOM - 1]), int(lat.atom_at[0])
        v[0, hot, 2], v[0, slow, 2] = 4.0, -2.0
        t = float(temperature(v, lat.atoms.flags)[0])
        return lat, x, v, hot, slow, 0.25 * t
    return cached(('last_block',), make)


def last_block_oracle():
    def make():
        lat, x, v, hot, slow, tt = last_block_case()
        p = engine_params(lat.prm, t_window=LAST_BLOCK_WINDOW)
        return oracle_md(p, x, v, lat.atoms, lat.poly, None, None, 1.0, 1.0, tt, tt, XMAX, LAST_BLOCK_STEPS)
    return cached(('last_block_oracle',), make)


def last_block_without(skip):
    """the run in NumPy (no forces: drift and rescale) with the kinetic energy of the atoms
    `skip` left out of the thermostat's sum -- the outcome of a sum that misses their block"""
    lat, x, v, hot, slow, tt = last_block_case()
    x, v = x.astype(np.float64), v.astype(np.float64)
    seen = np.ones(lat.natom, bool)
    seen[list(skip)] = False
    for _ in range(LAST_BLOCK_STEPS):
        x = x + DT * v
        tcur = (v[0, seen] ** 2).sum() / (3.0 * lat.natom - 3.0)
        if tcur > 0 and abs(tcur - tt) > LAST_BLOCK_WINDOW:
            v = v * np.sqrt(tt / tcur)
    return x, v
