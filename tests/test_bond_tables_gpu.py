"""The M-step bond tables at their type, degree and staging edges, through the C ABI.

prepare() (adj_degree_kernel / adj_slices_kernel / adj_fill_kernel in igm_amd/csrc/mstep.hip)
builds one device table per structure; every engine re-packs or stages it under limits of
its own.  The sets of tests/bond_tables.py sit on those limits:

    anneal_kernel, lds_bonds      bonds staged in LDS as u16 only if ntype <= 8 and
                                  (2 nb + 7) & ~7 <= rest_cap (per structure)     types8|9, mixed8_9_8, rest_cap
    bond_candidates/atom_force_md the pruning mask covers LDS entries 0..31        degrees8 (31 / 32 / 33 / 64), hub_bead
    pop_force_kernel              types staged in LDS if ntype <= 512              types512|513, mixed512_513_3
    pop_permute_slot, hbm_bonds   entries 4 at a time with clamps                  degrees8|9 (1, 3, 4, 5)
    adj_*, prepare()              4096 types pass, 4097 and 9000 are refused;
                                  an atom index out of range is refused            types4096, the refusals
    run_anneal_pop                a degree above 0xFFFF is refused                 the refusals

natom 257 runs on the population engine, 1100 on the LDS kernels <1024, 2> (and, forced, on
the population engine), 2100 on <1024, 3>.  References: the fp64 oracle and
bond_tables.brute (numpy fp64 over every pair), pinned to each other on the CPU by
tests/test_bond_tables.py, which also holds the f32 headroom of every input.  The bounds are
those of tests/test_mstep_sizes_gpu.py, through its own checking functions:
    f64 forces  max|d| <= 1e-6 max|F_ref| + 1e-6      energies  rtol 1e-9, atol 1e-9
    f32 forces  ||err|| <= 1e-5 ||F_ref|| over the batch
    md          max|dx| < 1e-3 max(1, moved), moved > 1
The batch norms could hide one bond, so the two atoms of each structure's highest-type
bond are held on their own, to the per-atom absolute form of the 'coincident' check:
|err_a| <= tol x (sum of the magnitudes of every term on atom a) (+ 1e-6 on the f64 path),
tol 1e-6 (f64) and 1e-5 (f32); that bond alone is >= 1 force unit of the sum.
"""
import numpy as np
import pytest

import bond_tables as bt
import oracle
import small_models as sm
from igm_amd import _lib
from igm_amd import model as M
from test_mstep_sizes_gpu import _brute_energy_cols, _check_f32, _check_f64, _engine, _short_protocol, _velocities

pytestmark = pytest.mark.gpu

EVF, ENVF = sm.EVF, sm.ENVF
ENGINES = ((257, 'default'), (1100, 'default'), (1100, 'global'), (2100, 'default'))


@pytest.fixture(scope='module')
def ms():
    from igm_amd import mstep
    return mstep


_REFS = {}


def _reference(name, natom):
    """(case, oracle (f, e), brute (f, e, parts)), computed once and left unchanged"""
    key = (name, natom)
    if key not in _REFS:
        c = bt.case(name, natom)
        radii, flags, shared, ptr, sb = c.args()
        orc = oracle.mstep_forces(c.prm, c.x, radii, flags, shared, ptr, sb, EVF, ENVF, nthreads=8)
        _REFS[key] = (c, orc, bt.brute(c, parts=True))
    return _REFS[key]


def _forces(ms, c, engine, f32=False):
    radii, flags, shared, ptr, sb = c.args()
    return ms.forces(_engine(c.prm, engine), c.x, radii, flags, shared, ptr, sb, EVF, ENVF, f32=f32)


def _check_top_bond(tag, c, fg, fref, parts, tol, atol):
    """the atoms of each structure's highest-type bond, one by one"""
    worst = 0.0
    for s, pair in enumerate(c.hi):
        for a in pair:
            if sm.struct_flags(c.atoms, s)[a] & M.IGM_ATOM_FIXED:
                assert np.all(fg[s, a] == 0.0)
                continue
            mag = parts[s]['mag'][a] + parts[s]['mag_pair'][a]
            err = np.linalg.norm(fg[s, a] - fref[s, a])
            worst = max(worst, err / (tol * mag + atol))
            assert err <= tol * mag + atol, (tag, s, a, err, mag)
    print('%s: top-type bond atoms, worst err / bound %.3g' % (tag, worst))


def _force_cases():
    return [(name, natom, engine) for name in bt.NAMES for natom, engine in ENGINES if natom in bt.sizes_of(name)]


# ------------------------------------------------------------------ forces
@pytest.mark.parametrize('name,natom,engine', _force_cases())
def test_gpu_forces_bond_tables(ms, name, natom, engine):
    """Every set on the default engine of its size and on the forced population engine: the
    f64 path (forces and energies against the oracle and against brute), the f32 path, the
    atoms of the highest-type bond on their own, and a rerun of both calls, bitwise (the
    entry sort fixes the summation order)."""
    c, (fo, eo), (fb, eb, parts) = _reference(name, natom)
    tag = '%s natom %d %s' % (name, natom, engine)
    fg, eg = _forces(ms, c, engine)
    if name.startswith('hub'):
        print('%s: adjacency %.3f ms' % (tag, _lib.context(0).kernel_ms('adjacency')))
    _check_f64(tag + ' vs oracle', fg, eg, fo, eo[:, :5])
    _check_f64(tag + ' vs brute', fg, eg, fb, _brute_energy_cols(eb))
    _check_top_bond(tag + ' f64', c, fg, fb, parts, 1e-6, 1e-6)
    f32, _ = _forces(ms, c, engine, f32=True)
    _check_f32(tag, f32, fo)
    _check_top_bond(tag + ' f32', c, f32, fb, parts, 1e-5, 0.0)
    fg2, eg2 = _forces(ms, c, engine)
    f32b, _ = _forces(ms, c, engine, f32=True)
    assert np.array_equal(fg, fg2) and np.array_equal(eg[:, :5], eg2[:, :5]) and np.array_equal(f32, f32b)


# ------------------------------------------------------------------ dynamics
@pytest.mark.parametrize('natom,engine', ENGINES)
@pytest.mark.parametrize('name', ['degrees8', 'degrees9', 'hub_dummy', 'hub_bead', 'mixed8_9_8', 'mixed512_513_3'])
def test_gpu_md_bond_tables(ms, name, natom, engine):
    """20 steps of igm_mstep_md (nve/limit + temp/rescale) from identical x, v against the
    fp64 oracle, and bitwise equal on a rerun."""
    c = bt.case(name, natom)
    radii, flags, shared, ptr, sb = c.args()
    v = _velocities(c.atoms, len(c.x))
    p = _engine(c.prm, engine)
    xg, vg = ms.md(p, c.x, v, radii, flags, shared, ptr, sb, EVF, ENVF, 50.0, 40.0, 1000.0, 20)
    xo, vo = oracle.mstep_md(c.prm, c.x.astype(np.float64), v.astype(np.float64), radii, flags, shared, ptr, sb, EVF,
                             ENVF, 50.0, 40.0, 1000.0, 20, nthreads=8)
    moved = np.abs(xo - c.x).max()
    print('%s natom %d %s: md 20 steps moved %.3g, max|dx| %.3g' % (name, natom, engine, moved, np.abs(xg - xo).max()))
    assert moved > 1.0
    assert np.all(np.isfinite(xg)) and np.all(np.isfinite(vg))
    assert np.abs(xg - xo).max(axis=(1, 2)).max() < 1e-3 * max(1.0, moved)
    xg2, vg2 = ms.md(p, c.x, v, radii, flags, shared, ptr, sb, EVF, ENVF, 50.0, 40.0, 1000.0, 20)
    assert np.array_equal(xg, xg2) and np.array_equal(vg, vg2)


# ------------------------------------------------------------------ pruning
MD_STEPS = 60 + 80 + 80 + 60 + 20


def _protocol_run(ms, c, engine):
    prm = M.params_from_cfg({'optimization': {'optimizer_options': _short_protocol()}}, sm.ENV_TWO)
    radii, flags, shared, ptr, sb = c.args()
    seeds = M.lammps_seeds(6535, list(range(len(c.x))), 3)
    return ms.run(_engine(prm, engine), c.x, radii, flags, shared, ptr, sb, seeds)


@pytest.mark.parametrize('natom', [1100, 2100])
@pytest.mark.parametrize('name', ['degrees8', 'hub_bead', 'mixed8_9_8'])
def test_gpu_lds_bond_pruning_is_bitwise_exact(ms, monkeypatch, name, natom):
    """The demo protocol at mdsteps (60, 80, 80, 60), relax 20, on the LDS engine with
    IGM_BOND_PRUNE=0 and by default: the same coordinates and info records, bit for bit.
    That pruning ran: the structures with <= 8 types are LDS-staged (every structure but
    the middle one of mixed8_9_8), for which the kernel recomputes every atom's candidate
    mask at each list build (the first step of the run always builds) and uses it in every
    step until the next one.  nrebuild counts the anneal's builds and the CG's, so it
    bounds the anneal's from above: it is below the run's 300 MD steps, so steps between
    builds ran on the masks -- which drop the idle bonds of the sets (the MID bonds of
    degrees8, asserted idle on the CPU; the slack polymer bonds everywhere) -- and at
    least 3, so masks were also recomputed from moved coordinates."""
    c = bt.case(name, natom)
    monkeypatch.setenv('IGM_BOND_PRUNE', '0')
    x0, i0 = _protocol_run(ms, c, 'default')
    monkeypatch.delenv('IGM_BOND_PRUNE')
    x1, i1 = _protocol_run(ms, c, 'default')
    print('%s natom %d: rebuilds %s' % (name, natom, i1['nrebuild'].tolist()))
    assert np.array_equal(x0, x1) and i0.tobytes() == i1.tobytes()
    assert np.all(np.isfinite(x1)) and np.all(i1['nrebuild'] >= 3) and np.all(i1['nrebuild'] < MD_STEPS)


@pytest.mark.parametrize('natom', [257, 1100])
@pytest.mark.parametrize('name', ['degrees8', 'hub_bead', 'mixed512_513_3'])
def test_gpu_pop_bond_pruning_is_bitwise_exact(ms, monkeypatch, name, natom):
    """The same protocol on the population engine (forced at 1100) with
    IGM_POP_BOND_PRUNE=0, by default (lists pruned at the first build and at builds whose
    lists served >= 6 steps), and with IGM_POP_PRUNE_AGE=0 (pruned at every build): the
    same bits.  That pruning ran: a structure's first build always prunes (its age starts
    large) and the force kernel reads the pruned candidates until a build that does not
    prune; with age 0 every build prunes.  nrebuild (the anneal's builds plus the CG's) is
    below the run's 300 MD steps, so steps ran between builds, all of them on pruned
    lists with age 0 and those after the first build by default."""
    c = bt.case(name, natom)
    monkeypatch.setenv('IGM_POP_BOND_PRUNE', '0')
    x0, i0 = _protocol_run(ms, c, 'global')
    monkeypatch.delenv('IGM_POP_BOND_PRUNE')
    x1, i1 = _protocol_run(ms, c, 'global')
    monkeypatch.setenv('IGM_POP_PRUNE_AGE', '0')
    x2, i2 = _protocol_run(ms, c, 'global')
    print('%s natom %d: rebuilds %s' % (name, natom, i1['nrebuild'].tolist()))
    assert np.array_equal(x0, x1) and i0.tobytes() == i1.tobytes()
    assert np.array_equal(x0, x2) and i0.tobytes() == i2.tobytes()
    assert np.all(np.isfinite(x1)) and np.all(i1['nrebuild'] >= 3) and np.all(i1['nrebuild'] < MD_STEPS)


# ------------------------------------------------------------------ refusals
def _good_again(ms, tag):
    """after a refusal the same context still computes: types8 at 257 against the oracle"""
    c, (fo, eo), _ = _reference('types8', 257)
    fg, eg = _forces(ms, c, 'default')
    _check_f64(tag + ': good input afterwards', fg, eg, fo, eo[:, :5])
    f32, _ = _forces(ms, c, 'default', f32=True)
    _check_f32(tag + ': good input afterwards', f32, fo)


@pytest.mark.parametrize('natom', [257, 1100])
@pytest.mark.parametrize('counts', [(4097, 4097, 4097), (9000, 9000, 9000), (8, 8, 4097), (8, 8, 9000)],
                         ids=lambda c: '-'.join(map(str, c)))
def test_gpu_too_many_bond_types_are_refused(ms, counts, natom):
    """4097 distinct (r0, k) in a structure, 9000 (more keys than the 8192 slots of the
    type hash: the insertion ends after one pass over the slots and the count still
    says too many), and batches where only the last structure is over the limit."""
    c = bt.types_counts(natom, counts)
    assert [len(np.unique(bt.keys(c.bonds(s)))) for s in range(3)] == list(counts)
    with pytest.raises(RuntimeError, match=r'code %d\).*more than 4096 distinct' % _lib.IGM_E_UNSUPPORTED):
        _forces(ms, c, 'default')
    _good_again(ms, 'types %s' % (counts,))


BAD_INDEX = {'i': lambda b, n: b.__setitem__('i', n), 'j': lambda b, n: b.__setitem__('j', n),
             'j-lower': lambda b, n: b.__setitem__('j', np.uint32(n) | _lib.LOWER_BOUND_BIT),
             'j-0x7fffffff': lambda b, n: b.__setitem__('j', 0x7fffffff)}


@pytest.mark.parametrize('where', ['shared', 'last-row'])
@pytest.mark.parametrize('what', sorted(BAD_INDEX))
def test_gpu_bond_index_out_of_range_is_refused(ms, what, where):
    """index natom (the first one past the atoms) as i, as j, as j with the lower-bound
    bit, and j = 0x7fffffff, in the shared array and in the last structure's own row"""
    c = bt.case('types8', 257)
    bad = bt.mk([0], [1], 500.0, 1.0)
    BAD_INDEX[what](bad, 257)
    radii, flags, shared, ptr, sb = c.args()
    if where == 'shared':
        shared = np.concatenate([shared, bad])
    else:
        ptr, sb = ptr.copy(), np.concatenate([sb, bad])
        ptr[-1] += 1
    for f32 in (False, True):
        with pytest.raises(RuntimeError, match=r'code %d\).*index out of range' % _lib.IGM_E_INVALID):
            ms.forces(c.prm, c.x, radii, flags, shared, ptr, sb, EVF, ENVF, f32=f32)
    _good_again(ms, 'index %s in %s' % (what, where))


def test_gpu_degree_65536_is_refused_by_the_population_engine(ms):
    """65 536 copies of one bond (and nothing else): the population engine stores degrees
    as u16 and says so"""
    c = bt.case('types8', 1100)
    radii, flags, _, _, _ = c.args()
    shared = np.repeat(bt.mk([3], [700], 500.0, 1.0), 65536)
    with pytest.raises(RuntimeError, match=r'code %d\).*an atom has 65536 bonds' % _lib.IGM_E_UNSUPPORTED):
        ms.forces(_engine(c.prm, 'global'), c.x, radii, flags, shared, None, None, EVF, ENVF, f32=True)
    _good_again(ms, 'degree 65536')
