"""CPU proofs that every input of tests/pop_step.py is the edge it claims (no GPU): the sizes at
which the population engine's step takes another path, the slot order the bullets rely on, and for
every case with a wrong outcome to guard against -- free flight, an unclamped run, a wrong dof --
that the oracle's result lies at least 100 comparison tolerances away from it."""
import os
import re

import numpy as np
import pytest

import oracle
import pop_step as ps
import small_models as sm
from igm_amd import model as M

MSTEP_HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'igm_amd', 'csrc', 'mstep.hip')


# ------------------------------------------------------------------ the constants and the edges derived from them
def test_restated_constants_are_those_of_the_source():
    src = open(MSTEP_HIP).read()

    def const(pattern):
        m = re.search(pattern, src)
        assert m, pattern
        return m.group(1)
    assert int(const(r'constexpr int kPopBS = (\d+);')) == ps.POP_BS
    assert int(const(r'constexpr int kPopSortNT = (\d+);')) == ps.SORT_NT
    assert int(const(r'#define IGM_POP_CELL_CAP (\d+)')) == ps.CELL_CAP
    assert int(const(r'constexpr int kCellCapBig = (\d+);')) == ps.CELL_CAP_BIG
    assert int(const(r'#define IGM_POP_LIST_CAP (\d+)')) == ps.LIST_CAP
    assert const(r'constexpr size_t kLdsBytes = ([^;]+);') == '160 * 1024 - 1024' and ps.LDS_BYTES == 162816
    # the strides of the two sums over a structure's blocks, and the sort's choice by size
    assert 'for (int i = threadIdx.x; i < A.nbs; i += %d) ke += kp[i];' % ps.PARTIAL_STRIDE in src
    assert 'for (int b = lane; b < A.nbs; b += %d) m = fmaxf(m, bp[b * 6 + w]);' % ps.PARTIAL_STRIDE in src
    assert 'N <= 16 * kPopSortNT ? pop_sort_kernel<true, 16>' in src
    assert 'N <= 32 * kPopSortNT ? pop_sort_kernel<true, 32> : pop_sort_kernel<true, 0>' in src
    assert 'sizeof(uint32_t) * ((ccap + 3) / 2) + (ids_lds ? sizeof(uint16_t) * (size_t)natom : 0)' in src


def test_sort_instantiations_switch_where_the_cases_stand():
    assert ps.sort_variant(16384) == (True, 16) and ps.sort_variant(16385) == (True, 32)
    assert ps.sort_variant(32768) == (True, 32) and ps.sort_variant(32769) == (True, 0)
    assert ps.sort_variant(48638) == (True, 0) and ps.sort_variant(48639) == (False, 0)
    # the last pair from the constants: 4 x 16 385 words of counts + 2 N bytes of ids
    assert ps.sort_lds(True, 0, ps.CELL_CAP) == 65540
    assert ps.sort_lds(True, 48638, ps.CELL_CAP) == 162816 == ps.LDS_BYTES
    assert ps.sort_lds(True, 48639, ps.CELL_CAP) == 162818 > ps.LDS_BYTES
    assert (ps.LDS_BYTES - 65540) // 2 == 48638
    # past the edge no smaller grid keeps the ids in LDS (the room is below kCellCapBig): HBM ids, full grid
    assert (ps.LDS_BYTES - 2 * 48639) // 2 - 4 == 32765 < ps.CELL_CAP_BIG and ps.sort_cells(48639) == ps.CELL_CAP
    for n in (1, 257, 48638, 65535):
        assert ps.sort_cells(n) == ps.CELL_CAP
    # no size in between switches again
    kinds = [ps.sort_variant(n) for n in range(1, 65536)]
    assert sum(a != b for a, b in zip(kinds, kinds[1:])) == 3


def test_block_counts_of_the_sizes():
    assert [ps.nbs(n) for n in (257, 1024, 1100, 3073, 16384, 16385)] == [2, 4, 5, 13, 64, 65]
    assert 257 - 256 == 1 and 16385 - 64 * 256 == 1  # the last block holds one slot
    assert ps.nbs(16385) > ps.PARTIAL_STRIDE >= ps.nbs(16384)
    assert all(ps.engine_of(n) == 'default' for n in (257, 1024, 3073, 48639)) and ps.engine_of(1100) == 'global'


# ------------------------------------------------------------------ slot order
@pytest.mark.parametrize('natom', [257, 1024, 1100, 3073, 16384, 16385])
def test_slot_order_of_the_lattice_is_site_order(natom):
    """One site per cell (the cells are narrower than the spacing), so after the setup build the
    slot of an atom is its site, whatever its id."""
    lat = ps.Lattice(natom)
    slot, nb = ps.slots_of(lat.x()[0], lat.cut, ps.sort_cells(natom))
    ext = lat.site.max(axis=0) - lat.site.min(axis=0)
    print('natom %d: grid %s, cell sides %s' % (natom, nb.tolist(), (ext / nb).round(1).tolist()))
    assert np.all(ext / nb < lat.spacing) and np.all(ext / nb >= lat.cut) and nb.prod() <= ps.CELL_CAP
    assert np.array_equal(slot[lat.atom_at], np.arange(natom))
    assert not np.array_equal(lat.atom_at, np.arange(natom))  # id and slot are not correlated
    assert abs(np.corrcoef(lat.atom_at, np.arange(natom))[0, 1]) < 0.1


@pytest.mark.parametrize('natom', [32768, 32769, 48638, 48639])
def test_slot_order_where_sites_share_a_cell(natom):
    """32 and 33 sites a side: the capped cell side is the spacing, and the clamp puts the last
    two sites of a row into one cell.  37 a side: more atoms than cells.  Atoms of one cell are
    ordered by id, so the 'last' bullet's site is found with its id (bullet_site)."""
    lat = ps.Lattice(natom)
    slot, nb = ps.slots_of(lat.x()[0], lat.cut, ps.sort_cells(natom))
    assert nb.prod() <= ps.CELL_CAP and nb.max() < lat.n
    assert slot[lat.atom_at[0]] < 8 and sorted(slot.tolist()) == list(range(natom))
    assert not np.array_equal(slot[lat.atom_at], np.arange(natom))


# ------------------------------------------------------------------ bullets
def test_bullet_cases_cover_sites_ids_and_axes():
    cases = ps.bullet_cases()
    assert len(cases) == 4 * 9 + 6 * 3
    for natom in (257, 1100, 3073):
        mine = [c for c in cases if c[0] == natom]
        assert {(c[1], c[3]) for c in mine} == {(w, i) for w in ('low', 'mid', 'last') for i in ps.IDS}
        assert {c[2] for c in mine if c[1] == 'mid'} == {0, 1, 2}
    for natom in (16384, 16385, 32768, 32769, 48638, 48639):
        mine = [c for c in cases if c[0] == natom]
        assert [c[1] for c in mine] == ['low', 'mid', 'last'] and {c[3] for c in mine} == set(ps.IDS)
        assert {c[2] for c in mine} == ({0, 1} if natom == 32769 else {0, 1, 2})  # (32 769: flight_axis)


@pytest.mark.parametrize('natom,where,axis,which,nsteps,start', ps.bullet_cases())
def test_bullet_is_stopped_only_by_a_rebuild(natom, where, axis, which, nsteps, start):
    case = ps.bullet_case(natom, where, axis, which, nsteps, start)
    (s, a, ta, ax, d, st), = case.bullets
    assert a == ps.atom_id(natom, which) and ax == axis
    # the setup: the target outside the bullet's list, every other bead further still
    r = np.linalg.norm(case.x[0].astype(np.float64) - case.x[0, a].astype(np.float64), axis=1)
    r[a] = np.inf
    assert np.argmin(r) == ta and abs(r[ta] - start) < 1e-3 and r[ta] > case.lat.cut
    assert np.sort(r)[1] >= ps.SPACING - 1e-3
    # where it sits: slot 0, the last slot, or a late lane of a middle block
    slot, _ = ps.slots_of(case.x[0], case.lat.cut, ps.sort_cells(natom))
    if where == 'low':
        assert slot[a] == 0
    elif where == 'last':
        assert slot[a] == natom - 1 and slot[a] // ps.POP_BS == ps.nbs(natom) - 1
    else:
        assert 0 < slot[a] // ps.POP_BS < ps.nbs(natom) - 1 or natom == 257
    xo, vo = ps.bullet_power(case)
    (b0, b1), = ps.block_change(case, xo)
    print('slot %d, block %d -> %d' % (slot[a], b0, b1))
    assert b0 == slot[a] // ps.POP_BS
    if ps.must_change_block(natom, where, axis):
        assert b0 != b1
    # nothing but the chain the bullet set off has moved
    still = np.abs(xo[0] - case.x[0]).max(axis=1) == 0
    assert natom - 4 <= still.sum() <= natom - 2


def test_every_size_from_1024_has_a_flight_that_changes_block():
    for natom in sorted({c[0] for c in ps.bullet_cases()}):
        mine = [c for c in ps.bullet_cases() if c[0] == natom and ps.must_change_block(c[0], c[1], c[2])]
        assert mine, natom
        if natom >= 1024:
            assert any(c[1] == 'mid' for c in mine)


@pytest.mark.parametrize('natom', [257, 1100])
def test_isolation_case(natom):
    """Structures 1 and 3 carry a bullet each, in different blocks; 0, 2 and 4 rest, and the
    oracle leaves them bitwise unchanged."""
    case = ps.isolation_case(natom)
    assert [b[0] for b in case.bullets] == [1, 3]
    xo, vo = ps.bullet_power(case)
    blocks = []
    for (s, a, ta, axis, d, start) in case.bullets:
        slot, _ = ps.slots_of(case.x[s], case.lat.cut, ps.sort_cells(natom))
        blocks.append(int(slot[a]) // ps.POP_BS)
    assert blocks == [0, ps.nbs(natom) - 1]
    for s in (0, 2, 4):
        assert np.array_equal(xo[s], case.x[s].astype(np.float64)) and not vo[s].any()
        assert np.array_equal(case.x[s], case.x[0]) and not case.v[s].any()
    one = ps.isolation_case(natom, 1)
    assert one.x.shape[0] == 1 and one.bullets[0][1:] == case.bullets[0][1:]
    ps.bullet_power(one)


@pytest.mark.parametrize('natom', [257, 1100, 3073])
def test_two_bullets_collide_three_steps_apart(natom):
    case = ps.two_bullet_case(natom)
    xo, vo = ps.bullet_power(case)
    slot, _ = ps.slots_of(case.x[0], case.lat.cut, ps.sort_cells(natom))
    assert [int(slot[b[1]]) // ps.POP_BS for b in case.bullets] == [0, ps.nbs(natom) - 1]
    # the step at which each target first feels its bullet
    first = []
    for (s, a, ta, axis, d, start) in case.bullets:
        for k in range(1, case.nsteps + 1):
            _, vk = ps.oracle_md(case.prm, case.x, case.v, case.lat.atoms, case.lat.poly, None, None, 1.0, 1.0, 50.0,
                                 50.0, ps.XMAX, k)
            if vk[s, ta].any():
                first.append(k)
                break
    print('natom %d: first contact at steps %s' % (natom, first))
    assert len(first) == 2 and first[1] - first[0] == 3
    # each contact needs a build of its own: the second target is not in any list of the first's builds
    assert first[0] >= 2 and case.bullets[1][5] - ps.SPEED * ps.DT * first[0] > case.lat.cut


# ------------------------------------------------------------------ thermostat
@pytest.mark.parametrize('natom', ps.THERMO_SIZES)
def test_thermostat_window_branch_matters(natom):
    """A window of 1e7 is never left (bitwise the unbounded run); the default 0.1 is, and the run
    differs by far more than the comparison allows."""
    x = ps.thermo_inputs(natom)[5]
    xw, vw = ps.thermo_oracle(natom, False, 1.0e7, 1.0, 50.0, 50.0)
    xu, vu = ps.thermo_oracle(natom, False, 1.0e30, 1.0, 50.0, 50.0)
    xd, vd = ps.thermo_oracle(natom, False, 0.1, 1.0, 50.0, 50.0)
    assert np.array_equal(xw, xu) and np.array_equal(vw, vu)
    ax, av = ps.apart(x, xd, vd, xu, vu)
    print('natom %d: default window against none: %.3g x tol, %.3g v tol' % (natom, ax, av))
    assert av >= 100.0 and np.abs(vd - vu).max() > 0.2 * np.abs(vu).max()


@pytest.mark.parametrize('natom', ps.THERMO_SIZES)
def test_thermostat_cases_differ_from_each_other(natom):
    """fraction 0.5 against 1, the ramp against the constant target, FIXED beads against none:
    each at least 100 velocity tolerances from the case it could be mistaken for"""
    x = ps.thermo_inputs(natom)[5]
    full = ps.thermo_oracle(natom, False, 0.1, 1.0, 50.0, 50.0)
    half = ps.thermo_oracle(natom, False, 0.1, 0.5, 50.0, 50.0)
    ramp = ps.thermo_oracle(natom, False, 0.1, 1.0, 50.0, 40.0)
    rampf = ps.thermo_oracle(natom, True, 0.1, 1.0, 50.0, 40.0)
    assert ps.apart(x, full[0], full[1], half[0], half[1])[1] >= 100.0
    assert ps.apart(x, full[0], full[1], ramp[0], ramp[1])[1] >= 50.0  # sqrt(40 / 50): 10 % of |v|
    fl, flf = ps.thermo_inputs(natom)[7], ps.thermo_inputs(natom, True)[7]
    assert np.all(np.abs(ps.temperature(ramp[1], fl) - 40.0) <= 0.1)
    assert np.all(np.abs(ps.temperature(rampf[1], flf) - 40.0) <= 0.1)
    # a dof that counted the held beads would leave the final T off by the ratio of the counts
    nm, nmf = int((fl & M.IGM_ATOM_FIXED == 0).sum()), int((flf & M.IGM_ATOM_FIXED == 0).sum())
    assert nmf < nm and abs(40.0 * (3.0 * nm - 3.0) / (3.0 * nmf - 3.0) - 40.0) > 100.0 * (0.1 + 1e-3 * 40.0)


@pytest.mark.parametrize('natom', ps.THERMO_SIZES)
def test_oracle_honours_per_structure_dof(natom):
    """oracle.mstep_md on the batch with (S, N) flags equals its runs of each structure alone;
    every structure ends at the target; structure 0's dof applied to structure 2 would miss it
    by more than 100 allowances."""
    atoms, poly, prm, ptr, sb, x, v, flags = ps.dof_inputs(natom)
    mobile = (flags & M.IGM_ATOM_FIXED == 0).sum(axis=1)
    assert mobile[0] == natom - 1 and mobile[0] > mobile[1] > mobile[2]
    assert not v[flags & M.IGM_ATOM_FIXED != 0].any()
    xo, vo = ps.dof_oracle(natom)
    for s in range(3):
        b = sm.struct_bonds(poly, ptr, sb, s)
        x1, v1 = oracle.mstep_md(prm, x[s:s + 1].astype(np.float64), v[s:s + 1].astype(np.float64), atoms.radii,
                                 flags[s], b, None, None, sm.EVF, sm.ENVF, 50.0, 50.0, ps.XMAX, ps.thermo_steps(natom))
        assert np.array_equal(x1[0], xo[s]) and np.array_equal(v1[0], vo[s])
    T = ps.temperature(vo, flags)
    allow = ps.dof_allowance(prm)
    print('natom %d: mobile %s, final T %s, allowance %.3g' % (natom, mobile.tolist(), T.tolist(), allow))
    assert np.all(np.abs(T - ps.DOF_TARGET) <= allow)
    dof = 3.0 * mobile - 3.0
    wrong = ps.DOF_TARGET * dof[0] / dof[2]  # sum v^2 rescaled to target x dof[0], read with dof[2]
    assert abs(wrong - ps.DOF_TARGET) > 100.0 * allow
    # the held beads have not moved
    held = flags & M.IGM_ATOM_FIXED != 0
    assert np.array_equal(xo[held], x.astype(np.float64)[held]) and not vo[held].any()


def test_last_block_case_puts_the_kinetic_energy_in_the_65th_partial():
    lat, x, v, hot, slow, tt = ps.last_block_case()
    xo, vo = ps.last_block_oracle()
    assert ps.nbs(lat.natom) == ps.PARTIAL_STRIDE + 1
    for pos in (x[0], xo[0]):  # no build in between: nobody passes skin / 2
        slot, _ = ps.slots_of(pos, lat.cut, ps.sort_cells(lat.natom))
        assert slot[hot] == lat.natom - 1 and slot[hot] // ps.POP_BS == ps.PARTIAL_STRIDE and slot[slow] == 0
    assert np.abs(xo - x).max() < lat.skin / 2
    assert (v[0, hot] ** 2).sum() == 0.8 * (v ** 2).sum()
    # the NumPy run with every partial is the oracle's; without the 65th it is far away
    xa, va = ps.last_block_without(())
    assert np.allclose(xa, xo, rtol=0, atol=1e-9) and np.allclose(va, vo, rtol=1e-12, atol=0)
    assert np.allclose(vo[0, hot], [0, 0, 2.0]) and np.allclose(vo[0, slow], [0, 0, -1.0])
    xw, vw = ps.last_block_without((hot,))
    ax, av = ps.apart(x, xo, vo, xw, vw)
    print('without the last block: %.3g x tol, %.3g v tol away; v %s' % (ax, av, vw[0, hot]))
    assert ax >= 100.0 and av >= 100.0


# ------------------------------------------------------------------ nve/limit
@pytest.mark.parametrize('natom', ps.LIMIT_POP + ps.LIMIT_LDS)
def test_limit_without_forces_moves_ten_a_step(natom):
    lat, x, v, who, dirs = ps.limit_free_case(natom)
    assert len(set(who)) == 3 and np.allclose(np.linalg.norm(v[0, who], axis=1), ps.SPEED, rtol=1e-6)
    xo, vo = ps.limit_free_oracle(natom)
    for a, u in zip(who, dirs):
        assert np.allclose(xo[0, a] - x[0, a], 20 * ps.LIMIT_XMAX_FREE * u, rtol=0, atol=1e-4)  # v is float32
        assert np.allclose(vo[0, a], ps.LIMIT_XMAX_FREE / ps.DT * u, rtol=0, atol=1e-4)
    rest = np.delete(np.arange(natom), who)
    assert np.array_equal(xo[0, rest], x[0, rest].astype(np.float64)) and not vo[0, rest].any()
    # nobody meets anybody: the closest approach of the run's end is the spacing or more
    from scipy.spatial import cKDTree
    assert cKDTree(xo[0]).query(xo[0], 2)[0][:, 1].min() >= ps.SPACING - 1e-3
    xu, vu = ps.limit_free_oracle(natom, ps.XMAX)
    ax, av = ps.apart(x, xo, vo, xu, vu)
    print('natom %d: unclamped run %.3g x tol, %.3g v tol away' % (natom, ax, av))
    assert ax > 100.0 and av > 100.0
    assert 20 * ps.LIMIT_XMAX_FREE > ps.SKIN / 2  # the three beads cause list builds on the way


@pytest.mark.parametrize('natom', ps.LIMIT_POP + ps.LIMIT_LDS)
def test_limit_with_forces_clamps_most_atoms(natom):
    share = ps.clamped_at_step_1(natom)
    x = ps.thermo_inputs(natom)[5]
    xo, vo = ps.limit_forces_oracle(natom)
    xu, vu = ps.limit_forces_oracle(natom, ps.XMAX)
    ax, av = ps.apart(x, xo, vo, xu, vu)
    print('natom %d: %.0f %% clamped at step 1; unclamped run %.3g x tol, %.3g v tol away' % (natom, 100 * share, ax,
                                                                                         av))
    assert share >= 0.5 and ax >= 100.0 and av >= 100.0
    # no step moves an atom further than xmax
    assert np.linalg.norm(xo - x, axis=2).max() <= 20 * ps.LIMIT_XMAX_FORCES * (1 + 1e-9)


# ------------------------------------------------------------------ the cell walk after motion
@pytest.mark.parametrize('natom', ps.WALK_SIZES)
def test_walk_case_overflows_the_list_at_both_ends(natom):
    atoms, poly, prm, ptr, sb, x, v = ps.walk_inputs(natom)
    xo, vo = ps.walk_oracle(natom)
    cut, skin = ps.list_cut(atoms, prm)
    bead = atoms.flags & M.IGM_ATOM_BEAD != 0
    moved = np.abs(xo - x).max(axis=(1, 2))
    for s in range(len(x)):
        n0, n1 = ps.most_neighbours(x[s], bead, cut), ps.most_neighbours(xo[s], bead, cut)
        print('natom %d structure %d: most neighbours inside %.0f: %d at the start, %d at the end; moved %.0f' % (
            natom, s, cut, n0, n1, moved[s]))
        assert n0 > ps.LIST_CAP and n1 > ps.LIST_CAP
    assert np.all(moved > skin / 2)


# ------------------------------------------------------------------ run()
@pytest.mark.parametrize('natom', ps.RUN_SIZES)
def test_run_case_never_interacts_and_rebuilds_often(natom):
    lat = ps.run_case(natom)
    prm = lat.prm
    assert [prm.mdsteps[k] for k in range(4)] == [5, 6, 7, 4] and prm.relax_steps == 3 and prm.nstages == 4
    assert prm.max_velocity == ps.RUN_XMAX and prm.relax_max_velocity == 10.0
    total = sum(ps.RUN_STEPS) + 4 * ps.RUN_RELAX
    # nve/limit bounds every step, so no pair ever comes inside 2 r + skin
    assert ps.run_path_bound() == 22 * 15.0 + 12 * 10.0
    assert lat.spacing - 2 * ps.run_path_bound() > lat.cut == 2 * ps.RADIUS + ps.RUN_SKIN
    info, x64 = ps.run_oracle(natom)
    disp = np.linalg.norm(x64 - lat.x(), axis=2)
    print('natom %d: rebuilds %s, largest displacement %.1f of at most %.1f' % (natom, info['nrebuild'].tolist(),
                                                                                 disp.max(), ps.run_path_bound()))
    assert disp.max() <= ps.run_path_bound() and disp.max() > 3 * lat.skin / 2  # past skin / 2 several times
    from scipy.spatial import cKDTree
    for s in range(lat.nstruct):
        assert cKDTree(x64[s]).query(x64[s], 2)[0][:, 1].min() > lat.cut
    assert np.all(info['nrebuild'] >= 3) and np.all(info['nrebuild'] <= total // 2)
    assert np.all(info['final_energy'] == 0.0)
    # the GPU's count may differ by one per segment.  An engine that never rebuilt would count the
    # setup's build and the minimiser's, 2 at most; one that always did, every step: both outside
    assert ps.RUN_SEGMENTS == 8
    assert info['nrebuild'].min() - ps.RUN_SEGMENTS > 2 and info['nrebuild'].max() + ps.RUN_SEGMENTS < total
