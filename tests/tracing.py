"""Test helper for the position anchors (chromatin tracing).

dummy_form()     the reference's own formulation of an anchor set, for the unchanged fp64
                 oracle: one IGM_ATOM_FIXED atom per anchor, appended after all existing
                 atoms, at the (float32) target, radius 0, plus a bond (fixed atom, locus,
                 r0, k).  The appended atoms draw their RanPark numbers after every existing
                 atom and are outside group nonfixed, so the beads' velocities, the rescale
                 and the CG are those of the native form.  Every structure of a batch gets
                 the same number of appended atoms; the spare ones carry no bond.
anchor_forces()  the anchor term in numpy, on top of small_models.brute_forces:
                 E = k (r - r0)^2 for r > r0, force on the atom only, 0 at r = 0; an
                 IGM_ATOM_FIXED atom contributes energy and takes no force.
anchor_sets()    the anchor sets of the force tests (structure 0: the ends, a random quarter
                 of the beads, a second anchor on atom 0, one target on the atom itself, one
                 10 nm away; structure 1: none; structure 2: every atom, the dummy included).
anchor_record()  the ModelingStep record of an anchor set in numpy (float32 norm, float64
                 ratio, np.histogram).
register_cpu_kernels()  optimization/kernel = 'tracing_test': the CPU oracle kernels with the
                 anchors of a Batch run in their dummy-atom form.
"""
import numpy as np

import oracle
import small_models as sm
from igm_amd import model as M
from igm_amd._lib import IGM_ATOM_FIXED, anchor_dtype, bond_dtype

R0, K = 50.0, 1.0


def make_anchors(per):
    """[(atom ids, targets (n, 3)[, r0, k])] per structure -> (ptr, igm_anchor array)"""
    ptr = np.zeros(len(per) + 1, np.int64)
    out = []
    for s, item in enumerate(per):
        atom, target = np.asarray(item[0], np.int64), np.asarray(item[1], np.float64).reshape(-1, 3)
        a = np.zeros(len(atom), anchor_dtype)
        a['atom'] = atom
        a['x'], a['y'], a['z'] = target[:, 0], target[:, 1], target[:, 2]
        a['r0'] = item[2] if len(item) > 2 else R0
        a['k'] = item[3] if len(item) > 3 else K
        out.append(a)
        ptr[s + 1] = ptr[s] + len(a)
    return ptr, (np.concatenate(out) if out else np.zeros(0, anchor_dtype))


def anchor_sets(x, natom, seed):
    """The anchor sets of the force tests for coordinates x (3, natom, 3) (small_models.case)."""
    assert x.shape[0] == 3 and x.shape[1] == natom
    rng = np.random.default_rng(seed)
    nbead = natom - 1
    quarter = np.sort(rng.choice(nbead, max(1, nbead // 4), replace=False))
    atoms0 = np.concatenate([[0, nbead - 1], quarter, [0]])
    t0 = x[0, atoms0].astype(np.float64) + rng.normal(0.0, 300.0, (len(atoms0), 3))
    on_atom = int(quarter[0])
    near = int(quarter[-1])
    atoms0 = np.concatenate([atoms0, [on_atom, near]])
    t0 = np.concatenate([t0, x[0, [on_atom]].astype(np.float64),
                         x[0, [near]].astype(np.float64) + np.array([[6.0, 0.0, 8.0]])])  # r = 0; r = 10 < r0
    atoms2 = np.arange(natom)
    t2 = x[2].astype(np.float64) + rng.normal(0.0, 300.0, (natom, 3))
    return make_anchors([(atoms0, t0), (np.zeros(0, np.int64), np.zeros((0, 3))), (atoms2, t2)])


def targets_of(anch):
    return np.stack([anch['x'], anch['y'], anch['z']], 1)  # float32


def anchor_forces(x, flags, anch, dtype=np.float64):
    """forces (N, 3), bond energy and per-atom term magnitudes of one structure's anchors"""
    T = dtype
    x = np.asarray(x).astype(T)
    f = np.zeros(x.shape, T)
    mag = np.zeros(len(x), T)
    if len(anch) == 0:
        return f, 0.0, mag
    a = anch['atom'].astype(np.int64)
    dv = x[a] - targets_of(anch).astype(T)
    r = np.sqrt(np.sum(dv * dv, axis=1, dtype=T))
    dr = r - anch['r0'].astype(T)
    k = anch['k'].astype(T)
    act = dr > 0
    e = float(np.sum(np.where(act, k * dr * dr, T(0)), dtype=T))
    g = np.where(act & (r > 0), T(-2) * k * dr / np.where(r > 0, r, T(1)), T(0))
    g = np.where((np.asarray(flags)[a] & IGM_ATOM_FIXED) != 0, T(0), g)
    for d in range(3):
        np.add.at(f[:, d], a, g * dv[:, d])
    np.add.at(mag, a, np.abs(g) * r)
    return f, e, mag


def brute_batch(atoms, poly, ptr, sb, x, envelopes, evf, envf, aptr, anch, dtype=np.float64, parts=False):
    """small_models.brute_batch plus the anchor term: forces (S, N, 3), energies (S, 2 + nenv)
    with the anchor energy in the bond column [, parts with 'mag' including the anchors]."""
    f, e, pp = sm.brute_batch(atoms, poly, ptr, sb, x, envelopes, evf, envf, dtype, parts=True)
    f, e = f.copy(), e.copy()
    for s in range(len(x)):
        fa, ea, mag = anchor_forces(x[s], sm.struct_flags(atoms, s), anch[aptr[s]:aptr[s + 1]], dtype)
        f[s] += fa.astype(np.float64)
        e[s, 1] += ea
        pp[s]['mag'] = pp[s]['mag'] + mag
        pp[s]['anchor'] = fa
    return (f, e, pp) if parts else (f, e)


def dummy_form(radii, flags, poly, ptr, sb, x, aptr, anch):
    """(radii, flags, poly, ptr, sb, x) with the anchors as fixed atoms + bonds; x float32"""
    S, N = x.shape[0], x.shape[1]
    cnt = np.diff(aptr)
    m = int(cnt.max()) if len(cnt) else 0
    radii2 = np.concatenate([np.asarray(radii, np.float32), np.zeros(m, np.float32)])
    flags = np.asarray(flags, np.uint32)
    fix = np.full(flags.shape[:-1] + (m,), IGM_ATOM_FIXED, np.uint32)
    flags2 = np.concatenate([flags, fix], axis=-1)
    x2 = np.zeros((S, N + m, 3), np.float32)
    x2[:, :N] = x
    per = []
    for s in range(S):
        a = anch[aptr[s]:aptr[s + 1]]
        x2[s, N:N + len(a)] = targets_of(a)
        b = np.zeros(len(a), bond_dtype)
        b['i'] = N + np.arange(len(a))
        b['j'] = a['atom']
        b['r0'], b['k'] = a['r0'], a['k']
        own = sb[ptr[s]:ptr[s + 1]] if sb is not None and ptr is not None else np.zeros(0, bond_dtype)
        per.append(np.concatenate([own, b]))
    ptr2, sb2 = M.concat_bonds(per)
    return radii2, flags2, poly, ptr2, sb2, x2


def anchor_ratios(x, anch):
    """violation ratios (forces.py:131-139) of one structure's anchors: float32 norm, float64 ratio"""
    d = (targets_of(anch) - np.asarray(x, np.float32)[anch['atom'].astype(np.int64)]).astype(np.float32)
    dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float64)
    r0, k = anch['r0'].astype(np.float64), anch['k'].astype(np.float64)
    score = np.where(dist <= r0, 0.0, k * (dist - r0))
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(r0 == 0.0, 0.0, score / (k * r0))


def anchor_record(x, aptr, anch, tol):
    """(S, 104) int64: counts[101], violated_restr, n_violations, n_imposed"""
    out = np.zeros((len(x), 104), np.int64)
    for s in range(len(x)):
        v = anchor_ratios(x[s], anch[aptr[s]:aptr[s + 1]])
        rec = oracle.violations(v, tol)
        out[s, :101] = rec['counts']
        out[s, 101], out[s, 102], out[s, 103] = rec['violated_restr'], rec['n_violations'], len(v)
    return out


# ---------------------------------------------------------------- the Step layer on the CPU
SEEN = []


def _run_dummy(b, seeds):
    """oracle.mstep_run of a Batch whose anchors are run in their dummy-atom form"""
    radii, flags, poly, ptr, sb, x = b.radii, b.flags, b.poly, b.ptr, b.bonds, b.x
    if b.anchors is not None:
        radii, flags, poly, ptr, sb, x = dummy_form(radii, flags, poly, ptr, sb, x, b.anchor_ptr, b.anchors)
    try:
        xo, info, _ = oracle.mstep_run(b.prm, x, radii, flags, poly, ptr, sb, seeds, nthreads=4)
    finally:
        oracle.set_volume(None)
    return xo[:, :b.natom], info


def _cpu_mstep(store, sids, cfg, device):
    import cpu_kernels as CK
    from igm_amd import assemble as A
    from igm_amd import steps as ST
    spec = ST.modeling_spec(cfg, sids)
    SEEN.append(('mstep', float(cfg['runtime']['tracing']['tol']), float(spec['tracing']['tol'])))
    b = A.build(ST.batch_coordinates(store, sids), sids, store, spec, None, select=CK.OracleSelect())
    seeds = M.lammps_seeds(ST.cget(cfg, 'optimization/optimizer_options/seed', 6535), sids,
                           ST.cget(cfg, 'runtime/step_no', 1))
    xo, info = _run_dummy(b, seeds)
    ncls = len(b.class_cr) + b.prm.nenvelopes
    stats = np.zeros((len(sids), ncls + 1, 104), np.int64)
    for q in range(len(sids)):
        c = b.bcls[b.ptr[q]:b.ptr[q + 1]]
        stats[q, :len(b.class_cr), 103] = np.bincount(c, minlength=len(b.class_cr))[:len(b.class_cr)]
        stats[q, M.CLASS_POLYMER, 103] += len(b.poly)
    stats[:, -1] = anchor_record(xo, b.anchor_ptr, b.anchors, float(ST.rget(cfg, 'optimization/violation_tolerance')))
    return {'xyz': xo[:, :b.nbead], 'info': info, 'stats': stats,
            'names': [b.vstat_names(q) for q in range(len(sids))], 'batch': b}


def _cpu_relax(store, sids, cfg, device):
    import cpu_kernels as CK
    from igm_amd import assemble as A
    from igm_amd import init
    from igm_amd import steps as ST
    rs = cfg['model']['restraints']
    spec = {'evfactor': float(rs['excluded']['evfactor']), 'protocol': cfg['optimization']['optimizer_options'],
            'polymer': {'contact_range': rs['polymer']['contact_range'], 'kspring': rs['polymer']['polymer_kspring']},
            'envelope': ST.envelope_section(cfg, sids),
            'tracing': {'data': ST.tracing_data(cfg), 'tol': init.RELAX_TRACING_TOL,
                        'k': cfg['restraints']['tracing']['kspring']}}
    SEEN.append(('relax', init.RELAX_TRACING_TOL))
    b = A.build(ST.batch_coordinates(store, sids), sids, store, spec, None, select=CK.OracleSelect())
    xo, info = _run_dummy(b, M.lammps_seeds(6535, sids, ST.cget(cfg, 'runtime/step_no', 1)))
    return xo[:, :b.nbead], info


def register_cpu_kernels():
    """a test calls this itself; nothing is registered on import"""
    import cpu_kernels  # noqa: F401  (registers 'cpu_oracle_test')
    from igm_amd import steps as ST
    ST.KERNELS['tracing_test'] = dict(ST.KERNELS['cpu_oracle_test'], mstep=_cpu_mstep, relax=_cpu_relax)
