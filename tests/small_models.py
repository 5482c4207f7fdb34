"""Small synthetic M-step models of any size and an independent force reference.

make()          a model of `nbead` beads + 1 static dummy (natom = nbead + 1), built only
                from igm_amd.model and numpy: radii from {100, 150, 200}, four chromosomes,
                polymer bonds shared by the structures, `nbonds` random bonds per structure
                (r0 in [100, 900], k in [0.5, 2]: far more than 8 distinct types; every
                third one lower-bound), coordinates normal(0, sigma = 700), and the
                degenerate geometries listed in GEOMETRIES.
brute_forces()  O(N^2) numpy evaluation of the force field, written from the formulas in
                the header of igm_amd/csrc/mstep_common.h (no cell lists, no oracle code):
                  pair soft   E = A [1 + cos(pi r / rc)], rc = r_i + r_j, A = evf (rc/pi)^2, r < rc
                  bond        E = K (r - r0)^2 beyond the bound (upper: r > r0, lower: r < r0)
                  envelope    E = |k|/2 t^2, t = (1 - k2^-1/2) |x|, k2 = sum x_d^2 / s_d^2,
                              s_d = envf abc_d - r_i; k > 0 acts where k2 > 1, k < 0 where 0 < k2 < 1
                fp64 by default; dtype=np.float32 evaluates every term and every sum in
                float32, which is how f32_headroom() sizes the f32 tolerance on the CPU.

CPU-side f32 headroom.  The GPU tests bound the f32 force path by
||err|| <= 1e-5 ||F_ref|| over the batch.  The bound is relative to the net force, so an
input is only fair if an honest float32 evaluation stays well under it:
headroom = 1e-5 ||F64|| / ||F32 - F64||, both sides from brute_forces (case(): S = 3,
seed = natom, evf 0.5, envf 1.2, the envelopes of f32_envelopes()).  Measured with numpy
float32; tests/test_small_models.py asserts >= 10 for every input the GPU tests use:

    random, natom   3: 134    64: 141    65: 127   257: 125  1024: 111  1025: 109
                 1100: 111  2048: 108  2049: 111  3072: 109  3073: 111
    natom 257:   line 169   plane 73   one_cell 64   outlier 217 (125 over the atoms not
                 bonded to the outlier)   origin 125   plane_outlier 254 (73)   dense 25
    natom 1100:  line 90    plane 40   one_cell 139  outlier 246 (111)   origin 111
                 plane_outlier 266 (40)   dense 40
    'line' with both envelopes: 2 -- hence f32_envelopes().
    'coincident' has no net pair force (every pair term is exactly 0), so the relative form
    does not apply: the tests use the absolute form, per atom, err_i <= 1e-5 x (sum of the
    magnitudes of the bond and envelope terms on atom i); float32 numpy stays 25x (257) and
    13x (1100) under it.  'one_cell' is held to the relative form (above) and to the
    absolute form over all of an atom's terms, pair terms included (28x and 62x).
"""
import numpy as np

from igm_amd import model as M
from igm_amd.synthetic import DEMO_PROTOCOL

GEOMETRIES = ('random', 'coincident', 'line', 'plane', 'one_cell', 'outlier', 'origin', 'plane_outlier', 'dense')
ENV_ONE = [((2000.0, 1800.0, 1500.0), 1.0)]
ENV_TWO = ENV_ONE + [((1900.0, 1700.0, 1400.0), -1.0)]
RADII = (100.0, 150.0, 200.0)


EVF, ENVF = 0.5, 1.2  # the force tests' excluded-volume and envelope factors
SIZES = (3, 64, 65, 257, 1024, 1025, 2048, 2049, 3072, 3073)  # natom: both sides of every engine boundary
GEOM_SIZES = (257, 1100)  # population engine; LDS kernels <1024, 2>


def case(natom, geometry='random', envelopes=None, nstruct=3):
    """The force-test input of natom atoms (beads + 1 dummy): 3 structures, the middle one
    with an empty per-structure bond row, seed = natom; two envelopes unless given."""
    return make(natom - 1, nstruct, natom, geometry, envelopes=envelopes or ENV_TWO, empty_rows=(1,))


def f32_envelopes(geometry):
    """Envelopes of the f32 force checks.  On a coordinate axis the two terms of the
    envelope gradient, (1 - k2^-1/2) x/|x| and |x| k2^-3/2 x/s^2, cancel in their
    k2^-1/2 parts, and the k < 0 envelope acts near the centre where k2^-1/2 is large:
    float32 numpy keeps only 2x under the 1e-5 bound on 'line' with ENV_TWO.  The f32
    checks of 'line' therefore use the k > 0 envelope alone; the f64 checks use both."""
    return ENV_ONE if geometry == 'line' else ENV_TWO


def outlier_index(nbead):
    return nbead // 2


def coordinates(nbead, nstruct, rng, geometry='random', sigma=700.0):
    """(S, nbead + 1, 3) float32; the dummy (last atom) stays at the origin."""
    x = np.zeros((nstruct, nbead + 1, 3), np.float32)
    p = rng.normal(0.0, sigma, (nstruct, nbead, 3))
    if geometry == 'coincident':  # all beads of a structure at one point that is not the origin
        p[:] = rng.normal(0.0, sigma, (nstruct, 1, 3)) + 50.0
    elif geometry == 'line':
        p[:, :, 1:] = 0.0
    elif geometry == 'plane':
        p[:, :, 2] = 0.0
    elif geometry == 'one_cell':  # everything within 0.1 x the smallest radius
        centre = rng.normal(0.0, sigma, (nstruct, 1, 3)) + 50.0
        p = centre + rng.uniform(-0.05, 0.05, (nstruct, nbead, 3)) * min(RADII)
    elif geometry == 'outlier':
        p[:, outlier_index(nbead)] = (1.0e6, 0.0, 0.0)
    elif geometry == 'origin':
        p[:, 0] = 0.0
    elif geometry == 'plane_outlier':
        # a flat structure with a stray bead: the thin axis keeps one cell whatever the cell
        # side, so a cell side sized from the box volume alone leaves more cells than the
        # grids hold (4e6 x 4000 x 0 nm: past the 32 768 cells of the population engine too)
        p[:, :, 2] = 0.0
        p[:, outlier_index(nbead)] = (4.0e6, 0.0, 0.0)
    elif geometry == 'dense':
        # normal(0, 200): ~60 % of the beads lie inside every bead's list cut and a quarter
        # overlap it, at every r up to the cutoff -- lists of ~150 entries at 257 atoms (stored
        # a block of quads at a time), past the 256-entry capacity at 1100 (the cell walk)
        p *= 200.0 / sigma
    elif geometry != 'random':
        raise ValueError('unknown geometry %r' % geometry)
    x[:, :nbead] = p
    return x


def make(nbead, nstruct, seed, geometry='random', nbonds=50, envelopes=ENV_ONE, empty_rows=(), sigma=700.0,
         protocol=None):
    """atoms, poly, prm, ptr, sb, x.  With a second envelope (ENV_TWO) atoms.flags is
    (S, N): the beads of envelope 1 are a per-structure random half, as de_model has them.
    The structures listed in empty_rows get no per-structure bonds (an empty CSR row)."""
    rng = np.random.default_rng(seed)
    radii = rng.choice(RADII, nbead).astype(np.float32)
    atoms = M.Atoms(radii)
    chrom = np.repeat(np.arange(4), (nbead + 3) // 4)[:nbead]
    poly = M.polymer_bonds(chrom, np.zeros(nbead, np.int64), radii)
    prm = M.params_from_cfg({'optimization': {'optimizer_options': protocol or DEMO_PROTOCOL}}, envelopes)
    x = coordinates(nbead, nstruct, rng, geometry, sigma)
    per = []
    for s in range(nstruct):
        n = 0 if s in empty_rows else nbonds
        b = np.zeros(n, poly.dtype)
        b['i'] = rng.integers(0, nbead, n)
        b['j'] = (b['i'] + 1 + rng.integers(0, nbead - 1, n)) % nbead  # j != i
        b['r0'] = rng.uniform(100.0, 900.0, n)
        b['k'] = rng.uniform(0.5, 2.0, n)
        b[::3] = M.lower_bound(b[::3])
        per.append(b)
    ptr, sb = M.concat_bonds(per)
    if len(envelopes) > 1:
        flags = np.tile(atoms.flags, (nstruct, 1))
        for e in range(1, len(envelopes)):
            member = rng.random((nstruct, nbead)) < 0.5
            if geometry == 'origin':
                member[:, 0] = True  # the bead at the envelope centre meets the k < 0 envelope
            flags[:, :nbead][member] |= np.uint32(M.IGM_ATOM_ENV0 << e)
        atoms.flags = flags
    return atoms, poly, prm, ptr, sb, x


def struct_flags(atoms, s):
    return atoms.flags[s] if atoms.flags.ndim == 2 else atoms.flags


def struct_bonds(poly, ptr, sb, s):
    own = sb[ptr[s]:ptr[s + 1]] if sb is not None and ptr is not None else poly[:0]
    return np.concatenate([poly, own])


def brute_forces(x, radii, flags, bonds, envelopes, evf, envf, dtype=np.float64, parts=False):
    """Forces (N, 3) and energies (pair, bond, env0, ...) of one structure, every pair
    visited.  parts=True also returns {'pair', 'bond', 'env': [..]} force arrays and
    'mag' (N,), the sum over an atom's terms of each term's magnitude ('mag_pair' for
    the pair terms, 'mag' for the bond and envelope terms)."""
    T = dtype
    x = np.asarray(x).astype(T)
    n = len(x)
    radii = np.asarray(radii, np.float32)
    pi = T(np.pi)
    # ---- soft pairs between beads
    idx = np.nonzero((flags & M.IGM_ATOM_BEAD) != 0)[0]
    X, R = x[idx], radii[idx]
    rc = (R[:, None] + R[None, :]).astype(T)  # the f32 sum of two f32 radii
    r2 = np.zeros((len(idx), len(idx)), T)
    for d in range(3):
        dd = X[:, d][:, None] - X[:, d][None, :]
        r2 += dd * dd
    near = r2 < rc * rc
    np.fill_diagonal(near, False)
    pi_, pj_ = np.nonzero(near)
    dv = X[pi_] - X[pj_]
    r = np.sqrt(r2[pi_, pj_])
    c = rc[pi_, pj_]
    A = T(evf) * (c / pi) * (c / pi)
    e_pair = T(0.5) * np.sum(A * (T(1) + np.cos(pi * r / c)))  # each pair appears twice
    mag = np.where(r > 0, A * np.sin(pi * r / c) * pi / c / np.where(r > 0, r, T(1)), T(0))
    f_pair = np.zeros((n, 3), T)
    mag_pair = np.zeros(n, T)
    for d in range(3):
        f_pair[idx, d] = _segment_sum(mag * dv[:, d], pi_, len(idx), T)
    mag_pair[idx] = _segment_sum(np.abs(mag) * r, pi_, len(idx), T)
    # ---- bonds
    f_bond = np.zeros((n, 3), T)
    mag_rest = np.zeros(n, T)
    bi = bonds['i'].astype(np.int64)
    bj = (bonds['j'] & np.uint32(0x7fffffff)).astype(np.int64)
    low = (bonds['j'] >> np.uint32(31)) != 0
    bv = x[bi] - x[bj]
    br = np.sqrt(np.sum(bv * bv, axis=1, dtype=T))
    dr = br - bonds['r0'].astype(T)
    act = np.where(low, dr < 0, dr > 0)
    k = bonds['k'].astype(T)
    e_bond = np.sum(np.where(act, k * dr * dr, T(0)), dtype=T)
    g = np.where(act & (br > 0), T(-2) * k * dr / np.where(br > 0, br, T(1)), T(0))
    for d in range(3):
        np.add.at(f_bond[:, d], bi, g * bv[:, d])
        np.add.at(f_bond[:, d], bj, -g * bv[:, d])
    np.add.at(mag_rest, bi, np.abs(g) * br)
    np.add.at(mag_rest, bj, np.abs(g) * br)
    # ---- envelopes
    f_envs, e_envs = [], []
    for e, (abc, ke) in enumerate(envelopes):
        fe = np.zeros((n, 3), T)
        mem = np.nonzero((flags & np.uint32(M.IGM_ATOM_ENV0 << e)) != 0)[0]
        p = x[mem]
        s = (T(envf) * np.asarray(abc, T))[None, :] - radii[mem].astype(T)[:, None]
        k2 = np.sum(p * p / (s * s), axis=1, dtype=T)
        on = (k2 > 1) if ke > 0 else ((k2 > 0) & (k2 < 1))
        p, s, k2, who = p[on], s[on], k2[on], mem[on]
        rn = np.sqrt(np.sum(p * p, axis=1, dtype=T))
        sk = np.sqrt(k2)
        t = (T(1) - T(1) / sk) * rn
        grad = ((T(1) - T(1) / sk) / rn)[:, None] * p + (rn / (k2 * sk))[:, None] * p / (s * s)
        fe[who] = -T(abs(ke)) * t[:, None] * grad
        e_envs.append(T(0.5) * T(abs(ke)) * np.sum(t * t, dtype=T))
        mag_rest += np.sqrt(np.sum(fe * fe, axis=1, dtype=T))
        f_envs.append(fe)
    f = f_pair + f_bond
    for fe in f_envs:
        f = f + fe
    energies = np.array([e_pair, e_bond] + e_envs, np.float64)
    if parts:
        return f, energies, {'pair': f_pair, 'bond': f_bond, 'env': f_envs, 'mag': mag_rest, 'mag_pair': mag_pair}
    return f, energies


def _segment_sum(v, seg, nseg, T):
    """sum of v over equal seg (sorted ascending: np.nonzero order), in dtype T"""
    out = np.zeros(nseg, T)
    if len(v):
        starts = np.flatnonzero(np.r_[True, seg[1:] != seg[:-1]])
        out[seg[starts]] = np.add.reduceat(v, starts, dtype=T)
    return out


def brute_batch(atoms, poly, ptr, sb, x, envelopes, evf, envf, dtype=np.float64, parts=False):
    """brute_forces over the structures of a batch: forces (S, N, 3), energies (S, 2 + nenv)
    [, list of parts]."""
    out = [brute_forces(x[s], atoms.radii, struct_flags(atoms, s), struct_bonds(poly, ptr, sb, s), envelopes, evf,
                        envf, dtype, parts) for s in range(len(x))]
    f = np.stack([o[0] for o in out]).astype(np.float64)
    e = np.stack([o[1] for o in out])
    return (f, e, [o[2] for o in out]) if parts else (f, e)


def bonded_to(poly, ptr, sb, s, atom):
    """atoms sharing a bond with `atom` in structure s, and the atom itself"""
    b = struct_bonds(poly, ptr, sb, s)
    bi = b['i'].astype(np.int64)
    bj = (b['j'] & np.uint32(0x7fffffff)).astype(np.int64)
    return np.unique(np.concatenate([[atom], bj[bi == atom], bi[bj == atom]]))


def outlier_rest(poly, ptr, sb, x):
    """(S, N) bool: the atoms that neither are the outlier nor share a bond with it"""
    keep = np.ones(x.shape[:2], bool)
    for s in range(len(x)):
        keep[s, bonded_to(poly, ptr, sb, s, outlier_index(x.shape[1] - 1))] = False
    return keep


def term_magnitudes(parts, geometry):
    """(S, N) base of the absolute f32 bound: per atom, the summed magnitudes of its bond
    and envelope terms.  'coincident' has no other term (every pair force is exactly 0).
    In 'one_cell' the beads overlap at r of a few nm and each pair term is of the order
    evf r ~ 5: an atom without an active bond or envelope would be allowed no rounding
    at all, so there the pair terms' magnitudes count as well."""
    m = np.stack([p['mag'] for p in parts])
    if geometry == 'one_cell':
        m = m + np.stack([p['mag_pair'] for p in parts])
    return m


def f32_headroom(atoms, poly, ptr, sb, x, envelopes, evf, envf, keep=None):
    """1e-5 ||F64|| / ||F32 - F64|| of brute_forces over the batch (the atoms `keep`, (S, N) bool)."""
    f64, _ = brute_batch(atoms, poly, ptr, sb, x, envelopes, evf, envf)
    f32, _ = brute_batch(atoms, poly, ptr, sb, x, envelopes, evf, envf, np.float32)
    err = np.linalg.norm(f32 - f64, axis=2)
    ref = np.linalg.norm(f64, axis=2)
    if keep is not None:
        err, ref = err[keep], ref[keep]
    return 1e-5 * np.linalg.norm(ref) / max(np.linalg.norm(err), 1e-300)
