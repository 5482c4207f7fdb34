#!/opt/conda/bin/python3.9
"""Golden vectors for the edges of the ModelingStep violation record, produced by
running the REFERENCE's own classes on crafted particles: HarmonicUpperBound /
HarmonicLowerBound.getViolationRatio, EllipticEnvelope.getScores
(igm/model/forces.py:95-247) and get_violation_histogram (ModelingStep.py:859-869).
Build container only, like make_golden.py:

    /opt/conda/bin/python3.9 tests/golden/make_golden_violations.py

violations_edges_golden.npz holds, per case, the inputs, the reference's float64
ratios and its record (counts[101], violated_restr, n_violations, n_imposed; tol 0.05):

  bond cases   <c>_pos (n, 3) f32, <c>_radii (n) f32, <c>_i, <c>_j, <c>_r0 f32, <c>_k f32,
               <c>_lower (bool), <c>_cr f64 (> 0: d = cr * (r_i + r_j) as polymer.py:53,
               inter_hic.py:54; 0: d = float(f32 r0) as fish.py, sprite.py:61),
               <c>_ratios f64, <c>_rec int64 (104)
  envelopes    <c>_pos, <c>_radii, <c>_abc f64 (3), <c>_k, <c>_scale, <c>_ratios, <c>_rec
  cases        the names of the bond cases and of the envelope cases

The bond parameters the product stores as float32 (r0, k) reach the reference as
float(np.float32(.)).  The file is data only.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402,F401  (builds the reference environment)
import importlib  # noqa: E402
import numpy as np  # noqa: E402

forces = importlib.import_module('igm.model.forces')
Particle = importlib.import_module('igm.model.particle').Particle
get_violation_histogram = importlib.import_module('igm.steps.ModelingStep').get_violation_histogram
assert np.__version__.startswith('1.')

TOL = 0.05
# ratios j/100 whose np.histogram bin is int(v * 100) + 1 (EDGE_UP) or - 1 (EDGE_DOWN): the edge
# correction of np.histogram matters here
EDGE_UP, EDGE_DOWN = (29, 58), (35, 41, 47, 69, 70, 82, 83, 94, 95)


def norm_is_plain(v):
    """np.linalg.norm of a float32 3-vector is sqrt(x.dot(x)), and the BLAS behind the dot product
    either adds the float32 squares in float32 or accumulates them in float64 and rounds once,
    depending on the kernel it picks for the CPU it runs on (about one vector in ten differs by an
    ulp).  The existing goldens were written where it adds in float32, which is what the product
    restates.  This file uses only vectors for which both give the same bits, so it is the same
    wherever it is generated."""
    v = np.asarray(v, np.float32)
    plain = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    p = (v * v).astype(np.float64)
    wide = np.sqrt(np.float32((p[0] + p[1]) + p[2]))
    assert plain.dtype == np.float32 and wide.dtype == np.float32
    assert np.linalg.norm(v) in (plain, wide)
    return plain == wide


def record(vs, n_imposed):
    """the record of ModelingStep.task:542-554"""
    vs = np.array(vs)
    H, _ = get_violation_histogram(vs)
    return np.concatenate([H, [np.count_nonzero(vs), np.count_nonzero(vs > TOL), n_imposed]]).astype(np.int64)


def bond_case(out, name, pos, radii, i, j, r0, k, lower, cr):
    pos = np.asarray(pos, np.float32)
    radii = np.asarray(radii, np.float32)
    r0 = np.broadcast_to(np.asarray(r0, np.float32), np.shape(i)).copy()
    k = np.broadcast_to(np.asarray(k, np.float32), np.shape(i)).copy()
    lower = np.broadcast_to(np.asarray(lower, bool), np.shape(i)).copy()
    parts = [Particle(p, r, Particle.NORMAL) for p, r in zip(pos, radii)]
    vs = []
    for q in range(len(i)):
        a, b = int(i[q]), int(j[q])
        assert norm_is_plain(parts[a].pos - parts[b].pos)
        d = cr * (parts[a].r + parts[b].r) if cr > 0 else float(np.float32(r0[q]))
        cls = forces.HarmonicLowerBound if lower[q] else forces.HarmonicUpperBound
        vs.append(cls((a, b), d, float(np.float32(k[q]))).getViolationRatio(parts))
    out.update({name + '_pos': pos, name + '_radii': radii, name + '_i': np.asarray(i, np.int32),
                name + '_j': np.asarray(j, np.int32), name + '_r0': r0, name + '_k': k, name + '_lower': lower,
                name + '_cr': np.float64(cr), name + '_ratios': np.array(vs, np.float64),
                name + '_rec': record(vs, len(i))})
    return np.array(vs, np.float64)


def ladder(axis, d, offsets):
    """atom 0 at the origin, atom 1 + q on the axis at d + offsets[q] * d / 100 (integers: exact in f32)"""
    pos = np.zeros((len(offsets) + 1, 3))
    pos[1:, axis] = d + np.asarray(offsets, np.float64) * (d / 100.0)
    assert np.all(pos == np.round(pos)) and np.all(pos >= 0)
    n = len(offsets)
    return pos, np.full(n + 1, 10.0), np.zeros(n, np.int32), np.arange(1, n + 1, dtype=np.int32)


def make_bonds(out):
    names = []
    up = np.arange(251)
    for tag, axis, d, k in (('up100', 0, 100.0, 1.0), ('up300', 1, 300.0, 1.0), ('up700', 2, 700.0, 1.0),
                            ('up100k', 0, 100.0, 0.37), ('up700k', 1, 700.0, 0.37)):
        pos, radii, i, j = ladder(axis, d, up)
        vs = bond_case(out, tag, pos, radii, i, j, d, k, False, 0.0)
        names.append(tag)
        if k == 1.0:
            assert np.array_equal(vs, up / 100.0)
            assert vs[5] == TOL and vs[100] == 1.0 and np.count_nonzero(vs > 1) == 150
            inner = vs[:101]
            ref_bin = np.minimum(np.searchsorted(np.linspace(0, 1, 101), inner, side='right') - 1, 99)
            H, _ = np.histogram(inner, bins=100, range=(0, 1))
            assert np.array_equal(np.bincount(ref_bin, minlength=100), H)
            plain = np.minimum((inner * 100).astype(int), 99)
            assert all(ref_bin[q] == plain[q] + 1 for q in EDGE_UP), 'int(v*100) must fall short here'
            assert all(ref_bin[q] == plain[q] - 1 for q in EDGE_DOWN), 'int(v*100) must overshoot here'
    down = np.concatenate([-np.arange(101), np.arange(1, 21)])  # distances 100 - j, then above d
    for tag, axis, k in (('lo100', 2, 1.0), ('lo100k', 0, 0.37)):
        pos, radii, i, j = ladder(axis, 100.0, down)
        vs = bond_case(out, tag, pos, radii, i, j, 100.0, k, True, 0.0)
        names.append(tag)
        if k == 1.0:
            assert np.array_equal(vs[:101], np.arange(101) / 100.0) and np.all(vs[101:] == 0)
    # d == 0: ratio 0 whatever the distance, upper and lower bound
    pos = np.zeros((9, 3))
    pos[1:, 0] = [0, 1, 3, 50, 1000, 7, 0, 250]
    i, j = np.zeros(8, np.int32), np.arange(1, 9, dtype=np.int32)
    vs = bond_case(out, 'zero_d', pos, np.full(9, 10.0), i, j, 0.0, [1.0, 1.0, 0.37, 1.0, 1.0, 1.0, 0.37, 1.0],
                   [False] * 5 + [True] * 3, 0.0)
    assert np.all(vs == 0)
    names.append('zero_d')
    # d from the radii: sums that round in f32, f64 product with the contact range
    rng = np.random.RandomState(11)
    for tag, cr in (('radii_cr2', 2.0), ('radii_cr105', 1.05)):
        n = 300
        radii = rng.uniform(40.0, 260.0, n).astype(np.float32)
        i = rng.randint(0, n, 600).astype(np.int32)
        j = ((i + 1 + rng.randint(0, n - 1, 600)) % n).astype(np.int32)
        # pull every pair to a distance of d * U(0.7, 2.3) along its own random direction
        pos = np.zeros((n + 2 * len(i), 3))
        pos[:n] = rng.uniform(-3000.0, 3000.0, (n, 3))
        radii = np.concatenate([radii, np.zeros(2 * len(i), np.float32)])
        ii, jj = [], []
        for q in range(len(i)):  # the bond joins two fresh atoms that carry the radii of (i, j)
            a, b = n + 2 * q, n + 2 * q + 1
            radii[a], radii[b] = radii[i[q]], radii[j[q]]
            while True:
                u = rng.normal(0.0, 1.0, 3)
                u /= np.linalg.norm(u)
                dd = cr * float(radii[a] + radii[b]) * rng.uniform(0.7, 2.3)
                pos[a] = rng.uniform(-3000.0, 3000.0, 3)
                pos[b] = pos[a] + u * dd
                if norm_is_plain(pos[a].astype(np.float32) - pos[b].astype(np.float32)):
                    break
            ii.append(a)
            jj.append(b)
        # boundary bonds: the second atom sits at exactly float32(d) on an axis, where the stored
        # f32 r0 and the f64 d = cr * (r_i + r_j) disagree on whether the bond is stretched
        nb = 0
        for q in range(0, len(i), 3):
            a, b = ii[q], jj[q]
            d64 = cr * float(np.float32(radii[a] + radii[b]))
            pos[a] = 0.0
            pos[b] = 0.0
            pos[b, (q // 3) % 3] = np.float32(d64)
            nb += float(np.float32(d64)) > d64
        assert cr == 2.0 or nb >= 20
        r0 = (cr * (radii[ii] + radii[jj]).astype(np.float32).astype(np.float64)).astype(np.float32)
        vs = bond_case(out, tag, pos, radii, np.array(ii, np.int32), np.array(jj, np.int32), r0, 1.0, False, cr)
        assert len(np.unique(np.minimum((vs[vs <= 1] * 100).astype(int), 99))) >= 50 and np.any(vs > 1)
        names.append(tag)
    return names


def make_envelopes(out):
    rng = np.random.RandomState(12)
    names = []
    n = 2000
    for shape, abc in (('sph', (5000.0, 5000.0, 5000.0)), ('ell', (6000.0, 4500.0, 3000.0))):
        m = n + n // 4
        u = rng.normal(0.0, 1.0, (m, 3))
        u /= np.linalg.norm(u, axis=1)[:, None]
        s = np.where(rng.rand(m) < 0.5, rng.uniform(0.0, 1.0, m), rng.uniform(0.9, 1.3, m))
        s[:60] = rng.uniform(1.5, 3.0, 60)  # far outside: k > 0 ratios above 1
        pos = (u * np.asarray(abc) * s[:, None]).astype(np.float32)
        pos = pos[[norm_is_plain(x) for x in pos]][:n]
        assert len(pos) == n
        pos[40] = 0.0  # the origin: 1.0 for k < 0
        pos[41] = [abc[0], 0.0, 0.0]
        pos[42] = [0.0, 0.0, -abc[2]]
        radii = rng.uniform(40.0, 260.0, n).astype(np.float32)
        parts = [Particle(p, r, Particle.NORMAL) for p, r in zip(pos, radii)]
        a, b, c = abc
        for k in (1.0, -1.0):
            if k > 0:  # Envelope._apply_sphere_envelop (restraints/envelope.py:46-51)
                f = forces.EllipticEnvelope(list(range(n)), 0, (a, b, c), k, scale=0.1 * np.mean([a, b, c]))
            else:  # Damid._apply_envelope (restraints/damid.py:117-134), contact_range 0.05, k 1
                cutoff = 1 - 0.05
                f = forces.EllipticEnvelope(list(range(n)), 0, np.array([a, b, c]) * cutoff, -1.0,
                                            scale=cutoff * np.mean([a, b, c]))
            vs = np.asarray(f.getScores(parts), np.float64)
            assert all(norm_is_plain(p.pos) for p in parts)
            name = '%s_k%+d' % (shape, int(k))
            bins = np.unique(np.minimum((vs[(vs > 0) & (vs <= 1)] * 100).astype(int), 99))
            assert len(bins) >= 20, (name, len(bins))
            assert np.count_nonzero(vs == 0) > n // 5 and np.count_nonzero(vs) > n // 5
            if k > 0:
                assert np.count_nonzero(vs > 1) >= 20
            else:
                assert vs[40] == 1.0
            out.update({name + '_pos': pos, name + '_radii': radii, name + '_abc': np.asarray(f.semiaxes, np.float64),
                        name + '_k': np.float64(f.k), name + '_scale': np.float64(f.scale), name + '_ratios': vs,
                        name + '_rec': record(vs, n)})
            names.append(name)
    return names


def main():
    out = {}
    out['bond_cases'] = np.array(make_bonds(out))
    out['env_cases'] = np.array(make_envelopes(out))
    out['tol'] = np.float64(TOL)
    path = os.path.join(HERE, 'violations_edges_golden.npz')
    np.savez_compressed(path, **out)
    print('violations_edges_golden.npz', os.path.getsize(path))


if __name__ == '__main__':
    main()
