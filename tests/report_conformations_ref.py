"""Plain NumPy restatement of the pairwise conformation RMSD (igm_report_conformations in
include/igm_hip.h, igm_amd/report.py), written independently of the library: centring and g
in float64, the optimal superposition by Kabsch's SVD with the determinant correction
(proper rotations only; Kabsch 1978) instead of Horn's eigenvalue, one rounding to float32,
the NaN rules, and every reduction computed from the float32 matrix.

conformations()  everything the entry returns, from the population and the bead table
reductions()     row_sum (sequential float64), row_n, same and hist of a float32 matrix: what
                 the GPU tests recompute from the matrix the library returned
bound()          the project's bar for this superposition core (tests/tracing_assign.py:
                 bound): |gpu - ref| <= 1e-6 ref + sqrt(1e-12 (g_a + g_b) / nlocus)
summary()        conformation_summary's numbers from the float32 matrix itself
"""
import numpy as np

f32 = np.float32


def gather(xyz, bead):
    """(M, nlocus, 3) float64: conformation a = k * nstruct + s"""
    xyz = np.asarray(xyz, f32)
    bead = np.asarray(bead)
    ncopy, nlocus = bead.shape
    x = xyz[bead].astype(np.float64)                       # (ncopy, nlocus, S, 3)
    return np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(ncopy * xyz.shape[1], nlocus, 3)


def centred(x):
    """(p, g, bad): the centred conformations (zeros where a coordinate is not finite), g (NaN
    there) and the flag"""
    bad = ~np.isfinite(x).all(axis=(1, 2))
    x = np.where(bad[:, None, None], 0.0, x)
    p = x - x.mean(axis=1, keepdims=True)
    g = (p * p).sum(axis=(1, 2))
    g[bad] = np.nan
    return p, g, bad


def kabsch_lambda(m):
    """sum of the singular values of the (..., 3, 3) covariances, the smallest one negated
    where the optimal orthogonal map is a reflection"""
    u, s, vt = np.linalg.svd(m)
    d = np.sign(np.linalg.det(u) * np.linalg.det(vt))
    return s[..., 0] + s[..., 1] + d * s[..., 2]


def rmsd_matrix(xyz, bead):
    """((M, M) float32, g (M,) float64)"""
    p, g, bad = centred(gather(xyz, bead))
    M, n = p.shape[:2]
    r = np.zeros((M, M), f32)
    ia, ib = np.triu_indices(M, 1)
    if len(ia):
        cov = np.tensordot(p, p, axes=([1], [1])).transpose(0, 2, 1, 3)    # (M, M, 3, 3): sum_i p_i^a (x) p_i^b
        lam = kabsch_lambda(cov[ia, ib])
        with np.errstate(invalid='ignore'):
            v = np.sqrt(np.maximum(0.0, (g[ia] + g[ib] - 2.0 * lam) / n)).astype(f32)
        r[ia, ib] = v
        r[ib, ia] = v
    r[bad, :] = np.nan
    r[:, bad] = np.nan
    return r, g


def reductions(r, nstruct, edges=None):
    """{'row_sum', 'row_n', 'same', 'hist'} of the (M, M) float32 matrix r"""
    r = np.asarray(r, f32)
    M = len(r)
    ncopy = M // nstruct
    off = np.isfinite(r) & ~np.eye(M, dtype=bool)
    terms = np.where(off, r, f32(0)).astype(np.float64)
    row_sum = np.cumsum(terms, axis=1)[:, -1]              # cumsum adds in sequence
    k = np.arange(ncopy) * nstruct
    same = np.stack([r[np.ix_(k + s, k + s)] for s in range(nstruct)])
    hist = None
    if edges is not None:
        ia, ib = np.triu_indices(M, 1)
        v = r[ia, ib]
        hist = np.histogram(v[np.isfinite(v)], bins=np.asarray(edges, f32))[0].astype(np.int64)
    return {'row_sum': row_sum, 'row_n': off.sum(axis=1).astype(np.int32), 'same': np.ascontiguousarray(same),
            'hist': hist}


def conformations(xyz, bead, edges=None):
    r, g = rmsd_matrix(xyz, bead)
    out = {'rmsd': r, 'g': g}
    out.update(reductions(r, np.asarray(xyz).shape[1], edges))
    return out


def bound(ref, g, nlocus):
    """(M, M) float64 bar on |gpu - ref| (NaN where ref is); holds while nlocus <= 9000"""
    return 1e-6 * ref.astype(np.float64) + np.sqrt(1e-12 * (g[:, None] + g[None, :]) / nlocus)


def summary(r, g, nstruct, nlocus):
    """conformation_summary's numbers, from the matrix: every mean is taken over the entries
    themselves"""
    r = np.asarray(r, np.float64)
    M = len(r)
    ncopy = M // nstruct
    off = np.isfinite(r) & ~np.eye(M, dtype=bool)
    with np.errstate(invalid='ignore', divide='ignore'):
        mean_rmsd = np.array([r[a][off[a]].mean() if off[a].any() else np.nan for a in range(M)])
    copy_of, struct_of = np.arange(M) // nstruct, np.arange(M) % nstruct
    same = off & (struct_of[:, None] == struct_of[None, :])
    diff = off & ~same
    res = {'mean_rmsd': mean_rmsd, 'mean': r[off].mean() if off.any() else np.nan,
           'mean_rg': np.sqrt(g[np.isfinite(g)] / nlocus).mean()}
    res['variability'] = res['mean'] / res['mean_rg']
    a = int(np.nanargmin(mean_rmsd)) if np.isfinite(mean_rmsd).any() else 0
    res['medoid'] = (int(struct_of[a]), int(copy_of[a]))
    res['medoid_mean_rmsd'] = mean_rmsd[a]
    res['same_mean'] = r[same].mean() if ncopy > 1 and same.any() else np.nan
    res['different_mean'] = r[diff].mean() if ncopy > 1 and diff.any() else np.nan
    res['ratio'] = res['same_mean'] / res['different_mean']
    return res
