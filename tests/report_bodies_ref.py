"""Plain NumPy restatement of the seeded nuclear bodies (igm_report_seed_bodies and
igm_report_body_features in include/igm_hip.h, igm_amd/report.py): the link test in float32
exactly as the header defines it, a plain union-find, the centres summed by an explicit
loop in rank order, and the features with the header's operation order, one loop over the
structures for the sums, and np.exp.  Labels, counts, sizes, centres, nearest, dist_sum,
dist_sqsum and assoc are compared with this by equality; tsa_sum carries the bar of
tests/test_report_bodies_gpu.py.
"""
import numpy as np

f32 = np.float32


def links(p, cutoff):
    """(n, n) bool: fl32(sqrt((dx*dx + dy*dy) + dz*dz)) <= cutoff between the rows of p
    (n, 3) float32, the diagonal False; a comparison with NaN is False"""
    p = np.asarray(p, f32)
    with np.errstate(invalid='ignore', over='ignore'):
        d = p[:, None, :] - p[None, :, :]
        d = d * d
        hit = np.sqrt((d[..., 0] + d[..., 1]) + d[..., 2]) <= f32(cutoff)
    np.fill_diagonal(hit, False)
    return hit


def link_pairs(p, cutoff, block=1024):
    """the linked pairs (a > b) of links(), found block by block so that 8192 seeds fit"""
    p = np.asarray(p, f32)
    out = []
    for a0 in range(0, len(p), block):
        with np.errstate(invalid='ignore', over='ignore'):
            d = p[a0:a0 + block, None, :] - p[None, :, :]
            d = d * d
            hit = np.sqrt((d[..., 0] + d[..., 1]) + d[..., 2]) <= f32(cutoff)
        a, b = np.nonzero(hit)
        a = a + a0
        out.append(np.stack([a[a > b], b[a > b]], axis=1))
    return np.concatenate(out)


def labels_of(n, pairs):
    """(n,) int32: the smallest rank of every seed's component (a plain union-find)"""
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for a, b in pairs:
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(a) for a in range(n)], np.int32)


def structure_bodies(p, cutoff, min_size):
    """(label (n,), sizes [k], centres [k][3] float64) of one structure's seeds p (n, 3)"""
    p = np.asarray(p, f32)
    label = labels_of(len(p), link_pairs(p, cutoff))
    sizes, centres = [], []
    for root in np.unique(label):                        # ascending label
        members = np.nonzero(label == root)[0]           # ascending rank
        if len(members) < min_size:
            continue
        acc = np.zeros(3, np.float64)
        with np.errstate(invalid='ignore'):
            for m in members:
                acc = acc + p[m].astype(np.float64)
            centres.append(acc / np.float64(len(members)))
        sizes.append(len(members))
    return label, sizes, centres


def seed_bodies(xyz, seed_idx, cutoff=500.0, min_size=3, max_bodies=None):
    """{'label' (S, n) int32, 'nbody' (S,) int32, 'size' (S, K) int32 with 0 past nbody,
    'centre' (S, K, 3) float64 with NaN past nbody}; K = max_bodies or nbody.max()"""
    xyz = np.asarray(xyz, f32)
    S = xyz.shape[1]
    seed_idx = np.asarray(seed_idx)
    per = [structure_bodies(xyz[seed_idx, s], cutoff, min_size) for s in range(S)]
    nbody = np.array([len(b[1]) for b in per], np.int32)
    K = int(nbody.max()) if max_bodies is None else int(max_bodies)
    size = np.zeros((S, K), np.int32)
    centre = np.full((S, K, 3), np.nan, np.float64)
    for s, (_, sizes, centres) in enumerate(per):
        for k in range(len(sizes)):
            size[s, k] = sizes[k]
            centre[s, k] = centres[k]
    return {'label': np.stack([b[0] for b in per]), 'nbody': nbody, 'size': size, 'centre': centre}


def component_sizes(label):
    """the member counts of the components of one structure's labels"""
    return np.unique(label, return_counts=True)[1]


def body_features(xyz, nbody, centre, assoc_cutoff=500.0, decay=0.004):
    """{'nearest' (n, S), 'dist_sum', 'dist_sqsum', 'assoc' int64, 'tsa_sum' (n,)}"""
    xyz = np.asarray(xyz, f32)
    n, S = xyz.shape[:2]
    centre = np.asarray(centre, np.float64)
    nearest = np.full((n, S), np.nan, np.float64)
    tval = np.zeros((n, S), np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        for s in range(S):
            x = xyz[:, s].astype(np.float64)
            bad = ~np.isfinite(x).all(axis=1)
            for k in range(int(nbody[s])):
                t = x - centre[s, k]
                d = np.sqrt((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2])
                d[bad] = np.nan
                if k == 0:
                    nearest[:, s] = d
                else:
                    lower = d < nearest[:, s]
                    nearest[lower, s] = d[lower]
                tval[:, s] = tval[:, s] + np.exp(-(np.float64(decay) * d))
        dist_sum = np.zeros(n, np.float64)
        dist_sqsum = np.zeros(n, np.float64)
        tsa_sum = np.zeros(n, np.float64)
        assoc = np.zeros(n, np.int64)
        for s in range(S):                               # structure order
            if nbody[s] > 0:
                dist_sum = dist_sum + nearest[:, s]
                dist_sqsum = dist_sqsum + nearest[:, s] * nearest[:, s]
            assoc += nearest[:, s] <= np.float64(assoc_cutoff)
            tsa_sum = tsa_sum + tval[:, s]
    return {'nearest': nearest, 'dist_sum': dist_sum, 'dist_sqsum': dist_sqsum, 'assoc': assoc, 'tsa_sum': tsa_sum}


def fold_mean(v, copy_ptr, copy_idx):
    """per haploid locus the mean of the copies' values that are not NaN (NaN without one)"""
    out = np.full(len(copy_ptr) - 1, np.nan)
    for h in range(len(out)):
        vals = [v[b] for b in copy_idx[copy_ptr[h]:copy_ptr[h + 1]] if not np.isnan(v[b])]
        if vals:
            out[h] = np.mean(vals)
    return out


def profiles(feat, nbody, copy_ptr, copy_idx):
    """(nhap, 4): mean distance, its standard deviation, association frequency, TSA"""
    nbody = np.asarray(nbody)
    S, m = len(nbody), int(np.count_nonzero(nbody > 0))
    nb = len(feat['dist_sum'])
    cols = np.full((nb, 4), np.nan)
    cols[:, 3] = feat['tsa_sum'] / S
    if m:
        for b in range(nb):
            mean = feat['dist_sum'][b] / m
            cols[b, 0] = mean
            var = feat['dist_sqsum'][b] / m - mean * mean
            cols[b, 1] = np.nan if np.isnan(var) else np.sqrt(max(0.0, var))   # a NaN stays one
            cols[b, 2] = feat['assoc'][b] / m
    return np.stack([fold_mean(cols[:, k], copy_ptr, copy_idx) for k in range(4)], axis=1)
