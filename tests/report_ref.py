"""Plain NumPy float64 restatement of the five report definitions (igm_amd/report.py,
include/igm_hip.h): the checker of the synthetic cases of test_report_gpu.py and the
bridge between the GPU outputs and the reference's own numbers (report_golden.npz).

Every per-element value is computed with the operations the header names, so it is
bit-equal to the kernel's; the sums are np.sum / cumulative sums in float64, whose order
differs from the kernel's (the tests bound that difference by 2 n 2^-53).
"""
import numpy as np


def levels(xyz, semiaxes):
    """(nbead, nstruct) f64: sqrt(((x/a)^2 + (y/b)^2) + (z/c)^2) on the widened coordinates"""
    q = np.asarray(xyz, np.float32).astype(np.float64) / np.asarray(semiaxes, np.float64)
    q = q * q
    return np.sqrt((q[..., 0] + q[..., 1]) + q[..., 2])


def level_mean(xyz, semiaxes):
    return levels(xyz, semiaxes).sum(axis=1) / xyz.shape[1]


def histogram(values, edges):
    """counts with edges[k] <= v < edges[k+1], the last bin closed, the rest dropped"""
    values = np.asarray(values, np.float64).ravel()
    edges = np.asarray(edges, np.float64)
    nb = len(edges) - 1
    k = np.searchsorted(edges, values, side='right') - 1
    k[values == edges[-1]] = nb - 1
    ok = (values >= edges[0]) & (values <= edges[-1])
    return np.bincount(k[ok], minlength=nb)[:nb].astype(np.int64)


def shell_bounds(n, nshell):
    return [int(k * n / nshell) for k in range(nshell)] + [n]


def shells(xyz, semiaxes, nshell, edges=None):
    """(shell_mean (nstruct, nshell), shell_hist (nshell, hnbins) or None)"""
    lev = levels(xyz, semiaxes)
    n, S = lev.shape
    bds = shell_bounds(n, nshell)
    mean = np.full((S, nshell), np.nan)
    hist = None if edges is None else np.zeros((nshell, len(edges) - 1), np.int64)
    for s in range(S):
        r = np.sort(lev[:, s])
        for j in range(nshell):
            part = r[bds[j]:bds[j + 1]]
            if len(part):
                mean[s, j] = part.sum() / len(part)
                if hist is not None:
                    hist[j] += histogram(part, edges)
    return mean, hist


def rg(xyz, chain_ptr, chain_idx):
    """(nchain, nstruct) f64: two passes in float64"""
    nchain = len(chain_ptr) - 1
    out = np.full((nchain, xyz.shape[1]), np.nan)
    for c in range(nchain):
        ii = np.asarray(chain_idx[chain_ptr[c]:chain_ptr[c + 1]])
        if len(ii) == 0:
            continue
        p = np.asarray(xyz, np.float32)[ii].astype(np.float64)  # (n, S, 3)
        v = p - p.sum(axis=0) / len(ii)
        v = v * v
        out[c] = np.sqrt(((v[..., 0] + v[..., 1]) + v[..., 2]).sum(axis=0) / len(ii))
    return out


def lamina_denoms(semiaxes, contact_range, radii, copy_ptr, copy_idx):
    """(nhap, 3) f64: the reference's (semiaxes * (1 - contact_range) - r)**2, r the
    float32 radius of the locus's first copy (report/damid.py:39-47, utils.py:86)"""
    nhap = len(copy_ptr) - 1
    out = np.empty((nhap, 3))
    for h in range(nhap):
        r = np.asarray(radii, np.float32)[copy_idx[copy_ptr[h]]]
        nuc_rad = np.array(semiaxes) * (1 - contact_range)
        a, b, c = np.array(nuc_rad) - r
        out[h] = (a**2, b**2, c**2)
    return out


def lamina_counts(xyz, copy_ptr, copy_idx, denoms):
    xyz = np.asarray(xyz, np.float32)
    nhap = len(copy_ptr) - 1
    out = np.zeros(nhap, np.int64)
    for h in range(nhap):
        for b in copy_idx[copy_ptr[h]:copy_ptr[h + 1]]:
            sq = (xyz[b] * xyz[b]).astype(np.float64)  # squared in float32, then widened
            v = (sq[:, 0] / denoms[h, 0] + sq[:, 1] / denoms[h, 1]) + sq[:, 2] / denoms[h, 2]
            out[h] += np.count_nonzero(v >= 1)
    return out


def pair_mean(xyz, k, m):
    """mean over the structures (float64) of the float32 norm of bead k - bead m"""
    d = xyz[k] - xyz[m]
    d = d * d
    return np.sqrt((d[:, 0] + d[:, 1]) + d[:, 2]).astype(np.float64).sum() / xyz.shape[1]


def distance_entry(xyz, copy_ptr, copy_idx, hap_chrom, a, b):
    xyz = np.asarray(xyz, np.float32)
    if a == b:
        return 0.0
    a, b = min(a, b), max(a, b)
    ca = copy_idx[copy_ptr[a]:copy_ptr[a + 1]]
    cb = copy_idx[copy_ptr[b]:copy_ptr[b + 1]]
    if hap_chrom[a] == hap_chrom[b]:
        aves = [pair_mean(xyz, k, m) for k, m in zip(ca, cb)]
    else:
        aves = [pair_mean(xyz, k, m) for k in ca for m in cb]
    if not aves:
        return np.nan
    t = 0.0
    for v in aves:
        t += v
    return t / len(aves)


def distance_map(xyz, copy_ptr, copy_idx, hap_chrom):
    nhap = len(copy_ptr) - 1
    out = np.zeros((nhap, nhap))
    for a in range(nhap):
        for b in range(a + 1, nhap):
            out[a, b] = out[b, a] = distance_entry(xyz, copy_ptr, copy_idx, hap_chrom, a, b)
    return out
