"""Plain NumPy restatement of the neighbourhood features (igm_report_neighbours in
include/igm_hip.h, igm_amd/report.py): the O(N^2) census one structure at a time, with the
norm and the bound in float32 exactly as the header defines them, the sequential
structure-order icp_sum, the host-side folds written out with loops, and the windowed Rg
built on report_ref.rg.  Everything the census kernel returns is compared with this by
equality, icp_sum included.
"""
import numpy as np

import report_ref as R

f32 = np.float32


def norms(p):
    """(n, n) float32: fl32(sqrt((dx*dx + dy*dy) + dz*dz)) between the rows of p (n, 3)"""
    p = np.asarray(p, f32)
    with np.errstate(invalid='ignore', over='ignore'):
        d = p[:, None, :] - p[None, :, :]
        d = d * d
        return np.sqrt((d[..., 0] + d[..., 1]) + d[..., 2])


def bounds(n, cutoff=None, radii=None, contact_range=None):
    """(n, n) float32: cutoff everywhere, or fl32(fl32(contact_range) * fl32(r_i + r_j))"""
    if radii is None:
        return np.full((n, n), f32(cutoff), f32)
    r = np.asarray(radii, f32)
    with np.errstate(invalid='ignore', over='ignore'):
        return (f32(contact_range) * (r[:, None] + r[None, :]).astype(f32)).astype(f32)


def columns(chain, cls, nclass):
    """(cis (n, n) bool, col (n, n)): the census column of partner j seen from i"""
    chain = np.asarray(chain)
    n = len(chain)
    label = np.full(n, nclass) if cls is None else np.where(np.asarray(cls) < 0, nclass, np.asarray(cls))
    cis = chain[:, None] == chain[None, :]
    return cis, np.where(cis, 0, 1 + label[None, :])


def census(xyz, chain, cls=None, nclass=0, min_sep=1, cutoff=500.0, radii=None, contact_range=None):
    """(nbead, nstruct, nclass + 2) int32"""
    xyz = np.asarray(xyz, f32)
    n, S = xyz.shape[:2]
    cis, col = columns(chain, cls, nclass)
    idx = np.arange(n)
    keep = ~(cis & (np.abs(idx[:, None] - idx[None, :]) < min_sep))
    keep[idx, idx] = False
    bound = bounds(n, cutoff, radii, contact_range)
    out = np.zeros((n, S, nclass + 2), np.int32)
    for s in range(S):
        with np.errstate(invalid='ignore'):
            hit = (norms(xyz[:, s]) <= bound) & keep  # a comparison with NaN is False
        for c in range(nclass + 2):
            out[:, s, c] = np.count_nonzero(hit & (col == c), axis=1)
    return out


def sums(cen):
    return cen.sum(axis=1, dtype=np.int64)


def icp(cen):
    """(icp_sum (nbead,) float64, icp_n (nbead,) int32): the quotients added one after the
    other in structure order (the last element of np.cumsum; np.sum is pairwise); adding
    +0.0 for a skipped structure changes no bit of a non-negative sum"""
    cis = cen[..., 0].astype(np.int64)
    trans = cen[..., 1:].sum(axis=2, dtype=np.int64)
    tot = cis + trans
    ok = tot > 0
    q = np.zeros(tot.shape, np.float64)
    q[ok] = trans[ok].astype(np.float64) / tot[ok].astype(np.float64)
    return np.cumsum(q, axis=1)[:, -1], np.count_nonzero(ok, axis=1).astype(np.int32)


def results(xyz, chain, cls=None, nclass=0, min_sep=1, cutoff=500.0, radii=None, contact_range=None):
    cen = census(xyz, chain, cls, nclass, min_sep, cutoff, radii, contact_range)
    s, n = icp(cen)
    return {'census': cen, 'sums': sums(cen), 'icp_sum': s, 'icp_n': n}


# ------------------------------------------------------------------ the host-side folds, with loops
def fold_mean(v, copy_ptr, copy_idx):
    """per haploid locus the mean of the copies' values that are not NaN (NaN without one)"""
    out = np.full(len(copy_ptr) - 1, np.nan)
    for h in range(len(out)):
        vals = [v[b] for b in copy_idx[copy_ptr[h]:copy_ptr[h + 1]] if not np.isnan(v[b])]
        if vals:
            out[h] = np.mean(vals)
    return out


def icp_per_locus(cen, copy_ptr, copy_idx):
    s, n = icp(cen)
    per_bead = np.array([s[b] / n[b] if n[b] else np.nan for b in range(len(n))])
    return fold_mean(per_bead, copy_ptr, copy_idx)


def mean_counts(cen, copy_ptr, copy_idx):
    m = sums(cen).astype(np.float64) / cen.shape[1]
    return np.stack([fold_mean(m[:, k], copy_ptr, copy_idx) for k in range(m.shape[1])], axis=1)


def trans_fraction(cen, copy_ptr, copy_idx):
    """(nhap, nclass): the median over (copy, structure) of n_k / the labelled trans partners"""
    nclass = cen.shape[2] - 2
    out = np.full((len(copy_ptr) - 1, nclass), np.nan)
    for h in range(len(out)):
        rows = []
        for b in copy_idx[copy_ptr[h]:copy_ptr[h + 1]]:
            for s in range(cen.shape[1]):
                lab = cen[b, s, 1:1 + nclass].astype(np.float64)
                if lab.sum() > 0:
                    rows.append(lab / lab.sum())
        if rows and nclass:
            out[h] = np.median(np.array(rows), axis=0)
    return out


# ------------------------------------------------------------------ local compaction
def windows(chrom, copy, halfwidth):
    """CSR of the beads within halfwidth positions of bead i on its (chrom, copy) chain,
    the chain's beads taken in index order and the window clipped at its ends"""
    chrom, copy = np.asarray(chrom), np.asarray(copy)
    ptr, idx, members = [0], [], {}
    for b in range(len(chrom)):
        members.setdefault((int(chrom[b]), int(copy[b])), []).append(b)
    for i in range(len(chrom)):
        mine = members[(int(chrom[i]), int(copy[i]))]
        p = mine.index(i)
        idx += mine[max(0, p - halfwidth):p + halfwidth + 1]
        ptr.append(len(idx))
    return np.array(ptr, np.int32), np.array(idx, np.int32)


def local_rg(xyz, chrom, copy, halfwidth):
    ptr, idx = windows(chrom, copy, halfwidth)
    return R.rg(xyz, ptr, idx), ptr
