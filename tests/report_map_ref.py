"""Plain NumPy restatement of the report on imaged nuclei (include/igm_hip.h:
igm_report_map_levels, igm_report_map_lamina; igm_amd/report.py: map_depth_scale,
map_shell_volumes), every promotion written out.  The checker of test_report_map.py and
test_report_map_gpu.py.

Per-element values use the operations the header names, so they are bit-equal to the
kernel's; sums are NumPy's, whose order differs from the kernel's (the tests bound that
difference by 2 n 2^-53).

The keyword switches restate a definition with ONE deliberate mistake; the tests use them
to show that an input tells the mistake from the contract:
  half_up       floor(x + 0.5) for rint in the voxel index
  swap_stride   n[1] for n[2] in the voxel offset
  no_voxel_clamp  the offset of an out-of-grid voxel taken from the unclamped index (wrapped
                into the map's table, where a kernel would read past it)
  ignore_w      the inside flag not read
  no_level_clamp  the raw level 1 - depth / scale
  own_radius    each copy's own radius in the contact test
  strict        < for <= in the contact test
  ignore_side   side = -1 treated as +1
"""
import numpy as np

import report_ref as R

f32, f64 = np.float32, np.float64


def geometry(vol):
    """(n int64 (3,), origin f64 (3,), grid f64 (3,)): the float32 header widened"""
    return (np.asarray(vol['nvoxel'], np.int64), np.asarray(vol['origin'], f32).astype(f64),
            np.asarray(vol['grid'], f32).astype(f64))


def voxel(xyz, vol, half_up=False):
    """(u float64 (..., 3) the rounded unclamped index, v int64 clamped, in_grid bool)"""
    n, o, g = geometry(vol)
    x = np.asarray(xyz, f32).astype(f64)
    q = (x - o) / g
    u = np.floor(q + 0.5) if half_up else np.rint(q)  # np.rint: half to even
    in_grid = np.all((u >= 0) & (u <= (n - 1).astype(f64)), axis=-1)
    v = np.clip(u, 0, (n - 1).astype(f64)).astype(np.int64)
    return u, v, in_grid


def depth(xyz, vol, half_up=False, swap_stride=False, no_voxel_clamp=False, ignore_w=False):
    """signed depth (...,) f64 of beads (..., 3) f32 on one map"""
    n, o, g = geometry(vol)
    x = np.asarray(xyz, f32).astype(f64)
    u, v, in_grid = voxel(xyz, vol, half_up)
    w = u.astype(np.int64) if no_voxel_clamp else v
    off = (w[..., 0] * n[1] + w[..., 1]) * (n[1] if swap_stride else n[2]) + w[..., 2]
    table = np.asarray(vol['matrice'], np.int32).reshape(-1, 4)
    rec = table[np.mod(off, len(table))]  # the contract never leaves the table; a mistake wraps
    L = rec[..., :3].astype(f64) * g + o
    t = x - L
    t0, t1, t2 = t[..., 0], t[..., 1], t[..., 2]
    dist = np.sqrt((t0 * t0 + t2 * t2) + t1 * t1)
    inside = in_grid if ignore_w else in_grid & (rec[..., 3] != 0)
    return np.where(inside, dist, -dist)


def depth_scale(vol):
    """max over the voxels with w != 0 of |(v - e) * grid| in float64"""
    n, _, g = geometry(vol)
    mat = np.asarray(vol['matrice'], np.int32)
    best = -1.0
    for i in range(n[0]):
        for j in range(n[1]):
            rec = mat[i, j]  # (n2, 4)
            sel = rec[:, 3] != 0
            if not sel.any():
                continue
            k = np.arange(n[2])[sel]
            t0 = (i - rec[sel, 0].astype(np.int64)).astype(f64) * g[0]
            t1 = (j - rec[sel, 1].astype(np.int64)).astype(f64) * g[1]
            t2 = (k - rec[sel, 2].astype(np.int64)).astype(f64) * g[2]
            best = max(best, float(np.sqrt((t0 * t0 + t2 * t2) + t1 * t1).max()))
    return best


def level_of_depth(d, scale, no_level_clamp=False):
    lv = 1.0 - d / f64(scale)
    return lv if no_level_clamp else np.where(lv > 0.0, lv, 0.0)


def levels(xyz, vols, smap, scales=None, no_level_clamp=False, **kw):
    """(level (nbead, nstruct) f64, depth (nbead, nstruct) f64); smap None: map 0"""
    xyz = np.asarray(xyz, f32)
    S = xyz.shape[1]
    smap = np.zeros(S, np.int64) if smap is None else np.asarray(smap)
    scales = [depth_scale(v) for v in vols] if scales is None else scales
    lev, dep = np.empty(xyz.shape[:2]), np.empty(xyz.shape[:2])
    for s in range(S):
        m = int(smap[s])
        dep[:, s] = depth(xyz[:, s], vols[m], **kw)
        lev[:, s] = level_of_depth(dep[:, s], scales[m], no_level_clamp)
    return lev, dep


def mean_over_structures(a):
    """(nbead,) f64: the sum over the structures in structure order, then one division --
    the order the header states for level_mean and depth_mean, so this one is bit-equal"""
    a = np.asarray(a, f64)
    acc = np.zeros(a.shape[0])
    for s in range(a.shape[1]):
        acc = acc + a[:, s]
    return acc / f64(a.shape[1])


def shells_of_levels(lev, nshell, edges=None):
    """report_ref.shells on a level matrix (nbead, nstruct)"""
    n, S = lev.shape
    bds = R.shell_bounds(n, nshell)
    mean = np.full((S, nshell), np.nan)
    hist = None if edges is None else np.zeros((nshell, len(edges) - 1), np.int64)
    for s in range(S):
        r = np.sort(lev[:, s])
        for j in range(nshell):
            part = r[bds[j]:bds[j + 1]]
            if len(part):
                mean[s, j] = part.sum() / len(part)
                if hist is not None:
                    hist[j] += R.histogram(part, edges)
    return mean, hist


def lamina_counts(xyz, radii, copy_ptr, copy_idx, vols, smap, thr, side, own_radius=False, strict=False,
                  ignore_side=False, **kw):
    """(nhap,) int64: the (copy, structure) with side * depth - f64(r) <= thr[map]"""
    xyz = np.asarray(xyz, f32)
    S = xyz.shape[1]
    smap = np.zeros(S, np.int64) if smap is None else np.asarray(smap)
    thr_s = np.asarray(thr, f64)[smap]
    sgn = 1 if ignore_side else side
    nhap = len(copy_ptr) - 1
    out = np.zeros(nhap, np.int64)
    dep = levels(xyz, vols, smap, scales=[1.0] * len(vols), **kw)[1]
    for h in range(nhap):
        beads = copy_idx[copy_ptr[h]:copy_ptr[h + 1]]
        for b in beads:
            r = f64(np.asarray(radii, f32)[b if own_radius else beads[0]])
            d = dep[b]
            v = (d if sgn > 0 else -d) - r
            out[h] += np.count_nonzero(v < thr_s if strict else v <= thr_s)
    return out


def shell_volumes(vol, edges, scale=None):
    """V[k]: voxel volume times the inside voxels whose centre level falls in bin k"""
    n, _, g = geometry(vol)
    scale = depth_scale(vol) if scale is None else scale
    mat = np.asarray(vol['matrice'], np.int32)
    idx = np.stack(np.meshgrid(*[np.arange(k) for k in n], indexing='ij'), axis=-1)
    sel = mat[..., 3] != 0
    t = (idx[sel] - mat[sel][:, :3].astype(np.int64)).astype(f64) * g
    d = np.sqrt((t[:, 0] * t[:, 0] + t[:, 2] * t[:, 2]) + t[:, 1] * t[:, 1])
    return R.histogram(1.0 - d / f64(scale), edges).astype(f64) * (g[0] * g[1] * g[2])


def population_volumes(vols, smap, nstruct, edges):
    """sum over the structures of the shell volumes of their maps"""
    smap = np.zeros(nstruct, np.int64) if smap is None else np.asarray(smap)
    out = np.zeros(len(edges) - 1)
    for m, v in enumerate(vols):
        k = int(np.count_nonzero(smap == m))
        if k:
            out += k * shell_volumes(v, edges)
    return out
