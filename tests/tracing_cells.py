"""Test helper for the joint placement of the traces of an imaged cell
(igm_tracing_assign_cells, igm_amd.tracing.assign_cell_costs).

The cost of (cell c, structure s) restated in fp64 NumPy, independently of the library
(np.linalg.eigh for the independent costs, np.linalg.svd for the joint superposition; no Jacobi):

cell_sums()      q_i = p_i - mean over the cell; per trace n_t, sq_t, sqq_t; per (trace, copy,
                 structure) sx, sxx and m[a][b] = sum q_a x_b of x_i = bead - o_s, o_s the bead of
                 the cell's first spot under copy 0.
joint()          cost, R, tau and the scale (Ga + Gb) / n of a labelling.
search()         the start (per chromosome the injective labelling of least independent cost, in
                 lexicographic order, first minimum) and at most ROUNDS re-labelling rounds; with
                 the cost after every joint fit and the decision margin of every choice:
                 second-smallest minus smallest labelling sum of the chromosome, relative to the
                 chromosome's sum of sqq_t + sxx at the chosen labelling (inf: one labelling only).
brute()          the least joint cost over ALL labellings of the cell.
cells_oracle()   search() on every (cell, structure).
genome()         the six-chromosome genome of the tests; planted() its planted cells.
cpu_cells()      the oracle as the 'tracing_assign_cells' kernel of a Step kernel set;
register_cpu_kernels() registers 'tracing_cells_test' on top of 'tracing_assign_test'.
"""
import itertools

import numpy as np

import tracing_assign as TA
from igm_amd import tracing as T
from igm_amd import workloads as W

ROUNDS = 16
# (chromosome, loci, copies): 8-14 loci, one single-copy chromosome
CHROMS = ((0, 12, 2), (1, 9, 2), (2, 14, 1), (3, 8, 2), (4, 11, 2), (5, 10, 2))
CALLS = []


def genome(S, seed=0, chroms=CHROMS):
    ix = TA.index(chroms)
    return ix, TA.random_walks(ix, S, seed)


def drop(traces, keep):
    """the trace set without the traces where keep is False (cell_ptr follows)"""
    ptr, cp = traces['trace_ptr'], traces['cell_ptr']
    keep = np.asarray(keep, bool)
    spots = np.repeat(keep, np.diff(ptr))
    cell = np.repeat(np.arange(len(cp) - 1), np.diff(cp))
    return {'trace_ptr': np.concatenate([[0], np.cumsum(np.diff(ptr)[keep])]).astype(np.int64),
            'locus': traces['locus'][spots], 'position': traces['position'][spots],
            'cell_ptr': np.concatenate([[0], np.cumsum(np.bincount(cell[keep], minlength=len(cp) - 1))]).astype(np.int64)}


def planted(ix, xyz, ncell=18, nspots=8, noise=(0.0, 30.0, 150.0), seed=3, missing_chrom=5):
    """ncell cells planted on distinct structures (workloads.synthetic_cells), noise cycling over
    `noise`; the copy-1 homologue of chromosome `missing_chrom` is not imaged.  Returns the
    checked traces, the planted structure (ncell,) and the planted copy (T,)."""
    noise = np.resize(np.asarray(noise, np.float64), ncell)
    tr, s, k = W.synthetic_cells(ix, xyz, ncell, nspots, noise, seed)
    keep = ~((ix.hap_chrom[tr['locus'][tr['trace_ptr'][:-1]]] == missing_chrom) & (k == 1))
    tr = T.check_traces(drop(tr, keep), ix.copy_ptr, ix.hap_chrom)
    return tr, s, k[keep]


def cell_sums(xyz, ix, traces, c):
    cp, ptr = traces['cell_ptr'], traces['trace_ptr']
    locus = np.asarray(traces['locus'], np.int64)
    t0, t1 = int(cp[c]), int(cp[c + 1])
    a, b = int(ptr[t0]), int(ptr[t1])
    p = np.asarray(traces['position'][a:b], np.float64)
    q = p - p.mean(axis=0)
    o = np.asarray(xyz[TA.beads_of(ix, locus[a], 0)], np.float64)  # (S, 3)
    nt, S = t1 - t0, xyz.shape[1]
    ncopy = np.diff(ix.copy_ptr)[locus[ptr[t0:t1]]]
    cmax = int(ncopy.max())
    r = {'n_t': np.diff(ptr[t0:t1 + 1]).astype(np.float64), 'sq': np.zeros((nt, 3)), 'sqq': np.zeros(nt),
         'ncopy': ncopy, 'chrom': np.asarray(ix.hap_chrom)[locus[ptr[t0:t1]]],
         'sx': np.zeros((nt, cmax, S, 3)), 'sxx': np.full((nt, cmax, S), np.inf), 'm': np.zeros((nt, cmax, S, 3, 3))}
    for j in range(nt):
        i0, i1 = int(ptr[t0 + j]) - a, int(ptr[t0 + j + 1]) - a
        qt = q[i0:i1]
        r['sq'][j], r['sqq'][j] = qt.sum(axis=0), np.sum(qt * qt)
        for k in range(int(ncopy[j])):
            x = np.asarray(xyz[TA.beads_of(ix, locus[a + i0:a + i1], k)], np.float64) - o[None]  # (n, S, 3)
            r['sx'][j, k] = x.sum(axis=0)
            r['sxx'][j, k] = np.sum(x * x, axis=(0, 2))
            r['m'][j, k] = np.einsum('na,nsb->sab', qt, x)
    r['Ga'], r['n'] = float(r['sqq'].sum()), float(r['n_t'].sum())
    # the chromosomes of the cell in order of first appearance, each with its traces in cell order
    r['groups'] = [np.where(r['chrom'] == ch)[0] for ch in dict.fromkeys(r['chrom'].tolist())]
    return r


def joint(r, L, s=None):
    """(cost, R, tau, scale) of the labelling L (nt,) on structure s, or on all structures
    (arrays over S) when s is None"""
    j = np.arange(len(L))
    sl = slice(None) if s is None else slice(s, s + 1)
    SX, SXX, M = r['sx'][j, L][:, sl].sum(axis=0), r['sxx'][j, L][:, sl].sum(axis=0), r['m'][j, L][:, sl].sum(axis=0)
    n = r['n']
    Gb = np.maximum(0.0, SXX - np.sum(SX * SX, axis=1) / n)
    U, sv, Vt = np.linalg.svd(M.transpose(0, 2, 1))  # x ~ R q
    d = np.where(np.linalg.det(U) * np.linalg.det(Vt) < 0.0, -1.0, 1.0)
    lam = sv[:, 0] + sv[:, 1] + d * sv[:, 2]
    D = np.zeros((len(d), 3, 3))
    D[:, 0, 0] = D[:, 1, 1] = 1.0
    D[:, 2, 2] = d
    R = U @ D @ Vt
    cost, scale = np.sqrt(np.maximum(0.0, (r['Ga'] + Gb - 2.0 * lam) / n)), (r['Ga'] + Gb) / n
    if s is None:
        return cost, R, SX / n, scale
    return float(cost[0]), R[0], SX[0] / n, float(scale[0])


def residuals(r, s, R, tau):
    """r(t, k) under the motion (R, tau); +inf where k >= C_t"""
    out = (r['sqq'][:, None] + r['sxx'][:, :, s] + r['n_t'][:, None] * (tau @ tau) +
           2.0 * (r['sq'] @ R.T @ tau)[:, None] - 2.0 * r['sx'][:, :, s] @ tau -
           2.0 * np.einsum('ba,tkab->tk', R, r['m'][:, :, s]))
    return out


def independent(r, s):
    """e(t, k): the trace's own centred Kabsch from the same sums (Horn's key matrix, eigh)"""
    n = r['n_t'][:, None]
    sx, sxx, m = r['sx'][:, :, s], r['sxx'][:, :, s], r['m'][:, :, s]
    ga = (r['sqq'] - np.sum(r['sq'] ** 2, axis=1) / r['n_t'])[:, None]
    gb = sxx - np.sum(sx * sx, axis=2) / n
    m = m - r['sq'][:, None, :, None] * sx[:, :, None, :] / n[:, :, None, None]
    N = np.zeros(m.shape[:2] + (4, 4))
    N[..., 0, 0] = m[..., 0, 0] + m[..., 1, 1] + m[..., 2, 2]
    N[..., 1, 1] = m[..., 0, 0] - m[..., 1, 1] - m[..., 2, 2]
    N[..., 2, 2] = -m[..., 0, 0] + m[..., 1, 1] - m[..., 2, 2]
    N[..., 3, 3] = -m[..., 0, 0] - m[..., 1, 1] + m[..., 2, 2]
    N[..., 0, 1] = N[..., 1, 0] = m[..., 1, 2] - m[..., 2, 1]
    N[..., 0, 2] = N[..., 2, 0] = m[..., 2, 0] - m[..., 0, 2]
    N[..., 0, 3] = N[..., 3, 0] = m[..., 0, 1] - m[..., 1, 0]
    N[..., 1, 2] = N[..., 2, 1] = m[..., 0, 1] + m[..., 1, 0]
    N[..., 1, 3] = N[..., 3, 1] = m[..., 2, 0] + m[..., 0, 2]
    N[..., 2, 3] = N[..., 3, 2] = m[..., 1, 2] + m[..., 2, 1]
    ok = np.isfinite(sxx)
    lam = np.linalg.eigvalsh(N)[..., 3]
    return np.where(ok, np.maximum(0.0, ga + np.where(ok, gb, 0.0) - 2.0 * lam), np.inf)


def labellings(m, C):
    """the injective labellings of m traces on C copies in lexicographic order"""
    return list(itertools.permutations(range(C), m))


def choose(table, members, C, r, s):
    """(labelling of least sum -- first minimum in lexicographic order --, its sum, the sums of
    all labellings, the decision margin)"""
    labs = labellings(len(members), C)
    sums = []
    for lab in labs:
        v = 0.0
        for t, k in zip(members, lab):
            v = v + table[t, k]
        sums.append(v)
    sums = np.asarray(sums)
    b = int(np.argmin(sums))
    if len(labs) < 2:
        return labs[b], sums[b], labs, sums, np.inf
    scale = sum(r['sqq'][t] + r['sxx'][t, k, s] for t, k in zip(members, labs[b]))
    two = np.partition(sums, 1)[:2]
    return labs[b], sums[b], labs, sums, float((two[1] - two[0]) / scale)


def search(r, s):
    """{'cost', 'scale', 'label' (nt,), 'rounds', 'fixed', 'costs': the joint cost after every
    fit, 'margins': of every choice made}"""
    nt = len(r['n_t'])
    L = np.zeros(nt, np.int64)
    margins, costs = [], []
    e = independent(r, s)
    for g in r['groups']:
        lab, _, _, _, mg = choose(e, g, int(r['ncopy'][g[0]]), r, s)
        L[g] = lab
        margins.append(mg)
    rounds, fixed = 0, False
    while True:
        cost, R, tau, scale = joint(r, L, s)
        costs.append(cost)
        if rounds == ROUNDS:
            break
        rounds += 1
        res = residuals(r, s, R, tau)
        moved = False
        for g in r['groups']:
            lab, best, labs, sums, mg = choose(res, g, int(r['ncopy'][g[0]]), r, s)
            margins.append(mg)
            cur = sums[labs.index(tuple(L[g].tolist()))]
            if best < cur:
                L[g] = lab
                moved = True
        if not moved:
            fixed = True
            break
    return {'cost': cost, 'scale': scale, 'label': L, 'rounds': rounds, 'fixed': fixed, 'costs': costs,
            'margins': np.asarray(margins)}


def all_labellings(r):
    """every labelling of the cell as an (nt,) array"""
    per = [labellings(len(g), int(r['ncopy'][g[0]])) for g in r['groups']]
    for combo in itertools.product(*per):
        L = np.zeros(len(r['n_t']), np.int64)
        for g, lab in zip(r['groups'], combo):
            L[g] = lab
        yield L


def brute(r):
    """(least joint cost over all labellings (S,), the first labelling that reaches it (S, nt))"""
    best, arg = None, None
    for L in all_labellings(r):
        cost = joint(r, L)[0]
        if best is None:
            best, arg = cost.copy(), np.tile(L, (len(cost), 1))
        else:
            better = cost < best
            best[better], arg[better] = cost[better], L
    return best, arg


def cells_oracle(xyz, ix, traces):
    """search() on every (cell, structure): {'cost', 'scale' (Ncell, S) float64, 'label' (T, S),
    'rounds' (Ncell, S), 'fixed' (Ncell, S), 'margin' (Ncell, S): the smallest margin of the
    pair's choices, 'costs': {(c, s): the cost sequence}}"""
    cp = traces['cell_ptr']
    nc, S, T_ = len(cp) - 1, xyz.shape[1], int(cp[-1])
    out = {'cost': np.zeros((nc, S)), 'scale': np.zeros((nc, S)), 'label': np.zeros((T_, S), np.int64),
           'rounds': np.zeros((nc, S), np.int64), 'fixed': np.zeros((nc, S), bool), 'margin': np.zeros((nc, S)),
           'costs': {}, 'nmargins': 0}
    for c in range(nc):
        r = cell_sums(xyz, ix, traces, c)
        for s in range(S):
            q = search(r, s)
            out['cost'][c, s], out['scale'][c, s] = q['cost'], q['scale']
            out['label'][cp[c]:cp[c + 1], s] = q['label']
            out['rounds'][c, s], out['fixed'][c, s] = q['rounds'], q['fixed']
            out['margin'][c, s] = q['margins'].min()
            out['nmargins'] += int(np.count_nonzero(np.isfinite(q['margins'])))
            out['costs'][(c, s)] = q['costs']
    return out


def select(cost, label, cell_ptr, keep_best):
    """the keep_best rule on an f32 cost (Ncell, S): (best_struct, best_cost, best_label (T, kb))"""
    cost = np.asarray(cost, np.float32)
    order = np.argsort(cost, axis=1, kind='stable')[:, :keep_best]
    cell = np.repeat(np.arange(len(cell_ptr) - 1), np.diff(cell_ptr))
    return (order.astype(np.int32), np.take_along_axis(cost, order, axis=1),
            np.take_along_axis(np.asarray(label), order[cell], axis=1).astype(np.uint8))


def cpu_cells(store, traces, keep_best, device):
    CALLS.append(len(traces['cell_ptr']) - 1)
    o = cells_oracle(np.asarray(store.coordinates()), store, traces)
    return select(o['cost'].astype(np.float32), o['label'], traces['cell_ptr'], keep_best)


def register_cpu_kernels():
    """optimization/kernel = 'tracing_cells_test': the kernels of 'tracing_assign_test' with the
    oracle above as 'tracing_assign_cells'"""
    from igm_amd import steps as ST
    TA.register_cpu_kernels()
    ST.KERNELS['tracing_cells_test'] = dict(ST.KERNELS['tracing_assign_test'], tracing_assign_cells=cpu_cells)
