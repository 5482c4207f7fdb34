"""Plain NumPy / scipy dense restatement of the Hi-C report step (igm_amd.report.hic_*,
include/igm_hip.h igm_report_hic): x and y are built dense, the masks taken, and
scipy.stats.pearsonr and np.histogram2d called on float64 -- what report_hic
(igm/report/hic.py) does through alabtools, with this project's reading of the parts
alabtools hides (symmetric matrices with their diagonal, the clip to [0, 1], '<=' in the
contact test).  Small inputs only: everything is dense.  Also the integer statistics of the
entry point, an exact rational r, and the dense contact count of the end-to-end case.
"""
import warnings
from fractions import Fraction
from math import isqrt

import numpy as np

MASKS = ('all', 'restrained', 'non_restrained')

# The largest distance of scipy.stats.pearsonr (float64) from the exactly rounded r (exact_r)
# over synthetic_cases(), measured on the CPU: 4 * 2^-53 = 4.44e-16
# (test_report_hic.py::test_scipy_distance_is_the_recorded_one re-measures it).  The kernels
# are held to 4 times that -- scipy sums the same centred products in float64 in another
# order, so its error is the right scale and 4x covers the order effects -- and never to
# less than 8 * 2^-53, which covers the final divide, square root and rounding.
SCIPY_DISTANCE = 4 * 2.0 ** -53
CORRELATION_BAR = max(4 * SCIPY_DISTANCE, 8 * 2.0 ** -53)  # = 16 * 2^-53 = 1.78e-15


def dense_input(matrix, nhap=None):
    """the symmetric float32 matrix of a read_hcs dict (upper triangle stored)"""
    indptr = np.asarray(matrix['indptr'], np.int64)
    n = len(indptr) - 1 if nhap is None else nhap
    rows = np.repeat(np.arange(n), np.diff(indptr))
    cols = np.asarray(matrix['indices'])[:indptr[-1]]
    up = np.zeros((n, n), np.float32)
    up[rows, cols] = np.asarray(matrix['data'], np.float32)[:indptr[-1]]
    return np.where(np.arange(n)[:, None] <= np.arange(n)[None, :], up, up.T)


def sub_matrix(matrix, loci):
    """the read_hcs dict of the sub-matrix on the (ascending) loci"""
    loci = np.asarray(loci)
    assert np.all(np.diff(loci) > 0)
    new = np.full(len(matrix['indptr']) - 1, -1, np.int64)
    new[loci] = np.arange(len(loci))
    indptr, indices, data = [0], [], []
    for a in loci:
        lo, hi = matrix['indptr'][a], matrix['indptr'][a + 1]
        c = new[matrix['indices'][lo:hi]]
        indices.append(c[c >= 0])
        data.append(matrix['data'][lo:hi][c >= 0])
        indptr.append(indptr[-1] + int((c >= 0).sum()))
    return {'indptr': np.array(indptr, np.int64), 'indices': np.concatenate(indices).astype(np.int32),
            'data': np.concatenate(data).astype(np.float32)}


def contact_counts(xyz, radii, contact_range, copy_ptr, copy_idx):
    """(nhap, nhap) int32: the structures with |x_i - x_j| (float32 norm) <= fl32(contact_range
    * fl32(r_i + r_j)), summed over the copies -- igm_contact_map_haploid in NumPy"""
    xyz = np.asarray(xyz, np.float32)
    n = xyz.shape[0]
    d = xyz[:, None] - xyz[None, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    bound = np.float32(contact_range) * (radii[:, None] + radii[None, :]).astype(np.float32)
    full = (np.sqrt(d2) <= bound[:, :, None]).sum(axis=2)
    hap_of = np.empty(n, np.int64)
    for a in range(len(copy_ptr) - 1):
        hap_of[copy_idx[copy_ptr[a]:copy_ptr[a + 1]]] = a
    out = np.zeros((len(copy_ptr) - 1,) * 2, np.int64)
    np.add.at(out, (hap_of[:, None], hap_of[None, :]), full)
    return out.astype(np.int32)


def sub_population(pop, loci):
    """The population of the haploid loci `loci` in the layout alabtools writes: beads
    0..n-1 are the first copies in locus order, the further copies follow."""
    cp, ci = pop['copy_ptr'], pop['copy_idx']
    beads, chrom, copy, rows = [], [], [], [[] for _ in loci]
    for k in range(int(np.diff(cp).max())):
        for q, h in enumerate(loci):
            if cp[h + 1] - cp[h] > k:
                rows[q].append(len(beads))
                beads.append(ci[cp[h] + k])
                chrom.append(pop['hap_chrom'][h])
                copy.append(k)
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    idx = np.array([b for r in rows for b in r], np.int32)
    beads = np.array(beads)
    return {'coordinates': np.ascontiguousarray(pop['coordinates'][beads]), 'radii': pop['radii'][beads],
            'chrom': np.array(chrom, np.int32), 'copy': np.array(copy, np.int32), 'copy_ptr': ptr, 'copy_idx': idx,
            'hap_chrom': np.asarray(pop['hap_chrom'])[loci].astype(np.int32)}


def probabilities(counts, nstruct):
    """y: counts / nstruct clipped to [0, 1], float64"""
    return np.clip(np.asarray(counts, np.int64), 0, nstruct) / np.float64(nstruct)


def populations(hap_chrom, nchrom=None):
    """boolean masks of the nchrom + 1 populations on the dense matrix: a chromosome's full
    block, then the inter pairs a < b"""
    hc = np.asarray(hap_chrom)
    nchrom = int(hc.max()) + 1 if nchrom is None else nchrom
    same = hc[:, None] == hc[None, :]
    pops = [same & (hc[:, None] == c) for c in range(nchrom)]
    pops.append(np.triu(~same))
    return pops


def _given(s):
    return s is not None and s > 0


def selections(x, hap_chrom, intra_sigma, inter_sigma, nchrom=None):
    """[(population, mask name, boolean selection or None when the sigma is not given)];
    x >= sigma is decided on the float32 input widened to float64"""
    x = np.asarray(x).astype(np.float64)
    pops = populations(hap_chrom, nchrom)
    out = []
    for p, pm in enumerate(pops):
        sig = inter_sigma if p == len(pops) - 1 else intra_sigma
        out.append((p, 'all', pm))
        out.append((p, 'restrained', pm & (x >= sig) if _given(sig) else None))
        out.append((p, 'non_restrained', pm & ~(x >= sig) if _given(sig) else None))
    return out


def pearson(x, y):
    """scipy's r on float64; NaN for fewer than 2 entries or a constant side"""
    from scipy.stats import pearsonr
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if len(x) < 2 or np.all(x == x[0]) or np.all(y == y[0]):
        return float('nan')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return float(pearsonr(x, y)[0])


def exact_r2(x, y):
    """(sign, r^2 as a Fraction) of the float64 vectors, or None when r is undefined"""
    fx, fy = [Fraction(float(v)) for v in x], [Fraction(float(v)) for v in y]
    n = len(fx)
    if n < 2:
        return None
    sx, sy = sum(fx), sum(fy)
    cxy = n * sum(a * b for a, b in zip(fx, fy)) - sx * sy
    vx = n * sum(a * a for a in fx) - sx * sx
    vy = n * sum(b * b for b in fy) - sy * sy
    if vx == 0 or vy == 0:
        return None
    return (cxy > 0) - (cxy < 0), cxy * cxy / (vx * vy)


def sqrt_fraction(q, bits=200):
    """sqrt of a non-negative Fraction rounded to float64: the integer square root of the
    fraction scaled by 4^bits carries `bits` correct bits"""
    if q == 0:
        return 0.0
    num = isqrt((q.numerator << (2 * bits)) // q.denominator)
    return float(Fraction(num, 1 << bits))


def exact_r(x, y):
    """Pearson r from exact rational arithmetic: r^2 exact, one square root"""
    e = exact_r2(x, y)
    if e is None:
        return float('nan')
    return e[0] * sqrt_fraction(e[1])


def correlations(x, y, hap_chrom, intra_sigma, inter_sigma, r=pearson, nchrom=None):
    """{'intra': {mask: (nchrom,)}, 'inter': {mask: float}} on dense x (float32 or float64)
    and y, with r the correlation function (pearson or exact_r)"""
    x64 = np.asarray(x).astype(np.float64)
    sel = selections(x, hap_chrom, intra_sigma, inter_sigma, nchrom)
    P = len(sel) // 3
    val = np.full((P, 3), np.nan)
    for k, (p, _, s) in enumerate(sel):
        if s is not None:
            val[p, k % 3] = r(x64[s], y[s])
    return {'intra': {m: val[:-1, k].copy() for k, m in enumerate(MASKS)},
            'inter': {m: float(val[-1, k]) for k, m in enumerate(MASKS)}}


def histogram(x, y, edges_x, edges_y):
    """np.histogram2d(y, x, bins=(edges_y, edges_x)) over the whole dense matrices: int64
    (ny, nx), rows = output, columns = input"""
    h = np.histogram2d(np.asarray(y, np.float64).ravel(), np.asarray(x).astype(np.float64).ravel(),
                       bins=(edges_y, edges_x))[0]
    assert np.array_equal(h, np.rint(h))
    return h.astype(np.int64)


def integer_statistics(counts, nstruct, x, hap_chrom, intra_sigma, inter_sigma, stored, nchrom=None):
    """(n, dense_sums (P, 2), sparse_ints (P, 2, 3)) of igm_report_hic from dense arrays;
    stored: the boolean symmetric mask of the entries the CSR stores"""
    c = np.clip(np.asarray(counts, np.int64), 0, nstruct)
    x = np.asarray(x).astype(np.float64)
    pops = populations(hap_chrom, nchrom)
    P = len(pops)
    n = np.array([int(pm.sum()) for pm in pops], np.int64)
    dense = np.array([[int(c[pm].sum()), int((c[pm] * c[pm]).sum())] for pm in pops], np.int64)
    sparse = np.zeros((P, 2, 3), np.int64)
    for p, pm in enumerate(pops):
        sig = inter_sigma if p == P - 1 else intra_sigma
        ge = (x >= sig) if _given(sig) else np.zeros_like(pm)
        for h, half in enumerate((ge, ~ge)):
            s = pm & stored & half
            sparse[p, h] = [int(s.sum()), int(c[s].sum()), int((c[s] * c[s]).sum())]
    return n, dense, sparse


def stored_mask(matrix, nhap=None):
    indptr = np.asarray(matrix['indptr'], np.int64)
    n = len(indptr) - 1 if nhap is None else nhap
    rows = np.repeat(np.arange(n), np.diff(indptr))
    m = np.zeros((n, n), bool)
    m[rows, np.asarray(matrix['indices'])[:indptr[-1]]] = True
    return m | m.T


def statistics(counts, nstruct, matrix, hap_chrom, intra_sigma=None, inter_sigma=None, log_edges=None,
               lin_edges=None, nchrom=None):
    """The dict igm_amd.report.hic_statistics returns, from dense NumPy arrays: the integer
    statistics exactly, the float64 ones with np.sum in place of the kernel's fixed order"""
    hc = np.asarray(hap_chrom)
    x = dense_input(matrix, len(hc)).astype(np.float64)
    st = stored_mask(matrix, len(hc))
    c = np.clip(np.asarray(counts, np.int64), 0, nstruct)
    y = c / np.float64(nstruct)
    intra_sigma = intra_sigma if _given(intra_sigma) else None
    inter_sigma = inter_sigma if _given(inter_sigma) else None
    n, dense, sparse = integer_statistics(counts, nstruct, x, hc, intra_sigma, inter_sigma, st, nchrom)
    pops = populations(hc, nchrom)
    P = len(pops)
    sumx, means, cent = np.zeros((P, 2)), np.zeros((P, 3, 2)), np.zeros((P, 3, 2))
    for p, pm in enumerate(pops):
        sig = inter_sigma if p == P - 1 else intra_sigma
        ge = (x >= sig) if sig is not None else np.zeros_like(pm)
        sumx[p] = [x[pm & st & ge].sum(), x[pm & st & ~ge].sum()]
        w0 = int(sparse[p, 0, 0])
        ns = (int(n[p]), w0, int(n[p]) - w0)
        sc = (int(dense[p, 0]), int(sparse[p, 0, 1]), int(dense[p, 0] - sparse[p, 0, 1]))
        sx = (sumx[p, 0] + sumx[p, 1], sumx[p, 0], sumx[p, 1])
        for m, sel in enumerate((pm & st, pm & st & ge, pm & st & ~ge)):
            if ns[m] > 0:
                means[p, m] = [float(Fraction(sc[m], ns[m] * nstruct)), sx[m] / ns[m]]
            cent[p, m] = [(x[sel] * (y[sel] - means[p, m, 0])).sum(),
                          ((x[sel] - means[p, m, 1]) * (x[sel] - means[p, m, 1])).sum()]
    hist = [None if e is None else histogram(x, y, e, e) for e in (log_edges, lin_edges)]
    return {'n': n, 'dense_sums': dense, 'sparse_ints': sparse, 'sparse_sumx': sumx, 'means': means, 'centred': cent,
            'log_hist': hist[0], 'lin_hist': hist[1], 'nstruct': int(nstruct), 'intra_sigma': intra_sigma,
            'inter_sigma': inter_sigma}


# ------------------------------------------------------------------ hand-made cases
def csr_from_dense(up, stored):
    """read_hcs dict of the entries `stored` (boolean, upper triangle) of the float32 `up`"""
    n = up.shape[0]
    stored = np.triu(stored)
    indptr = np.concatenate([[0], np.cumsum(stored.sum(axis=1))]).astype(np.int64)
    rows, cols = np.nonzero(stored)
    return {'indptr': indptr, 'indices': cols.astype(np.int32), 'data': up[rows, cols].astype(np.float32)}


def synthetic_case(sizes, nstruct, seed, ids=None, density=0.6, over=1.1, intra_sigma=None, inter_sigma=None,
                   specials=False):
    """Hand-made symmetric counts in [0, over * nstruct] and an input matrix with about
    `density` of its upper triangle stored.  ids: the chromosome id of each block (default
    0, 1, ..).  specials (nhap >= 130, nstruct = 1000): row 1 fully stored (129 entries),
    row 2 without any, stored diagonal entries, stored zeros, x equal to each sigma,
    x = float32(1e-3) and the float32 just below it, y exactly 1e-3 and exactly 1."""
    rng = np.random.default_rng(seed)
    ids = list(range(len(sizes))) if ids is None else ids
    hc = np.repeat(np.asarray(ids, np.int32), sizes)
    n = len(hc)
    c = rng.integers(0, int(over * nstruct) + 1, (n, n))
    c = np.triu(c) + np.triu(c, 1).T
    same = hc[:, None] == hc[None, :]
    up = np.triu(np.where(same, rng.uniform(0.0, 1.0, (n, n)), rng.uniform(0.0, 0.08, (n, n)))).astype(np.float32)
    stored = np.triu(rng.uniform(size=(n, n)) < density, 1)
    stored[np.arange(n), np.arange(n)] = rng.uniform(size=n) < 0.3
    if specials:
        assert n >= 130 and nstruct == 1000
        stored[1, 1:] = True
        stored[2, 2:] = False
        stored[5, 5] = stored[6, 6] = True
        up[7, 9] = up[8, 120] = 0.0          # stored explicit zeros, intra and inter
        stored[7, 9] = stored[8, 120] = True
        up[3, 4], up[3, 100] = intra_sigma, inter_sigma  # x == sigma: restrained
        up[4, 6], up[4, 101] = np.float32(1e-3), np.nextafter(np.float32(1e-3), np.float32(0))
        stored[3, 4] = stored[3, 100] = stored[4, 6] = stored[4, 101] = True
        c[3, 4] = c[4, 3] = 1                # y == 1e-3: the first edge
        c[4, 6] = c[6, 4] = 1000             # y == 1: the closed last bin
        c[3, 100] = c[100, 3] = 1000
        c[4, 101] = c[101, 4] = 500
    return {'counts': np.ascontiguousarray(c, np.int32), 'nstruct': nstruct, 'matrix': csr_from_dense(up, stored),
            'hap_chrom': hc, 'nchrom': int(max(ids)) + 1, 'intra_sigma': intra_sigma, 'inter_sigma': inter_sigma}


def synthetic_cases():
    """name -> case: nhap in {1, 2, 63, 65, 130}, one-locus chromosomes, odd nhap, blocks off
    every tile and wave edge, nstruct 1 and 50 000, a sigma absent on one side and on both"""
    return {
        'n1': synthetic_case((1,), 1, 1, density=1.0, intra_sigma=0.5, inter_sigma=0.02),
        'n2': synthetic_case((1, 1), 3, 2, density=1.0, intra_sigma=0.5, inter_sigma=0.02),
        'n2_one_chrom': synthetic_case((2,), 5, 3, density=1.0, intra_sigma=0.5, inter_sigma=0.02),
        'n63': synthetic_case((1, 2, 60), 7, 4, intra_sigma=0.3, inter_sigma=0.02),
        'n63_nstruct1': synthetic_case((1, 2, 60), 1, 5, over=2.0, intra_sigma=0.3, inter_sigma=0.02),
        'n63_no_sigma': synthetic_case((1, 2, 60), 7, 4),
        'n65_big': synthetic_case((1, 64), 50000, 6, over=1.0, intra_sigma=0.4),
        'n65_no_intra': synthetic_case((1, 64), 33, 7, inter_sigma=0.04),
        'n130': synthetic_case((3, 61, 66), 1000, 8, ids=(5, 0, 2), intra_sigma=0.0625, inter_sigma=0.03125,
                               specials=True),
    }


def case_xy(case):
    x = dense_input(case['matrix'], len(case['hap_chrom']))
    return x, probabilities(case['counts'], case['nstruct'])
