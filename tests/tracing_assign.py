"""Test helper for the chromatin tracing A-step (igm_tracing_assign, igm_amd.tracing).

oracle_rmsd()    the cost in fp64 NumPy, written independently of the library: Kabsch by
                 np.linalg.svd with the determinant correction (Kabsch 1978), batched over the
                 structures.  Returns the (T, S, Cmax) matrix (+inf where k >= C_t) and the scale
                 (Ga + Gb) / n of every entry, which the bound of the GPU tests needs.
bound()          |rmsd_gpu - rmsd_ref| <= 1e-6 rmsd_ref + sqrt(1e-12 (Ga + Gb) / n): the f32
                 rounding of the output, and about 4500 fp64 ulps of the sums that cancel in
                 Ga + Gb - 2 lambda (|a - b| <= sqrt|a^2 - b^2|).
select()         the keep_best rule on an f32 matrix: stable argsort, ties to the lower candidate.
model()          56 beads: chromosome A (12 loci) and B (9 loci) in two copies, C (14 loci) in
                 one; S independent random-walk structures (100 nm steps) whose coordinates are
                 multiples of 1/64 nm, so a trace cut from them, turned by an axis permutation
                 and shifted by whole nm is exact in float32.
chain_model()    one single-copy chromosome of nlocus loci.
traces_of()      trace arrays from [(loci, positions)].
cpu_tracing()    the oracle as the 'tracing_assign' kernel of a Step kernel set;
register_cpu_kernels() registers 'tracing_assign_test' on top of ST.KERNELS['tracing_test'].
"""
import types

import numpy as np

CHROMS = ((0, 12, 2), (1, 9, 2), (2, 14, 1))  # (chromosome, loci, copies)
PERM = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])  # a proper rotation, exact in f32
CALLS = []


def index(chroms=CHROMS):
    """the index of a genome: copy 0 of every chromosome, then the further copies"""
    hap_chrom = np.concatenate([np.full(n, c, np.int32) for c, n, _ in chroms])
    nhap = len(hap_chrom)
    beads = [[] for _ in range(nhap)]
    chrom, copy, b, h0 = [], [], 0, 0
    for k in range(max(c[2] for c in chroms)):
        h0 = 0
        for c, n, nc in chroms:
            if k < nc:
                for h in range(h0, h0 + n):
                    beads[h].append(b)
                    b += 1
                chrom += [c] * n
                copy += [k] * n
            h0 += n
    copy_ptr = np.concatenate([[0], np.cumsum([len(x) for x in beads])]).astype(np.int32)
    copy_idx = np.concatenate(beads).astype(np.int32)
    return types.SimpleNamespace(copy_ptr=copy_ptr, copy_idx=copy_idx, hap_chrom=hap_chrom,
                                 chrom=np.asarray(chrom, np.int32), copy=np.asarray(copy, np.int32), nbead=b)


def random_walks(ix, S, seed, step=100.0):
    """(nbead, S, 3) float32, every (chromosome, copy) an independent random walk from its own
    origin inside a 3 um box; multiples of 1/64 nm"""
    rng = np.random.default_rng(seed)
    xyz = np.zeros((ix.nbead, S, 3))
    key = ix.chrom.astype(np.int64) * 64 + ix.copy
    for q in np.unique(key):
        b = np.where(key == q)[0]
        d = rng.normal(size=(len(b), S, 3))
        d = step * d / np.linalg.norm(d, axis=2, keepdims=True)
        d[0] = rng.uniform(-3000.0, 3000.0, (S, 3))
        xyz[b] = np.cumsum(d, axis=0)
    return (np.round(xyz * 64.0) / 64.0).astype(np.float32)


def model(S, seed=0):
    ix = index()
    return ix, random_walks(ix, S, seed)


def chain_model(nlocus, S, seed=0):
    ix = index(((0, nlocus, 1),))
    return ix, random_walks(ix, S, seed)


def traces_of(items):
    """[(loci, positions (n, 3))] -> {'trace_ptr', 'locus', 'position' float32}"""
    ptr = np.concatenate([[0], np.cumsum([len(l) for l, _ in items])]).astype(np.int64)
    return {'trace_ptr': ptr, 'locus': np.concatenate([np.asarray(l, np.int32) for l, _ in items]),
            'position': np.concatenate([np.asarray(p, np.float64).reshape(-1, 3) for _, p in items]).astype(np.float32)}


def beads_of(ix, loci, k):
    return ix.copy_idx[ix.copy_ptr[np.asarray(loci)] + k]


def oracle_rmsd(xyz, ix, traces):
    """(rmsd (T, S, Cmax) float64, scale (T, S, Cmax) = (Ga + Gb) / n); +inf / 0 where k >= C_t"""
    ptr, locus = traces['trace_ptr'], np.asarray(traces['locus'], np.int64)
    T, S = len(ptr) - 1, xyz.shape[1]
    ncopy = np.diff(ix.copy_ptr)[locus[ptr[:-1]]]
    cmax = int(ncopy.max())
    out = np.full((T, S, cmax), np.inf)
    scale = np.zeros((T, S, cmax))
    for t in range(T):
        a, b = int(ptr[t]), int(ptr[t + 1])
        n = b - a
        p = np.asarray(traces['position'][a:b], np.float64)
        pc = p - p.mean(axis=0)
        ga = np.sum(pc * pc)
        for k in range(int(ncopy[t])):
            x = np.asarray(xyz[beads_of(ix, locus[a:b], k)], np.float64).transpose(1, 0, 2)  # (S, n, 3)
            xc = x - x.mean(axis=1, keepdims=True)
            gb = np.sum(xc * xc, axis=(1, 2))
            H = np.einsum('sna,nb->sab', xc, pc)
            U, sv, Vt = np.linalg.svd(H)
            d = np.where(np.linalg.det(U) * np.linalg.det(Vt) < 0.0, -1.0, 1.0)  # no reflection
            lam = sv[:, 0] + sv[:, 1] + d * sv[:, 2]
            out[t, :, k] = np.sqrt(np.maximum(0.0, ga + gb - 2.0 * lam) / n)
            scale[t, :, k] = (ga + gb) / n
    return out, scale


def noise_floor(scale):
    return np.sqrt(1e-12 * scale)


def bound(ref, scale):
    return 1e-6 * ref + noise_floor(scale)


def select(full, keep_best):
    """(cand (T, kb), value (T, kb)) of an f32 (T, S, Cmax) matrix: stable argsort of every row"""
    flat = np.asarray(full, np.float32).reshape(len(full), -1)
    order = np.argsort(flat, axis=1, kind='stable')[:, :keep_best]
    return order.astype(np.int32), np.take_along_axis(flat, order, axis=1)


def cpu_tracing(store, traces, keep_best, device):
    CALLS.append(len(traces['trace_ptr']) - 1)
    full, _ = oracle_rmsd(np.asarray(store.coordinates()), store, traces)
    return select(full.astype(np.float32), keep_best)


def register_cpu_kernels():
    """optimization/kernel = 'tracing_assign_test': the CPU oracle kernels of tests/tracing.py
    with the oracle above as 'tracing_assign'; RelaxInit without anchors while no assignment
    exists (a run on input_file alone starts as one without tracing)"""
    import cpu_kernels as CK
    import tracing as TR
    from igm_amd import steps as ST
    TR.register_cpu_kernels()
    base = ST.KERNELS['tracing_test']

    def relax(store, sids, cfg, device):
        return (base['relax'] if ST.tracing_assigned(cfg) else CK.relax)(store, sids, cfg, device)
    ST.KERNELS['tracing_assign_test'] = dict(base, tracing_assign=cpu_tracing, relax=relax)
