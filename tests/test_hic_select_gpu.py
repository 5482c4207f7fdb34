"""igm_hic_select on the MI355X at its edges.

The selection is expected from oracle.hic_select (pinned to the reference's own selection in
test_mstep_oracle.py) and from a NumPy restatement that also supplies the order of the output
(inter rows in file order, then intra rows in file order), r0 = float32(cr * float64(float32(
r_i + r_j))), k and the class.  Everything is exact: every comparison is equality of bits."""
import ctypes

import numpy as np
import pytest

import oracle
from igm_amd._lib import IGM_DEVICE_PTRS, IGM_OK, bond_dtype, row_dtype

pytestmark = pytest.mark.gpu

NATOM = 40
CHROM = np.repeat([0, 1, 2], [15, 13, 12]).astype(np.int32)


@pytest.fixture(scope='module')
def ctx():
    from igm_amd import _lib
    return _lib.context(0)


# ---------------------------------------------------------------- restatement
def norms(xyz, row, col):
    """(S, n) float32 norm of the float32 difference (particle.py:35-36): float32 squares, sum and
    square root, as the header of hic_select.hip states it"""
    d = (xyz[:, row] - xyz[:, col]).astype(np.float32)
    d2 = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(np.float32) + d[..., 2] * d[..., 2]).astype(np.float32)
    return np.sqrt(d2).astype(np.float32)


def select_ref(xyz, chrom, act):
    """(S, n) uint8 like oracle.hic_select: 1 inter bond, 2 intra bond, 0 not selected"""
    near = norms(xyz, act['row'], act['col']) <= act['dist'][None, :]
    inter = chrom[act['row']] != chrom[act['col']]
    return np.where(near, np.where(inter, 1, 2)[None, :], 0).astype(np.uint8)


def expected(sel, radii, act, cr, kspring, classes=(1, 2)):
    """CSR (ptr, bonds, class) of a selection (S, n): per structure the inter rows in file order,
    then the intra rows in file order"""
    ptr, bonds, cls = [0], [], []
    for s in range(len(sel)):
        for code in (1, 2):
            q = np.nonzero(sel[s] == code)[0]
            b = np.zeros(len(q), bond_dtype)
            b['i'], b['j'] = act['row'][q], act['col'][q]
            rs = (radii[act['row'][q]] + radii[act['col'][q]]).astype(np.float32)
            b['r0'] = (np.float64(cr) * rs.astype(np.float64)).astype(np.float32)
            b['k'] = np.float32(kspring)
            bonds.append(b)
            cls.append(np.full(len(q), classes[code - 1], np.int32))
        ptr.append(ptr[-1] + len(bonds[-1]) + len(bonds[-2]))
    return np.array(ptr, np.int64), np.concatenate(bonds), np.concatenate(cls)


# ---------------------------------------------------------------- the call
def gpu_select(ctx, xyz, radii, chrom, act, cr=2.0, kspring=1.0, classes=(1, 2), with_class=True):
    """count-only call, then the filling call: (ptr, bonds, class or None); asserts that both
    calls report the same CSR pointer and the same total"""
    S, N = xyz.shape[0], xyz.shape[1]
    assert xyz.dtype == np.float32 and xyz.flags['C_CONTIGUOUS'] and act.dtype == row_dtype
    assert len(act) == 0 or (act['row'].min() >= 0 and act['col'].min() >= 0 and
                             max(act['row'].max(), act['col'].max()) < N)
    ptr0 = np.full(S + 1, -1, np.int64)
    tot0 = ctypes.c_int64(-1)
    args = [ctx.h, 0, S, N, xyz.ctypes.data, radii.ctypes.data, chrom.ctypes.data,
            act.ctypes.data if len(act) else None, len(act), float(cr), float(kspring), classes[0], classes[1]]
    rc = ctx.lib.igm_hic_select(*(args + [ptr0.ctypes.data, None, None, ctypes.byref(tot0)]))
    ctx.check(rc, 'igm_hic_select (count)')
    n = tot0.value
    assert n == ptr0[-1] and ptr0[0] == 0 and np.all(np.diff(ptr0) >= 0)
    bonds = np.zeros(n + 1, bond_dtype)
    bonds[n]['i'] = 0xdeadbeef  # one record past the end: must stay
    cls = np.full(n + 1, -7, np.int32)
    ptr = np.full(S + 1, -1, np.int64)
    tot = ctypes.c_int64(-1)
    rc = ctx.lib.igm_hic_select(*(args + [ptr.ctypes.data, bonds.ctypes.data, cls.ctypes.data if with_class else None,
                                          ctypes.byref(tot)]))
    ctx.check(rc, 'igm_hic_select (fill)')
    assert tot.value == n and np.array_equal(ptr, ptr0)
    assert bonds[n]['i'] == 0xdeadbeef and cls[n] == -7
    return ptr, bonds[:n], (cls[:n] if with_class else None)


def check(ctx, xyz, radii, chrom, act, sel, **kw):
    ptr, bonds, cls = gpu_select(ctx, xyz, radii, chrom, act, **kw)
    eptr, ebonds, ecls = expected(sel, radii, act, kw.get('cr', 2.0), kw.get('kspring', 1.0), kw.get('classes', (1, 2)))
    assert np.array_equal(ptr, eptr)
    assert bonds.tobytes() == ebonds.tobytes()
    if cls is not None:
        assert np.array_equal(cls, ecls)
    return ptr


# ---------------------------------------------------------------- models
def model(S, seed=0):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-8000.0, 8000.0, (S, NATOM, 3)).astype(np.float32)
    radii = rng.uniform(50.0, 250.0, NATOM).astype(np.float32)
    return xyz, radii


def rows(xyz, n, seed, kind='any'):
    """n activation rows: unsorted, some with row > col, a tenth duplicated; the distance is the
    pair's own distance in a random structure times U(0.7, 1.3), so about half of the structures
    select a row"""
    rng = np.random.default_rng(seed)
    act = np.zeros(n, row_dtype)
    if n == 0:
        return act
    i = rng.integers(0, NATOM, n)
    j = (i + rng.integers(1, NATOM, n)) % NATOM
    if kind != 'any':
        pairs = np.array([(a, b) for a in range(NATOM) for b in range(NATOM)
                          if a != b and (CHROM[a] != CHROM[b]) == (kind == 'inter')])
        i, j = pairs[rng.integers(0, len(pairs), n)].T
    act['row'], act['col'] = i, j
    d = norms(xyz, i, j)[rng.integers(0, len(xyz), n), np.arange(n)]
    act['dist'] = d * rng.uniform(0.7, 1.3, n).astype(np.float32)
    act['prob'] = rng.random(n)
    dup = rng.random(n) < 0.1
    act[dup] = act[rng.integers(0, n, n)][dup]
    return act


def both_refs(xyz, act):
    sel = select_ref(xyz, CHROM, act)
    assert np.array_equal(sel, oracle.hic_select(xyz, CHROM, act['row'], act['col'], act['dist']))
    return sel


@pytest.fixture(scope='module')
def models():
    return {S: model(S, S) for S in (1, 3, 70)}


# ---------------------------------------------------------------- igm_hic_select
@pytest.mark.parametrize('S', [1, 3, 70])
@pytest.mark.parametrize('n_act', [0, 1, 255, 256, 257, 1023, 1024, 1025, 2048, 3000])
def test_gpu_hic_select_row_counts(ctx, models, n_act, S):
    """row counts around the 256-thread and the 1024-row block edges, zero rows included"""
    xyz, radii = models[S]
    act = rows(xyz, n_act, 1000 + n_act)
    sel = both_refs(xyz, act)
    ptr = check(ctx, xyz, radii, CHROM, act, sel)
    if n_act >= 255:
        assert np.any(act['row'] > act['col']) and np.any(act['row'] < act['col'])
        assert 0.2 * n_act * S < ptr[-1] < 0.8 * n_act * S
        key = (act['row'].astype(np.int64) * NATOM + act['col']) << 32 | act['dist'].view(np.uint32)
        assert len(np.unique(key)) < n_act  # duplicated rows


def test_gpu_hic_select_boundary_rows(ctx, models):
    """rows whose distance is exactly the float32 norm of the pair in structure 1 (selected there)
    or the next float32 below it (not selected there)"""
    xyz, radii = models[3]
    act = rows(xyz, 1200, 7)
    d = norms(xyz, act['row'], act['col'])[1]
    on, below = np.arange(0, 1200, 4), np.arange(1, 1200, 4)
    act['dist'][on] = d[on]
    act['dist'][below] = np.nextafter(d[below], np.float32(0))
    # the square root rounds: the squared distance is not the square of the norm
    dd = (xyz[1, act['row']] - xyz[1, act['col']]).astype(np.float64)
    assert np.count_nonzero((dd * dd).sum(1) != d.astype(np.float64) ** 2) > 0.9 * len(d)
    sel_o = oracle.hic_select(xyz, CHROM, act['row'], act['col'], act['dist'])
    sel_r = select_ref(xyz, CHROM, act)
    assert len(on) >= 50 and len(below) >= 50
    assert np.all(sel_o[1, on] > 0) and np.all(sel_o[1, below] == 0)
    assert np.array_equal(sel_o, sel_r)
    check(ctx, xyz, radii, CHROM, act, sel_r)


@pytest.mark.parametrize('kind', ['inter', 'intra'])
def test_gpu_hic_select_one_kind_only(ctx, models, kind):
    xyz, radii = models[3]
    act = rows(xyz, 1500, 11, kind)
    sel = both_refs(xyz, act)
    assert set(np.unique(sel)) == {0, 1 if kind == 'inter' else 2}
    check(ctx, xyz, radii, CHROM, act, sel)


def test_gpu_hic_select_empty_structures(ctx):
    """structures that select nothing (first, middle, last): ptr[s] == ptr[s + 1]"""
    xyz, radii = model(5, 21)
    act = rows(xyz[[1, 3]], 1300, 22)
    xyz[[0, 2, 4]] *= np.float32(1e3)
    sel = both_refs(xyz, act)
    ptr = check(ctx, xyz, radii, CHROM, act, sel)
    n = np.diff(ptr)
    assert n[0] == n[2] == n[4] == 0 and n[1] > 100 and n[3] > 100


def test_gpu_hic_select_every_row_selected(ctx, models):
    xyz, radii = models[3]
    act = rows(xyz, 1025, 31)
    act['dist'] = 1e9
    act['dist'][::7] = np.inf
    sel = both_refs(xyz, act)
    assert np.all(sel > 0)
    ptr = check(ctx, xyz, radii, CHROM, act, sel)
    assert np.array_equal(np.diff(ptr), [1025] * 3)


def test_gpu_hic_select_contact_range_spring_and_classes(ctx, models):
    """contact range 1.05 (the f64 product rounds to float32), spring 0.5, other class ids"""
    xyz, radii = models[3]
    act = rows(xyz, 1100, 41)
    sel = both_refs(xyz, act)
    check(ctx, xyz, radii, CHROM, act, sel, cr=1.05, kspring=0.5, classes=(5, 9))
    rs = (radii[act['row']] + radii[act['col']]).astype(np.float32)
    assert np.any((1.05 * rs.astype(np.float64)).astype(np.float32) != np.float32(1.05) * rs)  # a float32 product differs


def test_gpu_hic_select_without_class_output(ctx, models):
    xyz, radii = models[3]
    act = rows(xyz, 1100, 51)
    check(ctx, xyz, radii, CHROM, act, both_refs(xyz, act), with_class=False)


def test_gpu_hic_select_device_pointers(ctx, models):
    """torch tensors and IGM_DEVICE_PTRS: the same CSR as the host path"""
    import torch
    xyz, radii = models[70]
    act = rows(xyz, 2048, 61)
    ptr, bonds, cls = gpu_select(ctx, xyz, radii, CHROM, act)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()

    t = [dev(a) for a in (xyz, radii, CHROM, act)]
    dptr = torch.full((71,), -1, dtype=torch.int64, device='cuda')
    n = len(bonds)
    dbonds = torch.zeros((n + 1) * bond_dtype.itemsize, dtype=torch.uint8, device='cuda')
    dcls = torch.full((n + 1,), -7, dtype=torch.int32, device='cuda')
    tot = ctypes.c_int64(-1)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        args = [ctx.h, IGM_DEVICE_PTRS, 70, NATOM, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(),
                len(act), 2.0, 1.0, 1, 2, dptr.data_ptr()]
        assert ctx.lib.igm_hic_select(*(args + [None, None, ctypes.byref(tot)])) == IGM_OK
        assert tot.value == n
        assert ctx.lib.igm_hic_select(*(args + [dbonds.data_ptr(), dcls.data_ptr(), ctypes.byref(tot)])) == IGM_OK
    finally:
        ctx.set_stream(None)
    torch.cuda.synchronize()
    assert tot.value == n and np.array_equal(dptr.cpu().numpy(), ptr)
    assert dbonds.cpu().numpy()[:n * bond_dtype.itemsize].tobytes() == bonds.tobytes()
    assert np.array_equal(dcls.cpu().numpy()[:n], cls) and int(dcls[n]) == -7
