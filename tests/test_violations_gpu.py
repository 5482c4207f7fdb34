"""igm_mstep_violations and igm_mstep_anchor_violations on the MI355X at their edges: the records
of the reference's own classes on crafted particles (violations_edges_golden.npz), and the NumPy
restatement (tests/violations_ref.py, bit-equal to the reference on the CPU) on small random
models over every bond count, bond source, class table, atom count, batch size and envelope
layout.  Records are integer counts: every comparison is equality."""
import ctypes

import numpy as np
import pytest

import violations_ref as VR
from conftest import load_golden
from igm_amd import model as M
from igm_amd._lib import (IGM_ATOM_BEAD, IGM_ATOM_ENV0, IGM_DEVICE_PTRS, IGM_E_INVALID, IGM_MSTEP_STRUCT_FLAGS,
                          IGM_OK, LOWER_BOUND_BIT, MStepParams, anchor_dtype, bond_dtype)

pytestmark = pytest.mark.gpu

TOL = 0.05
OPT = {'optimization': {'optimizer_options': {'mdsteps': 10, 'tstart': 1, 'tstop': 1}}}
ENVS4 = [((120.0, 120.0, 120.0), 1.0), ((150.0, 100.0, 70.0), -1.0), ((90.0, 110.0, 130.0), 1.0),
         ((200.0, 200.0, 200.0), -1.0)]


@pytest.fixture(scope='module')
def ms():
    from igm_amd import mstep
    return mstep


@pytest.fixture(scope='module')
def ctx():
    from igm_amd import _lib
    return _lib.context(0)


@pytest.fixture(scope='module')
def edges():
    return load_golden('violations_edges_golden.npz')


def params(envelopes=()):
    return M.params_from_cfg(OPT, list(envelopes))


def golden_bonds(g, c, offset=0):
    b = np.zeros(len(g[c + '_i']), bond_dtype)
    b['i'] = g[c + '_i'] + offset
    b['j'] = (g[c + '_j'] + offset).astype(np.uint32) | np.where(g[c + '_lower'], LOWER_BOUND_BIT, np.uint32(0))
    b['r0'], b['k'] = g[c + '_r0'], g[c + '_k']
    return b


# ---------------------------------------------------------------- the reference's records
BOND_CASES = ['up100', 'up300', 'up700', 'up100k', 'up700k', 'lo100', 'lo100k', 'zero_d', 'radii_cr2',
              'radii_cr105']
ENV_CASES = ['sph_k+1', 'sph_k-1', 'ell_k+1', 'ell_k-1']


def test_case_lists_are_the_golden_s(edges):
    assert list(edges['bond_cases']) == BOND_CASES and list(edges['env_cases']) == ENV_CASES


@pytest.mark.parametrize('shared', [True, False])
@pytest.mark.parametrize('case', BOND_CASES)
def test_gpu_bond_record_equals_reference(edges, ms, case, shared):
    g = edges
    x = g[case + '_pos'][None]
    n = x.shape[1]
    b = golden_bonds(g, case)
    flags = np.full(n, IGM_ATOM_BEAD, np.uint32)
    cr = [float(g[case + '_cr'])]
    if shared:
        stats = ms.violations(params(), x, g[case + '_radii'], flags, b, None, None, None, None, cr, None, TOL)
    else:
        stats = ms.violations(params(), x, g[case + '_radii'], flags, None, None, np.array([0, len(b)]), b, None, cr,
                              None, TOL)
    assert stats.shape == (1, 1, 104)
    assert np.array_equal(stats[0, 0], g[case + '_rec'])


@pytest.mark.parametrize('case', ENV_CASES)
def test_gpu_envelope_record_equals_reference(edges, ms, case):
    g = edges
    x = g[case + '_pos'][None]
    n = x.shape[1]
    flags = np.full(n, IGM_ATOM_BEAD | IGM_ATOM_ENV0, np.uint32)
    prm = params([(tuple(g[case + '_abc']), float(g[case + '_k']))])
    stats = ms.violations(prm, x, g[case + '_radii'], flags, None, None, None, None, None, [0.0],
                          [float(g[case + '_scale'])], TOL)
    assert np.array_equal(stats[0, 1], g[case + '_rec'])
    assert not stats[0, 0].any()
    if case.endswith('+1'):  # the reference's scale is the default of a NULL env_scale (envelope.py:51)
        again = ms.violations(prm, x, g[case + '_radii'], flags, None, None, None, None, None, [0.0], None, TOL)
        assert np.array_equal(again, stats)


def test_gpu_all_golden_cases_in_one_structure(edges, ms):
    """ten bond classes and four envelopes, 14 of the 16 classes, in one model: each row is the
    reference's record of its case"""
    g = edges
    xs, rs, fl, bs, cl, off = [], [], [], [], [], 0
    for q, c in enumerate(BOND_CASES):
        xs.append(g[c + '_pos'])
        rs.append(g[c + '_radii'])
        fl.append(np.full(len(g[c + '_pos']), IGM_ATOM_BEAD, np.uint32))
        bs.append(golden_bonds(g, c, off))
        cl.append(np.full(len(bs[-1]), q, np.int32))
        off += len(g[c + '_pos'])
    # the k > 0 and the k < 0 case of a shape score the same particles: one copy, two flags
    for e0, shape in ((0, 'sph'), (2, 'ell')):
        assert np.array_equal(g[shape + '_k+1_pos'], g[shape + '_k-1_pos'])
        xs.append(g[shape + '_k+1_pos'])
        rs.append(g[shape + '_k+1_radii'])
        fl.append(np.full(len(xs[-1]), IGM_ATOM_BEAD | (IGM_ATOM_ENV0 << e0) | (IGM_ATOM_ENV0 << (e0 + 1)), np.uint32))
    prm = params([(tuple(g[c + '_abc']), float(g[c + '_k'])) for c in ENV_CASES])
    bonds, cls = np.concatenate(bs), np.concatenate(cl)
    order = np.random.default_rng(1).permutation(len(bonds))
    stats = ms.violations(prm, np.concatenate(xs)[None], np.concatenate(rs), np.concatenate(fl), bonds[order],
                          cls[order], None, None, None, [float(g[c + '_cr']) for c in BOND_CASES],
                          [float(g[c + '_scale']) for c in ENV_CASES], TOL)
    for q, c in enumerate(BOND_CASES + ENV_CASES):
        assert np.array_equal(stats[0, q], g[c + '_rec']), c


def test_gpu_ladders_through_the_anchor_kernel(edges, ms):
    """the upper-bound ladders as position anchors: the far atom becomes the target, the atom at
    the origin carries the anchors; one ladder per structure, one structure with none"""
    g = edges
    cases = ['up100', 'up300', 'up700', 'up100k', 'up700k']
    per = []
    for c in cases:
        assert not g[c + '_lower'].any() and np.all(g[c + '_i'] == 0) and not g[c + '_pos'][0].any()
        per.append((np.full(len(g[c + '_j']), 2), g[c + '_pos'][g[c + '_j']], g[c + '_r0'], g[c + '_k']))
    z = g['zero_d_lower'] == 0  # r0 == 0: ratio 0, counted
    per.append((np.full(int(z.sum()), 2), g['zero_d_pos'][g['zero_d_j'][z]], g['zero_d_r0'][z], g['zero_d_k'][z]))
    per.insert(3, (np.zeros(0, np.int64), np.zeros((0, 3))))
    ptr = np.zeros(len(per) + 1, np.int64)
    anch = []
    for s, item in enumerate(per):
        a = np.zeros(len(item[0]), anchor_dtype)
        if len(a):
            a['atom'] = item[0]
            a['x'], a['y'], a['z'] = item[1][:, 0], item[1][:, 1], item[1][:, 2]
            a['r0'], a['k'] = item[2], item[3]
        anch.append(a)
        ptr[s + 1] = ptr[s] + len(a)
    x = np.full((len(per), 3, 3), 7.0, np.float32)
    x[:, 2] = 0.0  # the anchored atom, at the origin like atom 0 of the ladders
    rec = ms.anchor_violations(x, TOL, (ptr, np.concatenate(anch)))
    want = [g[c + '_rec'] for c in cases]
    zero = np.zeros(104, np.int64)
    zero[0] = zero[103] = int(z.sum())
    want.append(zero)
    want.insert(3, np.zeros(104, np.int64))
    assert np.array_equal(rec, np.stack(want))


# ---------------------------------------------------------------- random small models
class Case(object):
    """A batch of S structures of natom atoms in a box of 150 nm: bonds whose ratios spread over
    the bins (classes with a contact range: d from the radii; the others: r0 drawn around the
    pair's distance in structure 0), a quarter of them lower bounds, k one of three values."""

    def __init__(self, seed, S, natom, class_cr, envelopes=(), struct_flags=False):
        rng = self.rng = np.random.default_rng(seed)
        self.S, self.natom, self.class_cr, self.envelopes = S, natom, list(class_cr), list(envelopes)
        self.x = rng.uniform(-150.0, 150.0, (S, natom, 3)).astype(np.float32)
        self.radii = rng.uniform(10.0, 60.0, natom).astype(np.float32)
        shape = (S, natom) if struct_flags else (natom,)
        self.flags = np.full(shape, IGM_ATOM_BEAD, np.uint32)
        for e in range(len(self.envelopes)):  # each envelope on its own subset of the atoms
            self.flags |= np.where(rng.random(shape) < 0.6, np.uint32(IGM_ATOM_ENV0 << e), np.uint32(0))
        self.flags[..., natom // 2] = IGM_ATOM_BEAD  # one atom in no envelope
        self.prm = params(self.envelopes)
        self.shared = self.shared_cls = self.ptr = self.sb = self.scls = None

    def bonds(self, n, s=0, classes=None):
        rng = self.rng
        b = np.zeros(n, bond_dtype)
        i = rng.integers(0, self.natom, n)
        j = rng.integers(0, self.natom, n)
        cls = rng.integers(0, max(1, len(self.class_cr)), n).astype(np.int32) if classes is None else \
            rng.choice(np.asarray(classes), n).astype(np.int32)
        d = self.x[s, i].astype(np.float64) - self.x[s, j].astype(np.float64)
        b['r0'] = np.sqrt((d * d).sum(1)) * rng.uniform(0.4, 1.6, n)
        b['r0'][rng.random(n) < 0.05] = 0.0
        b['k'] = rng.choice([1.0, 0.37, 2.5], n)
        b['i'] = i
        b['j'] = j.astype(np.uint32) | np.where(rng.random(n) < 0.25, LOWER_BOUND_BIT, np.uint32(0))
        return b, cls

    def set_shared(self, n, with_class=True, classes=None):
        self.shared, cls = self.bonds(n, 0, classes)
        self.shared_cls = cls if with_class else None

    def set_struct(self, counts, with_class=True, classes=None):
        assert len(counts) == self.S
        per = [self.bonds(n, s, classes) for s, n in enumerate(counts)]
        self.ptr, self.sb = M.concat_bonds([p[0] for p in per])
        self.scls = np.concatenate([p[1] for p in per]) if with_class else None

    def expected(self, env_scale=None):
        out = np.zeros((self.S, len(self.class_cr) + len(self.envelopes), 104), np.int64)
        none = np.zeros(0, bond_dtype)
        for s in range(self.S):
            own = self.sb[self.ptr[s]:self.ptr[s + 1]] if self.sb is not None else none
            sh = self.shared if self.shared is not None else none
            ocl = self.scls[self.ptr[s]:self.ptr[s + 1]] if self.scls is not None else np.zeros(len(own), np.int32)
            shc = self.shared_cls if self.shared_cls is not None else np.zeros(len(sh), np.int32)
            fl = self.flags[s] if self.flags.ndim == 2 else self.flags
            out[s] = VR.model_record(self.x[s], self.radii, fl, np.concatenate([sh, own]), np.concatenate([shc, ocl]),
                                     self.class_cr, self.envelopes, TOL, env_scale)
        return out

    def gpu(self, ms, env_scale=None):
        return ms.violations(self.prm, self.x, self.radii, self.flags, self.shared, self.shared_cls, self.ptr,
                             self.sb, self.scls, self.class_cr, env_scale, TOL)


COUNTS = [0, 1, 255, 256, 257, 1000]


def spread(stats, nbins=30):
    """the model exercises the histogram: many bins, the overflow, zero and violated ratios"""
    tot = stats.sum(axis=(0, 1))
    return np.count_nonzero(tot[:100]) >= nbins and tot[100] > 0 and 0 < tot[102] < tot[101] < tot[103]


@pytest.mark.parametrize('with_class', [False, True])
@pytest.mark.parametrize('source', ['shared', 'struct', 'both'])
def test_gpu_bond_counts_sources_and_class_arrays(ms, source, with_class):
    """0, 1, 255, 256, 257 and 1000 bonds per structure from the shared list (sbond_ptr NULL), from
    the per-structure lists (nshared 0) and from both; class arrays NULL (class 0) or given"""
    class_cr = [2.0, 0.0, 1.05] if with_class else [0.0]
    if source == 'shared':
        for q, n in enumerate(COUNTS):
            c = Case(100 + q, 2, 40, class_cr)
            c.set_shared(n, with_class)
            got = c.gpu(ms)
            assert np.array_equal(got, c.expected()), n
            assert got[:, :, 103].sum() == 2 * n
    else:
        c = Case(110, len(COUNTS), 40, class_cr)
        c.set_struct(COUNTS, with_class)
        if source == 'both':
            c.set_shared(257, not with_class)  # the two class arrays NULL and given in turn
        got = c.gpu(ms)
        assert np.array_equal(got, c.expected())
        assert np.array_equal(got[:, :, 103].sum(1), np.array(COUNTS) + (257 if source == 'both' else 0))
        assert spread(got)


def test_gpu_class_arrays_both_null_and_both_given(ms):
    for with_class in (False, True):
        c = Case(120, 3, 33, [0.0, 2.0])
        c.set_shared(300, with_class)
        c.set_struct([257, 0, 31], with_class)
        got = c.gpu(ms)
        assert np.array_equal(got, c.expected())
        assert (got[:, 1, 103].sum() > 0) == with_class


def test_gpu_out_of_range_classes_are_skipped(ms):
    """class ids -1 and >= nclass_bonds appear in no record, not even in n_imposed"""
    ids = [-1, 0, 1, 2, 3, 7, 2 ** 31 - 1, -2 ** 31]
    c = Case(130, 4, 50, [0.0, 2.0, 1.05], ENVS4[:1])
    c.set_shared(400, classes=ids)
    c.set_struct([300, 0, 257, 5], classes=ids)
    got = c.gpu(ms)
    assert np.array_equal(got, c.expected())
    kept = np.isin(c.shared_cls, [0, 1, 2]).sum() + np.array(
        [np.isin(c.scls[c.ptr[s]:c.ptr[s + 1]], [0, 1, 2]).sum() for s in range(4)])
    assert np.array_equal(got[:, :3, 103].sum(1), kept) and kept[1] < 400


def test_gpu_lower_bound_bit_on_the_last_atoms(ms):
    """bit 31 of j marks a lower bound; with j = natom - 1 and natom - 2 a kernel that did not
    mask it would read far outside the structure, one that ignored it scores an upper bound"""
    natom = 257
    c = Case(140, 3, natom, [0.0])
    b, _ = c.bonds(300)
    b['j'] = np.where(np.arange(300) % 2 == 0, natom - 1, natom - 2).astype(np.uint32) | LOWER_BOUND_BIT
    b['i'] = c.rng.integers(0, natom - 2, 300)
    c.shared = b
    got = c.gpu(ms)
    assert np.array_equal(got, c.expected())
    up = b.copy()
    up['j'] &= np.uint32(0x7fffffff)
    c.shared = up
    assert not np.array_equal(c.expected(), got)


def test_gpu_sixteen_classes_fill_the_table(ms):
    """nclass_bonds + nenvelopes == 16: every class populated and different"""
    c = Case(150, 3, 64, [0.0, 2.0, 1.05, 0.0, 3.0, 0.5, 0.0, 1.5, 2.5, 0.0, 1.0, 4.0], ENVS4)
    c.set_shared(900)
    c.set_struct([700, 13, 257])
    got = c.gpu(ms)
    assert got.shape == (3, 16, 104)
    assert np.array_equal(got, c.expected())
    assert np.all(got[0, :, 103] > 0) and len({r.tobytes() for r in got[0]}) == 16


@pytest.mark.parametrize('nb,ne', [(13, 4), (17, 0), (16, 1)])
def test_gpu_seventeen_classes_are_invalid(ctx, nb, ne):
    """one class more than the LDS table holds: IGM_E_INVALID from the argument check, the
    output untouched"""
    c = Case(160, 2, 8, [0.0] * nb, ENVS4[:ne])
    c.set_shared(5)
    stats = np.full((2, nb + ne, 104), -7, np.int64)
    ccr = np.zeros(nb, np.float64)
    rc = ctx.lib.igm_mstep_violations(ctx.h, 0, ctypes.byref(c.prm), 2, 8, c.x.ctypes.data, c.radii.ctypes.data,
                                      c.flags.ctypes.data, c.shared.ctypes.data, c.shared_cls.ctypes.data, 5, None,
                                      None, None, nb, ccr.ctypes.data, None, TOL, stats.ctypes.data)
    assert rc == IGM_E_INVALID
    assert np.all(stats == -7)


@pytest.mark.parametrize('natom', [1, 3, 257])
def test_gpu_atom_counts(ms, natom):
    c = Case(170 + natom, 3, natom, [0.0, 2.0], ENVS4[:2])
    c.set_shared(40)
    c.set_struct([0, 300, 7])
    got = c.gpu(ms)
    assert np.array_equal(got, c.expected())
    assert got[0, 2:, 103].sum() == np.count_nonzero(c.flags & IGM_ATOM_ENV0) + np.count_nonzero(
        c.flags & (IGM_ATOM_ENV0 << 1))


@pytest.mark.parametrize('S', [1, 2, 300])
def test_gpu_batch_sizes(ms, S):
    """300 structures are more blocks than CUs; every structure has its own coordinates and its
    own bond count, so a wrong block offset shows"""
    c = Case(180 + S, S, 37, [0.0, 2.0], ENVS4[:1], struct_flags=True)
    c.set_shared(20)
    c.set_struct([(17 * s + 3) % 301 for s in range(S)])
    got = c.gpu(ms)
    assert np.array_equal(got, c.expected())
    assert len({got[s].tobytes() for s in range(S)}) == S


@pytest.mark.parametrize('scale', [None, [30.0, 55.0, 8.0, 21.0]])
@pytest.mark.parametrize('struct_flags', [False, True])
def test_gpu_four_envelopes(ms, struct_flags, scale):
    """four ellipsoids, k > 0 and k < 0 mixed, each on its own atoms; flags shared or one row per
    structure (IGM_MSTEP_STRUCT_FLAGS); env_scale given or NULL"""
    c = Case(190, 5, 300, [0.0], ENVS4, struct_flags=struct_flags)
    c.set_struct([3, 0, 0, 9, 1])
    got = c.gpu(ms, scale)
    assert np.array_equal(got, c.expected(scale))
    assert spread(got[:, 1:])
    assert got[0, 1, 103] < 300 and len(set(got[0, 1:, 103])) > 1
    if struct_flags:
        assert len(set(got[:, 1, 103])) > 1
    other = c.expected([30.0, 55.0, 8.0, 21.0] if scale is None else None)
    assert not np.array_equal(other, got)


def test_gpu_device_pointers_give_the_same_record(ctx, ms):
    import torch
    c = Case(200, 7, 65, [0.0, 2.0, 1.05], ENVS4[:3], struct_flags=True)
    c.set_shared(300)
    c.set_struct([0, 1, 255, 256, 257, 1000, 2])
    host = c.gpu(ms)
    assert np.array_equal(host, c.expected())
    prm = MStepParams.from_buffer_copy(c.prm)
    prm.flags |= IGM_MSTEP_STRUCT_FLAGS

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()

    t = [dev(a) for a in (c.x, c.radii, c.flags, c.shared, c.shared_cls, c.ptr, c.sb, c.scls)]
    stats = torch.full((7, 6, 104), -7, dtype=torch.int64, device='cuda')
    ccr = np.asarray(c.class_cr, np.float64)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        rc = ctx.lib.igm_mstep_violations(ctx.h, IGM_DEVICE_PTRS, ctypes.byref(prm), 7, 65, t[0].data_ptr(),
                                          t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(), 300,
                                          t[5].data_ptr(), t[6].data_ptr(), t[7].data_ptr(), 3, ccr.ctypes.data, None,
                                          TOL, stats.data_ptr())
    finally:
        ctx.set_stream(None)
    assert rc == IGM_OK
    torch.cuda.synchronize()
    assert np.array_equal(stats.cpu().numpy(), host)
