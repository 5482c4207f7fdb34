"""igm_report_hic on the MI355X, through igm_amd.report and the C ABI.

Against what the reference's report_hic wrote on a sub-population of the demo
(report_hic_golden.npz) and against the dense restatement tests/report_hic_ref.py on
hand-made counts at the smallest shapes at which the kernels can go wrong.  Bars: every
integer statistic and both histograms are bit-equal to the restatement; a correlation is
held to CORRELATION_BAR of the exactly rounded r (r^2 in rational arithmetic, one square
root).  The bar is measured, not assumed: scipy.stats.pearsonr, which sums the same centred
products in float64 in another order, lies within 4 * 2^-53 of the exact r on these inputs
(test_report_hic.py::test_scipy_distance_is_the_recorded_one re-measures it); the kernels
get 4 times that for the order effects, never less than 8 * 2^-53 for the final divide,
square root and rounding.  Every call is made twice and must return the same bytes."""
import numpy as np
import pytest

import report_hic_ref as R
from conftest import load_golden
from igm_amd import _lib, evaluation, hss, report as RP

pytestmark = pytest.mark.gpu

# measured: scipy lies within 4 * 2^-53 of the exact r on these inputs; the bar is 4 times that
CORRELATION_BAR = R.CORRELATION_BAR  # max(4 * (4 * 2^-53), 8 * 2^-53) = 16 * 2^-53 = 1.78e-15
STAT_KEYS = ('n', 'dense_sums', 'sparse_ints', 'sparse_sumx', 'means', 'centred', 'log_hist', 'lin_hist')


@pytest.fixture(scope='module')
def ctx():
    return _lib.context(0)


@pytest.fixture(scope='module')
def gold():
    return load_golden('report_hic_golden.npz')


@pytest.fixture(scope='module')
def demo(gold):
    sub = R.sub_population(load_golden('demo_population.npz'), gold['loci'])
    return sub, {k: gold[k] for k in ('indptr', 'indices', 'data')}


@pytest.fixture(scope='module')
def cases():
    """the hand-made cases with their exact correlations, computed once"""
    out = R.synthetic_cases()
    for c in out.values():
        x, y = R.case_xy(c)
        c['x'], c['y'] = x, y
        c['exact'] = R.correlations(x, y, c['hap_chrom'], c['intra_sigma'], c['inter_sigma'], r=R.exact_r,
                                    nchrom=c['nchrom'])
    return out


def same_bytes(a, b):
    for k in STAT_KEYS:
        assert (a[k] is None and b[k] is None) or a[k].tobytes() == b[k].tobytes(), k


def run_case(ctx, c, log_edges='default', lin_edges='default', **kw):
    """hic_statistics twice (the rerun must be bitwise equal)"""
    le, li = RP.hic_edges()
    args = (c['counts'], c['nstruct'], c['matrix'], c['hap_chrom'], c['intra_sigma'], c['inter_sigma'],
            le if isinstance(log_edges, str) else log_edges, li if isinstance(lin_edges, str) else lin_edges)
    a = RP.hic_statistics(*args, nchrom=c['nchrom'], ctx=ctx, **kw)
    b = RP.hic_statistics(*args, nchrom=c['nchrom'], ctx=ctx, **kw)
    same_bytes(a, b)
    return a


def check_correlations(got, exact, what):
    worst = 0.0
    for m in R.MASKS:
        a = np.append(exact['intra'][m], exact['inter'][m])
        b = np.append(got['intra'][m], got['inter'][m])
        assert np.array_equal(np.isnan(a), np.isnan(b)), (what, m, a, b)
        worst = max(worst, np.max(np.abs(a - b)[~np.isnan(a)], initial=0.0))
    print('%s: max |r - exact r| = %.3g (bar %.3g)' % (what, worst, CORRELATION_BAR))
    assert worst <= CORRELATION_BAR, what


# ------------------------------------------------------------------ the demo golden
def test_demo_golden_correlations_and_histograms(ctx, gold, demo):
    sub, matrix = demo
    res = RP.hic_comparison(sub['coordinates'], matrix, float(gold['contact_range']), float(gold['intra_sigma']),
                            float(gold['inter_sigma']), sub['radii'], sub['copy_ptr'], sub['copy_idx'],
                            sub['hap_chrom'], ctx=ctx)
    ids = np.unique(sub['hap_chrom'])
    rows = {'intra': {m: res['intra'][m][ids] for m in R.MASKS}, 'inter': res['inter']}
    intra, inter = RP.hic_correlation_texts([str(c) for c in gold['chrom_names']], rows)
    assert intra == str(gold['intra_text'])
    assert inter == str(gold['inter_text'])
    assert np.array_equal(res['log_hist'], gold['log_hist']) and res['log_hist'].dtype == np.int64
    assert np.array_equal(res['lin_hist'], gold['lin_hist']) and res['lin_hist'].shape == (99, 99)
    assert res['log_edges'].tobytes() == gold['log_edges'].tobytes()
    assert res['lin_edges'].tobytes() == gold['lin_edges'].tobytes()
    absent = np.setdiff1d(np.arange(len(res['intra']['all'])), ids)
    assert np.isnan(res['intra']['all'][absent]).all()  # chromosome ids without a locus


def test_demo_command_line_writes_the_five_files(gold, demo, tmp_path, capsys):
    sub, matrix = demo
    names = [b'chr%d' % (k + 1) for k in range(22)] + [b'chrX', b'chrY']
    genome = {'assembly': 'hg38', 'chroms': np.array(names, 'S10'), 'lengths': np.zeros(24, np.int32),
              'origins': np.zeros(24, np.int32)}
    p = str(tmp_path / 'sub.hss')
    hss.write_hss(p, sub['coordinates'], sub['radii'],
                  hss.index_tree(sub['chrom'], sub['copy'], sub['copy_ptr'], sub['copy_idx']), genome=genome)
    hcs = str(tmp_path / 'input.hcs')
    hss.write_hcs(hcs, R.dense_input(matrix), chrom=sub['hap_chrom'])
    out = tmp_path / 'qc'
    rc = RP.main([p, '--steps', 'hic', '-l', 'g', '-o', str(out), '--hic', hcs, '--hic-contact-range',
                  str(float(gold['contact_range'])), '--hic-intra-sigma', str(float(gold['intra_sigma'])),
                  '--hic-inter-sigma', str(float(gold['inter_sigma']))])
    assert rc == 0
    mc = out / 'matrix_comparison'
    printed = capsys.readouterr().out.split()
    for name in ('outmap-g.hcs', 'intra_correlations-g.txt', 'inter_correlations-g.txt', 'log_histogram2d-g.npy',
                 'linear_histogram2d-g.npy'):
        assert (mc / name).is_file() and str(mc / name) in printed
    # the names come from genome/chroms by position among the chromosomes present, as the rgs step resolves them
    got = (mc / 'intra_correlations-g.txt').read_text().splitlines()
    want = str(gold['intra_text']).splitlines()
    assert got[0] == want[0] and [ln[6:] for ln in got[1:]] == [ln[6:] for ln in want[1:]]
    assert (mc / 'inter_correlations-g.txt').read_text() == str(gold['inter_text'])
    assert np.array_equal(np.load(mc / 'log_histogram2d-g.npy'), gold['log_hist'])
    assert np.array_equal(np.load(mc / 'linear_histogram2d-g.npy'), gold['lin_hist'])
    counts = R.contact_counts(sub['coordinates'], sub['radii'], float(gold['contact_range']), sub['copy_ptr'],
                              sub['copy_idx'])
    om = hss.read_hcs(str(mc / 'outmap-g.hcs'))
    assert np.array_equal(R.dense_input(om), R.probabilities(counts, 100).astype(np.float32))
    assert np.array_equal(om['chrom'], sub['hap_chrom'])


# ------------------------------------------------------------------ hand-made counts
@pytest.mark.parametrize('name', sorted(R.synthetic_cases()))
def test_synthetic_statistics(ctx, cases, name):
    c = cases[name]
    st = run_case(ctx, c)
    stored = R.stored_mask(c['matrix'], len(c['hap_chrom']))
    n, dense, sparse = R.integer_statistics(c['counts'], c['nstruct'], c['x'], c['hap_chrom'], c['intra_sigma'],
                                            c['inter_sigma'], stored, c['nchrom'])
    assert np.array_equal(st['n'], n)
    assert np.array_equal(st['dense_sums'], dense)
    assert np.array_equal(st['sparse_ints'], sparse)
    le, li = RP.hic_edges()
    assert np.array_equal(st['log_hist'], R.histogram(c['x'], c['y'], le, le))
    assert np.array_equal(st['lin_hist'], R.histogram(c['x'], c['y'], li, li))
    check_correlations(RP.hic_correlations(st), c['exact'], name)


def test_synthetic_special_entries(ctx, cases):
    """the entries placed by hand in the 130-locus case land where the definitions put them"""
    c = cases['n130']
    assert c['counts'].max() > c['nstruct']                       # the clip is exercised
    assert np.diff(c['matrix']['indptr'])[1] == 129 and np.diff(c['matrix']['indptr'])[2] == 0
    assert (c['matrix']['data'] == 0).sum() >= 2                  # stored explicit zeros
    assert len(np.unique(c['hap_chrom'])) == 3 and c['nchrom'] == 6  # ids 5, 0, 2: not contiguous
    st = run_case(ctx, c)
    le, _ = RP.hic_edges()
    h = st['log_hist']
    kx = lambda v: int(np.searchsorted(le, np.float64(v), side='right')) - 1  # noqa: E731
    assert h[0, kx(np.float32(c['intra_sigma']))] >= 2            # (3, 4): y == 1e-3 sits in the first row
    assert h[99, kx(np.float32(1e-3))] >= 2 and kx(np.float32(1e-3)) == 0  # (4, 6): x = f32(1e-3), y == 1: last bin
    below = np.float64(np.nextafter(np.float32(1e-3), np.float32(0)))
    assert below < le[0]                                          # (4, 101): dropped, checked through the total
    assert h.sum() == R.histogram(c['x'], c['y'], le, le).sum()
    # x == sigma is restrained: the hand-placed entries are in half 0
    x = c['x'].astype(np.float64)
    assert x[3, 4] == c['intra_sigma'] and x[3, 100] == c['inter_sigma']
    one_less = dict(c, intra_sigma=np.nextafter(c['intra_sigma'], 1.0))
    st2 = run_case(ctx, one_less)
    p = int(c['hap_chrom'][3])
    assert st['sparse_ints'][p, 0, 0] - st2['sparse_ints'][p, 0, 0] == 2  # the off-diagonal entry, weight 2


def test_int64_sums_past_2_31(ctx, cases):
    c = cases['n65_big']
    assert c['nstruct'] == 50000 and c['counts'].max() > 46341    # c'^2 passes 2^31
    st = run_case(ctx, c, log_edges=None, lin_edges=None)
    assert st['dense_sums'][:, 1].max() > 2 ** 40
    assert st['log_hist'] is None and st['lin_hist'] is None


def test_unaligned_counts_base(ctx, cases):
    """a counts matrix that starts 4, 8 and 12 bytes past a 16-byte boundary (device pointers)"""
    import torch
    c = cases['n63']
    n = len(c['hap_chrom'])
    want = run_case(ctx, c)
    idx = torch.from_numpy(c['matrix']['indices']).cuda()
    dat = torch.from_numpy(c['matrix']['data']).cuda()
    for off in (1, 2, 3):
        buf = torch.zeros(n * n + 4, dtype=torch.int32, device='cuda')
        view = buf[off:off + n * n].view(n, n)
        view.copy_(torch.from_numpy(c['counts']))
        assert view.data_ptr() % 16 == 4 * off
        got = run_case(ctx, dict(c, counts=view, matrix=dict(c['matrix'], indices=idx, data=dat)),
                       flags=_lib.IGM_DEVICE_PTRS)
        same_bytes(got, want)


def test_device_pointers_give_the_same_bytes(ctx, cases):
    import torch
    c = cases['n130']
    want = run_case(ctx, c)
    dev = dict(c, counts=torch.from_numpy(c['counts']).cuda(),
               matrix=dict(c['matrix'], indices=torch.from_numpy(c['matrix']['indices']).cuda(),
                           data=torch.from_numpy(c['matrix']['data']).cuda()))
    got = run_case(ctx, dev, flags=_lib.IGM_DEVICE_PTRS)
    torch.cuda.synchronize()
    same_bytes(got, want)


def test_each_histogram_nullable(ctx, cases):
    c = cases['n63']
    both = run_case(ctx, c)
    only_log = run_case(ctx, c, lin_edges=None)
    only_lin = run_case(ctx, c, log_edges=None)
    assert only_log['lin_hist'] is None and only_lin['log_hist'] is None
    assert np.array_equal(only_log['log_hist'], both['log_hist'])
    assert np.array_equal(only_lin['lin_hist'], both['lin_hist'])
    for k in ('dense_sums', 'sparse_ints', 'sparse_sumx', 'means', 'centred'):
        assert only_log[k].tobytes() == both[k].tobytes() == only_lin[k].tobytes()


def test_rectangular_histogram_orientation(ctx, cases):
    """different edges on the two axes: rows = output (y), columns = input (x)"""
    c = cases['n63']
    ex, ey = np.array([1e-3, 0.1, 0.5, 1.0]), np.array([1e-3, 0.5, 1.0])
    st = run_case(ctx, c, log_edges=(ex, ey), lin_edges=None)
    assert st['log_hist'].shape == (2, 3)
    assert np.array_equal(st['log_hist'], R.histogram(c['x'], c['y'], ex, ey))


# ------------------------------------------------------------------ end to end
def test_end_to_end_with_the_contact_kernel(ctx):
    """130 loci with one- and two-copy loci, 33 structures: the real contact kernel, then the
    comparison, against the restatement fed by a NumPy contact count"""
    rng = np.random.default_rng(21)
    sizes = (40, 57, 33)
    hap_chrom = np.repeat(np.arange(3), sizes).astype(np.int32)
    copies = np.where(hap_chrom < 2, 2, 1)
    copies[5:9] = 1
    rows, chrom, copy = [[] for _ in copies], [], []
    for k in range(2):
        for h in np.flatnonzero(copies > k):
            rows[h].append(len(chrom))
            chrom.append(hap_chrom[h])
            copy.append(k)
    copy_ptr = np.concatenate([[0], np.cumsum(copies)]).astype(np.int32)
    copy_idx = np.array([b for r in rows for b in r], np.int32)
    nbead = len(chrom)
    xyz = (rng.standard_normal((nbead, 33, 3)) * 500).astype(np.float32)
    radii = rng.uniform(150, 250, nbead).astype(np.float32)
    up = np.triu(rng.uniform(0.0, 0.6, (130, 130))).astype(np.float32)
    matrix = R.csr_from_dense(up, np.triu(rng.uniform(size=(130, 130)) < 0.7, 1))
    res = RP.hic_comparison(xyz, matrix, 2.0, 0.3, 0.2, radii, copy_ptr, copy_idx, hap_chrom, ctx=ctx)
    counts = R.contact_counts(xyz, radii, 2.0, copy_ptr, copy_idx)
    assert np.array_equal(res['counts'], counts) and counts.max() > 33  # copies summed: the clip matters
    x, y = R.dense_input(matrix, 130), R.probabilities(counts, 33)
    check_correlations(res, R.correlations(x, y, hap_chrom, 0.3, 0.2, r=R.exact_r), 'end to end')
    assert np.array_equal(res['log_hist'], R.histogram(x, y, res['log_edges'], res['log_edges']))
    assert np.array_equal(res['lin_hist'], R.histogram(x, y, res['lin_edges'], res['lin_edges']))
    assert np.array_equal(evaluation.haploid_counts(xyz, radii, 2.0, copy_ptr, copy_idx, ctx=ctx), counts)


# ------------------------------------------------------------------ argument checks (before any launch)
def raw_call(ctx, c, **over):
    a = dict(counts=c['counts'], nhap=len(c['hap_chrom']), nstruct=c['nstruct'], indptr=c['matrix']['indptr'],
             indices=c['matrix']['indices'], data=c['matrix']['data'], hap_chrom=c['hap_chrom'], nchrom=c['nchrom'],
             edges=RP.hic_edges()[0], flags=0)
    a.update(over)
    P = a['nchrom'] + 1
    e = np.ascontiguousarray(a['edges'], np.float64)
    hist = np.zeros((len(e) - 1, len(e) - 1), np.int64)
    outs = [np.zeros((P, 2), np.int64), np.zeros((P, 2, 3), np.int64), np.zeros((P, 2)), np.zeros((P, 3, 2)),
            np.zeros((P, 3, 2))]
    keep = [np.ascontiguousarray(a['indptr'], np.int64), np.ascontiguousarray(a['hap_chrom'], np.int32)]
    rc = ctx.lib.igm_report_hic(ctx.h, a['flags'], _lib.ptr(a['counts']), a['nhap'], a['nstruct'],
                                keep[0].ctypes.data, _lib.ptr(a['indices']), _lib.ptr(a['data']),
                                keep[1].ctypes.data, a['nchrom'], 0.3, 0.02, e.ctypes.data, len(e) - 1,
                                e.ctypes.data, len(e) - 1, hist.ctypes.data, None, 0, None, 0, None,
                                *[o.ctypes.data for o in outs])
    msg = ctx.lib.igm_last_error(ctx.h)
    return rc, msg.decode() if msg else ''


def test_invalid_arguments(ctx, cases):
    import torch
    c = cases['n63']
    m = c['matrix']
    rows = np.repeat(np.arange(63), np.diff(m['indptr']))
    k = int(np.flatnonzero(rows == 10)[0])
    below = m['indices'].copy()
    below[k] = 3                                            # an entry below the diagonal
    beyond = m['indices'].copy()
    beyond[k] = 63                                          # a column index >= nhap
    dec = m['indptr'].copy()
    dec[5] = dec[4] - 1                                     # decreasing indptr
    bad_chrom = c['hap_chrom'].copy()
    bad_chrom[7] = c['nchrom']                              # hap_chrom out of range
    edges = RP.hic_edges()[0].copy()
    edges[4] = edges[3]                                     # not strictly increasing
    for over, word in ((dict(indices=below), 'below the diagonal'), (dict(indices=beyond), 'outside'),
                       (dict(indptr=dec), 'indptr'), (dict(hap_chrom=bad_chrom), 'hap_chrom'),
                       (dict(edges=edges), 'increasing'), (dict(nstruct=0), 'nstruct')):
        rc, msg = raw_call(ctx, c, **over)
        assert rc == _lib.IGM_E_INVALID and word in msg, (over.keys(), rc, msg)
    # the same column checks on device arrays: the flag kernel, no other launch
    dev = dict(counts=torch.from_numpy(c['counts']).cuda(), data=torch.from_numpy(m['data']).cuda(),
               flags=_lib.IGM_DEVICE_PTRS)
    for idx, word in ((below, 'below the diagonal'), (beyond, 'outside')):
        rc, msg = raw_call(ctx, c, indices=torch.from_numpy(idx).cuda(), **dev)
        assert rc == _lib.IGM_E_INVALID and word in msg, (rc, msg)
    with pytest.raises(RuntimeError, match='below the diagonal'):
        RP.hic_statistics(c['counts'], c['nstruct'], dict(m, indices=below), c['hap_chrom'], 0.3, 0.02, ctx=ctx)
    rc, msg = raw_call(ctx, c)
    assert rc == 0, msg


def test_unsupported_arguments(ctx, cases):
    c = cases['n63']
    for first in (0.0, -1e-3):
        edges = RP.hic_edges()[0].copy()
        edges[0] = first
        rc, msg = raw_call(ctx, c, edges=edges)
        assert rc == _lib.IGM_E_UNSUPPORTED and '<= 0' in msg, (rc, msg)
    # nhap^2 nstruct^2 >= 2^63 is refused before anything is read: 63^2 * (2^31 - 1)^2 > 2^63
    rc, msg = raw_call(ctx, c, nstruct=2 ** 31 - 1)
    assert rc == _lib.IGM_E_UNSUPPORTED and '2^63' in msg, (rc, msg)
