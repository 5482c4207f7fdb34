"""Hi-C report step, host side (no GPU): the dense restatement tests/report_hic_ref.py
against what the reference's report_hic wrote (report_hic_golden.npz, made by
golden/make_golden_report_hic.py), the host combination hic_correlations against exact
rational arithmetic, and the host layer -- configuration, command line, the .hcs writer,
the files of the 'hic' step -- with the native calls replaced by the restatement.  The
kernels themselves are tested in test_report_hic_gpu.py."""
import json
from fractions import Fraction

import numpy as np
import pytest

import report_hic_ref as R
from conftest import load_golden
from igm_amd import hss, report as RP

SCIPY_DISTANCE = R.SCIPY_DISTANCE    # 4 * 2^-53, measured (test_scipy_distance_is_the_recorded_one)
CORRELATION_BAR = R.CORRELATION_BAR  # 16 * 2^-53


@pytest.fixture(scope='module')
def gold():
    return load_golden('report_hic_golden.npz')


@pytest.fixture(scope='module')
def demo(gold):
    """the golden's sub-population, its input matrix and the dense x, y of the restatement"""
    sub = R.sub_population(load_golden('demo_population.npz'), gold['loci'])
    matrix = {k: gold[k] for k in ('indptr', 'indices', 'data')}
    counts = R.contact_counts(sub['coordinates'], sub['radii'], float(gold['contact_range']), sub['copy_ptr'],
                              sub['copy_idx'])
    return sub, matrix, counts, R.dense_input(matrix), R.probabilities(counts, sub['coordinates'].shape[1])


@pytest.fixture(scope='module')
def cases():
    """the hand-made cases with their dense x, y and exact correlations, computed once"""
    out = R.synthetic_cases()
    for c in out.values():
        c['x'], c['y'] = R.case_xy(c)
        c['exact'] = R.correlations(c['x'], c['y'], c['hap_chrom'], c['intra_sigma'], c['inter_sigma'], r=R.exact_r,
                                    nchrom=c['nchrom'])
    return out


def texts(corr, gold):
    ids = np.unique(gold['hap_chrom'])
    rows = {'intra': {m: corr['intra'][m][ids] for m in R.MASKS}, 'inter': corr['inter']}
    return RP.hic_correlation_texts([str(c) for c in gold['chrom_names']], rows)


def test_golden_is_finite_and_records_versions(gold):
    assert str(gold['numpy_version']).startswith('2.') and str(gold['scipy_version'])
    assert 'nan' not in str(gold['intra_text']) and 'nan' not in str(gold['inter_text'])
    assert len(str(gold['intra_text']).splitlines()) == 1 + len(gold['chrom_names'])
    # the reference defects DESIGN.md section 2 lists: no intra rows without intra_sigma, no file at all without both
    assert str(gold['inter_only_intra_text']) == '# chrom all imposed non_imposed\n'
    assert str(gold['inter_only_inter_text']) == str(gold['inter_text'])
    assert len(gold['no_sigma_files']) == 0


def test_restatement_reproduces_reference_files(gold, demo):
    """every %8.5f field equals the reference's string (none sits on a rounding boundary)"""
    _, _, _, x, y = demo
    corr = R.correlations(x, y, gold['hap_chrom'], float(gold['intra_sigma']), float(gold['inter_sigma']))
    intra, inter = texts(corr, gold)
    assert intra == str(gold['intra_text'])
    assert inter == str(gold['inter_text'])


def test_restatement_reproduces_reference_histograms(gold, demo):
    _, _, _, x, y = demo
    log_edges, lin_edges = RP.hic_edges()
    assert log_edges.tobytes() == gold['log_edges'].tobytes() and lin_edges.tobytes() == gold['lin_edges'].tobytes()
    assert log_edges.tobytes() == np.logspace(-3, 0, 101).tobytes() and len(lin_edges) == 100  # 99 linear bins
    assert np.array_equal(R.histogram(x, y, log_edges, log_edges), gold['log_hist'])
    assert np.array_equal(R.histogram(x, y, lin_edges, lin_edges), gold['lin_hist'])
    assert gold['log_hist'].sum() > 0 and gold['lin_hist'].shape == (99, 99)


def test_correlations_of_restated_statistics_match_reference_files(gold, demo):
    """hic_correlations on the statistics (NumPy sums) gives the reference's strings too"""
    _, matrix, counts, _, _ = demo
    st = R.statistics(counts, 100, matrix, gold['hap_chrom'], float(gold['intra_sigma']), float(gold['inter_sigma']))
    intra, inter = texts(RP.hic_correlations(st), gold)
    assert intra == str(gold['intra_text']) and inter == str(gold['inter_text'])


def test_scipy_distance_is_the_recorded_one(cases):
    """the measurement behind CORRELATION_BAR: scipy against the exact r on every case"""
    worst = 0.0
    for name, c in cases.items():
        exact = c['exact']
        sp = R.correlations(c['x'], c['y'], c['hap_chrom'], c['intra_sigma'], c['inter_sigma'], nchrom=c['nchrom'])
        for m in R.MASKS:
            a = np.append(exact['intra'][m], exact['inter'][m])
            b = np.append(sp['intra'][m], sp['inter'][m])
            assert np.array_equal(np.isnan(a), np.isnan(b)), (name, m)
            worst = max(worst, np.max(np.abs(a - b)[~np.isnan(a)], initial=0.0))
    print('scipy distance %.3g = %.2f * 2^-53' % (worst, worst / 2.0 ** -53))
    assert worst <= SCIPY_DISTANCE


def test_hic_correlations_hand_made_statistics():
    """one chromosome of 2 loci and nothing else, nstruct 4:
         x = [[0.5, 0.25], [0.25, 0]] (the entry (1, 1) is not stored), c = [[4, 1], [1, 2]]
    and the statistics written out by hand"""
    xs, cs = [0.5, 0.25, 0.25, 0.0], [4, 1, 1, 2]
    ybar, xbar = Fraction(8, 16), Fraction(1, 4)
    cross = sum(Fraction(x) * (Fraction(c, 4) - ybar) for x, c in zip(xs[:3], cs[:3]))
    varx = sum((Fraction(x) - xbar) ** 2 for x in xs[:3])
    stats = {'n': np.array([4, 0]), 'nstruct': 4, 'intra_sigma': None, 'inter_sigma': None,
             'dense_sums': np.array([[8, 22], [0, 0]]),
             'sparse_ints': np.array([[[0, 0, 0], [3, 6, 18]], [[0, 0, 0], [0, 0, 0]]]),
             'sparse_sumx': np.array([[0.0, 1.0], [0.0, 0.0]]),
             'means': np.array([[[0.5, 0.25], [0, 0], [0.5, 0.25]], [[0, 0]] * 3], np.float64),
             'centred': np.array([[[float(cross), float(varx)], [0, 0], [float(cross), float(varx)]], [[0, 0]] * 3])}
    got = RP.hic_correlations(stats)
    want = R.exact_r(xs, [c / 4 for c in cs])
    assert abs(got['intra']['all'][0] - want) <= 8 * 2.0 ** -53
    assert np.isnan(got['intra']['restrained'][0]) and np.isnan(got['intra']['non_restrained'][0])  # no sigma
    assert all(np.isnan(got['inter'][m]) for m in R.MASKS)  # fewer than 2 entries
    # a constant side: every count equal
    flat = dict(stats, dense_sums=np.array([[8, 16], [0, 0]]))
    assert np.isnan(RP.hic_correlations(flat)['intra']['all'][0])
    # with a sigma of 0.3 the restrained set is one entry (NaN), the rest has three
    stats2 = dict(stats, intra_sigma=0.3)
    stats2['sparse_ints'] = np.array([[[1, 4, 16], [2, 2, 2]], [[0, 0, 0], [0, 0, 0]]])
    ybar2, xbar2 = Fraction(4, 12), Fraction(1, 6)
    cross2 = sum(Fraction(x) * (Fraction(c, 4) - ybar2) for x, c in zip(xs[1:3], cs[1:3]))
    varx2 = sum((Fraction(x) - xbar2) ** 2 for x in xs[1:3])
    stats2['means'] = np.array([[[0.5, 0.25], [1.0, 0.5], [float(ybar2), float(xbar2)]], [[0, 0]] * 3])
    stats2['centred'] = np.array([[[float(cross), float(varx)], [0, 0], [float(cross2), float(varx2)]],
                                  [[0, 0]] * 3])
    got = RP.hic_correlations(stats2)
    assert np.isnan(got['intra']['restrained'][0])
    assert abs(got['intra']['non_restrained'][0] - R.exact_r(xs[1:], [c / 4 for c in cs[1:]])) <= 8 * 2.0 ** -53


def test_hic_correlations_on_every_hand_made_case(cases):
    """the host combination on the restated statistics stays within the bar of the exact r"""
    for name, c in cases.items():
        exact = c['exact']
        st = R.statistics(c['counts'], c['nstruct'], c['matrix'], c['hap_chrom'], c['intra_sigma'], c['inter_sigma'],
                          nchrom=c['nchrom'])
        got = RP.hic_correlations(st)
        for m in R.MASKS:
            a = np.append(exact['intra'][m], exact['inter'][m])
            b = np.append(got['intra'][m], got['inter'][m])
            assert np.array_equal(np.isnan(a), np.isnan(b)), (name, m)
            assert np.all(np.abs(a - b)[~np.isnan(a)] <= CORRELATION_BAR), (name, m)


# ------------------------------------------------------------------ configuration and command line
def hic_cfg(**runtime_or_lists):
    cfg = {'restraints': {'Hi-C': {'input_matrix': 'in/matrix.hcs', 'contact_range': 2.0}}}
    for k, v in runtime_or_lists.items():
        if k.startswith('runtime_'):
            cfg.setdefault('runtime', {}).setdefault('Hi-C', {})[k[len('runtime_'):]] = v
        else:
            cfg['restraints']['Hi-C'][k] = v
    return cfg


def test_parameters_from_config_sigma_sources(tmp_path):
    base = str(tmp_path)
    lists = {'inter_sigma_list': [1.0, 0.2, 0.02], 'intra_sigma_list': [1.0, 0.05], 'sigma_list': [1.0, 0.3]}
    p = RP.parameters_from_config(hic_cfg(runtime_inter_sigma=0.01, runtime_intra_sigma=0.04, runtime_sigma=0.5,
                                          **lists), base)['hic']
    assert (p['inter_sigma'], p['intra_sigma']) == (0.01, 0.04)            # runtime/Hi-C/{inter,intra}_sigma first
    assert p['input_matrix'] == str(tmp_path / 'in' / 'matrix.hcs') and p['contact_range'] == 2.0
    p = RP.parameters_from_config(hic_cfg(runtime_sigma=0.5, **lists), base)['hic']
    assert (p['inter_sigma'], p['intra_sigma']) == (0.5, 0.5)              # then the old runtime/Hi-C/sigma
    p = RP.parameters_from_config(hic_cfg(**lists), base)['hic']
    assert (p['inter_sigma'], p['intra_sigma']) == (0.02, 0.05)            # then the last entries of the lists
    p = RP.parameters_from_config(hic_cfg(sigma_list=[1.0, 0.3]), base)['hic']
    assert (p['inter_sigma'], p['intra_sigma']) == (0.3, 0.3)              # then the old sigma_list
    p = RP.parameters_from_config(hic_cfg(), base)['hic']
    assert (p['inter_sigma'], p['intra_sigma']) == (None, None)
    absolute = hic_cfg()
    absolute['restraints']['Hi-C']['input_matrix'] = '/data/m.hcs'
    assert RP.parameters_from_config(absolute, base)['hic']['input_matrix'] == '/data/m.hcs'
    assert 'hic' not in RP.parameters_from_config({'restraints': {}}, base)


def test_command_line_precedence(tmp_path):
    prm = RP.parameters_from_config(hic_cfg(runtime_inter_sigma=0.01, runtime_intra_sigma=0.04), str(tmp_path))
    h = RP.apply_hic_arguments(prm)['hic']
    assert (h['inter_sigma'], h['intra_sigma'], h['contact_range']) == (0.01, 0.04, 2.0)
    h = RP.apply_hic_arguments(prm, hic_sigma=0.2)['hic']
    assert (h['inter_sigma'], h['intra_sigma']) == (0.2, 0.2)
    h = RP.apply_hic_arguments(prm, hic_sigma=0.2, hic_inter_sigma=0.3)['hic']   # the specific flag wins
    assert (h['inter_sigma'], h['intra_sigma']) == (0.3, 0.2)
    h = RP.apply_hic_arguments(prm, hic_sigma=0.2, hic_intra_sigma=0.1, hic_contact_range=1.5)['hic']
    assert (h['inter_sigma'], h['intra_sigma'], h['contact_range']) == (0.2, 0.1, 1.5)
    h = RP.apply_hic_arguments(prm, hic='other.hcs')['hic']
    assert h['input_matrix'].endswith('/other.hcs') and h['inter_sigma'] == 0.01
    assert prm['hic']['input_matrix'] == str(tmp_path / 'in' / 'matrix.hcs')      # the input is not modified
    # without a Hi-C section the sigmas are ignored; --hic opens one
    assert 'hic' not in RP.apply_hic_arguments({'semiaxes': None}, hic_sigma=0.2)
    h = RP.apply_hic_arguments({'semiaxes': None}, hic='m.hcs', hic_sigma=0.2, hic_contact_range=2.0)['hic']
    assert (h['inter_sigma'], h['intra_sigma'], h['contact_range']) == (0.2, 0.2, 2.0)


# ------------------------------------------------------------------ the .hcs writer
def test_write_hcs_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    c = rng.integers(0, 9, (7, 7))
    c = (np.triu(c) + np.triu(c, 1).T).astype(np.int32)
    c[2, :] = c[:, 2] = 0                      # a row without entries
    chrom = np.array([0, 0, 0, 1, 1, 2, 2], np.int32)
    p = str(tmp_path / 'out.hcs')
    genome = {'assembly': 'test', 'chroms': np.array([b'chrA', b'chrB', b'chrC'], 'S10'),
              'lengths': np.array([3, 2, 2], np.int32), 'origins': np.zeros(3, np.int32)}
    hss.write_hcs(p, c, nstruct=6, chrom=chrom, genome=genome)
    m = hss.read_hcs(p)
    want = np.clip(c, 0, 6) / np.float64(6)
    assert m['nbin'] == 7 and np.array_equal(m['chrom'], chrom)
    assert m['data'].dtype == np.float32 and np.all(m['data'] != 0)
    assert np.array_equal(R.dense_input(m), want.astype(np.float32))
    rows = np.repeat(np.arange(7), np.diff(m['indptr']))
    assert np.all(m['indices'] >= rows) and m['indptr'][3] == m['indptr'][2]
    from igm_amd import h5
    with h5.File(p) as f:
        assert [bytes(v) for v in f.read('genome/chroms')] == [b'chrA', b'chrB', b'chrC']
        assert 'copy_index' in f.keys('index')
    # probabilities are stored as given
    hss.write_hcs(p, want, chrom=chrom)
    assert np.array_equal(R.dense_input(hss.read_hcs(p)), want.astype(np.float32))
    with pytest.raises(ValueError):
        hss.write_hcs(p, c, chrom=chrom)       # counts without nstruct
    with pytest.raises(ValueError):
        hss.write_hcs(p, want[:3], chrom=chrom)


def test_write_hcs_read_by_libhdf5(tmp_path):
    h5py = pytest.importorskip('h5py')
    c = np.array([[3, 1, 0], [1, 0, 2], [0, 2, 5]], np.int32)
    p = str(tmp_path / 'out.hcs')
    hss.write_hcs(p, c, nstruct=4, chrom=[0, 0, 1])
    with h5py.File(p, 'r') as f:
        assert int(f.attrs['nbin']) == 3
        assert f['matrix/indptr'][:].tolist() == [0, 2, 3, 4] and f['matrix/indices'][:].tolist() == [0, 1, 2, 2]
        assert f['matrix/data'][:].tolist() == [0.75, 0.25, 0.5, 1.0]
        assert f['index/chrom'][:].tolist() == [0, 0, 1]


# ------------------------------------------------------------------ the report step
@pytest.fixture
def cpu_report(monkeypatch):
    """igm_amd.report with the contact kernel and igm_report_hic answered by the restatement"""
    from igm_amd import evaluation

    def haploid_counts(xyz, radii, contact_range, copy_ptr, copy_idx, ctx=None, device=0):
        return R.contact_counts(xyz, radii, contact_range, copy_ptr, copy_idx)

    def hic_statistics(counts, nstruct, matrix, hap_chrom, intra_sigma=None, inter_sigma=None, log_edges=None,
                       lin_edges=None, nchrom=None, flags=0, ctx=None, device=0):
        return R.statistics(counts, nstruct, matrix, hap_chrom, intra_sigma, inter_sigma, log_edges, lin_edges, nchrom)

    monkeypatch.setattr(evaluation, 'haploid_counts', haploid_counts)
    monkeypatch.setattr(RP, 'hic_statistics', hic_statistics)
    return RP


def small_case(tmp_path, config=None):
    """13 beads: chrA with two copies of 5 loci, chrB with 3 single loci; a random matrix"""
    hap_chrom = np.array([0] * 5 + [1] * 3, np.int32)
    chrom = np.concatenate([hap_chrom, hap_chrom[:5]]).astype(np.int32)
    copy = np.array([0] * 8 + [1] * 5, np.int32)
    copy_ptr = np.array([0, 2, 4, 6, 8, 10, 11, 12, 13], np.int32)
    copy_idx = np.array([0, 8, 1, 9, 2, 10, 3, 11, 4, 12, 5, 6, 7], np.int32)
    rng = np.random.default_rng(11)
    xyz = (rng.standard_normal((13, 6, 3)) * 700).astype(np.float32)
    radii = np.full(13, 200, np.float32)
    genome = {'assembly': 'test', 'chroms': np.array([b'chrA', b'chrB'], 'S10'),
              'lengths': np.array([5, 3], np.int32), 'origins': np.zeros(2, np.int32)}
    p = str(tmp_path / 'pop.hss')
    hss.write_hss(p, xyz, radii, hss.index_tree(chrom, copy, copy_ptr, copy_idx), genome=genome,
                  config_data=None if config is None else json.dumps(config))
    x = np.triu(rng.uniform(0.01, 1.0, (8, 8)), 1)
    (tmp_path / 'in').mkdir(exist_ok=True)
    hss.write_hcs(str(tmp_path / 'in' / 'matrix.hcs'), x + x.T, chrom=hap_chrom)
    return p, xyz, radii, copy_ptr, copy_idx, hap_chrom


def test_hic_step_files(cpu_report, tmp_path):
    cfg = hic_cfg(runtime_inter_sigma=0.4, runtime_intra_sigma=0.5)
    with open(tmp_path / 'igm-config.json', 'w') as f:  # found beside the .hss; the matrix path is relative to it
        json.dump(cfg, f)
    p, xyz, radii, cp, ci, hc = small_case(tmp_path)
    written = cpu_report.report_population(p, steps='hic', label='run')
    names = {'label.txt', 'matrix_comparison/outmap-run.hcs', 'matrix_comparison/intra_correlations-run.txt',
             'matrix_comparison/inter_correlations-run.txt', 'matrix_comparison/log_histogram2d-run.npy',
             'matrix_comparison/linear_histogram2d-run.npy'}
    assert set(written) == names
    out = tmp_path / 'QC_run' / 'matrix_comparison'
    matrix = hss.read_hcs(str(tmp_path / 'in' / 'matrix.hcs'))
    counts = R.contact_counts(xyz, radii, 2.0, cp, ci)
    x, y = R.dense_input(matrix), R.probabilities(counts, 6)
    corr = R.correlations(x, y, hc, 0.5, 0.4)
    intra, inter = RP.hic_correlation_texts(['chrA', 'chrB'], corr)
    assert (out / 'intra_correlations-run.txt').read_text() == intra
    assert (out / 'inter_correlations-run.txt').read_text() == inter
    assert intra.splitlines()[0] == '# chrom all imposed non_imposed' and intra.splitlines()[1].startswith('chrA   ')
    log_edges, lin_edges = RP.hic_edges()
    lg, li = np.load(out / 'log_histogram2d-run.npy'), np.load(out / 'linear_histogram2d-run.npy')
    assert lg.dtype == np.int64 and lg.shape == (100, 100) and li.dtype == np.int64 and li.shape == (99, 99)
    assert np.array_equal(lg, R.histogram(x, y, log_edges, log_edges))
    assert np.array_equal(li, R.histogram(x, y, lin_edges, lin_edges))
    om = hss.read_hcs(str(out / 'outmap-run.hcs'))
    assert np.array_equal(R.dense_input(om), y.astype(np.float32)) and np.array_equal(om['chrom'], hc)


def test_hic_step_without_sigmas_writes_nan_columns(cpu_report, tmp_path):
    p = small_case(tmp_path, config=hic_cfg())[0]  # the configuration stored in the .hss; no sigma anywhere
    cpu_report.report_population(p, steps=('hic',), out_dir=str(tmp_path / 'o'))
    lines = (tmp_path / 'o' / 'matrix_comparison' / 'intra_correlations.txt').read_text().splitlines()
    assert len(lines) == 3 and all(ln.split()[2:] == ['nan', 'nan'] for ln in lines[1:])
    assert all(np.isfinite(float(ln.split()[1])) for ln in lines[1:])
    inter = (tmp_path / 'o' / 'matrix_comparison' / 'inter_correlations.txt').read_text().splitlines()[1].split()
    assert np.isfinite(float(inter[0])) and inter[1:] == ['nan', 'nan']


def test_hic_step_command_line(cpu_report, tmp_path, capsys, monkeypatch):
    p = small_case(tmp_path)[0]
    seen = {}
    real = RP.hic_comparison

    def spy(pop, matrix, contact_range, intra_sigma=None, inter_sigma=None, *a, **k):
        seen.update(matrix=matrix, contact_range=contact_range, intra=intra_sigma, inter=inter_sigma)
        return real(pop, matrix, contact_range, intra_sigma, inter_sigma, *a, **k)

    monkeypatch.setattr(RP, 'hic_comparison', spy)
    matrix = str(tmp_path / 'in' / 'matrix.hcs')
    rc = RP.main([p, '--steps', 'hic', '-o', str(tmp_path / 'o'), '--hic', matrix, '--hic-sigma', '0.5',
                  '--hic-inter-sigma', '0.25', '--hic-contact-range', '2.5'])
    assert rc == 0
    assert seen == {'matrix': matrix, 'contact_range': 2.5, 'intra': 0.5, 'inter': 0.25}
    assert str(tmp_path / 'o' / 'matrix_comparison' / 'outmap.hcs') in capsys.readouterr().out.split()


def test_hic_step_needs_a_hic_section(cpu_report, tmp_path):
    p = small_case(tmp_path)[0]
    with pytest.raises(ValueError, match='hic step needs an input matrix'):
        cpu_report.report_population(p, steps='hic', out_dir=str(tmp_path / 'o'))
    with pytest.raises(ValueError, match='contact range'):
        cpu_report.report_population(p, steps='hic', out_dir=str(tmp_path / 'o'),
                                     hic=str(tmp_path / 'in' / 'matrix.hcs'))
    assert not (tmp_path / 'o').exists()


def test_step_names(cpu_report, tmp_path):
    assert RP.STEPS == ('rgs', 'shells', 'radials', 'damid', 'distance_map')  # the default is unchanged
    assert 'hic' not in RP.STEPS and RP.OPTIONAL_STEPS == ('hic',)
    p = small_case(tmp_path)[0]
    with pytest.raises(ValueError, match='unknown report steps'):
        cpu_report.report_population(p, steps='hic,violations', hic=str(tmp_path / 'in' / 'matrix.hcs'),
                                     hic_contact_range=2.0)
    import inspect
    assert inspect.signature(RP.report_population).parameters['steps'].default == RP.STEPS
