"""Population report, host side (no GPU): the float64 restatement tests/report_ref.py
against the reference's own numbers (report_golden.npz, made by
golden/make_golden_report.py from igm/report/*.py on the demo population), and the host
layer of igm_amd.report -- file names and formats of report_population, the semiaxes
resolution order, the argument errors -- with the native calls replaced by the
restatement.  The kernels themselves are tested in test_report_gpu.py."""
import json
import os

import numpy as np
import pytest

import report_ref as R
from conftest import load_golden
from igm_amd import report as RP

U53 = 2.0 ** -53
F32_SUM_BAR = 32 * 2.0 ** -24  # float32 pairwise sum of <= 128 terms + division, square, sqrt roundings


@pytest.fixture(scope='module')
def pop():
    return load_golden('demo_population.npz')


@pytest.fixture(scope='module')
def gold():
    return load_golden('report_golden.npz')


def sub_index(pop, loci):
    """copy CSR of the haploid loci `loci` on the full population's beads"""
    cp, ci = pop['copy_ptr'], pop['copy_idx']
    ptr = np.concatenate([[0], np.cumsum([cp[h + 1] - cp[h] for h in loci])]).astype(np.int32)
    idx = np.concatenate([ci[cp[h]:cp[h + 1]] for h in loci]).astype(np.int32)
    return ptr, idx


def test_golden_records_numpy_2(gold):
    assert str(gold['numpy_version']).startswith('2.')
    for k in ('max_rel_rg', 'max_rel_dmap'):
        assert gold[k] <= F32_SUM_BAR


def test_radial_levels_bit_equal(pop, gold):
    lev = R.level_mean(pop['coordinates'], gold['semiaxes'])
    got = RP.average_copies(lev, pop['copy_ptr'], pop['copy_idx'])
    assert got.tobytes() == gold['radial_level'].tobytes()


def test_density_counts_equal(pop, gold):
    edges = np.linspace(0, 1.1, 12)
    counts = R.histogram(R.levels(pop['coordinates'], gold['semiaxes']), edges)
    volumes = np.array([edges[i + 1]**3 - edges[i]**3 for i in range(11)])
    assert (counts / volumes).tobytes() == gold['density_histo'].tobytes()


def test_shell_means(pop, gold):
    n = pop['coordinates'].shape[0]
    smean, _ = R.shells(pop['coordinates'], gold['semiaxes'], 5)
    got = np.average(smean, axis=0)
    bar = 2 * (n // 5 + 1) * U53 + 2 * 100 * U53  # the shell sums, then the mean over 100 structures
    assert np.max(np.abs(got - gold['ave_radial']) / gold['ave_radial']) <= bar


def test_lamina_counts_equal(pop, gold):
    cp, ci = pop['copy_ptr'], pop['copy_idx']
    den = R.lamina_denoms(gold['semiaxes'], float(gold['contact_range']), pop['radii'], cp, ci)
    assert np.array_equal(den, RP.lamina_denominators(gold['semiaxes'], float(gold['contact_range']), pop['radii'],
                                                      cp, ci))
    counts = R.lamina_counts(pop['coordinates'], cp, ci, den)
    freq = counts.astype(np.float64) / 100 / np.diff(cp)
    assert freq.tobytes() == gold['damid_output'].tobytes()
    assert counts.sum() > 0


def test_rg_within_float32_sum(pop, gold):
    ids, chrom_ptr, chain_ptr, chain_idx = RP.chains(pop['chrom'], pop['copy'])
    rg = R.rg(pop['coordinates'], chain_ptr, chain_idx)
    assert np.array_equal(gold['rgs_ptr'], chrom_ptr * 100)
    want = gold['rgs_values'].astype(np.float64)
    assert np.max(np.abs(rg.ravel() - want) / want) <= F32_SUM_BAR


def test_distance_means_within_float32_sum(pop, gold):
    loci = gold['dmap_loci']
    ptr, idx = sub_index(pop, loci)
    d = R.distance_map(pop['coordinates'], ptr, idx, pop['hap_chrom'][loci])
    iu = np.triu_indices(len(loci), 1)
    assert np.max(np.abs(d[iu] - gold['dmap'][iu]) / gold['dmap'][iu]) <= F32_SUM_BAR
    assert np.array_equal(d, d.T) and not d.diagonal().any()


def test_histogram_is_np_histogram():
    rng = np.random.default_rng(0)
    edges = np.linspace(0, 1.5, 151)
    v = np.concatenate([rng.uniform(-0.1, 1.7, 5000), edges, np.nextafter(edges, 9), np.nextafter(edges, -9)])
    assert np.array_equal(R.histogram(v, edges), np.histogram(v, bins=150, range=(0, 1.5))[0])


def test_shell_bounds_and_empty_shells():
    xyz = np.arange(27, dtype=np.float32).reshape(3, 3, 3)
    smean, hist = R.shells(xyz, (10, 10, 10), 5, np.linspace(0, 10, 11))
    assert R.shell_bounds(3, 5) == [0, 0, 1, 1, 2, 3]
    assert np.isnan(smean[:, [0, 2]]).all() and np.isfinite(smean[:, [1, 3, 4]]).all()
    assert hist[[0, 2]].sum() == 0 and hist.sum() == 9


# ------------------------------------------------------------------ the host layer
@pytest.fixture
def cpu_report(monkeypatch):
    """igm_amd.report with its four native calls answered by the restatement"""
    def levels(xyz, semiaxes, ctx, device, want_mean=False, density_edges=None, nshell=0, shell_edges=None):
        sx = RP._semiaxes(semiaxes)
        mean = R.level_mean(xyz, sx) if want_mean else None
        dens = R.histogram(R.levels(xyz, sx), density_edges) if density_edges is not None else None
        smean, shist = R.shells(xyz, sx, nshell, shell_edges) if nshell else (None, None)
        return mean, dens, smean, shist

    def lamina_counts(pop, radii=None, copy_ptr=None, copy_idx=None, semiaxes=None, contact_range=0.05, **kw):
        den = RP.lamina_denominators(RP._semiaxes(semiaxes), contact_range, radii, copy_ptr, copy_idx)
        return R.lamina_counts(pop, copy_ptr, copy_idx, den), np.diff(copy_ptr)

    monkeypatch.setattr(RP, '_levels', levels)
    monkeypatch.setattr(RP, 'chain_rgs', lambda pop, p, i, **kw: R.rg(pop, p, i))
    monkeypatch.setattr(RP, 'lamina_counts', lamina_counts)
    monkeypatch.setattr(RP, 'average_distance_map', lambda pop, p, i, hc, **kw: R.distance_map(pop, p, i, hc))
    return RP


def small_hss(path, envelope=None, config=None, nstruct=4):
    """two chromosomes, the first with two copies: 5 + 3 haploid loci, 13 beads"""
    from igm_amd import hss
    hap_chrom = np.array([0] * 5 + [1] * 3, np.int32)
    chrom = np.concatenate([hap_chrom, hap_chrom[:5]]).astype(np.int32)
    copy = np.array([0] * 8 + [1] * 5, np.int32)
    copy_ptr = np.array([0, 2, 4, 6, 8, 10, 11, 12, 13], np.int32)
    copy_idx = np.array([0, 8, 1, 9, 2, 10, 3, 11, 4, 12, 5, 6, 7], np.int32)
    rng = np.random.default_rng(7)
    xyz = (rng.standard_normal((13, nstruct, 3)) * 2500).astype(np.float32)
    radii = np.full(13, 200, np.float32)
    genome = {'assembly': 'test', 'chroms': np.array([b'chrA', b'chrB'], 'S10'),
              'lengths': np.array([5, 3], np.int32), 'origins': np.zeros(2, np.int32)}
    hss.write_hss(path, xyz, radii, hss.index_tree(chrom, copy, copy_ptr, copy_idx), genome=genome,
                  envelope=envelope, config_data=None if config is None else json.dumps(config))
    return xyz, radii, copy_ptr, copy_idx, hap_chrom


def test_report_population_files(cpu_report, tmp_path):
    p = str(tmp_path / 'pop.hss')
    xyz, radii, cp, ci, hc = small_hss(p, envelope={'shape': 'ellipsoid', 'volume': np.float64(1.0),
                                                    'params': np.array([5000.0, 4000.0, 3000.0])})
    profile = tmp_path / 'damid.txt'
    np.savetxt(profile, np.linspace(0.1, 0.8, 8))
    cfg = {'restraints': {'DamID': {'input_profile': 'damid.txt', 'contact_range': 0.05}}}
    with open(tmp_path / 'igm-config.json', 'w') as f:  # found beside the .hss; the profile path is relative to it
        json.dump(cfg, f)
    written = cpu_report.report_population(p, label='run')
    out = tmp_path / 'QC_run'
    names = {'label.txt', 'radius_of_gyration/chromosomes-run.npz', 'shells/ave_radial-run.txt',
             'radials/radials-run.txt', 'radials/density_histo-run.txt', 'radials/radials_norm-run.txt',
             'damid/output.txt', 'damid/input-run.txt', 'damid/pearsonr-run.txt', 'distance_map/average-run.npy'}
    assert set(written) == names
    for n in names:
        assert (out / n).is_file()
    sx = (5000.0, 4000.0, 3000.0)
    rgs = np.load(out / 'radius_of_gyration/chromosomes-run.npz')
    assert rgs.files == ['chrA', 'chrB'] and rgs['chrA'].shape == (8,) and rgs['chrB'].shape == (4,)
    radials = np.loadtxt(out / 'radials/radials-run.txt')
    assert np.array_equal(radials, RP.average_copies(R.level_mean(xyz, sx), cp, ci))
    ave = np.loadtxt(out / 'shells/ave_radial-run.txt')
    assert ave.shape == (5,) and np.all(np.diff(ave) > 0)
    assert np.array_equal(np.loadtxt(out / 'radials/radials_norm-run.txt'), radials / ave[-1])
    assert np.loadtxt(out / 'radials/density_histo-run.txt').shape == (11,)
    freq = np.loadtxt(out / 'damid/output.txt')
    assert freq.shape == (8,) and np.all((freq >= 0) & (freq <= 1))
    r = np.loadtxt(out / 'damid/pearsonr-run.txt')
    assert abs(np.atleast_1d(r)[0] - np.corrcoef(np.linspace(0.1, 0.8, 8).astype(np.float32), freq)[0, 1]) < 1e-12
    d = np.load(out / 'distance_map/average-run.npy')
    assert d.shape == (8, 8) and d.dtype == np.float64 and np.array_equal(d, d.T)
    assert (out / 'label.txt').read_text() == 'run'


def test_report_population_no_label_no_profile(cpu_report, tmp_path):
    p = str(tmp_path / 'igm-model.hss')
    small_hss(p)
    written = cpu_report.report_population(p, steps='radials,damid')
    out = tmp_path / 'QC_igm-model'
    assert set(written) == {'label.txt', 'radials/radials.txt', 'radials/density_histo.txt', 'damid/output.txt'}
    assert (out / 'radials/radials.txt').is_file() and not (out / 'radials/radials_norm.txt').exists()


def test_semiaxes_resolution_order(cpu_report, tmp_path):
    cfg = {'model': {'restraints': {'envelope': {'nucleus_shape': 'ellipsoid',
                                                 'nucleus_semiaxes': [4100.0, 4200.0, 4300.0]}}}}
    prm = RP.parameters_from_config(cfg)
    env = ('ellipsoid', np.array([5100.0, 5200.0, 5300.0]))
    assert RP.resolve_semiaxes(env, prm, (1.0, 2.0, 3.0)).tolist() == [1.0, 2.0, 3.0]      # explicit first
    assert RP.resolve_semiaxes(env, prm).tolist() == [5100.0, 5200.0, 5300.0]              # then the .hss
    assert RP.resolve_semiaxes(('sphere', np.array([4000.0])), prm).tolist() == [4000.0] * 3  # a scalar is a sphere
    assert RP.resolve_semiaxes((None, None), prm).tolist() == [4100.0, 4200.0, 4300.0]     # then the config
    radius = {'model': {'restraints': {'envelope': {'nucleus_shape': 'sphere', 'nucleus_radius': 5500.0}}}}
    assert RP.resolve_semiaxes((None, None), RP.parameters_from_config(radius)).tolist() == [5500.0] * 3
    assert RP.resolve_semiaxes((None, None), None).tolist() == [5000.0] * 3                # then 5000
    # end to end: the stored configuration is found in the .hss, the stored envelope wins over it
    p = str(tmp_path / 'a.hss')
    xyz, _, cp, ci, _ = small_hss(p, config=cfg)
    cpu_report.report_population(p, steps=('radials',), out_dir=str(tmp_path / 'a'))
    want = RP.average_copies(R.level_mean(xyz, (4100.0, 4200.0, 4300.0)), cp, ci)
    assert np.array_equal(np.loadtxt(tmp_path / 'a' / 'radials/radials.txt'), want)
    q = str(tmp_path / 'b.hss')
    xyz, _, cp, ci, _ = small_hss(q, envelope={'shape': 'sphere', 'volume': np.float64(1.0),
                                               'params': np.float64(4000.0)}, config=cfg)
    cpu_report.report_population(q, steps=('radials',), out_dir=str(tmp_path / 'b'))
    want = RP.average_copies(R.level_mean(xyz, (4000.0,) * 3), cp, ci)
    assert np.array_equal(np.loadtxt(tmp_path / 'b' / 'radials/radials.txt'), want)


def test_exp_map_needs_explicit_semiaxes(cpu_report, tmp_path):
    cfg = {'model': {'restraints': {'envelope': {'nucleus_shape': 'exp_map'}}}}
    p = str(tmp_path / 'e.hss')
    small_hss(p, envelope={'shape': 'exp_map', 'volume': np.float64(1.0), 'params': np.float64(4000.0)}, config=cfg)
    for step in ('radials', 'shells', 'damid'):
        with pytest.raises(ValueError, match='exp_map'):
            cpu_report.report_population(p, steps=(step,), out_dir=str(tmp_path / 'e'))
    assert not (tmp_path / 'e').exists()
    # the steps without an envelope run, and explicit semiaxes lift the error
    written = cpu_report.report_population(p, steps=('rgs', 'distance_map'), out_dir=str(tmp_path / 'e'))
    assert 'distance_map/average.npy' in written
    written = cpu_report.report_population(p, steps=('radials',), out_dir=str(tmp_path / 'e'),
                                           semiaxes=(4000.0, 4000.0, 3000.0))
    assert 'radials/radials.txt' in written


def test_argument_errors():
    xyz = np.zeros((4, 2, 3), np.float32)
    with pytest.raises(ValueError):
        RP.radial_levels(np.zeros((4, 2), np.float32), (1, 1, 1))
    for bad in ((1.0, 0.0, 1.0), (1.0, np.nan, 1.0), (1.0, 2.0), (-1.0, 1.0, 1.0)):
        with pytest.raises(ValueError, match='semiaxes'):
            RP.radial_levels(xyz, bad)
    with pytest.raises(ValueError):
        RP.radial_density(xyz, (1, 1, 1), n=0)
    with pytest.raises(ValueError):
        RP.shells(xyz, (1, 1, 1), nshell=0)
    with pytest.raises(ValueError, match='chain_ptr'):
        RP._csr([0, 3, 2], [0, 1], 4, 'chain')
    with pytest.raises(ValueError, match='outside'):
        RP._csr([0, 2], [0, 4], 4, 'copy')
    with pytest.raises(ValueError, match='required'):
        RP.average_distance_map(xyz)


def test_unknown_step(cpu_report, tmp_path):
    small_hss(str(tmp_path / 'u.hss'))
    with pytest.raises(ValueError, match='unknown report steps'):
        cpu_report.report_population(str(tmp_path / 'u.hss'), steps='radials,violations')


def test_command_line(cpu_report, tmp_path, capsys):
    p = str(tmp_path / 'pop.hss')
    small_hss(p)
    rc = RP.main([p, '-l', 'x', '--semiaxes', '5000', '5000', '4000', '--steps', 'shells,radials', '-o',
                  str(tmp_path / 'out')])
    assert rc == 0
    lines = capsys.readouterr().out.split()
    assert str(tmp_path / 'out' / 'radials' / 'radials_norm-x.txt') in lines
    assert (tmp_path / 'out' / 'shells' / 'ave_radial-x.txt').is_file()
