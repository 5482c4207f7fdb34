"""Host-side helpers of bench.py (no GPU): the warmup protocol of the config C block, the
force-evaluation count the roofline's algorithmic bytes are priced on, the --full switch
and the --dump-outputs writer."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from igm_amd import model as M  # noqa: E402
from igm_amd import synthetic as syn  # noqa: E402


@pytest.fixture
def prm():
    return M.params_from_cfg({'optimization': {'optimizer_options': syn.DEMO_PROTOCOL}}, [((5500.0,) * 3, 1.0)])


def test_scaled_prm_scales_md_steps_only(prm):
    w = bench._scaled_prm(prm, 0.1)
    cap = syn.DEMO_PROTOCOL['custom_annealing_protocol']
    assert w.nstages == prm.nstages == len(cap['mdsteps'])
    assert [w.mdsteps[k] for k in range(w.nstages)] == [round(n * 0.1) for n in cap['mdsteps']]
    assert w.relax_steps == round(cap['relax']['mdsteps'] * 0.1)
    # the original is untouched (the timed iteration runs it) and everything else is copied
    assert [prm.mdsteps[k] for k in range(prm.nstages)] == cap['mdsteps']
    assert bytes(bench._scaled_prm(prm, 1.0)) == bytes(prm)
    for name, _ in type(prm)._fields_:
        if name not in ('mdsteps', 'relax_steps'):
            a, b = getattr(w, name), getattr(prm, name)
            assert (bytes(a) == bytes(b)) if hasattr(a, '_length_') else a == b, name


def test_scaled_prm_keeps_one_step(prm):
    w = bench._scaled_prm(prm, 1e-6)
    assert all(w.mdsteps[k] == 1 for k in range(w.nstages)) and w.relax_steps == 1


def test_evaluations_counts_setup_steps(prm):
    # every run (relax + stage) evaluates its forces nsteps + 1 times (Verlet::setup + steps)
    cap = syn.DEMO_PROTOCOL['custom_annealing_protocol']
    n = sum(s + 1 for s in cap['mdsteps']) + len(cap['mdsteps']) * (cap['relax']['mdsteps'] + 1)
    assert bench._evaluations(prm) == n


def test_bench_defaults(monkeypatch):
    monkeypatch.setattr(sys, 'argv', ['bench.py'])
    a = bench.parse()
    assert a.gpus == 1 and a.c_warmup == 1 and a.c_warmup_scale == 0.1 and a.c_shard == 125
    assert a.protocol_scale == 1.0 and a.config == 'B' and a.nstruct == 1000
    # a plain run times its steps only: everything that takes runs of its own waits for --full
    assert a.full is False and a.dump_outputs is None


def test_bench_full_and_dump_options(monkeypatch):
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '3', '--warmup', '2', '--full',
                                      '--dump-outputs', 'some/dir'])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == 'some/dir' and a.steps == 3 and a.warmup == 2


def test_sample_rows_is_fixed_and_bounded():
    a = np.arange(1000 * 7 * 3, dtype=np.float32).reshape(1000, 7, 3)
    whole, idx = bench.sample_rows(a, a.nbytes)
    assert whole is a and idx is None
    s1, i1 = bench.sample_rows(a, 10000)
    s2, i2 = bench.sample_rows(a.copy(), 10000)
    assert np.array_equal(i1, i2) and np.array_equal(s1, s2)  # the same rows from run to run
    assert s1.nbytes + 8 * len(i1) <= 10000 and len(i1) == 10000 // (7 * 3 * 4 + 8)
    assert np.all(np.diff(i1) > 0) and np.array_equal(s1, a[i1])


def test_dump_outputs_writes_float_arrays_of_the_last_step(tmp_path, monkeypatch):
    import types

    import torch
    from igm_amd._lib import optinfo_dtype, row_dtype
    S, natom = 6, 11
    rng = np.random.default_rng(3)
    rows = np.zeros(9, row_dtype)
    rows['row'], rows['col'] = np.arange(9), np.arange(9) + 20
    rows['dist'], rows['prob'] = rng.random(9), rng.random(9)
    info = np.zeros(S, optinfo_dtype)
    info['final_energy'], info['env_energy'], info['nrebuild'] = rng.random(S), rng.random((S, 4)), np.arange(S)
    it = types.SimpleNamespace(
        xyz=torch.from_numpy(rng.standard_normal((S, natom, 3)).astype(np.float32)),
        rows=torch.from_numpy(np.concatenate([rows.view(np.uint8), np.zeros(32, np.uint8)])), nrows=len(rows),
        info=torch.from_numpy(info.view(np.uint8).copy()),
        stats=torch.from_numpy(rng.integers(0, 1000, (S, 4, 104))))
    out = tmp_path / 'dump'
    files = bench.dump_outputs(it, str(out))
    assert sorted(os.path.basename(f) for f in files) == ['actdist_rows.npy', 'coordinates.npy', 'optinfo.npy',
                                                          'violation_stats.npy']
    got = {os.path.basename(f)[:-4]: np.load(f) for f in files}
    assert got['coordinates'].dtype == np.float32 and np.array_equal(got['coordinates'], it.xyz.numpy())
    assert got['actdist_rows'].dtype == np.float64 and got['actdist_rows'].shape == (9, 4)
    assert np.array_equal(got['actdist_rows'][:, 1], rows['col']) and np.array_equal(
        got['actdist_rows'][:, 2], rows['dist'].astype(np.float64))
    assert got['optinfo'].dtype == np.float64 and got['optinfo'].shape == (S, 14)
    assert np.array_equal(got['optinfo'][:, 3:7], info['env_energy'])
    assert np.array_equal(got['optinfo'][:, 13], np.arange(S))
    assert got['violation_stats'].dtype == np.float64 and np.array_equal(got['violation_stats'], it.stats.numpy())
    # an output over its share is cut to the seeded sample, with the rows' indices beside it
    monkeypatch.setattr(bench, 'DUMP_COORD_BYTES', 3 * (natom * 3 * 4 + 8))
    files = bench.dump_outputs(it, str(out), rank=1, world=2)
    assert all(f.endswith('_rank1.npy') for f in files)
    idx = np.load(str(out / 'coordinates_index_rank1.npy'))
    assert idx.dtype == np.float64 and len(idx) == 3
    assert np.array_equal(np.load(str(out / 'coordinates_rank1.npy')), it.xyz.numpy()[idx.astype(int)])
