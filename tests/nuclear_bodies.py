"""Test helper for the nuclear-body restraints: a NumPy restatement of the reference's
two snormsq_exp forms (gendamid.py:17-47, the bead-to-lamina form GenDamid selects with;
NuclDamidActivationDistanceStep.py:78-110, the voxel-to-voxel form of the nuclear-body
A-step), pinned to nuclear_bodies_golden.npz in test_nuclear_bodies.py, and the CPU
selection backend of igm_amd.assemble built on it.  Every dtype is explicit, so the
arithmetic is the reference's NumPy 1.x arithmetic under any NumPy."""
import numpy as np

import os

import cpu_kernels as CK
from conftest import load_golden
from igm_amd import assemble as A
from igm_amd import model as M
from igm_amd import steps as ST
from igm_amd import volume as V
from igm_amd._lib import IGM_ATOM_ENV0, damid_row_dtype
from oracle import asteps as OA

MAP_KEYS = ('nvoxel', 'center', 'origin', 'grid', 'matrice')


def golden_maps():
    """[nucleus b0 (117^3), nucleolus b1 (37^3), second nucleolus n1 (31^3)]"""
    g, h = load_golden('volume_golden.npz'), load_golden('nuclear_bodies_golden.npz')
    maps = [dict(body_idx=b, **{k: g['b%d_%s' % (b, k)] for k in MAP_KEYS}) for b in (0, 1)]
    maps.append(dict(body_idx=1, **{k: h['n1_%s' % k] for k in MAP_KEYS}))
    return maps


def snormsq_exp(x, vol, nucl=False):
    """x (..., 3) float32 -> float64 squared distances; nucl: voxel to voxel inside the grid"""
    x = np.asarray(x, np.float32)
    o, g, c = (np.asarray(vol[k], np.float32).astype(np.float64) for k in ('origin', 'grid', 'center'))
    n = np.asarray(vol['nvoxel'], np.int64)
    xd = x.astype(np.float64)
    v = np.round((xd - o) / g).astype(np.int64)  # np.round: half to even
    inside = np.all((v >= 0) & (v < n), axis=-1)
    w = np.clip(v, 0, n - 1)
    edt = np.asarray(vol['matrice'])[w[..., 0], w[..., 1], w[..., 2], :3].astype(np.int64)
    if nucl:
        t_in = (v - edt).astype(np.float64) * g
    else:
        t_in = xd - (edt.astype(np.float64) * g + o)
    t_out = (v.astype(np.float64) - c) * g  # mixed units, as the reference
    t = np.where(inside[..., None], t_in, t_out)
    return (t[..., 0] * t[..., 0] + t[..., 2] * t[..., 2]) + t[..., 1] * t[..., 1], inside


def volume_select_rows(x, rows, vols, pool_index):
    """(S, nrows) bool: GenDamid's test snormsq_exp(x[s, loc]) < d**2 per row; d is a NumPy
    float32 scalar in the reference and d**2 (scalar with a Python int, NumPy 1.x) is
    float64(d)**2 -- the golden's boundary rows tell it from the float32 square"""
    loc = np.asarray(rows['loc'], np.int64)
    d = np.asarray(rows['dist'], np.float32).astype(np.float64)
    d2 = d * d
    out = np.zeros((x.shape[0], len(loc)), bool)
    for s in range(x.shape[0]):
        key, _ = snormsq_exp(x[s, loc], vols[int(pool_index[s])])
        out[s] = key < d2
    return out


def volume_select(x, rows, vols, pool_index, env_index, base):
    base = np.asarray(base, np.uint32)
    out = np.repeat(base[None], x.shape[0], 0) if base.ndim == 1 else base.copy()
    sel = volume_select_rows(x, rows, vols, pool_index)
    loc = np.asarray(rows['loc'], np.int64)
    for s in range(x.shape[0]):
        out[s, loc[sel[s]]] |= np.uint32(IGM_ATOM_ENV0 << env_index)
    return out


def _clean(pij, pexist):
    """cleanProbability; a float32 scalar with a Python float is float64 under NumPy 1.x"""
    pij, pexist = float(pij), float(pexist)
    if pexist < 1:
        pclean = (pij - pexist) / (1.0 - pexist)
    else:
        pclean = pij
    return max(0, pclean)


def nucl_damid_actdist(crd, copy_ptr, copy_idx, loci, pexp, plast, it_corr, contact_range, vols, volumes_idx):
    """get_damid_actdist_exp (NuclDamidActivationDistanceStep.py:476-570) + the
    '%6d %.5f %.5f' round trip; crd (nbead, S, 3) float32, pexp / plast per listed locus"""
    S = crd.shape[1]
    vidx = np.asarray(volumes_idx)
    rows = []
    for q, I in enumerate(loci):
        ii = [int(v) for v in copy_idx[copy_ptr[I]:copy_ptr[I + 1]]]
        n = len(ii) * S
        d_sq = np.zeros((len(ii), S))
        for m in sorted(set(vidx.tolist())):
            where = np.where(vidx == m)[0]
            d_sq[:, where] = snormsq_exp(crd[ii][:, where], vols[m], nucl=True)[0]
        d_sq = np.sort(d_sq.ravel())
        if it_corr == 1:
            pnow = float(np.count_nonzero(d_sq >= contact_range)) / n
            p = _clean(pexp[q], _clean(pnow, plast[q]))
        else:
            p = float(pexp[q])
        ad = 1e-9
        if p > 0:
            ad = float(np.sqrt(d_sq[min(n - 1, int(np.round(np.float64(n) * p)))]))
        for i in ii:
            a, b, c = ('%6d %.5f %.5f' % (i, ad, p)).split()
            rows.append((int(a), np.float32(float(b)), np.float32(float(c))))
    out = np.zeros(len(rows), damid_row_dtype)
    if rows:
        out['loc'], out['dist'], out['prob'] = zip(*rows)
    return out


class BodiesSelect(CK.OracleSelect):
    """CK.OracleSelect plus the nuclear-body selections on the restatement above; keeps
    the staged pool and the per-envelope tables for the tests to look at."""

    def __init__(self):
        self.pool, self.struct_map, self.tables = None, None, {}

    def volumes(self, vols, struct_map):
        self.pool, self.struct_map, self.tables = list(vols), struct_map, {}

    def envelope_maps(self, env_index, pool_index):
        self.tables[env_index] = np.asarray(pool_index, np.int32).copy()

    def volume_select(self, x, rows, pool_index, env_index, base):
        return volume_select(x, rows, self.pool, pool_index, env_index, base)


def batch_digest(b, strip=''):
    """sha256 per piece of an assemble.Batch (arrays as bytes, names with the directory
    `strip` removed): what test_nuclear_bodies.py compares with the values recorded from
    the commit before the nuclear-body sections existed"""
    import hashlib
    import json
    out = {}
    for key in ('x', 'radii', 'flags', 'poly', 'poly_cls', 'ptr', 'bonds', 'bcls', 'class_cr', 'env_scale', 'active'):
        a = np.ascontiguousarray(getattr(b, key))
        out[key] = '%s %s %s' % (a.dtype.str, list(a.shape), hashlib.sha256(a.tobytes()).hexdigest())
    out['prm'] = hashlib.sha256(bytes(b.prm)).hexdigest()
    out['names'] = json.loads(json.dumps(b.names).replace(strip, '<dir>')) if strip else b.names
    out['layout'] = [int(b.nbead), int(b.natom), int(b.nslot), int(b.centre)]
    out['nvolumes'] = 0 if b.volumes is None else len(b.volumes)
    return out


def parent_case(tmp, config):
    """the Batch of configuration D / E of test_steps_de.py after its A-steps, on the CPU
    oracle kernels: (batch, selection backend calls)"""
    import test_steps_de as TD
    from igm_amd import igm_run as RUN
    cfg, _ = (TD._config_D if config == 'D' else TD._config_E)(tmp)
    for Step in RUN.iteration_steps(cfg)[:-1]:  # every A-step; ModelingStep is assembled below
        Step(cfg).run()
    store = ST.PopulationStore(cfg['optimization']['structure_output'])
    sids = np.arange(TD.S)
    calls = []

    class Recording(CK.OracleSelect):
        def __getattribute__(self, name):
            if not name.startswith('_'):
                calls.append(name)
            return CK.OracleSelect.__getattribute__(self, name)

    b = A.build(ST.batch_coordinates(store, sids), sids, store, ST.modeling_spec(cfg, sids), None, select=Recording())
    CK.oracle.set_volume(None)
    return b, calls


# ---------------------------------------------------------------- inputs shared by the CPU and GPU tests
def golden_rows(gold):
    r = np.zeros(len(gold['loc']), damid_row_dtype)
    r['loc'], r['dist'] = gold['loc'], gold['dist']
    return r


def _steps_de():
    import test_steps_de as TD
    return TD


def index_of(pop):
    import types
    return types.SimpleNamespace(radii=pop['radii'], chrom=pop['chrom'], copy=pop['copy'], copy_ptr=pop['copy_ptr'],
                                 copy_idx=pop['copy_idx'])


def four_envelope_spec(gold, maps, protocol=None):
    """exp_map nucleus (b0) + nucleolus (b1) + nuclDamID + DamID on the golden rows"""
    rows = golden_rows(gold)
    return {'evfactor': 1.0, 'protocol': protocol or {'mdsteps': 10, 'tstart': 1, 'tstop': 1},
            'polymer': {'contact_range': 2.0, 'kspring': 1.0},
            'envelope': {'shape': 'exp_map', 'k': 1.0, 'repr_k': 1.0, 'volumes': [maps[0]], 'files': ['nuc_0.bin'],
                         'struct_map': np.zeros(4, np.int32)},
            'nucleolus': {'shape': 'exp_map', 'k': 2.0, 'repr_k': 2.0, 'volumes': [maps[1]],
                          'files': ['nucleolus_3.bin'], 'struct_map': np.zeros(4, np.int32)},
            'nucldamid': {'rows': rows, 'contact_range': 0.9, 'k': 0.5, 'repr_cr': 0.9, 'repr_k': 0.5},
            'damid': {'rows': rows, 'contact_range': 0.05, 'k': 0.05, 'repr_cr': 0.05, 'repr_k': 0.05}}


def bodies_config(tmp, S=6):
    """exp_map nucleus + Hi-C + DamID + nucleolus + nuclDamID on the demo population"""
    V.write_volume(os.path.join(tmp, 'nuc_0.bin'), V.sphere_map(5500.0, 250.0))
    V.write_volume(os.path.join(tmp, 'body_0.bin'), V.sphere_map(1500.0, 250.0, body_idx=1, center=(1000.0, 0.0, 500.0)))
    V.write_volume(os.path.join(tmp, 'body_1.bin'), V.sphere_map(1200.0, 250.0, body_idx=1, center=(-1500.0, 800.0, 0.0)))
    cfg, pop = _steps_de()._base(tmp, {'nucleus_shape': 'exp_map', 'volume_prefix': os.path.join(tmp, 'nuc_'),
                              'volumes_idx': [0], 'nucleus_kspring': 1.0}, S=S)
    cfg['model']['restraints']['nucleolus'] = {'nucleus_shape': 'exp_map', 'volume_prefix': os.path.join(tmp, 'body_'),
                                               'volumes_idx': [s % 2 for s in range(S)], 'nucleus_kspring': 1.0}
    prof = os.path.join(tmp, 'damid_profile.txt')
    np.savetxt(prof, np.random.default_rng(1).beta(2.0, 5.0, len(pop['copy_ptr']) - 1).astype(np.float32))
    cfg['restraints']['DamID'] = {'input_profile': prof, 'sigma_list': [0.6, 0.45], 'contact_range': 0.95,
                                  'contact_kspring': 1.0, 'tmp_dir': 'damid'}
    nprof = os.path.join(tmp, 'nucldamid_profile.txt')
    np.savetxt(nprof, np.random.default_rng(2).beta(2.0, 5.0, len(pop['copy_ptr']) - 1).astype(np.float32))
    cfg['restraints']['nuclDamID'] = {'input_profile': nprof, 'sigma_list': [0.6, 0.45], 'contact_range': 0.95,
                                      'contact_kspring': 1.0}
    return cfg, pop


def _cpu_damid_exp(store, loci, pexp, plast, cfg, device):
    env = ST.envelope_section(cfg, range(store.coordinates().shape[1]))
    return OA.damid_actdist_exp(np.ascontiguousarray(store.coordinates()), store.copy_ptr, store.copy_idx, loci, pexp,
                                plast, int(ST.cget(cfg, 'runtime/DamID/iter_corr_knob', 1)),
                                float(ST.rget(cfg, 'restraints/DamID/contact_range', 0.95)), env['volumes'],
                                env['struct_map'])


def _cpu_nucldamid(store, loci, pexp, plast, cfg, device):
    nu = ST.nucleolus_section(cfg, range(store.coordinates().shape[1]))
    return nucl_damid_actdist(np.ascontiguousarray(store.coordinates()), store.copy_ptr, store.copy_idx, loci, pexp,
                                 plast, int(ST.cget(cfg, 'runtime/nuclDamID/iter_corr_knob', 1)),
                                 float(ST.rget(cfg, 'restraints/nuclDamID/contact_range', 0.95)), nu['volumes'],
                                 nu['struct_map'])


BUILT = []


def _cpu_assemble_only(store, sids, cfg, device):
    """ModelingStep's kernel without the optimisation (the CPU oracle holds one map): the
    assembly on the restatement backend, coordinates unchanged, n_imposed per class"""
    from igm_amd._lib import optinfo_dtype
    b = A.build(ST.batch_coordinates(store, sids), sids, store, ST.modeling_spec(cfg, sids), None,
                select=BodiesSelect())
    BUILT.append(b)
    ncls = len(b.class_cr) + b.prm.nenvelopes
    stats = np.zeros((len(sids), ncls, 104), np.int64)
    for q in range(len(sids)):
        stats[q, :A.NCLASS, 103] = np.bincount(b.bcls[b.ptr[q]:b.ptr[q + 1]], minlength=A.NCLASS)[:A.NCLASS]
        stats[q, M.CLASS_POLYMER, 103] += len(b.poly)
        for e in range(b.prm.nenvelopes):
            stats[q, A.NCLASS + e, 103] = np.count_nonzero(b.flags[q] & (IGM_ATOM_ENV0 << e))
    return {'xyz': b.x[:, :b.nbead], 'info': np.zeros(len(sids), optinfo_dtype), 'stats': stats,
            'names': [b.vstat_names(q) for q in range(len(sids))]}


def register_cpu_kernels():
    """optimization/kernel = 'nuclear_bodies_test': the CPU oracle kernels with the exp_map
    DamID A-steps on the restatements and ModelingStep reduced to its assembly; a test calls
    this itself, nothing is registered on import"""
    ST.KERNELS['nuclear_bodies_test'] = dict(ST.KERNELS['cpu_oracle_test'], damid=_cpu_damid_exp,
                                             nucldamid=_cpu_nucldamid, mstep=_cpu_assemble_only)
