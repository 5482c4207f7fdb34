"""Chromatin tracing data in the M-step (igm/restraints/tracing.py; ModelingStep.py:281-300,
RelaxInit.py:186-207, RandomInit.py:70-102): every locus imaged in a cell is tied to its
imaged position by a harmonic upper bound of radius `tol`.

The reference adds one DUMMY_STATIC centroid per imaged locus and a bond to it; here the
restraint is a position anchor of the engine (igm_anchor, include/igm_hip.h): no atom is
added, so a traced 2 Mb structure stays in the LDS engine.  The M-step reads the assignment
file,

    locus       (n,)   diploid bead index
    target      (n, 3) imaged position in the model's frame
    assignment  (n,)   structure index the locus was imaged in

which is either an input (restraints/tracing/assignment_file) or the product of the A-step
below.  The reference has no A-step for tracing (bin/igm-run:122-136: its
ImagedLociAssignmentStep is commented out); this one takes the traces as they are imaged
(restraints/tracing/input_file),

    trace_ptr   (T + 1,) the spots of trace t are the entries trace_ptr[t] .. trace_ptr[t + 1]
    locus       (n,)     haploid locus of each spot, strictly increasing inside a trace, one
                         chromosome per trace
    position    (n, 3)   nm, in a frame of the trace's own

and decides, from the current population, which (structure, copy) each trace is:

  read_traces        the validated trace file
  assign_costs       the minimal RMSD under a proper rigid motion of every (trace, structure,
                     copy) and the keep_best cheapest candidates per trace, on the GPU
                     (igm_tracing_assign; no CPU fallback)
  greedy_assignment  every (structure, chromosome, copy) slot takes at most one trace: the
                     traces in ascending order of their best cost take their first free
                     candidate (host, deterministic)
  aligned_targets    the assigned traces superposed on their beads (Kabsch, fp64, host)
  write_assignment   the assignment file the M-step reads

Traces imaged in one cell share the cell's frame: with a fourth dataset

    cell_ptr    (Ncell + 1,) the traces of cell c are cell_ptr[c] .. cell_ptr[c + 1]; at most C
                             traces of a chromosome of C copies

a cell is placed as a whole -- one structure, one rigid motion, one homologue labelling:

  assign_cell_costs       per (cell, structure) the joint RMSD at the labelling an alternating
                          search ends at, the keep_best cheapest structures per cell and the
                          copy of every trace there, on the GPU (igm_tracing_assign_cells)
  greedy_cell_assignment  a structure is one cell: it takes at most one
  aligned_cell_targets    one Kabsch per assigned cell over all its spots
"""
import numpy as np

from ._lib import anchor_dtype

MIN_SPOTS = 3  # a rigid superposition of fewer spots says nothing


def read_assignment(path, nbead=None):
    """The assignment file as {'locus' (n,) int64, 'target' (n, 3) float64, 'assignment'
    (n,) int64}.  ValueError: mismatched lengths, a non-finite target, a locus outside
    [0, nbead) when nbead is given."""
    from . import h5
    with h5.File(path) as f:
        data = {k: np.asarray(f.read(k)) for k in ('locus', 'target', 'assignment')}
    return check_assignment(data, nbead)


def check_assignment(data, nbead=None):
    locus = np.asarray(data['locus']).astype(np.int64).reshape(-1)
    target = np.asarray(data['target'], np.float64)
    assignment = np.asarray(data['assignment']).astype(np.int64).reshape(-1)
    n = len(locus)
    if target.shape != (n, 3) or len(assignment) != n:
        raise ValueError('tracing assignment: locus %r, target %r and assignment %r do not match' % (
            (n,), target.shape, assignment.shape))
    if not np.all(np.isfinite(target)):
        raise ValueError('tracing assignment: non-finite target at entry %d' % int(
            np.where(~np.isfinite(target).all(axis=1))[0][0]))
    if nbead is not None and n and (locus.min() < 0 or locus.max() >= nbead):
        bad = int(np.where((locus < 0) | (locus >= nbead))[0][0])
        raise ValueError('tracing assignment: locus %d of entry %d is outside [0, %d)' % (locus[bad], bad, nbead))
    return {'locus': locus, 'target': target, 'assignment': assignment}


def anchors_for(data, sids, tol, k, nbead=None):
    """Tracing._apply (tracing.py:36-61) for the structures sids: (ptr (S+1) int64, anchors)
    -- the CSR of igm_anchor the engine takes; a structure's entries in file order
    (np.where(assignment == sid)), target rounded to float32 as a centroid's position is."""
    data = check_assignment(data, nbead)
    per = [np.where(data['assignment'] == int(sid))[0] for sid in sids]
    ptr = np.zeros(len(per) + 1, np.int64)
    ptr[1:] = np.cumsum([len(h) for h in per])
    a = np.zeros(int(ptr[-1]), anchor_dtype)
    here = np.concatenate(per) if per else np.zeros(0, np.int64)
    a['atom'] = data['locus'][here]
    a['x'], a['y'], a['z'] = (data['target'][here, d].astype(np.float32) for d in range(3))
    a['r0'] = float(tol)
    a['k'] = float(k)
    return ptr, a


def initial_coordinates(crd, data, sid, rng=None, init_noise=None):
    """RandomInit.task's tracing block (RandomInit.py:80-102) on one structure's territories
    crd (nbead, 3) float64, quirks included: the structure's targets are written in file
    order; between CONSECUTIVE ENTRIES of its list (file order, no chromosome test) with
    pin_2 - pin_1 > 1 the loci in between are put on the segment; init_noise * randn is
    added to every bead when model/init_noise is set (rng: the structure's RandomState)."""
    crd = np.array(crd, np.float64)
    locus, target = data['locus'], data['target']
    here = np.where(data['assignment'] == int(sid))[0]
    for j in here:
        crd[locus[j], :] = target[j]
    for i in range(len(here) - 1):
        p1, p2 = int(locus[here[i]]), int(locus[here[i + 1]])
        if p2 - p1 > 1:
            for m, q in enumerate(range(p1 + 1, p2)):
                crd[q, :] = crd[p1, :] + (m + 1) * (crd[p2, :] - crd[p1, :]) / (p2 - p1)
    if init_noise is not None:
        rng = np.random.mtrand._rand if rng is None else rng
        crd = crd + init_noise * rng.randn(crd.shape[0], 3)
    return crd


# ---------------------------------------------------------------------------- the A-step
def check_traces(data, copy_ptr, hap_chrom):
    """The trace arrays validated against the model's index: {'trace_ptr' (T + 1,) int64,
    'locus' (n,) int32, 'position' (n, 3) float32 -- the precision the device reads --,
    'chrom' (T,) the chromosome of every trace, 'ncopy' (T,) its number of copies, 'cell_ptr'
    (Ncell + 1,) int64 or None: the traces cell_ptr[c] .. cell_ptr[c + 1] were imaged in cell c
    and share its frame}.
    ValueError naming the first offending trace: a non-monotone trace_ptr, fewer than
    MIN_SPOTS spots, a locus outside [0, nhap), non-increasing loci, more than one chromosome,
    a non-finite position; naming the first offending cell: a cell_ptr that is not monotone,
    does not span the traces or has an empty cell, more traces of a chromosome than it has
    copies."""
    ptr = np.asarray(data['trace_ptr']).astype(np.int64).reshape(-1)
    locus = np.asarray(data['locus']).astype(np.int64).reshape(-1)
    position = np.asarray(data['position'], np.float64)
    copy_ptr = np.asarray(copy_ptr, np.int64)
    hap_chrom = np.asarray(hap_chrom)
    nhap = len(copy_ptr) - 1
    if len(ptr) < 1 or ptr[0] != 0:
        raise ValueError('tracing input: trace_ptr must start at 0')
    if position.shape != (len(locus), 3):
        raise ValueError('tracing input: locus %r and position %r do not match' % ((len(locus),), position.shape))
    T = len(ptr) - 1
    d = np.diff(ptr)
    if np.any(d < 0):
        raise ValueError('tracing input: trace_ptr is not monotone at trace %d' % int(np.where(d < 0)[0][0]))
    if ptr[-1] != len(locus):
        raise ValueError('tracing input: trace_ptr ends at %d, the file has %d spots' % (ptr[-1], len(locus)))
    if np.any(d < MIN_SPOTS):
        t = int(np.where(d < MIN_SPOTS)[0][0])
        raise ValueError('tracing input: trace %d has %d spots, fewer than %d' % (t, d[t], MIN_SPOTS))
    trace = np.repeat(np.arange(T), d)
    bad = (locus < 0) | (locus >= nhap)
    if np.any(bad):
        q = int(np.where(bad)[0][0])
        raise ValueError('tracing input: trace %d: locus %d is outside [0, %d)' % (trace[q], locus[q], nhap))
    inner = np.ones(len(locus), bool)  # spots that have a predecessor in their trace
    inner[ptr[:-1]] = False
    step = np.zeros(len(locus), bool)
    step[1:] = locus[1:] <= locus[:-1]
    if np.any(step & inner):
        raise ValueError('tracing input: trace %d: loci are not strictly increasing' % trace[np.where(step & inner)[0][0]])
    ch = hap_chrom[locus]
    jump = np.zeros(len(locus), bool)
    jump[1:] = ch[1:] != ch[:-1]
    if np.any(jump & inner):
        raise ValueError('tracing input: trace %d has loci of more than one chromosome' %
                         trace[np.where(jump & inner)[0][0]])
    fin = np.isfinite(position).all(axis=1)
    if not np.all(fin):
        raise ValueError('tracing input: trace %d has a non-finite position' % trace[np.where(~fin)[0][0]])
    first = locus[ptr[:-1]]
    chrom, ncopy = np.asarray(ch[ptr[:-1]]), (copy_ptr[first + 1] - copy_ptr[first]).astype(np.int32)
    cells = None if data.get('cell_ptr') is None else _check_cells(data['cell_ptr'], T, chrom, ncopy)
    return {'trace_ptr': ptr, 'locus': locus.astype(np.int32), 'position': position.astype(np.float32),
            'chrom': chrom, 'ncopy': ncopy, 'cell_ptr': cells}


def _check_cells(cell_ptr, T, chrom, ncopy):
    """cell_ptr (Ncell + 1,) int64 validated against the T traces: starts at 0, ends at T, every
    cell with at least one trace and at most C traces of a chromosome of C copies"""
    cp = np.asarray(cell_ptr).astype(np.int64).reshape(-1)
    if len(cp) < 1 or cp[0] != 0:
        raise ValueError('tracing input: cell_ptr must start at 0')
    d = np.diff(cp)
    if np.any(d < 0):
        raise ValueError('tracing input: cell_ptr is not monotone at cell %d' % int(np.where(d < 0)[0][0]))
    if np.any(d == 0):
        raise ValueError('tracing input: cell %d has no trace' % int(np.where(d == 0)[0][0]))
    if cp[-1] != T:
        raise ValueError('tracing input: cell_ptr ends at %d, the file has %d traces' % (cp[-1], T))
    names, cid = np.unique(chrom, return_inverse=True)
    key = np.repeat(np.arange(len(d)), d) * max(len(names), 1) + cid  # (cell, chromosome), sorted by cell
    uniq, first, count = np.unique(key, return_index=True, return_counts=True)
    over = np.where(count > ncopy[first])[0]
    if len(over):
        t = int(first[over[0]])
        raise ValueError('tracing input: cell %d has %d traces of chromosome %s, which has %d copies' % (
            uniq[over[0]] // max(len(names), 1), count[over[0]], chrom[t], ncopy[t]))
    return cp


def read_traces(path, store):
    """The trace file of restraints/tracing/input_file, validated against the population
    `store` (copy_ptr, hap_chrom): see check_traces."""
    from . import h5
    with h5.File(path) as f:
        data = {k: np.asarray(f.read(k)) for k in ('trace_ptr', 'locus', 'position')}
        if 'cell_ptr' in f.keys():
            data['cell_ptr'] = np.asarray(f.read('cell_ptr'))
    return check_traces(data, store.copy_ptr, store.hap_chrom)


def slice_traces(traces, t0, t1):
    """the traces t0 .. t1 as a trace set of their own"""
    p = traces['trace_ptr']
    return {'trace_ptr': p[t0:t1 + 1] - p[t0], 'locus': traces['locus'][p[t0]:p[t1]],
            'position': traces['position'][p[t0]:p[t1]], 'chrom': traces['chrom'][t0:t1],
            'ncopy': traces['ncopy'][t0:t1]}


def _entry_arrays(xyz, copy_ptr, copy_idx, traces):
    """(xyz, copy_ptr, copy_idx, trace_ptr, locus, position) contiguous and of the types both
    library entries read"""
    xyz = np.ascontiguousarray(xyz, np.float32)
    assert xyz.ndim == 3 and xyz.shape[2] == 3, 'xyz must be (nbead, nstruct, 3)'
    return (xyz, np.ascontiguousarray(copy_ptr, np.int32), np.ascontiguousarray(copy_idx, np.int32),
            np.ascontiguousarray(traces['trace_ptr'], np.int64), np.ascontiguousarray(traces['locus'], np.int32),
            np.ascontiguousarray(traces['position'], np.float32))


def assign_costs(xyz, copy_ptr, copy_idx, traces, keep_best, ctx=None, return_full=False, device=0):
    """One igm_tracing_assign call: best_cand (T, keep_best) int32 = s * Cmax + k and best_rmsd
    (T, keep_best) float32 in increasing order (ties to the lower candidate), Cmax = the largest
    copy count among the traces [, and the full (T, S, Cmax) float32 matrix, +inf where k >= C_t].
    xyz is the bead-major (nbead, S, 3) float32 population."""
    from . import _lib
    c = ctx or _lib.context(device)
    xyz, copy_ptr, copy_idx, ptr, locus, pos = _entry_arrays(xyz, copy_ptr, copy_idx, traces)
    T, kb, S = len(ptr) - 1, int(keep_best), xyz.shape[1]
    # (every locus of a trace has its trace's copy count; clipped: the library rejects a bad locus)
    cmax = int(np.diff(copy_ptr)[np.clip(locus, 0, len(copy_ptr) - 2)].max()) if len(locus) else 1
    bc = np.zeros((T, max(kb, 0)), np.int32)
    bv = np.zeros((T, max(kb, 0)), np.float32)
    full = np.zeros((T, S, cmax), np.float32) if return_full else None
    rc = c.lib.igm_tracing_assign(c.h, 0, xyz.ctypes.data, xyz.shape[0], S, copy_ptr.ctypes.data,
                                  copy_idx.ctypes.data, len(copy_ptr) - 1, T, ptr.ctypes.data, _lib.ptr(locus),
                                  _lib.ptr(pos), kb, _lib.ptr(full), bc.ctypes.data, bv.ctypes.data)
    c.check(rc, 'igm_tracing_assign')
    return (bc, bv, full) if return_full else (bc, bv)


def greedy_assignment(best_cand, best_rmsd, trace_chain):
    """Which of its keep_best candidates every trace takes: pick (T,) int64, the column of
    best_cand, -1 for a trace left unassigned.  A slot is (structure, chromosome, copy) = (the
    candidate, trace_chain[t]: the chromosome of the trace) and takes at most one trace.  The
    traces are visited in ascending (best_rmsd[t, 0], t); each takes its first free candidate.
    best_cand of all traces must share one encoding (one Cmax)."""
    chain = np.asarray(trace_chain)
    return _greedy(best_cand, best_rmsd, lambda t, cand: (cand, chain[t].item()))


def _greedy(best, cost, slot):
    """pick (n,) int64: the rows of best (n, keep_best) in ascending (cost[i, 0], i) each take the
    first column j whose slot(i, best[i, j]) no earlier row has taken, -1 when none is free"""
    best = np.asarray(best)
    cost = np.asarray(cost)
    n = len(best)
    pick = np.full(n, -1, np.int64)
    taken = set()
    for i in np.lexsort((np.arange(n), cost[:, 0])) if n else []:
        for j, cand in enumerate(best[i].tolist()):
            key = slot(i, cand)
            if key not in taken:
                taken.add(key)
                pick[i] = j
                break
    return pick


def kabsch(p, x):
    """(R, rmsd): the proper rotation (det = +1) and the RMSD of the best superposition
    R (p - mean p) + mean x of the points p (n, 3) on x (n, 3), fp64."""
    p = np.asarray(p, np.float64)
    x = np.asarray(x, np.float64)
    pc, xc = p - p.mean(axis=0), x - x.mean(axis=0)
    U, sv, Vt = np.linalg.svd(xc.T @ pc)
    d = 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0.0 else -1.0
    R = U @ np.diag([1.0, 1.0, d]) @ Vt
    r = R @ pc.T - xc.T
    return R, float(np.sqrt(np.sum(r * r) / len(p)))


def _superpose(xyz, copy_ptr, copy_idx, traces, a, b, k, s, target):
    """The spots a .. b superposed on their beads in structure s, spot i on copy k (one copy, or
    one per spot): writes target[a:b] = R (p - mean p) + mean x and returns (R, kabsch's rmsd, x)."""
    x = np.asarray(xyz[np.asarray(copy_idx)[copy_ptr[traces['locus'][a:b]] + k], s], np.float64)
    p = np.asarray(traces['position'][a:b], np.float64)
    R, rmsd = kabsch(p, x)
    target[a:b] = (p - p.mean(axis=0)) @ R.T + x.mean(axis=0)
    return R, rmsd, x


def aligned_targets(xyz, copy_ptr, copy_idx, traces, structure, copy):
    """The assigned traces in the model's frame.  structure / copy (T,): the slot of every
    trace, -1 = unassigned.  Returns (target (n, 3) float64 with NaN rows for the spots of
    unassigned traces, rmsd (T,) float64 with NaN, rotation (T, 3, 3)): Kabsch with the
    determinant correction, target_i = R (p_i - mean p) + mean x, x the trace's beads in its
    structure.  At most T small SVDs, so on the host."""
    ptr = traces['trace_ptr']
    T = len(ptr) - 1
    target = np.full((int(ptr[-1]), 3), np.nan)
    rmsd = np.full(T, np.nan)
    rot = np.full((T, 3, 3), np.nan)
    copy_ptr = np.asarray(copy_ptr, np.int64)
    for t in range(T):
        s, k = int(structure[t]), int(copy[t])
        if s < 0:
            continue
        rot[t], rmsd[t], _ = _superpose(xyz, copy_ptr, copy_idx, traces, int(ptr[t]), int(ptr[t + 1]), k, s, target)
    return target, rmsd, rot


# ---------------------------------------------------------------------------- imaged cells
def slice_cells(traces, c0, c1):
    """the cells c0 .. c1 as a trace set of their own"""
    cp = traces['cell_ptr']
    sub = slice_traces(traces, int(cp[c0]), int(cp[c1]))
    sub['cell_ptr'] = cp[c0:c1 + 1] - cp[c0]
    return sub


def assign_cell_costs(xyz, copy_ptr, copy_idx, traces, keep_best, ctx=None, return_full=False, device=0,
                      scratch_bytes=0):
    """One igm_tracing_assign_cells call on the cells of `traces` (check_traces with cell_ptr):
    best_struct (Ncell, keep_best) int32 and best_cost (Ncell, keep_best) float32 in increasing
    order (ties to the lower structure), best_label (T, keep_best) uint8: the copy of every trace
    at that candidate [, and the full cost (Ncell, S) float32, label (T, S) uint8 and rounds
    (Ncell, S) uint8].  The cost of (cell, structure) is the RMSD of all the cell's spots under
    ONE proper rigid motion and the homologue labelling the alternating search ends at
    (include/igm_hip.h).  scratch_bytes: device scratch of the per-trace sums, 0 = 1 GiB."""
    from . import _lib
    c = ctx or _lib.context(device)
    xyz, copy_ptr, copy_idx, ptr, locus, pos = _entry_arrays(xyz, copy_ptr, copy_idx, traces)
    cell_ptr = np.ascontiguousarray(traces['cell_ptr'], np.int64)
    _, chrom = np.unique(np.asarray(traces['chrom']), return_inverse=True)
    chrom = np.ascontiguousarray(chrom, np.int32)
    T, nc, kb, S = len(ptr) - 1, len(cell_ptr) - 1, int(keep_best), xyz.shape[1]
    bs = np.zeros((nc, max(kb, 0)), np.int32)
    bv = np.zeros((nc, max(kb, 0)), np.float32)
    bl = np.zeros((T, max(kb, 0)), np.uint8)
    cost = np.zeros((nc, S), np.float32) if return_full else None
    label = np.zeros((T, S), np.uint8) if return_full else None
    rounds = np.zeros((nc, S), np.uint8) if return_full else None
    rc = c.lib.igm_tracing_assign_cells(c.h, 0, xyz.ctypes.data, xyz.shape[0], S, copy_ptr.ctypes.data,
                                        copy_idx.ctypes.data, len(copy_ptr) - 1, T, ptr.ctypes.data, _lib.ptr(locus),
                                        _lib.ptr(pos), _lib.ptr(chrom), nc, cell_ptr.ctypes.data, kb,
                                        int(scratch_bytes), _lib.ptr(cost), _lib.ptr(label), _lib.ptr(rounds),
                                        bs.ctypes.data, bv.ctypes.data, bl.ctypes.data)
    c.check(rc, 'igm_tracing_assign_cells')
    return (bs, bv, bl, cost, label, rounds) if return_full else (bs, bv, bl)


def greedy_cell_assignment(best_struct, best_cost):
    """Which of its keep_best candidate structures every cell takes: pick (Ncell,) int64, the
    column of best_struct, -1 for a cell left unassigned.  A structure is one cell, so it takes
    at most one: the cells are visited in ascending (best_cost[c, 0], c) and each takes its first
    free candidate."""
    return _greedy(best_struct, best_cost, lambda c, s: s)


def aligned_cell_targets(xyz, copy_ptr, copy_idx, traces, cell_structure, copy):
    """The assigned cells in the model's frame.  cell_structure (Ncell,): the structure of every
    cell, -1 = unassigned; copy (T,): the homologue labelling of its traces.  One Kabsch (fp64,
    determinant corrected) per cell over ALL its spots: target_i = R (p_i - mean p) + mean x.
    Returns (target (n, 3) float64 with NaN rows for unassigned cells, cell_rmsd (Ncell,), the
    RMSD of every trace on its own under the cell's motion (T,), rotation (Ncell, 3, 3))."""
    ptr, cp = traces['trace_ptr'], traces['cell_ptr']
    T, nc = len(ptr) - 1, len(cp) - 1
    target = np.full((int(ptr[-1]), 3), np.nan)
    cell_rmsd, trace_rmsd = np.full(nc, np.nan), np.full(T, np.nan)
    rot = np.full((nc, 3, 3), np.nan)
    copy_ptr = np.asarray(copy_ptr, np.int64)
    for c in range(nc):
        s = int(cell_structure[c])
        if s < 0:
            continue
        t0, t1 = int(cp[c]), int(cp[c + 1])
        a, b = int(ptr[t0]), int(ptr[t1])
        k = np.repeat(np.asarray(copy[t0:t1], np.int64), np.diff(ptr[t0:t1 + 1]))
        rot[c], cell_rmsd[c], x = _superpose(xyz, copy_ptr, copy_idx, traces, a, b, k, s, target)
        d2 = np.sum((target[a:b] - x) ** 2, axis=1)
        trace_rmsd[t0:t1] = np.sqrt(np.add.reduceat(d2, ptr[t0:t1] - a) / np.diff(ptr[t0:t1 + 1]))
    return target, cell_rmsd, trace_rmsd, rot


def write_assignment(path, traces, copy_ptr, copy_idx, structure, copy, target, rmsd, cell_structure=None,
                     cell_rmsd=None):
    """The assignment file of the M-step from an A-step result: the datasets read_assignment
    reads -- locus (the DIPLOID bead), target float64, assignment (the structure) -- over the
    spots of the assigned traces, by trace then by spot; 'trace' (per entry) and, per trace,
    trace_structure, trace_copy (-1 = unassigned) and trace_rmsd (NaN).  A run on imaged cells
    (cell_structure given) adds trace_cell (T,), cell_structure and cell_rmsd (Ncell,), and its
    trace_rmsd is every trace's own RMSD under its cell's motion."""
    from . import h5
    ptr = traces['trace_ptr']
    T = len(ptr) - 1
    structure = np.asarray(structure, np.int64)
    copy = np.asarray(copy, np.int64)
    trace = np.repeat(np.arange(T), np.diff(ptr))
    keep = structure[trace] >= 0
    copy_ptr = np.asarray(copy_ptr, np.int64)
    slot = copy_ptr[np.asarray(traces['locus'], np.int64)[keep]] + copy[trace[keep]]
    out = {'locus': np.asarray(copy_idx)[slot].astype(np.int64),
           'target': np.ascontiguousarray(np.asarray(target, np.float64)[keep]),
           'assignment': structure[trace[keep]], 'trace': trace[keep].astype(np.int64),
           'trace_structure': structure, 'trace_copy': np.where(structure >= 0, copy, -1),
           'trace_rmsd': np.asarray(rmsd, np.float64)}
    if cell_structure is not None:
        out.update({'trace_cell': np.repeat(np.arange(len(traces['cell_ptr']) - 1), np.diff(traces['cell_ptr'])),
                    'cell_structure': np.asarray(cell_structure, np.int64),
                    'cell_rmsd': np.asarray(cell_rmsd, np.float64)})
    h5.write(path, out)
