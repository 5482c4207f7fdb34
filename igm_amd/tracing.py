"""Chromatin tracing data in the M-step (igm/restraints/tracing.py; ModelingStep.py:281-300,
RelaxInit.py:186-207, RandomInit.py:70-102): every locus imaged in a cell is tied to its
imaged position by a harmonic upper bound of radius `tol`.

The reference adds one DUMMY_STATIC centroid per imaged locus and a bond to it; here the
restraint is a position anchor of the engine (igm_anchor, include/igm_hip.h): no atom is
added, so a traced 2 Mb structure stays in the LDS engine.  The reference has no A-step
for tracing: the assignment file is an input,

    locus       (n,)   diploid bead index
    target      (n, 3) imaged position
    assignment  (n,)   structure index the locus was imaged in
"""
import numpy as np

from ._lib import anchor_dtype


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
