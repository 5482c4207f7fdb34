"""The igm-run pipeline body on the Step layer (bin/igm-run:50-325): the
start-up steps, then A/M iterations until every data set's threshold list is used
up with an acceptable violation score, or max_iterations unsuccessful iterations.

  start-up   starting_coordinates copied, or RandomInit [+ PolymerAssignmentStep when
             the chain is modelled by distance distributions] + RelaxInit (:50-82)
  iteration  PolymerAssignmentStep (restraints/polymer), NuclDamidActivationDistanceStep
             (nuclDamID), TracingAssignmentStep (tracing with input_file),
             ActivationDistanceStep (Hi-C), FishAssignmentStep (FISH),
             SpriteAssignmentStep (sprite), DamidActivationDistanceStep (DamID),
             ModelingStep (:105-167), in that order
  control    is_acceptable = runtime/violation_score < optimization/max_violations;
             the threshold lists advance together when acceptable and no further
             iteration is forced (min_iterations, force_last_iteration,
             force_minimum_iterations_hic_cutoff), else opt_iter += 1 (:169-325)

The nucleolus exclusion body (model/restraints/nucleolus) needs no A-step; it and
nuclDamID are modelled on an exp_map nucleus only (ModelingStep raises otherwise, as
the reference fails there).  Chromatin tracing (restraints/tracing) works through
restraints/tracing/tol_list as FISH does through its own (bin/igm-run:122-133, 218-223,
283-285).  With assignment_file the assignment is an input and there is no step, as in the
reference; with input_file alone TracingAssignmentStep makes it from the imaged traces every
iteration, at the place of the reference's commented-out ImagedLociAssignmentStep (:135).  A
tracing section with neither raises: there is nothing to model.  Preprocess (genome/index,
.hss allocation) is the caller's: the population file must exist.  No email
notifications, no control socket.
"""
import os
import shutil

from . import steps as ST


def startup_steps(cfg):
    """bin/igm-run:50-82"""
    start = ST.cget(cfg, 'model/starting_coordinates', '')
    if start:
        if ST.cget(cfg, 'optimization/clean_restart', False) or \
                not os.path.isfile(ST.cget(cfg, 'parameters/step_db', 'stepdb.sqlite')):
            out = cfg['optimization']['structure_output']
            if os.path.abspath(start) != os.path.abspath(out):
                shutil.copyfile(start, out)
        return []
    steps = [ST.RandomInit]
    if 'polymer' not in cfg['model']['restraints']:
        steps.append(ST.PolymerAssignmentStep)
    steps.append(ST.RelaxInit)
    return steps


def iteration_steps(cfg):
    """bin/igm-run:105-161"""
    R = cfg.get('restraints', {})
    tr = R.get('tracing')
    assign_traces = tr is not None and bool(tr.get('input_file')) and not tr.get('assignment_file')
    if tr is not None and not assign_traces:  # the file is given (bin/igm-run:122-133), or nothing can be done
        ST.tracing_assignment_file(cfg)
    steps = []
    if 'polymer' in R:
        steps.append(ST.PolymerAssignmentStep)
    if 'nuclDamID' in R:  # bin/igm-run:118-119
        steps.append(ST.NuclDamidActivationDistanceStep)
    if assign_traces:  # the place of the reference's commented-out ImagedLociAssignmentStep (bin/igm-run:135)
        steps.append(ST.TracingAssignmentStep)
    if 'Hi-C' in R:
        steps.append(ST.ActivationDistanceStep)
    if 'FISH' in R:
        steps.append(ST.FishAssignmentStep)
    if 'sprite' in R:
        steps.append(ST.SpriteAssignmentStep)
    if 'DamID' in R:
        steps.append(ST.DamidActivationDistanceStep)
    steps.append(ST.ModelingStep)
    return steps


def _remaining(cfg, section, key):
    return section in cfg.get('restraints', {}) and len(ST.cget(cfg, 'runtime/%s/%s' % (section, key), [])) != 0


def run_pipeline(cfg, on_iteration=None):
    """Run the pipeline; returns 'completed' or 'max_iterations'.  on_iteration(cfg,
    opt_iter, steps) is called after every A/M iteration (tests, logging)."""
    rt = cfg.setdefault('runtime', {})
    for k in cfg.get('restraints', {}):  # Config.__init__ gives every restraint a runtime section
        rt.setdefault(k, {})
    for S in startup_steps(cfg):
        S(cfg).run()
    opt_iter = 0
    min_iter = ST.cget(cfg, 'optimization/min_iterations', 5)
    max_iter = ST.cget(cfg, 'optimization/max_iterations', 12)
    while True:
        rt['opt_iter'] = opt_iter
        if 'tracing' in cfg.get('restraints', {}):  # bin/igm-run:122-133
            if ST.tracing_assigned(cfg):  # (else TracingAssignmentStep makes the file in this iteration)
                ST.tracing_assignment_file(cfg)
            tr = rt.setdefault('tracing', {})
            if 'tol_list' not in tr:
                tr['tol_list'] = list(cfg['restraints']['tracing']['tol_list'])
            if 'tol' not in tr:
                tr['tol'] = tr['tol_list'].pop(0)
        steps = iteration_steps(cfg)
        for S in steps:
            S(cfg).run()
        if on_iteration is not None:
            on_iteration(cfg, opt_iter, steps)
        acceptable = ST.cget(cfg, 'runtime/violation_score') < ST.rget(cfg, 'optimization/max_violations', 0.01)
        hic_inc = 'Hi-C' in cfg.get('restraints', {}) and (
            len(ST.cget(cfg, 'runtime/Hi-C/intra_sigma_list', [])) != 0 or
            len(ST.cget(cfg, 'runtime/Hi-C/inter_sigma_list', [])) != 0)
        damid_inc = _remaining(cfg, 'DamID', 'sigma_list')
        nucldamid_inc = _remaining(cfg, 'nuclDamID', 'sigma_list')  # bin/igm-run:196-199
        fish_inc = _remaining(cfg, 'FISH', 'tol_list')
        sprite_inc = _remaining(cfg, 'sprite', 'volume_fraction_list')
        tracing_inc = _remaining(cfg, 'tracing', 'tol_list')  # bin/igm-run:218-223
        all_done = not (hic_inc or damid_inc or nucldamid_inc or fish_inc or sprite_inc or tracing_inc)
        force = (opt_iter < min_iter - 1) and (opt_iter != 0)
        if ST.cget(cfg, 'optimization/force_last_iteration', False) and all_done and opt_iter == 0:
            force = True
        if 'Hi-C' in cfg.get('restraints', {}) and opt_iter == 0 and \
                ST.cget(cfg, 'runtime/Hi-C/intra_sigma') <= ST.cget(cfg, 'optimization/force_minimum_iterations_hic_cutoff',
                                                                  0.0):
            force = True
        if acceptable and not force:
            if hic_inc:
                del rt['Hi-C']['intra_sigma']
                del rt['Hi-C']['inter_sigma']
                opt_iter = 0
            if damid_inc:
                del rt['DamID']['sigma']
                opt_iter = 0
            if nucldamid_inc:  # bin/igm-run:265-269
                del rt['nuclDamID']['sigma']
                opt_iter = 0
            if fish_inc:
                del rt['FISH']['tol']
                opt_iter = 0
            if sprite_inc:
                del rt['sprite']['volume_fraction']
                opt_iter = 0
            if tracing_inc:  # bin/igm-run:283-285
                del rt['tracing']['tol']
                opt_iter = 0
            if all_done:
                open(os.path.join(ST.cget(cfg, 'parameters/workdir', '.'), 'completed'), 'w').close()
                return 'completed'
        else:
            opt_iter += 1
            if max_iter is not None and opt_iter >= max_iter:
                return 'max_iterations'
