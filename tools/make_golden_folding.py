#!/usr/bin/env python
"""Mint tests/golden/folding_sampler.{json,npz} from the REAL reference samplers, CEM base controller and towel experiments.

Runs the reference's ``FoldingCEMSampler`` and ``AutograspSampler`` (``visual_mpc/policy/cem_controllers/samplers/``), its
``CEMBaseController`` and its two towel-folding experiment files under ``tools/make_golden.py``'s stubs (that file is not
edited) plus the learned-cost stubs of ``tools/make_golden_learned_cost.py``, on the cases and through the drivers of
``tests/helpers/folding_fixtures.py`` - the very functions ``tests/test_folding_sampler.py`` then runs on this project's
classes.  Recorded:

* folding sampler: per case the initial draw, a refit on its ten best, ``_base_mean`` / ``_full_sigma`` after each; the
  default hyper-parameters; the exception types of ``M`` 200, ``nactions`` 7, ``nactions`` 4 and ``adim`` 5;
* autograsp sampler: the default hyper-parameters; the exception type of a refit of the class AS IT STANDS (its
  ``sample_next_actions`` calls the parent without ``scores``); then, with the parent's ``sample_next_actions`` wrapped so
  that ``scores`` is optional and nothing else changed, initial draws and refits of every case;
* ``act()`` traces: ``CEMBaseController`` with the folding sampler and a deterministic cost, two planning calls;
* both towel ``hparams.py`` files: the ``policy`` dict, ``_hp.values()`` after the reference's ``_default_hparams`` /
  ``_override_defaults`` on a bare ``ClassifierController`` (its constructor needs the absent scorer package), the
  agent's sizes and the plain settings of the ``conf.py`` beside it.

Only numbers and names travel.

    python tools/make_golden_folding.py        # rewrites tests/golden/folding_sampler.{json,npz}
"""
import json
import os
import sys

import numpy as np

TOOLS = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, TOOLS)
import make_golden as mg  # noqa: E402
import make_golden_learned_cost as mlc  # noqa: E402
from tests.helpers import folding_fixtures as fx  # noqa: E402

OUT = os.path.join(mg.REPO, 'tests', 'golden')
TOWEL_FILES = {'sawyer': 'experiments/sawyer/towel_classifier', 'offline': 'experiments/offline_exp/towel_classifier'}
PLAIN = (bool, int, float, str, list, tuple)


def golden_towel_files():
    from visual_mpc.policy.cem_controllers.variants.classifier_controller import ClassifierController
    out = {}
    # conf.py imports the predictor set-up code and the model class, which need the real TensorFlow and robonet: only their
    # names are wanted here
    for name in ('visual_mpc.video_prediction.setup_predictor', 'visual_mpc.video_prediction.vpred_model_interface',
                 'robonet.video_prediction.models', 'robonet.video_prediction.models.savp_model'):
        sys.modules.setdefault(name, mg._StubModule(name))
    with mg.experiment_import_stubs():
        for name, rel in TOWEL_FILES.items():
            mod = mg.load_experiment_file(rel + '/hparams.py')
            policy, agent = mod.config['policy'], mod.config['agent']
            assert policy['type'] is ClassifierController
            pdict = {k: v for k, v in policy.items() if k != 'type'}
            ctrl = object.__new__(ClassifierController)
            with mg.quiet():
                ctrl._hp = ctrl._default_hparams()
                ctrl._override_defaults(dict(policy))
            conf = mg.load_experiment_file(rel + '/conf.py').configuration
            out[name] = {'file': rel + '/hparams.py', 'controller': policy['type'].__name__, 'policy': mg.jsonable(pdict),
                         'values': mg.jsonable(ctrl._hp.values()),
                         'agent': {k: agent[k] for k in ('T', 'image_height', 'image_width')},
                         'conf': {k: mg.jsonable(v) for k, v in sorted(conf.items())
                                  if isinstance(v, PLAIN) and not isinstance(v, type) and 'home' not in str(v)}}
    return out


def main():
    mg.install_stubs()
    mlc.install_learned_cost_stubs()
    from visual_mpc.policy.cem_controllers import CEMBaseController
    from visual_mpc.policy.cem_controllers.samplers import AutograspSampler, GaussianCEMSampler
    from visual_mpc.policy.cem_controllers.samplers.folding_sampler import FoldingCEMSampler
    arrays, meta = {}, {'numpy': np.__version__}

    # ---- folding sampler
    cases = []
    for i, (name, over, M, state) in enumerate(fx.FOLDING_CASES):
        arrays.update(fx.run_folding_case(mg.HParams, FoldingCEMSampler, i))
        cases.append({'name': name, 'over': over, 'M': M, 'current_state': state, 'seed': fx.FOLDING_SEED0 + i})
    meta['folding'] = {'cases': cases, 'default_hparams': mg.jsonable(FoldingCEMSampler.get_default_hparams()),
                       'errors': {label: fx.folding_error(mg.HParams, FoldingCEMSampler, label)
                                  for label in fx.FOLDING_ERRORS}}

    # ---- autograsp sampler: the class as it stands, then with `scores` optional in the parent
    meta['autograsp'] = {'default_hparams': mg.jsonable(AutograspSampler.get_default_hparams()),
                         'refit_error': fx.autograsp_refit_error(mg.HParams, AutograspSampler)}
    parent_refit = GaussianCEMSampler.sample_next_actions
    GaussianCEMSampler.sample_next_actions = \
        lambda self, n_samples, best_actions, scores=None: parent_refit(self, n_samples, best_actions, scores)
    try:
        cases = []
        for i, (name, over, state) in enumerate(fx.AUTOGRASP_CASES):
            got = fx.run_autograsp_case(mg.HParams, AutograspSampler, i)
            height = np.cumsum(got[name + '/a0'][:, :, 2] * over.get('action_norm_factor', 1.0), axis=1) + state[2]
            low = (height < over.get('z_thresh', 0.15)).any(axis=1)
            assert low.any() and not low.all(), (name, low)         # some sequences cross z_thresh, some do not
            arrays.update(got)
            cases.append({'name': name, 'over': over, 'current_state': state, 'seed': fx.AUTOGRASP_SEED0 + i,
                          'M': fx.AUTOGRASP_M, 'sequences_below_z_thresh': int(low.sum())})
        meta['autograsp']['cases'] = cases
    finally:
        GaussianCEMSampler.sample_next_actions = parent_refit

    # ---- act() traces
    trace_arrays, trace = fx.run_act_trace(CEMBaseController, FoldingCEMSampler)
    arrays.update(trace_arrays)
    meta['trace'] = {'t_since_replan': trace, 'seed': fx.TRACE_SEED, 'policy': fx.TRACE_POLICY, 'steps': fx.TRACE_STEPS}

    # ---- the towel experiments
    meta['towel'] = golden_towel_files()

    np.savez_compressed(os.path.join(OUT, 'folding_sampler.npz'), **arrays)
    with open(os.path.join(OUT, 'folding_sampler.json'), 'w') as f:
        json.dump(mg.jsonable(meta), f, indent=1, sort_keys=True)
    for fn in ('folding_sampler.json', 'folding_sampler.npz'):
        print('  %-22s %8d B' % (fn, os.path.getsize(os.path.join(OUT, fn))))


if __name__ == '__main__':
    main()
