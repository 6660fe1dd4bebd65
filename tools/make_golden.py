#!/usr/bin/env python
"""Mint the golden fixtures under tests/golden/ by running the REAL reference host code.

Runs only in the build container: it imports ``/root/reference`` (read-only) with the five
stub modules SURVEY.md 8(c) lists injected into ``sys.modules`` (funcsigs, tensorflow's
HParams, cv2, robonet's VPredEvaluation, and the removed ``np.int`` alias; three more for
``register_gtruth_controller.py``, see ``install_registration_stubs``), drives the
reference's own ``get_policy_args`` / ``CEMBaseController`` / ``PixelCostController`` /
samplers / ``controller_utils`` / ``pred_util`` on seeded synthetic inputs, and stores the
inputs' seeds plus the observed outputs.  Nothing of the reference travels: the fixtures are
numbers only.  The tests then require this repo's host code (and the oracle restatement of
the cost) to reproduce the outputs from the same inputs.

    python tools/make_golden.py        # rewrites tests/golden/*.npz|json

The TF ``HParams`` class does not exist in this image; the stub the reference runs on is
``oracle/tf_hparams.py`` - a restatement of TF 1.6's class from its published source (type
rules of ``_cast_to_type_if_compatible`` included) that shares no code with this repo's
``visual_foresight_amd.hparams.HParams`` - so the fixtures pin the reference's override
protocol (policy.py:51-63, cem_base_controller.py:66-76) AND TF's cast rules against the
product class instead of pinning the product class against itself.
"""
import io
import json
import os
import re
import sys
import types
import contextlib

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = '/root/reference'
OUT = os.path.join(REPO, 'tests', 'golden')
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

from tests.helpers.fake_predictor import make_fake_predictor_class  # noqa: E402
from oracle.tf_hparams import HParams  # noqa: E402  (the TF 1.6 restatement, not the product's class)


def install_stubs():
    import inspect
    if not hasattr(np, 'int'):
        np.int = int        # pixel_cost_controller.py:208 uses the removed alias

    funcsigs = types.ModuleType('funcsigs')
    funcsigs.signature, funcsigs.Parameter = inspect.signature, inspect.Parameter
    sys.modules['funcsigs'] = funcsigs

    tf = types.ModuleType('tensorflow')
    contrib = types.ModuleType('tensorflow.contrib')
    training = types.ModuleType('tensorflow.contrib.training')
    training.HParams = HParams
    tf.contrib, contrib.training = contrib, training
    sys.modules.update({'tensorflow': tf, 'tensorflow.contrib': contrib,
                        'tensorflow.contrib.training': training})

    cv2 = types.ModuleType('cv2')
    cv2.circle = lambda *a, **k: None
    sys.modules['cv2'] = cv2

    robonet = types.ModuleType('robonet')
    vp = types.ModuleType('robonet.video_prediction')
    testing = types.ModuleType('robonet.video_prediction.testing')
    testing.VPredEvaluation = make_fake_predictor_class(5, 16, 16)
    robonet.video_prediction, vp.testing = vp, testing
    sys.modules.update({'robonet': robonet, 'robonet.video_prediction': vp,
                        'robonet.video_prediction.testing': testing})

    import matplotlib
    matplotlib.use('Agg')
    sys.path.insert(0, REFERENCE)


def reference_predictor(fake):
    """Make ``fake`` the predictor class the reference constructs.  It cannot travel as a ``predictor_class`` override:
    TF's ``set_hparam`` ends in ``type(value)`` for a class-valued parameter (oracle/tf_hparams.py), the reference never
    overrides that key, so the stub takes the place of the default class the reference imported
    (``pixel_cost_controller.py:11-12``: ``VPredEvaluation as DefaultPredClass``)."""
    sys.modules['visual_mpc.policy.cem_controllers.pixel_cost_controller'].DefaultPredClass = fake


@contextlib.contextmanager
def quiet():
    with contextlib.redirect_stdout(io.StringIO()):
        yield


def jsonable(x):
    if isinstance(x, dict):
        return {str(k): jsonable(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [jsonable(v) for v in x]
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, (np.floating, np.integer)):
        return x.item()
    if isinstance(x, type):
        return 'class:' + x.__name__
    return x


# ----------------------------------------------------------------------------- a1
def golden_policy_args(ref):
    from visual_mpc.policy.policy import get_policy_args
    PCC = ref['PixelCostController']
    pol = PCC.__new__(PCC)          # only the signature of act() matters
    rs = np.random.RandomState(11)
    obs = {'images': rs.randint(0, 256, (3, 1, 8, 8, 3)).astype(np.uint8),
           'state': rs.normal(size=(3, 5))}
    agent_data = {'desig_pix': [[3, 4]], 'goal_pix': [[6, 1]], 'verbose_worker': 'queue-handle'}
    got = get_policy_args(pol, obs, 2, 7, agent_data)
    out = {'keys': sorted(got.keys()), 't': got['t'], 'i_tr': got['i_tr'],
           'desig_pix': got['desig_pix'], 'goal_pix': got['goal_pix'],
           'verbose_worker': got['verbose_worker'],
           'images_is_obs': bool(got['images'] is obs['images']),
           'state_is_obs': bool(got['state'] is obs['state'])}

    class NeedsGoal(object):
        def act(self, t, goal_image):
            pass
    try:
        get_policy_args(NeedsGoal(), obs, 0, 0, agent_data)
        out['missing_required'] = None
    except ValueError as e:
        out['missing_required'] = str(e)
    return out


# ----------------------------------------------------------------------------- a2
AG = {'adim': 4, 'sdim': 5, 'image_height': 16, 'image_width': 16}


# the reference's OWN experiment files: import stubs and loader
class _Anything(object):
    """Stands in for every class / function an experiment file imports from the parts of the reference that are out of
    scope (environments, agents, ROS topics): constructible with any arguments, any attribute is another one."""
    def __init__(self, *a, **k):
        pass

    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        return _Anything()

    def __call__(self, *a, **k):
        return _Anything()


class _StubModule(types.ModuleType):
    __path__ = []

    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        return type(name, (_Anything,), {})


class _StubFinder(object):
    """Catch-all import stub.  `front`: intercepts the reference's environment / agent / robot packages before their real
    modules (which need MuJoCo, ROS, ...) are found; otherwise: the last resort for anything the image lacks."""
    FRONT = ('visual_mpc.envs', 'visual_mpc.agent', 'visual_mpc.utils', 'visual_mpc.sim', 'visual_mpc.foresight_rospkg')

    def __init__(self, front):
        self.front = front

    def find_spec(self, name, path=None, target=None):
        import importlib.machinery
        if self.front and not any(name == p or name.startswith(p + '.') for p in self.FRONT):
            return None
        return importlib.machinery.ModuleSpec(name, self)

    def create_module(self, spec):
        return _StubModule(spec.name)

    def exec_module(self, module):
        pass



@contextlib.contextmanager
def experiment_import_stubs():
    """While active, the environment / agent / robot imports of the reference's experiment files resolve to catch-all stubs."""
    front, back = _StubFinder(True), _StubFinder(False)
    for k in ('VMPC_DATA_DIR', 'VMPC_EXP_DIR'):     # (experiment files build paths from them)
        os.environ.setdefault(k, '/nonexistent/' + k.lower())
    sys.meta_path.insert(0, front)
    sys.meta_path.append(back)
    try:
        yield
    finally:
        sys.meta_path.remove(front)
        sys.meta_path.remove(back)


def load_experiment_file(rel):
    import importlib.machinery
    import importlib.util
    path = os.path.join(REFERENCE, rel)
    name = 'vf_exp_' + re.sub(r'\W', '_', rel)
    loader = importlib.machinery.SourceFileLoader(name, path)
    mod = importlib.util.module_from_spec(importlib.util.spec_from_loader(name, loader))
    with quiet():
        loader.exec_module(mod)
    return mod



def policy_dicts():
    """The `policy` dicts of three experiment files, minus 'type' - read from the reference's own files (no hand-typed copy)."""
    files = {'sim_cartgripper': 'experiments/sim/cartgripper_2d_grasping/pixel_cost/hparams.py',
             'robonet_pixel_cost': 'experiments/robonet/pixel_cost/hparams.py',
             'robotiq_zero_shot': 'experiments/robonet/robotiq/zero_shot.py'}
    out = {}
    with experiment_import_stubs():
        for name, rel in files.items():
            mod = load_experiment_file(rel)
            out[name] = {k: v for k, v in mod.config['policy'].items() if k != 'type'}
    return out


def golden_hparams(ref):
    PCC = ref['PixelCostController']
    out = {'ag_params': AG, 'cases': {}}
    for name, pdict in policy_dicts().items():
        with quiet():
            ctrl = PCC(dict(AG), dict(pdict), 0, 1)
        vals = ctrl._hp.values()
        vals.pop('predictor_class')     # class object of the stub, not comparable
        out['cases'][name] = {'policy': jsonable(pdict), 'values': jsonable(vals),
                              'start_planning_after_ctor': ctrl._hp.start_planning}
    errs = {}
    for label, pdict in [('identical_to_default', {'iterations': 3}),
                         ('unknown_key', {'no_such_param': 1}),
                         ('list_for_scalar', {'T': [400, 200]}),
                         ('wrong_type', {'num_samples': 'many'})]:
        try:
            with quiet():
                PCC(dict(AG), dict(pdict), 0, 1)
            errs[label] = None
        except Exception as e:      # noqa
            errs[label] = type(e).__name__
    out['errors'] = errs
    return out


# ----------------------------------------------------------------------------- a2, every experiment file
def golden_experiment_files():
    """Load EVERY ``experiments/**`` file of the reference whose ``policy['type']`` is ``PixelCostController`` or
    ``Register_Gtruth_Controller`` from the reference itself (``SourceFileLoader``; the environment / agent / robot imports of
    those files resolve to catch-all stubs), run the reference's constructor on each ``policy`` dict with the fake predictor,
    and record per file either ``_hp.values()`` or the exception the REFERENCE raises (several of its own files do not load:
    keys that are no hyper-parameters, a list-valued ``num_samples``).  The product classes must reproduce all of it
    (tests/test_host_golden.py) - no hand-typed dict can skip a key.  Reference: policy.py:51-63, cem_base_controller.py:66-76."""
    import glob
    install_registration_stubs()
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        from visual_mpc.policy.cem_controllers.register_gtruth_controller import Register_Gtruth_Controller
    from visual_mpc.policy.cem_controllers import PixelCostController
    out = {'files': {}, 'skipped': {}}
    with experiment_import_stubs():
        for path in sorted(glob.glob(os.path.join(REFERENCE, 'experiments', '**', '*.py'), recursive=True)):
            rel = os.path.relpath(path, REFERENCE)
            with open(path) as f:
                ours = re.search(r"'type'\s*:\s*(PixelCostController|Register_Gtruth_Controller)\b", f.read()) is not None
            try:
                mod = load_experiment_file(rel)
            except Exception as e:      # noqa  (files of other sub-systems are not ours to load; one of OURS that does not
                if ours:                # even import in the reference - a syntax error, a sampler module that is gone - is pinned as such)
                    out['files'][rel] = {'unloadable': type(e).__name__}
                else:
                    out['skipped'][rel] = type(e).__name__
                continue
            cfg = getattr(mod, 'config', None)
            policy = cfg.get('policy') if isinstance(cfg, dict) else getattr(mod, 'policy', None)
            agent = cfg.get('agent') if isinstance(cfg, dict) else getattr(mod, 'agent', None)
            if not isinstance(policy, dict) or policy.get('type') not in (PixelCostController, Register_Gtruth_Controller):
                continue
            cls = policy['type']
            agent = agent if isinstance(agent, dict) else {}
            ag = {'adim': 4, 'sdim': 5, 'image_height': int(agent.get('image_height', 48)),
                  'image_width': int(agent.get('image_width', 64))}
            for k in ('register_gtruth', 'current_dir'):
                if k in agent:
                    ag[k] = agent[k]
            pdict = {k: v for k, v in policy.items() if k != 'type'}
            entry = {'controller': cls.__name__, 'ag_params': {k: v for k, v in ag.items() if k != 'current_dir'},
                     'policy': jsonable(pdict)}
            try:
                with quiet():
                    ctrl = cls(dict(ag), dict(policy), 0, 1)
                vals = ctrl._hp.values()
                vals.pop('predictor_class')
                entry['values'] = jsonable(vals)
                entry['start_planning_after_ctor'] = ctrl._hp.start_planning
            except Exception as e:      # noqa
                entry['raises'] = type(e).__name__
            out['files'][rel] = entry
    return out


# ----------------------------------------------------------------------------- a5
def golden_sampler(ref):
    from visual_mpc.policy.cem_controllers.samplers import GaussianCEMSampler, CorrelatedNoiseSampler
    from visual_mpc.policy.utils import controller_utils as cu
    arrays, meta = {}, {'cases': []}

    def hp_for(sampler_cls, **over):
        hp = HParams(replan_interval=0)
        for k, v in sampler_cls.get_default_hparams().items():
            hp.add_hparam(k, v)
        for k, v in over.items():
            setattr(hp, k, v)
        return hp

    cases = [
        ('gauss_a4', dict(rejection_sampling=False), 4, 0),
        ('gauss_a3_order', dict(rejection_sampling=False, action_order=['x', 'z', 'grasp'],
                                initial_std_lift=0.5), 3, 0),
        ('gauss_a5_t2', dict(rejection_sampling=False, reduce_std_dev=0.2), 5, 2),
        ('gauss_a4_h13', dict(rejection_sampling=False, nactions=13, repeat=1,
                              initial_std_lift=0.2, initial_std_rot=np.pi / 10), 4, 1),
        ('gauss_blockdiag_smooth', dict(rejection_sampling=False, cov_blockdiag=True,
                                        smooth_cov=True), 4, 0),
        ('gauss_discrete_zero', dict(rejection_sampling=False, discrete_ind=[3],
                                     add_zero_action=True), 4, 0),
        ('gauss_rejection', dict(rejection_sampling=True, stochastic_planning=None), 4, 0),
    ]
    for name, over, adim, t in cases:
        hp = hp_for(GaussianCEMSampler, **over)
        with quiet():
            sigma0 = cu.construct_initial_sigma(hp, adim, t)
            smp = GaussianCEMSampler(hp, adim, 5)
            np.random.seed(100 + len(meta['cases']))
            a0 = smp.sample_initial_actions(t, 32, np.zeros(5))
            elites = a0[np.argsort(np.abs(a0).sum((1, 2)))[:10]].copy()
            a1 = smp.sample_next_actions(32, elites, np.arange(10.))
        arrays[name + '/sigma0'] = sigma0
        arrays[name + '/a0'] = a0
        arrays[name + '/a1'] = a1
        arrays[name + '/mean'] = smp._mean
        arrays[name + '/sigma'] = smp._sigma
        meta['cases'].append({'name': name, 'over': jsonable(over), 'adim': adim, 't': t,
                              'seed': 100 + len(meta['cases'])})

    # reuse_mean across two planning calls (uses the logged best plan tails)
    hp = hp_for(GaussianCEMSampler, rejection_sampling=False, reuse_mean=True, reduce_std_dev=0.5)
    with quiet():
        smp = GaussianCEMSampler(hp, 4, 5)
        np.random.seed(7)
        a0 = smp.sample_initial_actions(1, 16, np.zeros(5))
        smp.log_best_action(a0[0, 0], a0[:5, 1:])
        b0 = smp.sample_initial_actions(2, 16, np.zeros(5))
    arrays['gauss_reuse_mean/a0'] = a0
    arrays['gauss_reuse_mean/b0'] = b0
    arrays['gauss_reuse_mean/mean'] = smp._mean

    # correlated noise sampler
    for name, over in [('corr_default', {}), ('corr_refit', dict(refit_cov=True, kappa=2)),
                       ('corr_bias', dict(mean_bias=np.array([0.01, 0., 0., 0.]), nactions=6))]:
        hp = hp_for(CorrelatedNoiseSampler, **over)
        with quiet():
            smp = CorrelatedNoiseSampler(hp, 4, 5)
            np.random.seed(55)
            a0 = smp.sample_initial_actions(0, 24, None)
            elites = a0[:8].copy()
            a1 = smp.sample_next_actions(24, elites, np.linspace(1., 3., 8))
        arrays[name + '/a0'] = a0
        arrays[name + '/a1'] = a1
        meta['cases'].append({'name': name, 'over': jsonable(over), 'seed': 55, 'kind': 'corr'})

    # helper functions on their own
    hp = hp_for(GaussianCEMSampler)
    x3 = np.random.RandomState(3).normal(0, 0.3, (6, 5, 4))
    x2 = np.random.RandomState(4).normal(0, 0.3, (6, 4))
    arrays['helpers/trunc3_in'], arrays['helpers/trunc2_in'] = x3.copy(), x2.copy()
    arrays['helpers/trunc3_out'] = cu.truncate_movement(x3.copy(), hp)
    arrays['helpers/trunc2_out'] = cu.truncate_movement(x2.copy(), hp)
    hp_o = hp_for(GaussianCEMSampler, action_order=['x', 'y', 'z', 'theta'])
    arrays['helpers/trunc3_order_out'] = cu.truncate_movement(x3.copy(), hp_o)
    cov = np.random.RandomState(5).normal(size=(20, 20))
    arrays['helpers/cov_in'] = cov
    arrays['helpers/blockdiag_out'] = cu.make_blockdiagonal(cov, 5, 4)
    d = np.random.RandomState(6).normal(2, 3, (4, 5, 4))
    arrays['helpers/disc_in'] = d.copy()
    arrays['helpers/disc_out'] = cu.discretize(d.copy(), 4, 5, [2, 3])
    hp_r = hp_for(GaussianCEMSampler, reuse_cov=0.25)
    hp_r.replan_interval = 3
    sig = np.random.RandomState(8).normal(size=(20, 20))
    arrays['helpers/reuse_cov_in'] = sig
    # with the sampler defaults present, reuse_cov calls construct_initial_sigma(t=None), which
    # compares None >= 2 (controller_utils.py:78): the stock path raises
    try:
        with quiet():
            cu.reuse_cov(sig, 4, hp_r)
        meta['reuse_cov_with_defaults'] = 'ok'
    except TypeError:
        meta['reuse_cov_with_defaults'] = 'TypeError'
    hp_r.del_hparam('reduce_std_dev')
    with quiet():
        arrays['helpers/reuse_cov_out'] = cu.reuse_cov(sig, 4, hp_r)
    return arrays, meta


# ----------------------------------------------------------------------------- a8 a9 a10 a11
def golden_cost(ref):
    PCC = ref['PixelCostController']
    arrays, meta = {}, {'numpy': np.__version__, 'cases': []}
    cases = [  # name, H, W, ncam(=1 in ref), ndesig, M, T, finalweight, only_first
        ('small', 16, 16, 1, 8, 5, 10., False),
        ('two_desig', 16, 20, 2, 8, 5, 10., False),
        ('four_desig', 12, 16, 4, 6, 4, 3., False),
        # with ndesig > 1 the reference's own logging indexes past the sliced score matrix
        # (pixel_cost_controller.py:158-159 -> IndexError), so the flag is only usable at ndesig=1
        ('first_view_nd1', 12, 16, 1, 6, 4, 3., True),
        ('c2_shape', 64, 64, 1, 32, 13, 10., False),
    ]
    for name, H, W, nd, M, T, fw, first in cases:
        fake = make_fake_predictor_class(T, H, W)
        reference_predictor(fake)
        pol = {'designated_pixel_count': nd, 'nactions': T, 'repeat': 1,
               'rejection_sampling': False, 'verbose': False, 'num_samples': M + 1}
        if nd == 1:
            pol.pop('designated_pixel_count')
        if T == 5:
            pol.pop('nactions')         # equal-to-default overrides raise (policy.py:57-58)
        if fw != 10.:
            pol['finalweight'] = fw
        if first:
            pol['only_take_first_view'] = True
        ag = dict(AG, image_height=H, image_width=W)
        with quiet():
            ctrl = PCC(ag, pol, 0, 1)
            ctrl.reset()
        seed = 1000 + len(meta['cases'])
        rs = np.random.RandomState(seed)
        distrib = rs.uniform(0.0, 1.0, (M, T, 1, H, W, nd)).astype(np.float32)
        goal = rs.randint(-3, max(H, W) + 3, (1, nd, 2))
        desig = rs.randint(-3, max(H, W) + 3, (1, nd, 2))
        ctrl._goal_pix, ctrl._desig_pix = goal, desig
        with quiet():
            scores = ctrl._eval_pixel_cost(0, distrib, None)
            per_task = np.stack([ctrl._expected_distance(0, p, distrib[:, :, 0, :, :, p],
                                                         ctrl._get_distancegrid(goal[0, p]))
                                 for p in range(nd)], axis=1)
            grid0 = ctrl._get_distancegrid(goal[0, 0])
            onehot = ctrl._switch_on_pix(desig)
        arrays[name + '/goal'], arrays[name + '/desig'] = goal, desig
        arrays[name + '/scores'] = scores
        arrays[name + '/scores_per_task'] = per_task
        arrays[name + '/argsort'] = scores.argsort()
        arrays[name + '/grid0'] = grid0
        arrays[name + '/onehot_nonzero'] = np.argwhere(onehot != 0)
        meta['cases'].append({'name': name, 'H': H, 'W': W, 'ndesig': nd, 'M': M, 'T': T,
                              'finalweight': fw, 'only_take_first_view': first, 'seed': seed,
                              'scores_dtype': str(scores.dtype), 'onehot_shape': list(onehot.shape)})
    return arrays, meta


# ----------------------------------------------------------------------------- a3 a4
def golden_act(ref):
    PCC = ref['PixelCostController']
    arrays, meta = {}, {'cases': []}
    H = W = 16
    T = 5
    cases = [
        ('replan_every_step', dict(num_samples=40), 4),
        ('replan_interval3', dict(num_samples=40, replan_interval=3, selection_frac=0.2), 6),
        ('propagation', dict(num_samples=30, predictor_propagation=True, iterations=2,
                             replan_interval=2), 5),
        ('correlated', dict(num_samples=40, sampler='corr', nactions=5), 4),
        ('append_action', dict(num_samples=24, append_action=[0.25]), 3),
    ]
    for name, over, n_steps in cases:
        from visual_mpc.policy.cem_controllers.samplers import CorrelatedNoiseSampler
        fake = make_fake_predictor_class(T, H, W)
        reference_predictor(fake)
        pol = {'verbose': False}
        if over.get('sampler') == 'corr':
            pol['sampler'] = CorrelatedNoiseSampler
            over = {k: v for k, v in over.items() if k != 'sampler'}
            pol.update(over)
            pol.pop('nactions')     # 5 != default 15 is set below
            pol['nactions'] = T
        else:
            pol.update(dict(rejection_sampling=False, repeat=1))   # nactions: default 5 == T
            pol.update(over)
        adim = 4 + (1 if 'append_action' in over else 0)
        sampler_adim = 4
        ag = dict(AG, adim=adim, image_height=H, image_width=W)
        with quiet():
            ctrl = PCC(ag, pol, 0, 1)
            if 'append_action' in over:
                ctrl._adim = sampler_adim       # sampler draws 4 dims, the 5th is appended
            ctrl.reset()
        seed = 2000 + len(meta['cases'])
        np.random.seed(seed)
        rs = np.random.RandomState(seed)
        images = rs.randint(0, 256, (n_steps + 1, 1, H, W, 3)).astype(np.uint8)
        states = rs.normal(0, 0.1, (n_steps + 1, 5))
        desig, goal = [[8, 8]], [[3, 12]]
        trace = []
        for t in range(n_steps):
            with quiet():
                out = ctrl.act(t=t, i_tr=0, desig_pix=desig, goal_pix=goal,
                               images=images[:t + 1], state=states[:t + 1])
            arrays['%s/t%d/action' % (name, t)] = np.array(out['actions'])
            for k, v in out['plan_stat'].items():
                arrays['%s/t%d/%s' % (name, t, k)] = np.array(v)
            if ctrl._best_indices is not None:
                arrays['%s/t%d/best_indices' % (name, t)] = np.array(ctrl._best_indices)
            trace.append(ctrl._t_since_replan)
        meta['cases'].append({'name': name, 'over': jsonable(over), 'n_steps': n_steps, 'seed': seed,
                              'T': T, 'H': H, 'W': W, 'adim': adim, 'sampler_adim': sampler_adim,
                              't_since_replan': trace, 'desig': desig, 'goal': goal,
                              'correlated': 'sampler' in pol,
                              'predictor_calls': list(fake.calls)})
    return arrays, meta


# ----------------------------------------------------------------------------- a13
def golden_pred_util(ref):
    from visual_mpc.video_prediction.pred_util import get_context, rollout_predictions
    arrays, meta = {}, {}
    rs = np.random.RandomState(31)
    images = rs.randint(0, 256, (5, 1, 6, 8, 3)).astype(np.uint8)
    state = rs.normal(size=(5, 3))
    hp = types.SimpleNamespace(state_append=[0.5, -1.0])
    f, s = get_context(2, 4, state, images, hp)
    arrays['ctx/images'], arrays['ctx/state'] = images, state
    arrays['ctx/frames_out'], arrays['ctx/states_out'] = f, s
    f2, s2 = get_context(2, 3, state, images, None)
    arrays['ctx/frames_out_t3'], arrays['ctx/states_out_t3'] = f2, s2

    seen = []

    def recording_predictor(input_images=None, input_state=None, input_actions=None,
                            input_one_hot_images=None):
        seen.append(np.array(input_actions))
        b = input_actions.shape[0]
        tag = input_actions.sum((1, 2))
        return tag[:, None] * np.ones((b, 2)), tag[:, None] + np.ones((b, 3)), None

    actions = rs.normal(size=(450, 3, 2))
    gi, gd, gs = rollout_predictions(recording_predictor, 200, actions, f, s, None)
    arrays['roll/actions'] = actions
    meta['chunk_shapes'] = [list(x.shape) for x in seen]
    arrays['roll/last_chunk_sum_padded_rows'] = np.array([np.abs(seen[-1][50:]).sum()])
    arrays['roll/gen_images'] = np.concatenate(gi, 0)
    arrays['roll/gen_distrib'] = np.concatenate(gd, 0)
    meta['gen_state_all_none'] = all(x is None for x in gs)
    meta['n_runs'] = len(seen)
    return arrays, meta


# ----------------------------------------------------------------------------- f4: trajectory layout
def golden_traj_layout():
    """Drive the reference's own ``Sim._save_raw_data`` (``visual_mpc/sim/simulator.py:64-93``) on a synthetic
    trajectory, with ``cv2.imwrite`` replaced by a recorder: the directory tree it creates, the image file
    names, the pixel array each ``imwrite`` call receives (BGR = the RGB frame with channels reversed) and the
    pickles' contents pin the on-disk layout this repo's rollout harness must reproduce."""
    import pickle
    import tempfile
    import cv2
    from visual_mpc.sim.simulator import Sim
    written = {}
    cv2.imwrite = lambda path, arr: written.__setitem__(path, np.array(arr))
    rs = np.random.RandomState(12)
    T, ncam, H, W = 4, 2, 6, 8
    images = rs.randint(0, 256, (T, ncam, H, W, 3)).astype(np.uint8)
    obs = {'images': images.copy(), 'state': rs.normal(0, 1, (T, 5))}
    agent_data = {'traj_ok': True, 'final_goal_distance': 3.5}
    policy_out = [{'actions': rs.normal(0, 1, 4)} for _ in range(T - 1)]
    with tempfile.TemporaryDirectory() as tmp:
        fake = types.SimpleNamespace(agentparams={'data_save_dir': tmp}, _hyperparams={'ngroup': 10},
                                     task_mode='train')
        with quiet():
            Sim._save_raw_data(fake, 23, agent_data, obs, policy_out)
        tree = sorted(os.path.relpath(os.path.join(d, f), tmp) for d, _, fs in os.walk(tmp) for f in fs)
        dirs = sorted(os.path.relpath(os.path.join(d, x), tmp) for d, xs, _ in os.walk(tmp) for x in xs)
        traj = os.path.join(tmp, 'train', 'traj_group2', 'traj23')
        obs_back = pickle.load(open(os.path.join(traj, 'obs_dict.pkl'), 'rb'))
        meta = {'files_on_disk': tree, 'dirs': dirs,
                'imwrite_paths': sorted(os.path.relpath(p, tmp) for p in written),
                'obs_dict_keys': sorted(obs_back.keys()),
                'agent_data': pickle.load(open(os.path.join(traj, 'agent_data.pkl'), 'rb')),
                'n_policy_out': len(pickle.load(open(os.path.join(traj, 'policy_out.pkl'), 'rb'))),
                'itr': 23, 'ngroup': 10, 'numpy': np.__version__}
        arrays = {'images': images, 'state': obs_back['state']}
        for p, arr in written.items():
            arrays['imwrite/' + os.path.relpath(p, traj)] = arr
    return arrays, meta


# ----------------------------------------------------------------------------- a15 / f2: registration
def install_registration_stubs():
    """Three more stubs so that ``register_gtruth_controller.py`` imports: the two visualizer modules
    (``:4,5``) and ``visual_mpc.registration_network.setup_registration`` (``:7``) are absent from the
    snapshot.  None of them is touched by ``get_warp_err`` / ``register_gtruth`` apart from the warper
    object, which the fixture replaces by a seeded fake (``tests/helpers/flow_warper.py``)."""
    base = 'visual_mpc.policy.cem_controllers.visualizer.'
    ru = types.ModuleType(base + 'render_utils')
    ru.resize_image = lambda *a, **k: (_ for _ in ()).throw(NotImplementedError('stub'))
    mv = types.ModuleType(base + 'make_cem_visuals')
    mv.CEM_Visual_Preparation_Registration = type('CEM_Visual_Preparation_Registration', (), {})
    rn = types.ModuleType('visual_mpc.registration_network')
    sr = types.ModuleType('visual_mpc.registration_network.setup_registration')
    sr.setup_gdn = lambda conf, gpu_id: None
    rn.setup_registration = sr
    sys.modules.update({base + 'render_utils': ru, base + 'make_cem_visuals': mv,
                        'visual_mpc.registration_network': rn,
                        'visual_mpc.registration_network.setup_registration': sr})


def golden_registration():
    """Run the reference's REAL ``Register_Gtruth_Controller.get_warp_err`` (:113-173) and
    ``register_gtruth`` (:54-111) on an instance made with ``object.__new__`` (its ``__init__`` needs
    a gdnconf.py and the absent network) and a seeded fake warper."""
    install_registration_stubs()
    from tests.helpers.flow_warper import registration_inputs
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        from visual_mpc.policy.cem_controllers.register_gtruth_controller import Register_Gtruth_Controller as RGC
    arrays, meta = {}, {'numpy': np.__version__, 'cases': []}

    def make(ncam, ntask, H, W, regs, region, pred_height, pix_t0, goal_pix):
        c = object.__new__(RGC)
        c._hp = HParams(register_gtruth=list(regs), register_region=region)
        c.ntask, c._n_cam, c._n_desig = ntask, ncam, ntask * len(regs)
        c.agentparams = {'image_height': H, 'image_width': W}
        c._img_height = pred_height
        c.desig_pix_t0 = np.array(pix_t0).reshape(ncam, ntask, 2)
        c.goal_pix_sel = np.array(goal_pix).reshape(ncam, ntask, 2)
        # the *_med arrays are what act() derives (:183,190); the reference tiles goal_pix over r first
        c.desig_pix_t0_med = (c.desig_pix_t0 * H / pred_height).astype(int)
        c.goal_pix_med = (c.goal_pix_sel * H / pred_height).astype(int)
        return c

    cases = [  # name, seed, ncam, ntask, H, W, regs, region, pred_height, pix_t0, goal_pix
        ('region64', 41, 2, 3, 64, 64, ['start', 'goal'], True, 64,
         [[[0, 0], [63, 63], [1, 62]], [[30, 31], [62, 2], [17, 40]]],
         [[[63, 63], [0, 0], [62, 1]], [[5, 60], [33, 33], [63, 0]]]),
        ('region128', 42, 1, 2, 128, 128, ['start', 'goal'], True, 128,
         [[[3, 125], [70, 64]]], [[[126, 2], [127, 127]]]),
        ('region48x64', 43, 1, 2, 48, 64, ['start', 'goal'], True, 48,
         [[[47, 10], [20, 63]]], [[[0, 63], [47, 0]]]),
        ('point64', 44, 2, 2, 64, 64, ['start', 'goal'], False, 64,
         [[[0, 0], [63, 63]], [[30, 31], [12, 50]]], [[[63, 0], [9, 9]], [[5, 60], [33, 33]]]),
        ('point_start_only', 45, 1, 2, 64, 64, ['start'], False, 64,
         [[[10, 20], [40, 41]]], [[[1, 1], [2, 2]]]),
        ('region_medium', 46, 1, 2, 96, 96, ['start', 'goal'], True, 48,
         [[[10, 40], [47, 0]]], [[[24, 24], [0, 47]]]),
    ]
    for name, seed, ncam, ntask, H, W, regs, region, ph, pix_t0, goal_pix in cases:
        start, goal, cur, ws, ps, wg, pg = registration_inputs(seed, ncam, H, W)
        c = make(ncam, ntask, H, W, regs, region, ph, pix_t0, goal_pix)
        for icam in range(ncam):
            with quiet():
                e, d = c.get_warp_err(icam, start, goal, ps, pg if 'goal' in regs else None, ws,
                                      wg if 'goal' in regs else None)
            arrays['%s/cam%d/warperrs' % (name, icam)] = e
            arrays['%s/cam%d/desig' % (name, icam)] = d
        meta['cases'].append({'name': name, 'seed': seed, 'ncam': ncam, 'ntask': ntask, 'H': H, 'W': W,
                              'regs': regs, 'region': region, 'pred_height': ph,
                              'pix_t0': pix_t0, 'goal_pix': goal_pix, 'flow_scale': 2.5})
    # region mode with only 'start' registered: the goal half of the region branch is unconditional
    # (:152-160) and indexes goal_warp_pts = None
    start, goal, cur, ws, ps, wg, pg = registration_inputs(47, 1, 64, 64)
    c = make(1, 1, 64, 64, ['start'], True, 64, [[[5, 5]]], [[[6, 6]]])
    try:
        with quiet():
            c.get_warp_err(0, start, goal, ps, None, ws, None)
        meta['region_start_only'] = 'ok'
    except TypeError:
        meta['region_start_only'] = 'TypeError'

    # the whole register_gtruth (:54-111) with the fake warper behind goal_image_warper
    from tests.helpers.flow_warper import make_flow_warper
    for name, seed, ncam, ntask, H, W, region in [('full64', 51, 2, 2, 64, 64, True),
                                                   ('full128', 52, 1, 1, 128, 128, True)]:
        rs = np.random.RandomState(seed)
        start, goal, cur = (rs.uniform(0, 1, (ncam, H, W, 3)).astype(np.float32) for _ in range(3))
        pix_t0 = rs.randint(0, [H, W], (ncam, ntask, 2))
        goal_pix = rs.randint(0, [H, W], (ncam, ntask, 2))
        c = make(ncam, ntask, H, W, ['start', 'goal'], region, H, pix_t0, goal_pix)
        warper = make_flow_warper(2.5)
        c.goal_image_warper = lambda a, b: warper(a[0], b[0])       # the reference adds a batch axis (:64-66)
        c.goal_image, c.start_image = goal, start
        c._net_context, c.plan_stat, c.vd = 2, {}, types.SimpleNamespace()
        last_frames = np.stack([np.zeros_like(cur), cur], 0)[None]   # [1, n_context, ncam, H, W, 3]
        with quiet():
            _, _, tradeoff = c.register_gtruth(start, last_frames)
        arrays[name + '/pix_t0'], arrays[name + '/goal_pix'] = pix_t0, goal_pix
        arrays[name + '/desig_pix'] = c.desig_pix
        arrays[name + '/tradeoff'] = tradeoff
        arrays[name + '/warperrs'] = c.plan_stat['warperrs']
        meta['cases'].append({'name': name, 'seed': seed, 'ncam': ncam, 'ntask': ntask, 'H': H, 'W': W,
                              'regs': ['start', 'goal'], 'region': region, 'full': True, 'flow_scale': 2.5})
    return arrays, meta


# ----------------------------------------------------------------------------- inverse-model policy
INVERSE_MODEL_EPISODES = (   # name, seed, policy overrides, actions per plan of the fake, steps, steps after the second reset()
    ('replan2', 7, {'T': 3}, 3, 9, 4),                          # num_context 2, replan_every 2 (the defaults)
    ('replan2_short', 7, {'T': 3}, 1, 9, 4),                    # ... and a plan of one action: it runs out at its second step
    ('replan1', 8, {'T': 2, 'replan_every': 1}, 2, 5, 3),
    ('replan1_short', 8, {'T': 2, 'replan_every': 1}, 0, 5, 3),  # ... and an empty plan
)


def inverse_model_inputs(seed, steps, H=16, W=16, ncam=2):
    """The image stream and the goal of an episode: uint8 frames ``[steps, ncam, H, W, 3]``, float64 goal ``[1, ncam, H, W, 3]``."""
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, (steps, ncam, H, W, 3)).astype(np.uint8), rs.uniform(0, 1, (1, ncam, H, W, 3))


def run_inverse_model_episode(ctrl_class, fake, seed, overrides, steps, steps_again):
    """Drive a controller class (the reference's while minting, this repo's in tests/test_inverse_model.py) through one
    episode, ``reset()`` and a second one -> (arrays, meta)."""
    ag = {'adim': 4, 'sdim': 5, 'image_height': 16, 'image_width': 16}
    frames, goal = inverse_model_inputs(seed, max(steps, steps_again))
    ctrl = ctrl_class(ag, dict(overrides), 0, 1)
    pred = fake.instances[-1]
    arrays, meta = {}, {'seed': seed, 'overrides': overrides, 'steps': steps, 'steps_again': steps_again,
                        'constructed': {'model_params_path': pred.model_params_path, 'n_gpus': pred.n_gpus,
                                        'first_gpu': pred.first_gpu, 'restored': pred.restored}}
    try:
        ctrl.act(t=0, i_tr=0, images=frames[:1], goal_image=goal)
        meta['act_before_reset'] = 'ok'
    except AttributeError as e:
        meta['act_before_reset'] = 'AttributeError: ' + str(e).split("'")[-2]
    for episode, n in enumerate((steps, steps_again)):
        ctrl.reset()
        np.random.seed(seed + 100 * episode)
        actions, counters, error = [], [], None
        for t in range(n):
            try:
                out = ctrl.act(t=t, i_tr=episode, images=frames[:t + 1], goal_image=goal)
            except AssertionError as e:
                error = {'t': t, 'text': str(e)}
                break
            assert out['plan_stat'] is ctrl.plan_stat and out['plan_stat'] == {}
            actions.append(np.asarray(out['actions'], dtype=np.float64))
            counters.append(ctrl.action_counter)
        if actions:
            arrays['ep%d/actions' % episode] = np.stack(actions)
            arrays['ep%d/context_frames' % episode] = np.stack(ctrl.context_frames)
            arrays['ep%d/context_actions' % episode] = np.stack([np.asarray(a, np.float64) for a in ctrl.context_actions])
        meta['ep%d' % episode] = {'counters': counters, 'error': error, 'calls_so_far': len(pred.calls),
                                  'action_dtypes': [str(np.asarray(a).dtype) for a in actions]}
    meta['calls'] = pred.calls
    return arrays, meta


def golden_inverse_model():
    """Run the reference's REAL ``InvModelBaseController`` (``visual_mpc/policy/inverse_models/
    inverse_model_base_controller.py``) behind an import stub for ``robonet.inverse_model.testing.
    action_inference_interface`` (absent from the snapshot) whose ``ActionInferenceInterface`` is the deterministic fake of
    ``tests/helpers/fake_action_inference.py`` - the default ``predictor_class`` the reference then constructs."""
    from tests.helpers.fake_action_inference import make_fake_action_inference
    arrays, meta = {}, {'numpy': np.__version__, 'episodes': {}}
    for name, seed, overrides, n_plan, steps, steps_again in INVERSE_MODEL_EPISODES:
        fake = make_fake_action_inference(n_plan, 4)
        base = 'robonet.inverse_model'
        im, testing, aii = (types.ModuleType(base), types.ModuleType(base + '.testing'),
                            types.ModuleType(base + '.testing.action_inference_interface'))
        aii.ActionInferenceInterface = fake
        im.testing, testing.action_inference_interface = testing, aii
        sys.modules['robonet'].inverse_model = im
        sys.modules.update({base: im, base + '.testing': testing, base + '.testing.action_inference_interface': aii})
        sys.modules.pop('visual_mpc.policy.inverse_models.inverse_model_base_controller', None)   # (binds the class at import)
        from visual_mpc.policy.inverse_models.inverse_model_base_controller import InvModelBaseController
        with quiet():
            a, m = run_inverse_model_episode(InvModelBaseController, fake, seed, overrides, steps, steps_again)
        arrays.update({name + '/' + k: v for k, v in a.items()})
        meta['episodes'][name] = m
    return arrays, meta


def main():
    install_stubs()
    from visual_mpc.policy.cem_controllers import PixelCostController, CEMBaseController
    ref = {'PixelCostController': PixelCostController, 'CEMBaseController': CEMBaseController}
    os.makedirs(OUT, exist_ok=True)

    def dump(name, arrays, meta):
        if arrays:
            np.savez_compressed(os.path.join(OUT, name + '.npz'), **arrays)
        with open(os.path.join(OUT, name + '.json'), 'w') as f:
            json.dump(jsonable(meta), f, indent=1, sort_keys=True)

    dump('policy_args', None, golden_policy_args(ref))
    dump('hparams', None, golden_hparams(ref))
    dump('sampler', *golden_sampler(ref))
    dump('cost', *golden_cost(ref))
    dump('act', *golden_act(ref))
    dump('pred_util', *golden_pred_util(ref))
    dump('traj_layout', *golden_traj_layout())
    dump('registration', *golden_registration())
    dump('inverse_model', *golden_inverse_model())
    dump('experiment_files', None, golden_experiment_files())
    print('wrote fixtures to', OUT, 'with numpy', np.__version__)
    for fn in sorted(os.listdir(OUT)):
        print('  %-20s %8d B' % (fn, os.path.getsize(os.path.join(OUT, fn))))


if __name__ == '__main__':
    main()
