"""The plain-bf16 precision mode (``precision='bf16'``, vf_config.precision = 2) on whole rollouts: determinism, accuracy class,
and its surface.  Exactness of the gate tile is tests/test_gpu_bf16_layer.py's business - a rollout cannot pin it (one bf16 flip
moves whole frames through LayerNorm and the normalised CDNA kernels), so the accuracy check here is a wide two-sided band
around the rounding twin of the oracle (tests/helpers/oracle_bf16.py) in float64: its RMS distance to the float64 oracle is the
size of the rounding effect, stable within 1.6x over these shapes while the twin in float32 vs float64 moved by 1/3 .. 1/3000 of
it.  Above 4x: an error compounding outside the tile (LayerNorm staging, late-start items); below 1/4: the mode runs something
else."""
import functools
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from oracle import pixel_cost                                           # noqa: E402
from oracle.cdna_predictor import OracleCdna                            # noqa: E402
from oracle.savp_predictor import OracleSavp                            # noqa: E402
from tests.helpers.oracle_bf16 import OracleCdnaBf16, OracleSavpBf16    # noqa: E402
from visual_foresight_amd import _lib                                   # noqa: E402
from visual_foresight_amd.video_prediction.cdna_arch import CdnaConfig, CdnaWeights   # noqa: E402
from visual_foresight_amd.video_prediction.savp_arch import SavpConfig  # noqa: E402

SHAPES = [('cdna', 64, 64, 3, 5, 1), ('cdna', 48, 64, 2, 5, 2), ('cdna', 32, 32, 4, 9, 1)]
ARCH = {'cdna': (CdnaConfig, OracleCdna, OracleCdnaBf16, 4), 'savp': (SavpConfig, OracleSavp, OracleSavpBf16, 6)}


def _predictor(arch, H, W, T, nd, bs, precision='bf16', **extra):
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    adim = ARCH[arch][3]
    hp = dict(designated_pixel_count=nd, run_batch_size=bs, adim=adim, sdim=5, image_height=H, image_width=W,
              sequence_length=T + 2, precision=precision, **extra)
    if arch != 'cdna':
        hp['arch'] = arch
    pred = HipVPredEvaluation('', hp)
    cfg = ARCH[arch][0](height=H, width=W, adim=adim, ndesig=nd, sequence_length=T + 2)
    weights = CdnaWeights.random(cfg, seed=3, bias_scale=0.05, ln_jitter=0.1)      # the weights of tests/test_gpu_parity.py
    pred.restore(weights)
    return pred, weights


@functools.lru_cache(maxsize=None)
def _inputs(arch, H, W, T, M, nd):
    adim = ARCH[arch][3]
    rs = np.random.RandomState(H + W + T + M)
    desig = np.stack([rs.randint(0, H, (1, nd)), rs.randint(0, W, (1, nd))], axis=-1)
    ctx = {'context_frames': rs.randint(0, 256, (2, 1, H, W, 3)).astype(np.uint8),
           'context_actions': rs.normal(0, 0.05, (1, adim)),
           'context_states': rs.normal(0, 0.1, (2, 5)),
           'context_pixel_distributions': pixel_cost.one_hot_distrib(desig, 2, 1, H, W, nd)}
    actions = rs.normal(0, 0.1, (M, T, adim))
    goal = np.stack([rs.randint(0, H, (1, nd)), rs.randint(0, W, (1, nd))], axis=-1)
    return ctx, actions, goal


@functools.lru_cache(maxsize=None)
def _device_run(arch, H, W, T, M, nd):
    """Scores and predictions of the precision-2 engine (persistent launch), computed once per shape."""
    ctx, actions, goal = _inputs(arch, H, W, T, M, nd)
    pred, weights = _predictor(arch, H, W, T, nd, bs=M)
    assert pred.precision == 2
    scores, _ = pred.score(ctx, {'actions': actions}, goal, finalweight=10.)
    out = pred(ctx, {'actions': actions})
    assert pred.device_status() == 0
    return pred, weights, scores, out


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.mark.parametrize('arch,H,W,T,M,nd', SHAPES)
def test_mode_is_deterministic(arch, H, W, T, M, nd):
    ctx, actions, goal = _inputs(arch, H, W, T, M, nd)
    pred, _, scores, out = _device_run(arch, H, W, T, M, nd)
    # a second call
    again, _ = pred.score(ctx, {'actions': actions}, goal, finalweight=10.)
    assert _same_bits(again, scores)
    assert _same_bits(pred(ctx, {'actions': actions})['predicted_frames'], out['predicted_frames'])
    # per-layer launches
    layered, _ = _predictor(arch, H, W, T, nd, bs=M, persistent=0)
    got, _ = layered.score(ctx, {'actions': actions}, goal, finalweight=10.)
    assert _same_bits(got, scores)
    lo = layered(ctx, {'actions': actions})
    assert _same_bits(lo['predicted_frames'], out['predicted_frames'])
    assert _same_bits(lo['predicted_pixel_distributions'], out['predicted_pixel_distributions'])
    # a sample alone, and the same sample in a slot of a ragged batch of a larger engine
    alone = pred(ctx, {'actions': actions[2:3]})
    assert _same_bits(alone['predicted_frames'][0], out['predicted_frames'][2])
    larger, _ = _predictor(arch, H, W, T, nd, bs=M + 3)
    ragged = larger(ctx, {'actions': np.concatenate([actions[4:5], actions[:M - 1]])})
    assert _same_bits(ragged['predicted_frames'][3], out['predicted_frames'][2])
    assert _same_bits(ragged['predicted_pixel_distributions'][3], out['predicted_pixel_distributions'][2])
    s_r, _ = larger.score(ctx, {'actions': np.concatenate([actions[4:5], actions[:M - 1]])}, goal, finalweight=10.)
    assert _same_bits(s_r[3], scores[2]) and _same_bits(s_r[0], scores[4])


def _rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


@pytest.mark.parametrize('arch,H,W,T,M,nd', SHAPES + [('savp', 128, 128, 1, 2, 1)])
def test_accuracy_class_is_that_of_the_rounding_twin(arch, H, W, T, M, nd):
    ctx, actions, goal = _inputs(arch, H, W, T, M, nd)
    _, weights, scores, out = _device_run(arch, H, W, T, M, nd)
    args = (ctx['context_frames'], ctx['context_actions'], ctx['context_pixel_distributions'], ctx['context_states'], actions)
    f64, d64, _ = ARCH[arch][1](weights, torch.float64).rollout(*args)
    ft, dt, _ = ARCH[arch][2](weights, torch.float64).rollout(*args)
    dmax = d64.max(axis=(3, 4), keepdims=True)
    twin_f, twin_d = _rms(ft, f64), _rms(dt / dmax, d64 / dmax)
    got_f = _rms(out['predicted_frames'], f64)
    got_d = _rms(out['predicted_pixel_distributions'] / dmax, d64 / dmax)
    print('%s %dx%d T%d M%d nd%d: RMS to float64 oracle, frames %.3g (twin %.3g, x%.2f), distributions %.3g (twin %.3g, x%.2f)'
          % (arch, H, W, T, M, nd, got_f, twin_f, got_f / twin_f, got_d, twin_d, got_d / twin_d))
    assert twin_f > 0 and twin_d > 0
    assert twin_f / 4 <= got_f <= 4 * twin_f
    assert twin_d / 4 <= got_d <= 4 * twin_d
    # and it is not precision 0 under another name
    exact, _ = _predictor(arch, H, W, T, nd, bs=M, precision='fp32')
    s0, _ = exact.score(ctx, {'actions': actions}, goal, finalweight=10.)
    assert not _same_bits(s0, scores)


def test_keys_that_select_the_mode(monkeypatch):
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    hp = dict(designated_pixel_count=1, run_batch_size=2, image_height=32, image_width=32, sequence_length=4)
    for key in ('bf16', 2, '2'):
        assert HipVPredEvaluation('', dict(hp, precision=key)).precision == 2
    monkeypatch.setenv('VF_PRECISION', 'bf16')
    assert HipVPredEvaluation('', hp).precision == 2
    assert HipVPredEvaluation('', dict(hp, precision='fp32')).precision == 0
    assert HipVPredEvaluation('', dict(hp, float16='')).precision == 1       # the bare float16 key keeps the split-bf16 mode
    monkeypatch.delenv('VF_PRECISION')
    # the ensemble and stochastic wrappers hand the key to their engines
    from visual_foresight_amd.video_prediction.ensemble_predictor import EnsembleHipPredictor
    from visual_foresight_amd.video_prediction.stochastic_predictor import StochasticHipPredictor
    ens = EnsembleHipPredictor('', dict(hp, precision='bf16', num_ensembles=2))
    assert [m.precision for m in ens.members] == [2, 2]
    sto = StochasticHipPredictor('', dict(hp, precision='bf16', adim=4, n_latent=2))
    assert sto.precision == 2


def test_nothing_is_allocated_after_create():
    """tests/test_gpu_abi.py's rule at precision 'bf16': weight hot-swaps (which re-pack the bf16 plane), context changes, ragged
    batches and exports leave the device's free memory untouched."""
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation

    def small():
        hp = dict(designated_pixel_count=1, run_batch_size=8, adim=4, sdim=5, image_height=32, image_width=32,
                  sequence_length=4, precision='bf16')
        return HipVPredEvaluation('', hp).restore()
    pred = small()
    rs = np.random.RandomState(1)
    ctx = {'context_frames': rs.randint(0, 256, (2, 1, 32, 32, 3)).astype(np.uint8),
           'context_actions': rs.normal(0, 0.05, (1, 4)), 'context_states': rs.normal(0, 0.1, (2, 5)),
           'context_pixel_distributions': pixel_cost.one_hot_distrib([[[16, 16]]], 2, 1, 32, 32, 1)}
    actions = rs.normal(0, 0.1, (8, 2, 4))
    cfg = pred.cfg
    pred(ctx, {'actions': actions[:3]})
    free0 = None
    for i in range(4):          # round 0 warms PyTorch's own caching allocator
        pred.restore(CdnaWeights.random(cfg, seed=40 + i))
        for n in (8, 5, 8, 1):
            pred.score(ctx, {'actions': actions[:n]}, [[[3 + i, 20]]])
        pred.fetch_pixel_distributions(0)
        if i == 0:
            torch.cuda.synchronize()
            free0 = torch.cuda.mem_get_info(pred.device)[0]
    pred.restore(CdnaWeights.random(cfg, seed=40))
    s, _ = pred.score(ctx, {'actions': actions}, [[[3, 20]]])
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info(pred.device)[0] == free0
    fresh = small()
    fresh.restore(CdnaWeights.random(cfg, seed=40))
    np.testing.assert_array_equal(fresh.score(ctx, {'actions': actions}, [[[3, 20]]])[0], s)


def test_c_host_agrees_with_the_python_host_at_precision_2(tmp_path):
    from tests.test_gpu_c_host import build_c_host
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    H = W = 32
    nd, M, T, nc, adim, sdim, nex = 1, 5, 2, 2, 4, 5, 2
    cfg = CdnaConfig(height=H, width=W, ndesig=nd, sequence_length=T + nc)
    weights = CdnaWeights.random(cfg, seed=11, bias_scale=0.05, ln_jitter=0.1)
    rs = np.random.RandomState(7)
    desig = rs.randint(0, H, (1, nd, 2))
    ctx = {'context_frames': rs.randint(0, 256, (nc, 1, H, W, 3)).astype(np.uint8),
           'context_actions': rs.normal(0, 0.05, (nc - 1, adim)), 'context_states': rs.normal(0, 0.1, (nc, sdim)),
           'context_pixel_distributions': pixel_cost.one_hot_distrib(desig, nc, 1, H, W, nd)}
    actions = rs.normal(0, 0.1, (M, T, adim))
    goal = rs.randint(0, H, (1, nd, 2))
    fw = 7.5
    hp = dict(designated_pixel_count=nd, run_batch_size=M, adim=adim, sdim=sdim, image_height=H, image_width=W,
              sequence_length=T + nc, precision='bf16')
    pred = HipVPredEvaluation('', hp)
    pred.restore(weights)
    scores, per_task = pred.score(ctx, {'actions': actions}, goal, finalweight=fw)
    out = pred(ctx, {'actions': actions[:nex]})

    blob = np.concatenate([v.ravel() for v in weights.tensors.values()]).astype(np.float32)
    inp, outp = tmp_path / 'in.bin', tmp_path / 'out.bin'
    with open(inp, 'wb') as f:
        np.array([H, W, adim, sdim, nd, nc, T + nc, M, nex, blob.size], np.int32).tofile(f)
        blob.tofile(f)
        ctx['context_frames'].tofile(f)
        ctx['context_states'].astype(np.float32).tofile(f)
        ctx['context_actions'].astype(np.float32).tofile(f)
        ctx['context_pixel_distributions'].astype(np.float32).tofile(f)
        actions.astype(np.float32).tofile(f)
        goal.astype(np.int32).tofile(f)
        np.array([fw], np.float32).tofile(f)
    exe = build_c_host(tmp_path)
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.dirname(_lib.LIB_PATH) + ':' + os.environ.get('LD_LIBRARY_PATH', ''))
    proc = subprocess.run([exe, str(inp), str(outp), '2'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                          env=env, timeout=600)
    assert proc.returncode == 0, proc.stdout
    raw = np.fromfile(outp, np.uint8)
    n_s, n_p = M * 8, M * nd * 8
    n_f = nex * T * H * W * 3 * 4
    c_scores = raw[:n_s].view(np.float64)
    c_per_task = raw[n_s:n_s + n_p].view(np.float64).reshape(M, nd)
    c_frames = raw[n_s + n_p:n_s + n_p + n_f].view(np.float32).reshape(nex, T, 1, H, W, 3)
    np.testing.assert_array_equal(c_scores, scores)
    np.testing.assert_array_equal(c_per_task, per_task)
    np.testing.assert_array_equal(c_frames, out['predicted_frames'])
    # ... and precision 2 it was: the exact mode gives other bits
    proc0 = subprocess.run([exe, str(inp), str(outp)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env,
                           timeout=600)
    assert proc0.returncode == 0, proc0.stdout
    assert not np.array_equal(np.fromfile(outp, np.uint8)[:n_s].view(np.float64), scores)
