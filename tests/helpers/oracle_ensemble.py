"""Ensemble duck-type around the CPU oracle (test infrastructure only): one ``OracleCdna`` per member, no ``score``, so
``CEM_Controller_Ensemble_Vidpred`` scores it on the host from ``ensemble_pixel_distributions``."""
import numpy as np
import torch

from oracle.cdna_predictor import OracleCdna
from visual_foresight_amd.video_prediction.cdna_arch import CdnaConfig


def make_oracle_ensemble_class(weights_factory, num_ensembles, dtype=torch.float32):
    """``weights_factory(cfg, member)`` -> one single-view weight set per member."""
    class OracleEnsemble(object):
        wants_agent_params = True
        n_context_default = 2

        def __init__(self, model_path, hparams, n_gpus=1, first_gpu=0):
            hp = dict(hparams)
            self.n_context = 2
            self.sequence_length = hp['sequence_length']
            self.cfg = CdnaConfig(height=hp['image_height'], width=hp['image_width'], adim=hp['adim'],
                                  sdim=hp['sdim'], ndesig=hp['designated_pixel_count'],
                                  sequence_length=hp['sequence_length'])
            self.n_cam = 1

        def restore(self):
            self.oracles = [OracleCdna(weights_factory(self.cfg, m), dtype) for m in range(num_ensembles)]

        def __call__(self, context, inputs):
            frames, distribs = [], []
            for oracle in self.oracles:
                f, d, s = oracle.rollout(np.asarray(context['context_frames'])[:, :1], context['context_actions'],
                                         np.asarray(context['context_pixel_distributions'])[:, :1],
                                         context['context_states'], np.asarray(inputs['actions']))
                frames.append(f.astype(np.float32))
                distribs.append(d.astype(np.float32))
            ens = np.stack(distribs)
            return {'predicted_frames': np.mean(frames, axis=0), 'predicted_pixel_distributions': ens.mean(axis=0),
                    'ensemble_pixel_distributions': ens}

    return OracleEnsemble
