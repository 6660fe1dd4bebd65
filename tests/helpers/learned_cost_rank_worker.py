"""One rank of the multi-rank learned-cost test: ``HipVPredEvaluation.score_frames`` on a fixed candidate set with both
heads, ranks sharing one GPU over gloo; writes the score rows and ``last_frame_cost_per_step``."""
import os
import pickle
import sys

import numpy as np

H, W, T, M, NCAM, EMBED = 64, 64, 3, 24, 2, 16


def build(run_batch_size=M, n_gpus=1, **extra):
    """The predictor, both scorers, the context, the candidates and the goal embedding of the bit-identity tests."""
    from visual_foresight_amd.video_prediction.frame_scorer import HipFrameScorer
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    hp = dict(designated_pixel_count=1, run_batch_size=run_batch_size, adim=4, sdim=5, image_height=H, image_width=W,
              sequence_length=T + 2, ncam=NCAM, **extra)
    pred = HipVPredEvaluation('', hp, n_gpus=n_gpus, first_gpu=0).restore()
    shp = dict(image_height=H, image_width=W, ncam=NCAM, max_frames=M * T, bias_scale=0.2)
    scorers = {'classifier': HipFrameScorer('', dict(shp, head='classifier', seed=5), pred.device).restore(),
               'embedding': HipFrameScorer('', dict(shp, head='embedding', embed_dim=EMBED, seed=9), pred.device).restore()}
    rs = np.random.RandomState(5)
    ctx = {'context_frames': rs.randint(0, 256, (2, NCAM, H, W, 3)).astype(np.uint8),
           'context_actions': rs.normal(0, 0.05, (1, 4)), 'context_states': rs.normal(0, 0.1, (2, 5))}
    actions = rs.normal(0, 0.1, (M, T, 4))
    goal = rs.uniform(0, 1, (NCAM, H, W, 3)).astype(np.float32)
    goal_enc = scorers['embedding'].goal_enc(goal, ctx['context_frames'][-1].astype(np.float32) / np.float32(255.))
    return pred, scorers, ctx, actions, goal_enc


def score_both(pred, scorers, ctx, actions, goal_enc, finalweight=4.):
    out = {}
    for head, scorer in scorers.items():
        s = pred.score_frames(ctx, {'actions': actions}, scorer, goal_enc=goal_enc if head == 'embedding' else None,
                              finalweight=finalweight)
        out[head] = (s, pred.last_frame_cost_per_step)
    return out


def run(rank, world, port, out_dir):
    import torch.distributed as dist
    if world > 1:
        dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%d' % port, rank=rank, world_size=world)
    pred, scorers, ctx, actions, goal_enc = build()
    out = score_both(pred, scorers, ctx, actions, goal_enc)
    with open(os.path.join(out_dir, 'learned_rank%d_of%d.pkl' % (rank, world)), 'wb') as f:
        pickle.dump(out, f)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    rank, world, port, out_dir = sys.argv[1:5]
    run(int(rank), int(world), int(port), out_dir)
