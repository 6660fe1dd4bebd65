"""One rank of the multi-rank goal-image test: ``HipVPredEvaluation.score_goal_image`` on a fixed candidate set, ranks
sharing one GPU over gloo; writes the score rows and ``last_goal_cost_per_step``."""
import os
import pickle
import sys

import numpy as np


def run(rank, world, port, out_dir):
    import torch.distributed as dist
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    if world > 1:
        dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%d' % port, rank=rank, world_size=world)
    H = W = 32
    T, M = 3, 23
    hp = dict(designated_pixel_count=1, run_batch_size=M, adim=4, sdim=5, image_height=H, image_width=W,
              sequence_length=T + 2, ncam=2)
    pred = HipVPredEvaluation('', hp).restore()
    rs = np.random.RandomState(5)
    ctx = {'context_frames': rs.randint(0, 256, (2, 2, H, W, 3)).astype(np.uint8),
           'context_actions': rs.normal(0, 0.05, (1, 4)), 'context_states': rs.normal(0, 0.1, (2, 5))}
    actions = rs.normal(0, 0.1, (M, T, 4))
    goal = rs.randint(0, 256, (2, H, W, 3)).astype(np.uint8)
    scores, per_view = pred.score_goal_image(ctx, {'actions': actions}, goal, steps='weighted', finalweight=4.)
    out = {'scores': scores, 'per_view': per_view, 'cps': pred.last_goal_cost_per_step}
    with open(os.path.join(out_dir, 'goal_rank%d_of%d.pkl' % (rank, world)), 'wb') as f:
        pickle.dump(out, f)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    rank, world, port, out_dir = sys.argv[1:5]
    run(int(rank), int(world), int(port), out_dir)
