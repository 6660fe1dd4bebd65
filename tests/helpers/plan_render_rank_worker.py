"""One rank of the multi-rank plan-render test: ``HipVPredEvaluation.score`` on a fixed candidate set, ranks sharing one
GPU over gloo, then ``render_plans`` of a shuffled subset and a propagation fetch; writes the bytes."""
import os
import pickle
import sys

import numpy as np

INDICES = [17, 2, 9, 22, 11, 0, 5]


def run(rank, world, port, out_dir):
    import torch.distributed as dist
    from visual_foresight_amd.video_prediction.hip_predictor import HipVPredEvaluation
    if world > 1:
        dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%d' % port, rank=rank, world_size=world)
    H = W = 32
    T, M, ncam, nd = 3, 23, 2, 2
    hp = dict(designated_pixel_count=nd, run_batch_size=M, adim=4, sdim=5, image_height=H, image_width=W,
              sequence_length=T + 2, ncam=ncam)
    pred = HipVPredEvaluation('', hp).restore()
    rs = np.random.RandomState(5)
    distrib = np.zeros((2, ncam, H, W, nd), np.float32)
    distrib[:, :, 10, 12, 0] = 1.
    distrib[:, :, 20, 7, 1] = 1.
    ctx = {'context_frames': rs.randint(0, 256, (2, ncam, H, W, 3)).astype(np.uint8),
           'context_actions': rs.normal(0, 0.05, (1, 4)), 'context_states': rs.normal(0, 0.1, (2, 5)),
           'context_pixel_distributions': distrib}
    actions = rs.normal(0, 0.1, (M, T, 4))
    scores, _ = pred.score(ctx, {'actions': actions}, goal_pix=np.array([[[5, 5], [25, 25]]] * ncam))
    before = pred.fetch_pixel_distributions(9)
    out = pred.render_plans(INDICES)
    out['fetch_before'], out['fetch_after'] = before, pred.fetch_pixel_distributions(9)
    out['scores'] = scores
    with open(os.path.join(out_dir, 'render_rank%d_of%d.pkl' % (rank, world)), 'wb') as f:
        pickle.dump(out, f)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    rank, world, port, out_dir = sys.argv[1:5]
    run(int(rank), int(world), int(port), out_dir)
