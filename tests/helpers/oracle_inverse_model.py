"""PyTorch-CPU restatement of the action-inference network (``visual_foresight_amd/video_prediction/inverse_model_arch.py``:
two convolution towers of four 3x3 / 2 layers with a mean over the positions, an LSTM cell of 128 units that is warmed up
on the context and then decodes ``n_actions`` actions) in float32 AND float64, plus naive NumPy loops of each block for
tiny shapes.  Test infrastructure only."""
import numpy as np
import torch
import torch.nn.functional as F

UNITS = 128


def conv_block(x, w, b):
    """x ``[n, H, W, Cin]``, w ``[3, 3, Cin, Cout]`` -> relu(conv 3x3 / 2, zero pad 1, + b) ``[n, H/2, W/2, Cout]``."""
    return F.relu(F.conv2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), b, stride=2, padding=1)).permute(0, 2, 3, 1)


def tower_block(x, t, tower):
    """``[n, H, W, Cin]`` -> ``[n, 128]``: c1 .. c4, then the mean over the positions."""
    for l in range(1, 5):
        x = conv_block(x, t['%s/c%d/w' % (tower, l)], t['%s/c%d/b' % (tower, l)])
    return x.reshape(x.shape[0], -1, x.shape[3]).mean(dim=1)


def cell_block(x, a, h, c, t, order=0):
    """One LSTM step on ``x [n, 128]``, ``a [n, adim]``, ``h``, ``c [n, 128]`` -> ``(h', c')``.  ``order`` 1 adds the terms of
    the gate sum the other way round (for the spread between two float32 summation orders)."""
    if order == 0:
        z = t['lstm/b'] + x @ t['lstm/wx'] + a @ t['lstm/wa'] + h @ t['lstm/wh']
    else:
        z = h @ t['lstm/wh'] + (a @ t['lstm/wa'] + (x @ t['lstm/wx'] + t['lstm/b']))
    i, f, g, o = (z[:, k * UNITS:(k + 1) * UNITS] for k in range(4))
    c2 = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c2), c2


def forward(weights, start, goal, ctx_actions, ctx_frames, dtype=torch.float64, order=0):
    """``start``, ``goal [n, H, W, 3]``, ``ctx_actions [n, n_context, adim]``, ``ctx_frames [n, n_context, H, W, 3]`` (float32
    values) -> ``(actions [n, n_actions, adim], hidden [n, n_context + n_actions, 2, 128])`` in ``dtype``."""
    cfg = weights.cfg
    as_t = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dtype)
    start, goal, ctx_actions, ctx_frames = as_t(start), as_t(goal), as_t(ctx_actions), as_t(ctx_frames)
    t = {k: torch.from_numpy(v).to(dtype) for k, v in weights.tensors.items()}
    scale = torch.tensor(np.float32(cfg.input_scale)).to(dtype)
    n = start.shape[0]
    with torch.no_grad():
        p = tower_block(torch.cat([goal, start], dim=-1) * scale, t, 'pair')
        q = tower_block(ctx_frames.reshape((n * cfg.n_context,) + tuple(ctx_frames.shape[2:])) * scale, t, 'ctx')
        q = q.reshape(n, cfg.n_context, UNITS)
        h = torch.zeros((n, UNITS), dtype=dtype)
        c = torch.zeros((n, UNITS), dtype=dtype)
        hidden, actions = [], []
        for i in range(cfg.n_context):
            h, c = cell_block(q[:, i], ctx_actions[:, i], h, c, t, order)
            hidden.append(torch.stack([h, c], dim=1))
        a = ctx_actions[:, -1]
        for _ in range(cfg.n_actions):
            h, c = cell_block(p, a, h, c, t, order)
            hidden.append(torch.stack([h, c], dim=1))
            a = t['out/b'] + h @ t['out/w']
            actions.append(a)
        return torch.stack(actions, dim=1).numpy(), torch.stack(hidden, dim=1).numpy()


# ----------------------------------------------------------------------------------------------- naive loops (tiny shapes)
def naive_conv_block(x, w, b):
    x, w, b = [np.asarray(a, dtype=np.float64) for a in (x, w, b)]
    n, H, W, _ = x.shape
    out = np.zeros((n, H // 2, W // 2, w.shape[3]))
    for i in range(n):
        for oy in range(H // 2):
            for ox in range(W // 2):
                acc = b.copy()
                for ky in range(3):
                    for kx in range(3):
                        iy, ix = 2 * oy + ky - 1, 2 * ox + kx - 1
                        if 0 <= iy < H and 0 <= ix < W:
                            acc += x[i, iy, ix] @ w[ky, kx]
                out[i, oy, ox] = np.maximum(acc, 0.)
    return out


def naive_pool_block(x):
    x = np.asarray(x, dtype=np.float64)
    n, H, W, C = x.shape
    out = np.zeros((n, C))
    for r in range(H):
        for c in range(W):
            out += x[:, r, c]
    return out / (H * W)


def naive_cell_block(x, a, h, c, wx, wa, wh, b):
    x, a, h, c, wx, wa, wh, b = [np.asarray(v, dtype=np.float64) for v in (x, a, h, c, wx, wa, wh, b)]
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    h2, c2 = np.zeros_like(h), np.zeros_like(c)
    for u in range(UNITS):
        z = []
        for gate in range(4):
            col = gate * UNITS + u
            acc = b[col]
            for k in range(x.shape[0]):
                acc += x[k] * wx[k, col]
            for k in range(a.shape[0]):
                acc += a[k] * wa[k, col]
            for k in range(h.shape[0]):
                acc += h[k] * wh[k, col]
            z.append(acc)
        c2[u] = sig(z[1]) * c[u] + sig(z[0]) * np.tanh(z[2])
        h2[u] = sig(z[3]) * np.tanh(c2[u])
    return h2, c2


def naive_forward(weights, start, goal, ctx_actions, ctx_frames):
    """One problem (no batch axis) through naive loops, float64 -> ``(actions [n_actions, adim], hidden)``."""
    cfg, t = weights.cfg, weights.tensors
    s = np.float64(np.float32(cfg.input_scale))

    def tower(x, name):
        x = np.asarray(x, dtype=np.float64)[None] * s
        for l in range(1, 5):
            x = naive_conv_block(x, t['%s/c%d/w' % (name, l)], t['%s/c%d/b' % (name, l)])
        return naive_pool_block(x)[0]

    p = tower(np.concatenate([goal, start], axis=-1), 'pair')
    h, c = np.zeros(UNITS), np.zeros(UNITS)
    hidden, actions = [], []
    lstm = [t['lstm/wx'], t['lstm/wa'], t['lstm/wh'], t['lstm/b']]
    for i in range(cfg.n_context):
        h, c = naive_cell_block(tower(ctx_frames[i], 'ctx'), ctx_actions[i], h, c, *lstm)
        hidden.append(np.stack([h, c]))
    a = np.asarray(ctx_actions[-1], dtype=np.float64)
    for _ in range(cfg.n_actions):
        h, c = naive_cell_block(p, a, h, c, *lstm)
        hidden.append(np.stack([h, c]))
        a = np.asarray(t['out/b'], dtype=np.float64) + h @ np.asarray(t['out/w'], dtype=np.float64)
        actions.append(a)
    return np.stack(actions), np.stack(hidden)
