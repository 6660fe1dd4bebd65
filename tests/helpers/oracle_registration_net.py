"""PyTorch-CPU restatement of the registration network (``visual_foresight_amd/video_prediction/registration_net_arch.py``:
3x3 convolutions with zero padding 1, bias, ReLU; 2x2 max-pool on the way down, four-tap bilinear transposed convolution on
the way up; a 5x5 flow head) in float32 AND float64, plus naive NumPy loops of each block for tiny shapes.  Test
infrastructure only."""
import numpy as np
import torch
import torch.nn.functional as F


def conv_block(x, w, b, relu=True):
    """x ``[n, H, W, Cin]``, w ``[k, k, Cin, Cout]`` -> conv k x k / 1, zero pad k // 2, + b (, ReLU) ``[n, H, W, Cout]``."""
    y = F.conv2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), b, padding=w.shape[0] // 2)
    return (F.relu(y) if relu else y).permute(0, 2, 3, 1)


def pool_block(x):
    return F.max_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)


def bilinear_kernel_1d():
    return 1.0 - np.abs(np.arange(4) - 1.5) / 2.0


def upsample_block(x):
    C = x.shape[3]
    v = bilinear_kernel_1d()
    k = torch.from_numpy(np.outer(v, v)).to(x.dtype).view(1, 1, 4, 4).expand(C, 1, 4, 4).contiguous()
    return F.conv_transpose2d(x.permute(0, 3, 1, 2), k, stride=2, padding=1, groups=C).permute(0, 2, 3, 1)


def forward(weights, current, reference, dtype=torch.float64):
    """One view: ``current``, ``reference [n, H, W, 3]`` (float32 values) -> flow ``[n, H, W, 2]`` in ``dtype``."""
    x = torch.cat([torch.from_numpy(np.ascontiguousarray(current, dtype=np.float32)),
                   torch.from_numpy(np.ascontiguousarray(reference, dtype=np.float32))], dim=-1).to(dtype)
    t = {k: torch.from_numpy(v).to(dtype) for k, v in weights.tensors.items()}
    with torch.no_grad():
        for name in ('d1', 'd2', 'd3'):
            x = pool_block(conv_block(x, t[name + '/w'], t[name + '/b']))
        for name in ('u1', 'u2', 'u3'):
            x = upsample_block(conv_block(x, t[name + '/w'], t[name + '/b']))
        return conv_block(x, t['flow/w'], t['flow/b'], relu=False).contiguous().numpy()


def forward_views(weight_views, current, reference, dtype=torch.float64):
    """``current``, ``reference [n, ncam, H, W, 3]`` -> ``[n, ncam, H, W, 2]``."""
    current, reference = np.asarray(current), np.asarray(reference)
    return np.stack([forward(w, current[:, c], reference[:, c], dtype) for c, w in enumerate(weight_views)], axis=1)


# ----------------------------------------------------------------------------------------------- naive loops (tiny shapes)
def naive_conv_block(x, w, b, relu=True):
    x, w, b = [np.asarray(a, dtype=np.float64) for a in (x, w, b)]
    n, H, W, _ = x.shape
    k, pad = w.shape[0], w.shape[0] // 2
    out = np.zeros((n, H, W, w.shape[3]))
    for i in range(n):
        for oy in range(H):
            for ox in range(W):
                acc = b.copy()
                for ky in range(k):
                    for kx in range(k):
                        iy, ix = oy + ky - pad, ox + kx - pad
                        if 0 <= iy < H and 0 <= ix < W:
                            acc += x[i, iy, ix] @ w[ky, kx]
                out[i, oy, ox] = np.maximum(acc, 0.) if relu else acc
    return out


def naive_pool_block(x):
    x = np.asarray(x, dtype=np.float64)
    n, H, W, C = x.shape
    out = np.zeros((n, H // 2, W // 2, C))
    for r in range(H // 2):
        for c in range(W // 2):
            out[:, r, c] = np.maximum(np.maximum(x[:, 2 * r, 2 * c], x[:, 2 * r, 2 * c + 1]),
                                      np.maximum(x[:, 2 * r + 1, 2 * c], x[:, 2 * r + 1, 2 * c + 1]))
    return out


def naive_upsample_block(x):
    """out[o] += in[i] * k[o - 2 i + 1] on both axes (transposed convolution, stride 2, padding 1)."""
    x = np.asarray(x, dtype=np.float64)
    n, H, W, C = x.shape
    k = bilinear_kernel_1d()
    out = np.zeros((n, 2 * H, 2 * W, C))
    for iy in range(H):
        for ix in range(W):
            for ky in range(4):
                for kx in range(4):
                    oy, ox = 2 * iy - 1 + ky, 2 * ix - 1 + kx
                    if 0 <= oy < 2 * H and 0 <= ox < 2 * W:
                        out[:, oy, ox] += x[:, iy, ix] * (k[ky] * k[kx])
    return out
