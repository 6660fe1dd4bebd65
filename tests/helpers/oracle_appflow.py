"""CPU restatement of the appearance-flow predictor (test infrastructure only).

PARITY UNPINNED, like ``oracle/cdna_predictor.py``: the reference names the model (``'model': 'appflow'`` in its legacy
predictor configurations) but holds no network code, so ``cdna_arch.py`` (``CdnaConfig(transformation='flow')``) is the
specification and this file restates it in plain PyTorch CPU ops.  Everything up to ``enc6`` is ``OracleCdna``'s own layers;
the transformation is restated here::

    scratch = sigmoid(conv1x1(enc6, ->3));  masks = softmax_c(conv1x1(enc6, ->K+1))
    flow    = conv1x1(enc6, ->2*NF)                channel 2k = dx_k, 2k+1 = dy_k, in pixels      (NF = K - 1)
    warp_k(img)[y, x] = bilinear(img, x + dx_k[y, x], y + dy_k[y, x])
    frame'  = masks_0 * frame + masks_1 * scratch + sum_k masks_{k+2} * warp_k(frame)
    distr'  = normalise_hw(masks_0 * distr + sum_k masks_{k+2} * warp_k(distr))

``bilinear`` is the clamped sampler of ``oracle/registration.py`` (``bilinear_warp_loops``): coordinates clamped to the image,
``x1 = min(x0 + 1, W - 1)``, ``fmaf(fx, b - a, a)`` then ``fmaf(fy, bot - top, top)``.  In float32 the fused multiply-adds are
emulated the way that file emulates them: the product of two float32 values is exact in float64, one float64 addition, one
rounding to float32.  In float64 (used to measure rounding) they are plain arithmetic.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.cdna_predictor import OracleCdna, LSTM_SIZES, expected_shapes as _cdna_shapes

def NF_OF(cfg):
    """Number of warps: the cdna path uses nine of its ten kernels too."""
    return cfg.num_masks - 1


def expected_shapes(cfg):
    """The helper's own reading of the flow table: the survey table with ``flow/w``, ``flow/b`` in place of ``cdna/w``,
    ``cdna/b`` (name -> shape; the order of the flat weight blob is checked against the library's count elsewhere)."""
    out = {}
    for name, shape in _cdna_shapes(cfg).items():
        if name == 'cdna/w':
            out['flow/w'] = (1, 1, 32, 2 * NF_OF(cfg))
        elif name == 'cdna/b':
            out['flow/b'] = (2 * NF_OF(cfg),)
        else:
            out[name] = shape
    return out


def _fma(x, y, z):
    """fmaf(x, y, z) for float32 tensors (exact product in float64, one sum, one rounding); plain for float64."""
    if x.dtype == torch.float64:
        return x * y + z
    return (x.double() * y.double() + z.double()).float()


def warp_bilinear(img, dx, dy):
    """img [B, C, H, W], dx / dy [B, H, W] in pixels -> img sampled at (x + dx, y + dy), clamped bilinear."""
    B, C, H, W = img.shape
    dt = img.dtype
    xs = torch.arange(W, dtype=dt).view(1, 1, W)
    ys = torch.arange(H, dtype=dt).view(1, H, 1)
    x = torch.clamp(xs + dx, 0, W - 1)
    y = torch.clamp(ys + dy, 0, H - 1)
    x0f, y0f = torch.floor(x), torch.floor(y)
    x0, y0 = x0f.long(), y0f.long()
    x1, y1 = torch.clamp(x0 + 1, max=W - 1), torch.clamp(y0 + 1, max=H - 1)
    fx, fy = (x - x0f).unsqueeze(1), (y - y0f).unsqueeze(1)
    flat = img.reshape(B, C, H * W)

    def tap(yy, xx):
        idx = (yy * W + xx).view(B, 1, H * W).expand(B, C, H * W)
        return flat.gather(2, idx).view(B, C, H, W)

    a, b, c, d = tap(y0, x0), tap(y0, x1), tap(y1, x0), tap(y1, x1)
    top, bot = _fma(fx, b - a, a), _fma(fx, d - c, c)
    return _fma(fy, bot - top, top)


def warp_bilinear_loops(img, dx, dy):
    """The same warp, one pixel at a time in NumPy scalars (what the vectorised form is checked against, bit for bit)."""
    img, dx, dy = (np.asarray(t) for t in (img, dx, dy))
    B, C, H, W = img.shape
    f = img.dtype.type
    out = np.zeros_like(img)

    def fma(x, y, z):
        if img.dtype == np.float64:
            return x * y + z
        return np.float32(np.float64(x) * np.float64(y) + np.float64(z))

    for b in range(B):
        for r in range(H):
            for col in range(W):
                x = min(max(f(col) + dx[b, r, col], f(0)), f(W - 1))
                y = min(max(f(r) + dy[b, r, col], f(0)), f(H - 1))
                x0, y0 = int(np.floor(x)), int(np.floor(y))
                x1, y1 = min(x0 + 1, W - 1), min(y0 + 1, H - 1)
                fx, fy = f(x - f(x0)), f(y - f(y0))
                for ch in range(C):
                    p, q = img[b, ch, y0, x0], img[b, ch, y0, x1]
                    s, t = img[b, ch, y1, x0], img[b, ch, y1, x1]
                    top, bot = fma(fx, f(q - p), p), fma(fx, f(t - s), s)
                    out[b, ch, r, col] = fma(fy, f(bot - top), top)
    return out


class OracleAppflow(OracleCdna):
    expected_shapes = staticmethod(expected_shapes)

    def step(self, frame, distrib, state_vec, action, lstm_states):
        """frame [B,3,H,W], distrib [B,nd,H,W], state_vec [B,sdim], action [B,adim]."""
        cfg, L = self.cfg, LSTM_SIZES
        B = frame.shape[0]
        NF = NF_OF(cfg)
        new_states = [None] * 7

        enc0 = F.relu(self._ln(self._conv(frame, 'enc0', 2), 'ln1'))
        h1, new_states[0] = self._lstm(enc0, lstm_states[0], 'lstm1', L[0]); h1 = self._ln(h1, 'ln2')
        h2, new_states[1] = self._lstm(h1, lstm_states[1], 'lstm2', L[1]);   h2 = self._ln(h2, 'ln3')
        enc1 = F.relu(self._conv(h2, 'enc1', 2))
        h3, new_states[2] = self._lstm(enc1, lstm_states[2], 'lstm3', L[2]); h3 = self._ln(h3, 'ln4')
        h4, new_states[3] = self._lstm(h3, lstm_states[3], 'lstm4', L[3]);   h4 = self._ln(h4, 'ln5')
        enc2 = F.relu(self._conv(h4, 'enc2', 2))
        sa = torch.cat([action, state_vec], dim=1)
        smear = sa.view(B, -1, 1, 1).expand(B, sa.shape[1], enc2.shape[2], enc2.shape[3])
        enc3 = F.relu(self._conv(torch.cat([enc2, smear], dim=1), 'enc3'))
        h5, new_states[4] = self._lstm(enc3, lstm_states[4], 'lstm5', L[4]); h5 = self._ln(h5, 'ln6')
        enc4 = F.relu(self._convt(h5, 'convt1'))
        h6, new_states[5] = self._lstm(enc4, lstm_states[5], 'lstm6', L[5]); h6 = self._ln(h6, 'ln7')
        enc5 = F.relu(self._convt(torch.cat([h6, enc1], dim=1), 'convt2'))
        h7, new_states[6] = self._lstm(enc5, lstm_states[6], 'lstm7', L[6]); h7 = self._ln(h7, 'ln8')
        enc6 = F.relu(self._ln(self._convt(torch.cat([h7, enc0], dim=1), 'convt3'), 'ln9'))

        scratch = torch.sigmoid(self._conv(enc6, 'rgb'))
        masks = torch.softmax(self._conv(enc6, 'masks'), dim=1)              # [B, K+1, H, W]
        flow = self._conv(enc6, 'flow')                                      # [B, 2*NF, H, W]

        next_frame = masks[:, 0:1] * frame + masks[:, 1:2] * scratch
        next_distrib = masks[:, 0:1] * distrib
        for k in range(NF):
            dx, dy = flow[:, 2 * k], flow[:, 2 * k + 1]
            next_frame = next_frame + masks[:, k + 2:k + 3] * warp_bilinear(frame, dx, dy)
            next_distrib = next_distrib + masks[:, k + 2:k + 3] * warp_bilinear(distrib, dx, dy)
        next_distrib = next_distrib / next_distrib.sum(dim=(2, 3), keepdim=True)

        next_state = sa @ self.p['state/w'] + self.p['state/b']
        return next_frame, next_distrib, next_state, new_states


def make_appflow_predictor_class(weights_factory, dtype=torch.float32):
    """VPredEvaluation duck-type around ``OracleAppflow`` (one view), as ``tests/helpers/oracle_predictor.py`` builds one
    around ``OracleCdna``: the controller's host cost path scores its predictions."""
    from visual_foresight_amd.video_prediction.cdna_arch import CdnaConfig

    class OracleAppflowEvaluation(object):
        wants_agent_params = True
        n_context_default = 2

        def __init__(self, model_path, hparams, n_gpus=1, first_gpu=0):
            hp = dict(hparams)
            self.n_context = 2
            self.sequence_length = hp['sequence_length']
            self.cfg = CdnaConfig(height=hp['image_height'], width=hp['image_width'], adim=hp['adim'], sdim=hp['sdim'],
                                  ndesig=hp['designated_pixel_count'], sequence_length=hp['sequence_length'],
                                  transformation='flow')
            self.n_cam = 1

        def restore(self):
            self.weights = weights_factory(self.cfg)
            self.oracle = OracleAppflow(self.weights, dtype)

        def __call__(self, context, inputs):
            f, d, _ = self.oracle.rollout(np.asarray(context['context_frames'])[:, :1], context['context_actions'],
                                          np.asarray(context['context_pixel_distributions'])[:, :1],
                                          context['context_states'], np.asarray(inputs['actions']))
            return {'predicted_frames': f.astype(np.float32), 'predicted_pixel_distributions': d.astype(np.float32)}

    return OracleAppflowEvaluation
