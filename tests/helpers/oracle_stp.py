"""CPU restatement of the STP predictor (test infrastructure only).

PARITY UNPINNED, like ``oracle/cdna_predictor.py``: the reference names the model ("CDNA, DNA, or STP" beside the ``'model'``
key of its legacy predictor configurations) but holds no network code, so ``stp_arch.py`` (``StpConfig``) is the
specification and this file restates it in plain PyTorch CPU ops.  Everything up to ``enc6`` is ``OracleCdna``'s own layers,
the mask and scratch heads are the appearance-flow helper's; the transformation is restated here::

    hid     = relu(FC(flatten(LN6(h5)), ->100))                          NHWC flatten, as the CDNA FC
    theta_k = FC(hid, ->6 NF)[6k .. 6k+5] + (1,0,0, 0,1,0)
    sx = (W-1)/2, sy = (H-1)/2, cx = x - sx, cy = y - sy
    xs = sx + t0*cx + t1*(sx/sy)*cy + t2*sx ;  ys = sy + t3*(sy/sx)*cx + t4*cy + t5*sy
    warp_k(img)[y, x] = bilinear_clamped(img, xs, ys)
    frame'  = masks_0*frame + masks_1*scratch + sum_k masks_{k+2} * warp_k(frame)
    distr'  = normalise_hw(masks_0*distr + sum_k masks_{k+2} * warp_k(distr))

in the arithmetic order ``stp_arch.py`` lays down: the second FC one fma chain over the 100 hidden units ascending from the
bias, then the identity; the row in pixel units ``a0 = t0, a1 = t1 * (sx / sy), a2 = fma(t2, sx, sx), b0 = t3 * (sy / sx),
b1 = t4, b2 = fma(t5, sy, sy)``; ``xs = fma(a0, cx, fma(a1, cy, a2))``, ``ys = fma(b0, cx, fma(b1, cy, b2))``; clamp and taps
as ``oracle_appflow.warp_bilinear``.  The first FC is a plain matrix product (its order is not normative).  In float32 the
fused multiply-adds are emulated as ``oracle_appflow.py`` emulates them: the product of two float32 values is exact in
float64, one float64 addition, one rounding to float32.  In float64 (used to measure rounding) they are plain arithmetic.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.cdna_predictor import OracleCdna, LSTM_SIZES
from oracle.cdna_predictor import expected_shapes as _cdna_shapes

HIDDEN = 100
PARAMS = 6


def NF_OF(cfg):
    """Number of warps: the cdna path uses nine of its ten kernels too."""
    return cfg.num_masks - 1


def expected_shapes(cfg):
    """The helper's own reading of the STP table: the survey table with the two FC layers of the head in place of
    ``cdna/w``, ``cdna/b`` (name -> shape)."""
    out = {}
    for name, shape in _cdna_shapes(cfg).items():
        if name == 'cdna/w':
            out['stp_fc/w'] = (shape[0], HIDDEN)
            out['stp_fc/b'] = (HIDDEN,)
            out['stp/w'] = (HIDDEN, PARAMS * NF_OF(cfg))
            out['stp/b'] = (PARAMS * NF_OF(cfg),)
        elif name != 'cdna/b':
            out[name] = shape
    return out


def _fma(x, y, z):
    """fmaf(x, y, z) for float32 tensors (exact product in float64, one sum, one rounding); plain for float64."""
    if x.dtype == torch.float64:
        return x * y + z
    return (x.double() * y.double() + z.double()).float()


def theta_of(hid, w2, b2):
    """hid [B, 100], w2 [100, 6 NF], b2 [6 NF] -> theta [B, NF, 6]: one fma chain over the hidden units ascending from the
    bias, then the identity (1, 0, 0, 0, 1, 0)."""
    B = hid.shape[0]
    acc = b2.view(1, -1).expand(B, -1).contiguous()
    for j in range(hid.shape[1]):
        acc = _fma(hid[:, j:j + 1], w2[j:j + 1], acc)
    ident = torch.tensor([1, 0, 0, 0, 1, 0], dtype=hid.dtype).repeat(acc.shape[1] // PARAMS)
    return (acc + ident).view(B, -1, PARAMS)


def pixel_rows(theta, H, W):
    """theta [..., 6] -> the rows in pixel units [..., 6]: (a0, a1, a2, b0, b1, b2)."""
    dt = theta.dtype
    sx = torch.tensor((W - 1) / 2.0, dtype=dt)
    sy = torch.tensor((H - 1) / 2.0, dtype=dt)
    t = theta.unbind(-1)
    return torch.stack([t[0], t[1] * (sx / sy), _fma(t[2], sx, sx), t[3] * (sy / sx), t[4], _fma(t[5], sy, sy)], dim=-1)


def sample_coords(rows, H, W):
    """rows [B, 6] in pixel units -> (xs, ys) [B, H, W]: ``xs = fma(a0, cx, fma(a1, cy, a2))``, ``ys`` likewise."""
    dt = rows.dtype
    cx = (torch.arange(W, dtype=dt) - torch.tensor((W - 1) / 2.0, dtype=dt)).view(1, 1, W)
    cy = (torch.arange(H, dtype=dt) - torch.tensor((H - 1) / 2.0, dtype=dt)).view(1, H, 1)
    r = [rows[:, i].view(-1, 1, 1) for i in range(PARAMS)]
    cxe, cye = cx.expand(rows.shape[0], H, W), cy.expand(rows.shape[0], H, W)
    xs = _fma(r[0], cxe, _fma(r[1], cye, r[2].expand(-1, H, W)))
    ys = _fma(r[3], cxe, _fma(r[4], cye, r[5].expand(-1, H, W)))
    return xs, ys


def gather_bilinear(img, xs, ys):
    """img [B, C, H, W], xs / ys [B, H, W] absolute sample positions in pixels -> clamped bilinear samples (the clamp, taps
    and fma order of ``oracle_appflow.warp_bilinear``)."""
    B, C, H, W = img.shape
    x = torch.clamp(xs, 0, W - 1)
    y = torch.clamp(ys, 0, H - 1)
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


def warp_affine(img, theta):
    """img [B, C, H, W], theta [B, 6] (normalised, identity included) -> the affine warp of the specification."""
    H, W = img.shape[-2:]
    xs, ys = sample_coords(pixel_rows(theta, H, W), H, W)
    return gather_bilinear(img, xs, ys)


def warp_affine_loops(img, theta):
    """The same warp, one pixel at a time in NumPy scalars (what the vectorised form is checked against, bit for bit)."""
    img, theta = np.asarray(img), np.asarray(theta)
    B, C, H, W = img.shape
    f = img.dtype.type
    out = np.zeros_like(img)

    def fma(x, y, z):
        if img.dtype == np.float64:
            return x * y + z
        return np.float32(np.float64(x) * np.float64(y) + np.float64(z))

    sx, sy = f((W - 1) / 2.0), f((H - 1) / 2.0)
    for b in range(B):
        t = [f(v) for v in theta[b]]
        a0, a1, a2 = t[0], f(t[1] * f(sx / sy)), fma(t[2], sx, sx)
        b0, b1, b2 = f(t[3] * f(sy / sx)), t[4], fma(t[5], sy, sy)
        for r in range(H):
            for col in range(W):
                cx, cy = f(f(col) - sx), f(f(r) - sy)
                x = min(max(fma(a0, cx, fma(a1, cy, a2)), f(0)), f(W - 1))
                y = min(max(fma(b0, cx, fma(b1, cy, b2)), f(0)), f(H - 1))
                x0, y0 = int(np.floor(x)), int(np.floor(y))
                x1, y1 = min(x0 + 1, W - 1), min(y0 + 1, H - 1)
                fx, fy = f(x - f(x0)), f(y - f(y0))
                for ch in range(C):
                    p, q = img[b, ch, y0, x0], img[b, ch, y0, x1]
                    s, u = img[b, ch, y1, x0], img[b, ch, y1, x1]
                    top, bot = fma(fx, f(q - p), p), fma(fx, f(u - s), s)
                    out[b, ch, r, col] = fma(fy, f(bot - top), top)
    return out


class OracleStp(OracleCdna):
    expected_shapes = staticmethod(expected_shapes)

    def step(self, frame, distrib, state_vec, action, lstm_states):
        """frame [B,3,H,W], distrib [B,nd,H,W], state_vec [B,sdim], action [B,adim]."""
        cfg, L = self.cfg, LSTM_SIZES
        B = frame.shape[0]
        NF = NF_OF(cfg)
        H, W = frame.shape[-2:]
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

        # per-sample transforms from the NHWC-flattened bottleneck
        flat = h5.permute(0, 2, 3, 1).reshape(B, -1)
        hid = F.relu(flat @ self.p['stp_fc/w'] + self.p['stp_fc/b'])
        theta = theta_of(hid, self.p['stp/w'], self.p['stp/b'])               # [B, NF, 6]
        rows = pixel_rows(theta, H, W)
        self.last_theta = theta         # (what the tests' weight scale is judged by)

        next_frame = masks[:, 0:1] * frame + masks[:, 1:2] * scratch
        next_distrib = masks[:, 0:1] * distrib
        for k in range(NF):
            xs, ys = sample_coords(rows[:, k], H, W)
            next_frame = next_frame + masks[:, k + 2:k + 3] * gather_bilinear(frame, xs, ys)
            next_distrib = next_distrib + masks[:, k + 2:k + 3] * gather_bilinear(distrib, xs, ys)
        next_distrib = next_distrib / next_distrib.sum(dim=(2, 3), keepdim=True)

        next_state = sa @ self.p['state/w'] + self.p['state/b']
        return next_frame, next_distrib, next_state, new_states


def make_stp_predictor_class(weights_factory, dtype=torch.float32):
    """VPredEvaluation duck-type around ``OracleStp`` (one view), as ``tests/helpers/oracle_predictor.py`` builds one around
    ``OracleCdna``: the controller's host cost path scores its predictions."""
    from visual_foresight_amd.video_prediction.stp_arch import StpConfig

    class OracleStpEvaluation(object):
        wants_agent_params = True
        n_context_default = 2

        def __init__(self, model_path, hparams, n_gpus=1, first_gpu=0):
            hp = dict(hparams)
            self.n_context = 2
            self.sequence_length = hp['sequence_length']
            self.cfg = StpConfig(height=hp['image_height'], width=hp['image_width'], adim=hp['adim'], sdim=hp['sdim'],
                                 ndesig=hp['designated_pixel_count'], sequence_length=hp['sequence_length'])
            self.n_cam = 1

        def restore(self):
            self.weights = weights_factory(self.cfg)
            self.oracle = OracleStp(self.weights, dtype)

        def __call__(self, context, inputs):
            f, d, _ = self.oracle.rollout(np.asarray(context['context_frames'])[:, :1], context['context_actions'],
                                          np.asarray(context['context_pixel_distributions'])[:, :1],
                                          context['context_states'], np.asarray(inputs['actions']))
            return {'predicted_frames': f.astype(np.float32), 'predicted_pixel_distributions': d.astype(np.float32)}

    return OracleStpEvaluation
