"""Architecture table of the STP predictor (``vf_config`` arch 0, layer_spec 4, num_masks 10; manifest tag ``'stp'``).

STP - spatial transformer predictors (Finn, Goodfellow & Levine 2016, arXiv:1605.07157 section 3.3) - is the last of the
transformations the reference's legacy predictor configurations name beside their ``'model'`` key ("CDNA, DNA, or STP").
A head on the bottleneck predicts ``NF = num_masks - 1 = 9`` affine transforms per SAMPLE; each warps the whole previous
frame by bilinear sampling, and the masks mix the warps.  It is the only one of the three that can express rotation and
zoom.  Like every network here the model is external to the reference, so the table below is THIS project's
specification, parity unpinned.

Everything up to and including ``enc6`` is the ``'survey'`` table of ``cdna_arch.py``; ``K = 10``; the mask and scratch
heads are those of the appearance-flow table::

    scratch = sigmoid(conv1x1(enc6, ->3));  masks = softmax_c(conv1x1(enc6, ->K+1))
    hid     = relu(FC(flatten(LN6(h5)), ->100))              stp_fc/w [fc_in, 100], stp_fc/b [100]   (where cdna/w, cdna/b sit)
    theta_k = FC(hid, ->6 NF)[6k .. 6k+5] + (1,0,0, 0,1,0)   stp/w [100, 6*NF], stp/b [6*NF]
    sx = (W-1)/2, sy = (H-1)/2, cx = x - sx, cy = y - sy     (align-corners normalised coordinates, stated in pixels)
    xs = sx + t0*cx + t1*(sx/sy)*cy + t2*sx ;  ys = sy + t3*(sy/sx)*cx + t4*cy + t5*sy
    warp_k(img)[y, x] = bilinear_clamped(img, xs, ys)        the gather of the flow path, clamping included
    frame'  = masks_0*frame + masks_1*scratch + sum_{k<NF} masks_{k+2} * warp_k(frame)
    distr'  = normalise_hw(masks_0*distr + sum_{k<NF} masks_{k+2} * warp_k(distr))
    state'  = FC(concat[action, state])

Tensor order: the survey table through ``masks``, then ``stp_fc``, ``stp``, ``state``.

Arithmetic order (normative for ``csrc/vf_small_kernels.h`` - ``stp_finalize_sample``, ``composite_values_stp`` - and
``tests/helpers/oracle_stp.py``):

* ``hid_j = max(sum_j, 0)``, ``sum_j`` the first FC's output with its bias (its summation order is the engine's K-split
  GEMM and is NOT normative: the helper uses a plain matrix product).
* second FC: ``acc = stp/b_o``, then ``acc = fma(hid_j, stp/w[j, o], acc)`` for ``j = 0 .. 99`` ascending - one chain;
  ``t_e = acc + (1 if e in (0, 4) else 0)`` with ``e = o mod 6``.
* the row in pixel units, each entry rounded once: ``a0 = t0``, ``a1 = t1 * (sx / sy)``, ``a2 = fma(t2, sx, sx)``,
  ``b0 = t3 * (sy / sx)``, ``b1 = t4``, ``b2 = fma(t5, sy, sy)`` (``sx / sy`` and ``sy / sx`` one division each).
* ``xs = fma(a0, cx, fma(a1, cy, a2))``, ``ys = fma(b0, cx, fma(b1, cy, b2))`` with ``cx = x - sx``, ``cy = y - sy`` (exact).

Two properties of that order, used by the closed-form tests: with ``theta`` exactly the identity ``a1 = 0``, ``a2 = sx`` and
``xs = cx + sx = x`` bit for bit (likewise ``ys = y``); with ``theta = (-1,0,0, 0,-1,0)`` ``xs = sx - cx = W-1-x`` and
``ys = H-1-y`` bit for bit - sums and differences of half-integers below ``2^23`` are exact.

The clamp (``min(max(., 0), W-1)``), the taps (``top = fma(fx, b - a, a)``, ``bot = fma(fx, d - c, c)``,
``fma(fy, bot - top, top)``), the accumulation order of a pixel (previous frame, scratch, then the warps with ``k``
ascending) and the ``1 / mass`` scale of a fed-back distribution applied to each tap before the interpolation are the
appearance-flow path's (``cdna_arch.py``).  Exact fp32 only (``precision`` 1 and 2 are refused), arch 0 only, ``'survey'``
decoder only.
"""
from collections import OrderedDict

from visual_foresight_amd.video_prediction.cdna_arch import CdnaConfig
from visual_foresight_amd.video_prediction import cdna_arch as _cdna

STP_HIDDEN = 100
STP_PARAMS = 6


class StpConfig(CdnaConfig):
    """Static shape of one STP predictor instance.  ``transformation``, ``num_masks`` and the decoder are fixed."""

    arch = 'stp'            # manifest tag: an stp checkpoint is refused for a cdna / flow / dna config and the reverse
    arch_id = 0             # vf_config.arch: the CDNA engine, selected by layer_spec 4

    def __init__(self, height=64, width=64, adim=4, sdim=5, ndesig=1, n_context=2, sequence_length=15, num_masks=10,
                 ncam=1, decoder='survey', transformation='stp'):
        if transformation != 'stp':
            raise ValueError("StpConfig is the table of transformation 'stp', got %r" % (transformation,))
        if decoder != 'survey':
            raise ValueError("transformation='stp' is built for the 'survey' decoder only, not %r" % (decoder,))
        if int(num_masks) != 10:
            raise ValueError("transformation='stp' has nine transforms: num_masks = 10, got %r" % (num_masks,))
        super(StpConfig, self).__init__(height, width, adim, sdim, ndesig, n_context, sequence_length, 10, ncam)
        self.transformation = 'stp'

    @property
    def layer_spec(self):
        """``vf_config.layer_spec`` of this table."""
        return 4

    @property
    def num_warps(self):
        return self.num_masks - 1

    def as_dict(self):
        return dict(height=self.height, width=self.width, adim=self.adim, sdim=self.sdim, ndesig=self.ndesig,
                    n_context=self.n_context, sequence_length=self.sequence_length, num_masks=self.num_masks)

    def tensor_shapes(self):
        """Ordered name -> shape table: the survey table through ``masks``, then ``stp_fc``, ``stp``, ``state``."""
        t = OrderedDict()
        for name, shape in _cdna.tensor_shapes(self).items():
            if name == 'cdna/w':
                t['stp_fc/w'] = (shape[0], STP_HIDDEN)
                t['stp_fc/b'] = (STP_HIDDEN,)
                t['stp/w'] = (STP_HIDDEN, STP_PARAMS * self.num_warps)
                t['stp/b'] = (STP_PARAMS * self.num_warps,)
            elif name != 'cdna/b':
                t[name] = shape
        return t

    def macs_per_sample_step(self):
        """As ``cdna_arch.macs_per_sample_step``: the two FC layers of the head in place of ``cdna_fc``, four bilinear taps
        per warp and channel in place of the 5 x 5 warps."""
        H, W, NF = self.height, self.width, self.num_warps
        shp = self.tensor_shapes()
        out = OrderedDict()
        for name, n in _cdna.macs_per_sample_step(self).items():
            if name in ('cdna_fc', 'warp_frame', 'warp_distrib', 'state_fc'):
                continue
            out[name] = n
        out['stp_fc'] = shp['stp_fc/w'][0] * shp['stp_fc/w'][1]
        out['stp'] = shp['stp/w'][0] * shp['stp/w'][1]
        out['warp_frame'] = H * W * 4 * 3 * NF
        out['warp_distrib'] = H * W * 4 * self.ndesig * NF
        out['state_fc'] = (self.adim + self.sdim) * self.sdim
        return out
