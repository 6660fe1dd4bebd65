"""Architecture table of the DNA predictor (``vf_config`` arch 0, layer_spec 3, num_masks 1; manifest tag ``'dna'``).

DNA - dynamic neural advection (Finn, Goodfellow & Levine 2016, arXiv:1605.07157 section 3.1) - is the third of the
transformations the reference's legacy predictor configurations name beside their ``'model'`` key ("CDNA, DNA, or STP").
A 1x1 head predicts a separate normalised 5x5 kernel for every PIXEL, where CDNA shares nine kernels per sample and mixes
them by masks.  Like every network here the model is external to the reference, so the table below is THIS project's
specification, parity unpinned; it follows the DNA branch of the public ``prediction_model.py``: one DNA transform,
``num_masks = 1``, two mask channels, no scratch image.

Everything up to and including ``enc6`` is the ``'survey'`` table of ``cdna_arch.py``::

    masks = softmax_c(conv1x1(enc6, ->2))                              masks/w [1,1,32,2], masks/b [2]
    a     = conv1x1(enc6, ->25)                                        dna/w   [1,1,32,25], dna/b [25]; channel t = 5*dy + dx
    v_t   = relu(a_t - 1e-12) + 1e-12;   k_t = v_t / sum_t v_t         per pixel
    dna(img)[y, x] = sum_t k_t[y, x] * img[y + dy - 2, x + dx - 2]     zero outside the image
    frame'  = masks_0 * frame + masks_1 * dna(frame)
    distr'  = normalise_hw(masks_0 * distr + masks_1 * dna(distr))
    state'  = FC(concat[action, state])

There is no ``rgb`` head, no ``cdna/w`` and no ``cdna/b``.  Tensor order: the survey table through ``ln9``, then ``masks``,
``dna``, ``state``.

Arithmetic order of one pixel (normative for ``csrc/vf_small_kernels.h`` and ``tests/helpers/oracle_dna.py``): every head sum
is one fma chain over the 32 channels ascending from its bias on ``f_c = relu(LN9(enc6)_c)``; the two-way softmax is max,
``exp``, ``1 / den``; ``s`` is 25 plain additions with ``t`` ascending from 0, ``g = masks_1 / s`` one division,
``ke_t = g * v_t``; ``of_c = masks_0 * prev_c(y, x)``, then ``of_c = fma(ke_t, prev_c(tap t), of_c)`` with ``t`` ascending;
the distributions likewise, the ``1 / mass`` scale of a fed-back distribution applied to each tap.  Exact fp32 only
(``precision`` 1 and 2 are refused), ``'survey'`` decoder only.
"""
from collections import OrderedDict

from visual_foresight_amd.video_prediction.cdna_arch import CdnaConfig, DNA_KERN
from visual_foresight_amd.video_prediction import cdna_arch as _cdna

DNA_TAPS = DNA_KERN * DNA_KERN


class DnaConfig(CdnaConfig):
    """Static shape of one DNA predictor instance.  ``transformation``, ``num_masks`` and the decoder are fixed."""

    arch = 'dna'            # manifest tag: a dna checkpoint is refused for a cdna / flow config and the reverse
    arch_id = 0             # vf_config.arch: the CDNA engine, selected by layer_spec 3

    def __init__(self, height=64, width=64, adim=4, sdim=5, ndesig=1, n_context=2, sequence_length=15, num_masks=1,
                 ncam=1, decoder='survey', transformation='dna'):
        if transformation != 'dna':
            raise ValueError("DnaConfig is the table of transformation 'dna', got %r" % (transformation,))
        if decoder != 'survey':
            raise ValueError("transformation='dna' is built for the 'survey' decoder only, not %r" % (decoder,))
        if int(num_masks) != 1:
            raise ValueError("transformation='dna' has one transform: num_masks = 1, got %r" % (num_masks,))
        super(DnaConfig, self).__init__(height, width, adim, sdim, ndesig, n_context, sequence_length, 1, ncam)
        self.transformation = 'dna'

    @property
    def layer_spec(self):
        """``vf_config.layer_spec`` of this table."""
        return 3

    def as_dict(self):
        return dict(height=self.height, width=self.width, adim=self.adim, sdim=self.sdim, ndesig=self.ndesig,
                    n_context=self.n_context, sequence_length=self.sequence_length, num_masks=self.num_masks)

    def tensor_shapes(self):
        """Ordered name -> shape table: the survey table through ``ln9``, then ``masks``, ``dna``, ``state``."""
        t = OrderedDict()
        for name, shape in _cdna.tensor_shapes(self).items():      # (num_masks = 1: masks/w [1, 1, 32, 2])
            head = name.split('/')[0]
            if head == 'rgb':
                continue
            if head == 'cdna':
                name, shape = 'dna/' + name.split('/')[1], ((1, 1, 32, DNA_TAPS) if name.endswith('/w') else (DNA_TAPS,))
            t[name] = shape
        return t

    def macs_per_sample_step(self):
        """As ``cdna_arch.macs_per_sample_step``: no ``cdna_fc`` and no ``rgb``; the DNA head and one 5x5 kernel per pixel."""
        H, W = self.height, self.width
        out = OrderedDict()
        for name, n in _cdna.macs_per_sample_step(self).items():
            if name in ('rgb', 'cdna_fc', 'warp_frame', 'warp_distrib', 'state_fc'):
                continue
            out[name] = n
        out['dna'] = H * W * 32 * DNA_TAPS
        out['warp_frame'] = H * W * DNA_TAPS * 3
        out['warp_distrib'] = H * W * DNA_TAPS * self.ndesig
        out['state_fc'] = (self.adim + self.sdim) * self.sdim
        return out
