"""Rounding twin of the oracles for the plain-bf16 precision mode (``vf_config.precision = 2``).

The mode rounds the two operands of every conv-LSTM gate convolution - the concatenated input ``[x | h]`` and the gate
weights - ONCE, to nearest even, to bfloat16; products are exact and accumulation, bias, gate math and everything else stay
in the oracle's own precision.  Both ``OracleCdna`` and ``OracleSavp`` reach the gate convolution through ``_lstm``, so one
mixin that overrides ``_lstm`` serves both.  In float64 the operands go float64 -> float32 -> bfloat16, as on the device
(whose activations are float32 before they are rounded).
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.cdna_predictor import OracleCdna, _same_pad
from oracle.savp_predictor import OracleSavp


def rne_bits(x):
    """float32 array -> float32 array rounded to bfloat16 (nearest, ties to even) on the integer bits."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def round_bf16(t):
    """Tensor of any float dtype -> same dtype, values rounded through float32 -> bfloat16 (torch's conversion)."""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def lstm_layer(x, h, c, w, b, dtype=torch.float64, rounded=True):
    """One conv-LSTM layer in closed form: x [B,Cx,H,W], h / c [B,C,H,W], w [5,5,Cx+C,4C] (HWIO, input order [x | h]), b [4C]
    -> (h', c') as arrays of ``dtype``; ``rounded``: operands of the convolution through bfloat16."""
    tx, th, tc, tw, tb = (torch.from_numpy(np.asarray(a)).to(dtype) for a in (x, h, c, w, b))
    inp = torch.cat([tx, th], dim=1)
    if rounded:
        inp, tw = round_bf16(inp), round_bf16(tw)
    gates = F.conv2d(_same_pad(inp, tw.shape[0], 1), tw.permute(3, 2, 0, 1).contiguous(), tb)
    i, j, f, o = torch.split(gates, tc.shape[1], dim=1)
    c_new = tc * torch.sigmoid(f + 1.0) + torch.sigmoid(i) * torch.tanh(j)
    h_new = torch.tanh(c_new) * torch.sigmoid(o)
    return h_new.numpy(), c_new.numpy()


class Bf16GateMixin(object):
    def _lstm(self, x, state, name, C):
        c, h = state
        inp = round_bf16(torch.cat([x, h], dim=1))
        w = round_bf16(self.p[name + '/w']).permute(3, 2, 0, 1).contiguous()       # HWIO -> OIHW
        gates = F.conv2d(_same_pad(inp, w.shape[-1], 1), w, self.p[name + '/b'])
        i, j, f, o = torch.split(gates, C, dim=1)
        c_new = c * torch.sigmoid(f + 1.0) + torch.sigmoid(i) * torch.tanh(j)
        h_new = torch.tanh(c_new) * torch.sigmoid(o)
        return h_new, (c_new, h_new)


class OracleCdnaBf16(Bf16GateMixin, OracleCdna):
    pass


class OracleSavpBf16(Bf16GateMixin, OracleSavp):
    pass
