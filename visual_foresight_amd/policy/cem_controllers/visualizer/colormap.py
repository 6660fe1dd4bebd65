"""Colouring of plan visualisations on the host: the normative restatement of ``vf_render_plans`` (include/vf_hip.h).

The reference renders every designated-pixel distribution of the ten best plans with
``(plt.cm.viridis(dist / (np.amax(dist) + 1e-6))[..., :3] * 255).astype(np.uint8)`` and every predicted frame with
``(gen_images * 255).astype(np.uint8)`` (``visual_mpc/policy/cem_controllers/pixel_cost_controller.py:107-126``).  Under
NumPy >= 2 scalar promotion all of it is float32 arithmetic on float32 inputs:

    mx = max over the plane;  q = dist / (mx + 1e-6)         (float32 add, float32 division)
    index = min(int(q * 256), 255)                             (matplotlib: ``xa *= N``, ``xa[xa == N] = N - 1``, truncation)
    pixel = VIRIDIS_U8[index]                                  (``(viridis.colors * 255).astype(uint8)``)

``VIRIDIS_U8`` is matplotlib's viridis table (CC0) as bytes, so that neither the device path nor this one needs matplotlib.
These functions serve predictors without ``render_plans`` and are what the device kernel is tested against, bit for bit.
"""
import numpy as np

_VIRIDIS_HEX = (
    '44015444025544035745055845065a45085b46095c460b5e460c5f460e61470f62471163471265471466471567471669'
    '47186a48196b481a6c481c6e481d6f481e70482071482172482273482374472575472676472777472878472a79472b7a'
    '472c7b462d7c462f7c46307d46317e45327f45347f453580453681443781443982433a83433b83433c84423d84423e85'
    '4240854141864142864043874044873f45873f47883e48883e49893d4a893d4b893d4c893c4d8a3c4e8a3b508a3b518a'
    '3a528b3a538b39548b39558b38568b38578c37588c37598c365a8c365b8c355c8c355d8c345e8d345f8d33608d33618d'
    '32628d32638d31648d31658d31668d30678d30688d2f698d2f6a8d2e6b8e2e6c8e2e6d8e2d6e8e2d6f8e2c708e2c718e'
    '2c728e2b738e2b748e2a758e2a768e2a778e29788e29798e287a8e287a8e287b8e277c8e277d8e277e8e267f8e26808e'
    '26818e25828e25838d24848d24858d24868d23878d23888d23898d22898d228a8d228b8d218c8d218d8c218e8c208f8c'
    '20908c20918c1f928c1f938b1f948b1f958b1f968b1e978a1e988a1e998a1e998a1e9a891e9b891e9c891e9d881e9e88'
    '1e9f881ea0871fa1871fa2861fa38620a48520a58521a68521a78422a78423a88323a98224aa8225ab8126ac8127ad80'
    '28ae7f29af7f2ab07e2bb17d2cb17d2eb27c2fb37b30b47a32b57a33b67935b77836b87738b97639b9763bba753dbb74'
    '3ebc7340bd7242be7144be7045bf6f47c06e49c16d4bc26c4dc26b4fc36951c46853c56755c66657c66559c7645bc862'
    '5ec96160c96062ca5f64cb5d67cc5c69cc5b6bcd596dce5870ce5672cf5574d05477d05279d1517cd24f7ed24e81d34c'
    '83d34b86d44988d5478bd5468dd64490d64392d74195d73f97d83e9ad83c9dd93a9fd938a2da37a5da35a7db33aadb32'
    'addc30afdc2eb2dd2cb5dd2bb7dd29bade27bdde26bfdf24c2df22c5df21c7e01fcae01ecde01dcfe11cd2e11bd4e11a'
    'd7e219dae218dce218dfe318e1e318e4e318e7e419e9e419ece41aeee51bf1e51cf3e51ef6e61ff8e621fae622fde724'
)
VIRIDIS_U8 = np.frombuffer(bytes.fromhex(_VIRIDIS_HEX), np.uint8).reshape(256, 3).copy()
VIRIDIS_U8.setflags(write=False)


def check_lut(lut):
    """-> a contiguous uint8 ``[256, 3]`` colour table (None: viridis)."""
    if lut is None:
        return VIRIDIS_U8
    lut = np.ascontiguousarray(lut)
    if lut.dtype != np.uint8 or lut.shape != (256, 3):
        raise ValueError('a colour table is uint8 [256, 3], got %s %s' % (lut.dtype, lut.shape))
    return lut


def render_distribution_planes(planes, lut=None):
    """float32 ``[..., H, W]`` (each ``[H, W]`` plane is coloured against its own maximum) -> uint8 ``[..., H, W, 3]``."""
    lut = check_lut(lut)
    p = np.asarray(planes, dtype=np.float32)
    if p.ndim < 2:
        raise ValueError('need [..., H, W] planes, got shape %s' % (p.shape,))
    denom = p.max(axis=(-2, -1), keepdims=True) + np.float32(1e-6)
    q = p / denom
    index = np.clip((q * np.float32(256.)).astype(np.int64), 0, 255)
    return lut[index]


def render_frames(frames):
    """float32 frames in [0, 1], any shape -> uint8 by truncation of ``frame * 255`` (one float32 multiply)."""
    return (np.asarray(frames, dtype=np.float32) * np.float32(255.)).astype(np.uint8)


def render_prediction(frames=None, distributions=None, lut=None):
    """Predictions in the layout a predictor's ``__call__`` returns - frames ``[K, T, ncam, H, W, 3]``, normalised
    distributions ``[K, T, ncam, H, W, ndesig]`` - rendered into the layout of ``HipVPredEvaluation.render_plans``:
    ``{'frames': uint8 [K, ncam, T, H, W, 3], 'distributions': uint8 [K, ncam, ndesig, T, H, W, 3]}`` (one movie is
    contiguous).  A missing input gives no entry."""
    out = {}
    if frames is not None:
        out['frames'] = np.ascontiguousarray(np.transpose(render_frames(frames), (0, 2, 1, 3, 4, 5)))
    if distributions is not None:
        planes = np.transpose(np.asarray(distributions, dtype=np.float32), (0, 2, 5, 1, 3, 4))
        out['distributions'] = render_distribution_planes(planes, lut)
    return out
