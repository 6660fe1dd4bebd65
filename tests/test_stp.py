"""STP compositing (``StpConfig``, ``vf_config`` arch 0 / layer_spec 4 / num_masks 10) without a GPU: the helper oracle's warp
against naive loops, the table in Python against the table behind the C ABI, the refusals, and the persistent schedule of an
stp engine in the host self-test."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers import oracle_stp
from visual_foresight_amd import _lib
from visual_foresight_amd.video_prediction.cdna_arch import CdnaConfig, CdnaWeights
from visual_foresight_amd.video_prediction.dna_arch import DnaConfig
from visual_foresight_amd.video_prediction.stp_arch import StpConfig


def _c_cfg(cfg, precision=0, arch=0, layer_spec=None, num_masks=None, max_batch=4, ndesig=None):
    return _lib.VfConfig(cfg.height, cfg.width, cfg.adim, cfg.sdim, cfg.ndesig if ndesig is None else ndesig, cfg.n_context,
                         cfg.sequence_length, cfg.num_masks if num_masks is None else num_masks, max_batch, 0, precision, 1,
                         1, arch, 0, cfg.layer_spec if layer_spec is None else layer_spec)


def _thetas(rs, dtype):
    """Seven transforms: identity, flip, a rotation with zoom, zoom 0.5, zoom 2, a shear with a translation that samples
    off-image, a random one."""
    c, s = np.cos(0.4), np.sin(0.4)
    t = np.array([[1, 0, 0, 0, 1, 0], [-1, 0, 0, 0, -1, 0], [1.2 * c, -1.2 * s, 0.1, 1.2 * s, 1.2 * c, -0.2],
                  [0.5, 0, 0, 0, 0.5, 0], [2, 0, 0, 0, 2, 0], [1, 0.4, 0.6, -0.3, 1, -0.7],
                  list(rs.normal(0, 0.7, 6))], np.float64)
    return torch.from_numpy(t).to(dtype)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_vectorised_warp_equals_naive_loops_bit_for_bit(dtype):
    """8 x 12 (non-square: ``sx / sy`` is on the path), two channels, seven transforms; identity and flip are exact."""
    rs = np.random.RandomState(4)
    theta = _thetas(rs, dtype)
    B, C, H, W = theta.shape[0], 2, 8, 12
    img = torch.from_numpy(rs.uniform(0, 1, (B, C, H, W))).to(dtype)
    got = oracle_stp.warp_affine(img, theta).numpy()
    want = oracle_stp.warp_affine_loops(img.numpy(), theta.numpy())
    assert got.dtype == want.dtype == img.numpy().dtype
    np.testing.assert_array_equal(got, want)
    # the two properties the arithmetic order keeps: the identity and the flip of both axes are exact
    np.testing.assert_array_equal(got[0], img.numpy()[0])
    np.testing.assert_array_equal(got[1], img.numpy()[1, :, ::-1, ::-1])
    xs, ys = oracle_stp.sample_coords(oracle_stp.pixel_rows(theta[:2], H, W), H, W)
    np.testing.assert_array_equal(xs[0].numpy(), np.broadcast_to(np.arange(W), (H, W)))
    np.testing.assert_array_equal(ys[0].numpy(), np.broadcast_to(np.arange(H)[:, None], (H, W)))
    np.testing.assert_array_equal(xs[1].numpy(), np.broadcast_to(W - 1 - np.arange(W), (H, W)))
    np.testing.assert_array_equal(ys[1].numpy(), np.broadcast_to(H - 1 - np.arange(H)[:, None], (H, W)))
    # some samples lie off-image (the clamp is on the path), and zoom 0.5 about the centre averages neighbours:
    # xs = sx + (x - sx) / 2 is a quarter or three quarters between two pixels in both axes
    xs5, ys5 = oracle_stp.sample_coords(oracle_stp.pixel_rows(theta[5:6], H, W), H, W)
    assert (xs5 < 0).any() or (xs5 > W - 1).any() or (ys5 < 0).any() or (ys5 > H - 1).any()
    i = img.numpy()[3].astype(np.float64)
    y, x = 2, 4                                     # ys = 3.5 + (2 - 3.5) / 2 = 2.75, xs = 5.5 + (4 - 5.5) / 2 = 4.75
    want_px = 0.25 * (0.25 * i[:, 2, 4] + 0.75 * i[:, 2, 5]) + 0.75 * (0.25 * i[:, 3, 4] + 0.75 * i[:, 3, 5])
    np.testing.assert_allclose(got[3][:, y, x], want_px, rtol=0, atol=1e-6)


def test_second_fc_chain_and_identity():
    """``theta_of``: one fma chain over the hidden units ascending from the bias, then the identity."""
    rs = np.random.RandomState(1)
    hid = torch.from_numpy(rs.uniform(0, 1, (3, 100)).astype(np.float32))
    w2 = torch.from_numpy(rs.normal(0, 0.1, (100, 54)).astype(np.float32))
    b2 = torch.from_numpy(rs.normal(0, 0.1, 54).astype(np.float32))
    got = oracle_stp.theta_of(hid, w2, b2).numpy()
    assert got.shape == (3, 9, 6)
    acc = np.tile(b2.numpy(), (3, 1))
    for j in range(100):
        acc = (hid.numpy()[:, j:j + 1].astype(np.float64) * w2.numpy()[j].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    np.testing.assert_array_equal(got.reshape(3, 54), acc + np.tile(np.float32([1, 0, 0, 0, 1, 0]), 9))
    zero = oracle_stp.theta_of(torch.zeros(2, 100), torch.zeros(100, 54), torch.zeros(54)).numpy()
    np.testing.assert_array_equal(zero, np.tile(np.float32([1, 0, 0, 0, 1, 0]), (2, 9, 1)))


def test_table_in_python():
    cfg = StpConfig(ndesig=2)
    cdna = CdnaConfig(ndesig=2)
    assert cfg.layer_spec == 4 and cfg.transformation == 'stp' and cfg.num_masks == 10 and cfg.arch_id == 0 and cfg.arch == 'stp'
    shp, ref = cfg.tensor_shapes(), cdna.tensor_shapes()
    assert not any(n.startswith(('cdna/', 'flow/', 'dna/')) for n in shp)
    assert shp['stp_fc/w'] == (8 * 8 * 128, 100) and shp['stp_fc/b'] == (100,)
    assert shp['stp/w'] == (100, 54) and shp['stp/b'] == (54,)
    # the survey table through masks, then stp_fc, stp, state
    names, ref_names = list(shp), list(ref)
    cut = ref_names.index('masks/b') + 1
    assert names[:cut] == ref_names[:cut] and all(shp[n] == ref[n] for n in names[:cut])
    assert names[cut:] == ['stp_fc/w', 'stp_fc/b', 'stp/w', 'stp/b', 'state/w', 'state/b']
    assert {k: tuple(v) for k, v in shp.items()} == oracle_stp.expected_shapes(cfg)
    macs, macs_ref = cfg.macs_per_sample_step(), cdna.macs_per_sample_step()
    assert 'cdna_fc' not in macs
    assert macs['stp_fc'] == 8192 * 100 and macs['stp'] == 100 * 54
    assert macs['warp_frame'] == 64 * 64 * 4 * 3 * 9 and macs['warp_distrib'] == 64 * 64 * 4 * 2 * 9
    same = [k for k in macs_ref if k not in ('cdna_fc', 'warp_frame', 'warp_distrib')]
    assert all(macs[k] == macs_ref[k] for k in same) and len(macs) == len(same) + 4
    # as_dict() of the other configs is what it was
    assert cdna.as_dict() == dict(height=64, width=64, adim=4, sdim=5, ndesig=2, n_context=2, sequence_length=15, num_masks=10)
    assert 'transformation' not in cfg.as_dict() and cfg.as_dict()['num_masks'] == 10
    # the oracle helper accepts this table's weights and refuses the cdna table's
    oracle_stp.OracleStp(CdnaWeights.random(StpConfig(height=16, width=16), seed=0))
    with pytest.raises(ValueError, match='layer table'):
        oracle_stp.OracleStp(CdnaWeights.random(CdnaConfig(height=16, width=16), seed=0))


@pytest.mark.parametrize('H,W,nd', [(32, 32, 1), (48, 64, 2), (64, 64, 4)])
def test_c_abi_table_equals_python_table(H, W, nd):
    cfg = StpConfig(height=H, width=W, ndesig=nd)
    lib = _lib.load_library()
    c = _c_cfg(cfg)
    assert c.arch == 0 and c.layer_spec == 4 and c.num_masks == 10
    assert lib.vf_weight_count(ctypes.byref(c)) == CdnaWeights.random(cfg, seed=0).n_floats() > 0
    assert lib.vf_macs_per_sample_step(ctypes.byref(c)) == sum(cfg.macs_per_sample_step().values())
    c0 = _c_cfg(CdnaConfig(height=H, width=W, ndesig=nd))
    assert lib.vf_weight_count(ctypes.byref(c0)) > lib.vf_weight_count(ctypes.byref(c))
    # a frames-only stp handle is a valid configuration (ndesig 0)
    assert lib.vf_weight_count(ctypes.byref(_c_cfg(cfg, ndesig=0))) == lib.vf_weight_count(ctypes.byref(c))
    assert lib.vf_abi_version() == 7


def test_refusals_of_the_library():
    lib = _lib.load_library()
    cfg = StpConfig()
    for precision in (1, 2):                                        # exact fp32 only
        bad = _c_cfg(cfg, precision=precision)
        assert lib.vf_weight_count(ctypes.byref(bad)) == 0
        assert b'STP table (arch 0, layer_spec 4)' in lib.vf_last_error() and b'precision 0' in lib.vf_last_error()
        assert lib.vf_macs_per_sample_step(ctypes.byref(bad)) == 0.0
        h = ctypes.c_void_p()
        assert lib.vf_create(ctypes.byref(bad), ctypes.byref(h)) == -1 and not h.value
    for masks in (0, 1, 6, 9, 11):                                  # nine transforms
        bad = _c_cfg(cfg, num_masks=masks)
        assert lib.vf_weight_count(ctypes.byref(bad)) == 0
        assert b'layer_spec 4' in lib.vf_last_error() and b'num_masks must be 10' in lib.vf_last_error()
    for arch, size, adim, masks in ((1, 128, 12, 10), (2, 128, 12, 6), (2, 128, 12, 10)):    # layer_spec 4 belongs to arch 0
        c = _lib.VfConfig(size, size, adim, 5, 1, 2, 15, masks, 4, 0, 0, 1, 1, arch, 0, 4)
        assert lib.vf_weight_count(ctypes.byref(c)) == 0
        assert b'layer_spec' in lib.vf_last_error() and b'arch 0' in lib.vf_last_error()
    c = _lib.VfConfig(64, 64, 12, 5, 1, 2, 15, 4, 4, 0, 0, 1, 1, 3, 8, 4)       # arch 3 reads the field as its own table
    assert lib.vf_weight_count(ctypes.byref(c)) == 0 and b'layer_spec' in lib.vf_last_error()
    c = _lib.VfConfig(64, 64, 4, 5, 1, 2, 15, 10, 4, 0, 0, 1, 1, 0, 0, 5)       # no fifth table
    assert lib.vf_weight_count(ctypes.byref(c)) == 0 and b'layer_spec' in lib.vf_last_error()
    c = _c_cfg(DnaConfig(), num_masks=10)                                       # layer_spec 3 with ten masks stays refused
    assert lib.vf_weight_count(ctypes.byref(c)) == 0 and b'layer_spec 3' in lib.vf_last_error()


def test_refusals_in_python():
    with pytest.raises(ValueError, match="'survey' decoder only"):
        StpConfig(decoder='public')
    with pytest.raises(ValueError, match='num_masks = 10'):
        StpConfig(num_masks=1)
    with pytest.raises(ValueError, match="transformation 'stp'"):
        StpConfig(transformation='flow')
    with pytest.raises(ValueError, match="transformation must be 'cdna' or 'flow'"):     # CdnaConfig is not widened
        CdnaConfig(transformation='stp')
    from visual_foresight_amd.video_prediction import checkpoint_import
    cfg = StpConfig(height=16, width=16)
    with pytest.raises(ValueError, match='no TensorFlow name table exists for the STP head'):
        checkpoint_import.import_named_arrays({}, cfg)
    with pytest.raises(ValueError, match='no TensorFlow name table'):
        checkpoint_import.export_named_arrays(CdnaWeights.random(cfg, seed=0))


def test_manifest_round_trip_and_mismatch(tmp_path):
    stp = StpConfig(height=16, width=16)
    cdna = CdnaConfig(height=16, width=16)
    flow = CdnaConfig(height=16, width=16, transformation='flow')
    dna = DnaConfig(height=16, width=16)
    w = CdnaWeights.random(stp, seed=5, bias_scale=0.05)
    w.save(str(tmp_path / 'stp'))
    with open(str(tmp_path / 'stp' / 'manifest.json')) as f:
        man = json.load(f)
    assert man['arch'] == 'stp' and man['config']['num_masks'] == 10 and 'transformation' not in man['config']
    assert [t['name'] for t in man['tensors']][-6:] == ['stp_fc/w', 'stp_fc/b', 'stp/w', 'stp/b', 'state/w', 'state/b']
    for cfg in (None, stp, StpConfig(height=16, width=16, ndesig=3, sequence_length=7)):
        back = CdnaWeights.load(str(tmp_path / 'stp'), cfg)
        assert isinstance(back.cfg, StpConfig) and back.cfg.layer_spec == 4 and list(back.tensors) == list(w.tensors)
        assert all(np.array_equal(back.tensors[k], w.tensors[k]) for k in w.tensors)
    with pytest.raises(ValueError, match="checkpoint height=16 does not match requested 32"):
        CdnaWeights.load(str(tmp_path / 'stp'), StpConfig(height=32, width=16))
    for other in (cdna, flow, dna):         # an stp checkpoint is refused for another table ...
        with pytest.raises(ValueError, match="checkpoint architecture 'stp' does not match requested '%s'" % other.arch):
            CdnaWeights.load(str(tmp_path / 'stp'), other)
    for name, other in (('cdna', cdna), ('flow', flow), ('dna', dna)):    # ... and the reverse
        CdnaWeights.random(other, seed=5).save(str(tmp_path / name))
        with pytest.raises(ValueError, match="checkpoint architecture '%s' does not match requested 'stp'" % other.arch):
            CdnaWeights.load(str(tmp_path / name), stp)
        assert CdnaWeights.load(str(tmp_path / name), other).cfg.transformation == other.transformation


def test_predictor_hyper_parameters_select_the_table():
    """The constructor needs a GPU; which table a hyper-parameter dictionary selects is decided before it asks for one."""
    from visual_foresight_amd.video_prediction import hip_predictor
    sel = hip_predictor.transformation_of
    assert sel({'transformation': 'stp'}) == 'stp'
    assert sel({'model': 'STP'}) == 'cdna' and sel({'model': 'stp'}) == 'cdna'      # the legacy key keeps selecting cdna
    assert sel({'model': 'STP', 'transformation': 'stp'}) == 'stp'
    assert sel({'model': 'dna', 'transformation': 'stp'}) == 'stp' and sel({'model': 'appflow', 'transformation': 'stp'}) == 'stp'
    assert sel({}) == 'cdna' and sel({'model': 'DNA'}) == 'dna' and sel({'model': 'appflow'}) == 'flow'


# the stp shapes of tools/sanitize/host_selftest.cc: shape line -> batches
STP_SHAPES = {'64x64 adim 9 nd 2 ncam 1': (1, 7, 16, 37),
              '40x56 adim 9 nd 4 ncam 2': (1, 7, 16),
              '32x32 adim 9 nd 1 ncam 1': (1, 7, 16),
              '64x64 adim 9 nd 1 ncam 1': (200, 125, 25)}


@pytest.mark.slow
def test_stp_schedule_passes_the_host_selftest_and_is_as_long_as_the_cdna_twin():
    """The persistent schedule of an stp engine on the CPU (the host self-test build of the engine):
    ``vf_selftest_schedule`` refuses an stp schedule whose compositing phase lacks the finish dependency or the table of
    transforms, or that carries a flow / dna head or a CDNA kernel-finish item, and checks every pointer of every phase.
    Each stp shape is printed behind the cdna table of the same shape.  The derived difference of their item counts is 0:
    per predicted step and view an stp schedule holds the FC's K splits - the first FC reads the same ``H/8 * W/8 * 128``
    inputs in the same 32-channel chunks, so the same number of splits, and the wide FC tile holds all column groups (four
    of 100 columns or eight of 250) in ONE item per (128-row tile, split) - and one finish item per sample, exactly where
    the cdna schedule holds its FC items and kernel-finish items; every other phase is shared."""
    import re
    import shutil
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')):
        pytest.skip('hipcc not available')
    proc = subprocess.run(['bash', os.path.join(repo, 'tools', 'sanitize', 'build_and_run.sh')], stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True, timeout=900)
    assert proc.returncode == 0 and 'HOST SELFTEST OK' in proc.stdout, proc.stdout[-4000:]
    for shape, batches in STP_SHAPES.items():
        rows = re.findall(r'^  %s prec 0  B=(\d+)\s+([^:]+): (\d+) items$' % shape, proc.stdout, re.M)
        n = 4 * len(batches)                    # full / cached context x fused / two-phase top
        assert len(rows) == 2 * n, (shape, len(rows))
        cdna, stp = rows[:n], rows[n:]          # the cdna table first
        assert sorted(set(int(b) for b, _, _ in stp)) == sorted(batches)
        for (b0, v0, n0), (b1, v1, n1) in zip(cdna, stp):
            assert (b0, v0) == (b1, v1)
            assert int(n0) - int(n1) == 0, (shape, b0, v0, n0, n1)
