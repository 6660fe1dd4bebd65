"""Appearance-flow compositing (``CdnaConfig(transformation='flow')``, ``vf_config`` arch 0 / layer_spec 2) without a GPU:
the helper oracle's warp against naive loops, the table in Python against the table behind the C ABI, and the refusals."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers import oracle_appflow
from visual_foresight_amd import _lib
from visual_foresight_amd.video_prediction.cdna_arch import CdnaConfig, CdnaWeights


def _c_cfg(cfg, precision=0, arch=0, layer_spec=None, max_batch=4):
    return _lib.VfConfig(cfg.height, cfg.width, cfg.adim, cfg.sdim, cfg.ndesig, cfg.n_context, cfg.sequence_length,
                         cfg.num_masks, max_batch, 0, precision, 1, 1, arch, 0,
                         cfg.layer_spec if layer_spec is None else layer_spec)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_vectorised_warp_equals_naive_loops_bit_for_bit(dtype):
    """8 x 8, two channels (ND 2), flows that reach past all four borders and land exactly on pixels and on the last
    row / column (x1 = min(x0 + 1, W - 1))."""
    rs = np.random.RandomState(4)
    B, C, H, W = 3, 2, 8, 8
    img = torch.from_numpy(rs.uniform(0, 1, (B, C, H, W))).to(dtype)
    dx = torch.from_numpy(rs.uniform(-12, 12, (B, H, W))).to(dtype)
    dy = torch.from_numpy(rs.uniform(-12, 12, (B, H, W))).to(dtype)
    dx[0, 0, :4] = torch.tensor([0., 1., -1., 7.]).to(dtype)        # whole-pixel shifts, the last one onto column W - 1
    dy[0, 0, :4] = torch.tensor([0., 7., 2.5, 6.75]).to(dtype)
    x = np.arange(W)[None, None, :] + dx.numpy()
    y = np.arange(H)[None, :, None] + dy.numpy()
    assert (x < 0).any() and (x > W - 1).any() and (y < 0).any() and (y > H - 1).any()
    got = oracle_appflow.warp_bilinear(img, dx, dy).numpy()
    want = oracle_appflow.warp_bilinear_loops(img.numpy(), dx.numpy(), dy.numpy())
    assert got.dtype == want.dtype
    np.testing.assert_array_equal(got, want)
    # a zero flow is the identity, a flow far outside takes the corner it clamps to
    zero = torch.zeros(B, H, W, dtype=dtype)
    np.testing.assert_array_equal(oracle_appflow.warp_bilinear(img, zero, zero).numpy(), img.numpy())
    far = oracle_appflow.warp_bilinear(img, zero + 40, zero - 40).numpy()
    np.testing.assert_array_equal(far, np.broadcast_to(img.numpy()[:, :, :1, -1:], far.shape))


def test_table_in_python():
    cfg = CdnaConfig(ndesig=2, transformation='flow')
    cdna = CdnaConfig(ndesig=2)
    assert cfg.layer_spec == 2 and cdna.layer_spec == 0 and cdna.transformation == 'cdna'
    shp, ref = cfg.tensor_shapes(), cdna.tensor_shapes()
    assert 'cdna/w' not in shp and 'cdna/b' not in shp
    assert shp['flow/w'] == (1, 1, 32, 18) and shp['flow/b'] == (18,)
    # flow/w, flow/b sit where cdna/w, cdna/b sat; every other tensor is the survey table's
    assert [n.replace('flow/', 'cdna/') for n in shp] == list(ref)
    assert all(shp[n] == ref[n] for n in shp if not n.startswith('flow/'))
    assert {k: tuple(v) for k, v in shp.items()} == oracle_appflow.expected_shapes(cfg)
    macs, macs_ref = cfg.macs_per_sample_step(), cdna.macs_per_sample_step()
    assert 'cdna_fc' not in macs
    assert macs['flow'] == 64 * 64 * 32 * 18
    assert macs['warp_frame'] + macs['warp_distrib'] == 64 * 64 * 4 * (3 + 2) * 9
    same = [k for k in macs_ref if k not in ('cdna_fc', 'warp_frame', 'warp_distrib')]
    assert all(macs[k] == macs_ref[k] for k in same) and len(macs) == len(same) + 3
    # the oracle helper accepts this table's weights and refuses the cdna table's
    oracle_appflow.OracleAppflow(CdnaWeights.random(CdnaConfig(height=16, width=16, transformation='flow'), seed=0))
    with pytest.raises(ValueError, match='layer table'):
        oracle_appflow.OracleAppflow(CdnaWeights.random(CdnaConfig(height=16, width=16), seed=0))


@pytest.mark.parametrize('H,W,nd', [(64, 64, 1), (48, 64, 2), (40, 56, 4)])
def test_c_abi_table_equals_python_table(H, W, nd):
    cfg = CdnaConfig(height=H, width=W, ndesig=nd, transformation='flow')
    lib = _lib.load_library()
    c = _c_cfg(cfg)
    assert c.arch == 0 and c.layer_spec == 2
    assert lib.vf_weight_count(ctypes.byref(c)) == CdnaWeights.random(cfg, seed=0).n_floats()
    assert lib.vf_macs_per_sample_step(ctypes.byref(c)) == sum(cfg.macs_per_sample_step().values())
    # ... and differs from the cdna table's of the same shape
    c0 = _c_cfg(CdnaConfig(height=H, width=W, ndesig=nd))
    assert lib.vf_weight_count(ctypes.byref(c0)) > lib.vf_weight_count(ctypes.byref(c))
    assert lib.vf_abi_version() == 7


def test_refusals_of_the_library():
    lib = _lib.load_library()
    cfg = CdnaConfig(transformation='flow')
    bad = _c_cfg(cfg, precision=1)                                  # exact fp32 only
    assert lib.vf_weight_count(ctypes.byref(bad)) == 0
    assert b'appearance-flow table (arch 0, layer_spec 2)' in lib.vf_last_error() and b'precision 0' in lib.vf_last_error()
    assert lib.vf_macs_per_sample_step(ctypes.byref(bad)) == 0.0
    h = ctypes.c_void_p()
    assert lib.vf_create(ctypes.byref(bad), ctypes.byref(h)) == -1 and not h.value
    assert b'appearance-flow' in lib.vf_last_error()
    for arch, size, adim, masks in ((1, 128, 12, 10), (2, 128, 12, 6)):        # layer_spec 2 belongs to arch 0
        c = _lib.VfConfig(size, size, adim, 5, 1, 2, 15, masks, 4, 0, 0, 1, 1, arch, 0, 2)
        assert lib.vf_weight_count(ctypes.byref(c)) == 0
        assert b'layer_spec' in lib.vf_last_error() and b'arch 0' in lib.vf_last_error()
    c = _lib.VfConfig(64, 64, 12, 5, 1, 2, 15, 4, 4, 0, 0, 1, 1, 3, 8, 2)       # arch 3 reads the field as its own table
    assert lib.vf_weight_count(ctypes.byref(c)) == 0 and b'layer_spec' in lib.vf_last_error()
    c = _lib.VfConfig(64, 64, 4, 5, 1, 2, 15, 10, 4, 0, 0, 1, 1, 0, 0, 3)       # no third table
    assert lib.vf_weight_count(ctypes.byref(c)) == 0 and b'layer_spec' in lib.vf_last_error()


def test_refusals_in_python():
    with pytest.raises(ValueError, match="transformation must be 'cdna' or 'flow'"):
        CdnaConfig(transformation='dna')
    with pytest.raises(ValueError, match="'survey' decoder only"):
        CdnaConfig(transformation='flow', decoder='public')
    with pytest.raises(ValueError, match='num_masks = 10'):
        CdnaConfig(transformation='flow', num_masks=6)
    from visual_foresight_amd.video_prediction.savp_arch import SavpConfig, Savp2Config
    from visual_foresight_amd.video_prediction.savp3_arch import Savp3Config
    for cls in (SavpConfig, Savp2Config, Savp3Config):              # the other architectures keep refusing the key
        with pytest.raises(TypeError):
            cls(transformation='flow')
    from visual_foresight_amd.video_prediction import checkpoint_import
    cfg = CdnaConfig(height=16, width=16, transformation='flow')
    with pytest.raises(ValueError, match='no TensorFlow name table exists for the appearance-flow head'):
        checkpoint_import.import_named_arrays({}, cfg)
    with pytest.raises(ValueError, match='no TensorFlow name table'):
        checkpoint_import.export_named_arrays(CdnaWeights.random(cfg, seed=0))


def test_manifest_round_trip_and_mismatch(tmp_path):
    flow = CdnaConfig(height=16, width=16, transformation='flow')
    cdna = CdnaConfig(height=16, width=16)
    assert 'transformation' not in cdna.as_dict()                   # manifests of cdna checkpoints are unchanged
    assert flow.as_dict()['transformation'] == 'flow'
    w = CdnaWeights.random(flow, seed=5, bias_scale=0.05)
    w.save(str(tmp_path / 'flow'))
    with open(str(tmp_path / 'flow' / 'manifest.json')) as f:
        man = json.load(f)
    assert man['config']['transformation'] == 'flow' and man['arch'] == 'cdna'
    assert [t['name'] for t in man['tensors']][-4:] == ['flow/w', 'flow/b', 'state/w', 'state/b']
    for cfg in (None, flow, CdnaConfig(height=16, width=16, ndesig=3, sequence_length=7, transformation='flow')):
        back = CdnaWeights.load(str(tmp_path / 'flow'), cfg)
        assert back.cfg.transformation == 'flow' and list(back.tensors) == list(w.tensors)
        assert all(np.array_equal(back.tensors[k], w.tensors[k]) for k in w.tensors)
    with pytest.raises(ValueError, match="checkpoint transformation='flow' does not match requested 'cdna'"):
        CdnaWeights.load(str(tmp_path / 'flow'), cdna)
    CdnaWeights.random(cdna, seed=5).save(str(tmp_path / 'cdna'))
    with open(str(tmp_path / 'cdna' / 'manifest.json')) as f:
        assert 'transformation' not in json.load(f)['config']
    with pytest.raises(ValueError, match="checkpoint transformation='cdna' does not match requested 'flow'"):
        CdnaWeights.load(str(tmp_path / 'cdna'), flow)
    assert CdnaWeights.load(str(tmp_path / 'cdna'), cdna).cfg.transformation == 'cdna'


def test_predictor_hyper_parameters_select_the_table():
    """The constructor needs a GPU; which table a hyper-parameter dictionary selects is decided before it asks for one."""
    from visual_foresight_amd.video_prediction import hip_predictor
    sel = hip_predictor.transformation_of
    assert sel({}) == 'cdna' and sel({'model': 'CDNA'}) == 'cdna'
    assert sel({'transformation': 'flow'}) == 'flow'
    assert sel({'model': 'appflow'}) == 'flow'                      # the key of the reference's legacy configurations
    assert sel({'model': 'appflow', 'transformation': 'cdna'}) == 'cdna'       # ... only when 'transformation' is absent


@pytest.mark.slow
def test_flow_schedule_has_no_kernel_items_and_passes_the_host_selftest():
    """The persistent schedule of a flow engine on the CPU (the host self-test build of the engine, as
    ``tests/test_share_recurrent_schedule.py`` uses it): ``vf_selftest_schedule`` refuses a flow schedule that holds a CDNA FC
    or kernel-finish item or a compositing phase without the flow head, and checks every pointer of every phase.  Against the
    cdna table of the same shape a flow schedule is shorter by exactly those items: per predicted step (T = 3) the FC's
    32 K-splits of one 128-row tile and one finish item per sample - fused and two-phase top, full and cached context."""
    import re
    import shutil
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')):
        pytest.skip('hipcc not available')
    proc = subprocess.run(['bash', os.path.join(repo, 'tools', 'sanitize', 'build_and_run.sh')], stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True, timeout=900)
    assert proc.returncode == 0 and 'HOST SELFTEST OK' in proc.stdout, proc.stdout[-4000:]
    rows = re.findall(r'^  64x64 adim 7 nd 2 ncam 1 prec 0  B=(\d+)\s+([^:]+): (\d+) items$', proc.stdout, re.M)
    assert len(rows) == 32                      # the cdna table first, then the flow table: 4 batches x 4 variants each
    cdna, flow = rows[:16], rows[16:]
    for (b0, v0, n0), (b1, v1, n1) in zip(cdna, flow):
        assert (b0, v0) == (b1, v1)
        assert int(n0) - int(n1) == 3 * (32 + int(b0)), (b0, v0, n0, n1)
    # the other flow shapes were built and verified too: 32 x 32 with one context frame, 40 x 56 (two views, four pixels,
    # a top that cannot be fused), the 200-sample planning shape
    for shape, n in (('32x32 adim 7 nd 1 ncam 1', 12), ('40x56 adim 7 nd 4 ncam 2', 12), ('64x64 adim 7 nd 1 ncam 1', 12)):
        assert len(re.findall(r'^  %s prec 0  B=' % shape, proc.stdout, re.M)) == n
