"""DNA compositing (``DnaConfig``, ``vf_config`` arch 0 / layer_spec 3 / num_masks 1) without a GPU: the helper oracle's warp
against naive loops, the table in Python against the table behind the C ABI, the refusals, and the persistent schedule of a
dna engine in the host self-test."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers import oracle_dna
from visual_foresight_amd import _lib
from visual_foresight_amd.video_prediction.cdna_arch import CdnaConfig, CdnaWeights
from visual_foresight_amd.video_prediction.dna_arch import DnaConfig


def _c_cfg(cfg, precision=0, arch=0, layer_spec=None, num_masks=None, max_batch=4):
    return _lib.VfConfig(cfg.height, cfg.width, cfg.adim, cfg.sdim, cfg.ndesig, cfg.n_context, cfg.sequence_length,
                         cfg.num_masks if num_masks is None else num_masks, max_batch, 0, precision, 1, 1, arch, 0,
                         cfg.layer_spec if layer_spec is None else layer_spec)


def _wrap(x):
    """``x [B, C, H, W]`` continued periodically by two pixels on every side."""
    return torch.nn.functional.pad(x, (2, 2, 2, 2), mode='circular')


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_vectorised_warp_equals_naive_loops_bit_for_bit(dtype):
    """8 x 8, two channels: every pixel within two of a border has taps outside the image on that side, the corners on two
    sides at once; the kernels are those ``dna_kernels`` makes of random head outputs (some taps at the relu shift)."""
    rs = np.random.RandomState(4)
    B, C, H, W = 3, 2, 8, 8
    img = torch.from_numpy(rs.uniform(0, 1, (B, C, H, W))).to(dtype)
    m0, ke = oracle_dna.dna_kernels(torch.from_numpy(rs.normal(0, 1, (B, 2, H, W))).to(dtype),
                                    torch.from_numpy(rs.normal(0, 1, (B, 25, H, W))).to(dtype))
    assert (ke < 1e-10).any() and (ke > 1e-3).any()
    got = oracle_dna.dna_warp(img, ke, m0 * img).numpy()
    want = oracle_dna.dna_warp_loops(img.numpy(), ke.numpy(), (m0 * img).numpy())
    assert got.dtype == want.dtype == img.numpy().dtype
    np.testing.assert_array_equal(got, want)
    # the borders are on the path: against a wrap-around border the result differs in every border band, and only there
    wrapped = oracle_dna.dna_warp(_wrap(img), _wrap(ke), _wrap(m0 * img)).numpy()[:, :, 2:-2, 2:-2]
    diff = np.abs(wrapped - got).max(axis=(0, 1)) > 0
    assert diff[:2].any() and diff[-2:].any() and diff[:, :2].any() and diff[:, -2:].any() and not diff[2:-2, 2:-2].any()
    # a one-hot centre kernel is the identity; a one-hot tap (dy, dx) shifts the image by (dy - 2, dx - 2) with zeros entering
    one = torch.zeros(B, 25, H, W, dtype=dtype)
    one[:, 12] = 1
    np.testing.assert_array_equal(oracle_dna.dna_warp(img, one, torch.zeros_like(img)).numpy(), img.numpy())
    one = torch.zeros(B, 25, H, W, dtype=dtype)
    one[:, 4] = 1                                                   # tap (0, 4): out[y, x] = img[y - 2, x + 2]
    shifted = np.zeros_like(img.numpy())
    shifted[:, :, 2:, :-2] = img.numpy()[:, :, :-2, 2:]
    np.testing.assert_array_equal(oracle_dna.dna_warp(img, one, torch.zeros_like(img)).numpy(), shifted)


def test_table_in_python():
    cfg = DnaConfig(ndesig=2)
    cdna = CdnaConfig(ndesig=2)
    assert cfg.layer_spec == 3 and cfg.transformation == 'dna' and cfg.num_masks == 1 and cfg.arch_id == 0 and cfg.arch == 'dna'
    shp, ref = cfg.tensor_shapes(), cdna.tensor_shapes()
    assert not any(n.startswith(('rgb/', 'cdna/')) for n in shp)
    assert shp['masks/w'] == (1, 1, 32, 2) and shp['masks/b'] == (2,)
    assert shp['dna/w'] == (1, 1, 32, 25) and shp['dna/b'] == (25,)
    # the survey table through ln9, then masks, dna, state
    names, ref_names = list(shp), list(ref)
    cut = ref_names.index('ln9/b') + 1
    assert names[:cut] == ref_names[:cut] and all(shp[n] == ref[n] for n in names[:cut])
    assert names[cut:] == ['masks/w', 'masks/b', 'dna/w', 'dna/b', 'state/w', 'state/b']
    assert shp['state/w'] == ref['state/w'] and shp['state/b'] == ref['state/b']
    assert {k: tuple(v) for k, v in shp.items()} == oracle_dna.expected_shapes(cfg)
    macs, macs_ref = cfg.macs_per_sample_step(), cdna.macs_per_sample_step()
    assert 'cdna_fc' not in macs and 'rgb' not in macs
    assert macs['dna'] == 64 * 64 * 32 * 25 and macs['masks'] == 64 * 64 * 32 * 2
    assert macs['warp_frame'] == 64 * 64 * 25 * 3 and macs['warp_distrib'] == 64 * 64 * 25 * 2
    same = [k for k in macs_ref if k not in ('rgb', 'masks', 'cdna_fc', 'warp_frame', 'warp_distrib')]
    assert all(macs[k] == macs_ref[k] for k in same) and len(macs) == len(same) + 4
    # as_dict() of cdna and flow configs is what it was
    assert cdna.as_dict() == dict(height=64, width=64, adim=4, sdim=5, ndesig=2, n_context=2, sequence_length=15, num_masks=10)
    assert CdnaConfig(transformation='flow').as_dict()['transformation'] == 'flow'
    assert 'transformation' not in cfg.as_dict() and cfg.as_dict()['num_masks'] == 1
    # the oracle helper accepts this table's weights and refuses the cdna table's
    oracle_dna.OracleDna(CdnaWeights.random(DnaConfig(height=16, width=16), seed=0))
    with pytest.raises(ValueError, match='layer table'):
        oracle_dna.OracleDna(CdnaWeights.random(CdnaConfig(height=16, width=16), seed=0))


@pytest.mark.parametrize('H,W,nd', [(64, 64, 1), (48, 64, 2), (40, 56, 4)])
def test_c_abi_table_equals_python_table(H, W, nd):
    cfg = DnaConfig(height=H, width=W, ndesig=nd)
    lib = _lib.load_library()
    c = _c_cfg(cfg)
    assert c.arch == 0 and c.layer_spec == 3 and c.num_masks == 1
    assert lib.vf_weight_count(ctypes.byref(c)) == CdnaWeights.random(cfg, seed=0).n_floats() > 0
    assert lib.vf_macs_per_sample_step(ctypes.byref(c)) == sum(cfg.macs_per_sample_step().values())
    c0 = _c_cfg(CdnaConfig(height=H, width=W, ndesig=nd))
    assert lib.vf_weight_count(ctypes.byref(c0)) > lib.vf_weight_count(ctypes.byref(c))
    assert lib.vf_abi_version() == 7


def test_refusals_of_the_library():
    lib = _lib.load_library()
    cfg = DnaConfig()
    for precision in (1, 2):                                        # exact fp32 only
        bad = _c_cfg(cfg, precision=precision)
        assert lib.vf_weight_count(ctypes.byref(bad)) == 0
        assert b'DNA table (arch 0, layer_spec 3)' in lib.vf_last_error() and b'precision 0' in lib.vf_last_error()
        assert lib.vf_macs_per_sample_step(ctypes.byref(bad)) == 0.0
        h = ctypes.c_void_p()
        assert lib.vf_create(ctypes.byref(bad), ctypes.byref(h)) == -1 and not h.value
    for masks in (0, 2, 6, 10):                                     # one transform
        bad = _c_cfg(cfg, num_masks=masks)
        assert lib.vf_weight_count(ctypes.byref(bad)) == 0
        assert b'layer_spec 3' in lib.vf_last_error() and b'num_masks must be 1' in lib.vf_last_error()
    assert lib.vf_weight_count(ctypes.byref(_c_cfg(CdnaConfig(), num_masks=1))) == 0       # ... and only the dna table has one
    for arch, size, adim, masks in ((1, 128, 12, 10), (2, 128, 12, 6), (1, 128, 12, 1)):    # layer_spec 3 belongs to arch 0
        c = _lib.VfConfig(size, size, adim, 5, 1, 2, 15, masks, 4, 0, 0, 1, 1, arch, 0, 3)
        assert lib.vf_weight_count(ctypes.byref(c)) == 0
        assert b'layer_spec' in lib.vf_last_error() and b'arch 0' in lib.vf_last_error()
    c = _lib.VfConfig(64, 64, 12, 5, 1, 2, 15, 4, 4, 0, 0, 1, 1, 3, 8, 3)       # arch 3 reads the field as its own table
    assert lib.vf_weight_count(ctypes.byref(c)) == 0 and b'layer_spec' in lib.vf_last_error()
    c = _lib.VfConfig(64, 64, 4, 5, 1, 2, 15, 1, 4, 0, 0, 1, 1, 0, 0, 4)        # no fourth table
    assert lib.vf_weight_count(ctypes.byref(c)) == 0 and b'layer_spec' in lib.vf_last_error()


def test_refusals_in_python():
    with pytest.raises(ValueError, match="'survey' decoder only"):
        DnaConfig(decoder='public')
    with pytest.raises(ValueError, match='num_masks = 1'):
        DnaConfig(num_masks=10)
    with pytest.raises(ValueError, match="transformation 'dna'"):
        DnaConfig(transformation='flow')
    with pytest.raises(ValueError, match="transformation must be 'cdna' or 'flow'"):     # CdnaConfig is not widened
        CdnaConfig(transformation='dna')
    from visual_foresight_amd.video_prediction import checkpoint_import
    cfg = DnaConfig(height=16, width=16)
    with pytest.raises(ValueError, match='no TensorFlow name table exists for the DNA head'):
        checkpoint_import.import_named_arrays({}, cfg)
    with pytest.raises(ValueError, match='no TensorFlow name table'):
        checkpoint_import.export_named_arrays(CdnaWeights.random(cfg, seed=0))


def test_manifest_round_trip_and_mismatch(tmp_path):
    dna = DnaConfig(height=16, width=16)
    cdna = CdnaConfig(height=16, width=16)
    flow = CdnaConfig(height=16, width=16, transformation='flow')
    w = CdnaWeights.random(dna, seed=5, bias_scale=0.05)
    w.save(str(tmp_path / 'dna'))
    with open(str(tmp_path / 'dna' / 'manifest.json')) as f:
        man = json.load(f)
    assert man['arch'] == 'dna' and man['config']['num_masks'] == 1 and 'transformation' not in man['config']
    assert [t['name'] for t in man['tensors']][-6:] == ['masks/w', 'masks/b', 'dna/w', 'dna/b', 'state/w', 'state/b']
    for cfg in (None, dna, DnaConfig(height=16, width=16, ndesig=3, sequence_length=7)):
        back = CdnaWeights.load(str(tmp_path / 'dna'), cfg)
        assert isinstance(back.cfg, DnaConfig) and back.cfg.layer_spec == 3 and list(back.tensors) == list(w.tensors)
        assert all(np.array_equal(back.tensors[k], w.tensors[k]) for k in w.tensors)
    with pytest.raises(ValueError, match="checkpoint height=16 does not match requested 32"):
        CdnaWeights.load(str(tmp_path / 'dna'), DnaConfig(height=32, width=16))
    for other in (cdna, flow):              # a dna checkpoint is refused for a cdna or flow config ...
        with pytest.raises(ValueError, match="checkpoint architecture 'dna' does not match requested 'cdna'"):
            CdnaWeights.load(str(tmp_path / 'dna'), other)
    for name, other in (('cdna', cdna), ('flow', flow)):    # ... and the reverse
        CdnaWeights.random(other, seed=5).save(str(tmp_path / name))
        with pytest.raises(ValueError, match="checkpoint architecture 'cdna' does not match requested 'dna'"):
            CdnaWeights.load(str(tmp_path / name), dna)
        assert CdnaWeights.load(str(tmp_path / name), other).cfg.transformation == other.transformation


def test_predictor_hyper_parameters_select_the_table():
    """The constructor needs a GPU; which table a hyper-parameter dictionary selects is decided before it asks for one."""
    from visual_foresight_amd.video_prediction import hip_predictor
    sel = hip_predictor.transformation_of
    assert sel({}) == 'cdna' and sel({'model': 'CDNA'}) == 'cdna' and sel({'model': 'STP'}) == 'cdna'
    assert sel({'transformation': 'dna'}) == 'dna'
    assert sel({'model': 'DNA'}) == 'dna' and sel({'model': 'dna'}) == 'dna' and sel({'model': 'Dna'}) == 'dna'
    assert sel({'model': 'dna', 'transformation': 'cdna'}) == 'cdna'            # ... only when 'transformation' is absent
    assert sel({'model': 'dna', 'transformation': 'flow'}) == 'flow'
    assert sel({'model': 'appflow'}) == 'flow' and sel({'model': 'appflow', 'transformation': 'dna'}) == 'dna'


# the dna shapes of tools/sanitize/host_selftest.cc: shape line -> (predicted steps T, views, batches, K splits of the CDNA FC)
# The FC reads H/8 * W/8 * 128 inputs in chunks of 32, dealt to at most 32 splits of equal chunk count.
def _fc_splits(H, W):
    chunks = (H // 8) * (W // 8) * 128 // 32
    per = -(-chunks // min(32, chunks))
    return -(-chunks // per)


DNA_SHAPES = {'64x64 adim 5 nd 2 ncam 1': (3, 1, (1, 7, 16, 37), _fc_splits(64, 64)),
              '40x56 adim 5 nd 4 ncam 2': (2, 2, (1, 7, 16), _fc_splits(40, 56)),
              '32x32 adim 5 nd 1 ncam 1': (2, 1, (1, 7, 16), _fc_splits(32, 32)),
              '64x64 adim 5 nd 1 ncam 1': (13, 1, (200, 125, 25), _fc_splits(64, 64))}


@pytest.mark.slow
def test_dna_schedule_has_no_kernel_items_and_passes_the_host_selftest():
    """The persistent schedule of a dna engine on the CPU (the host self-test build of the engine):
    ``vf_selftest_schedule`` refuses a dna schedule that holds a CDNA FC or kernel-finish item or a compositing phase without
    the dna head, and checks every pointer of every phase.  Each dna shape is printed behind the cdna table of the same
    shape, and is shorter than it by exactly the kernel items: per predicted step and view the FC's K splits (32; one
    128-row tile of samples each) and one finish item per sample - ``T * (32 + B)`` with one view and up to 128 samples -
    for the fused and the two-phase top, full and cached context."""
    import re
    import shutil
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')):
        pytest.skip('hipcc not available')
    proc = subprocess.run(['bash', os.path.join(repo, 'tools', 'sanitize', 'build_and_run.sh')], stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True, timeout=900)
    assert proc.returncode == 0 and 'HOST SELFTEST OK' in proc.stdout, proc.stdout[-4000:]
    assert _fc_splits(64, 64) == _fc_splits(32, 32) == 32
    for shape, (T, ncam, batches, splits) in DNA_SHAPES.items():
        rows = re.findall(r'^  %s prec 0  B=(\d+)\s+([^:]+): (\d+) items$' % shape, proc.stdout, re.M)
        n = 4 * len(batches)                    # full / cached context x fused / two-phase top
        assert len(rows) == 2 * n, (shape, len(rows))
        cdna, dna = rows[:n], rows[n:]          # the cdna table first
        assert sorted(set(int(b) for b, _, _ in dna)) == sorted(batches)
        for (b0, v0, n0), (b1, v1, n1) in zip(cdna, dna):
            assert (b0, v0) == (b1, v1)
            B = int(b0)
            want = T * ncam * (splits * -(-B // 128) + B)
            if ncam == 1 and B <= 128 and splits == 32:
                assert want == T * (32 + B)
            assert int(n0) - int(n1) == want, (shape, b0, v0, n0, n1)
