"""Where ``vf_config.precision = 2`` (plain bf16) is accepted and where it is refused - validation precedes device access, so
this runs without a GPU (as tests/test_lib_abi.py does)."""
import ctypes

import pytest

from visual_foresight_amd import _lib


def _cfg(arch=0, layer_spec=0, precision=2, size=64, adim=4, masks=10, zdim=0):
    return _lib.VfConfig(size, size, adim, 5, 1, 2, 6, masks, 4, 0, precision, 1, 1, arch, zdim, layer_spec)


def _refused(cfg):
    lib = _lib.load_library()
    h = ctypes.c_void_p()
    assert lib.vf_create(ctypes.byref(cfg), ctypes.byref(h)) == -1 and not h.value
    assert lib.vf_weight_count(ctypes.byref(cfg)) == 0
    return lib.vf_last_error()


@pytest.mark.parametrize('precision', [1, 2])
def test_accepted_exactly_where_the_split_mode_is(precision):
    lib = _lib.load_library()
    assert lib.vf_weight_count(ctypes.byref(_cfg(0, 0, precision))) == lib.vf_weight_count(ctypes.byref(_cfg(0, 0, 0))) > 0
    assert lib.vf_weight_count(ctypes.byref(_cfg(1, 0, precision, adim=6))) == \
        lib.vf_weight_count(ctypes.byref(_cfg(1, 0, 0, adim=6))) > 0


@pytest.mark.parametrize('precision', [1, 2])
def test_refused_combinations(precision):
    msg = _refused(_cfg(0, 1, precision))
    assert b'public decoder table (arch 0, layer_spec 1)' in msg and b'precision 0 (exact fp32) only' in msg
    msg = _refused(_cfg(0, 2, precision))
    assert b'appearance-flow table (arch 0, layer_spec 2)' in msg and b'precision 0 (exact fp32) only' in msg
    msg = _refused(_cfg(2, 0, precision, adim=6, masks=6))
    assert b'arch 2 is built for precision 0 (exact fp32) only' in msg
    msg = _refused(_cfg(3, 0, precision, adim=12, masks=4, zdim=8))
    assert b'arch 3 is built for precision 0 (exact fp32) only' in msg


@pytest.mark.parametrize('precision', [3, -1])
def test_unknown_precision_names_the_three_valid_values(precision):
    msg = _refused(_cfg(0, 0, precision))
    assert b'precision must be 0 (fp32), 1 (split bf16) or 2 (plain bf16)' in msg


def test_abi_is_additive():
    lib = _lib.load_library()
    assert lib.vf_abi_version() == 7 == _lib.ABI_VERSION
    assert 'vf_debug_lstm_layer' in _lib.EXPORTS and hasattr(lib, 'vf_debug_lstm_layer')
    # the debug entry validates before it touches a device
    assert lib.vf_debug_lstm_layer(None, 0, 1, None, None, None, None, None, None) != 0
    assert b'null argument' in lib.vf_last_error()
