"""Child process of tests/test_gpu_frames_only.py: free device memory (``hipMemGetInfo``) around ``vf_create`` of a
frames-only engine and of the same engine with one designated pixel, in a process that has allocated nothing else.  Prints one
JSON line ``{"bytes": {"0": ..., "1": ...}, "distrib_bytes": ...}``."""
import ctypes
import json
import sys

import torch

from visual_foresight_amd import _lib


def main():
    H, W, T, B = (int(a) for a in sys.argv[1:5])
    lib = _lib.load_library()
    torch.cuda.init()
    torch.cuda.synchronize()
    used, handles = {}, []
    # the first vf_create of a process also loads the code object and sizes the kernels' LDS: spend that on a small engine
    warm, hw = _lib.VfConfig(32, 32, 4, 5, 1, 2, 3, 10, 1, 0, 0, 1, 1, 0, 0, 0), ctypes.c_void_p()
    _lib.check(lib.vf_create(ctypes.byref(warm), ctypes.byref(hw)))
    handles.append(hw)
    torch.cuda.synchronize()
    for nd in (0, 1):
        cfg = _lib.VfConfig(H, W, 4, 5, nd, 2, T + 2, 10, B, 0, 0, 1, 1, 0, 0, 0)
        h = ctypes.c_void_p()
        before = torch.cuda.mem_get_info(0)[0]
        _lib.check(lib.vf_create(ctypes.byref(cfg), ctypes.byref(h)))
        torch.cuda.synchronize()
        used[str(nd)] = before - torch.cuda.mem_get_info(0)[0]
        handles.append(h)
    for h in handles:
        _lib.check(lib.vf_destroy(h))
    print(json.dumps({'bytes': used, 'distrib_bytes': B * T * 1 * H * W * 4}))


if __name__ == '__main__':
    main()
