"""
_device.py — what the GPU tests ask the device and the library's debug hooks, once.  Keyword-only where two integers could
be swapped.
"""
import ctypes as C

import torch

from pyroved_amd import _abi


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def kernel_name(*, fused, units, grads=1, lik=0):
    """the decoder kernel the library's size rule names for this many units of 16 rows (pv_debug_decoder_kernel_name)"""
    lib = _abi.lib()
    lib.pv_debug_decoder_kernel_name.restype = C.c_char_p
    lib.pv_debug_decoder_kernel_name.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int]
    return lib.pv_debug_decoder_kernel_name(fused, units, grads, lik).decode()


def last_fold_build():
    """the build the last guide-hosting decoder launch dispatched (pv_debug_w8_last_fold_build)"""
    lib = _abi.lib()
    lib.pv_debug_w8_last_fold_build.restype = C.c_int
    lib.pv_debug_w8_last_fold_build.argtypes = []
    return int(lib.pv_debug_w8_last_fold_build())
