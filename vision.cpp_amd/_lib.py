"""ctypes bindings of the C ABI in lib/libvisioncpp.so, derived from include/visp_c_api.h and include/visp_hip_kernels.h.

The counterpart of the reference's bindings/python/visioncpp/_lib.py (:36-171): same structures, same
11 `visp_*` prototypes, plus the batched extension (include/visp_c_api.h part 2) and the
kernel-level `vx_*` launchers (include/visp_hip_kernels.h) that the parity tests drive. The structures,
enumerators and prototypes are not written down here: _cdecl.py reads them from the headers at import.
There is no fallback: if the library is missing or a symbol cannot be resolved this raises.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path

from . import _cdecl


class Error(Exception):
    pass


# the C ABI is declared once, in the two headers; everything below is derived from them
INCLUDE_DIR = Path(__file__).resolve().parent.parent / "include"
C_API_DECLS = _cdecl.parse((INCLUDE_DIR / "visp_c_api.h").read_text())
KERNEL_DECLS = _cdecl.parse((INCLUDE_DIR / "visp_hip_kernels.h").read_text())
C_API_SYMBOLS = list(C_API_DECLS.functions)
KERNEL_SYMBOLS = list(KERNEL_DECLS.functions)

STRUCT_NAMES = {
    "visp_image_view": "ImageView", "visp_depthany_info": "DepthAnyInfo", "visp_timing": "Timing", "visp_esrgan_info": "EsrganInfo",
    "visp_migan_info": "MiganInfo", "visp_detection": "Detection", "visp_yolov9t_nms_params": "Yolov9tNmsParams",
    "visp_yolov9t_info": "Yolov9tInfo", "vx_gemm_args": "GemmArgs", "vx_dconv_args": "DconvArgs", "vx_rcu_args": "RcuArgs",
    "vx_tile_layout": "TileLayout", "vx_deform_conv_args": "DeformConvArgs", "vx_dino_block_args": "DinoBlockArgs",
    "vx_gemm_fp8_args": "GemmFp8Args",
}
STRUCTS = {**_cdecl.structures(C_API_DECLS, STRUCT_NAMES), **_cdecl.structures(KERNEL_DECLS, STRUCT_NAMES)}  # by C name
assert set(STRUCTS) == set(STRUCT_NAMES), set(STRUCTS) ^ set(STRUCT_NAMES)
globals().update({cls.__name__: cls for cls in STRUCTS.values()})  # ImageView, GemmArgs, ...
# EPI_F16 ... EPI_SILU (enum vx_epilogue) and DC_F16, DC_RGB_F32, DC_HEAD_F32: the header's names without the VX_ prefix
globals().update({k.removeprefix("VX_"): v for values in KERNEL_DECLS.enums.values() for k, v in values.items()})

# VISP_LIBRARY selects another build of the same ABI (same-box A/B comparisons of kernel variants)
LIB_PATH = Path(os.environ["VISP_LIBRARY"]).resolve() if os.environ.get("VISP_LIBRARY") else Path(__file__).resolve().parent / "lib" / "libvisioncpp.so"


def init() -> ctypes.CDLL:
    if not LIB_PATH.exists():
        raise OSError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                      f"(make -C vision.cpp_amd/csrc). There is no CPU fallback.")
    lib = ctypes.CDLL(str(LIB_PATH))
    for name, function in (*C_API_DECLS.functions.items(), *KERNEL_DECLS.functions.items()):
        fn = getattr(lib, name)  # AttributeError if the build dropped a declared symbol
        fn.argtypes, fn.restype = _cdecl.prototype(function, STRUCTS)
    return lib


_lib: ctypes.CDLL | None = None


def get_lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        _lib = init()
    return _lib


def check(return_value: int):
    if return_value == 0:
        raise Error(get_lib().visp_get_last_error().decode())


def vx_check(return_value: int):
    if return_value == 0:
        raise Error(get_lib().vx_last_error().decode())


def path_to_char_p(p) -> bytes:
    return str(p).encode()
