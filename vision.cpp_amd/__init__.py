"""MI355X-native backend for the visp:: Depth-Anything hot path.

The directory name contains a dot, so import it through `__graft_entry__.load_package()`
(registers it as module `visioncpp_amd`). Contents:
  csrc/      HIP kernels + C++ host code + the C ABI (built into lib/libvisioncpp.so)
  _lib.py    ctypes bindings of the C ABI (counterpart of the reference's
             bindings/python/visioncpp/_lib.py), derived from the two headers in include/
  _cdecl.py  the strict reader of those headers' declarations
  vision.py  Device / Model classes with the reference's Python API plus the batched extension
  gguf.py    GGUF v3 writer/reader (numpy)
  synth.py   synthetic checkpoints / inputs
"""
__all__ = ["gguf", "synth"]
