"""sqeazy_amd -- MI355X-native drop-in for sqeazy's pipeline encode path.

The product is ``sqeazy_amd/lib/libsqeazy_amd.so`` (C-ABI in ``include/sqeazy_amd.h``, hand-written HIP
kernels for gfx950).  This module is only the ctypes binding used by the tests and ``bench.py``; it mirrors
the reference's C-ABI names (``src/cpp/inc/sqeazy.h``) one to one and adds thin numpy / device-pointer helpers.

There is no CPU fallback: if the library is missing, importing works but every call raises, and every encode
on a machine without a HIP device returns the reference's error code 1.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libsqeazy_amd.so")
_lib = None

EXPORTED_SYMBOLS = (
    "SQY_Header_Size", "SQY_Decompressed_NDims", "SQY_Decompressed_Shape", "SQY_Decompressed_Sizeof",
    "SQY_Version_Triple", "SQY_PipelineEncode_UI8", "SQY_PipelineEncode_UI16",
    "SQY_Pipeline_Max_Compressed_Length_UI8", "SQY_Pipeline_Max_Compressed_Length_UI16",
    "SQY_Pipeline_Max_Compressed_Length_3D_UI8", "SQY_Pipeline_Max_Compressed_Length_3D_UI16",
    "SQY_Pipeline_Possible_UI16", "SQY_Pipeline_Possible_UI8", "SQY_Pipeline_Possible",
    "SQY_Decompressed_Length", "SQY_Decode_UI16", "SQY_Decode_UI8",
    "SQYAMD_PipelineEncode_UI16_Device", "SQYAMD_PipelineEncode_UI8_Device",
    "SQYAMD_PipelineEncode_UI16_DeviceAt", "SQYAMD_PipelineEncode_UI8_DeviceAt",
    "SQYAMD_PipelineEncode_UI16_DeviceAt_Frames", "SQYAMD_PipelineEncode_UI8_DeviceAt_Frames",
    "SQYAMD_PipelineEncode_Slabs_UI16_Device", "SQYAMD_PipelineEncode_Slabs_UI8_Device",
    "SQYAMD_PipelineEncode_Batch_UI16_Device", "SQYAMD_PipelineEncode_Batch_UI8_Device", "SQYAMD_PipelineEncode_Batch_UI16", "SQYAMD_PipelineEncode_Batch_UI8",
    "SQYAMD_PipelineEncode_BatchStrided_UI16_Device", "SQYAMD_PipelineEncode_BatchStrided_UI8_Device",
    "SQYAMD_PipelineEncode_BatchPacked_UI16_Device", "SQYAMD_PipelineEncode_BatchPacked_UI8_Device",
    "SQYAMD_PipelineEncode_BatchPacked_UI16", "SQYAMD_PipelineEncode_BatchPacked_UI8",
    "SQYAMD_Decode_BatchStrided_UI16_Device", "SQYAMD_Decode_BatchStrided_UI8_Device",
    "SQYAMD_Decode_BatchWindow_UI16_Device", "SQYAMD_Decode_BatchWindow_UI8_Device",
    "SQYAMD_Update_BatchWindow_UI16_Device", "SQYAMD_Update_BatchWindow_UI8_Device", "SQYAMD_Update_Box_UI16_Device", "SQYAMD_Update_Box_UI8_Device",
    "SQYAMD_Update_Boxes_UI16_Device", "SQYAMD_Update_Boxes_UI8_Device", "SQYAMD_Update_Boxes_UI16", "SQYAMD_Update_Boxes_UI8",
    "SQYAMD_Compare_BatchWindow_UI16_Device", "SQYAMD_Compare_BatchWindow_UI8_Device",
    "SQYAMD_PipelineEncode_UI16_Cap", "SQYAMD_PipelineEncode_UI8_Cap",
    "SQYAMD_Decode_UI16_Device", "SQYAMD_Decode_UI8_Device",
    "SQYAMD_Decode_Frames_UI16_Device", "SQYAMD_Decode_Frames_UI8_Device", "SQYAMD_Decode_Frames_UI16", "SQYAMD_Decode_Frames_UI8",
    "SQYAMD_Decode_Box_UI16_Device", "SQYAMD_Decode_Box_UI8_Device", "SQYAMD_Decode_Box_UI16", "SQYAMD_Decode_Box_UI8",
    "SQYAMD_Decode_Boxes_UI16_Device", "SQYAMD_Decode_Boxes_UI8_Device", "SQYAMD_Decode_Boxes_UI16", "SQYAMD_Decode_Boxes_UI8",
    "SQYAMD_Compare_Boxes_UI16_Device", "SQYAMD_Compare_Boxes_UI8_Device", "SQYAMD_Compare_Boxes_UI16", "SQYAMD_Compare_Boxes_UI8",
    "SQYAMD_Project_Boxes_UI16_Device", "SQYAMD_Project_Boxes_UI8_Device", "SQYAMD_Project_Boxes_UI16", "SQYAMD_Project_Boxes_UI8",
    "SQYAMD_Bin_Boxes_UI16_Device", "SQYAMD_Bin_Boxes_UI8_Device", "SQYAMD_Bin_Boxes_UI16", "SQYAMD_Bin_Boxes_UI8",
    "SQYAMD_Pyramid_Boxes_UI16_Device", "SQYAMD_Pyramid_Boxes_UI8_Device", "SQYAMD_Pyramid_Boxes_UI16", "SQYAMD_Pyramid_Boxes_UI8",
    "SQYAMD_Histogram_Boxes_UI16_Device", "SQYAMD_Histogram_Boxes_UI8_Device", "SQYAMD_Histogram_Boxes_UI16", "SQYAMD_Histogram_Boxes_UI8",
    "SQYAMD_Decode_Slabs_UI16_Device", "SQYAMD_Decode_Slabs_UI8_Device", "SQYAMD_Decode_Slabs_UI16", "SQYAMD_Decode_Slabs_UI8",
    "SQYAMD_Decode_Batch_UI16_Device", "SQYAMD_Decode_Batch_UI8_Device", "SQYAMD_Decode_Batch_UI16", "SQYAMD_Decode_Batch_UI8",
    "SQYAMD_Profile_Enable", "SQYAMD_Profile_Reset", "SQYAMD_Profile_Get",
    "SQYAMD_Release_Workspace", "SQYAMD_Set_Option", "SQYAMD_Get_Option", "SQYAMD_Call_Stamps", "SQYAMD_Dedupe_Report", "SQYAMD_Version", "SQYAMD_Header_Pipeline", "SQYAMD_Header_Build",
    "SQYAMD_Comm_UniqueId", "SQYAMD_Comm_Init", "SQYAMD_Comm_Destroy", "SQYAMD_Gather_Blobs",
)


class LibraryMissing(RuntimeError):
    pass


def lib():
    """the loaded libsqeazy_amd.so; raises LibraryMissing when it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LibraryMissing("%s not built: run `python -m sqeazy_amd.build` (hipcc, gfx950)" % LIB_PATH)
        # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64.so.7.  When it is loaded first,
        # our DT_NEEDED libamdhip64.so.7 resolves to that same copy; loaded the other way round the process
        # ends up with two runtimes and the second one sees no device.  So bring torch's in first when torch
        # is installed (tests / bench use torch for device memory); plain C/C++ callers simply get /opt/rocm's.
        if os.environ.get("SQEAZY_AMD_NO_TORCH_PRELOAD", "0") != "1":
            try:
                import torch  # noqa: F401
            except Exception:
                pass
        L = ctypes.CDLL(LIB_PATH)
        c_long_p = ctypes.POINTER(ctypes.c_long)
        L.SQY_Pipeline_Possible_UI16.restype = ctypes.c_bool
        L.SQY_Pipeline_Possible_UI8.restype = ctypes.c_bool
        L.SQY_Pipeline_Possible.restype = ctypes.c_bool
        L.SQYAMD_Version.restype = ctypes.c_char_p
        L.SQYAMD_Set_Option.argtypes = [ctypes.c_char_p, ctypes.c_long]
        L.SQYAMD_Get_Option.argtypes = [ctypes.c_char_p]
        L.SQYAMD_Get_Option.restype = ctypes.c_long
        L.SQYAMD_Profile_Get.restype = ctypes.c_char_p
        L.SQYAMD_Profile_Get.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_double), c_long_p]
        for f in ("SQY_PipelineEncode_UI8", "SQY_PipelineEncode_UI16"):
            getattr(L, f).argtypes = [ctypes.c_char_p, ctypes.c_void_p, c_long_p, ctypes.c_uint, ctypes.c_void_p, c_long_p, ctypes.c_int]
        for f in ("SQYAMD_PipelineEncode_UI8_Device", "SQYAMD_PipelineEncode_UI16_Device"):
            getattr(L, f).argtypes = [ctypes.c_char_p, ctypes.c_void_p, c_long_p, ctypes.c_uint, ctypes.c_void_p, ctypes.c_long,
                                      c_long_p, ctypes.c_int, ctypes.c_void_p]
        for f in ("SQYAMD_PipelineEncode_UI8_DeviceAt", "SQYAMD_PipelineEncode_UI16_DeviceAt"):
            getattr(L, f).argtypes = [ctypes.c_char_p, ctypes.c_void_p, c_long_p, ctypes.c_uint, ctypes.c_void_p, ctypes.c_long,
                                      c_long_p, c_long_p, ctypes.c_int, ctypes.c_void_p]
        for f in ("SQYAMD_PipelineEncode_Slabs_UI8_Device", "SQYAMD_PipelineEncode_Slabs_UI16_Device"):
            getattr(L, f).argtypes = [ctypes.c_char_p, ctypes.c_void_p, c_long_p, ctypes.c_uint, ctypes.c_int, ctypes.c_void_p, ctypes.c_long,
                                      c_long_p, c_long_p, ctypes.c_int, ctypes.c_int]
        for f in ("SQYAMD_PipelineEncode_Batch_UI8_Device", "SQYAMD_PipelineEncode_Batch_UI16_Device"):
            getattr(L, f).argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p), c_long_p, ctypes.c_uint, ctypes.c_int, ctypes.c_void_p, ctypes.c_long,
                                      c_long_p, c_long_p, ctypes.c_int, ctypes.c_void_p]
        for f in ("SQYAMD_PipelineEncode_BatchStrided_UI8_Device", "SQYAMD_PipelineEncode_BatchStrided_UI16_Device"):
            getattr(L, f).argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p), c_long_p, c_long_p, ctypes.c_uint, ctypes.c_int, ctypes.c_void_p,
                                      ctypes.c_long, c_long_p, c_long_p, ctypes.c_int, ctypes.c_void_p]
        for f in ("SQYAMD_PipelineEncode_BatchPacked_UI8_Device", "SQYAMD_PipelineEncode_BatchPacked_UI16_Device"):
            getattr(L, f).argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p), c_long_p, c_long_p, ctypes.c_uint, ctypes.c_int, ctypes.c_void_p,
                                      ctypes.c_long, ctypes.c_long, c_long_p, c_long_p, c_long_p, ctypes.c_int, ctypes.c_void_p]
        for f in ("SQYAMD_PipelineEncode_BatchPacked_UI8", "SQYAMD_PipelineEncode_BatchPacked_UI16"):
            getattr(L, f).argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p), c_long_p, ctypes.c_uint, ctypes.c_int, ctypes.c_void_p, ctypes.c_long,
                                      ctypes.c_long, c_long_p, c_long_p, c_long_p, ctypes.c_int]
        for f in ("SQYAMD_Decode_BatchStrided_UI8_Device", "SQYAMD_Decode_BatchStrided_UI16_Device"):
            getattr(L, f).argtypes = [ctypes.c_void_p, c_long_p, c_long_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), c_long_p, c_long_p, ctypes.c_uint,
                                      c_long_p, ctypes.c_void_p]
        for f in ("SQYAMD_Decode_BatchWindow_UI8_Device", "SQYAMD_Decode_BatchWindow_UI16_Device"):
            getattr(L, f).argtypes = [ctypes.c_void_p, c_long_p, c_long_p, ctypes.c_int, c_long_p, ctypes.POINTER(ctypes.c_void_p), c_long_p, c_long_p,
                                      ctypes.c_uint, c_long_p, ctypes.c_void_p]
        for f in ("SQYAMD_Compare_BatchWindow_UI8_Device", "SQYAMD_Compare_BatchWindow_UI16_Device"):
            getattr(L, f).argtypes = [ctypes.c_void_p, c_long_p, c_long_p, ctypes.c_int, c_long_p, ctypes.POINTER(ctypes.c_void_p), c_long_p, c_long_p,
                                      ctypes.c_uint, ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_void_p]
        for f in ("SQYAMD_Update_BatchWindow_UI8_Device", "SQYAMD_Update_BatchWindow_UI16_Device"):
            getattr(L, f).argtypes = [ctypes.c_char_p, ctypes.c_void_p, c_long_p, c_long_p, ctypes.c_int, c_long_p, ctypes.POINTER(ctypes.c_void_p), c_long_p, c_long_p,
                                      ctypes.c_uint, ctypes.c_void_p, ctypes.c_long, c_long_p, c_long_p, ctypes.c_int, ctypes.c_void_p]
        for f in ("SQYAMD_Update_Box_UI8_Device", "SQYAMD_Update_Box_UI16_Device"):
            getattr(L, f).argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_long, c_long_p, ctypes.c_void_p, c_long_p, c_long_p, ctypes.c_uint, ctypes.c_void_p,
                                      ctypes.c_long, c_long_p, ctypes.c_int, ctypes.c_void_p]
        for f in ("SQYAMD_Update_Boxes_UI8_Device", "SQYAMD_Update_Boxes_UI16_Device"):
            getattr(L, f).argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_long, c_long_p, ctypes.POINTER(ctypes.c_void_p), c_long_p, c_long_p,
                                      ctypes.c_uint, ctypes.c_void_p, ctypes.c_long, c_long_p, ctypes.c_int, ctypes.c_void_p]
        for f in ("SQYAMD_Update_Boxes_UI8", "SQYAMD_Update_Boxes_UI16"):
            getattr(L, f).argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_long, c_long_p, c_long_p, ctypes.c_uint, ctypes.c_void_p, ctypes.c_long,
                                      ctypes.c_void_p, ctypes.c_long, c_long_p, ctypes.c_int]
        for f in ("SQYAMD_PipelineEncode_Batch_UI8", "SQYAMD_PipelineEncode_Batch_UI16"):
            getattr(L, f).argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p), c_long_p, ctypes.c_uint, ctypes.c_int, ctypes.c_void_p, ctypes.c_long,
                                      c_long_p, c_long_p, ctypes.c_int]
        for f in ("SQYAMD_PipelineEncode_UI8_Cap", "SQYAMD_PipelineEncode_UI16_Cap"):
            getattr(L, f).argtypes = [ctypes.c_char_p, ctypes.c_void_p, c_long_p, ctypes.c_uint, ctypes.c_void_p, ctypes.c_long, c_long_p,
                                      ctypes.c_int]
        for f in ("SQY_Decode_UI8", "SQY_Decode_UI16"):
            getattr(L, f).argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_int]
        for f in ("SQYAMD_Decode_UI8_Device", "SQYAMD_Decode_UI16_Device"):
            getattr(L, f).argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p]
        for f in ("SQYAMD_Decode_Frames_UI8_Device", "SQYAMD_Decode_Frames_UI16_Device"):
            getattr(L, f).argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p]
        for f in ("SQYAMD_Decode_Frames_UI8", "SQYAMD_Decode_Frames_UI16"):
            getattr(L, f).argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_void_p, ctypes.c_long]
        for f in ("SQYAMD_Decode_Box_UI8_Device", "SQYAMD_Decode_Box_UI16_Device"):
            getattr(L, f).argtypes = [ctypes.c_void_p, ctypes.c_long, c_long_p, ctypes.c_void_p, c_long_p, c_long_p, ctypes.c_uint, ctypes.c_void_p]
        for f in ("SQYAMD_Decode_Box_UI8", "SQYAMD_Decode_Box_UI16"):
            getattr(L, f).argtypes = [ctypes.c_void_p, ctypes.c_long, c_long_p, c_long_p, ctypes.c_uint, ctypes.c_void_p, ctypes.c_long]
        for f in ("SQYAMD_Decode_Boxes_UI8_Device", "SQYAMD_Decode_Boxes_UI16_Device"):
            getattr(L, f).argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_long, c_long_p, ctypes.POINTER(ctypes.c_void_p), c_long_p, c_long_p, ctypes.c_uint,
                                      ctypes.c_void_p]
        for f in ("SQYAMD_Decode_Boxes_UI8", "SQYAMD_Decode_Boxes_UI16"):
            getattr(L, f).argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_long, c_long_p, c_long_p, ctypes.c_uint, ctypes.c_void_p, ctypes.c_long]
        for f in ("SQYAMD_Compare_Boxes_UI8_Device", "SQYAMD_Compare_Boxes_UI16_Device"):
            getattr(L, f).argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_long, c_long_p, ctypes.POINTER(ctypes.c_void_p), c_long_p, c_long_p, ctypes.c_uint,
                                      ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_void_p]
        for f in ("SQYAMD_Compare_Boxes_UI8", "SQYAMD_Compare_Boxes_UI16"):
            getattr(L, f).argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_long, c_long_p, c_long_p, ctypes.c_uint, ctypes.c_void_p, ctypes.c_long,
                                      ctypes.POINTER(ctypes.c_ulonglong)]
        for f in ("SQYAMD_Project_Boxes_UI8_Device", "SQYAMD_Project_Boxes_UI16_Device"):
            getattr(L, f).argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_long, c_long_p, c_long_p, ctypes.c_uint, ctypes.c_int, ctypes.c_int,
                                      ctypes.POINTER(ctypes.c_void_p), c_long_p, ctypes.c_void_p]
        for f in ("SQYAMD_Project_Boxes_UI8", "SQYAMD_Project_Boxes_UI16"):
            getattr(L, f).argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_long, c_long_p, c_long_p, ctypes.c_uint, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                      ctypes.c_long]
        for f in ("SQYAMD_Bin_Boxes_UI8_Device", "SQYAMD_Bin_Boxes_UI16_Device"):
            getattr(L, f).argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_long, c_long_p, c_long_p, ctypes.c_uint, c_long_p, ctypes.c_int,
                                      ctypes.POINTER(ctypes.c_void_p), c_long_p, ctypes.c_void_p]
        for f in ("SQYAMD_Bin_Boxes_UI8", "SQYAMD_Bin_Boxes_UI16"):
            getattr(L, f).argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_long, c_long_p, c_long_p, ctypes.c_uint, c_long_p, ctypes.c_int, ctypes.c_void_p,
                                      ctypes.c_long]
        for f in ("SQYAMD_Pyramid_Boxes_UI8_Device", "SQYAMD_Pyramid_Boxes_UI16_Device"):
            getattr(L, f).argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_long, c_long_p, c_long_p, ctypes.c_uint, ctypes.c_long, c_long_p, ctypes.c_int,
                                      ctypes.POINTER(ctypes.c_void_p), c_long_p, ctypes.c_void_p]
        for f in ("SQYAMD_Pyramid_Boxes_UI8", "SQYAMD_Pyramid_Boxes_UI16"):
            getattr(L, f).argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_long, c_long_p, c_long_p, ctypes.c_uint, ctypes.c_long, c_long_p, ctypes.c_int,
                                      ctypes.c_void_p, ctypes.c_long]
        for f in ("SQYAMD_Histogram_Boxes_UI8_Device", "SQYAMD_Histogram_Boxes_UI16_Device"):
            getattr(L, f).argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_long, c_long_p, c_long_p, ctypes.c_uint, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                                      ctypes.c_void_p]
        for f in ("SQYAMD_Histogram_Boxes_UI8", "SQYAMD_Histogram_Boxes_UI16"):
            getattr(L, f).argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_long, c_long_p, c_long_p, ctypes.c_uint, ctypes.c_int, ctypes.c_void_p, ctypes.c_long]
        for f in ("SQYAMD_Decode_Slabs_UI8_Device", "SQYAMD_Decode_Slabs_UI16_Device"):
            getattr(L, f).argtypes = [ctypes.c_void_p, c_long_p, c_long_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_long, c_long_p, ctypes.c_int,
                                      ctypes.c_void_p]
        for f in ("SQYAMD_Decode_Slabs_UI8", "SQYAMD_Decode_Slabs_UI16"):
            getattr(L, f).argtypes = [ctypes.c_void_p, c_long_p, c_long_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_long, c_long_p]
        for f in ("SQYAMD_Decode_Batch_UI8_Device", "SQYAMD_Decode_Batch_UI16_Device"):
            getattr(L, f).argtypes = [ctypes.c_void_p, c_long_p, c_long_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), c_long_p, c_long_p, ctypes.c_void_p]
        for f in ("SQYAMD_Decode_Batch_UI8", "SQYAMD_Decode_Batch_UI16"):
            getattr(L, f).argtypes = [ctypes.c_void_p, c_long_p, c_long_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), c_long_p, c_long_p]
        _lib = L
    return _lib


def _suffix(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.uint16:
        return "UI16"
    if dtype == np.uint8:
        return "UI8"
    raise TypeError("sqeazy pipelines take uint8 or uint16 voxels, got %s" % dtype)


def _longs(values):
    return (ctypes.c_long * len(values))(*[int(v) for v in values])


def version_triple():
    v = (ctypes.c_int * 3)()
    lib().SQY_Version_Triple(v)
    return tuple(v)


def pipeline_possible(pipeline, dtype=np.uint16):
    return bool(getattr(lib(), "SQY_Pipeline_Possible_" + _suffix(dtype))(pipeline.encode()))


def max_compressed_length(pipeline, shape, dtype=np.uint16):
    """SQY_Pipeline_Max_Compressed_Length_3D_*: note the in/out convention (*length in = strlen(pipeline))."""
    p = pipeline.encode()
    length = ctypes.c_long(len(p))
    rc = getattr(lib(), "SQY_Pipeline_Max_Compressed_Length_3D_" + _suffix(dtype))(p, _longs(shape), ctypes.c_uint(len(shape)),
                                                                                  ctypes.byref(length))
    if rc:
        raise ValueError("SQY_Pipeline_Max_Compressed_Length_3D returned %d for %r" % (rc, pipeline))
    return length.value


def max_compressed_length_bytes(pipeline, nbytes, dtype=np.uint16):
    p = pipeline.encode()
    length = ctypes.c_long(int(nbytes))
    rc = getattr(lib(), "SQY_Pipeline_Max_Compressed_Length_" + _suffix(dtype))(p, ctypes.c_long(len(p)), ctypes.byref(length))
    if rc:
        raise ValueError("SQY_Pipeline_Max_Compressed_Length returned %d for %r" % (rc, pipeline))
    return length.value


def encode(pipeline, volume, nthreads=0, extra_capacity=None):
    """SQY_PipelineEncode_UI8/UI16 on a host ndarray ({z,y,x}); returns (return code, blob bytes or None).

    With extra_capacity=None this is the reference protocol: dst holds exactly SQY_Pipeline_Max_Compressed_Length_3D
    bytes.  With a number, dst is that much larger and the explicit-capacity entry point is used."""
    vol = np.ascontiguousarray(volume)
    sfx = _suffix(vol.dtype)
    if not pipeline_possible(pipeline, vol.dtype):
        cap = 64
    else:
        cap = max(max_compressed_length(pipeline, vol.shape, vol.dtype), 64)
    dlen = ctypes.c_long(0)
    if extra_capacity is None:
        dst = np.empty(cap, dtype=np.uint8)
        rc = getattr(lib(), "SQY_PipelineEncode_" + sfx)(pipeline.encode(), vol.ctypes.data, _longs(vol.shape), ctypes.c_uint(vol.ndim),
                                                        dst.ctypes.data, ctypes.byref(dlen), ctypes.c_int(nthreads))
    else:
        cap += int(extra_capacity)
        dst = np.empty(cap, dtype=np.uint8)
        rc = getattr(lib(), "SQYAMD_PipelineEncode_%s_Cap" % sfx)(pipeline.encode(), vol.ctypes.data, _longs(vol.shape),
                                                                 ctypes.c_uint(vol.ndim), dst.ctypes.data, ctypes.c_long(cap),
                                                                 ctypes.byref(dlen), ctypes.c_int(nthreads))
    if rc:
        return rc, None
    return 0, dst[:dlen.value].tobytes()


def encode_device(pipeline, d_src, shape, dtype, d_dst, dst_capacity, nthreads=0, stream=None):
    """SQYAMD_PipelineEncode_*_Device on raw device pointers (ints); returns (rc, bytes written)."""
    sfx = _suffix(dtype)
    dlen = ctypes.c_long(0)
    rc = getattr(lib(), "SQYAMD_PipelineEncode_%s_Device" % sfx)(
        pipeline.encode(), ctypes.c_void_p(int(d_src)), _longs(shape), ctypes.c_uint(len(shape)), ctypes.c_void_p(int(d_dst)),
        ctypes.c_long(int(dst_capacity)), ctypes.byref(dlen), ctypes.c_int(nthreads), ctypes.c_void_p(stream or 0))
    return rc, dlen.value


def encode_device_at(pipeline, d_src, shape, dtype, d_dst, dst_capacity, nthreads=0, stream=None):
    """SQYAMD_PipelineEncode_*_DeviceAt: the blob may start anywhere inside the destination; returns (rc, offset, bytes)."""
    sfx = _suffix(dtype)
    dlen, doff = ctypes.c_long(0), ctypes.c_long(0)
    rc = getattr(lib(), "SQYAMD_PipelineEncode_%s_DeviceAt" % sfx)(
        pipeline.encode(), ctypes.c_void_p(int(d_src)), _longs(shape), ctypes.c_uint(len(shape)), ctypes.c_void_p(int(d_dst)),
        ctypes.c_long(int(dst_capacity)), ctypes.byref(doff), ctypes.byref(dlen), ctypes.c_int(nthreads), ctypes.c_void_p(stream or 0))
    return rc, doff.value, dlen.value


def encode_device_at_frames(pipeline, d_src, shape, dtype, d_dst, dst_capacity, every, nthreads=0, stream=None):
    """SQYAMD_PipelineEncode_*_DeviceAt_Frames: returns (rc, offset, bytes, frame_offsets) -- frame_offsets[i] = start of LZ4
    frame i * every relative to the blob start, the last entry is the blob length."""
    nvox = 1
    for d in shape:
        nvox *= int(d)
    max_entries = nvox * np.dtype(dtype).itemsize // (64 << 10) // max(int(every), 1) + 4
    fo = (ctypes.c_long * max_entries)()
    cnt = ctypes.c_int(0)
    dlen, doff = ctypes.c_long(0), ctypes.c_long(0)
    rc = getattr(lib(), "SQYAMD_PipelineEncode_%s_DeviceAt_Frames" % _suffix(dtype))(
        ctypes.c_char_p(pipeline.encode()), ctypes.c_void_p(int(d_src)), _longs(shape), ctypes.c_uint(len(shape)), ctypes.c_void_p(int(d_dst)),
        ctypes.c_long(int(dst_capacity)), ctypes.byref(doff), ctypes.byref(dlen), ctypes.c_int(nthreads), ctypes.c_void_p(stream or 0),
        ctypes.c_int(int(every)), fo, ctypes.c_int(max_entries), ctypes.byref(cnt))
    return rc, doff.value, dlen.value, list(fo[:cnt.value + 1])


def encode_slabs_device(pipeline, d_src, shape, dtype, nslabs, d_dst, slab_capacity, nthreads=0, inflight=3):
    """SQYAMD_PipelineEncode_Slabs_*_Device: a whole volume as nslabs z-slab blobs with one call; returns (rc, offsets, lengths)."""
    offs = (ctypes.c_long * nslabs)()
    lens = (ctypes.c_long * nslabs)()
    rc = getattr(lib(), "SQYAMD_PipelineEncode_Slabs_%s_Device" % _suffix(dtype))(
        pipeline.encode(), ctypes.c_void_p(int(d_src)), _longs(shape), ctypes.c_uint(len(shape)), ctypes.c_int(nslabs),
        ctypes.c_void_p(int(d_dst)), ctypes.c_long(int(slab_capacity)), offs, lens, ctypes.c_int(nthreads), ctypes.c_int(inflight))
    return rc, list(offs), list(lens)


def encode_batch_device(pipeline, d_srcs, shapes, dtype, d_dst, slot_capacity, nthreads=0, stream=None):
    """SQYAMD_PipelineEncode_Batch_*_Device: volume i ({z,y,x} = shapes[i]) at device pointer d_srcs[i] becomes a blob inside slot i of d_dst
    (slot_capacity bytes each); returns (rc, offsets, lengths), offsets relative to d_dst."""
    n = len(d_srcs)
    rank = len(shapes[0]) if n else 0
    ptrs = (ctypes.c_void_p * max(n, 1))(*[int(p) for p in d_srcs])
    flat = _longs([x for s in shapes for x in s]) if n else None
    offs = (ctypes.c_long * max(n, 1))()
    lens = (ctypes.c_long * max(n, 1))()
    rc = getattr(lib(), "SQYAMD_PipelineEncode_Batch_%s_Device" % _suffix(dtype))(
        pipeline.encode(), ptrs, flat, ctypes.c_uint(rank), ctypes.c_int(n), ctypes.c_void_p(int(d_dst)), ctypes.c_long(int(slot_capacity)), offs, lens,
        ctypes.c_int(nthreads), ctypes.c_void_p(stream or 0))
    return rc, list(offs[:n]), list(lens[:n])


def encode_batch_strided_device(pipeline, d_srcs, shapes, strides, dtype, d_dst, slot_capacity, nthreads=0, stream=None):
    """SQYAMD_PipelineEncode_BatchStrided_*_Device: encode_batch_device for views -- volume i is the strided view at device pointer d_srcs[i]
    with shape shapes[i] and strides[i] in VOXELS (outermost first, the innermost 1; strides None: dense volumes).  Returns (rc, offsets,
    lengths), offsets relative to d_dst."""
    n = len(d_srcs)
    rank = len(shapes[0]) if n else 0
    ptrs = (ctypes.c_void_p * max(n, 1))(*[int(p) for p in d_srcs])
    flat = _longs([x for s in shapes for x in s]) if n else None
    flat_strides = _longs([x for s in strides for x in s]) if n and strides is not None else None
    offs = (ctypes.c_long * max(n, 1))()
    lens = (ctypes.c_long * max(n, 1))()
    rc = getattr(lib(), "SQYAMD_PipelineEncode_BatchStrided_%s_Device" % _suffix(dtype))(
        pipeline.encode(), ptrs, flat, flat_strides, ctypes.c_uint(rank), ctypes.c_int(n), ctypes.c_void_p(int(d_dst)), ctypes.c_long(int(slot_capacity)),
        offs, lens, ctypes.c_int(nthreads), ctypes.c_void_p(stream or 0))
    return rc, list(offs[:n]), list(lens[:n])


def encode_batch_packed_device(pipeline, d_srcs, shapes, strides, dtype, d_dst, dst_capacity, align=1, nthreads=0, stream=None):
    """SQYAMD_PipelineEncode_BatchPacked_*_Device: encode_batch_strided_device (strides None: dense volumes) with the blobs back to back in
    the dst_capacity bytes at d_dst -- offsets[0] = 0, offsets[i + 1] = offsets[i] + lengths[i] rounded up to align (a power of two up to
    65536), total = offsets[-1] + lengths[-1].  Returns (rc, offsets, lengths, total); rc 1 with zeroed tables and total > 0: the blobs do
    not fit, total is the capacity a retry needs."""
    n = len(d_srcs)
    rank = len(shapes[0]) if n else 0
    ptrs = (ctypes.c_void_p * max(n, 1))(*[int(p) for p in d_srcs])
    flat = _longs([x for s in shapes for x in s]) if n else None
    flat_strides = _longs([x for s in strides for x in s]) if n and strides is not None else None
    offs = (ctypes.c_long * max(n, 1))()
    lens = (ctypes.c_long * max(n, 1))()
    total = ctypes.c_long(0)
    rc = getattr(lib(), "SQYAMD_PipelineEncode_BatchPacked_%s_Device" % _suffix(dtype))(
        pipeline.encode(), ptrs, flat, flat_strides, ctypes.c_uint(rank), ctypes.c_int(n), ctypes.c_void_p(int(d_dst)), ctypes.c_long(int(dst_capacity)),
        ctypes.c_long(int(align)), offs, lens, ctypes.byref(total), ctypes.c_int(nthreads), ctypes.c_void_p(stream or 0))
    return rc, list(offs[:n]), list(lens[:n]), total.value


def tile_views(base_ptr, shape, tile, itemsize):
    """The regular grid of tiles of a dense volume of `shape` at device pointer base_ptr (itemsize bytes a voxel), as views for
    encode_batch_strided_device / decode_batch_strided_device: returns (ptrs, shapes, strides), tiles in row-major grid order, the tiles
    at the high ends smaller where `tile` does not divide `shape`.  Strides are in voxels."""
    shape, tile = [int(x) for x in shape], [int(x) for x in tile]
    if len(shape) != len(tile) or not 1 <= len(shape) <= 3 or min(shape + tile) < 1:
        raise ValueError("tile_views: shape and tile of one rank (1 to 3), positive extents")
    strides = [1] * len(shape)
    for k in range(len(shape) - 2, -1, -1):
        strides[k] = strides[k + 1] * shape[k + 1]
    ptrs, shapes = [], []
    starts = [[]]
    for k in range(len(shape)):
        starts = [s + [o] for s in starts for o in range(0, shape[k], tile[k])]
    for s in starts:
        ptrs.append(int(base_ptr) + sum(o * st for o, st in zip(s, strides)) * int(itemsize))
        shapes.append(tuple(min(t, d - o) for o, t, d in zip(s, tile, shape)))
    return ptrs, shapes, [tuple(strides)] * len(ptrs)


def encode_batch(pipeline, volumes, nthreads=0):
    """SQYAMD_PipelineEncode_Batch_UI8/UI16 on host ndarrays of one dtype and rank (shapes may differ); returns the list of blobs (bytes).
    Raises ValueError when the call returns non-zero."""
    vols = [np.ascontiguousarray(v) for v in volumes]
    if not vols:
        raise ValueError("encode_batch: no volumes")
    dtype, rank = vols[0].dtype, vols[0].ndim
    if any(v.dtype != dtype or v.ndim != rank for v in vols):
        raise TypeError("encode_batch takes volumes of one dtype and rank")
    n = len(vols)
    cap = max(max(max_compressed_length(pipeline, v.shape, dtype), 64) for v in vols) if pipeline_possible(pipeline, dtype) else 64
    dst = np.empty(n * cap, dtype=np.uint8)
    ptrs = (ctypes.c_void_p * n)(*[v.ctypes.data for v in vols])
    offs = (ctypes.c_long * n)()
    lens = (ctypes.c_long * n)()
    rc = getattr(lib(), "SQYAMD_PipelineEncode_Batch_" + _suffix(dtype))(
        pipeline.encode(), ptrs, _longs([x for v in vols for x in v.shape]), ctypes.c_uint(rank), ctypes.c_int(n), dst.ctypes.data, ctypes.c_long(cap),
        offs, lens, ctypes.c_int(nthreads))
    if rc:
        raise ValueError("SQYAMD_PipelineEncode_Batch returned %d for %r" % (rc, pipeline))
    return [dst[offs[i]:offs[i] + lens[i]].tobytes() for i in range(n)]


def encode_batch_packed(pipeline, volumes, align=1, nthreads=0):
    """SQYAMD_PipelineEncode_BatchPacked_UI8/UI16 on host ndarrays of one dtype and rank (shapes may differ); returns (buffer, offsets, lengths):
    the blobs back to back in `buffer` (bytes, exactly the call's total; for align > 1 zeros between the blobs), blob i =
    buffer[offsets[i]:offsets[i] + lengths[i]].  Raises ValueError when the call returns non-zero."""
    vols = [np.ascontiguousarray(v) for v in volumes]
    if not vols:
        raise ValueError("encode_batch_packed: no volumes")
    dtype, rank = vols[0].dtype, vols[0].ndim
    if any(v.dtype != dtype or v.ndim != rank for v in vols):
        raise TypeError("encode_batch_packed takes volumes of one dtype and rank")
    n, align = len(vols), int(align)
    # (the capacity that needs no retry; a bad align is the call's to refuse)
    step = align if align >= 1 else 1
    cap = sum(-(-max(max_compressed_length(pipeline, v.shape, dtype), 64) // step) * step for v in vols) if pipeline_possible(pipeline, dtype) else 64
    dst = np.empty(cap, dtype=np.uint8)
    ptrs = (ctypes.c_void_p * n)(*[v.ctypes.data for v in vols])
    offs = (ctypes.c_long * n)()
    lens = (ctypes.c_long * n)()
    total = ctypes.c_long(0)
    rc = getattr(lib(), "SQYAMD_PipelineEncode_BatchPacked_" + _suffix(dtype))(
        pipeline.encode(), ptrs, _longs([x for v in vols for x in v.shape]), ctypes.c_uint(rank), ctypes.c_int(n), dst.ctypes.data, ctypes.c_long(cap),
        ctypes.c_long(align), offs, lens, ctypes.byref(total), ctypes.c_int(nthreads))
    if rc:
        raise ValueError("SQYAMD_PipelineEncode_BatchPacked returned %d for %r" % (rc, pipeline))
    return dst[:total.value].tobytes(), list(offs), list(lens)


def header_size(blob):
    n = ctypes.c_long(len(blob))
    lib().SQY_Header_Size(bytes(blob), ctypes.byref(n))
    return n.value


def decompressed_length(blob):
    n = ctypes.c_long(len(blob))
    lib().SQY_Decompressed_Length(bytes(blob), ctypes.byref(n))
    return n.value


def decompressed_ndims(blob):
    n = ctypes.c_long(len(blob))
    lib().SQY_Decompressed_NDims(bytes(blob), ctypes.byref(n))
    return n.value


def decompressed_shape(blob):
    nd = decompressed_ndims(blob)
    arr = (ctypes.c_long * max(nd, 1))()
    arr[0] = len(blob)
    lib().SQY_Decompressed_Shape(bytes(blob), arr)
    return tuple(arr[i] for i in range(nd))


def decompressed_sizeof(blob):
    n = ctypes.c_long(len(blob))
    lib().SQY_Decompressed_Sizeof(bytes(blob), ctypes.byref(n))
    return n.value


def decode(blob, nthreads=0):
    """SQY_Decode_UI8/UI16; returns (rc, ndarray or None)."""
    blob = bytes(blob)
    size = decompressed_sizeof(blob)
    shape = decompressed_shape(blob)
    if size not in (1, 2) or not shape:
        return 1, None
    dtype = np.uint16 if size == 2 else np.uint8
    out = np.empty(shape, dtype=dtype)
    src = np.frombuffer(blob, dtype=np.uint8)
    rc = getattr(lib(), "SQY_Decode_" + _suffix(dtype))(src.ctypes.data, ctypes.c_long(len(blob)), out.ctypes.data, ctypes.c_int(nthreads))
    return (rc, None) if rc else (0, out)


def decode_frames(blob, z0, nz):
    """SQYAMD_Decode_Frames_UI8/UI16: frames [z0, z0 + nz) of the blob (along shape[0]); returns (rc, ndarray or None)."""
    blob = bytes(blob)
    size = decompressed_sizeof(blob)
    shape = decompressed_shape(blob)
    if size not in (1, 2) or not shape:
        return 1, None
    dtype = np.uint16 if size == 2 else np.uint8
    out = np.empty((max(int(nz), 0),) + tuple(shape[1:]), dtype=dtype)
    src = np.frombuffer(blob, dtype=np.uint8)
    rc = getattr(lib(), "SQYAMD_Decode_Frames_" + _suffix(dtype))(src.ctypes.data, ctypes.c_long(len(blob)), ctypes.c_long(int(z0)),
                                                                  ctypes.c_long(int(nz)), out.ctypes.data, ctypes.c_long(out.nbytes))
    return (rc, None) if rc else (0, out)


def decode_frames_device(d_src, srclength, z0, nz, d_dst, dst_capacity, dtype, stream=None):
    """SQYAMD_Decode_Frames_*_Device on raw device pointers (ints); returns rc."""
    return getattr(lib(), "SQYAMD_Decode_Frames_%s_Device" % _suffix(dtype))(
        ctypes.c_void_p(int(d_src)), ctypes.c_long(int(srclength)), ctypes.c_long(int(z0)), ctypes.c_long(int(nz)), ctypes.c_void_p(int(d_dst)),
        ctypes.c_long(int(dst_capacity)), ctypes.c_void_p(stream or 0))


def decode_box(blob, origin, extent):
    """SQYAMD_Decode_Box_UI8/UI16: the box [origin, origin + extent) of the blob's volume; returns (rc, ndarray of shape extent or None)."""
    blob = bytes(blob)
    size = decompressed_sizeof(blob)
    if size not in (1, 2) or not decompressed_shape(blob):
        return 1, None
    dtype = np.uint16 if size == 2 else np.uint8
    out = np.empty(tuple(max(int(e), 0) for e in extent), dtype=dtype)
    src = np.frombuffer(blob, dtype=np.uint8)
    rc = getattr(lib(), "SQYAMD_Decode_Box_" + _suffix(dtype))(src.ctypes.data, ctypes.c_long(len(blob)), _longs(origin), _longs(extent), ctypes.c_uint(len(extent)),
                                                               out.ctypes.data, ctypes.c_long(out.nbytes))
    return (rc, None) if rc else (0, out)


def decode_box_device(d_src, srclength, origin, d_dst, shape, strides, dtype, stream=None):
    """SQYAMD_Decode_Box_*_Device on raw device pointers (ints): the box of extent `shape` that begins at voxel `origin` of the blob, into the
    view at d_dst with that shape and `strides` in voxels (None: dense); only the view's voxels are written.  Returns rc."""
    return getattr(lib(), "SQYAMD_Decode_Box_%s_Device" % _suffix(dtype))(
        ctypes.c_void_p(None if d_src is None else int(d_src)), ctypes.c_long(int(srclength)), None if origin is None else _longs(origin),
        ctypes.c_void_p(None if d_dst is None else int(d_dst)), None if shape is None else _longs(shape), None if strides is None else _longs(strides),
        ctypes.c_uint(len(shape) if shape is not None else len(origin or ())), ctypes.c_void_p(stream or 0))


def _long_rows(rows):
    """rows of longs, row after row (None stays None)"""
    return None if rows is None else _longs([int(v) for row in rows for v in row])


def decode_boxes(blob, origins, extents):
    """SQYAMD_Decode_Boxes_UI8/UI16: the boxes [origins[i], origins[i] + extents[i]) of the blob's volume with one call; returns
    (rc, [ndarray of shape extents[i], ..] or None)."""
    blob = bytes(blob)
    size = decompressed_sizeof(blob)
    if size not in (1, 2) or not decompressed_shape(blob) or len(origins) != len(extents) or not len(extents):
        return 1, None
    dtype = np.uint16 if size == 2 else np.uint8
    rank = len(extents[0])
    shapes = [tuple(max(int(e), 0) for e in ext) for ext in extents]
    counts = [int(np.prod(sh, dtype=np.int64)) for sh in shapes]
    out = np.empty(sum(counts), dtype=dtype)
    src = np.frombuffer(blob, dtype=np.uint8)
    rc = getattr(lib(), "SQYAMD_Decode_Boxes_" + _suffix(dtype))(src.ctypes.data, ctypes.c_long(len(blob)), ctypes.c_long(len(extents)), _long_rows(origins),
                                                                 _long_rows(extents), ctypes.c_uint(rank), out.ctypes.data, ctypes.c_long(out.nbytes))
    if rc:
        return rc, None
    ends = np.cumsum(counts)
    return 0, [out[e - c:e].reshape(sh) for e, c, sh in zip(ends, counts, shapes)]


def decode_boxes_device(d_src, srclength, origins, d_dsts, shapes, strides, dtype, stream=None, count=None):
    """SQYAMD_Decode_Boxes_*_Device on raw device pointers (ints): box i of extent shapes[i] that begins at voxel origins[i] of the blob, into
    the view at d_dsts[i] with that shape and strides[i] in voxels (strides None: every view dense); only the views' voxels are written.
    count: the number of boxes (default: as many as there are shapes).  Returns rc."""
    n = len(shapes) if shapes is not None else len(origins or ())
    first = (shapes or origins or [()])[0] if n else ()
    ptrs = None if d_dsts is None else (ctypes.c_void_p * max(len(d_dsts), 1))(*[None if p is None else int(p) for p in d_dsts])
    return getattr(lib(), "SQYAMD_Decode_Boxes_%s_Device" % _suffix(dtype))(
        ctypes.c_void_p(None if d_src is None else int(d_src)), ctypes.c_long(int(srclength)), ctypes.c_long(n if count is None else int(count)), _long_rows(origins),
        ptrs, _long_rows(shapes), _long_rows(strides), ctypes.c_uint(len(first)), ctypes.c_void_p(stream or 0))


def decode_slabs_device(d_src, offsets, lengths, d_dst, dst_capacity, dtype, inflight=0, stream=None):
    """SQYAMD_Decode_Slabs_*_Device: blob i at d_src + offsets[i] (lengths[i] bytes), the volume they make to d_dst; returns (rc, frames)."""
    n = len(offsets)
    frames = (ctypes.c_long * max(n, 1))()
    rc = getattr(lib(), "SQYAMD_Decode_Slabs_%s_Device" % _suffix(dtype))(
        ctypes.c_void_p(int(d_src)), _longs(offsets) if n else None, _longs(lengths) if n else None, ctypes.c_int(n), ctypes.c_void_p(int(d_dst)),
        ctypes.c_long(int(dst_capacity)), frames, ctypes.c_int(int(inflight)), ctypes.c_void_p(stream or 0))
    return rc, list(frames[:n])


def decode_slabs_packed(buf, offsets, lengths):
    """SQYAMD_Decode_Slabs_UI8/UI16 on blobs that lie in `buf` (bytes) at offsets[i], lengths[i] bytes; returns (rc, ndarray or None)"""
    buf = bytes(buf)
    if not offsets:
        return 1, None
    first = buf[offsets[0]:offsets[0] + lengths[0]]
    size, shape = decompressed_sizeof(first), decompressed_shape(first)
    if size not in (1, 2) or not shape:
        return 1, None
    dtype = np.uint16 if size == 2 else np.uint8
    Z = 0
    for o, n in zip(offsets, lengths):
        s = decompressed_shape(buf[o:o + n])
        if tuple(s[1:]) != tuple(shape[1:]):
            return 1, None
        Z += s[0]
    out = np.empty((Z,) + tuple(shape[1:]), dtype=dtype)
    src = np.frombuffer(buf, dtype=np.uint8)
    frames = (ctypes.c_long * len(offsets))()
    rc = getattr(lib(), "SQYAMD_Decode_Slabs_" + _suffix(dtype))(src.ctypes.data, _longs(offsets), _longs(lengths), ctypes.c_int(len(offsets)),
                                                                 out.ctypes.data, ctypes.c_long(out.nbytes), frames)
    return (rc, None) if rc else (0, out)


def decode_slabs(blobs):
    """SQYAMD_Decode_Slabs_UI8/UI16: z-slab blobs (a list of byte strings), packed back to back; returns (rc, volume ndarray or None)"""
    blobs = [bytes(b) for b in blobs]
    offsets, at = [], 0
    for b in blobs:
        offsets.append(at)
        at += len(b)
    return decode_slabs_packed(b"".join(blobs), offsets, [len(b) for b in blobs])


def decode_batch_device(d_src, offsets, lengths, d_dsts, dst_capacities, dtype, stream=None):
    """SQYAMD_Decode_Batch_*_Device: blob i at d_src + offsets[i] (lengths[i] bytes) into the device pointer d_dsts[i] (dst_capacities[i] bytes);
    returns (rc, decoded_bytes).  The offsets and lengths of encode_batch_device can be passed straight through."""
    n = len(offsets)
    ptrs = (ctypes.c_void_p * max(n, 1))(*[int(p) for p in d_dsts])
    decoded = (ctypes.c_long * max(n, 1))()
    rc = getattr(lib(), "SQYAMD_Decode_Batch_%s_Device" % _suffix(dtype))(
        ctypes.c_void_p(int(d_src)), _longs(offsets) if n else None, _longs(lengths) if n else None, ctypes.c_int(n), ptrs,
        _longs(dst_capacities) if n else None, decoded, ctypes.c_void_p(stream or 0))
    return rc, list(decoded[:n])


def decode_batch_strided_device(d_src, offsets, lengths, d_dsts, shapes, strides, dtype, stream=None):
    """SQYAMD_Decode_BatchStrided_*_Device: blob i at d_src + offsets[i] (lengths[i] bytes) into the strided view at device pointer d_dsts[i]
    with shape shapes[i] (the blob's own) and strides[i] in voxels (None: dense); only the view's voxels are written.  Returns (rc,
    decoded_bytes).  The offsets and lengths of encode_batch_strided_device can be passed straight through."""
    n = len(offsets)
    rank = len(shapes[0]) if n else 0
    ptrs = (ctypes.c_void_p * max(n, 1))(*[int(p) for p in d_dsts])
    decoded = (ctypes.c_long * max(n, 1))()
    rc = getattr(lib(), "SQYAMD_Decode_BatchStrided_%s_Device" % _suffix(dtype))(
        ctypes.c_void_p(int(d_src)), _longs(offsets) if n else None, _longs(lengths) if n else None, ctypes.c_int(n), ptrs,
        _longs([x for s in shapes for x in s]) if n else None, _longs([x for s in strides for x in s]) if n and strides is not None else None,
        ctypes.c_uint(rank), decoded, ctypes.c_void_p(stream or 0))
    return rc, list(decoded[:n])


def decode_batch_window_device(d_src, offsets, lengths, origins, d_dsts, shapes, strides, dtype, stream=None):
    """SQYAMD_Decode_BatchWindow_*_Device: of blob i at d_src + offsets[i] (lengths[i] bytes) the window that begins at its voxel origins[i]
    (None: every window at its blob's first voxel) and has the extent shapes[i], into the strided view at device pointer d_dsts[i] with
    that shape and strides[i] in voxels (None: dense); only the view's voxels are written.  Returns (rc, decoded_bytes)."""
    n = len(offsets)
    rank = len(shapes[0]) if n else 0
    ptrs = (ctypes.c_void_p * max(n, 1))(*[p if p is None else int(p) for p in d_dsts])
    decoded = (ctypes.c_long * max(n, 1))()
    rc = getattr(lib(), "SQYAMD_Decode_BatchWindow_%s_Device" % _suffix(dtype))(
        ctypes.c_void_p(int(d_src)), _longs(offsets) if n else None, _longs(lengths) if n else None, ctypes.c_int(n),
        _longs([x for o in origins for x in o]) if n and origins is not None else None, ptrs, _longs([x for s in shapes for x in s]) if n else None,
        _longs([x for s in strides for x in s]) if n and strides is not None else None, ctypes.c_uint(rank), decoded, ctypes.c_void_p(stream or 0))
    return rc, list(decoded[:n])


COMPARE_FIELDS = ("voxels", "ndiff", "sum_abs", "sum_sq", "max_abs", "view_sum", "view_min", "view_max")      # SQYAMD_COMPARE_* in index order


def compare_batch_window_device(d_src, offsets, lengths, origins, d_views, shapes, strides, dtype, stream=None):
    """SQYAMD_Compare_BatchWindow_*_Device: the window of blob i of decode_batch_window_device compared with the strided view at device
    pointer d_views[i] (shape shapes[i], strides[i] in voxels; None: dense); the views are read, nothing is written.  Returns (rc, stats):
    stats an (n, 8) uint64 array, row i the exact integers COMPARE_FIELDS of window i (a: the decoded voxel, b: the view's).  box_windows
    makes the table."""
    n = len(offsets)
    rank = len(shapes[0]) if n else 0
    ptrs = (ctypes.c_void_p * max(n, 1))(*[p if p is None else int(p) for p in d_views])
    stats = np.zeros((n, len(COMPARE_FIELDS)), dtype=np.uint64)
    rc = getattr(lib(), "SQYAMD_Compare_BatchWindow_%s_Device" % _suffix(dtype))(
        ctypes.c_void_p(int(d_src)), _longs(offsets) if n else None, _longs(lengths) if n else None, ctypes.c_int(n),
        _longs([x for o in origins for x in o]) if n and origins is not None else None, ptrs, _longs([x for s in shapes for x in s]) if n else None,
        _longs([x for s in strides for x in s]) if n and strides is not None else None, ctypes.c_uint(rank),
        stats.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)) if n else None, ctypes.c_void_p(stream or 0))
    return rc, stats


def compare_metrics(row, dtype):
    """The metrics of the reference's `sqy compare` from one row of compare_batch_window_device's stats, the view being the original side:
    mse = sum_sq / voxels, rms = sqrt(mse), nrmse = rms / (view_max - view_min), mnmse = rms / (view_sum / voxels), l1norm = sum_abs,
    l2norm = sum_sq, psnr = 20 log10(type max) - 10 log10(mse), drange = view_max - view_min.  float64 on the exact integers; a zero
    denominator or a zero mse gives inf / nan as numpy does."""
    f = dict(zip(COMPARE_FIELDS, (np.float64(int(x)) for x in row)))
    with np.errstate(divide="ignore", invalid="ignore"):
        mse = f["sum_sq"] / f["voxels"]
        rms = np.sqrt(mse)
        drange = f["view_max"] - f["view_min"]
        return {"mse": mse, "rms": rms, "nrmse": rms / drange, "mnmse": rms / (f["view_sum"] / f["voxels"]), "l1norm": f["sum_abs"], "l2norm": f["sum_sq"],
                "psnr": np.float64(20.0) * np.log10(np.float64(np.iinfo(np.dtype(dtype)).max)) - np.float64(10.0) * np.log10(mse), "drange": drange}


def compare_boxes_device(d_src, srclength, origins, d_views, shapes, strides, dtype, stream=None, count=None):
    """SQYAMD_Compare_Boxes_*_Device on raw device pointers (ints): box i of extent shapes[i] that begins at voxel origins[i] of the ONE blob
    at d_src, compared with the view at d_views[i] with that shape and strides[i] in voxels (strides None: every view dense); the views are
    read, nothing is written.  count: the number of boxes (default: as many as there are shapes).  Returns (rc, stats): stats a (count, 8)
    uint64 array, row i the exact integers COMPARE_FIELDS of box i (a: the decoded voxel, b: the view's); compare_metrics takes a row."""
    n = len(shapes) if shapes is not None else len(origins or ())
    first = (shapes or origins or [()])[0] if n else ()
    ptrs = None if d_views is None else (ctypes.c_void_p * max(len(d_views), 1))(*[None if p is None else int(p) for p in d_views])
    k = n if count is None else int(count)
    stats = np.zeros((k if 0 < k < 2 ** 31 else 0, len(COMPARE_FIELDS)), dtype=np.uint64)      # (no rows: stats NULL, which the call refuses)
    rc = getattr(lib(), "SQYAMD_Compare_Boxes_%s_Device" % _suffix(dtype))(
        ctypes.c_void_p(None if d_src is None else int(d_src)), ctypes.c_long(int(srclength)), ctypes.c_long(n if count is None else int(count)), _long_rows(origins),
        ptrs, _long_rows(shapes), _long_rows(strides), ctypes.c_uint(len(first)),
        stats.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)) if stats.size else None, ctypes.c_void_p(stream or 0))
    return rc, stats


def compare_boxes(blob, origins, views):
    """SQYAMD_Compare_Boxes_UI8/UI16: the boxes of the blob's volume that begin at origins[i] and have the shape of the ndarray views[i],
    compared with those arrays with one call; returns (rc, stats) as compare_boxes_device."""
    blob = bytes(blob)
    size = decompressed_sizeof(blob)
    n = len(views)
    stats = np.zeros((n, len(COMPARE_FIELDS)), dtype=np.uint64)
    if size not in (1, 2) or not decompressed_shape(blob) or len(origins) != n or not n:
        return 1, stats
    dtype = np.uint16 if size == 2 else np.uint8
    dense = np.concatenate([np.ascontiguousarray(v, dtype=dtype).reshape(-1) for v in views])
    src = np.frombuffer(blob, dtype=np.uint8)
    rc = getattr(lib(), "SQYAMD_Compare_Boxes_" + _suffix(dtype))(
        src.ctypes.data, ctypes.c_long(len(blob)), ctypes.c_long(n), _long_rows(origins), _long_rows([np.shape(v) for v in views]), ctypes.c_uint(np.ndim(views[0])),
        dense.ctypes.data, ctypes.c_long(dense.nbytes), stats.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)))
    return rc, stats


PROJECT_MAX, PROJECT_MIN, PROJECT_SUM = 0, 1, 2
_PROJECT_OPS = {"max": PROJECT_MAX, "min": PROJECT_MIN, "sum": PROJECT_SUM}


def _project_op(op):
    """the op as SQYAMD_PROJECT_*: a name ("max", "min", "sum") or the constant itself"""
    return _PROJECT_OPS[op] if isinstance(op, str) else int(op)


def project_boxes_device(d_src, srclength, origins, extents, axis, op, d_outs, out_strides, dtype, stream=None, count=None):
    """SQYAMD_Project_Boxes_*_Device on raw device pointers (ints): box i of extent extents[i] that begins at voxel origins[i] of the ONE blob
    at d_src, projected along `axis` with op ("max", "min", "sum" or PROJECT_*) into the uint32 image at d_outs[i], whose shape is the
    extent with `axis` removed and whose pitches in elements are out_strides[i] (None: every image dense).  count: the number of boxes
    (default: as many as there are extents).  Returns rc."""
    n = len(extents) if extents is not None else len(origins or ())
    first = (extents or origins or [()])[0] if n else ()
    ptrs = None if d_outs is None else (ctypes.c_void_p * max(len(d_outs), 1))(*[None if p is None else int(p) for p in d_outs])
    strides = None if out_strides is None or len(first) < 2 else _long_rows(out_strides)
    return getattr(lib(), "SQYAMD_Project_Boxes_%s_Device" % _suffix(dtype))(
        ctypes.c_void_p(None if d_src is None else int(d_src)), ctypes.c_long(int(srclength)), ctypes.c_long(n if count is None else int(count)), _long_rows(origins),
        _long_rows(extents), ctypes.c_uint(len(first)), ctypes.c_int(int(axis)), ctypes.c_int(_project_op(op)), ptrs, strides, ctypes.c_void_p(stream or 0))


def project_boxes(blob, origins, extents, axis, op="max"):
    """SQYAMD_Project_Boxes_UI8/UI16: the boxes [origins[i], origins[i] + extents[i]) of the blob's volume projected along `axis` with one
    call; op "max", "min", "sum" (or PROJECT_*) gives uint32 images, "mean" the sum divided by extents[i][axis] in float64.  Returns
    (rc, [ndarray of the extent with `axis` removed, ..] or None)."""
    blob = bytes(blob)
    size = decompressed_sizeof(blob)
    if size not in (1, 2) or not decompressed_shape(blob) or len(origins) != len(extents) or not len(extents):
        return 1, None
    mean = op == "mean"
    code = PROJECT_SUM if mean else _project_op(op)
    dtype = np.uint16 if size == 2 else np.uint8
    rank = len(extents[0])
    if not 0 <= int(axis) < rank:
        return 1, None
    shapes = [tuple(max(int(e), 0) for k, e in enumerate(ext) if k != int(axis)) for ext in extents]
    counts = [int(np.prod(sh, dtype=np.int64)) for sh in shapes]
    out = np.empty(sum(counts), dtype=np.uint32)
    src = np.frombuffer(blob, dtype=np.uint8)
    rc = getattr(lib(), "SQYAMD_Project_Boxes_" + _suffix(dtype))(src.ctypes.data, ctypes.c_long(len(blob)), ctypes.c_long(len(extents)), _long_rows(origins),
                                                                  _long_rows(extents), ctypes.c_uint(rank), ctypes.c_int(int(axis)), ctypes.c_int(code),
                                                                  out.ctypes.data, ctypes.c_long(out.nbytes))
    if rc:
        return rc, None
    ends = np.cumsum(counts)
    images = [out[e - c:e].reshape(sh) for e, c, sh in zip(ends, counts, shapes)]
    if mean:
        images = [im.astype(np.float64) / np.float64(int(ext[int(axis)])) for im, ext in zip(images, extents)]
    return 0, images


def bin_boxes_device(d_src, srclength, origins, extents, bins, op, d_outs, out_strides, dtype, stream=None, count=None):
    """SQYAMD_Bin_Boxes_*_Device on raw device pointers (ints): box i of extent extents[i] that begins at voxel origins[i] of the ONE blob at
    d_src, read at a coarser resolution -- cells of `bins` voxels (one entry per dimension, the same for all boxes) reduced with op ("max",
    "min", "sum" or PROJECT_*) -- into the uint32 output at d_outs[i], whose shape is ceil(extents[i] / bins) and whose pitches in elements
    are out_strides[i] (None: every output dense).  count: the number of boxes (default: as many as there are extents).  Returns rc."""
    n = len(extents) if extents is not None else len(origins or ())
    first = (extents or origins or [()])[0] if n else ()
    ptrs = None if d_outs is None else (ctypes.c_void_p * max(len(d_outs), 1))(*[None if p is None else int(p) for p in d_outs])
    return getattr(lib(), "SQYAMD_Bin_Boxes_%s_Device" % _suffix(dtype))(
        ctypes.c_void_p(None if d_src is None else int(d_src)), ctypes.c_long(int(srclength)), ctypes.c_long(n if count is None else int(count)), _long_rows(origins),
        _long_rows(extents), ctypes.c_uint(len(first)), None if bins is None else _long_rows([bins]), ctypes.c_int(_project_op(op)), ptrs,
        None if out_strides is None else _long_rows(out_strides), ctypes.c_void_p(stream or 0))


def bin_shape(extent, bins):
    """the shape of a box's binned output: ceil(extent / bins) per dimension"""
    return tuple(-(-max(int(e), 0) // max(int(b), 1)) for e, b in zip(extent, bins))


def bin_counts(extent, bins):
    """the number of voxels in every cell of a box's binned output (partial cells at the far edges hold fewer), as float64"""
    n = np.ones((), np.float64)
    for e, b in zip(extent, bins):
        e, b = int(e), min(int(b), int(e))
        edge = np.minimum(np.arange(b, e + b, b), e) - np.arange(0, e, b)
        n = np.multiply.outer(n, edge.astype(np.float64))
    return n


def bin_boxes(blob, origins, extents, bins, op="max"):
    """SQYAMD_Bin_Boxes_UI8/UI16: the boxes [origins[i], origins[i] + extents[i]) of the blob's volume read at a coarser resolution with one
    call; op "max", "min", "sum" (or PROJECT_*) gives uint32 arrays, "mean" the sum divided by each cell's actual voxel count in float64 (a
    partial cell by fewer).  Returns (rc, [ndarray of shape ceil(extents[i] / bins), ..] or None)."""
    blob = bytes(blob)
    size = decompressed_sizeof(blob)
    if size not in (1, 2) or not decompressed_shape(blob) or len(origins) != len(extents) or not len(extents):
        return 1, None
    mean = op == "mean"
    code = PROJECT_SUM if mean else _project_op(op)
    dtype = np.uint16 if size == 2 else np.uint8
    rank = len(extents[0])
    if bins is None or len(bins) != rank or any(int(b) < 1 for b in bins):
        return 1, None
    shapes = [bin_shape(ext, bins) for ext in extents]
    counts = [int(np.prod(sh, dtype=np.int64)) for sh in shapes]
    out = np.empty(sum(counts), dtype=np.uint32)
    src = np.frombuffer(blob, dtype=np.uint8)
    rc = getattr(lib(), "SQYAMD_Bin_Boxes_" + _suffix(dtype))(src.ctypes.data, ctypes.c_long(len(blob)), ctypes.c_long(len(extents)), _long_rows(origins),
                                                              _long_rows(extents), ctypes.c_uint(rank), _long_rows([bins]), ctypes.c_int(code), out.ctypes.data,
                                                              ctypes.c_long(out.nbytes))
    if rc:
        return rc, None
    ends = np.cumsum(counts)
    cells = [out[e - c:e].reshape(sh) for e, c, sh in zip(ends, counts, shapes)]
    if mean:
        cells = [a.astype(np.float64) / bin_counts(ext, bins) for a, ext in zip(cells, extents)]
    return 0, cells


def histogram_bins(dtype, shift):
    """the number of bins of a histogram of SQYAMD_Histogram_Boxes_*: 65536 >> shift for 16-bit voxels, 256 >> shift for 8-bit ones"""
    bits = 8 * np.dtype(dtype).itemsize
    if bits not in (8, 16) or not 0 <= int(shift) < bits:
        raise ValueError("shift %r out of range for %s" % (shift, np.dtype(dtype)))
    return (1 << bits) >> int(shift)


def histogram_boxes_device(d_src, srclength, origins, extents, shift, d_hists, dtype, stream=None, count=None):
    """SQYAMD_Histogram_Boxes_*_Device on raw device pointers (ints): the voxels of box i -- extent extents[i], first voxel origins[i] of the
    ONE blob at d_src -- counted into the histogram at d_hists[i]: histogram_bins(dtype, shift) uint32 counters, voxel v in bin v >> shift.
    count: the number of boxes (default: as many as there are extents).  Returns rc."""
    n = len(extents) if extents is not None else len(origins or ())
    first = (extents or origins or [()])[0] if n else ()
    ptrs = None if d_hists is None else (ctypes.c_void_p * max(len(d_hists), 1))(*[None if p is None else int(p) for p in d_hists])
    return getattr(lib(), "SQYAMD_Histogram_Boxes_%s_Device" % _suffix(dtype))(
        ctypes.c_void_p(None if d_src is None else int(d_src)), ctypes.c_long(int(srclength)), ctypes.c_long(n if count is None else int(count)), _long_rows(origins),
        _long_rows(extents), ctypes.c_uint(len(first)), ctypes.c_int(int(shift)), ptrs, ctypes.c_void_p(stream or 0))


def histogram_boxes(blob, origins, extents, shift=0):
    """SQYAMD_Histogram_Boxes_UI8/UI16: the intensity histograms of the boxes [origins[i], origins[i] + extents[i]) of the blob's volume with
    one call, voxel v in bin v >> shift.  Returns (rc, [uint32 ndarray of histogram_bins(dtype, shift) counters, ..] or None)."""
    blob = bytes(blob)
    size = decompressed_sizeof(blob)
    if size not in (1, 2) or not decompressed_shape(blob) or len(origins) != len(extents) or not len(extents) or not 0 <= int(shift) < 8 * size:
        return 1, None
    dtype = np.uint16 if size == 2 else np.uint8
    nbins = histogram_bins(dtype, shift)
    out = np.empty(len(extents) * nbins, dtype=np.uint32)
    src = np.frombuffer(blob, dtype=np.uint8)
    rc = getattr(lib(), "SQYAMD_Histogram_Boxes_" + _suffix(dtype))(src.ctypes.data, ctypes.c_long(len(blob)), ctypes.c_long(len(extents)), _long_rows(origins),
                                                                    _long_rows(extents), ctypes.c_uint(len(extents[0])), ctypes.c_int(int(shift)), out.ctypes.data,
                                                                    ctypes.c_long(out.nbytes))
    if rc:
        return rc, None
    return 0, [out[i * nbins:(i + 1) * nbins] for i in range(len(extents))]


def histogram_quantile(hist, q, shift=0):
    """The nearest-rank quantile of a histogram of SQYAMD_Histogram_Boxes_*: the lower edge b << shift of the smallest bin b whose cumulative
    count reaches max(1, ceil(q N)), N the histogram's total.  ValueError for an empty histogram or q outside [0, 1]."""
    hist = np.asarray(hist)
    if not 0.0 <= q <= 1.0:
        raise ValueError("q outside [0, 1]")
    cum = np.cumsum(hist.astype(np.uint64))
    total = int(cum[-1]) if cum.size else 0
    if total == 0:
        raise ValueError("empty histogram")
    rank = max(1, int(np.ceil(q * total)))
    return int(np.searchsorted(cum, rank, side="left")) << int(shift)


def pyramid_boxes_device(d_src, srclength, origins, extents, bins_per_level, op, d_outs, out_strides, dtype, stream=None, count=None, levels=None):
    """SQYAMD_Pyramid_Boxes_*_Device on raw device pointers (ints): bin_boxes_device at every row of bins_per_level (one row of bins per
    level, the rows nesting) with one call.  d_outs[i][l] is the uint32 output of level l of box i, out_strides[i][l] its pitches in
    elements (None: every output dense).  count: the number of boxes, levels: the number of rows (defaults: as given).  Returns rc."""
    n = len(extents) if extents is not None else len(origins or ())
    first = (extents or origins or [()])[0] if n else ()
    nlev = len(bins_per_level) if bins_per_level is not None else 0
    flat = None if d_outs is None else [p for row in d_outs for p in row]
    ptrs = None if flat is None else (ctypes.c_void_p * max(len(flat), 1))(*[None if p is None else int(p) for p in flat])
    return getattr(lib(), "SQYAMD_Pyramid_Boxes_%s_Device" % _suffix(dtype))(
        ctypes.c_void_p(None if d_src is None else int(d_src)), ctypes.c_long(int(srclength)), ctypes.c_long(n if count is None else int(count)), _long_rows(origins),
        _long_rows(extents), ctypes.c_uint(len(first)), ctypes.c_long(nlev if levels is None else int(levels)), None if not nlev else _long_rows(bins_per_level),
        ctypes.c_int(_project_op(op)), ptrs, None if out_strides is None else _long_rows([s for row in out_strides for s in row]), ctypes.c_void_p(stream or 0))


def pyramid_boxes(blob, origins, extents, bins_per_level, op="max"):
    """SQYAMD_Pyramid_Boxes_UI8/UI16: the boxes [origins[i], origins[i] + extents[i]) of the blob's volume read at every resolution of
    bins_per_level (rows of bins, each a whole multiple of the row before per dimension) with one call; op as for bin_boxes, "mean" the
    sum divided by each cell's actual voxel count in float64.  Returns (rc, [[level arrays] per box] or None)."""
    blob = bytes(blob)
    size = decompressed_sizeof(blob)
    if size not in (1, 2) or not decompressed_shape(blob) or len(origins) != len(extents) or not len(extents):
        return 1, None
    mean = op == "mean"
    code = PROJECT_SUM if mean else _project_op(op)
    dtype = np.uint16 if size == 2 else np.uint8
    rank = len(extents[0])
    if not bins_per_level or any(len(row) != rank or any(int(b) < 1 for b in row) for row in bins_per_level):
        return 1, None
    shapes = [bin_shape(ext, row) for ext in extents for row in bins_per_level]
    counts = [int(np.prod(sh, dtype=np.int64)) for sh in shapes]
    out = np.empty(sum(counts), dtype=np.uint32)
    src = np.frombuffer(blob, dtype=np.uint8)
    rc = getattr(lib(), "SQYAMD_Pyramid_Boxes_" + _suffix(dtype))(src.ctypes.data, ctypes.c_long(len(blob)), ctypes.c_long(len(extents)), _long_rows(origins),
                                                                  _long_rows(extents), ctypes.c_uint(rank), ctypes.c_long(len(bins_per_level)),
                                                                  _long_rows(bins_per_level), ctypes.c_int(code), out.ctypes.data, ctypes.c_long(out.nbytes))
    if rc:
        return rc, None
    ends = np.cumsum(counts)
    cells = [out[e - c:e].reshape(sh) for e, c, sh in zip(ends, counts, shapes)]
    nlev = len(bins_per_level)
    if mean:
        cells = [a.astype(np.float64) / bin_counts(extents[k // nlev], bins_per_level[k % nlev]) for k, a in enumerate(cells)]
    return 0, [cells[i * nlev:(i + 1) * nlev] for i in range(len(extents))]


def update_batch_window_device(pipeline, d_src, offsets, lengths, origins, d_wins, shapes, strides, dtype, d_dst, slot_capacity, nthreads=0, stream=None):
    """SQYAMD_Update_BatchWindow_*_Device: old blob i at d_src + offsets[i] (lengths[i] bytes) is decoded, the window that begins at its voxel
    origins[i] (None: at its first voxel) and has the extent shapes[i] is replaced by the strided view at device pointer d_wins[i] with
    that shape and strides[i] in voxels (None: dense), and the result encoded with `pipeline` into slot i of d_dst (slot_capacity bytes
    each) -- byte for byte the single call's blob.  Returns (rc, offsets, lengths), offsets relative to d_dst."""
    n = len(offsets)
    rank = len(shapes[0]) if n else 0
    ptrs = (ctypes.c_void_p * max(n, 1))(*[p if p is None else int(p) for p in d_wins])
    offs = (ctypes.c_long * max(n, 1))()
    lens = (ctypes.c_long * max(n, 1))()
    rc = getattr(lib(), "SQYAMD_Update_BatchWindow_%s_Device" % _suffix(dtype))(
        pipeline.encode(), ctypes.c_void_p(int(d_src)), _longs(offsets) if n else None, _longs(lengths) if n else None, ctypes.c_int(n),
        _longs([x for o in origins for x in o]) if n and origins is not None else None, ptrs, _longs([x for s in shapes for x in s]) if n else None,
        _longs([x for s in strides for x in s]) if n and strides is not None else None, ctypes.c_uint(rank), ctypes.c_void_p(int(d_dst)),
        ctypes.c_long(int(slot_capacity)), offs, lens, ctypes.c_int(nthreads), ctypes.c_void_p(stream or 0))
    return rc, list(offs[:n]), list(lens[:n])


def update_box_device(pipeline, d_src, srclength, origin, d_view, shape, strides, dtype, d_dst, dst_capacity, nthreads=0, stream=None):
    """SQYAMD_Update_Box_*_Device on raw device pointers (ints): the old blob at d_src (srclength bytes) with the box of extent `shape` that
    begins at voxel `origin` replaced by the view at d_view with that shape and `strides` in voxels (None: dense), encoded with `pipeline`
    into d_dst (dst_capacity bytes) -- byte for byte the single call's blob of the pasted volume.  Returns (rc, dstlength); rc 1 with a
    dstlength above 0: the bytes a retry needs."""
    n = ctypes.c_long(0)
    rc = getattr(lib(), "SQYAMD_Update_Box_%s_Device" % _suffix(dtype))(
        None if pipeline is None else pipeline.encode(), ctypes.c_void_p(None if d_src is None else int(d_src)), ctypes.c_long(int(srclength)),
        None if origin is None else _longs(origin), ctypes.c_void_p(None if d_view is None else int(d_view)), None if shape is None else _longs(shape),
        None if strides is None else _longs(strides), ctypes.c_uint(len(shape) if shape is not None else len(origin or ())),
        ctypes.c_void_p(None if d_dst is None else int(d_dst)), ctypes.c_long(int(dst_capacity)), ctypes.byref(n), ctypes.c_int(nthreads), ctypes.c_void_p(stream or 0))
    return rc, n.value


def update_boxes_device(pipeline, d_src, srclength, origins, d_views, shapes, strides, dtype, d_dst, dst_capacity, nthreads=0, stream=None, count=None):
    """SQYAMD_Update_Boxes_*_Device on raw device pointers (ints): the old blob at d_src with box 0, then box 1, .. replaced by their views --
    box i of extent shapes[i] begins at voxel origins[i], its new voxels are the view at d_views[i] with strides[i] in voxels (strides
    None: every view dense); where boxes overlap the one with the higher index holds.  The new blob goes to d_dst (dst_capacity bytes),
    byte for byte what a chain of update_box_device calls gives.  count: the number of boxes (default: as many as there are shapes).
    Returns (rc, dstlength); rc 1 with a dstlength above 0: the bytes a retry needs."""
    k = len(shapes) if shapes is not None else len(origins or ())
    first = (shapes or origins or [()])[0] if k else ()
    ptrs = None if d_views is None else (ctypes.c_void_p * max(len(d_views), 1))(*[None if p is None else int(p) for p in d_views])
    n = ctypes.c_long(0)
    rc = getattr(lib(), "SQYAMD_Update_Boxes_%s_Device" % _suffix(dtype))(
        None if pipeline is None else pipeline.encode(), ctypes.c_void_p(None if d_src is None else int(d_src)), ctypes.c_long(int(srclength)),
        ctypes.c_long(k if count is None else int(count)), _long_rows(origins), ptrs, _long_rows(shapes), _long_rows(strides), ctypes.c_uint(len(first)),
        ctypes.c_void_p(None if d_dst is None else int(d_dst)), ctypes.c_long(int(dst_capacity)), ctypes.byref(n), ctypes.c_int(nthreads), ctypes.c_void_p(stream or 0))
    return rc, n.value


def update_boxes(pipeline, blob, origins, views, nthreads=0):
    """SQYAMD_Update_Boxes_UI8/UI16: the blob (bytes) with the boxes that begin at origins[i] and have the shape of the ndarray views[i]
    replaced by those arrays, in box order, with one call; returns (rc, new blob as bytes or None)."""
    blob = bytes(blob)
    size, shape = decompressed_sizeof(blob), decompressed_shape(blob)
    n = len(views)
    if size not in (1, 2) or not shape or len(origins) != n or not n:
        return 1, None
    dtype = np.uint16 if size == 2 else np.uint8
    dense = np.concatenate([np.ascontiguousarray(v, dtype=dtype).reshape(-1) for v in views])
    src = np.frombuffer(blob, dtype=np.uint8)
    out = np.empty(max_compressed_length(pipeline, shape, dtype), dtype=np.uint8)
    got = ctypes.c_long(0)
    rc = getattr(lib(), "SQYAMD_Update_Boxes_" + _suffix(dtype))(
        pipeline.encode(), src.ctypes.data, ctypes.c_long(len(blob)), ctypes.c_long(n), _long_rows(origins), _long_rows([np.shape(v) for v in views]),
        ctypes.c_uint(np.ndim(views[0])), dense.ctypes.data, ctypes.c_long(dense.nbytes), out.ctypes.data, ctypes.c_long(out.nbytes), ctypes.byref(got), ctypes.c_int(nthreads))
    return (rc, None) if rc else (0, out[:got.value].tobytes())


def box_windows(shape, tile, box_origin, box_extent, dst_ptr, dst_strides, itemsize):
    """The read of the box [box_origin, box_origin + box_extent) of a parent of `shape` that is stored as the blobs of tile_views(.., shape,
    tile, ..) in that grid order, as the arguments of decode_batch_window_device: returns (tile_indices, origins, ptrs, shapes, strides) --
    the tiles the box intersects in ascending index order and for each one the window inside the tile (origin, shape) and the view that
    takes it inside a box buffer whose first voxel is at device pointer dst_ptr (ptr; strides = dst_strides, in voxels; None: a dense box).
    The same table serves update_batch_window_device, the write of the box: the views then hold the tiles' new voxels.
    Pure Python.  ValueError: ranks that differ, a rank outside 1 to 3, a non-positive extent, a box outside the parent."""
    shape, tile, o, e = ([int(x) for x in v] for v in (shape, tile, box_origin, box_extent))
    rank = len(shape)
    if not 1 <= rank <= 3 or any(len(v) != rank for v in (tile, o, e)) or (dst_strides is not None and len(dst_strides) != rank):
        raise ValueError("box_windows: shape, tile, box and strides of one rank (1 to 3)")
    if min(shape + tile + e) < 1:
        raise ValueError("box_windows: positive extents")
    if any(o[k] < 0 or o[k] + e[k] > shape[k] for k in range(rank)):
        raise ValueError("box_windows: the box lies outside the parent")
    if dst_strides is None:
        strides = [1] * rank
        for k in range(rank - 2, -1, -1):
            strides[k] = strides[k + 1] * e[k + 1]
    else:
        strides = [int(x) for x in dst_strides]
    grid = [(shape[k] + tile[k] - 1) // tile[k] for k in range(rank)]
    cells = [[]]                                                    # the grid cells the box reaches, row-major: ascending tile index
    for k in range(rank):
        cells = [c + [t] for c in cells for t in range(o[k] // tile[k], (o[k] + e[k] - 1) // tile[k] + 1)]
    indices, origins, ptrs, shapes = [], [], [], []
    for c in cells:
        index = 0
        for k in range(rank):
            index = index * grid[k] + c[k]
        lo = [max(o[k], c[k] * tile[k]) for k in range(rank)]       # the part of the box in this tile, parent coordinates
        hi = [min(o[k] + e[k], (c[k] + 1) * tile[k]) for k in range(rank)]
        indices.append(index)
        origins.append(tuple(lo[k] - c[k] * tile[k] for k in range(rank)))
        shapes.append(tuple(hi[k] - lo[k] for k in range(rank)))
        ptrs.append(int(dst_ptr) + sum((lo[k] - o[k]) * strides[k] for k in range(rank)) * int(itemsize))
    return indices, origins, ptrs, shapes, [tuple(strides)] * len(indices)


def decode_batch(blobs):
    """SQYAMD_Decode_Batch_UI8/UI16 on blobs of one voxel type (a list of byte strings; shapes and pipelines may differ): the counterpart of
    encode_batch.  Returns the list of volumes (ndarrays); raises ValueError when the call returns non-zero."""
    blobs = [bytes(b) for b in blobs]
    if not blobs:
        raise ValueError("decode_batch: no blobs")
    size = decompressed_sizeof(blobs[0])
    if size not in (1, 2):
        raise ValueError("decode_batch: blob 0 holds no 8- or 16-bit voxels")
    dtype = np.uint16 if size == 2 else np.uint8
    outs = []
    for i, b in enumerate(blobs):
        shape = decompressed_shape(b)
        if decompressed_sizeof(b) != size or not shape:
            raise ValueError("decode_batch: blob %d has another voxel type or no shape" % i)
        outs.append(np.empty(shape, dtype=dtype))
    offsets, at = [], 0
    for b in blobs:
        offsets.append(at)
        at += len(b)
    src = np.frombuffer(b"".join(blobs), dtype=np.uint8)
    n = len(blobs)
    ptrs = (ctypes.c_void_p * n)(*[o.ctypes.data for o in outs])
    decoded = (ctypes.c_long * n)()
    rc = getattr(lib(), "SQYAMD_Decode_Batch_" + _suffix(dtype))(src.ctypes.data, _longs(offsets), _longs([len(b) for b in blobs]), ctypes.c_int(n), ptrs,
                                                                 _longs([o.nbytes for o in outs]), decoded)
    if rc:
        raise ValueError("SQYAMD_Decode_Batch returned %d" % rc)
    return outs


def set_option(name, value):
    """SQYAMD_Set_Option (run-time switches, include/sqeazy_amd.h); raises on an unknown name / a value out of range"""
    if lib().SQYAMD_Set_Option(name.encode(), ctypes.c_long(int(value))):
        raise ValueError("SQYAMD_Set_Option(%r, %r) refused" % (name, value))


def get_option(name):
    return int(lib().SQYAMD_Get_Option(name.encode()))


CALL_STAMP_FIELDS = ("seq", "lane", "thread", "entry", "lanes_taken", "clear_launched", "transpose_launched", "parse_queued", "sync_returned", "returned")


def call_stamps(max_records=8192):
    """SQYAMD_Call_Stamps: the newest records of the encode calls made under option "call_stamps", oldest first, one dict per call
    (CALL_STAMP_FIELDS: place on the transpose lane, parse lane, steady-clock nanoseconds; include/sqeazy_amd.h)"""
    fn = lib().SQYAMD_Call_Stamps
    fn.restype = ctypes.c_long
    fn.argtypes = [ctypes.POINTER(ctypes.c_long), ctypes.c_long]
    nf = len(CALL_STAMP_FIELDS)
    buf = (ctypes.c_long * (nf * max_records))()
    n = fn(buf, max_records)
    return [dict(zip(CALL_STAMP_FIELDS, buf[i * nf:(i + 1) * nf])) for i in range(n)]


def dedupe_report():
    """SQYAMD_Dedupe_Report: (keys, dup_of) of the newest chunked encode call that ran the duplicate-chunk search under option
    "dedupe_report" -- uint64 keys of the full chunks, uint32 dup_of of all chunks; two empty arrays when there is no record"""
    fn = lib().SQYAMD_Dedupe_Report
    fn.restype = ctypes.c_long
    fn.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_uint), ctypes.c_long]
    n = fn(None, None, 0)
    keys, dup_of = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
    if n:
        n = min(n, fn(keys.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)), dup_of.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)), n))
    return keys[:n], dup_of[:n]


class option:
    """with sqeazy_amd.option("block_parallel", 0): ...  -- the option for the duration of the block (process-wide)"""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = get_option(self.name)
        set_option(self.name, self.value)
        return self

    def __exit__(self, *exc):
        set_option(self.name, self.old)
        return False


def profile_enable(on=True):
    lib().SQYAMD_Profile_Enable(ctypes.c_int(1 if on else 0))


def profile_reset():
    lib().SQYAMD_Profile_Reset()


def profile_get():
    """{kernel name: (total ms, launches)} since the last reset"""
    out = {}
    i = 0
    while True:
        ms = ctypes.c_double(0)
        n = ctypes.c_long(0)
        name = lib().SQYAMD_Profile_Get(ctypes.c_int(i), ctypes.byref(ms), ctypes.byref(n))
        if not name:
            break
        out[name.decode()] = (ms.value, n.value)
        i += 1
    return out
