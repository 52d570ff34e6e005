"""fennec_amd -- fennec's per-pixel hot path on AMD Instinct MI355X (gfx950).

A thin ctypes binding of ``libfennec_hip.so`` (C ABI: ``include/fennec_hip.h``):
hand-written HIP kernels behind the reference's own function names
(``SSIM``, ``SSIMFast``, ``MSSSIM``, ``GaussianBlur``, ``Sharpen``,
``AdaptiveSharpen``, ``ApplyOrientation``, ``lanczosResize``, ``smartResize``,
``boxDownsample``; shamspias/fennec ssim.go / resize.go / effects.go / exif.go).

Images are ``image.NRGBA`` byte buffers:

* numpy ``uint8`` arrays of shape ``(h, w, 4)`` with contiguous rows -> host space
  (the library stages them through the GPU and returns numpy arrays);
* torch ``uint8`` CUDA/HIP tensors of shape ``(h, w, 4)`` -> device space (results
  are new device tensors; nothing crosses PCIe).

There is NO CPU implementation in this package: without the built library or
without a GPU every call raises.  Build with ``python -c "import __graft_entry__
as g; g.build()"`` or ``make -C fennec_amd/csrc``.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

from . import synth  # noqa: F401  (deterministic test/bench images)

__all__ = [
    "Context", "default_context", "load_library", "FennecError",
    "SSIM", "SSIMFast", "MSSSIM", "GaussianBlur", "Sharpen", "AdaptiveSharpen",
    "ApplyOrientation", "lanczosResize", "smartResize", "boxDownsample",
    "gaussianKernel", "blurKernel", "precomputeWeights", "Summarize",
]

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FENNEC_HIP_LIB") or os.path.join(_HERE, "libfennec_hip.so")   # override: A/B builds

FNX_OK, FNX_NOOP, FNX_EMPTY = 0, 1, 2
FNX_HOST, FNX_DEVICE, FNX_DEVICE_SRC = 0, 1, 2
FNX_BLUR_FAST, FNX_BLUR_EXACT, FNX_BLUR_KEEP_BOX_SUMS = 0, 1, 2
FNX_PNG_PALETTED, FNX_PNG_GRAY, FNX_PNG_NRGBA = 1, 2, 3      # fnx_png_reduce's kinds (compress.go:90-108)
FNX_PNG_DECODE_ROWS = 1024                                    # png_decode.hip: rows a workgroup of png_unfilter_kernel keeps in flight
FNX_PNG_DECODE_CHUNK = 32                                     # fnx_png_decode_batch: files per set of launches, at most
FNX_PNG_COMPRESS_CHUNK = 32                                   # fnx_png_compress_batch: images per set of launches, at most
FNX_DEFLATE_CHUNK, FNX_DEFLATE_SUB = 32768, 128               # deflate.hip: bytes per chunk (= per workgroup, per block) and per lane
FNX_DEFLATE_LEVEL_FAST, FNX_DEFLATE_LEVEL_DENSE = 0, 1         # fnx_ctx_set_deflate_level
FNX_JPEG_HUFFMAN_STANDARD, FNX_JPEG_HUFFMAN_OPTIMIZED = 0, 1   # fnx_ctx_set_jpeg_huffman
FNX_JPEG_SUBSAMPLING_420, FNX_JPEG_SUBSAMPLING_444 = 0, 1      # fnx_ctx_set_jpeg_subsampling
FNX_DEFLATE_DENSE_DEPTH = 32                                   # the dense level: the most chain candidates a position tries
FNX_CRC_RUN, FNX_CRC_PIECE = 64, 16384                         # crc32.hip: bytes per lane and per workgroup
FNX_PNG_CRC_HOST, FNX_PNG_CRC_DEVICE = 0, 1                    # fnx_ctx_set_png_crc
PROF_MAIN, PROF_SSIM, PROF_RESIZE, PROF_FX, PROF_JPEG = 1, 2, 4, 8, 16

_u8p = C.c_void_p
_f64p = C.POINTER(C.c_double)
_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)


class Analysis(C.Structure):
    """fnx_analysis (include/fennec_hip.h): what the device computes for Analyze."""
    _fields_ = [("histogram", C.c_uint64 * 256), ("bright_sum", C.c_double), ("variance_sum", C.c_double),
                ("sample_count", C.c_int64), ("edge_count", C.c_int64), ("edge_total", C.c_int64),
                ("unique_colors", C.c_int32), ("has_alpha", C.c_int32), ("is_grayscale", C.c_int32),
                ("pad", C.c_int32)]


class ImageStats(C.Structure):
    """fennec_ImageStats = ImageStats (analyze.go:9-22)."""
    _fields_ = [("Width", C.c_int32), ("Height", C.c_int32), ("HasAlpha", C.c_int32), ("IsGrayscale", C.c_int32),
                ("UniqueColors", C.c_int32), ("RecommendedFormat", C.c_int32), ("RecommendedQuality", C.c_int32),
                ("pad", C.c_int32), ("Entropy", C.c_double), ("EdgeDensity", C.c_double),
                ("MeanBrightness", C.c_double), ("Contrast", C.c_double), ("EstimatedCompression", C.c_double)]


class NativeBatchResult(C.Structure):
    """fennec_BatchResult (include/fennec_hip.h)."""
    _fields_ = [("index", C.c_int32), ("failed", C.c_int32), ("has_result", C.c_int32), ("quality", C.c_int32), ("steps", C.c_int32),
                ("status", C.c_int32), ("original_size", C.c_int64), ("compressed_size", C.c_int64), ("ssim", C.c_double),
                ("device", C.c_int32), ("reserved", C.c_int32)]


FNX_ERR_INVALID = -1
FNX_ERR_UNSUPPORTED = -5

# fnx_jpeg_target_size's strategies (include/fennec_hip.h): strategy 1, 3, 4 of hitTargetSize and its JPEG fallback
FNX_TS_QUALITY, FNX_TS_QUALITY_SCALE, FNX_TS_SCALE, FNX_TS_FALLBACK = 1, 2, 4, 8
FNX_TS_ALL = FNX_TS_QUALITY | FNX_TS_QUALITY_SCALE | FNX_TS_SCALE | FNX_TS_FALLBACK
FNX_TS_QUANTIZE, FNX_TS_SCALE_PNG, FNX_TS_FALLBACK_PNG = 16, 32, 64    # fnx_png_target_size's legs
FNX_TS_PNG_ALL = FNX_TS_QUANTIZE | FNX_TS_SCALE_PNG | FNX_TS_FALLBACK_PNG
FNX_FORMAT_AUTO, FNX_FORMAT_JPEG, FNX_FORMAT_PNG = 0, 1, 2             # fnx_hit_target_size's format (types.go:35-42)


class SizeCandidate(C.Structure):
    """fnx_size_candidate (include/fennec_hip.h): one strategy's sizeResult."""
    _fields_ = [("strategy", C.c_int32), ("quality", C.c_int32), ("final_w", C.c_int32), ("final_h", C.c_int32),
                ("steps", C.c_int32), ("reserved", C.c_int32), ("nbytes", C.c_int64), ("ssim", C.c_double)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


class FileOptions(C.Structure):
    """fennec_FileOptions (include/fennec_hip.h): the Options fields CompressFile's JPEG path reads."""
    _fields_ = [("orient", C.c_int32), ("max_w", C.c_int32), ("max_h", C.c_int32), ("auto_format", C.c_int32), ("target_ssim", C.c_double)]


class TargetOptions(C.Structure):
    """fennec_TargetOptions (include/fennec_hip.h): CompressFile's options in target-size mode."""
    _fields_ = [("file", FileOptions), ("target_bytes", C.c_int64), ("strategies", C.c_int32), ("reserved", C.c_int32)]

    @classmethod
    def make(cls, target_bytes: int, orient: int = 1, max_w: int = 0, max_h: int = 0, strategies: int = FNX_TS_ALL):
        return cls(FileOptions(int(orient), int(max_w), int(max_h), 0, 0.0), int(target_bytes), int(strategies), 0)


class FennecError(RuntimeError):
    pass


class FennecUnsupported(FennecError):
    """fnx_jpeg_decode / fnx_jpeg_recompress / fnx_png_decode: a file the device decoder does not take (FNX_ERR_UNSUPPORTED) -- decode it
    on the host."""


_lib = None
_lib_lock = threading.Lock()


def _sig(L, name, restype, argtypes):
    f = getattr(L, name)
    f.restype = restype
    f.argtypes = argtypes


def load_library() -> C.CDLL:
    """dlopen libfennec_hip.so and declare every entry point of include/fennec_hip.h."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise FennecError(
                f"{LIB_PATH} is missing: build the HIP extension first "
                "(make -C fennec_amd/csrc, or __graft_entry__.build()); there is no CPU fallback")
        # PyTorch wheels bundle their own HIP runtime and link it by file name, so it is not
        # deduplicated against /opt/rocm's copy by soname: if our library pulled the system
        # runtime in first, torch would later load a SECOND runtime that sees no GPUs.  Let
        # torch (when present) load its runtime first; ours then binds to the same one.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        L = C.CDLL(LIB_PATH)
        ctx = C.c_void_p
        i = C.c_int
        d = C.c_double
        img = [_u8p, i]                                   # pointer, stride
        _sig(L, "fnx_version", C.c_char_p, [])
        _sig(L, "fnx_device_count", i, [])
        _sig(L, "fnx_set_devices", i, [C.POINTER(C.c_int), i])
        _sig(L, "fnx_last_error", C.c_char_p, [])
        _sig(L, "fnx_ctx_create", i, [i, C.POINTER(ctx)])
        _sig(L, "fnx_ctx_destroy", None, [ctx])
        _sig(L, "fnx_ctx_device", i, [ctx])
        _sig(L, "fnx_ctx_stream", C.c_void_p, [ctx])
        _sig(L, "fnx_ctx_sync", i, [ctx])
        _sig(L, "fnx_ctx_use_stream", i, [ctx, C.c_void_p])
        _sig(L, "fnx_ctx_use_own_stream", i, [ctx])
        _sig(L, "fnx_ctx_profile", i, [ctx, i])
        _sig(L, "fnx_ctx_kernel_ms", i, [ctx, C.POINTER(C.c_float)])
        _sig(L, "fnx_ctx_last_kernel", C.c_char_p, [ctx, i])
        _sig(L, "fnx_ctx_set_form", i, [ctx, C.c_char_p, C.c_char_p])
        _sig(L, "fnx_ctx_resize_mfma_report", i, [ctx, C.POINTER(C.c_uint), C.POINTER(C.c_uint)])
        _sig(L, "fnx_ctx_set_ssim_mode", i, [ctx, i])
        _sig(L, "fnx_ctx_set_png_adam7", i, [ctx, i])
        _sig(L, "fnx_ctx_set_deflate_level", i, [ctx, i])
        _sig(L, "fnx_ctx_set_jpeg_huffman", i, [ctx, i])
        _sig(L, "fnx_ctx_set_jpeg_subsampling", i, [ctx, i])
        _sig(L, "fnx_ctx_set_png_crc", i, [ctx, i])
        _sig(L, "fnx_crc32", i, [ctx, i, _u8p, C.c_size_t, C.c_uint32, C.POINTER(C.c_uint32)])
        _sig(L, "fnx_jpeg_symbol_histogram", i, [ctx, i] + img + [i, i, i, C.POINTER(C.c_uint32)])
        _sig(L, "fnx_jpeg_huffman_tables", i, [ctx, C.POINTER(C.c_uint32), _u8p, _u8p, C.POINTER(C.c_int), C.POINTER(C.c_uint32),
                                               C.POINTER(C.c_int)])
        _sig(L, "fnx_png_adam7_passes", i, [i, i, i, i, C.POINTER(i), C.POINTER(i), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)])
        _sig(L, "fnx_malloc", i, [ctx, C.c_size_t, C.POINTER(C.c_void_p)])
        _sig(L, "fnx_free", i, [ctx, C.c_void_p])
        _sig(L, "fnx_upload", i, [ctx, C.c_void_p, i, C.c_void_p, i, i, i])
        _sig(L, "fnx_download", i, [ctx, C.c_void_p, i, C.c_void_p, i, i, i])
        _sig(L, "fnx_gaussian_blur", i, [ctx, i] + img + [i, i, _f64p, i, i] + img)
        _sig(L, "fnx_blur_fixed_point", i, [_f64p, i, C.POINTER(C.c_longlong), C.POINTER(d)])
        _sig(L, "fnx_blur3x3", i, [ctx, i] + img + [i, i] + img)
        _sig(L, "fnx_sharpen", i, [ctx, i] + img + [i, i, d] + img)
        _sig(L, "fnx_adaptive_sharpen", i, [ctx, i] + img + [i, i, d] + img)
        _sig(L, "fnx_resize_h", i, [ctx, i] + img + [i, i, _i32p, _i32p, _f64p] + img + [i])
        _sig(L, "fnx_resize_v", i, [ctx, i] + img + [i, i, _i32p, _i32p, _f64p] + img + [i])
        _sig(L, "fnx_lanczos_resize", i, [ctx, i] + img + [i, i, _i32p, _i32p, _f64p, _i32p, _i32p, _f64p] + img + [i, i])
        _sig(L, "fnx_resize_fixed_point", i, [_i32p, _i32p, _f64p, i, i, C.POINTER(i), C.POINTER(i), _i32p, _i32p, _i32p])
        _sig(L, "fnx_box_downsample", i, [ctx, i] + img + [i, i] + img + [i, i])
        tabs = [_i32p, _i32p, _f64p, _i32p, _i32p, _f64p]   # offH, idxH, wH, offV, idxV, wV
        _sig(L, "fnx_lanczos_box_downsample", i, [ctx, i] + img + [i, i] + tabs + [i, i] + img + [i, i])
        _sig(L, "fnx_lanczos_box_fused", i, [i, i] + tabs + [i, i, i, i])
        _sig(L, "fnx_ssim_fast_resized", i, [ctx, i] + img + [i, i] + img + [i, i] + tabs + [_f64p, _f64p])
        _sig(L, "fnx_ssim_resized", i, [ctx, i] + img + [i, i] + img + [i, i] + tabs + [_f64p, _f64p])
        _sig(L, "fnx_msssim_resized", i, [ctx, i] + img + [i, i] + img + [i, i] + tabs + [_f64p, _f64p, _f64p])
        _sig(L, "fnx_ssim_fast", i, [ctx, i] + img + img + [i, i, _f64p, _f64p])
        _sig(L, "fnx_ssim", i, [ctx, i] + img + img + [i, i, _f64p, _f64p])
        _sig(L, "fnx_pixel_ssim", i, [ctx, i, _u8p, C.c_size_t, _u8p, C.c_size_t, i, i, _f64p])
        _sig(L, "fnx_msssim", i, [ctx, i] + img + img + [i, i, _f64p, _f64p, _f64p])
        _sig(L, "fnx_ssim_fast_prepare", i, [ctx, i] + img + [i, i, C.POINTER(C.c_void_p)])
        _sig(L, "fnx_ssim_fast_against", i, [ctx, C.c_void_p, i] + img + [_f64p, _f64p])
        _sig(L, "fnx_prepared_free", None, [ctx, C.c_void_p])
        _sig(L, "fnx_orient", i, [ctx, i] + img + [i, i, i] + img)
        _sig(L, "fnx_gaussian_blur_batch", i, [ctx, i, C.POINTER(C.c_void_p), i, i, i, _f64p, i, i, C.POINTER(C.c_void_p), i])
        _sig(L, "fnx_ssim_fast_batch", i, [ctx, i, C.POINTER(C.c_void_p), i, C.POINTER(C.c_void_p), i, i, i, _f64p, _f64p])
        _sig(L, "fnx_ssim_fast_batch_enqueue", i, [ctx, i, C.POINTER(C.c_void_p), i, C.POINTER(C.c_void_p), i, i, i, _f64p])
        _sig(L, "fnx_results_fetch", i, [ctx, i, _f64p])
        _sig(L, "fnx_ssim_enqueue", i, [ctx] + img + img + [i, i, _f64p])
        _sig(L, "fnx_msssim_enqueue", i, [ctx] + img + img + [i, i, _f64p])
        _sig(L, "fennec_MSSSIM_enqueue", i, [ctx] + img + [i, i] + img + [i, i])
        _sig(L, "fnx_jpeg_encode", i, [ctx, i] + img + [i, i, i, _u8p, C.c_size_t, C.POINTER(C.c_size_t)])
        _sig(L, "fennec_CompressBatchNRGBA", i, [i, i, i, i, C.POINTER(C.c_void_p), C.POINTER(i), C.POINTER(i), C.POINTER(i), _i64p, d,
                                                  C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(NativeBatchResult), C.POINTER(i),
                                                  C.c_void_p, C.c_void_p])
        _sig(L, "fennec_CompressBatchJPEG", i, [i, i, i, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), d, C.POINTER(C.c_void_p),
                                                 C.POINTER(C.c_size_t), C.POINTER(NativeBatchResult), C.POINTER(i), C.c_void_p, C.c_void_p])
        _sig(L, "fennec_CompressBatchNRGBADevices", i, [C.POINTER(i), i, i, i, i, C.POINTER(C.c_void_p), C.POINTER(i), C.POINTER(i), C.POINTER(i),
                                                         _i64p, d, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(NativeBatchResult),
                                                         C.POINTER(i), C.c_void_p, C.c_void_p])
        _sig(L, "fennec_CompressBatchJPEGDevices", i, [C.POINTER(i), i, i, i, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), d,
                                                        C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(NativeBatchResult), C.POINTER(i),
                                                        C.c_void_p, C.c_void_p])
        _sig(L, "fennec_CompressFileJPEG", i, [ctx, _u8p, C.c_size_t, C.POINTER(FileOptions), _u8p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(i),
                                                _f64p, C.POINTER(i), C.POINTER(i)])
        _sig(L, "fennec_CompressBatchJPEGOpts", i, [i, i, i, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(FileOptions),
                                                     C.POINTER(C.POINTER(FileOptions)), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                                     C.POINTER(NativeBatchResult), C.POINTER(i), C.POINTER(i), C.c_void_p, C.c_void_p])
        _sig(L, "fennec_CompressFileTargetSize", i, [ctx, _u8p, C.c_size_t, C.POINTER(TargetOptions), C.POINTER(i), C.POINTER(SizeCandidate),
                                                      C.POINTER(i), _u8p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(i)])
        _sig(L, "fennec_CompressBatchTargetSize", i, [i, i, i, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(TargetOptions),
                                                       C.POINTER(C.POINTER(TargetOptions)), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                                       C.POINTER(NativeBatchResult), C.POINTER(SizeCandidate), C.POINTER(i), C.POINTER(i),
                                                       C.c_void_p, C.c_void_p])
        _sig(L, "fennec_pool_release", None, [])
        _sig(L, "fennec_SummarizeResults", d, [i, C.POINTER(NativeBatchResult), _i64p])
        _sig(L, "fnx_jpeg_size_search", i, [ctx, i] + img + [i, i, C.c_longlong, i, _f64p, _u8p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(i),
                                             _f64p, C.POINTER(i)])
        _sig(L, "fnx_jpeg_compress", i, [ctx, i] + img + [i, i, d, _f64p, _u8p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(i), _f64p,
                                          C.POINTER(i)])
        _sig(L, "fnx_jpeg_compress_batch", i, [ctx, i, C.POINTER(C.c_void_p), i, i, i, _f64p, _f64p, C.POINTER(C.c_void_p),
                                                C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(i), _f64p, C.POINTER(i),
                                                C.POINTER(i)])
        _sig(L, "fnx_jpeg_roundtrip", i, [ctx, i] + img + [i, i, i] + img)
        _sig(L, "fnx_jpeg_decode", i, [ctx, _u8p, C.c_size_t, i, C.c_void_p, i, C.POINTER(i), C.POINTER(i)])
        _sig(L, "fnx_jpeg_progressive_coefficients", i, [_u8p, C.c_size_t, C.POINTER(C.c_int16), C.c_size_t, C.POINTER(C.c_size_t),
                                                        C.POINTER(i), C.POINTER(i), C.POINTER(i)])
        _sig(L, "fnx_jpeg_recompress", i, [ctx, _u8p, C.c_size_t, d, _f64p, _u8p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(i), _f64p,
                                            C.POINTER(i), C.POINTER(i), C.POINTER(i)])
        _sig(L, "fnx_jpeg_decode_batch", i, [ctx, i, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.POINTER(i), C.POINTER(i),
                                             C.POINTER(i), C.POINTER(i)])
        _sig(L, "fnx_jpeg_recompress_batch", i, [ctx, i, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), _f64p, _f64p, C.POINTER(C.c_void_p),
                                                 C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(i), _f64p, C.POINTER(i), C.POINTER(i),
                                                 C.POINTER(i), C.POINTER(i)])
        _sig(L, "fnx_jpeg_quality_search", i, [ctx, i] + img + [i, i, d, _f64p, C.POINTER(i), _f64p, C.POINTER(i)])
        _sig(L, "fnx_jpeg_encode_scaled", i, [ctx, i] + img + [i, i, i, i, i, _u8p, C.c_size_t, C.POINTER(C.c_size_t)])
        _sig(L, "fnx_jpeg_target_size", i, [ctx, i] + img + [i, i, C.c_longlong, i, _f64p, C.POINTER(C.c_int), C.POINTER(SizeCandidate),
                                             C.POINTER(i), _u8p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p, i])
        for name in ("fnx_png_target_size", "fnx_hit_target_size"):
            _sig(L, name, i, [ctx, i] + img + [i, i, C.c_longlong, i, _f64p, C.POINTER(C.c_int), C.POINTER(SizeCandidate),
                              C.POINTER(i), _u8p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p, i])
        _sig(L, "fennec_CompressFileHitTargetSize", i, [ctx, _u8p, C.c_size_t, C.POINTER(FileOptions), C.c_longlong, i, C.POINTER(i),
                                                         C.POINTER(SizeCandidate), C.POINTER(i), _u8p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(i)])
        _sig(L, "fnx_gaussian_blur_ssim_fast", i, [ctx, i] + img + [i, i, _f64p, i, i] + img + [_f64p, _f64p])
        _sig(L, "fnx_ssim_batch_enqueue", i, [ctx, i, C.POINTER(C.c_void_p), i, C.POINTER(C.c_void_p), i, i, i, _f64p])
        _sig(L, "fnx_sharpen_batch", i, [ctx, i, C.POINTER(C.c_void_p), i, i, i, C.c_double, C.POINTER(C.c_void_p), i])
        _sig(L, "fnx_adaptive_sharpen_batch", i, [ctx, i, C.POINTER(C.c_void_p), i, i, i, C.c_double, C.POINTER(C.c_void_p), i])
        _sig(L, "fnx_msssim_batch_enqueue", i, [ctx, i, C.POINTER(C.c_void_p), i, C.POINTER(C.c_void_p), i, i, i, _f64p])
        _sig(L, "fennec_MSSSIM_batch_enqueue", i, [ctx, i, C.POINTER(C.c_void_p), i, i, i, C.POINTER(C.c_void_p), i, i, i])
        _sig(L, "fnx_lanczos_resize_batch", i, [ctx, i, C.POINTER(C.c_void_p), i, i, i, _i32p, _i32p, _f64p, _i32p, _i32p, _f64p,
                                                C.POINTER(C.c_void_p), i, i, i])
        _sig(L, "fennec_lanczosResizeBatch", i, [ctx, i, C.POINTER(C.c_void_p), i, i, i, C.POINTER(C.c_void_p), i, i, i])
        _sig(L, "fnx_gaussian_blur_ssim_fast_batch", i,
             [ctx, i, C.POINTER(C.c_void_p), i, i, i, _f64p, i, i, C.POINTER(C.c_void_p), i, _f64p, _f64p])
        _sig(L, "fnx_gaussian_blur_ssim_fast_batch_enqueue", i,
             [ctx, i, C.POINTER(C.c_void_p), i, i, i, _f64p, i, i, C.POINTER(C.c_void_p), i, _f64p])
        _sig(L, "fnx_analyze", i, [ctx, i] + img + [i, i, C.POINTER(Analysis)])
        _sig(L, "fnx_analyze_batch", i, [ctx, i, C.POINTER(C.c_void_p), i, i, i, C.POINTER(Analysis)])
        _sig(L, "fnx_scan_flags", i, [ctx, i, _u8p, C.c_size_t, C.POINTER(i), C.POINTER(i)])
        _sig(L, "fennec_Analyze", i, [ctx, i] + img + [i, i, C.POINTER(ImageStats)])
        _sig(L, "fennec_statsFromAnalysis", None, [C.POINTER(Analysis), i, i, C.POINTER(ImageStats)])
        _sig(L, "fennec_isOpaque", i, [ctx, i] + img + [i, i, C.POINTER(i)])
        _sig(L, "fennec_isGrayscale", i, [ctx, i] + img + [i, i, C.POINTER(i)])
        _sig(L, "fnx_ycbcr_to_nrgba", i, [ctx, i, _u8p, i, _u8p, _u8p, i, i, i, i] + img)
        _sig(L, "fnx_ssim_fast_against_ycbcr", i, [ctx, C.c_void_p, i, _u8p, i, _u8p, _u8p, i, i, _f64p, _f64p])
        _sig(L, "fnx_apply_palette", i, [ctx, i] + img + [i, i, _u8p, i, _u8p, i, _u8p, i])
        _sig(L, "fnx_median_cut", i, [ctx, i] + img + [i, i, i, C.POINTER(i), _u8p, C.POINTER(i)])
        _sig(L, "fnx_quantize", i, [ctx, i] + img + [i, i, i, _u8p, C.POINTER(i), _u8p, i, _u8p, i, _f64p, _f64p])
        _sig(L, "fnx_png_reduce", i, [ctx, i] + img + [i, i, i, C.POINTER(i), _u8p, C.POINTER(i), _u8p, i])
        _sig(L, "fennec_CompressFilePNGReduce", i, [ctx, _u8p, C.c_size_t, C.POINTER(FileOptions), C.POINTER(i), _u8p, C.POINTER(i), _u8p,
                                                     C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(i)])
        _sig(L, "fnx_png_filter", i, [ctx, i, i, _u8p, i, i, i, i, i, _u8p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(i), C.POINTER(i)])
        _sig(L, "fennec_CompressFilePNGStream", i, [ctx, _u8p, C.c_size_t, C.POINTER(FileOptions), C.POINTER(i), _u8p, C.POINTER(i),
                                                     C.POINTER(i), C.POINTER(i), _u8p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(i)])
        _sig(L, "fnx_deflate_bound", C.c_size_t, [C.c_size_t])
        _sig(L, "fnx_deflate", i, [ctx, i, _u8p, C.c_size_t, i, _u8p, C.c_size_t, C.POINTER(C.c_size_t)])
        _sig(L, "fnx_png_encode", i, [ctx, i, i, _u8p, i, i, i, i, i, _u8p, _u8p, C.c_size_t, C.POINTER(C.c_size_t)])
        _sig(L, "fnx_png_encoded_size", i, [ctx, i, i, _u8p, i, i, i, i, i, _u8p, C.POINTER(C.c_size_t)])
        _sig(L, "fnx_inflate", i, [_u8p, C.c_size_t, _u8p, C.c_size_t, C.POINTER(C.c_size_t)])
        _sig(L, "fnx_png_info", i, [_u8p, C.c_size_t, C.POINTER(i), C.POINTER(i), C.POINTER(i), C.POINTER(i), C.POINTER(i)])
        _sig(L, "fnx_png_decode", i, [ctx, _u8p, C.c_size_t, i, C.c_void_p, i, C.POINTER(i), C.POINTER(i)])
        _sig(L, "fnx_png_decode_batch", i, [ctx, i, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.POINTER(i), i,
                                            C.POINTER(i), C.POINTER(i), C.POINTER(i)])
        _sig(L, "fennec_CompressFilePNG", i, [ctx, _u8p, C.c_size_t, C.POINTER(FileOptions), _u8p, C.c_size_t, C.POINTER(C.c_size_t),
                                               C.POINTER(i), C.POINTER(i)])
        _sig(L, "fnx_png_file_bound", C.c_size_t, [i, i])
        _sig(L, "fnx_png_compress_batch", i, [ctx, i, C.POINTER(C.c_void_p), C.POINTER(i), C.POINTER(i), C.POINTER(i), C.POINTER(C.c_void_p),
                                              C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(i), C.POINTER(i)])
        _sig(L, "fnx_png_recompress_batch", i, [ctx, i, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), i, C.POINTER(C.c_void_p),
                                                C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(i), C.POINTER(i), C.POINTER(i),
                                                C.POINTER(i)])
        _sig(L, "fennec_gaussianKernel", None, [i, d, _f64p])
        _sig(L, "fennec_blurKernel", i, [d, _f64p])
        _sig(L, "fennec_lanczosKernel", d, [d])
        _sig(L, "fennec_precomputeWeights", i, [i, i, _i32p, _i32p, _f64p])
        _sig(L, "fennec_smartResizeDims", i, [i, i, i, i, C.POINTER(i), C.POINTER(i)])
        _sig(L, "fennec_ssimFastDims", i, [i, i, C.POINTER(i), C.POINTER(i)])
        _sig(L, "fennec_SSIM", i, [ctx, i] + img + [i, i] + img + [i, i, _f64p])
        _sig(L, "fennec_SSIMFast", i, [ctx, i] + img + img + [i, i, _f64p])
        _sig(L, "fennec_MSSSIM", i, [ctx, i] + img + [i, i] + img + [i, i, _f64p])
        _sig(L, "fennec_computeSSIMNRGBA", i, [ctx, i] + img + [i, i] + img + [i, i, _f64p])
        _sig(L, "fennec_GaussianBlur", i, [ctx, i] + img + [i, i, d] + img)
        _sig(L, "fennec_Sharpen", i, [ctx, i] + img + [i, i, d] + img)
        _sig(L, "fennec_AdaptiveSharpen", i, [ctx, i] + img + [i, i, d] + img)
        _sig(L, "fennec_ApplyOrientation", i, [ctx, i] + img + [i, i, i] + img)
        _sig(L, "fennec_lanczosResize", i, [ctx, i] + img + [i, i] + img + [i, i])
        _sig(L, "fennec_boxDownsample", i, [ctx, i] + img + [i, i] + img + [i, i])
        _sig(L, "fennec_Summarize", d, [i, _i32p, _i32p, _i64p, _i64p, _f64p, _i64p])
        _lib = L
        return L


# names include/fennec_hip.h declares (checked by tests/test_abi.py against the header itself)
def exported_symbols():
    import re
    hdr = os.path.join(os.path.dirname(_HERE), "include", "fennec_hip.h")
    text = open(hdr).read()
    return sorted(set(re.findall(r"\b((?:fnx|fennec)_\w+)\s*\(", text)))


# ---------------------------------------------------------------------------------------
def _is_torch(x) -> bool:
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")


class _Img:
    """(space, pointer, stride, w, h) view of a numpy array or a torch device tensor."""

    __slots__ = ("space", "ptr", "stride", "w", "h", "obj")

    def __init__(self, x):
        self.obj = x
        if _is_torch(x):
            import torch
            if not x.is_cuda or x.dtype != torch.uint8 or x.dim() != 3 or x.shape[2] != 4:
                raise FennecError("device images must be uint8 CUDA/HIP tensors of shape (h, w, 4)")
            h, w = int(x.shape[0]), int(x.shape[1])
            if h > 0 and w > 0 and (x.stride(2) != 1 or x.stride(1) != 4):
                raise FennecError("image rows must be contiguous")
            self.space, self.ptr = FNX_DEVICE, x.data_ptr()
            self.stride = int(x.stride(0)) if h > 1 else w * 4
        else:
            a = x
            if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 4:
                raise FennecError("host images must be numpy uint8 arrays of shape (h, w, 4)")
            h, w = a.shape[:2]
            if h > 0 and w > 0 and (a.strides[2] != 1 or a.strides[1] != 4):
                raise FennecError("image rows must be contiguous")
            self.space, self.ptr = FNX_HOST, a.ctypes.data
            self.stride = int(a.strides[0]) if h > 1 else w * 4
        self.w, self.h = int(w), int(h)

    def like(self, w: int, h: int):
        """A fresh tight w x h image in the same space.  Every kernel writes every dst pixel
        (zeros where image.NewNRGBA's zero pixel survives in the reference), so no memset --
        a torch.zeros fill would also run on torch's stream and race with the ctx stream."""
        if self.space == FNX_DEVICE:
            import torch
            return torch.empty((h, w, 4), dtype=torch.uint8, device=self.obj.device)
        return np.empty((h, w, 4), dtype=np.uint8)


def _f64(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(_f64p)


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(_i32p)


def _into_buffer(call, cap: int, n):
    """call(buf, cap) -> rc: an entry point that writes a file into `buf` and its size into the c_size_t `n`.  When it fails
    with a size over `cap`, it runs once more into a buffer of that size.  -> (rc, buf)"""
    buf = np.empty(cap, dtype=np.uint8)
    rc = call(buf, cap)
    if rc < 0 and n.value > cap:
        cap = n.value
        buf = np.empty(cap, dtype=np.uint8)
        rc = call(buf, cap)
    return rc, buf


class Context:
    """One GPU, one stream, its scratch (fnx_ctx).  Not re-entrant: one per worker thread."""

    def __init__(self, device: int = 0):
        self._lib = load_library()
        h = C.c_void_p()
        rc = self._lib.fnx_ctx_create(int(device), C.byref(h))
        if rc < 0:
            raise FennecError(f"fnx_ctx_create({device}): {self._err()}")
        self._h = h
        self.device = int(device)
        self._lent = -1            # handle of the torch stream the ctx currently launches on (-1: its own stream)
        self._png_adam7 = False    # set_png_adam7: what the wrappers' own header checks follow

    # -- plumbing ---------------------------------------------------------------------
    def _err(self) -> str:
        return (self._lib.fnx_last_error() or b"").decode()

    def _chk(self, rc: int, what: str) -> int:
        if rc == FNX_ERR_UNSUPPORTED:
            raise FennecUnsupported(f"{what} ({rc}): {self._err()}")
        if rc < 0:
            raise FennecError(f"{what} failed ({rc}): {self._err()}")
        return rc

    def close(self):
        if getattr(self, "_h", None):
            self._lib.fnx_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        self._chk(self._lib.fnx_ctx_sync(self._h), "fnx_ctx_sync")

    def profile(self, enable=True):
        """Bracket kernel launches with HIP events (fnx_ctx_profile).  True / 1: the blur / analyze pass
        kernels; or a mask of PROF_MAIN | PROF_SSIM | PROF_RESIZE | PROF_FX."""
        self._chk(self._lib.fnx_ctx_profile(self._h, int(enable)), "fnx_ctx_profile")

    def kernel_ms(self) -> float:
        """Duration, in ms, of the oldest bracketed kernel launch not read yet (waits for it): one call per
        launch, in launch order."""
        ms = C.c_float(0.0)
        self._chk(self._lib.fnx_ctx_kernel_ms(self._h, C.byref(ms)), "fnx_ctx_kernel_ms")
        return float(ms.value)

    def last_kernel(self, prof_class: int = 1) -> str:
        """The kernel this ctx's last call of a class (PROF_MAIN = GaussianBlur, PROF_SSIM, PROF_RESIZE) launched: the
        route the library's dispatch really took (fnx_ctx_last_kernel); "" before the first such call."""
        s = self._lib.fnx_ctx_last_kernel(self._h, int(prof_class))
        if s is None:
            raise FennecError("fnx_ctx_last_kernel: bad class")
        return s.decode()

    def resize_mfma_report(self):
        """fnx_ctx_resize_mfma_report, after sync(): (gave_up, workgroups) of this ctx's most recent resize call that launched
        resize_mfma_kernel -- how many of its workgroups handed their region back to resize_fused_sparse_kernel, and how many
        it launched; workgroups == 0: no such call on record.  Reporting only."""
        g, n = C.c_uint(0), C.c_uint(0)
        self._chk(self._lib.fnx_ctx_resize_mfma_report(self._h, C.byref(g), C.byref(n)), "fnx_ctx_resize_mfma_report")
        return int(g.value), int(n.value)

    def set_ssim_mode(self, fast: bool) -> None:
        """fnx_ctx_set_ssim_mode: fp32 moments (<= 1e-6) instead of fp64 (<= 1e-9) for full-resolution SSIM planes"""
        self._chk(self._lib.fnx_ctx_set_ssim_mode(self._h, 1 if fast else 0), "fnx_ctx_set_ssim_mode")

    def set_png_adam7(self, accept: bool) -> None:
        """fnx_ctx_set_png_adam7: the PNG entries of this ctx decode Adam7-interlaced files (True) instead of answering
        FennecUnsupported for them (False, the default)"""
        self._chk(self._lib.fnx_ctx_set_png_adam7(self._h, 1 if accept else 0), "fnx_ctx_set_png_adam7")
        self._png_adam7 = bool(accept)

    def set_deflate_level(self, level) -> None:
        """fnx_ctx_set_deflate_level: "fast" (FNX_DEFLATE_LEVEL_FAST, the default: the bytes the library always gave) or
        "dense" (FNX_DEFLATE_LEVEL_DENSE: hash chains, lazy and cross-chunk matches -- a smaller stream of the same layout)
        for every device deflate of this ctx: deflate, png_encode, compress_png(device_deflate=True), png_compress_batch,
        png_recompress_batch.  The integer constants are accepted too."""
        if isinstance(level, str):
            names = {"fast": FNX_DEFLATE_LEVEL_FAST, "dense": FNX_DEFLATE_LEVEL_DENSE}
            if level not in names:
                raise FennecError(f"set_deflate_level: 'fast' or 'dense', not {level!r}")
            level = names[level]
        self._chk(self._lib.fnx_ctx_set_deflate_level(self._h, int(level)), "fnx_ctx_set_deflate_level")

    def set_jpeg_huffman(self, mode) -> None:
        """fnx_ctx_set_jpeg_huffman: "standard" (FNX_JPEG_HUFFMAN_STANDARD, the default: the typical tables of T.81 Annex K.3.3,
        the bytes the library always wrote) or "optimized" (FNX_JPEG_HUFFMAN_OPTIMIZED: the four tables built from the file's
        own symbols, Annex K.2 -- the same coefficients in fewer bytes) for every JPEG file and file size of this ctx:
        jpeg_encode, jpeg_encoded_size, jpeg_encode_scaled, jpeg_size_search, jpeg_compress, jpeg_target_size, hit_target_size,
        jpeg_recompress, the file entries, jpeg_compress_batch, jpeg_recompress_batch.  The integer constants are accepted too."""
        if isinstance(mode, str):
            names = {"standard": FNX_JPEG_HUFFMAN_STANDARD, "optimized": FNX_JPEG_HUFFMAN_OPTIMIZED}
            if mode not in names:
                raise FennecError(f"set_jpeg_huffman: 'standard' or 'optimized', not {mode!r}")
            mode = names[mode]
        self._chk(self._lib.fnx_ctx_set_jpeg_huffman(self._h, int(mode)), "fnx_ctx_set_jpeg_huffman")

    def set_jpeg_subsampling(self, mode) -> None:
        """fnx_ctx_set_jpeg_subsampling: "420" (FNX_JPEG_SUBSAMPLING_420, the default: the bytes the library always wrote) or
        "444" (FNX_JPEG_SUBSAMPLING_444: chroma at full resolution, every component at sampling 1 x 1) for the single-image
        entries of this ctx: jpeg_roundtrip, jpeg_quality_search, jpeg_encode, jpeg_encoded_size, jpeg_compress,
        jpeg_size_search, jpeg_symbol_histogram.  Every other JPEG-writing entry refuses a ctx set to "444" (FennecError,
        FNX_ERR_UNSUPPORTED).  The integer constants are accepted too."""
        if isinstance(mode, str):
            names = {"420": FNX_JPEG_SUBSAMPLING_420, "444": FNX_JPEG_SUBSAMPLING_444}
            if mode not in names:
                raise FennecError(f"set_jpeg_subsampling: '420' or '444', not {mode!r}")
            mode = names[mode]
        self._chk(self._lib.fnx_ctx_set_jpeg_subsampling(self._h, int(mode)), "fnx_ctx_set_jpeg_subsampling")

    def set_png_crc(self, mode) -> None:
        """fnx_ctx_set_png_crc: "host" (FNX_PNG_CRC_HOST, the default: the host walks the IDAT chunk once its bytes have come
        down) or "device" (FNX_PNG_CRC_DEVICE: crc32.hip's kernels read the gathered stream on the device and the CRC word
        comes down with the sizes) for every PNG file this ctx makes from a device deflate: png_encode,
        compress_png(device_deflate=True), compress_file_png, hit_target_size, png_compress_batch, png_recompress_batch.  The
        files are the same bytes.  The integer constants are accepted too."""
        if isinstance(mode, str):
            names = {"host": FNX_PNG_CRC_HOST, "device": FNX_PNG_CRC_DEVICE}
            if mode not in names:
                raise FennecError(f"set_png_crc: 'host' or 'device', not {mode!r}")
            mode = names[mode]
        self._chk(self._lib.fnx_ctx_set_png_crc(self._h, int(mode)), "fnx_ctx_set_png_crc")

    def set_form(self, name: str, value=None) -> None:
        """fnx_ctx_set_form: which of several kernels that compute the same bytes this ctx takes (tests, A/B timing);
        value None: the product's own choice again."""
        v = None if value is None else str(value).encode()
        self._chk(self._lib.fnx_ctx_set_form(self._h, name.encode(), v), "fnx_ctx_set_form")

    def forms(self, **kw):
        """`with ctx.forms(fx_stream=0, fx_pairs=1): ...` -- set_form for the block, defaults afterwards"""
        ctx = self

        class _Forms:
            def __enter__(self_inner):
                for k, v in kw.items():
                    ctx.set_form(k, v)

            def __exit__(self_inner, *exc):
                for k in kw:
                    ctx.set_form(k, None)
                return False
        return _Forms()

    @property
    def stream(self) -> int:
        return int(self._lib.fnx_ctx_stream(self._h) or 0)

    # -- ordering against torch's streams ---------------------------------------------------
    # Device-space calls only ENQUEUE.  torch knows nothing about a private HIP stream: inputs may still be being
    # written on torch's current stream, outputs would be read by torch before the kernels have run, and the caching
    # allocator could recycle a dropped tensor while kernels still use it.  So every method that takes device tensors
    # runs inside `_ordered(...)`, which makes the ctx LAUNCH ON torch's current stream (fnx_ctx_use_stream): the work
    # is then ordered like any torch op on that stream and the allocator's stream-ordered reuse is safe -- with no
    # cross-stream event per call (the first version waited both ways on every call: ~25 us of idle GPU between two
    # back-to-back calls, measured on the config-4 timeline).  The switch happens once per (ctx, stream) change.
    # Concurrency between worker contexts therefore needs a torch stream per worker (`with torch.cuda.stream(s)`),
    # exactly as for torch's own ops.  Host (numpy) calls are synchronous and skip all of this.
    class _Ordered:
        __slots__ = ("ctx", "tensors")

        def __init__(self, ctx, tensors):
            self.ctx = ctx
            self.tensors = [t for t in tensors if _is_torch(t) and t.is_cuda]

        def __enter__(self):
            if self.tensors:
                import torch
                cur = torch.cuda.current_stream(self.tensors[0].device).cuda_stream
                if self.ctx._lent != cur:
                    self.ctx._chk(self.ctx._lib.fnx_ctx_use_stream(self.ctx._h, C.c_void_p(cur)), "fnx_ctx_use_stream")
                    self.ctx._lent = cur
            return self

        def add(self, *tensors):
            self.tensors.extend(t for t in tensors if _is_torch(t) and t.is_cuda)

        def __exit__(self, *exc):
            return False

    def _ordered(self, *tensors):
        return Context._Ordered(self, tensors)

    def use_own_stream(self):
        """Back to the ctx's private stream (plans and C-style callers that order work themselves)."""
        self._chk(self._lib.fnx_ctx_use_own_stream(self._h), "fnx_ctx_use_own_stream")
        self._lent = -1

    def _pair(self, a, b):
        ia, ib = _Img(a), _Img(b)
        if ia.space != ib.space:
            raise FennecError("both images must live in the same space (numpy or device tensors)")
        return ia, ib

    # -- table generators (Go side of the seam) -----------------------------------------
    def gaussianKernel(self, size: int = 8, sigma: float = 1.5) -> np.ndarray:
        k = np.empty(size * size, dtype=np.float64)
        self._lib.fennec_gaussianKernel(size, sigma, k.ctypes.data_as(_f64p))
        return k

    def blurKernel(self, sigma: float):
        r = self._lib.fennec_blurKernel(float(sigma), None)
        k = np.empty(2 * r + 1, dtype=np.float64)
        self._lib.fennec_blurKernel(float(sigma), k.ctypes.data_as(_f64p))
        return r, k

    def precomputeWeights(self, dst_size: int, src_size: int):
        off = np.zeros(dst_size + 1, dtype=np.int32)
        n = self._lib.fennec_precomputeWeights(dst_size, src_size, off.ctypes.data_as(_i32p), None, None)
        idx = np.zeros(max(n, 1), dtype=np.int32)
        wt = np.zeros(max(n, 1), dtype=np.float64)
        self._lib.fennec_precomputeWeights(dst_size, src_size, off.ctypes.data_as(_i32p),
                                           idx.ctypes.data_as(_i32p), wt.ctypes.data_as(_f64p))
        return off, idx[:max(n, 0)], wt[:max(n, 0)]

    def smartResizeDims(self, w, h, max_w, max_h):
        dw, dh = C.c_int(), C.c_int()
        r = self._lib.fennec_smartResizeDims(w, h, max_w, max_h, C.byref(dw), C.byref(dh))
        return bool(r), dw.value, dh.value

    def ssimFastDims(self, w, h):
        nw, nh = C.c_int(), C.c_int()
        r = self._lib.fennec_ssimFastDims(w, h, C.byref(nw), C.byref(nh))
        return bool(r), nw.value, nh.value

    # -- ssim.go ------------------------------------------------------------------------
    def SSIM(self, img1, img2) -> float:
        """ssim.go:24 -- full-resolution SSIM; a differently sized img2 is Lanczos-resized."""
        a, b = self._pair(img1, img2)
        out = C.c_double()
        with self._ordered(img1, img2):
            self._chk(self._lib.fennec_SSIM(self._h, a.space, a.ptr, a.stride, a.w, a.h, b.ptr, b.stride,
                                            b.w, b.h, C.byref(out)), "SSIM")
        return out.value

    def pixelSSIM(self, pix_a, pix_b, w: int, h: int) -> float:
        """ssim.go:169 over the two FLAT Pix slices as Go holds them (1-D uint8 numpy arrays or device tensors): for a
        SubImage that is everything up to the end of the parent's buffer, which SSIM / SSIMFast cannot know."""
        def flat(x):
            if _is_torch(x):
                return FNX_DEVICE, x.data_ptr(), int(x.numel())
            x = np.ascontiguousarray(x, dtype=np.uint8).reshape(-1)
            keep.append(x)
            return FNX_HOST, x.ctypes.data, int(x.size)
        keep = []
        (sa, pa, na), (sb, pb, nb) = flat(pix_a), flat(pix_b)
        if sa != sb:
            raise FennecError("both Pix slices must live in the same space")
        out = C.c_double()
        with self._ordered(pix_a, pix_b):
            self._chk(self._lib.fnx_pixel_ssim(self._h, sa, C.cast(pa, _u8p), na, C.cast(pb, _u8p), nb, int(w), int(h),
                                               C.byref(out)), "pixelSSIM")
        return out.value

    def ssim_enqueue(self, img1, img2, window=None):
        """fnx_ssim_enqueue: SSIM of a device pair of equal dims, result fetched later with fetch_result()
        (FIFO, at most 4 unfetched).  The caller keeps img1 / img2 alive until then."""
        a, b = self._pair(img1, img2)
        if a.space != FNX_DEVICE or (a.w, a.h) != (b.w, b.h):
            raise FennecError("ssim_enqueue takes two device tensors of equal dims")
        k, pk = _f64(self.gaussianKernel() if window is None else window)
        with self._ordered(img1, img2):
            self._chk(self._lib.fnx_ssim_enqueue(self._h, a.ptr, a.stride, b.ptr, b.stride, a.w, a.h, pk), "fnx_ssim_enqueue")

    def msssim_enqueue(self, img1, img2):
        """fennec_MSSSIM_enqueue: MSSSIM of a device pair (img2 resized to img1's dims first when they differ,
        ssim.go:320-322) through the result FIFO; fetch_result() returns the value.  The caller keeps both alive."""
        a, b = self._pair(img1, img2)
        if a.space != FNX_DEVICE:
            raise FennecError("msssim_enqueue takes two device tensors")
        with self._ordered(img1, img2):
            self._chk(self._lib.fennec_MSSSIM_enqueue(self._h, a.ptr, a.stride, a.w, a.h, b.ptr, b.stride, b.w, b.h),
                      "fennec_MSSSIM_enqueue")

    def msssim_batch_enqueue(self, imgs1, imgs2):
        """fennec_MSSSIM_batch_enqueue: n device pairs (every imgs1[i] of one size, every imgs2[i] of one size) as ONE FIFO
        entry; the imgs2 are resized to imgs1's dims by one batched lanczosResize when the dims differ.  fetch_results(n)."""
        va, vb = [_Img(t) for t in imgs1], [_Img(t) for t in imgs2]
        n = len(va)
        if n == 0 or n != len(vb) or any(v.space != FNX_DEVICE for v in va + vb):
            raise FennecError("msssim_batch_enqueue takes two equally long, non-empty lists of device tensors")
        a0, b0 = va[0], vb[0]
        if any((v.w, v.h, v.stride) != (a0.w, a0.h, a0.stride) for v in va) or any((v.w, v.h, v.stride) != (b0.w, b0.h, b0.stride) for v in vb):
            raise FennecError("every image of a side must share width, height and stride")
        pa = (C.c_void_p * n)(*[v.ptr for v in va])
        pb = (C.c_void_p * n)(*[v.ptr for v in vb])
        with self._ordered(*imgs1, *imgs2):
            self._chk(self._lib.fennec_MSSSIM_batch_enqueue(self._h, n, pa, a0.stride, a0.w, a0.h, pb, b0.stride, b0.w, b0.h),
                      "fennec_MSSSIM_batch_enqueue")

    def ssim_batch_enqueue(self, imgs1, imgs2, window=None):
        """fnx_ssim_batch_enqueue: SSIM of n same-sized device pairs in one launch; fetch_results(n)."""
        va, vb = [_Img(t) for t in imgs1], [_Img(t) for t in imgs2]
        n = len(va)
        if n == 0 or n != len(vb) or any(v.space != FNX_DEVICE for v in va + vb):
            raise FennecError("ssim_batch_enqueue takes two equally long, non-empty lists of device tensors")
        a0, b0 = va[0], vb[0]
        if any((v.w, v.h, v.stride) != (a0.w, a0.h, a0.stride) for v in va) or any((v.w, v.h, v.stride) != (a0.w, a0.h, b0.stride) for v in vb):
            raise FennecError("every image of a batch must share width and height, and every image of a side its stride")
        pa = (C.c_void_p * n)(*[v.ptr for v in va])
        pb = (C.c_void_p * n)(*[v.ptr for v in vb])
        k, pk = _f64(self.gaussianKernel() if window is None else window)
        with self._ordered(*imgs1, *imgs2):
            self._chk(self._lib.fnx_ssim_batch_enqueue(self._h, n, pa, a0.stride, pb, b0.stride, a0.w, a0.h, pk), "fnx_ssim_batch_enqueue")

    def sharpen_batch(self, imgs, strength: float, adaptive: bool = False, outs=None):
        """Sharpen / AdaptiveSharpen (effects.go:10 / :49) of n same-sized device images in one launch (fnx_*_sharpen_batch);
        strength <= 0 or images under 3 x 3 come back as they are, as from the single calls.  Enqueued."""
        views = [_Img(t) for t in imgs]
        if not views or any(v.space != FNX_DEVICE for v in views):
            raise FennecError("sharpen_batch takes a non-empty list of device tensors")
        v0 = views[0]
        if any((v.w, v.h, v.stride) != (v0.w, v0.h, v0.stride) for v in views):
            raise FennecError("every image of a batch must share width, height and stride")
        if strength <= 0 or v0.w < 3 or v0.h < 3:
            return list(imgs)
        amount = 1.0 + min(strength, 1.0) * (2.0 if adaptive else 1.5)
        if outs is None:
            outs = [v0.like(v0.w, v0.h) for _ in views]
        ov = [_Img(t) for t in outs]
        n = len(views)
        srcs = (C.c_void_p * n)(*[v.ptr for v in views])
        dsts = (C.c_void_p * n)(*[v.ptr for v in ov])
        fn = self._lib.fnx_adaptive_sharpen_batch if adaptive else self._lib.fnx_sharpen_batch
        with self._ordered(*imgs, *outs):
            self._chk(fn(self._h, n, srcs, v0.stride, v0.w, v0.h, C.c_double(amount), dsts, ov[0].stride), "sharpen_batch")
        return outs

    def fetch_results(self, n: int) -> np.ndarray:
        """The oldest FIFO entry's n values (fnx_results_fetch)."""
        out = np.empty(n, dtype=np.float64)
        self._chk(self._lib.fnx_results_fetch(self._h, n, out.ctypes.data_as(_f64p)), "fnx_results_fetch")
        return out

    def fetch_result(self) -> float:
        """The oldest enqueued scalar result (fnx_results_fetch)."""
        out = C.c_double()
        self._chk(self._lib.fnx_results_fetch(self._h, 1, C.byref(out)), "fnx_results_fetch")
        return out.value

    def SSIMFast(self, img1, img2) -> float:
        """ssim.go:48 -- SSIM on <=512 px box-downsampled copies."""
        a, b = self._pair(img1, img2)
        out = C.c_double()
        with self._ordered(img1, img2):
            self._chk(self._lib.fennec_SSIMFast(self._h, a.space, a.ptr, a.stride, b.ptr, b.stride, a.w, a.h,
                                                C.byref(out)), "SSIMFast")
        return out.value

    def MSSSIM(self, img1, img2) -> float:
        """ssim.go:313 -- 5-level multi-scale SSIM.  A strided / cropped view is treated as a Go SubImage: the pyramid starts from
        the first 4*w*h flat bytes (convert.go:16), not from the view's rows; pass a contiguous copy for row-wise semantics."""
        a, b = self._pair(img1, img2)
        out = C.c_double()
        with self._ordered(img1, img2):
            self._chk(self._lib.fennec_MSSSIM(self._h, a.space, a.ptr, a.stride, a.w, a.h, b.ptr, b.stride,
                                              b.w, b.h, C.byref(out)), "MSSSIM")
        return out.value

    def computeSSIMNRGBA(self, img1, img2) -> float:
        """targetsize.go:563 -- SSIMFast(img1, lanczosResize(img2, img1's dims)).  img2 goes to the device at its own size;
        under set_form("resize_box", 1), where SSIMFast downsamples (img1 above 512 px) and img2 is the smaller image, the resized
        image is never stored."""
        a, b = self._pair(img1, img2)
        out = C.c_double()
        with self._ordered(img1, img2):
            self._chk(self._lib.fennec_computeSSIMNRGBA(self._h, a.space, a.ptr, a.stride, a.w, a.h, b.ptr, b.stride,
                                                        b.w, b.h, C.byref(out)), "computeSSIMNRGBA")
        return out.value

    def _resized_args(self, a, b, tables):
        """(keep-alive arrays, the six table pointers) of a *_resized call: `tables` = (table_h, table_v) as precomputeWeights
        returns them (b.w -> a.w, b.h -> a.h), None: computed here; NULL pointers when the dims are equal."""
        if tables is None:
            if (a.w, a.h) == (b.w, b.h) or min(a.w, a.h, b.w, b.h) <= 0:
                return [], [None] * 6
            tables = (self.precomputeWeights(a.w, b.w), self.precomputeWeights(a.h, b.h))
        keep, ptrs = [], []
        for off, idx, wt in tables:
            for arr, conv in ((off, _i32), (idx, _i32), (wt, _f64)):
                if arr is None:
                    ptrs.append(None)
                    continue
                k, ptr = conv(arr)
                keep.append(k)
                ptrs.append(ptr)
        return keep, ptrs

    def _scored_resized(self, name, img1, img2, tables, window, levels=False):
        a, b = self._pair(img1, img2)
        keep, t = self._resized_args(a, b, tables)
        k, pk = _f64(self.gaussianKernel() if window is None else window)
        out = C.c_double()
        extra = []
        if levels:
            lv = np.empty(5, dtype=np.float64)
            extra = [lv.ctypes.data_as(_f64p)]
        with self._ordered(img1, img2):
            self._chk(getattr(self._lib, name)(self._h, a.space, a.ptr, a.stride, a.w, a.h, b.ptr, b.stride, b.w, b.h, *t, pk,
                                               C.byref(out), *extra), name)
        return (out.value, lv) if levels else out.value

    def ssim_fast_resized(self, img1, img2, tables=None, window=None) -> float:
        """fnx_ssim_fast_resized: computeSSIMNRGBA with the CALLER's tap tables ((table_h, table_v), None: precomputeWeights')."""
        return self._scored_resized("fnx_ssim_fast_resized", img1, img2, tables, window)

    def ssim_resized(self, img1, img2, tables=None, window=None) -> float:
        """fnx_ssim_resized: SSIM (ssim.go:24) of differently sized images with the caller's tap tables."""
        return self._scored_resized("fnx_ssim_resized", img1, img2, tables, window)

    def msssim_resized(self, img1, img2, tables=None, window=None):
        """fnx_msssim_resized: MSSSIM (ssim.go:313) of differently sized images -> (value, the five per-level values)."""
        return self._scored_resized("fnx_msssim_resized", img1, img2, tables, window, levels=True)

    def lanczosBoxDownsample(self, img, midW: int, midH: int, dstW: int, dstH: int, to_host: bool = False, tables=None):
        """boxDownsample(lanczosResize(img, midW, midH), dstW, dstH) (resize.go:37, ssim.go:244) in one call
        (fnx_lanczos_box_downsample): under set_form("resize_box", 1), where the fused kernel applies, the midW x midH image is
        never stored.
        to_host: see boxDownsample."""
        s = _Img(img)
        if min(s.w, s.h, midW, midH, dstW, dstH) <= 0:
            return self._out_for(s, 0, 0, to_host)[1]
        if tables is None and (s.w, s.h) != (midW, midH):
            tables = (self.precomputeWeights(midW, s.w), self.precomputeWeights(midH, s.h))
        keep, t = self._resized_args(s, s, tables)
        space, dst = self._out_for(s, dstW, dstH, to_host)
        d = _Img(dst)
        with self._ordered(img, dst):
            self._chk(self._lib.fnx_lanczos_box_downsample(self._h, space, s.ptr, s.stride, s.w, s.h, *t, midW, midH,
                                                           d.ptr, d.stride, dstW, dstH), "fnx_lanczos_box_downsample")
        return dst

    def msssim_levels(self, img1, img2, window=None):
        """fnx_msssim with per-level SSIMFast values (equal dims)."""
        a, b = self._pair(img1, img2)
        k, pk = _f64(self.gaussianKernel() if window is None else window)
        out = C.c_double()
        lv = np.empty(5, dtype=np.float64)
        with self._ordered(img1, img2):
            self._chk(self._lib.fnx_msssim(self._h, a.space, a.ptr, a.stride, b.ptr, b.stride, a.w, a.h, pk,
                                           C.byref(out), lv.ctypes.data_as(_f64p)), "fnx_msssim")
        return out.value, lv

    def boxDownsample(self, img, dstW: int, dstH: int, to_host: bool = False):
        """ssim.go:244.  to_host=True with a device image (FNX_DEVICE_SRC): the result is a numpy array and the
        call returns when it is filled -- the scale searches of targetsize.go:240-313 keep ONE source
        resident and fetch a small downsample per iteration."""
        s = _Img(img)
        if s.w <= 0 or s.h <= 0 or dstW <= 0 or dstH <= 0:
            return self._out_for(s, 0, 0, to_host)[1]
        space, dst = self._out_for(s, dstW, dstH, to_host)
        d = _Img(dst)
        with self._ordered(img, dst):
            self._chk(self._lib.fennec_boxDownsample(self._h, space, s.ptr, s.stride, s.w, s.h, d.ptr,
                                                     d.stride, dstW, dstH), "boxDownsample")
        return dst

    @staticmethod
    def _out_for(s: "_Img", w: int, h: int, to_host: bool):
        """(space, fresh destination) for an image -> image op on `s`."""
        if to_host and s.space == FNX_DEVICE:
            return FNX_DEVICE_SRC, np.empty((h, w, 4), dtype=np.uint8)
        return s.space, s.like(w, h)

    def ssim_fast_prepare(self, img):
        s = _Img(img)
        p = C.c_void_p()
        with self._ordered(img):
            self._chk(self._lib.fnx_ssim_fast_prepare(self._h, s.space, s.ptr, s.stride, s.w, s.h, C.byref(p)),
                      "fnx_ssim_fast_prepare")
        return _Prepared(self, p, s.w, s.h)

    # -- the JPEG quantisation round trip (first slice) -----------------------
    def jpeg_roundtrip(self, img, quality: int):
        """toNRGBARef(jpeg.Decode(jpeg.Encode(img, quality))) as far as the pixels go (fnx_jpeg_roundtrip): baseline
        4:2:0 with Go's image/jpeg arithmetic, no entropy coding."""
        s = _Img(img)
        dst = s.like(s.w, s.h)
        d = _Img(dst)
        with self._ordered(img, dst):
            self._chk(self._lib.fnx_jpeg_roundtrip(self._h, s.space, s.ptr, s.stride, s.w, s.h, int(quality), d.ptr, d.stride),
                      "fnx_jpeg_roundtrip")
        return dst

    def jpeg_encode(self, img, quality: int) -> bytes:
        """jpeg.Encode(img, &jpeg.Options{Quality: quality}) on the device (fnx_jpeg_encode) -> the file's bytes."""
        s = _Img(img)
        cap = 4096 + (s.w * s.h * 3) // 2
        n = C.c_size_t(0)
        with self._ordered(img):
            rc, buf = _into_buffer(lambda b, c: self._lib.fnx_jpeg_encode(self._h, s.space, s.ptr, s.stride, s.w, s.h, int(quality),
                                                                          b.ctypes.data_as(_u8p), c, C.byref(n)), cap, n)
            if rc == FNX_OK:
                return buf[:n.value].tobytes()
        self._chk(rc, "fnx_jpeg_encode")

    def jpeg_symbol_histogram(self, img, quality: int):
        """fnx_jpeg_symbol_histogram -> (4, 256) uint32: how often the scan of jpeg_encode(img, quality) codes every symbol with
        the luminance DC, luminance AC, chrominance DC and chrominance AC table (jpeg_symhist_kernel's counts)."""
        s = _Img(img)
        hist = np.zeros((4, 256), dtype=np.uint32)
        with self._ordered(img):
            self._chk(self._lib.fnx_jpeg_symbol_histogram(self._h, s.space, s.ptr, s.stride, s.w, s.h, int(quality),
                                                          hist.ctypes.data_as(C.POINTER(C.c_uint32))), "fnx_jpeg_symbol_histogram")
        return hist

    def jpeg_huffman_tables(self, hist):
        """fnx_jpeg_huffman_tables: jpeg_hufftab_kernel on four histograms ((4, 256), none all zero) -> a list of four dicts
        {bits: 16 counts, vals: the values in code order, lut: (256,) uint32 length << 24 | code, standard: bool}."""
        h = np.ascontiguousarray(hist, dtype=np.uint32)
        if h.shape != (4, 256):
            raise FennecError("jpeg_huffman_tables: hist must be (4, 256)")
        bits = np.zeros((4, 16), dtype=np.uint8)
        vals = np.zeros((4, 256), dtype=np.uint8)
        lut = np.zeros((4, 256), dtype=np.uint32)
        nvals = (C.c_int * 4)()
        std = (C.c_int * 4)()
        self._chk(self._lib.fnx_jpeg_huffman_tables(self._h, h.ctypes.data_as(C.POINTER(C.c_uint32)), bits.ctypes.data_as(_u8p),
                                                    vals.ctypes.data_as(_u8p), nvals, lut.ctypes.data_as(C.POINTER(C.c_uint32)), std),
                  "fnx_jpeg_huffman_tables")
        return [dict(bits=bits[t].tolist(), vals=vals[t, :nvals[t]].tolist(), lut=lut[t].copy(), standard=bool(std[t])) for t in range(4)]

    def jpeg_encoded_size(self, img, quality: int) -> int:
        """len(jpeg.Encode(img, quality)) without fetching the bytes (fnx_jpeg_encode's size query)."""
        s = _Img(img)
        n = C.c_size_t(0)
        with self._ordered(img):
            self._chk(self._lib.fnx_jpeg_encode(self._h, s.space, s.ptr, s.stride, s.w, s.h, int(quality), None, 0, C.byref(n)),
                      "fnx_jpeg_encode")
        return int(n.value)

    def jpeg_size_search(self, img, target_bytes: int, skip_ssim: bool = False, window=None):
        """jpegQualitySearchOpt (targetsize.go:125-176) on the device -> (bytes, quality, ssim, steps), or None when no
        quality fits target_bytes."""
        s = _Img(img)
        k, pk = _f64(self.gaussianKernel() if window is None else window)
        cap = max(4096, int(target_bytes) + 16)
        buf = np.empty(cap, dtype=np.uint8)
        n, q, st, v = C.c_size_t(0), C.c_int(), C.c_int(), C.c_double()
        with self._ordered(img):
            rc = self._chk(self._lib.fnx_jpeg_size_search(self._h, s.space, s.ptr, s.stride, s.w, s.h, int(target_bytes), int(bool(skip_ssim)), pk,
                                                          buf.ctypes.data_as(_u8p), cap, C.byref(n), C.byref(q), C.byref(v), C.byref(st)),
                           "fnx_jpeg_size_search")
        if rc != FNX_OK:
            return None
        return buf[:n.value].tobytes(), q.value, v.value, st.value

    def jpeg_compress(self, img, target_ssim: float, window=None):
        """compressJPEGOptimal on the device (fnx_jpeg_compress): search + the winning file -> (bytes, quality, ssim, steps)."""
        s = _Img(img)
        k, pk = _f64(self.gaussianKernel() if window is None else window)
        cap = 4096 + (s.w * s.h * 3) // 2
        n, q, st, v = C.c_size_t(0), C.c_int(), C.c_int(), C.c_double()
        with self._ordered(img):
            rc, buf = _into_buffer(lambda b, c: self._lib.fnx_jpeg_compress(self._h, s.space, s.ptr, s.stride, s.w, s.h, float(target_ssim), pk,
                                                                            b.ctypes.data_as(_u8p), c, C.byref(n), C.byref(q), C.byref(v),
                                                                            C.byref(st)), cap, n)
            if rc == FNX_OK:
                return buf[:n.value].tobytes(), q.value, v.value, st.value
        self._chk(rc, "fnx_jpeg_compress")

    def jpeg_compress_batch(self, imgs, target_ssim, window=None):
        """compressJPEGOptimal of n device images of one geometry in one call (fnx_jpeg_compress_batch) -> a list of
        (bytes, quality, ssim, steps): item i's is what jpeg_compress(imgs[i], target_ssim[i]) returns.  target_ssim: one
        float for every item, or a sequence of n."""
        views = [_Img(t) for t in imgs]
        if not views or any(v.space != FNX_DEVICE for v in views):
            raise FennecError("jpeg_compress_batch takes a non-empty list of device tensors")
        v0 = views[0]
        if any((v.w, v.h, v.stride) != (v0.w, v0.h, v0.stride) for v in views):
            raise FennecError("every image of a batch must share width, height and stride")
        n = len(views)
        if isinstance(target_ssim, (int, float)):
            targets = [float(target_ssim)] * n
        else:
            targets = [float(t) for t in target_ssim]
            if len(targets) != n:
                raise FennecError(f"jpeg_compress_batch: {len(targets)} targets for {n} images")
        k, pk = _f64(self.gaussianKernel() if window is None else window)
        tg, ptg = _f64(targets)
        cap = 4096 + (v0.w * v0.h * 3) // 2          # as jpeg_compress
        buf = np.empty((n, cap), dtype=np.uint8)
        srcs = (C.c_void_p * n)(*[v.ptr for v in views])
        outs = (C.c_void_p * n)(*[buf.ctypes.data + i * cap for i in range(n)])
        caps = (C.c_size_t * n)(*([cap] * n))
        nb, q, st, status = (C.c_size_t * n)(), (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)()
        v = (C.c_double * n)()
        with self._ordered(*imgs):
            self._chk(self._lib.fnx_jpeg_compress_batch(self._h, n, srcs, v0.stride, v0.w, v0.h, ptg, pk, outs, caps, nb, q, v, st,
                                                        status), "fnx_jpeg_compress_batch")
            res = []
            for i in range(n):
                if status[i] == FNX_OK:
                    data = buf[i, :nb[i]].tobytes()
                else:                                       # the buffer was small: the file at the quality found, no new search
                    data = self.jpeg_encode(imgs[i], q[i])
                res.append((data, q[i], v[i], st[i]))
        return res

    def jpeg_encode_scaled(self, img, dw: int, dh: int, quality: int, size_only: bool = False):
        """jpeg.Encode(boxDownsample(img, dw, dh), quality) (fnx_jpeg_encode_scaled) without the scaled image -> the file's
        bytes, or with size_only=True its length only."""
        s = _Img(img)
        dw, dh = int(dw), int(dh)
        if dw <= 0 or dh <= 0 or dw > 65535 or dh > 65535:
            raise FennecError(f"jpeg_encode_scaled: {dw} x {dh} is not a JPEG size (1..65535 each way)")
        n = C.c_size_t(0)
        with self._ordered(img):
            if size_only:
                self._chk(self._lib.fnx_jpeg_encode_scaled(self._h, s.space, s.ptr, s.stride, s.w, s.h, dw, dh, int(quality), None, 0,
                                                           C.byref(n)), "fnx_jpeg_encode_scaled")
                return int(n.value)
            cap = 4096 + (dw * dh * 3) // 2
            rc, buf = _into_buffer(lambda b, c: self._lib.fnx_jpeg_encode_scaled(self._h, s.space, s.ptr, s.stride, s.w, s.h, dw, dh, int(quality),
                                                                                 b.ctypes.data_as(_u8p), c, C.byref(n)), cap, n)
            if rc == FNX_OK:
                return buf[:n.value].tobytes()
        self._chk(rc, "fnx_jpeg_encode_scaled")

    def jpeg_target_size(self, img, target_bytes: int, strategies: int = FNX_TS_ALL, cancel=None, window=None):
        """hitTargetSize's JPEG strategies (targetsize.go:26-357) on the device (fnx_jpeg_target_size) -> a dict: `candidates`
        (four dicts in FNX_TS_* bit order; strategy 0 = none), `winner` (index, or None), `data` (the winner's file, or None),
        `image` (the winner's final image: the source itself for strategy 1 and the fallback, else the Lanczos-scaled image --
        numpy for a host source, a device tensor for a device one) and `status` (FNX_OK / FNX_NOOP).  `cancel`: a
        ctypes.c_int whose non-zero value stops the search where the reference checks ctx.Err()."""
        s = _Img(img)
        target_bytes, strategies = int(target_bytes), int(strategies)
        if s.w <= 0 or s.h <= 0 or s.w > 65535 or s.h > 65535:
            raise FennecError(f"jpeg_target_size: a {s.w} x {s.h} source is not a JPEG size (1..65535 each way)")
        if target_bytes <= 0:
            raise FennecError("jpeg_target_size: target_bytes must be > 0")
        if strategies <= 0 or strategies & ~FNX_TS_ALL:
            raise FennecError("jpeg_target_size: strategies must be a non-empty set of FNX_TS_* bits")
        if cancel is not None and not isinstance(cancel, C.c_int):
            raise FennecError("jpeg_target_size: cancel must be a ctypes.c_int (or None)")
        k, pk = _f64(self.gaussianKernel() if window is None else window)
        cand = (SizeCandidate * 4)()
        win, n = C.c_int(-1), C.c_size_t(0)
        scaled = s.like(s.w, s.h)                  # the winner's final image fits the source's footprint
        sv = _Img(scaled)
        cap = max(4096, target_bytes + 4096)
        buf = np.empty(cap, dtype=np.uint8)
        with self._ordered(img, scaled):
            rc = self._lib.fnx_jpeg_target_size(self._h, s.space, s.ptr, s.stride, s.w, s.h, target_bytes, strategies, pk,
                                                C.byref(cancel) if cancel is not None else None, cand, C.byref(win),
                                                buf.ctypes.data_as(_u8p), cap, C.byref(n), sv.ptr, sv.stride)
            too_small = rc == FNX_ERR_INVALID and n.value > cap and win.value >= 0
            if not too_small:
                self._chk(rc, "fnx_jpeg_target_size")
            if s.space == FNX_DEVICE:
                self.sync()
        cands = [c.as_dict() for c in cand]
        if rc == FNX_NOOP:
            return {"candidates": cands, "winner": None, "data": None, "image": None, "status": rc}
        c = cands[win.value]
        image = scaled[:c["final_h"], :c["final_w"]] if c["strategy"] in (FNX_TS_QUALITY_SCALE, FNX_TS_SCALE) else img
        # a winner over the target (the fallback, strategy 4's encode at bestQ) did not fit `buf`: its file from the image the
        # call left, at its quality -- no second search
        data = self.jpeg_encode(image, c["quality"]) if too_small else buf[:n.value].tobytes()
        return {"candidates": cands, "winner": win.value, "data": data, "image": image, "status": FNX_OK}

    def _target_size(self, entry: str, ncand: int, img, target_bytes: int, which: int, cancel, window):
        """fnx_png_target_size / fnx_hit_target_size -> jpeg_target_size's dict.  The first buffer holds two bytes a pixel; a
        winner that does not fit it (the call is then a second search) is asked for again with the size the call reported."""
        s = _Img(img)
        target_bytes = int(target_bytes)
        if s.w <= 0 or s.h <= 0 or s.w > 65535 or s.h > 65535:
            raise FennecError(f"{entry}: a {s.w} x {s.h} source (1..65535 each way)")
        if target_bytes <= 0:
            raise FennecError(f"{entry}: target_bytes must be > 0")
        if cancel is not None and not isinstance(cancel, C.c_int):
            raise FennecError(f"{entry}: cancel must be a ctypes.c_int (or None)")
        k, pk = _f64(self.gaussianKernel() if window is None else window)
        cand = (SizeCandidate * ncand)()
        win, n = C.c_int(-1), C.c_size_t(0)
        scaled = s.like(s.w, s.h)                  # the winner's final image fits the source's footprint
        sv = _Img(scaled)
        fn = getattr(self._lib, entry)
        with self._ordered(img, scaled):
            rc, buf = _into_buffer(lambda b, c: fn(self._h, s.space, s.ptr, s.stride, s.w, s.h, target_bytes, int(which), pk,
                                                   C.byref(cancel) if cancel is not None else None, cand, C.byref(win),
                                                   b.ctypes.data_as(_u8p), c, C.byref(n), sv.ptr, sv.stride),
                                   4096 + 2 * s.w * s.h, n)     # room for a winner over the target; a larger one is asked for again
            self._chk(rc, entry)
            if s.space == FNX_DEVICE:
                self.sync()
        cands = [c.as_dict() for c in cand]
        if rc == FNX_NOOP:
            return {"candidates": cands, "winner": None, "data": None, "image": None, "status": rc}
        c = cands[win.value]
        own = c["strategy"] in (FNX_TS_QUALITY_SCALE, FNX_TS_SCALE, FNX_TS_QUANTIZE, FNX_TS_SCALE_PNG)
        image = scaled[:c["final_h"], :c["final_w"]] if own else img
        return {"candidates": cands, "winner": win.value, "data": buf[:n.value].tobytes(), "image": image, "status": FNX_OK}

    def png_target_size(self, img, target_bytes: int, strategies: int = FNX_TS_PNG_ALL, cancel=None, window=None):
        """hitTargetSize's PNG legs on the device (fnx_png_target_size): quantizeStrategy, scaleSearch with format PNG, the PNG
        fallback -> jpeg_target_size's dict with three candidates (quantize, scale, fallback).  Every size is the size of this
        library's own file under the context's deflate level (set_deflate_level("dense") is the nearer to
        png.BestCompression); `image`: the quantized image, the Lanczos-scaled image, or the source for the fallback."""
        strategies = int(strategies)
        if strategies <= 0 or strategies & ~FNX_TS_PNG_ALL:
            raise FennecError("png_target_size: strategies must be a non-empty set of FNX_TS_QUANTIZE, FNX_TS_SCALE_PNG, FNX_TS_FALLBACK_PNG")
        return self._target_size("fnx_png_target_size", 3, img, target_bytes, strategies, cancel, window)

    def hit_target_size(self, img, target_bytes: int, format: int = FNX_FORMAT_AUTO, cancel=None, window=None):
        """All of hitTargetSize (targetsize.go:26-75) in one call (fnx_hit_target_size) -> jpeg_target_size's dict with five
        candidates: strategy 1, quantize, strategy 3, strategy 4 and the fallback in the format the reference picks (their
        `strategy` bits say which).  The winner's file is a PNG when its strategy is one of the FNX_TS_PNG_ALL bits."""
        if int(format) not in (FNX_FORMAT_AUTO, FNX_FORMAT_JPEG, FNX_FORMAT_PNG):
            raise FennecError("hit_target_size: format is FNX_FORMAT_AUTO, FNX_FORMAT_JPEG or FNX_FORMAT_PNG")
        return self._target_size("fnx_hit_target_size", 5, img, target_bytes, int(format), cancel, window)

    def compress_file_hit_target_size(self, data: bytes, target_bytes: int, format: int = FNX_FORMAT_AUTO, orient: int = 1, max_w: int = 0,
                                      max_h: int = 0, cancel=None):
        """compress_file_target_size under any Options.Format (fennec_CompressFileHitTargetSize): the same staging, then
        hit_target_size on the resident image -> the same dict, five candidates."""
        if cancel is not None and not isinstance(cancel, C.c_int):
            raise FennecError("compress_file_hit_target_size: cancel must be a ctypes.c_int (or None)")
        src = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, dtype=np.uint8)
        o = FileOptions(int(orient), int(max_w), int(max_h), 0, 0.0)
        cand = (SizeCandidate * 5)()
        win, n = C.c_int(-1), C.c_size_t(0)
        dims = (C.c_int * 4)()
        pc = C.byref(cancel) if cancel is not None else None
        rc, buf = _into_buffer(lambda b, c: self._lib.fennec_CompressFileHitTargetSize(self._h, src.ctypes.data_as(_u8p), len(data), C.byref(o),
                                                                                       int(target_bytes), int(format), pc, cand, C.byref(win),
                                                                                       b.ctypes.data_as(_u8p), c, C.byref(n), dims),
                               max(4096, int(target_bytes) + 4096), n)
        self._chk(rc, "fennec_CompressFileHitTargetSize")
        return {"candidates": [c.as_dict() for c in cand], "winner": win.value if rc == FNX_OK else None,
                "data": buf[:n.value].tobytes() if rc == FNX_OK else None, "dims": ((dims[0], dims[1]), (dims[2], dims[3])), "status": rc}

    @staticmethod
    def jpeg_progressive_coefficients(data: bytes):
        """Host only (fnx_jpeg_progressive_coefficients): a progressive file's quantised coefficients over all its scans, as the
        device's IDCT launch gets them -> (coef [blocks, 64] int16 in natural order, blocks MCU by MCU, (w, h), ratio)."""
        L = load_library()
        buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, dtype=np.uint8)
        nb, w, h, ratio = C.c_size_t(0), C.c_int(), C.c_int(), C.c_int()

        def chk(rc):
            if rc == FNX_ERR_UNSUPPORTED:
                raise FennecUnsupported(L.fnx_last_error().decode())
            if rc < 0:
                raise FennecError(f"fnx_jpeg_progressive_coefficients failed ({rc}): {L.fnx_last_error().decode()}")
        chk(L.fnx_jpeg_progressive_coefficients(buf.ctypes.data_as(_u8p), len(data), None, 0, C.byref(nb), C.byref(w), C.byref(h), C.byref(ratio)))
        coef = np.empty((nb.value, 64), dtype=np.int16)
        chk(L.fnx_jpeg_progressive_coefficients(buf.ctypes.data_as(_u8p), len(data), coef.ctypes.data_as(C.POINTER(C.c_int16)), nb.value,
                                                C.byref(nb), C.byref(w), C.byref(h), C.byref(ratio)))
        return coef, (w.value, h.value), ratio.value

    @staticmethod
    def jpeg_parse(data: bytes):
        """jpeg_decode_config without a ctx (the segment parser is host code): (w, h), FennecUnsupported, or FennecError."""
        L = load_library()
        buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, dtype=np.uint8)
        w, h = C.c_int(), C.c_int()
        rc = L.fnx_jpeg_decode(None, buf.ctypes.data_as(_u8p), len(data), FNX_HOST, None, 0, C.byref(w), C.byref(h))
        if rc == FNX_ERR_UNSUPPORTED:
            raise FennecUnsupported(L.fnx_last_error().decode())
        if rc < 0:
            raise FennecError(f"fnx_jpeg_decode failed ({rc}): {L.fnx_last_error().decode()}")
        return w.value, h.value

    def jpeg_decode_config(self, data: bytes):
        """jpeg.DecodeConfig as far as the device decoder goes: (w, h); FennecUnsupported for files it does not take."""
        buf = np.frombuffer(data, dtype=np.uint8)
        w, h = C.c_int(), C.c_int()
        self._chk(self._lib.fnx_jpeg_decode(self._h, buf.ctypes.data_as(_u8p), len(data), FNX_HOST, None, 0, C.byref(w), C.byref(h)),
                  "fnx_jpeg_decode")
        return w.value, h.value

    def jpeg_decode(self, data: bytes, device: bool = False):
        """toNRGBARef(jpeg.Decode(data)) on the device (fnx_jpeg_decode): the file's bytes go up, an (h, w, 4) uint8 array
        comes back -- or, with device=True, a torch tensor that stays on the ctx's device."""
        w, h = self.jpeg_decode_config(data)
        buf = np.frombuffer(data, dtype=np.uint8)
        if device:
            import torch
            dst = torch.empty((h, w, 4), dtype=torch.uint8, device=f"cuda:{self.device}")
        else:
            dst = np.empty((h, w, 4), dtype=np.uint8)
        d = _Img(dst)
        with self._ordered(dst):
            self._chk(self._lib.fnx_jpeg_decode(self._h, buf.ctypes.data_as(_u8p), len(data), d.space, d.ptr, d.stride, C.byref(C.c_int()),
                                                C.byref(C.c_int())), "fnx_jpeg_decode")
        return dst

    def jpeg_recompress(self, data: bytes, target_ssim: float, window=None):
        """CompressBatch's item body for a JPEG source on the device (fnx_jpeg_recompress): decode, quality search, the
        winner's file -> (bytes, quality, ssim, steps, (w, h))."""
        src = np.frombuffer(data, dtype=np.uint8)
        k, pk = _f64(self.gaussianKernel() if window is None else window)
        cap = len(data) + 4096       # a search ends below the quality a camera wrote; a larger file asks again with its size
        n, q, st, v, w, h = C.c_size_t(0), C.c_int(), C.c_int(), C.c_double(), C.c_int(), C.c_int()
        rc, buf = _into_buffer(lambda b, c: self._lib.fnx_jpeg_recompress(self._h, src.ctypes.data_as(_u8p), len(data), float(target_ssim), pk,
                                                                          b.ctypes.data_as(_u8p), c, C.byref(n), C.byref(q), C.byref(v),
                                                                          C.byref(st), C.byref(w), C.byref(h)), cap, n)
        if rc == FNX_OK:
            return buf[:n.value].tobytes(), q.value, v.value, st.value, (w.value, h.value)
        self._chk(rc, "fnx_jpeg_recompress")

    def _item_error(self, rc: int, what: str):
        """the exception the single call raises for a batch item's status (the message is the status: a batch keeps one text)"""
        kind = FennecUnsupported if rc == FNX_ERR_UNSUPPORTED else FennecError
        return kind(f"{what}: status {rc}")

    def jpeg_decode_batch(self, files, device: bool = False):
        """toNRGBARef(jpeg.Decode(f)) of every file of a list in one call (fnx_jpeg_decode_batch: one set of launches per chunk of
        baseline files) -> (images, statuses).  images[i] is an (h, w, 4) uint8 array -- with device=True a torch tensor on the
        ctx's device -- and what jpeg_decode(files[i]) returns, or None where statuses[i] != FNX_OK."""
        import torch
        files = [bytes(f) for f in files]
        n = len(files)
        if n == 0:
            raise FennecError("jpeg_decode_batch takes a non-empty list of files")
        bufs = [np.frombuffer(f, dtype=np.uint8) if len(f) else np.zeros(1, dtype=np.uint8) for f in files]
        dsts = []
        for f in files:                                   # a file whose config fails goes in with no destination
            try:
                w, h = self.jpeg_decode_config(f)
                dsts.append(torch.empty((h, w, 4), dtype=torch.uint8, device=f"cuda:{self.device}"))
            except FennecError:
                dsts.append(None)
        views = [None if t is None else _Img(t) for t in dsts]
        pf = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
        ps = (C.c_size_t * n)(*[len(f) for f in files])
        pd = (C.c_void_p * n)(*[None if v is None else v.ptr for v in views])
        pst = (C.c_int * n)(*[0 if v is None else v.stride for v in views])
        ws, hs, status = (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)()
        with self._ordered(*[t for t in dsts if t is not None]):
            self._chk(self._lib.fnx_jpeg_decode_batch(self._h, n, pf, ps, pd, pst, ws, hs, status), "fnx_jpeg_decode_batch")
            images = [dsts[i] if status[i] == FNX_OK else None for i in range(n)]
            if not device:
                images = [None if t is None else t.cpu().numpy() for t in images]
        return images, list(status)

    def jpeg_recompress_batch(self, files, target_ssim, window=None):
        """CompressBatch's item body for a list of JPEG files in one call (fnx_jpeg_recompress_batch) -> a list with, per item,
        what jpeg_recompress(files[i], target_ssim[i]) returns -- (bytes, quality, ssim, steps, (w, h)) -- or the FennecError /
        FennecUnsupported instance it would raise.  target_ssim: one float for every item, or a sequence of n."""
        files = [bytes(f) for f in files]
        n = len(files)
        if n == 0:
            raise FennecError("jpeg_recompress_batch takes a non-empty list of files")
        if isinstance(target_ssim, (int, float)):
            targets = [float(target_ssim)] * n
        else:
            targets = [float(t) for t in target_ssim]
            if len(targets) != n:
                raise FennecError(f"jpeg_recompress_batch: {len(targets)} targets for {n} files")
        k, pk = _f64(self.gaussianKernel() if window is None else window)
        tg, ptg = _f64(targets)
        bufs = [np.frombuffer(f, dtype=np.uint8) if len(f) else np.zeros(1, dtype=np.uint8) for f in files]
        outs = [np.empty(len(f) + 4096, dtype=np.uint8) for f in files]          # as jpeg_recompress
        pf = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
        ps = (C.c_size_t * n)(*[len(f) for f in files])
        po = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        caps = (C.c_size_t * n)(*[len(o) for o in outs])
        nb, q, st, status = (C.c_size_t * n)(), (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)()
        ws, hs = (C.c_int * n)(), (C.c_int * n)()
        v = (C.c_double * n)()
        self._chk(self._lib.fnx_jpeg_recompress_batch(self._h, n, pf, ps, ptg, pk, po, caps, nb, q, v, st, ws, hs, status),
                  "fnx_jpeg_recompress_batch")
        res = []
        for i in range(n):
            if status[i] == FNX_OK:
                res.append((outs[i][:nb[i]].tobytes(), q[i], v[i], st[i], (ws[i], hs[i])))
            elif status[i] == FNX_ERR_INVALID and nb[i] > caps[i]:          # the buffer was small: that item through the single call
                res.append(self.jpeg_recompress(files[i], targets[i], window))
            else:
                res.append(self._item_error(status[i], f"fnx_jpeg_recompress_batch: file {i}"))
        return res

    def compress_file_jpeg(self, data: bytes, target_ssim: float, orient: int = 1, max_w: int = 0, max_h: int = 0, auto_format: bool = False):
        """CompressFile for a JPEG or PNG source (the signature decides) in standard mode, every pixel stage on the device (fennec_CompressFileJPEG): decode,
        ApplyOrientation(orient), smartResize(max_w, max_h), analyzeFormat (auto_format), compressJPEGOptimal ->
        (bytes, quality, ssim, steps, original (w, h), final (w, h)); bytes is None when analyzeFormat chose PNG."""
        src = np.frombuffer(data, dtype=np.uint8)
        o = FileOptions(int(orient), int(max_w), int(max_h), 1 if auto_format else 0, float(target_ssim))
        cap = max(4096, len(data) + 4096)
        n, q, st, v = C.c_size_t(0), C.c_int(), C.c_int(), C.c_double()
        dims = (C.c_int * 4)()
        rc, buf = _into_buffer(lambda b, c: self._lib.fennec_CompressFileJPEG(self._h, src.ctypes.data_as(_u8p), len(data), C.byref(o),
                                                                              b.ctypes.data_as(_u8p), c, C.byref(n), C.byref(q), C.byref(v),
                                                                              C.byref(st), dims), cap, n)
        if rc == FNX_OK:
            return buf[:n.value].tobytes(), q.value, v.value, st.value, (dims[0], dims[1]), (dims[2], dims[3])
        if rc == FNX_NOOP:
            return None, 0, 1.0, 0, (dims[0], dims[1]), (dims[2], dims[3])
        self._chk(rc, "fennec_CompressFileJPEG")

    def compress_file_target_size(self, data: bytes, target_bytes: int, orient: int = 1, max_w: int = 0, max_h: int = 0,
                                  strategies: int = FNX_TS_ALL, cancel=None):
        """CompressFile for a JPEG or PNG source (the signature decides) in target-size mode, every pixel stage on the device
        (fennec_CompressFileTargetSize): decode, ApplyOrientation(orient), smartResize(max_w, max_h), hitTargetSize's JPEG
        strategies -> a dict: `data` (the winner's file, or None), `candidates` and `winner` as jpeg_target_size's, `dims`
        ((original w, h), (final w, h)) and `status` (FNX_OK / FNX_NOOP).  `cancel`: a ctypes.c_int, as jpeg_target_size's."""
        if cancel is not None and not isinstance(cancel, C.c_int):
            raise FennecError("compress_file_target_size: cancel must be a ctypes.c_int (or None)")
        src = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, dtype=np.uint8)
        o = TargetOptions.make(target_bytes, orient, max_w, max_h, strategies)
        cand = (SizeCandidate * 4)()
        win, n = C.c_int(-1), C.c_size_t(0)
        dims = (C.c_int * 4)()
        pc = C.byref(cancel) if cancel is not None else None
        # a winner within the target fits; one over it (the fallback, strategy 4's encode at bestQ) asks again with its size
        rc, buf = _into_buffer(lambda b, c: self._lib.fennec_CompressFileTargetSize(self._h, src.ctypes.data_as(_u8p), len(data), C.byref(o), pc,
                                                                                    cand, C.byref(win), b.ctypes.data_as(_u8p), c, C.byref(n),
                                                                                    dims), max(4096, int(target_bytes) + 4096), n)
        self._chk(rc, "fennec_CompressFileTargetSize")
        out = {"candidates": [c.as_dict() for c in cand], "winner": win.value if rc == FNX_OK else None,
               "data": buf[:n.value].tobytes() if rc == FNX_OK else None, "dims": ((dims[0], dims[1]), (dims[2], dims[3])), "status": rc}
        return out

    def jpeg_quality_search(self, img, target_ssim: float, window=None):
        """compressJPEGOptimal's binary search with every candidate round-tripped and scored on the device
        (fnx_jpeg_quality_search) -> (quality, ssim, steps, found)."""
        s = _Img(img)
        k, pk = _f64(self.gaussianKernel() if window is None else window)
        q, st, v = C.c_int(), C.c_int(), C.c_double()
        with self._ordered(img):
            rc = self._chk(self._lib.fnx_jpeg_quality_search(self._h, s.space, s.ptr, s.stride, s.w, s.h, float(target_ssim), pk,
                                                             C.byref(q), C.byref(v), C.byref(st)), "fnx_jpeg_quality_search")
        return q.value, v.value, st.value, rc == FNX_OK

    # -- effects.go ---------------------------------------------------------------------
    def GaussianBlur(self, img, sigma: float, exact: bool | None = False, kernel=None, keep_box_sums: bool = False):
        """effects.go:146.  sigma <= 0 returns `img` itself (same pointer).  exact=False: fast fp32 kernel
        (<= 1 LSB on <= 0.1 % of samples); exact=True: bit-exact fp64 kernels; exact=None: what the
        reference-named mirror fennec_GaussianBlur picks (exact for host images, fast for device tensors).
        keep_box_sums (device tensors, FNX_BLUR_KEEP_BOX_SUMS): the next call on this ctx is SSIMFast(img, result) and nothing
        writes either image in between -- that call then reads neither of them again."""
        if sigma <= 0:
            return img
        s = _Img(img)
        dst = s.like(s.w, s.h)
        d = _Img(dst)
        with self._ordered(img, dst):
            if kernel is None and exact is None:
                rc = self._lib.fennec_GaussianBlur(self._h, s.space, s.ptr, s.stride, s.w, s.h, float(sigma),
                                                   d.ptr, d.stride)
            else:
                if kernel is None:
                    radius, kernel = self.blurKernel(sigma)
                else:
                    radius = (len(kernel) - 1) // 2
                k, pk = _f64(kernel)
                rc = self._lib.fnx_gaussian_blur(self._h, s.space, s.ptr, s.stride, s.w, s.h, pk, radius,
                                                 (FNX_BLUR_EXACT if exact else FNX_BLUR_FAST) | (FNX_BLUR_KEEP_BOX_SUMS if keep_box_sums else 0),
                                                 d.ptr, d.stride)
            self._chk(rc, "GaussianBlur")
        return dst

    def GaussianBlurSSIMFast(self, img, sigma: float, exact: bool = True, window=None, out=None):
        """GaussianBlur(img, sigma) and SSIMFast(img, blurred) in ONE call (fnx_gaussian_blur_ssim_fast): a host image crosses
        PCIe once each way.  -> (blurred, ssim); the bytes and the score of the two separate calls.  out: the image to write
        (same kind and size as img) instead of a new one."""
        if sigma <= 0:
            raise FennecError("GaussianBlurSSIMFast: sigma <= 0 (GaussianBlur would return the image itself)")
        s = _Img(img)
        dst = s.like(s.w, s.h) if out is None else out
        d = _Img(dst)
        if (d.w, d.h, d.space) != (s.w, s.h, s.space):
            raise FennecError("GaussianBlurSSIMFast: out must be an image of img's size in img's memory space")
        radius, kernel = self.blurKernel(sigma)
        k, pk = _f64(kernel)
        wk, pw = _f64(self.gaussianKernel() if window is None else window)
        out = C.c_double()
        with self._ordered(img, dst):
            self._chk(self._lib.fnx_gaussian_blur_ssim_fast(self._h, s.space, s.ptr, s.stride, s.w, s.h, pk, radius,
                                                            FNX_BLUR_EXACT if exact else FNX_BLUR_FAST, d.ptr, d.stride, pw, C.byref(out)),
                      "GaussianBlurSSIMFast")
        return dst, float(out.value)

    def blur3x3(self, img):
        """effects.go:116 gaussianBlur3x3.  A strided / cropped view is a Go SubImage here (as for Sharpen / AdaptiveSharpen):
        borders and alpha come from the first 4*w*h flat bytes (effects.go:120), as in the reference; pass a contiguous copy
        for row-wise semantics."""
        s = _Img(img)
        dst = s.like(s.w, s.h)
        d = _Img(dst)
        with self._ordered(img, dst):
            self._chk(self._lib.fnx_blur3x3(self._h, s.space, s.ptr, s.stride, s.w, s.h, d.ptr, d.stride), "blur3x3")
        return dst

    def _sharpen(self, fn, name, img, strength):
        s = _Img(img)
        dst = s.like(s.w, s.h)
        d = _Img(dst)
        with self._ordered(img, dst):
            rc = self._chk(fn(self._h, s.space, s.ptr, s.stride, s.w, s.h, float(strength), d.ptr, d.stride), name)
        return img if rc == FNX_NOOP else dst

    def sharpen_amount(self, img, amount: float, adaptive: bool = False):
        """fnx_sharpen / fnx_adaptive_sharpen with the unsharp `amount` itself (1 + 1.5 s / 1 + 2 s in the
        reference, effects.go:24,63): the kernel-level entry points, for callers and tests."""
        s = _Img(img)
        dst = s.like(s.w, s.h)
        d = _Img(dst)
        fn = self._lib.fnx_adaptive_sharpen if adaptive else self._lib.fnx_sharpen
        with self._ordered(img, dst):
            self._chk(fn(self._h, s.space, s.ptr, s.stride, s.w, s.h, float(amount), d.ptr, d.stride), "sharpen_amount")
        return dst

    def Sharpen(self, img, strength: float):
        """effects.go:10.  strength <= 0 or an image under 3x3 returns `img` itself.  Strided views: see blur3x3."""
        return self._sharpen(self._lib.fennec_Sharpen, "Sharpen", img, strength)

    def AdaptiveSharpen(self, img, strength: float):
        """effects.go:49.  Strided views: see blur3x3."""
        return self._sharpen(self._lib.fennec_AdaptiveSharpen, "AdaptiveSharpen", img, strength)

    # -- resize.go ----------------------------------------------------------------------
    def lanczosResize(self, img, dstW: int, dstH: int, to_host: bool = False):
        """resize.go:37.  to_host: see boxDownsample."""
        s = _Img(img)
        if s.w <= 0 or s.h <= 0 or dstW <= 0 or dstH <= 0:
            return self._out_for(s, 0, 0, to_host)[1]
        space, dst = self._out_for(s, dstW, dstH, to_host)
        d = _Img(dst)
        with self._ordered(img, dst):
            self._chk(self._lib.fennec_lanczosResize(self._h, space, s.ptr, s.stride, s.w, s.h, d.ptr,
                                                     d.stride, dstW, dstH), "lanczosResize")
        return dst

    def lanczosResizeBatch(self, imgs, dstW: int, dstH: int, outs=None):
        """n same-sized device images through ONE set of launches (fennec_lanczosResizeBatch): the bytes of n lanczosResize
        calls; enqueued (sync() or a later blocking call waits)."""
        views = [_Img(t) for t in imgs]
        if not views or any(v.space != FNX_DEVICE for v in views):
            raise FennecError("lanczosResizeBatch takes a non-empty list of device tensors")
        v0 = views[0]
        if any((v.w, v.h, v.stride) != (v0.w, v0.h, v0.stride) for v in views):
            raise FennecError("every image of a batch must share width, height and stride")
        if v0.w <= 0 or v0.h <= 0 or dstW <= 0 or dstH <= 0:
            return [v0.like(0, 0) for _ in views]
        if outs is None:
            outs = [v0.like(dstW, dstH) for _ in views]
        ov = [_Img(t) for t in outs]
        if len(ov) != len(views) or any((o.w, o.h, o.stride, o.space) != (dstW, dstH, ov[0].stride, FNX_DEVICE) for o in ov):
            raise FennecError("outs must hold one device image of dstW x dstH per input, all of one stride")
        n = len(views)
        srcs = (C.c_void_p * n)(*[v.ptr for v in views])
        dsts = (C.c_void_p * n)(*[v.ptr for v in ov])
        with self._ordered(*imgs, *outs):
            self._chk(self._lib.fennec_lanczosResizeBatch(self._h, n, srcs, v0.stride, v0.w, v0.h, dsts, ov[0].stride, dstW, dstH),
                      "lanczosResizeBatch")
        return outs

    def smartResize(self, img, maxW: int, maxH: int):
        """resize.go:12.  Returns `img` itself when it already fits."""
        s = _Img(img)
        r, dw, dh = self.smartResizeDims(s.w, s.h, maxW, maxH)
        return self.lanczosResize(img, dw, dh) if r else img

    def resize_pass(self, img, dst_size: int, vertical: bool, table=None):
        """resizeH / resizeV (resize.go:77,121) with an explicit CSR tap table."""
        s = _Img(img)
        src_size = s.h if vertical else s.w
        off, idx, wt = table if table is not None else self.precomputeWeights(dst_size, src_size)
        off, po = _i32(off); idx, pi = _i32(idx); wt, pw = _f64(wt)
        dst = s.like(s.w, dst_size) if vertical else s.like(dst_size, s.h)
        d = _Img(dst)
        fn = self._lib.fnx_resize_v if vertical else self._lib.fnx_resize_h
        with self._ordered(img, dst):
            self._chk(fn(self._h, s.space, s.ptr, s.stride, s.w, s.h, po, pi, pw, d.ptr, d.stride, dst_size),
                      "resize_pass")
        return dst

    def lanczos_resize_tables(self, img, dst_w: int, dst_h: int, table_h, table_v):
        """fnx_lanczos_resize: lanczosResize (resize.go:37-53) with the CALLER's two CSR tap tables (what a Go caller
        passes: its own precomputeWeights output) -- both passes, one launch where the tables allow it."""
        s = _Img(img)
        oh, ih, wh = table_h
        ov, iv, wv = table_v
        oh, poh = _i32(oh); ih, pih = _i32(ih); wh, pwh = _f64(wh)
        ov, pov = _i32(ov); iv, piv = _i32(iv); wv, pwv = _f64(wv)
        dst = s.like(dst_w, dst_h)
        d = _Img(dst)
        with self._ordered(img, dst):
            self._chk(self._lib.fnx_lanczos_resize(self._h, s.space, s.ptr, s.stride, s.w, s.h, poh, pih, pwh, pov, piv, pwv,
                                                   d.ptr, d.stride, dst_w, dst_h), "fnx_lanczos_resize")
        return dst

    # -- exif.go ------------------------------------------------------------------------
    def ApplyOrientation(self, img, orient: int):
        """exif.go:178.  Orientation 0, 1 and unknown values return `img` itself."""
        orient = int(orient)
        if orient < 2 or orient > 8:
            return img
        s = _Img(img)
        ow, oh = (s.h, s.w) if orient >= 5 else (s.w, s.h)
        dst = s.like(ow, oh)
        d = _Img(dst)
        with self._ordered(img, dst):
            self._chk(self._lib.fennec_ApplyOrientation(self._h, s.space, s.ptr, s.stride, s.w, s.h, orient,
                                                        d.ptr, d.stride), "ApplyOrientation")
        return dst

    # -- Analyze (analyze.go) ---------------------------------------------------------------
    @staticmethod
    def _stats_dict(st: ImageStats) -> dict:
        return {name: getattr(st, name) for name, _ in ImageStats._fields_ if name != "pad"}

    @staticmethod
    def _analysis_dict(a: Analysis) -> dict:
        d = {name: getattr(a, name) for name, _ in Analysis._fields_ if name not in ("pad", "histogram")}
        d["histogram"] = np.array(a.histogram[:], dtype=np.uint64)
        return d

    def Analyze(self, img) -> dict:
        """Analyze (analyze.go:26-124) -> dict with the ImageStats field names."""
        v = _Img(img)
        st = ImageStats()
        with self._ordered(img):
            self._chk(self._lib.fennec_Analyze(self._h, v.space, v.ptr, v.stride, v.w, v.h, C.byref(st)), "Analyze")
        return self._stats_dict(st)

    def analyze_raw(self, img) -> dict:
        """fnx_analyze: the device-side accumulators (histogram, sums, counts)."""
        v = _Img(img)
        a = Analysis()
        with self._ordered(img):
            self._chk(self._lib.fnx_analyze(self._h, v.space, v.ptr, v.stride, v.w, v.h, C.byref(a)), "fnx_analyze")
        return self._analysis_dict(a)

    def plan_analyze_batch(self, imgs):
        """Pre-marshalled fnx_analyze_batch over n same-sized device images: run() -> list of ImageStats dicts."""
        views = self._batch_views(imgs)
        n, w, h, st = len(views), views[0].w, views[0].h, views[0].stride
        srcs = (C.c_void_p * n)(*[v.ptr for v in views])
        res = (Analysis * n)()
        ctx, lib = self, self._lib

        class _Plan:
            def __init__(p):
                p._keep = (imgs, srcs, res)
                p.raw = res

            def run(p):
                ctx._chk(lib.fnx_analyze_batch(ctx._h, n, srcs, st, w, h, res), "AnalyzeBatch")
                return res

            def stats(p):
                out = []
                for k in range(n):
                    s = ImageStats()
                    lib.fennec_statsFromAnalysis(C.byref(res[k]), w, h, C.byref(s))
                    out.append(ctx._stats_dict(s))
                return out
        return _Plan()

    def AnalyzeBatch(self, imgs):
        plan = self.plan_analyze_batch(imgs)
        plan.run()
        return plan.stats()

    def isOpaque(self, img) -> bool:
        v = _Img(img)
        o = C.c_int(0)
        with self._ordered(img):
            self._chk(self._lib.fennec_isOpaque(self._h, v.space, v.ptr, v.stride, v.w, v.h, C.byref(o)), "isOpaque")
        return bool(o.value)

    def isGrayscale(self, img) -> bool:
        v = _Img(img)
        o = C.c_int(0)
        with self._ordered(img):
            self._chk(self._lib.fennec_isGrayscale(self._h, v.space, v.ptr, v.stride, v.w, v.h, C.byref(o)), "isGrayscale")
        return bool(o.value)

    @staticmethod
    def _planes(y, cb, cr):
        """(space, y ptr/stride, cb ptr, cr ptr, cstride, w, h) of numpy or torch uint8 planes."""
        def view(p):
            if p is None:
                return None, 0, 0
            if _is_torch(p):
                return p.data_ptr(), int(p.stride(0)) if p.shape[0] > 1 else int(p.shape[1]), FNX_DEVICE
            return p.ctypes.data, int(p.strides[0]) if p.shape[0] > 1 else int(p.shape[1]), FNX_HOST
        yp, ys, space = view(y)
        cbp, cs, _ = view(cb)
        crp, cs2, _ = view(cr)
        if cb is not None and cs != cs2:
            raise FennecError("Cb and Cr must share a stride (image.YCbCr.CStride)")
        return space, yp, ys, cbp, crp, cs, int(y.shape[1]), int(y.shape[0])

    def ycbcrToNRGBA(self, y, cb, cr, ratio: int):
        """toNRGBARef of an image.YCbCr (convert.go:22-64); cb = cr = None: image.Gray.  Planes: 2-D uint8."""
        space, yp, ys, cbp, crp, cs, w, h = self._planes(y, cb, cr)
        if space == FNX_DEVICE:
            import torch
            dst = torch.empty((h, w, 4), dtype=torch.uint8, device=y.device)
        else:
            dst = np.empty((h, w, 4), dtype=np.uint8)
        d = _Img(dst)
        with self._ordered(y, cb, cr, dst):
            self._chk(self._lib.fnx_ycbcr_to_nrgba(self._h, space, yp, ys, cbp, crp, cs, int(ratio), w, h, d.ptr, d.stride),
                      "ycbcrToNRGBA")
        return dst

    def applyPalette(self, img, palette, want_quantized: bool = True):
        """applyPalette (targetsize.go:488-527) [+ palettedToNRGBA]: -> (indices (h, w) uint8,
        quantized (h, w, 4) or None).  palette: (n, 4) uint8, opaque."""
        v = _Img(img)
        pal = np.ascontiguousarray(palette, dtype=np.uint8).reshape(-1, 4)
        if v.space == FNX_DEVICE:
            import torch
            idx = torch.empty((v.h, v.w), dtype=torch.uint8, device=img.device)
            iptr, istride = idx.data_ptr(), v.w
        else:
            idx = np.empty((v.h, v.w), dtype=np.uint8)
            iptr, istride = idx.ctypes.data, v.w
        q = v.like(v.w, v.h) if want_quantized else None
        qv = _Img(q) if want_quantized else None
        with self._ordered(img, idx, q):
            self._chk(self._lib.fnx_apply_palette(self._h, v.space, v.ptr, v.stride, v.w, v.h, pal.ctypes.data, len(pal),
                                                  iptr, istride, qv.ptr if qv else None, qv.stride if qv else 0),
                      "applyPalette")
        return idx, q

    def median_cut(self, img, levels=(16, 32, 64, 128, 256)):
        """medianCut (targetsize.go:422-486; fnx_median_cut) at every palette size of `levels` (strictly ascending, 1..256) in one
        run -> a list of (ncolors, 4) uint8 arrays.  Tied samples split in the order they were taken (the library's tie rule: the
        reference's order is pdqsort's, so any is a reference answer).  img: tight rows."""
        v = _Img(img)
        lv = (C.c_int * len(levels))(*[int(c) for c in levels])
        pal = np.zeros((len(levels), 256, 4), dtype=np.uint8)
        n = (C.c_int * max(len(levels), 1))()
        with self._ordered(img):
            self._chk(self._lib.fnx_median_cut(self._h, v.space, v.ptr, v.stride, v.w, v.h, len(levels), lv, pal.ctypes.data, n),
                      "fnx_median_cut")
        return [pal[l, :n[l]].copy() for l in range(len(levels))]

    def quantize(self, img, max_colors: int, want_indices: bool = True, want_quantized: bool = True, want_ssim: bool = True, window=None):
        """One iteration of quantizeStrategy's loop (targetsize.go:183-205; fnx_quantize) without the PNG size test ->
        (palette (n, 4) uint8, indices (h, w) uint8, quantized (h, w, 4), ssim): medianCut at max_colors, applyPalette +
        palettedToNRGBA, SSIMFast(img, quantized).  An output not wanted is None."""
        v = _Img(img)
        idx = q = None
        iptr, qptr, qstride = None, None, 0
        if want_indices:
            if v.space == FNX_DEVICE:
                import torch
                idx = torch.empty((v.h, v.w), dtype=torch.uint8, device=img.device)
                iptr = idx.data_ptr()
            else:
                idx = np.empty((v.h, v.w), dtype=np.uint8)
                iptr = idx.ctypes.data
        if want_quantized:
            q = v.like(v.w, v.h)
            qv = _Img(q)
            qptr, qstride = qv.ptr, qv.stride
        win, winp = _f64(self.gaussianKernel() if window is None else window)
        pal = np.zeros((256, 4), dtype=np.uint8)
        n, out = C.c_int(0), C.c_double(0.0)
        with self._ordered(img, idx, q):
            self._chk(self._lib.fnx_quantize(self._h, v.space, v.ptr, v.stride, v.w, v.h, int(max_colors), pal.ctypes.data, C.byref(n),
                                             iptr, v.w, qptr, qstride, winp if want_ssim else None, C.byref(out) if want_ssim else None),
                      "fnx_quantize")
        return pal[:n.value].copy(), idx, q, (out.value if want_ssim else None)

    def png_reduce(self, img, max_colors: int = 256, want_plane: bool = True, plane=None):
        """compressPNG's decision and reduced image (compress.go:90-153; fnx_png_reduce) -> (kind, palette (n, 4) uint8, plane):
        FNX_PNG_PALETTED with tryPalettize's palette (first-occurrence order) and index plane, FNX_PNG_GRAY with toGray's
        plane, or FNX_PNG_NRGBA (plane None: the image is the image).  want_plane=False: classify only.  plane: an (h, >= w)
        uint8 array to write into (rows contiguous) -- numpy beside a device image is the device-source / host-plane form;
        it is returned as it is, and left untouched for FNX_PNG_NRGBA."""
        v = _Img(img)
        space = v.space
        pptr, pstride = None, 0
        if want_plane:
            if plane is None:
                if v.space == FNX_DEVICE:
                    import torch
                    plane = torch.empty((v.h, v.w), dtype=torch.uint8, device=img.device)
                else:
                    plane = np.empty((v.h, v.w), dtype=np.uint8)
            on_device = _is_torch(plane)
            if on_device and v.space != FNX_DEVICE:
                raise FennecError("a device plane needs a device image")
            if tuple(plane.shape[:1]) != (v.h,) or plane.ndim != 2 or plane.shape[1] < v.w:
                raise FennecError("plane must be (h, >= w) uint8")
            if on_device:
                pptr, pstride = plane.data_ptr(), int(plane.stride(0)) if v.h > 1 else int(plane.shape[1])
                ok = plane.stride(1) == 1
            else:
                pptr, pstride = plane.ctypes.data, int(plane.strides[0]) if v.h > 1 else int(plane.shape[1])
                ok = plane.dtype == np.uint8 and plane.strides[1] == 1
                if v.space == FNX_DEVICE:
                    space = FNX_DEVICE_SRC
            if not ok:
                raise FennecError("plane rows must be contiguous uint8")
        kind, n = C.c_int(0), C.c_int(0)
        pal = np.zeros((256, 4), dtype=np.uint8)
        with self._ordered(img, plane if want_plane and _is_torch(plane) else None):
            self._chk(self._lib.fnx_png_reduce(self._h, space, v.ptr, v.stride, v.w, v.h, int(max_colors), C.byref(kind),
                                               pal.ctypes.data, C.byref(n), pptr, pstride),
                      "fnx_png_reduce")
        out = plane if want_plane and kind.value != FNX_PNG_NRGBA else None
        return kind.value, pal[:n.value].copy(), out

    def tryPalettize(self, img, max_colors: int = 256):
        """tryPalettize (compress.go:112-153) -> (palette (n, 4), indices (h, w)), or None when the image holds more than
        max_colors colours.  The palette is in first-occurrence order (the reference's is a Go map's: any order)."""
        v = _Img(img)
        if v.space == FNX_DEVICE:
            import torch
            keep = torch.empty((v.h, v.w), dtype=torch.uint8, device=img.device)
        else:
            keep = np.empty((v.h, v.w), dtype=np.uint8)
        kind, pal, plane = self.png_reduce(img, max_colors, True, keep)
        return (pal, plane) if kind == FNX_PNG_PALETTED else None

    def compress_file_png_reduce(self, data: bytes, orient: int = 1, max_w: int = 0, max_h: int = 0, cap: int | None = None):
        """CompressFile's PNG branch for a JPEG source up to the encoder (fennec_CompressFilePNGReduce): decode,
        ApplyOrientation(orient), smartResize(max_w, max_h), then compressPNG's reduction on the resident image ->
        (kind, palette (n, 4), image, original (w, h), final (w, h)); image: (h, w) uint8 indices or grays, or (h, w, 4) NRGBA."""
        src = np.frombuffer(data, dtype=np.uint8)
        o = FileOptions(int(orient), int(max_w), int(max_h), 0, 0.0)
        kind, nc, n = C.c_int(0), C.c_int(0), C.c_size_t(0)
        pal = np.zeros((256, 4), dtype=np.uint8)
        dims = (C.c_int * 4)()
        rc, buf = _into_buffer(lambda b, c: self._lib.fennec_CompressFilePNGReduce(self._h, src.ctypes.data_as(_u8p), len(data), C.byref(o),
                                                                                   C.byref(kind), pal.ctypes.data, C.byref(nc),
                                                                                   b.ctypes.data_as(_u8p), c, C.byref(n), dims),
                               1 << 16 if cap is None else int(cap), n)
        self._chk(rc, "fennec_CompressFilePNGReduce")
        w, h = dims[2], dims[3]
        image = buf[:n.value].reshape((h, w, 4) if kind.value == FNX_PNG_NRGBA else (h, w))
        return kind.value, pal[:nc.value].copy(), image, (dims[0], dims[1]), (w, h)

    @staticmethod
    def _png_src(src, kind):
        """(kind, space, pointer, stride, w, h) of png_filter's / png_encode's source: an (h, w, 4) image or an (h, w) plane"""
        torch_src = _is_torch(src)
        if src.ndim == 3:
            v = _Img(src)
            kind = FNX_PNG_NRGBA if kind is None else kind
            if kind != FNX_PNG_NRGBA:
                raise FennecError("an (h, w, 4) image is FNX_PNG_NRGBA")
            space, ptr, stride, w, h = v.space, v.ptr, v.stride, v.w, v.h
        else:
            kind = FNX_PNG_GRAY if kind is None else kind
            if kind not in (FNX_PNG_GRAY, FNX_PNG_PALETTED) or src.ndim != 2:
                raise FennecError("an (h, w) plane is FNX_PNG_GRAY or FNX_PNG_PALETTED")
            h, w = int(src.shape[0]), int(src.shape[1])
            if torch_src:
                import torch
                if not src.is_cuda or src.dtype != torch.uint8 or (w > 0 and src.stride(1) != 1):
                    raise FennecError("device planes must be uint8 CUDA/HIP tensors with contiguous rows")
                space, ptr, stride = FNX_DEVICE, src.data_ptr(), int(src.stride(0)) if h > 1 else w
            else:
                if not isinstance(src, np.ndarray) or src.dtype != np.uint8 or (w > 0 and src.strides[1] != 1):
                    raise FennecError("host planes must be numpy uint8 arrays with contiguous rows")
                space, ptr, stride = FNX_HOST, src.ctypes.data, int(src.strides[0]) if h > 1 else w
        return kind, space, ptr, stride, w, h

    @staticmethod
    def _flat_out(out, space):
        """(pointer, space of the call) for png_filter's / deflate's `out`, a flat uint8 buffer: a device tensor (device sources
        only) or a numpy array, which a device source fills through FNX_DEVICE_SRC"""
        on_device = _is_torch(out)
        if on_device and space != FNX_DEVICE:
            raise FennecError("a device stream needs a device source")
        if out.ndim != 1 or not (out.is_contiguous() if on_device else (out.dtype == np.uint8 and out.flags.c_contiguous)):
            raise FennecError("out must be a flat contiguous uint8 buffer")
        return (out.data_ptr() if on_device else out.ctypes.data), (space if on_device or space == FNX_HOST else FNX_DEVICE_SRC)

    def png_filter(self, src, kind: int | None = None, ncolors: int = 0, opaque: int = -1, out=None):
        """The PNG encoder's row stage (fnx_png_filter; compress.go:94-107) -> (stream (h, 1 + n) uint8, color_type, bit_depth):
        every row packed, filtered by the cheapest of the five PNG filters and led by its type byte -- the bytes zlib reads.
        src: an (h, w, 4) NRGBA image (kind FNX_PNG_NRGBA; opaque 1 / 0 states whether RGB or RGBA rows are written, -1 decides
        as image.NRGBA.Opaque() does) or an (h, w) uint8 plane: toGray's (FNX_PNG_GRAY, the default for a plane) or an index
        plane (FNX_PNG_PALETTED with ncolors, which sets the bit depth).  numpy in, numpy out; a device tensor gives a device
        tensor, or fills `out` -- a flat uint8 numpy array (the device-source / host-stream form) or device tensor of at least
        h * (1 + n) bytes, of which the stream's bytes are returned as an (h, 1 + n) view."""
        kind, space, ptr, stride, w, h = self._png_src(src, kind)
        n, ct, bd = C.c_size_t(0), C.c_int(0), C.c_int(0)

        def call(sp, optr, cap):
            return self._lib.fnx_png_filter(self._h, sp, int(kind), ptr, stride, w, h, int(ncolors), int(opaque), optr, cap, C.byref(n),
                                            C.byref(ct), C.byref(bd))
        if out is not None:
            optr, sp = self._flat_out(out, space)
            with self._ordered(src, out):
                self._chk(call(sp, optr, int(out.shape[0])), "fnx_png_filter")
            return out[:n.value].reshape(h, n.value // h), ct.value, bd.value
        # one call: an image whose opacity the call itself finds gets room for RGBA rows, and the stream is a view of its front
        cap = h * (1 + (4 * w if kind == FNX_PNG_NRGBA and opaque != 1 else 3 * w if kind == FNX_PNG_NRGBA else w))
        with self._ordered(src):
            if space == FNX_DEVICE:
                import torch
                buf = torch.empty(cap, dtype=torch.uint8, device=src.device)
                optr = buf.data_ptr()
            else:
                buf = np.empty(cap, dtype=np.uint8)
                optr = buf.ctypes.data
            self._chk(call(space, optr, cap), "fnx_png_filter")
        return buf[:n.value].reshape(h, n.value // h), ct.value, bd.value

    def compress_png(self, img, level: int = 9, device_deflate: bool = False) -> bytes:
        """compressPNG (compress.go:90-108) end to end -> the PNG file: the reduction (png_reduce), the encoder's row stage
        (png_filter) on the reduced image where it lives, then zlib and the chunks on the host (png_file).  The file differs
        from Go's in the deflate bytes only (Python's zlib is not Go's compress/flate) and decodes to the same pixels.
        device_deflate=True: the row stage and the deflate on the device (png_encode; `level` does not apply) -- a larger
        file, no scanline on the host."""
        v = _Img(img)
        kind, pal, plane = self.png_reduce(img)
        src = img if kind == FNX_PNG_NRGBA else plane
        if device_deflate:
            return self.png_encode(src, kind, len(pal), -1, pal if kind == FNX_PNG_PALETTED else None)
        host = np.empty(v.h * (1 + (4 * v.w if kind == FNX_PNG_NRGBA else v.w)), dtype=np.uint8) if v.space == FNX_DEVICE else None
        stream, ct, bd = self.png_filter(src, kind, len(pal), -1, host)
        return png_file(stream, v.w, v.h, ct, bd, pal if kind == FNX_PNG_PALETTED else None, level)

    def deflate(self, buf, row: int = 0, out=None):
        """The zlib stream of `buf` (fnx_deflate; deflate.hip): independent chunks of FNX_DEFLATE_CHUNK bytes, one workgroup
        and one deflate block each; zlib.decompress reads it back.  buf: bytes or a flat uint8 numpy array -> bytes; a flat
        uint8 device tensor -> a device tensor (the front of a buffer of deflate_bound(len) bytes), or fills `out`: a flat
        uint8 numpy array (device source, host stream) or device tensor, of which the stream's bytes are returned as a view.
        row: the stream's row length (1 + n of png_filter) as a match-distance hint, 0 for none."""
        if _is_torch(buf):
            import torch
            if not buf.is_cuda or buf.dtype != torch.uint8 or buf.dim() != 1 or not buf.is_contiguous():
                raise FennecError("a device buffer must be a flat contiguous uint8 CUDA/HIP tensor")
            space, ptr, n, keep = FNX_DEVICE, buf.data_ptr(), int(buf.shape[0]), buf
        else:
            keep = np.frombuffer(buf, dtype=np.uint8) if isinstance(buf, (bytes, bytearray, memoryview)) else buf
            if not isinstance(keep, np.ndarray) or keep.dtype != np.uint8 or keep.ndim != 1 or not keep.flags.c_contiguous:
                raise FennecError("a host buffer must be bytes or a flat contiguous uint8 numpy array")
            space, ptr, n = FNX_HOST, keep.ctypes.data, int(keep.shape[0])
        if n < 1:
            raise FennecError("deflate takes at least one byte")
        size = C.c_size_t(0)
        if out is None:
            cap = int(self._lib.fnx_deflate_bound(n))
            if space == FNX_DEVICE:
                import torch
                out = torch.empty(cap, dtype=torch.uint8, device=buf.device)
            else:
                out = np.empty(cap, dtype=np.uint8)
            fresh = True
        else:
            fresh = False
        on_device = _is_torch(out)
        optr, sp = self._flat_out(out, space)
        with self._ordered(buf if space == FNX_DEVICE else None, out if on_device else None):
            self._chk(self._lib.fnx_deflate(self._h, sp, ptr, n, int(row), optr, int(out.shape[0]), C.byref(size)), "fnx_deflate")
        view = out[:size.value]
        return view.tobytes() if fresh and not on_device else view

    def crc32(self, data, crc: int = 0) -> int:
        """zlib.crc32(data, crc) on the device (fnx_crc32; crc32.hip): data is bytes or a flat uint8 numpy array (uploaded
        first) or a flat uint8 device tensor (read where it lies, at any alignment); crc the CRC of what came before."""
        if _is_torch(data):
            import torch
            if not data.is_cuda or data.dtype != torch.uint8 or data.dim() != 1 or not data.is_contiguous():
                raise FennecError("a device buffer must be a flat contiguous uint8 CUDA/HIP tensor")
            space, ptr, n, keep = FNX_DEVICE, data.data_ptr(), int(data.shape[0]), data
        else:
            keep = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else data
            if not isinstance(keep, np.ndarray) or keep.dtype != np.uint8 or keep.ndim != 1 or not keep.flags.c_contiguous:
                raise FennecError("a host buffer must be bytes or a flat contiguous uint8 numpy array")
            space, ptr, n = FNX_HOST, keep.ctypes.data, int(keep.shape[0])
        out = C.c_uint32(0)
        with self._ordered(keep if space == FNX_DEVICE else None):
            self._chk(self._lib.fnx_crc32(self._h, space, ptr if n else None, n, int(crc) & 0xffffffff, C.byref(out)), "fnx_crc32")
        return int(out.value)

    def png_encode(self, src, kind: int | None = None, ncolors: int = 0, opaque: int = -1, palette=None) -> bytes:
        """The complete PNG file of `src` (fnx_png_encode): png_filter's row stage and the deflate on the device, the chunks
        (signature, IHDR, PLTE and tRNS for paletted kinds, one IDAT, IEND: png_file's layout) and their CRCs on the host.
        src, kind, ncolors, opaque: as png_filter's; palette: (ncolors, 4) r,g,b,a for FNX_PNG_PALETTED."""
        kind, space, ptr, stride, w, h = self._png_src(src, kind)
        pal = None
        if kind == FNX_PNG_PALETTED:
            if palette is None:
                raise FennecError("a paletted image needs its palette")
            pal = np.ascontiguousarray(palette, dtype=np.uint8).reshape(-1, 4)
            ncolors = ncolors or len(pal)
            if len(pal) < ncolors:
                raise FennecError("the palette is shorter than ncolors")
        n = C.c_size_t(0)
        sp = FNX_DEVICE_SRC if space == FNX_DEVICE else FNX_HOST
        with self._ordered(src):
            rc, buf = _into_buffer(lambda b, c: self._lib.fnx_png_encode(self._h, sp, int(kind), ptr, stride, w, h, int(ncolors), int(opaque),
                                                                         pal.ctypes.data if pal is not None else None,
                                                                         b.ctypes.data, c, C.byref(n)),
                                   max(1 << 16, (w * h) // 2), n)
            self._chk(rc, "fnx_png_encode")
        return buf[:n.value].tobytes()

    def png_encoded_size(self, src, kind: int | None = None, ncolors: int = 0, opaque: int = -1, palette=None) -> int:
        """len(png_encode(...)) of the same arguments on this context without the file (fnx_png_encoded_size): the row stage,
        then the deflate kernels' size-only forms -- the parse and the choice of block form, no codes, no bits, no gather --
        and 8 bytes back.  palette: needed for FNX_PNG_PALETTED as png_encode needs it (its alphas size the tRNS chunk)."""
        kind, space, ptr, stride, w, h = self._png_src(src, kind)
        pal = None
        if kind == FNX_PNG_PALETTED:
            if palette is None:
                raise FennecError("a paletted image needs its palette")
            pal = np.ascontiguousarray(palette, dtype=np.uint8).reshape(-1, 4)
            ncolors = ncolors or len(pal)
            if len(pal) < ncolors:
                raise FennecError("the palette is shorter than ncolors")
        n = C.c_size_t(0)
        sp = FNX_DEVICE_SRC if space == FNX_DEVICE else FNX_HOST
        with self._ordered(src):
            self._chk(self._lib.fnx_png_encoded_size(self._h, sp, int(kind), ptr, stride, w, h, int(ncolors), int(opaque),
                                                     pal.ctypes.data if pal is not None else None, C.byref(n)), "fnx_png_encoded_size")
        return int(n.value)

    def png_decode_config(self, data: bytes):
        """png.DecodeConfig as far as the device decoder goes: (w, h); FennecUnsupported for files it does not take (Adam7,
        a dimension above 65535), FennecError for damaged ones.  Host work only."""
        buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, dtype=np.uint8)
        w, h = C.c_int(), C.c_int()
        self._chk(self._lib.fnx_png_decode(self._h, buf.ctypes.data_as(_u8p), len(data), FNX_HOST, None, 0, C.byref(w), C.byref(h)),
                  "fnx_png_decode")
        return w.value, h.value

    def png_decode(self, data: bytes, space: str = "device", out=None):
        """toNRGBA(image.Decode(data)) for a PNG file (fnx_png_decode): chunk walk and inflate on the host, the row filters'
        inverse and the pixel conversion on the device.  space="device": a torch tensor on the ctx's device; "host": an
        (h, w, 4) uint8 array.  out: the destination instead of a fresh one (an (h, w, 4) view, rows may be strided)."""
        if space not in ("device", "host"):
            raise FennecError('space is "device" or "host"')
        w, h, _, _, interlace = png_info(data)             # IHDR alone: the call below walks the file, once
        if (interlace and not self._png_adam7) or w > 65535 or h > 65535:
            raise FennecUnsupported("fnx_png_decode: Adam7 interlace or a dimension above 65535 -- decode it on the host")
        buf = np.frombuffer(data, dtype=np.uint8)
        if out is not None:
            dst = out
        elif space == "device":
            import torch
            dst = torch.empty((h, w, 4), dtype=torch.uint8, device=f"cuda:{self.device}")
        else:
            dst = np.empty((h, w, 4), dtype=np.uint8)
        d = _Img(dst)
        if (d.w, d.h) != (w, h):
            raise FennecError(f"out is {d.w} x {d.h}, the file {w} x {h}")
        with self._ordered(dst):
            self._chk(self._lib.fnx_png_decode(self._h, buf.ctypes.data_as(_u8p), len(data), d.space, d.ptr, d.stride, C.byref(C.c_int()),
                                               C.byref(C.c_int())), "fnx_png_decode")
        return dst

    def png_decode_batch(self, files, device: bool = False, workers: int = 0):
        """toNRGBA(image.Decode(f)) of every PNG file of a list in one call (fnx_png_decode_batch: the files' host side on
        `workers` threads -- 0: min(8, files in a chunk) --, then one set of launches per chunk) -> (images, statuses).
        images[i] is an (h, w, 4) uint8 array -- with device=True a torch tensor on the ctx's device -- and what
        png_decode(files[i]) returns, or None where statuses[i] != FNX_OK."""
        import torch
        files = [bytes(f) for f in files]
        n = len(files)
        if n == 0:
            raise FennecError("png_decode_batch takes a non-empty list of files")
        bufs = [np.frombuffer(f, dtype=np.uint8) if len(f) else np.zeros(1, dtype=np.uint8) for f in files]
        dsts = []
        for f in files:                                   # a file whose header does not parse goes in with no destination
            try:
                w, h, _, _, interlace = png_info(f)
                if (interlace and not self._png_adam7) or w > 65535 or h > 65535:   # refused by the call; no memory is sized by such a header
                    dsts.append(None)
                else:
                    dsts.append(torch.empty((h, w, 4), dtype=torch.uint8, device=f"cuda:{self.device}"))
            except FennecError:
                dsts.append(None)
        views = [None if t is None else _Img(t) for t in dsts]
        pf = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
        ps = (C.c_size_t * n)(*[len(f) for f in files])
        pd = (C.c_void_p * n)(*[None if v is None else v.ptr for v in views])
        pst = (C.c_int * n)(*[0 if v is None else v.stride for v in views])
        ws, hs, status = (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)()
        with self._ordered(*[t for t in dsts if t is not None]):
            self._chk(self._lib.fnx_png_decode_batch(self._h, n, pf, ps, pd, pst, int(workers), ws, hs, status), "fnx_png_decode_batch")
            images = [dsts[i] if status[i] == FNX_OK else None for i in range(n)]
            if not device:
                images = [None if t is None else t.cpu().numpy() for t in images]
        return images, list(status)

    def png_compress_batch(self, imgs):
        """compressPNG of a list of device images in one call (fnx_png_compress_batch: one set of launches and three host waits
        per chunk of up to FNX_PNG_COMPRESS_CHUNK images) -> (files, kinds).  files[i] is, byte for byte, what
        compress_png(imgs[i], device_deflate=True) returns; kinds[i] its FNX_PNG_* kind.  The images are (h, w, 4) uint8 device
        tensors and may differ in size, stride and content."""
        imgs = list(imgs)
        n = len(imgs)
        if n == 0:
            raise FennecError("png_compress_batch takes a non-empty list of images")
        views = [_Img(t) for t in imgs]
        if any(v.space != FNX_DEVICE for v in views):
            raise FennecError("png_compress_batch takes device images")
        bufs = [np.empty(int(self._lib.fnx_png_file_bound(v.w, v.h)), dtype=np.uint8) for v in views]
        ps = (C.c_void_p * n)(*[v.ptr for v in views])
        pst = (C.c_int * n)(*[v.stride for v in views])
        pw = (C.c_int * n)(*[v.w for v in views])
        ph = (C.c_int * n)(*[v.h for v in views])
        po = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
        pc = (C.c_size_t * n)(*[len(b) for b in bufs])
        nb, kinds, status = (C.c_size_t * n)(), (C.c_int * n)(), (C.c_int * n)()
        with self._ordered(*imgs):
            self._chk(self._lib.fnx_png_compress_batch(self._h, n, ps, pst, pw, ph, po, pc, nb, kinds, status), "fnx_png_compress_batch")
        for i in range(n):
            if status[i] != FNX_OK:
                self._chk(status[i], f"fnx_png_compress_batch: image {i}")
        return [bufs[i][:nb[i]].tobytes() for i in range(n)], list(kinds)

    def png_recompress_batch(self, files, workers: int = 0):
        """CompressBatch's item body for files that end as PNG (fnx_png_recompress_batch): PNG and JPEG files decoded by the
        batched decoders into device images, then png_compress_batch's launches -> (files, kinds, statuses).  files[i] is what
        compress_png(png_decode(f) or jpeg_decode(f), device_deflate=True) returns, or None where statuses[i] != FNX_OK (the
        decoder's answer for a file it refused)."""
        files = [bytes(f) for f in files]
        n = len(files)
        if n == 0:
            raise FennecError("png_recompress_batch takes a non-empty list of files")
        srcs = [np.frombuffer(f, dtype=np.uint8) if len(f) else np.zeros(1, dtype=np.uint8) for f in files]
        caps = []
        for f in files:                                   # a file whose header does not parse is refused by the call: no room
            w = h = 0
            try:
                if f[:8] == b"\x89PNG\r\n\x1a\n":
                    w, h = png_info(f)[:2]
                else:
                    w, h = self.jpeg_decode_config(f)
            except FennecError:
                pass
            caps.append(int(self._lib.fnx_png_file_bound(w, h)) if 1 <= w <= 65535 and 1 <= h <= 65535 else 0)
        bufs = [np.empty(max(c, 1), dtype=np.uint8) for c in caps]
        pf = (C.c_void_p * n)(*[b.ctypes.data for b in srcs])
        ps = (C.c_size_t * n)(*[len(f) for f in files])
        po = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
        pc = (C.c_size_t * n)(*caps)
        nb, kinds, ws, hs, status = (C.c_size_t * n)(), (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)()
        self._chk(self._lib.fnx_png_recompress_batch(self._h, n, pf, ps, int(workers), po, pc, nb, kinds, ws, hs, status),
                  "fnx_png_recompress_batch")
        out = [bufs[i][:nb[i]].tobytes() if status[i] == FNX_OK else None for i in range(n)]
        return out, list(kinds), list(status)

    def compress_file_png(self, data: bytes, orient: int = 1, max_w: int = 0, max_h: int = 0, cap: int | None = None):
        """CompressFile's PNG branch for a JPEG source in one call (fennec_CompressFilePNG): decode, ApplyOrientation(orient),
        smartResize(max_w, max_h), compressPNG's reduction, the encoder's row stage and the deflate on the device ->
        (PNG file bytes, kind, original (w, h), final (w, h))."""
        src = np.frombuffer(data, dtype=np.uint8)
        o = FileOptions(int(orient), int(max_w), int(max_h), 0, 0.0)
        kind, n = C.c_int(0), C.c_size_t(0)
        dims = (C.c_int * 4)()
        rc, buf = _into_buffer(lambda b, c: self._lib.fennec_CompressFilePNG(self._h, src.ctypes.data_as(_u8p), len(data), C.byref(o),
                                                                             b.ctypes.data_as(_u8p), c, C.byref(n), dims, C.byref(kind)),
                               1 << 16 if cap is None else int(cap), n)
        self._chk(rc, "fennec_CompressFilePNG")
        return buf[:n.value].tobytes(), kind.value, (dims[0], dims[1]), (dims[2], dims[3])

    def compress_file_png_stream(self, data: bytes, orient: int = 1, max_w: int = 0, max_h: int = 0, cap: int | None = None):
        """CompressFile's PNG branch for a JPEG source up to the bytes deflate reads (fennec_CompressFilePNGStream): decode,
        ApplyOrientation(orient), smartResize(max_w, max_h), compressPNG's reduction, the encoder's row stage ->
        (kind, palette (n, 4), stream (h, 1 + n) uint8, color_type, bit_depth, original (w, h), final (w, h))."""
        src = np.frombuffer(data, dtype=np.uint8)
        o = FileOptions(int(orient), int(max_w), int(max_h), 0, 0.0)
        kind, nc, ct, bd, n = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_size_t(0)
        pal = np.zeros((256, 4), dtype=np.uint8)
        dims = (C.c_int * 4)()
        rc, buf = _into_buffer(lambda b, c: self._lib.fennec_CompressFilePNGStream(self._h, src.ctypes.data_as(_u8p), len(data), C.byref(o),
                                                                                   C.byref(kind), pal.ctypes.data, C.byref(nc), C.byref(ct),
                                                                                   C.byref(bd), b.ctypes.data_as(_u8p), c, C.byref(n), dims),
                               1 << 16 if cap is None else int(cap), n)
        self._chk(rc, "fennec_CompressFilePNGStream")
        w, h = dims[2], dims[3]
        return (kind.value, pal[:nc.value].copy(), buf[:n.value].reshape(h, n.value // h), ct.value, bd.value, (dims[0], dims[1]), (w, h))

    # -- batched forms (device tensors) ---------------------------------------------------
    # Contract of the plan_* objects: creating a plan synchronises torch's current stream once (the inputs
    # exist from then on); run() / enqueue() only touch the stream the ctx launches on (its own unless a per-image
    # device call lent it torch's; use_own_stream() goes back), fetch() / run() of the scoring plans
    # block until the results -- and therefore every kernel queued before them -- are complete.  A caller
    # that rewrites the input tensors with torch between two runs must order that itself (ctx.sync() /
    # torch.cuda.synchronize()).  The convenience wrappers (GaussianBlurBatch, ...) order both ways.
    @staticmethod
    def _batch_views(imgs, what="images"):
        """_Img views of n device tensors that share (w, h, stride, device); raises FennecError otherwise."""
        views = [_Img(t) for t in imgs]
        if not views:
            raise FennecError(f"{what}: empty batch")
        if any(v.space != FNX_DEVICE for v in views):
            raise FennecError("batched ops take device tensors")
        v0 = views[0]
        for k, v in enumerate(views):
            if (v.w, v.h, v.stride) != (v0.w, v0.h, v0.stride) or v.obj.device != v0.obj.device:
                raise FennecError(f"{what}[{k}]: every image of a batch must share width, height, stride and device "
                                  f"(got {v.w}x{v.h} stride {v.stride} on {v.obj.device}, "
                                  f"expected {v0.w}x{v0.h} stride {v0.stride} on {v0.obj.device})")
        import torch
        torch.cuda.current_stream(v0.obj.device).synchronize()
        return views

    def GaussianBlurBatch(self, imgs, sigma: float, outs=None, exact: bool = False):
        """n same-sized device images, one launch per stage (enqueued; call sync() to wait)."""
        if sigma <= 0:
            return list(imgs)
        with self._ordered(*imgs):
            plan = self.plan_blur_batch(imgs, sigma, outs=outs, exact=exact)
            plan.run()
        return plan.outs

    def plan_blur_batch(self, imgs, sigma: float, outs=None, exact: bool = False, keep_box_sums: bool = False):
        """Pre-marshal a batched blur (pointer tables, kernel) so that run() is one C call --
        lets a caller bracket the launch tightly with events.  keep_box_sums (FNX_BLUR_KEEP_BOX_SUMS): the caller's next call on
        this ctx is the SSIMFast batch over (imgs[i], outs[i]) and nothing writes the images in between -- that call then reads
        neither full-size image again."""
        views = self._batch_views(imgs)
        w, h, st = views[0].w, views[0].h, views[0].stride
        if outs is None:
            outs = [views[0].like(w, h) for _ in views]
        oviews = self._batch_views(outs, "outs")
        n = len(views)
        if len(oviews) != n or (oviews[0].w, oviews[0].h) != (w, h):
            raise FennecError("outs must hold one image of the inputs' size per input")
        srcs = (C.c_void_p * n)(*[v.ptr for v in views])
        dsts = (C.c_void_p * n)(*[v.ptr for v in oviews])
        radius, kernel = self.blurKernel(sigma)
        k, pk = _f64(kernel)
        flags = (FNX_BLUR_EXACT if exact else FNX_BLUR_FAST) | (FNX_BLUR_KEEP_BOX_SUMS if keep_box_sums else 0)
        ctx, lib, ost = self, self._lib, oviews[0].stride

        class _Plan:
            def __init__(p):
                p.outs = outs
                p._keep = (imgs, outs, srcs, dsts, k)

            def run(p):
                ctx._chk(lib.fnx_gaussian_blur_batch(ctx._h, n, srcs, st, w, h, pk, radius, flags, dsts, ost),
                         "GaussianBlurBatch")
        return _Plan()

    def plan_ssim_fast_batch(self, imgs_a, imgs_b, window=None):
        """Pre-marshalled SSIMFastBatch: run() -> numpy array of n SSIM values (synchronises)."""
        va = self._batch_views(imgs_a, "imgs_a")
        vb = self._batch_views(imgs_b, "imgs_b")
        n = len(va)
        if n != len(vb) or (va[0].w, va[0].h) != (vb[0].w, vb[0].h):
            raise FennecError("batched ops take two equally long lists of equally sized device tensors")
        as_ = (C.c_void_p * n)(*[v.ptr for v in va])
        bs_ = (C.c_void_p * n)(*[v.ptr for v in vb])
        k, pk = _f64(self.gaussianKernel() if window is None else window)
        out = np.empty(n, dtype=np.float64)
        po = out.ctypes.data_as(_f64p)
        ctx, lib = self, self._lib
        sa, sb, w, h = va[0].stride, vb[0].stride, va[0].w, va[0].h

        class _Plan:
            def __init__(p):
                p._keep = (imgs_a, imgs_b, as_, bs_, k, out)

            def run(p):
                ctx._chk(lib.fnx_ssim_fast_batch(ctx._h, n, as_, sa, bs_, sb, w, h, pk, po), "SSIMFastBatch")
                return out

            def enqueue(p):
                """Queue the kernels only; results stay on the device until fetch()."""
                ctx._chk(lib.fnx_ssim_fast_batch_enqueue(ctx._h, n, as_, sa, bs_, sb, w, h, pk), "SSIMFastBatch")

            def fetch(p):
                ctx._chk(lib.fnx_results_fetch(ctx._h, n, po), "fnx_results_fetch")
                return out
        return _Plan()

    def SSIMFastBatch(self, imgs_a, imgs_b, window=None) -> np.ndarray:
        return self.plan_ssim_fast_batch(imgs_a, imgs_b, window).run().copy()

    def plan_blur_ssim_fast_batch(self, imgs, sigma: float, outs=None, exact: bool = False, window=None,
                                  kernel=None):
        """Pre-marshalled `outs[i] = GaussianBlur(imgs[i], sigma); ssim[i] = SSIMFast(imgs[i], outs[i])`
        in one pass over the pixels (fnx_gaussian_blur_ssim_fast_batch).  run() -> numpy array of n
        SSIM values (synchronises); enqueue()/fetch() split it.  exact=True: the blurred images are
        bit-exact (guarded kernel) and so are the planes the score is computed from.  `kernel` replaces
        blurKernel(sigma) with a caller-supplied odd-length 1-D kernel."""
        if sigma <= 0:
            raise FennecError("sigma <= 0 returns the source itself (effects.go:147): nothing to plan")
        views = self._batch_views(imgs)
        w, h, st = views[0].w, views[0].h, views[0].stride
        if outs is None:
            outs = [views[0].like(w, h) for _ in views]
        oviews = self._batch_views(outs, "outs")
        n = len(views)
        if len(oviews) != n or (oviews[0].w, oviews[0].h) != (w, h):
            raise FennecError("outs must hold one image of the inputs' size per input")
        srcs = (C.c_void_p * n)(*[v.ptr for v in views])
        dsts = (C.c_void_p * n)(*[v.ptr for v in oviews])
        if kernel is None:
            radius, kernel = self.blurKernel(sigma)
        else:
            kernel = np.asarray(kernel, dtype=np.float64)
            if kernel.ndim != 1 or len(kernel) % 2 == 0:
                raise FennecError("kernel must be a 1-D array of odd length")
            radius = len(kernel) // 2
        k, pk = _f64(kernel)
        kw, pw = _f64(self.gaussianKernel() if window is None else window)
        flags = FNX_BLUR_EXACT if exact else FNX_BLUR_FAST
        out = np.empty(n, dtype=np.float64)
        po = out.ctypes.data_as(_f64p)
        ctx, lib, ost = self, self._lib, oviews[0].stride

        class _Plan:
            def __init__(p):
                p.outs = outs
                p._keep = (imgs, outs, srcs, dsts, k, kw, out)

            def run(p):
                ctx._chk(lib.fnx_gaussian_blur_ssim_fast_batch(ctx._h, n, srcs, st, w, h, pk, radius, flags,
                                                               dsts, ost, pw, po), "GaussianBlur+SSIMFast batch")
                return out

            def enqueue(p):
                ctx._chk(lib.fnx_gaussian_blur_ssim_fast_batch_enqueue(ctx._h, n, srcs, st, w, h, pk, radius,
                                                                       flags, dsts, ost, pw),
                         "GaussianBlur+SSIMFast batch")

            def fetch(p):
                ctx._chk(lib.fnx_results_fetch(ctx._h, n, po), "fnx_results_fetch")
                return out
        return _Plan()

    def GaussianBlurSSIMFastBatch(self, imgs, sigma: float, outs=None, exact: bool = False, window=None,
                                  kernel=None):
        """-> (blurred images, numpy array of SSIMFast(imgs[i], blurred[i]))."""
        with self._ordered(*imgs):
            plan = self.plan_blur_ssim_fast_batch(imgs, sigma, outs=outs, exact=exact, window=window, kernel=kernel)
            vals = plan.run().copy()
        return plan.outs, vals


class _Prepared:
    """Reference side of an SSIM-guided quality search (compress.go:45-74)."""

    def __init__(self, ctx: Context, handle, w, h):
        self._ctx, self._p, self.w, self.h = ctx, handle, w, h

    def against(self, img, window=None) -> float:
        s = _Img(img)
        if (s.w, s.h) != (self.w, self.h):
            raise FennecError("candidate dims differ from the prepared reference")
        k, pk = _f64(self._ctx.gaussianKernel() if window is None else window)
        out = C.c_double()
        with self._ctx._ordered(img):
            self._ctx._chk(self._ctx._lib.fnx_ssim_fast_against(self._ctx._h, self._p, s.space, s.ptr, s.stride,
                                                                pk, C.byref(out)), "fnx_ssim_fast_against")
        return out.value

    def against_ycbcr(self, y, cb, cr, ratio: int, window=None) -> float:
        """SSIMFast(reference, toNRGBARef(decoded planes)) -- fnx_ssim_fast_against_ycbcr."""
        space, yp, ys, cbp, crp, cs, w, h = Context._planes(y, cb, cr)
        if (w, h) != (self.w, self.h):
            raise FennecError("candidate dims differ from the prepared reference")
        k, pk = _f64(self._ctx.gaussianKernel() if window is None else window)
        out = C.c_double(0.0)
        with self._ctx._ordered(y, cb, cr):
            self._ctx._chk(self._ctx._lib.fnx_ssim_fast_against_ycbcr(self._ctx._h, self._p, space, yp, ys, cbp, crp, cs,
                                                                      int(ratio), pk, C.byref(out)), "against_ycbcr")
        return float(out.value)

    def close(self):
        if self._p:
            self._ctx._lib.fnx_prepared_free(self._ctx._h, self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def Summarize(failed, has_result, original_size, compressed_size, ssim) -> dict:
    """batch.go:140-158 over parallel arrays (pure host arithmetic, index order)."""
    L = load_library()
    n = len(failed)
    f, pf = _i32(np.asarray(failed)); hr, ph = _i32(np.asarray(has_result))
    o = np.ascontiguousarray(original_size, dtype=np.int64)
    c = np.ascontiguousarray(compressed_size, dtype=np.int64)
    s, ps = _f64(np.asarray(ssim))
    out = np.zeros(4, dtype=np.int64)
    avg = L.fennec_Summarize(n, pf, ph, o.ctypes.data_as(_i64p), c.ctypes.data_as(_i64p), ps,
                             out.ctypes.data_as(_i64p))
    return dict(Total=int(out[0]), Succeeded=int(out[1]), Failed=int(out[2]), TotalSaved=int(out[3]),
                AvgSSIM=float(avg))


# ---------------------------------------------------------------------------------------
# module-level functions with the reference's names, on a per-thread default context
_tls = threading.local()


def default_context(device: int | None = None) -> Context:
    dev = int(os.environ.get("FENNEC_HIP_DEVICE", os.environ.get("LOCAL_RANK", "0"))) if device is None else device
    ctxs = getattr(_tls, "ctxs", None)
    if ctxs is None:
        ctxs = _tls.ctxs = {}
    if dev not in ctxs:
        ctxs[dev] = Context(dev)
    return ctxs[dev]


def _dev_of(x):
    if _is_torch(x) and x.is_cuda:
        return x.device.index or 0
    return None


def SSIM(img1, img2): return default_context(_dev_of(img1)).SSIM(img1, img2)
def SSIMFast(img1, img2): return default_context(_dev_of(img1)).SSIMFast(img1, img2)
def MSSSIM(img1, img2): return default_context(_dev_of(img1)).MSSSIM(img1, img2)
def computeSSIMNRGBA(img1, img2): return default_context(_dev_of(img1)).computeSSIMNRGBA(img1, img2)
def GaussianBlur(img, sigma): return default_context(_dev_of(img)).GaussianBlur(img, sigma, exact=None)
def Sharpen(img, strength): return default_context(_dev_of(img)).Sharpen(img, strength)
def AdaptiveSharpen(img, strength): return default_context(_dev_of(img)).AdaptiveSharpen(img, strength)
def ApplyOrientation(img, orient): return default_context(_dev_of(img)).ApplyOrientation(img, orient)
def lanczosResize(img, dstW, dstH): return default_context(_dev_of(img)).lanczosResize(img, dstW, dstH)
def smartResize(img, maxW, maxH): return default_context(_dev_of(img)).smartResize(img, maxW, maxH)
def boxDownsample(img, dstW, dstH): return default_context(_dev_of(img)).boxDownsample(img, dstW, dstH)
def lanczosBoxDownsample(img, midW, midH, dstW, dstH): return default_context(_dev_of(img)).lanczosBoxDownsample(img, midW, midH, dstW, dstH)
def Analyze(img): return default_context(_dev_of(img)).Analyze(img)
def png_filter(src, kind=None, ncolors=0, opaque=-1): return default_context(_dev_of(src)).png_filter(src, kind, ncolors, opaque)
def compress_png(img, level=9, device_deflate=False): return default_context(_dev_of(img)).compress_png(img, level, device_deflate)
def deflate(buf, row=0): return default_context(_dev_of(buf)).deflate(buf, row)
def png_encode(src, kind=None, ncolors=0, opaque=-1, palette=None): return default_context(_dev_of(src)).png_encode(src, kind, ncolors, opaque, palette)
def png_encoded_size(src, kind=None, ncolors=0, opaque=-1, palette=None): return default_context(_dev_of(src)).png_encoded_size(src, kind, ncolors, opaque, palette)
def deflate_bound(n): return int(load_library().fnx_deflate_bound(int(n)))
def crc32(data, crc=0): return default_context(_dev_of(data)).crc32(data, crc)
def png_file_bound(w, h): return int(load_library().fnx_png_file_bound(int(w), int(h)))


def inflate(data: bytes, cap: int | None = None) -> bytes:
    """The bytes of a zlib stream (fnx_inflate: host code, no device, no zlib).  cap: the most the stream may hold; by default
    the buffer grows, up to the 1032 x len(data) a deflate stream can reach, until the stream fits.  FennecError for a damaged
    stream, or one that holds more than cap bytes."""
    L = load_library()
    src = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, dtype=np.uint8)
    bound = 1032 * len(data)
    size = min(bound, max(64, 4 * len(data))) if cap is None else int(cap)
    while True:
        out = np.empty(max(size, 1), dtype=np.uint8)
        n = C.c_size_t(0)
        rc = L.fnx_inflate(src.ctypes.data, len(data), out.ctypes.data, size, C.byref(n))
        if rc == FNX_OK:
            return out[:n.value].tobytes()
        if cap is None and n.value == size + 1 and size < bound:          # cap + 1: the buffer was small, nothing else is wrong so far
            size = min(bound, 8 * size)
            continue
        raise FennecError(f"fnx_inflate failed ({rc}): {L.fnx_last_error().decode()}")


def png_info(data: bytes):
    """(w, h, colour type, bit depth, interlace) of a PNG file's IHDR (fnx_png_info: host code); FennecError when the
    signature or the header is damaged."""
    L = load_library()
    src = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, dtype=np.uint8)
    v = [C.c_int() for _ in range(5)]
    rc = L.fnx_png_info(src.ctypes.data, len(data), *[C.byref(x) for x in v])
    if rc < 0:
        raise FennecError(f"fnx_png_info failed ({rc}): {L.fnx_last_error().decode()}")
    return tuple(x.value for x in v)


def png_adam7_passes(w: int, h: int, color_type: int, depth: int):
    """Adam7's pass geometry (fnx_png_adam7_passes: host code) -> (pw[7], ph[7], rowbytes[7], stream_bytes); an absent pass
    has zeros.  FennecError for a pair outside the 15 colour type / depth pairs or a dimension outside 1..65535."""
    L = load_library()
    pw, ph, rb, total = (C.c_int * 7)(), (C.c_int * 7)(), (C.c_size_t * 7)(), C.c_size_t()
    rc = L.fnx_png_adam7_passes(int(w), int(h), int(color_type), int(depth), pw, ph, rb, C.byref(total))
    if rc < 0:
        raise FennecError(f"fnx_png_adam7_passes failed ({rc}): {L.fnx_last_error().decode()}")
    return list(pw), list(ph), list(rb), total.value

def median_cut(img, levels=(16, 32, 64, 128, 256)): return default_context(_dev_of(img)).median_cut(img, levels)
def quantize(img, max_colors): return default_context(_dev_of(img)).quantize(img, max_colors)
def png_reduce(img, max_colors=256, want_plane=True): return default_context(_dev_of(img)).png_reduce(img, max_colors, want_plane)
def tryPalettize(img, max_colors=256): return default_context(_dev_of(img)).tryPalettize(img, max_colors)


def png_file(stream, w, h, color_type, bit_depth, palette=None, level=9) -> bytes:
    """The PNG file around fnx_png_filter's stream (host only): signature, IHDR, PLTE (3 bytes per palette entry), tRNS (the
    alphas up to and including the last entry whose alpha != 255; omitted when there is none), one IDAT holding
    zlib.compress(stream, level), IEND.  palette: (n, 4) r,g,b,a for colour type 3.  Python's zlib is not Go's compress/flate:
    the file differs from the reference's in the deflate bytes only."""
    import struct
    import zlib

    def chunk(tag: bytes, body: bytes) -> bytes:
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xffffffff)
    raw = np.ascontiguousarray(stream, dtype=np.uint8).tobytes()
    parts = [b"\x89PNG\r\n\x1a\n", chunk(b"IHDR", struct.pack(">IIBBBBB", int(w), int(h), int(bit_depth), int(color_type), 0, 0, 0))]
    if int(color_type) == 3:
        pal = np.asarray(palette, dtype=np.uint8).reshape(-1, 4)
        if not 1 <= len(pal) <= 1 << int(bit_depth):
            raise FennecError("a paletted PNG needs a palette of 1 .. 2^bit_depth entries")
        parts.append(chunk(b"PLTE", pal[:, :3].tobytes()))
        translucent = np.flatnonzero(pal[:, 3] != 255)
        if len(translucent):
            parts.append(chunk(b"tRNS", pal[:translucent[-1] + 1, 3].tobytes()))
    parts += [chunk(b"IDAT", zlib.compress(raw, int(level))), chunk(b"IEND", b"")]
    return b"".join(parts)


def gaussianKernel(size=8, sigma=1.5):
    k = np.empty(size * size, dtype=np.float64)
    load_library().fennec_gaussianKernel(size, sigma, k.ctypes.data_as(_f64p))
    return k


def lanczos_box_fused(srcW, srcH, midW, midH, dstW, dstH, tables=None) -> bool:
    """fnx_lanczos_box_fused: would boxDownsample(lanczosResize(srcW x srcH -> midW x midH), dstW, dstH) take resize_box_kernel?
    tables = (table_h, table_v), None: precomputeWeights'.  Host arithmetic only."""
    th, tv = tables if tables is not None else (precomputeWeights(midW, srcW), precomputeWeights(midH, srcH))
    oh, poh = _i32(th[0]); ih, pih = _i32(th[1]); wh, pwh = _f64(th[2])
    ov, pov = _i32(tv[0]); iv, piv = _i32(tv[1]); wv, pwv = _f64(tv[2])
    return bool(load_library().fnx_lanczos_box_fused(srcW, srcH, poh, pih, pwh, pov, piv, pwv, midW, midH, dstW, dstH))


def blur_fixed_point(kernel):
    """fnx_blur_fixed_point: (wq, err255) of a blur table as the matrix-pipe kernel quantises it, or None when the table is not
    that kernel's.  Host arithmetic only."""
    k = np.ascontiguousarray(kernel, dtype=np.float64)
    radius = (len(k) - 1) // 2
    wq = (C.c_longlong * len(k))()
    err = C.c_double()
    rc = load_library().fnx_blur_fixed_point(k.ctypes.data_as(_f64p), radius, wq, C.byref(err))
    if rc == FNX_NOOP:
        return None
    if rc != 0:
        raise RuntimeError("fnx_blur_fixed_point failed")
    return np.array(list(wq), dtype=np.int64), float(err.value)


def resize_fixed_point(table, src_n):
    """fnx_resize_fixed_point: (S, G, first, count, wq) of one CSR tap table (off, idx, wt) over src_n source px as the
    matrix-pipe resize kernel quantises it -- first / count: int32 per output, wq: int64 of shape (nout, 16), zeros behind the
    taps -- or None when the table is not that kernel's.  Host arithmetic only."""
    off, idx, wt = table
    off, po = _i32(off); idx, pi = _i32(idx); wt, pw = _f64(wt)
    nout = len(off) - 1
    S, G = C.c_int(0), C.c_int(0)
    first = np.zeros(max(nout, 1), dtype=np.int32)
    count = np.zeros(max(nout, 1), dtype=np.int32)
    wq = np.zeros((max(nout, 1), 16), dtype=np.int32)
    rc = load_library().fnx_resize_fixed_point(po, pi, pw, nout, int(src_n), C.byref(S), C.byref(G), first.ctypes.data_as(_i32p),
                                               count.ctypes.data_as(_i32p), wq.ctypes.data_as(_i32p))
    if rc == FNX_NOOP:
        return None
    if rc != 0:
        raise FennecError("fnx_resize_fixed_point: " + (load_library().fnx_last_error() or b"").decode())
    return int(S.value), int(G.value), first, count, wq.astype(np.int64)


def blurKernel(sigma):
    L = load_library()
    r = L.fennec_blurKernel(float(sigma), None)
    k = np.empty(2 * r + 1, dtype=np.float64)
    L.fennec_blurKernel(float(sigma), k.ctypes.data_as(_f64p))
    return r, k


def precomputeWeights(dst_size, src_size):
    L = load_library()
    off = np.zeros(dst_size + 1, dtype=np.int32)
    n = L.fennec_precomputeWeights(dst_size, src_size, off.ctypes.data_as(_i32p), None, None)
    idx = np.zeros(max(n, 1), dtype=np.int32)
    wt = np.zeros(max(n, 1), dtype=np.float64)
    L.fennec_precomputeWeights(dst_size, src_size, off.ctypes.data_as(_i32p), idx.ctypes.data_as(_i32p),
                               wt.ctypes.data_as(_f64p))
    return off, idx[:max(n, 0)], wt[:max(n, 0)]
