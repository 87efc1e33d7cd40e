"""image-compression_amd: MI355X (gfx950) block-encode backend -- Python plumbing over the C ABI.

This module only *binds* libic_amd.so (include/ic_amd.h) with ctypes -- the prototypes are the table in abi.py -- and
passes torch device pointers / streams through it.  All encoding happens in the hand-written HIP kernels inside the
shared library; there is no Python or CPU implementation here, and importing fails loudly if the
library has not been built (python __graft_entry__.py / make -C image-compression_amd).

The directory name contains '-', so import it via `ic_amd_loader.load_package()` (repo root) or
importlib; the package registers itself as `image_compression_amd`.
"""
import ctypes
import os
import threading

import torch  # must precede CDLL: libic_amd.so then binds to the HIP runtime torch already loaded

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
_DEFAULT_LIB_PATH = os.path.join(_HERE, "libic_amd.so")
# A/B experiments only: ICAMD_LIB_PATH swaps the product library for another build, and is honoured ONLY together with
# ICAMD_ALLOW_LIB_OVERRIDE=1 (a stray variable must not silently redirect a benchmark); bench.py records LIB_PATH and
# LIB_OVERRIDDEN in its output line.
if "ICAMD_LIB_PATH" in os.environ and os.environ.get("ICAMD_ALLOW_LIB_OVERRIDE") != "1":
    raise ImportError("ICAMD_LIB_PATH is set (%s) but ICAMD_ALLOW_LIB_OVERRIDE=1 is not: refusing to load a library "
                      "other than %s" % (os.environ["ICAMD_LIB_PATH"], _DEFAULT_LIB_PATH))
LIB_PATH = os.environ.get("ICAMD_LIB_PATH", _DEFAULT_LIB_PATH)
LIB_OVERRIDDEN = os.path.realpath(LIB_PATH) != os.path.realpath(_DEFAULT_LIB_PATH)

# enums of include/ic_amd.h
COMPRESSOR_DXTC, COMPRESSOR_ETC, COMPRESSOR_PVRTC = 0, 1, 2
RGB, BGR, RGBA, BGRA = 0, 1, 2, 3
ETC_SPLIT_HORIZONTALLY, ETC_SPLIT_VERTICALLY, ETC_SMALLER_ERROR, ETC_HEURISTIC = 0, 1, 2, 3
DXT1, DXT5, ETC1, PVRTC2 = 0, 1, 2, 3
PVRTC4 = 4  # EXTENSION, parity unpinned: PVRTC1 4 bpp (include/ic_amd.h); icamd_encode_device only
# EXTENSION, parity pinned through the reference's DXT5 alpha path (include/ic_amd.h): BC4 (RGTC1, one channel, 8 bytes per
# block) and BC5 (RGTC2, two channels, 16 bytes per block); encode_device / decode_device / encode_batch_sharded_device only
BC4, BC5 = 5, 6
# EXTENSION (include/ic_amd.h ICAMD_ETC2_RGBA8): ETC2 RGBA8 = EAC alpha word + ETC1-compatible colour word, 16 bytes per block,
# from RGBA8 sources; colour half pinned to the ETC1 encoder byte for byte, alpha half defined in DESIGN.md 3.11.  7..15 are
# unassigned and rejected.  encode_device / decode_device / measure_error_device / containers only
ETC2_RGBA8 = 16
# EXTENSION (include/ic_amd.h ICAMD_ETC2_RGB8): ETC2 RGB8, 8 bytes per block, from RGB888 or RGBA8 sources: per block the ETC1
# encoder's word or the least-squares planar word, whichever is strictly closer.  17 is unassigned and rejected.
# encode_device / decode_device / measure_error_device / containers only
ETC2_RGB8 = 18
# etc2_modes of encode_device (include/ic_amd.h icamd_encode_etc2_device): DEFAULT = what icamd_encode_device writes; TH = then the
# T / H pass, which replaces the blocks a T or H word renders strictly closer (ETC2_RGB8 only)
ETC2_MODES_DEFAULT, ETC2_MODES_TH = 0, 1
# colour_modes of encode_etc2_colour_device (include/ic_amd.h icamd_encode_etc2_colour_device; ETC2_RGBA8, ETC2_RGB8 and
# ETC2_RGB8A1): DEFAULT = what icamd_encode_device writes; PLANAR = + the planar word; PLANAR_TH = + T and H words
ETC2_COLOUR_DEFAULT, ETC2_COLOUR_PLANAR, ETC2_COLOUR_PLANAR_TH = 0, 1, 2
# EXTENSION (include/ic_amd.h ICAMD_EAC_R11): EAC R11 (one channel, 8 bytes per block) and EAC RG11 (two channels, 16 bytes per
# block), the ETC2 family's BC4 / BC5; every word is what ETC2 RGBA8's alpha search writes for the channel, the
# decoder is the 11-bit one.  Source channels as for BC4 / BC5.  encode_device / decode_device / measure_error_device /
# containers only
EAC_R11, EAC_RG11 = 19, 20
# EXTENSION (include/ic_amd.h ICAMD_ETC2_RGB8A1): ETC2 RGB8 with punch-through alpha, 8 bytes per block, from RGBA8 sources: a texel
# is transparent iff its alpha is < 128; opaque blocks as ETC2 RGB8 (without the individual mode), blocks with transparency by the
# masked differential search.  Decodes to RGBA8 with alpha 0 or 255.  encode_device / decode_device /
# measure_error_device / containers only
ETC2_RGB8A1 = 21
# EXTENSION (include/ic_amd.h ICAMD_EAC_SIGNED_R11): signed EAC R11 / RG11, 8 / 16 bytes per block, int16 samples in and out.
# encode_eac11_16_device / decode_eac11_16_device / measure_error_eac11_16_device / containers only (22 and 23 are unassigned)
EAC_SIGNED_R11, EAC_SIGNED_RG11 = 24, 25
# EXTENSION (include/ic_amd.h ICAMD_BC7): BC7 / BPTC, 16 bytes per block.  The decoder and the metric read all eight modes; the
# encoder writes mode 6 from 3- or 4-byte pixels (a definition stated in the header).  encode_device / decode_device (RGBA8 rows)
# / measure_error_device / encode_batch_sharded_device / containers only (26..31 are unassigned)
BC7 = 32
# bc7_modes of encode_bc7_device (include/ic_amd.h icamd_encode_bc7_device): DEFAULT = what encode_device(BC7) writes (mode 6);
# EXTENDED = per block also a mode-1 candidate (opaque blocks) or a mode-5 candidate (the others), written where strictly closer
# 
BC7_MODES_DEFAULT, BC7_MODES_EXTENDED = 0, 1
# EXTENSION (include/ic_amd.h ICAMD_BC6H_UF16): BC6H / BPTC float, unsigned and signed, 16 bytes per block of RGB halves.  The
# decoder and the metric read all fourteen modes; the encoder writes the one-subset 10-bit mode from RGB16F / RGBA16F pixels (a
# definition stated in the header).  encode_bc6h_device / decode_bc6h_device / measure_error_bc6h_device / containers (DDS, KTX)
# only (33 is unassigned)
BC6H_UF16, BC6H_SF16 = 34, 35
# bc6h_modes of encode_bc6h_modes_device (include/ic_amd.h icamd_encode_bc6h_modes_device): DEFAULT = what encode_bc6h_device
# writes (mode field 00011); EXTENDED = one fused kernel that also fits one two-subset candidate per block and writes it where
# it is strictly closer in the t domain.
BC6H_MODES_DEFAULT, BC6H_MODES_EXTENDED = 0, 1
# EXTENSIONS (include/ic_amd.h ICAMD_BC1A, ICAMD_BC2): BC1 with punch-through alpha (8 bytes per block; a texel is transparent iff
# its alpha is < 128, fully opaque blocks are the DXT1 bytes, the others a stated three-colour search) and BC2 (16 bytes: sixteen
# 4-bit alphas, then DXT5's colour block), both from RGBA8 sources and decoded to RGBA8 as the formats define.
# encode_device / decode_device / measure_error_device / encode_batch_sharded_device / containers only (38 and up are unassigned)
BC1A, BC2 = 36, 37
OK, FALSE = 0, 1

EXPORTS = abi.EXPORTS  # every function of include/ic_amd.h; the prototypes live in abi.py
RCCL_UNIQUE_ID_BYTES = 128
# mip filters (bits; include/ic_amd.h, "mip filters"): 0 is the box filter of the plain mip entry points
MIP_FILTER_BOX, MIP_FILTER_SRGB, MIP_FILTER_ALPHA_WEIGHTED = 0, 1, 2
MIP_FILTER_NORMAL = 4  # BC5 chains and the RG8 pyramid only; not combinable
MIP_PYRAMID = -1  # `codec` of mip_kernel_name for the pixel pyramid
CONTAINER_DDS, CONTAINER_KTX, CONTAINER_PKM, CONTAINER_PVR = 0, 1, 2, 3

_lib = None
_tls = threading.local()  # per-thread state mirrored from the C side (the PVRTC workspace override is thread-local there)


class BackendError(RuntimeError):
    """The device path could not run (negative ICAMD_ERR_* status)."""


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libic_amd.so is not built (%s); run `python __graft_entry__.py` or "
                              "`make -C image-compression_amd` -- there is no fallback path" % LIB_PATH)
        # a library swapped in for an A/B run may lack newer entry points; the product library may not
        _lib = abi.bind(ctypes.CDLL(LIB_PATH), allow_missing=LIB_OVERRIDDEN)
    return _lib


def _error(status, what):
    return BackendError("%s failed with status %d: %s" % (what, status, lib().icamd_last_error().decode()))


def _check(status, what):
    """True for ICAMD_OK, False for the reference's `false`; a negative status raises."""
    if status < 0:
        raise _error(status, what)
    return status == OK


def _require_ok(status, what):
    if status != OK:
        raise _error(status, what)


def compute_compressed_data_size(compressor, fmt, height, width):
    return lib().icamd_compute_compressed_data_size(compressor, fmt, height, width)


def encoded_size(codec, grid_height, grid_width):
    return lib().icamd_encoded_size(codec, grid_height, grid_width)


def kernel_name(codec, src_components):
    return lib().icamd_kernel_name(codec, src_components).decode()


def etc2_kernel_name(codec, src_components, etc2_modes):
    """icamd_etc2_kernel_name: the kernel of the T / H pass (etc2_modes = ETC2_MODES_TH), "" where there is none; with
    ETC2_MODES_DEFAULT what kernel_name answers."""
    return lib().icamd_etc2_kernel_name(codec, src_components, etc2_modes).decode()


def _stream_handle(stream=None):
    s = torch.cuda.current_stream() if stream is None else stream
    return ctypes.c_void_p(s.cuda_stream)


def _ptr(t):
    """A tensor's device address; the prototypes' c_void_p parameters take the plain integer."""
    return t.data_ptr()


def _assert_u8_cuda(t):
    assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()


def _grid_bytes(compressor, fmt, height, width):
    """Bytes of the block grid of a height x width image of (compressor, fmt)."""
    block = 8 if (compressor == COMPRESSOR_ETC or fmt in (RGB, BGR)) else 16
    return ((height + 3) // 4) * ((width + 3) // 4) * block


def _host_u8(buffer, copy=False):
    """bytes / bytearray / memoryview / numpy array -> its bytes as a flat contiguous numpy uint8 array: a view of the
    caller's memory where that is contiguous, a private (writable) copy with copy=True."""
    import numpy as np
    a = np.ascontiguousarray(buffer) if isinstance(buffer, np.ndarray) else np.frombuffer(buffer, np.uint8)
    a = a.reshape(-1).view(np.uint8)
    return a.copy() if copy else a


def _compress_out_size(compressor, fmt, height, width, padded, out_size):
    """out_size of Compress (padded None) / CompressAndPad: the caller's, else the data size of the image or padded grid."""
    if out_size is not None:
        return out_size
    if padded is not None:
        height, width = max(height, padded[0]), max(width, padded[1])
    return compute_compressed_data_size(compressor, fmt, height, width)


def encode_device(codec, src, height, width, src_components, *, swap_rb=False, etc_strategy=ETC_SMALLER_ERROR,
                  grid_height=None, grid_width=None, row_stride_bytes=None, n_images=1,
                  src_image_stride_bytes=None, out=None, stream=None, etc2_modes=0):
    """Launch the encode kernel on `src` (a torch.uint8 CUDA tensor, any shape, contiguous bytes).
    Returns the output tensor [n_images, encoded_size] (device).  No synchronisation.
    etc2_modes = ETC2_MODES_TH (ETC2_RGB8 only): icamd_encode_etc2_device, the encode followed by the T / H pass.
    BC4 and EAC_R11 read R from 1..4-byte pixels, BC5 and EAC_RG11 read R and G from 2..4-byte pixels: R = byte 0 (byte 2 with
    swap_rb, which needs 3 or 4 bytes per pixel), G = byte 1."""
    _assert_u8_cuda(src)
    gh = height if grid_height is None else max(grid_height, height)
    gw = width if grid_width is None else max(grid_width, width)
    stride = width * src_components if row_stride_bytes is None else row_stride_bytes
    img_stride = height * stride if src_image_stride_bytes is None else src_image_stride_bytes
    per = encoded_size(codec, gh, gw)
    if out is None:
        out = torch.empty((n_images, per), dtype=torch.uint8, device=src.device)
    if etc2_modes != ETC2_MODES_DEFAULT:
        st = lib().icamd_encode_etc2_device(codec, etc_strategy, etc2_modes, src_components, int(swap_rb), height, width, gh, gw,
                                            stride, n_images, img_stride, per, _ptr(src), _ptr(out), _stream_handle(stream))
        return out if _check(st, "icamd_encode_etc2_device") else None
    st = lib().icamd_encode_device(codec, etc_strategy, src_components, int(swap_rb), height, width, gh, gw, stride,
                                   n_images, img_stride, per, _ptr(src), _ptr(out), _stream_handle(stream))
    if not _check(st, "icamd_encode_device"):
        return None
    return out


def encode_etc2_colour_device(codec, src, height, width, src_components, *, colour_modes=ETC2_COLOUR_DEFAULT, swap_rb=False,
                              etc_strategy=ETC_SMALLER_ERROR, grid_height=None, grid_width=None, row_stride_bytes=None,
                              n_images=1, src_image_stride_bytes=None, out=None, stream=None):
    """icamd_encode_etc2_colour_device: encode_device for ETC2_RGBA8, ETC2_RGB8 or ETC2_RGB8A1 with a choice of colour words --
    ETC2_COLOUR_DEFAULT (encode_device itself), ETC2_COLOUR_PLANAR, ETC2_COLOUR_PLANAR_TH.  Returns the output tensor
    [n_images, encoded_size] (device).  No synchronisation."""
    _assert_u8_cuda(src)
    gh = height if grid_height is None else max(grid_height, height)
    gw = width if grid_width is None else max(grid_width, width)
    stride = width * src_components if row_stride_bytes is None else row_stride_bytes
    img_stride = height * stride if src_image_stride_bytes is None else src_image_stride_bytes
    per = encoded_size(codec, gh, gw)
    if out is None:
        out = torch.empty((n_images, per), dtype=torch.uint8, device=src.device)
    st = lib().icamd_encode_etc2_colour_device(codec, etc_strategy, colour_modes, src_components, int(swap_rb), height, width, gh,
                                               gw, stride, n_images, img_stride, per, _ptr(src), _ptr(out),
                                               _stream_handle(stream))
    return out if _check(st, "icamd_encode_etc2_colour_device") else None


def etc2_colour_kernel_name(codec, src_components, colour_modes):
    """icamd_etc2_colour_kernel_name: the kernel of the colour-mode pass, or of what the call forwards to; "" if refused."""
    return lib().icamd_etc2_colour_kernel_name(codec, src_components, colour_modes).decode()


def encode_bc7_device(src, height, width, src_components, *, bc7_modes=BC7_MODES_DEFAULT, swap_rb=False, grid_height=None,
                      grid_width=None, row_stride_bytes=None, n_images=1, src_image_stride_bytes=None, out=None, stream=None):
    """icamd_encode_bc7_device: encode_device(BC7, ...) with a choice of modes -- BC7_MODES_DEFAULT (encode_device itself) or
    BC7_MODES_EXTENDED (the fused kernel with the mode-1 / mode-5 candidates).  Returns the output tensor
    [n_images, encoded_size] (device).  No synchronisation."""
    _assert_u8_cuda(src)
    gh = height if grid_height is None else max(grid_height, height)
    gw = width if grid_width is None else max(grid_width, width)
    stride = width * src_components if row_stride_bytes is None else row_stride_bytes
    img_stride = height * stride if src_image_stride_bytes is None else src_image_stride_bytes
    per = encoded_size(BC7, gh, gw)
    if out is None:
        out = torch.empty((n_images, per), dtype=torch.uint8, device=src.device)
    st = lib().icamd_encode_bc7_device(bc7_modes, src_components, int(swap_rb), height, width, gh, gw, stride, n_images,
                                       img_stride, per, _ptr(src), _ptr(out), _stream_handle(stream))
    return out if _check(st, "icamd_encode_bc7_device") else None


def bc7_kernel_name(src_components, bc7_modes):
    """icamd_bc7_kernel_name: the kernel that writes the final bytes (BC7_MODES_DEFAULT: what kernel_name answers); "" if refused."""
    return lib().icamd_bc7_kernel_name(src_components, bc7_modes).decode()


def compress_device(compressor, fmt, src, height, width, *, padding_bytes_per_row=0,
                    etc_strategy=ETC_SMALLER_ERROR, padded=None, out_size=None, stream=None):
    """Compressor::Compress / CompressAndPad on a device-resident image; returns a device uint8 tensor or None
    where the reference returns false."""
    _assert_u8_cuda(src)
    if padded is None:
        fn, dims = lib().icamd_compress_device, (height, width)
    else:
        fn, dims = lib().icamd_compress_and_pad_device, (height, width, padded[0], padded[1])
    n = _compress_out_size(compressor, fmt, height, width, padded, out_size)
    out = torch.empty((max(n, 1),), dtype=torch.uint8, device=src.device)
    st = fn(compressor, etc_strategy, fmt, *dims, padding_bytes_per_row, _ptr(src), _ptr(out), n, _stream_handle(stream))
    if not _check(st, "icamd_compress_device"):
        return None
    return out[:n]


def host_register(array):
    """Page-locks a numpy array's memory (icamd_host_register); pair with host_unregister before it is freed."""
    return _check(lib().icamd_host_register(ctypes.c_void_p(array.ctypes.data), array.nbytes), "icamd_host_register")


def host_unregister(array):
    return _check(lib().icamd_host_unregister(ctypes.c_void_p(array.ctypes.data)), "icamd_host_unregister")


def compress_host(compressor, fmt, buffer, height, width, *, padding_bytes_per_row=0,
                  etc_strategy=ETC_SMALLER_ERROR, padded=None, out_size=None, out=None):
    """The host-buffer drop-in (H2D + kernel + D2H inside the library).  `buffer`: bytes-like / numpy uint8.
    Returns bytes, or None where the reference returns false.  `out`: a caller-owned numpy uint8 array of the exact
    output size to write into (returned as is instead of bytes)."""
    import numpy as np
    src = _host_u8(buffer)
    if padded is None:
        fn, dims = lib().icamd_compress, (height, width)
    else:
        fn, dims = lib().icamd_compress_and_pad, (height, width, padded[0], padded[1])
    n = _compress_out_size(compressor, fmt, height, width, padded, out_size)
    if out is None:
        dst = np.zeros(max(n, 1), np.uint8)
    else:
        assert out.dtype == np.uint8 and out.size == n and out.flags["C_CONTIGUOUS"]
        dst = out
    st = fn(compressor, etc_strategy, fmt, *dims, padding_bytes_per_row, src.ctypes.data, dst.ctypes.data, n)
    if not _check(st, "icamd_compress"):
        return None
    return dst[:n].tobytes() if out is None else out


def decode_device(codec, blocks, height, width, *, swap_rb=False, padding_bytes_per_row=0, n_images=1, stream=None):
    _assert_u8_cuda(blocks)
    # BC4 and EAC_R11 -> R8, BC5 and EAC_RG11 -> RG8
    comps = {DXT5: 4, PVRTC2: 4, PVRTC4: 4, ETC2_RGBA8: 4, ETC2_RGB8A1: 4, BC7: 4, BC1A: 4, BC2: 4, BC4: 1, BC5: 2, EAC_R11: 1, EAC_RG11: 2}.get(codec, 3)
    per_out = height * (width * comps + padding_bytes_per_row)
    per_in = encoded_size(codec, height, width)
    out = torch.zeros((n_images, per_out), dtype=torch.uint8, device=blocks.device)
    st = lib().icamd_decode_device(codec, int(swap_rb), height, width, padding_bytes_per_row, n_images, per_in,
                                   per_out, _ptr(blocks), _ptr(out), _stream_handle(stream))
    if not _check(st, "icamd_decode_device"):
        return None
    return out


def pad_host(compressor, fmt, blocks, compressed_height, compressed_width, padded_height, padded_width,
             etc_strategy=ETC_SMALLER_ERROR):
    """Compressor::Pad for the really-padding case, host buffers.  bytes or None (reference's false)."""
    import numpy as np
    b = _host_u8(blocks)
    n = _grid_bytes(compressor, fmt, padded_height, padded_width)
    out = np.zeros(max(n, 1), np.uint8)
    st = lib().icamd_pad(compressor, etc_strategy, fmt, compressed_height, compressed_width, b.ctypes.data,
                         padded_height, padded_width, out.ctypes.data, n)
    return out[:n].tobytes() if _check(st, "icamd_pad") else None


def downsample_host(compressor, fmt, blocks, height, width, etc_strategy=ETC_SMALLER_ERROR):
    import numpy as np
    b = _host_u8(blocks)
    dh, dw = (height + 1) // 2, (width + 1) // 2
    n = _grid_bytes(compressor, fmt, dh, dw)
    out = np.zeros(max(n, 1), np.uint8)
    st = lib().icamd_downsample(compressor, etc_strategy, fmt, height, width, b.ctypes.data, out.ctypes.data, n)
    return out[:n].tobytes() if _check(st, "icamd_downsample") else None


def downsample_device(compressor, fmt, blocks, height, width, *, etc_strategy=ETC_SMALLER_ERROR, n_images=1, stream=None):
    """Compressor::Downsample on device-resident block grids: `blocks` = torch.uint8 CUDA tensor [n_images, bytes of one
    height x width image] (contiguous); returns [n_images, bytes of the halved image] or None where the reference refuses."""
    _assert_u8_cuda(blocks)
    dh, dw = (height + 1) // 2, (width + 1) // 2
    per_out = _grid_bytes(compressor, fmt, dh, dw)
    if n_images < 1 or blocks.numel() % n_images:
        raise ValueError("downsample_device: %d bytes do not divide into %d images" % (blocks.numel(), n_images))
    per_in = blocks.numel() // n_images
    need = _grid_bytes(compressor, fmt, height, width)
    if per_in < need:  # the kernel's 16-byte block loads would run past the tensor
        raise ValueError("downsample_device: %d bytes per image, a %d x %d image has %d" % (per_in, height, width, need))
    out = torch.empty((n_images, per_out), dtype=torch.uint8, device=blocks.device)
    st = lib().icamd_downsample_batch_device(compressor, etc_strategy, fmt, height, width, n_images,
                                             _ptr(blocks), per_in, _ptr(out), per_out, per_out, _stream_handle(stream))
    return out if _check(st, "icamd_downsample_batch_device") else None


def transcode_dxt1_to_etc1_host(blocks):
    b = _host_u8(blocks, copy=True)
    st = lib().icamd_transcode_dxt1_to_etc1(b.ctypes.data, b.size)
    return b.tobytes() if _check(st, "icamd_transcode_dxt1_to_etc1") else None


def transcode_dxt5_to_etc2_rgba8_host(blocks):
    """icamd_transcode_dxt5_to_etc2_rgba8 (extension): DXT5 blocks (bytes-like) -> ETC2 RGBA8 blocks of the same size; bytes
    past the last whole 16-byte block come back unchanged."""
    b = _host_u8(blocks, copy=True)
    st = lib().icamd_transcode_dxt5_to_etc2_rgba8(b.ctypes.data, b.size)
    return b.tobytes() if _check(st, "icamd_transcode_dxt5_to_etc2_rgba8") else None


def transcode_dxt5_to_etc2_rgba8_device(t, stream=None):
    """icamd_transcode_dxt5_to_etc2_rgba8_device (extension): the DXT5 blocks in `t` (a contiguous torch.uint8 CUDA tensor whose
    storage is 16-byte aligned) become ETC2 RGBA8 blocks IN PLACE; returns `t`.  No synchronisation."""
    _assert_u8_cuda(t)
    st = lib().icamd_transcode_dxt5_to_etc2_rgba8_device(_ptr(t), t.numel(), _stream_handle(stream))
    return t if _check(st, "icamd_transcode_dxt5_to_etc2_rgba8_device") else None


def _transcode_host(symbol, blocks):
    b = _host_u8(blocks, copy=True)
    st = getattr(lib(), symbol)(b.ctypes.data, b.size)
    return b.tobytes() if _check(st, symbol) else None


def _transcode_device(symbol, t, stream):
    _assert_u8_cuda(t)
    st = getattr(lib(), symbol)(_ptr(t), t.numel(), _stream_handle(stream))
    return t if _check(st, symbol) else None


def transcode_dxt1_to_etc2_rgb8_host(blocks):
    """icamd_transcode_dxt1_to_etc2_rgb8 (extension): DXT1 blocks (bytes-like) -> ETC2 RGB8 blocks of the same size; bytes past
    the last whole 8-byte block come back unchanged."""
    return _transcode_host("icamd_transcode_dxt1_to_etc2_rgb8", blocks)


def transcode_dxt1_to_etc2_rgb8_device(t, stream=None):
    """icamd_transcode_dxt1_to_etc2_rgb8_device (extension): the DXT1 blocks in `t` (a contiguous torch.uint8 CUDA tensor whose
    storage is 8-byte aligned) become ETC2 RGB8 blocks IN PLACE; returns `t`.  No synchronisation."""
    return _transcode_device("icamd_transcode_dxt1_to_etc2_rgb8_device", t, stream)


def transcode_bc4_to_eac_r11_host(blocks):
    """icamd_transcode_bc4_to_eac_r11 (extension): BC4 blocks (bytes-like) -> EAC R11 blocks of the same size; bytes past the
    last whole 8-byte block come back unchanged."""
    return _transcode_host("icamd_transcode_bc4_to_eac_r11", blocks)


def transcode_bc4_to_eac_r11_device(t, stream=None):
    """icamd_transcode_bc4_to_eac_r11_device (extension): the BC4 blocks in `t` (8-byte aligned) become EAC R11 blocks IN PLACE;
    returns `t`.  No synchronisation."""
    return _transcode_device("icamd_transcode_bc4_to_eac_r11_device", t, stream)


def transcode_bc5_to_eac_rg11_host(blocks):
    """icamd_transcode_bc5_to_eac_rg11 (extension): BC5 blocks (bytes-like) -> EAC RG11 blocks of the same size; bytes past the
    last whole 16-byte block come back unchanged."""
    return _transcode_host("icamd_transcode_bc5_to_eac_rg11", blocks)


def transcode_bc5_to_eac_rg11_device(t, stream=None):
    """icamd_transcode_bc5_to_eac_rg11_device (extension): the BC5 blocks in `t` (16-byte aligned) become EAC RG11 blocks IN
    PLACE; returns `t`.  No synchronisation."""
    return _transcode_device("icamd_transcode_bc5_to_eac_rg11_device", t, stream)


def pvrtc_encode_region_device(src, size, first_block, n_blocks, *, out=None, stream=None):
    """icamd_pvrtc2_encode_region_device: blocks [first_block, first_block + n_blocks) of the Z-order output of the
    size x size RGBA8 image `src` (torch.uint8 CUDA tensor).  Returns the [8 * n_blocks] uint8 device tensor, or None
    where the reference would refuse the size.  No synchronisation."""
    _assert_u8_cuda(src)
    if out is None:
        out = torch.empty((8 * n_blocks,), dtype=torch.uint8, device=src.device)
    st = lib().icamd_pvrtc2_encode_region_device(size, first_block, n_blocks, _ptr(src), _ptr(out), _stream_handle(stream))
    if not _check(st, "icamd_pvrtc2_encode_region_device"):
        return None
    return out


def pvrtc_decompress_host(blocks, size):
    """icamd_pvrtc2_decompress (extension): bytes of size x size RGBA8, or None where the sizes are refused."""
    import numpy as np
    b = _host_u8(blocks)
    out = np.zeros(size * size * 4, np.uint8)
    st = lib().icamd_pvrtc2_decompress(size, b.ctypes.data, b.size, out.ctypes.data, out.size)
    return out.tobytes() if _check(st, "icamd_pvrtc2_decompress") else None


def pvrtc_workspace_size(size, n_images=1):
    return lib().icamd_pvrtc2_workspace_size(size, n_images)


def pvrtc4_workspace_size(size, n_images=1):
    return lib().icamd_pvrtc4_workspace_size(size, n_images)


def pvrtc_tune(mode=0, log2_strip=-1):
    """icamd_pvrtc2_tune (extension, test / tuning hook): 0 = automatic, 1 = always morph + encode, 2 = the one-pass kernel
    wherever it is eligible; log2_strip < 0 = automatic strip height.  Process-wide; results are identical either way."""
    return _check(lib().icamd_pvrtc2_tune(int(mode), int(log2_strip)), "icamd_pvrtc2_tune")


def pvrtc_set_workspace(workspace):
    """Caller-owned PVRTC scratch for the calls that follow on this thread (a torch.uint8 CUDA tensor of at least
    pvrtc_workspace_size bytes; needed to capture PVRTC launches into a HIP graph).  None: the library's own buffer."""
    if workspace is None:
        _tls.workspace = None
        return _check(lib().icamd_pvrtc2_set_workspace(None, 0), "icamd_pvrtc2_set_workspace")
    _assert_u8_cuda(workspace)
    if workspace.device.index not in (None, torch.cuda.current_device()):
        raise ValueError("PVRTC workspace lives on %s but the current device is cuda:%d"
                         % (workspace.device, torch.cuda.current_device()))
    ok = _check(lib().icamd_pvrtc2_set_workspace(_ptr(workspace), workspace.numel()), "icamd_pvrtc2_set_workspace")
    # the C side keeps only the raw pointer (per host thread): hold the tensor until the override is cleared, so that
    # a caller dropping its reference cannot leave the library writing into freed memory
    _tls.workspace = workspace if ok else None
    return ok


def compress_batch_host(compressor, fmt, images, height, width, devices, *, padding_bytes_per_row=0,
                        etc_strategy=ETC_SMALLER_ERROR):
    """icamd_compress_batch: `images` = list of numpy uint8 arrays (host), `devices` = list of HIP ordinals.
    Returns a list of bytes (None where the reference would return false)."""
    import numpy as np
    n = len(images)
    size = compute_compressed_data_size(compressor, fmt, height, width)
    srcs = [np.ascontiguousarray(im, dtype=np.uint8).reshape(-1) for im in images]
    outs = [np.zeros(max(size, 1), np.uint8) for _ in range(n)]
    in_ptrs = (ctypes.c_void_p * n)(*[s.ctypes.data for s in srcs])
    out_ptrs = (ctypes.c_void_p * n)(*[o.ctypes.data for o in outs])
    devs = (ctypes.c_int * len(devices))(*devices)
    statuses = (ctypes.c_int * n)()
    st = lib().icamd_compress_batch(compressor, etc_strategy, fmt, height, width, padding_bytes_per_row, n, in_ptrs,
                                    out_ptrs, size, devs, len(devices), statuses)
    if st < 0:
        _check(st, "icamd_compress_batch")
    return [outs[i][:size].tobytes() if statuses[i] == OK else None for i in range(n)]


def create_solid_device(compressor, fmt, height, width, color, *, device=None, out=None, stream=None):
    """Compressor::CreateSolidImage into a device-resident block grid; returns the uint8 device tensor, or None where
    the reference returns false."""
    c = bytes(bytearray(color))
    buf = (ctypes.c_uint8 * max(len(c), 4))(*c)
    n = _grid_bytes(compressor, fmt, height, width)
    if out is None:
        out = torch.empty((max(n, 1),), dtype=torch.uint8, device=device or torch.device("cuda", torch.cuda.current_device()))
    st = lib().icamd_create_solid_device(compressor, fmt, height, width, buf, _ptr(out), n, _stream_handle(stream))
    return out[:n] if _check(st, "icamd_create_solid_device") else None


def create_solid_batch_device(compressor, fmt, height, width, colors, *, device=None, stream=None):
    """icamd_create_solid_batch_device (extension): len(colors) solid images in one launch -> [n, bytes] device tensor."""
    comps = 3 if fmt in (RGB, BGR) else 4
    flat = bytes(bytearray(b for c in colors for b in bytearray(c)[:comps]))
    buf = (ctypes.c_uint8 * max(len(flat), 4))(*flat)
    per = _grid_bytes(compressor, fmt, height, width)
    out = torch.empty((len(colors), max(per, 1)), dtype=torch.uint8, device=device or torch.device("cuda", torch.cuda.current_device()))
    st = lib().icamd_create_solid_batch_device(compressor, fmt, height, width, len(colors), buf, _ptr(out),
                                               out.shape[1], per, _stream_handle(stream))
    return out[:, :per] if _check(st, "icamd_create_solid_batch_device") else None


def pad_batch_device(compressor, fmt, blocks, compressed_height, compressed_width, padded_height, padded_width, *,
                     etc_strategy=ETC_SMALLER_ERROR, stream=None):
    """icamd_pad_batch_device (extension): blocks = [n, bytes] device tensor of equally shaped grids -> [n, bytes] padded."""
    _assert_u8_cuda(blocks)
    assert blocks.dim() == 2
    per = _grid_bytes(compressor, fmt, padded_height, padded_width)
    need = _grid_bytes(compressor, fmt, compressed_height, compressed_width)
    if blocks.shape[1] < need:
        raise ValueError("pad_batch_device: %d bytes per image, the source grid takes %d" % (blocks.shape[1], need))
    out = torch.empty((blocks.shape[0], max(per, 1)), dtype=torch.uint8, device=blocks.device)
    st = lib().icamd_pad_batch_device(compressor, etc_strategy, fmt, compressed_height, compressed_width, blocks.shape[0],
                                      _ptr(blocks), blocks.shape[1], padded_height, padded_width, _ptr(out), out.shape[1], per,
                                      _stream_handle(stream))
    return out[:, :per] if _check(st, "icamd_pad_batch_device") else None


def copy_subimage_batch_device(compressor, fmt, blocks, compressed_height, compressed_width, start_row, start_column, height,
                               width, *, stream=None):
    """icamd_copy_subimage_batch_device (extension): the same window of every grid of blocks = [n, bytes]."""
    _assert_u8_cuda(blocks)
    assert blocks.dim() == 2
    per = _grid_bytes(compressor, fmt, height, width)
    need = _grid_bytes(compressor, fmt, compressed_height, compressed_width)
    if blocks.shape[1] < need:
        raise ValueError("copy_subimage_batch_device: %d bytes per image, the source grid takes %d" % (blocks.shape[1], need))
    out = torch.empty((blocks.shape[0], max(per, 1)), dtype=torch.uint8, device=blocks.device)
    st = lib().icamd_copy_subimage_batch_device(compressor, fmt, compressed_height, compressed_width, blocks.shape[0],
                                                _ptr(blocks), blocks.shape[1], start_row, start_column, height, width,
                                                _ptr(out), out.shape[1], per, _stream_handle(stream))
    return out[:, :per] if _check(st, "icamd_copy_subimage_batch_device") else None


def create_solid_host(compressor, fmt, height, width, color):
    import numpy as np
    c = bytes(bytearray(color))
    buf = (ctypes.c_uint8 * max(len(c), 4))(*c)
    n = _grid_bytes(compressor, fmt, height, width)
    out = np.zeros(max(n, 1), np.uint8)
    st = lib().icamd_create_solid(compressor, fmt, height, width, buf, out.ctypes.data, n)
    return out[:n].tobytes() if _check(st, "icamd_create_solid") else None


def container_size(container, codec, height, width, levels=1):
    return int(lib().icamd_container_size(container, codec, height, width, levels))


def container_write(container, codec, height, width, levels_data):
    """Frames the block streams of the mip levels (largest first, bytes-like each) as a DDS / KTX / PKM / PVR file image
    (extension, include/ic_amd.h: the reference has no container code); bytes, or None where the C side says false."""
    import numpy as np
    levels = [_host_u8(b) for b in levels_data]
    n = len(levels)
    total = container_size(container, codec, height, width, n)
    out = np.zeros(max(total, 1), np.uint8)
    ptrs = (ctypes.c_void_p * max(n, 1))(*[ctypes.c_void_p(a.ctypes.data if a.size else 0) for a in levels])
    sizes = (ctypes.c_size_t * max(n, 1))(*[a.size for a in levels])
    st = lib().icamd_container_write(container, codec, height, width, n, ptrs, sizes, out.ctypes.data, total)
    return out[:total].tobytes() if _check(st, "icamd_container_write") else None


def copy_subimage_device(compressor, fmt, blocks, compressed_height, compressed_width, start_row, start_column, height,
                         width, *, stream=None):
    """Compressor::CopySubimage on a device-resident block grid (torch.uint8 CUDA tensor); device tensor or None."""
    _assert_u8_cuda(blocks)
    n = _grid_bytes(compressor, fmt, height, width)
    out = torch.empty((max(n, 1),), dtype=torch.uint8, device=blocks.device)
    st = lib().icamd_copy_subimage_device(compressor, fmt, compressed_height, compressed_width, _ptr(blocks), start_row,
                                          start_column, height, width, _ptr(out), n, _stream_handle(stream))
    return out[:n] if _check(st, "icamd_copy_subimage_device") else None


def copy_subimage_host(compressor, fmt, blocks, compressed_height, compressed_width, start_row, start_column, height,
                       width):
    import numpy as np
    b = _host_u8(blocks)
    n = _grid_bytes(compressor, fmt, height, width)
    out = np.zeros(max(n, 1), np.uint8)
    st = lib().icamd_copy_subimage(compressor, fmt, compressed_height, compressed_width, b.ctypes.data, start_row,
                                   start_column, height, width, out.ctypes.data, n)
    return out[:n].tobytes() if _check(st, "icamd_copy_subimage") else None


def encode_batch_sharded_device(codec, srcs, height, width, src_components, devices, *, swap_rb=False,
                                etc_strategy=ETC_SMALLER_ERROR, row_stride_bytes=None, outs=None, gather_device=-1,
                                gathered=None):
    """icamd_encode_batch_sharded_device: `srcs` = list of torch.uint8 CUDA tensors, image i on device
    devices[i % len(devices)]; `outs` = optional list of per-image output tensors (same devices); gather_device >= 0
    additionally collects every image into `gathered` ([n, encoded_size] uint8 on that device, allocated if None).
    Returns (statuses, outs, gathered); synchronous."""
    n = len(srcs)
    per = encoded_size(codec, height, width)
    stride = width * src_components if row_stride_bytes is None else row_stride_bytes
    for i, s in enumerate(srcs):
        _assert_u8_cuda(s)
        assert s.device.index == devices[i % len(devices)], "image %d is not on its listed device" % i
    if gather_device >= 0 and gathered is None:
        gathered = torch.empty((n, per), dtype=torch.uint8, device=torch.device("cuda", gather_device))
    # The sources / outputs were produced on torch streams (and come from torch's caching allocator) on EVERY listed
    # device, the library uses its own streams: wait for all of them, not just the current device.
    involved = set(devices[i % len(devices)] for i in range(n))
    if gather_device >= 0:
        involved.add(gather_device)
    for d in sorted(involved):
        if 0 <= d < torch.cuda.device_count():  # (a bad ordinal is the C side's to refuse, with its own status)
            torch.cuda.synchronize(d)
    in_ptrs = (ctypes.c_void_p * n)(*[s.data_ptr() for s in srcs])
    out_ptrs = None if outs is None else (ctypes.c_void_p * n)(*[(o.data_ptr() if o is not None else None) for o in outs])
    devs = (ctypes.c_int * len(devices))(*devices)
    statuses = (ctypes.c_int * n)()
    st = lib().icamd_encode_batch_sharded_device(codec, etc_strategy, src_components, int(swap_rb), height, width, stride,
                                                 n, in_ptrs, out_ptrs, devs, len(devices), gather_device,
                                                 None if gathered is None else _ptr(gathered),
                                                 per if gathered is None else gathered.stride(0), statuses)
    if st < 0:
        _check(st, "icamd_encode_batch_sharded_device")
    return list(statuses), outs, gathered


def clock_probe_buffer():
    """A zeroed result buffer for clock_probe, allocated and cleared NOW (synchronised): allocate the buffers of all
    probes before the launches they are to overlap, or the clearing kernel queues up behind those launches."""
    out = torch.zeros(2, dtype=torch.int64, device=torch.device("cuda", torch.cuda.current_device()))
    torch.cuda.current_stream().synchronize()
    return out


def clock_probe(duration_us, stream, out=None):
    """Enqueues the one-wave clock probe on `stream`; returns a callable that (after a synchronize) yields the mean
    shader clock in MHz over the probe's interval, or None if the counters are unusable."""
    if out is None:
        out = clock_probe_buffer()
    khz = lib().icamd_wall_clock_rate_khz()
    st = lib().icamd_clock_probe_device(_ptr(out), int(duration_us), _stream_handle(stream))
    _check(st, "icamd_clock_probe_device")

    def result():
        cyc, ticks = [int(v) for v in out.cpu().tolist()]
        if ticks <= 0 or khz == 0:
            return None
        return {"shader_MHz": cyc / ticks * khz / 1e3, "shader_cycles": cyc, "ref_ticks": ticks, "ref_clock_kHz": khz,
                "interval_ms": ticks / khz}
    return result


class RcclGather:
    """The product's own gather of the compressed output (icamd_gather_blocks_rccl: one grouped ncclSend / ncclRecv exchange
    into rank `root`'s HBM).  torch.distributed is only used to hand rank 0's ncclUniqueId to the other ranks (any transport
    would do: the C entry points take the 128 bytes); the communicator and the collective are the library's."""

    def __init__(self, rank, world, broadcast_bytes, agree=None):
        """broadcast_bytes(bytes or None) -> bytes: hands rank 0's argument to every rank (collective).
        agree(bool) -> bool: True iff every rank passed True (collective; None in a world of one rank).  Every rank makes the SAME
        sequence of collective calls whatever fails where -- a rank without librccl, or rank 0 without an id, must not leave the
        others waiting inside ncclCommInitRank."""
        L = lib()
        agree = agree or (lambda ok: ok)
        self.rank, self.world = rank, world
        self.comm = ctypes.c_void_p()
        available = bool(L.icamd_rccl_available())
        why = None if available else "librccl could not be bound: %s" % L.icamd_last_error().decode()
        uid = (ctypes.c_uint8 * RCCL_UNIQUE_ID_BYTES)()
        if rank == 0 and available:
            try:
                _require_ok(L.icamd_rccl_get_unique_id(uid), "icamd_rccl_get_unique_id")
            except BackendError as e:  # not raised yet: the other ranks are waiting for the broadcast
                available, why = False, str(e)
                uid = (ctypes.c_uint8 * RCCL_UNIQUE_ID_BYTES)()
        raw = broadcast_bytes(bytes(uid) if rank == 0 else None)
        if available and not any(raw):
            available, why = False, "rank 0 could not create an ncclUniqueId"
        if not agree(available):
            raise BackendError(why or "another rank cannot use librccl")
        uid = (ctypes.c_uint8 * RCCL_UNIQUE_ID_BYTES)(*raw)
        _require_ok(L.icamd_rccl_comm_init(ctypes.byref(self.comm), world, rank, uid), "icamd_rccl_comm_init")

    def gather(self, local, bufs, counts_bytes, root=0, stream=None):
        """local: this rank's uint8 device tensor (counts_bytes[rank] bytes); bufs: on `root`, one device tensor per rank (any
        placement: their offsets from the lowest address are passed on), elsewhere None.  Enqueued, not synchronised."""
        n = self.world
        counts = (ctypes.c_size_t * n)(*[int(c) for c in counts_bytes])
        base, offs = None, None
        if self.rank == root:
            ptrs = [b.data_ptr() for b in bufs]
            lo = min(p for p, c in zip(ptrs, counts_bytes) if c > 0) if any(c > 0 for c in counts_bytes) else 0
            base = ctypes.c_void_p(lo)
            offs = (ctypes.c_size_t * n)(*[(p - lo) if c > 0 else 0 for p, c in zip(ptrs, counts_bytes)])
        st = lib().icamd_gather_blocks_rccl(self.comm, self.rank, n, root, counts,
                                            _ptr(local) if local.numel() else None, base, offs, _stream_handle(stream))
        _require_ok(st, "icamd_gather_blocks_rccl")

    def destroy(self):
        if self.comm:
            lib().icamd_rccl_comm_destroy(self.comm)
            self.comm = ctypes.c_void_p()


# ---- mip chains (EXTENSION, include/ic_amd.h): one source image -> every level, each encoded from its own pixels ----
def mip_max_levels(height, width):
    """floor(log2(max(height, width))) + 1: the levels of a full chain (0 for an empty image)."""
    return lib().icamd_mip_max_levels(height, width)


def mip_chain_size(codec, height, width, levels=None):
    """(bytes of one image's chain, [offset of level l for l in 0..levels]) -- the last entry is the total; (0, None) where
    the codec / size / level count is refused."""
    if levels is None:
        levels = mip_max_levels(height, width)
    offs = (ctypes.c_size_t * (max(levels, 0) + 1))()
    n = lib().icamd_mip_chain_size(codec, height, width, levels, offs)
    return (n, list(offs)) if n else (0, None)


def mip_workspace_size(codec, src_components, height, width, levels=None, n_images=1):
    if levels is None:
        levels = mip_max_levels(height, width)
    return lib().icamd_mip_workspace_size(codec, src_components, height, width, levels, n_images)


def _check_out(out, n_images, per, what):
    """A caller's `out` must be the [n_images, per] uint8 device tensor the kernels write (per = the destination image
    stride) and the views index: a shorter one would be written past its end."""
    if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.dim() == 2 and out.shape[0] == n_images
            and out.shape[1] == max(per, 1)):
        raise ValueError("%s: out must be a contiguous uint8 CUDA tensor of shape [%d, %d], got %s %s"
                         % (what, n_images, max(per, 1), tuple(out.shape), out.dtype))


def mip_level_shape(height, width, level):
    return max(1, height >> level), max(1, width >> level)


def encode_mips_device(codec, src, height, width, src_components, *, levels=None, swap_rb=False,
                       etc_strategy=ETC_SMALLER_ERROR, n_images=1, row_stride_bytes=None, src_image_stride_bytes=None,
                       dst_image_stride_bytes=None, out=None, workspace=None, stream=None, mip_filter=0):
    """Fused mip-chain encode (icamd_encode_mips_device; with mip_filter -- MIP_FILTER_SRGB | MIP_FILTER_ALPHA_WEIGHTED, or
    MIP_FILTER_NORMAL for BC5 -- other than 0, icamd_encode_mips_filtered_device) of `src` (a torch.uint8 CUDA tensor, contiguous bytes).
    Returns (flat, views): flat is [n_images, dst_image_stride] (device), views[l] = flat[:, offset[l]:offset[l + 1]], the
    blocks of level l.  The workspace is allocated here unless the caller passes one (a uint8 CUDA tensor of at least
    mip_workspace_size bytes).  No synchronisation."""
    _assert_u8_cuda(src)
    if levels is None:
        levels = mip_max_levels(height, width)
    stride = width * src_components if row_stride_bytes is None else row_stride_bytes
    img_stride = height * stride if src_image_stride_bytes is None else src_image_stride_bytes
    total, offs = mip_chain_size(codec, height, width, levels)
    per = total if dst_image_stride_bytes is None else dst_image_stride_bytes
    if out is None:
        out = torch.empty((n_images, max(per, 1)), dtype=torch.uint8, device=src.device)
    _check_out(out, n_images, per, "encode_mips_device")
    ws_bytes = mip_workspace_size(codec, src_components, height, width, levels, n_images) if total else 0
    if workspace is None and ws_bytes:
        workspace = torch.empty((ws_bytes,), dtype=torch.uint8, device=src.device)
    if workspace is not None and not (workspace.is_cuda and workspace.dtype == torch.uint8 and workspace.is_contiguous()):
        raise ValueError("encode_mips_device: workspace must be a contiguous uint8 CUDA tensor")
    ws_ptr = _ptr(workspace) if workspace is not None else None
    ws_len = workspace.numel() if workspace is not None else 0
    tail = (height, width, stride, levels, n_images, img_stride, per, _ptr(src), _ptr(out), ws_ptr, ws_len,
            _stream_handle(stream))
    if mip_filter == 0:
        st = lib().icamd_encode_mips_device(codec, etc_strategy, src_components, int(swap_rb), *tail)
    else:
        st = lib().icamd_encode_mips_filtered_device(codec, etc_strategy, src_components, int(swap_rb), mip_filter, *tail)
    if not _check(st, "icamd_encode_mips_device"):
        return None
    return out, [out[:, offs[l]:offs[l + 1]] for l in range(levels)]


def mip_pyramid_size(src_components, height, width, levels=None):
    """(bytes of one image's pyramid output -- levels 1 .. levels-1 --, [offset of level l for l in 1..levels])."""
    if levels is None:
        levels = mip_max_levels(height, width)
    offs = [0]
    for l in range(1, levels):
        h, w = mip_level_shape(height, width, l)
        offs.append(offs[-1] + h * w * src_components)
    return offs[-1], offs


def mip_pyramid_device(src, height, width, src_components, *, levels=None, n_images=1, row_stride_bytes=None,
                       src_image_stride_bytes=None, dst_image_stride_bytes=None, out=None, stream=None, mip_filter=0):
    """The pixel pyramid alone (icamd_mip_pyramid_device; icamd_mip_pyramid_filtered_device with mip_filter other than 0).
    Returns (flat, views): views[l - 1] is level l as a [n_images, h_l, w_l, src_components] view, for l = 1 .. levels-1."""
    _assert_u8_cuda(src)
    if levels is None:
        levels = mip_max_levels(height, width)
    stride = width * src_components if row_stride_bytes is None else row_stride_bytes
    img_stride = height * stride if src_image_stride_bytes is None else src_image_stride_bytes
    total, offs = mip_pyramid_size(src_components, height, width, levels)
    per = total if dst_image_stride_bytes is None else dst_image_stride_bytes
    if out is None:
        out = torch.empty((n_images, max(per, 1)), dtype=torch.uint8, device=src.device)
    _check_out(out, n_images, per, "mip_pyramid_device")
    tail = (height, width, stride, levels, n_images, img_stride, per, _ptr(src), _ptr(out), _stream_handle(stream))
    if mip_filter == 0:
        st = lib().icamd_mip_pyramid_device(src_components, *tail)
    else:
        st = lib().icamd_mip_pyramid_filtered_device(src_components, mip_filter, *tail)
    if not _check(st, "icamd_mip_pyramid_device"):
        return None
    views = []
    for l in range(1, levels):
        h, w = mip_level_shape(height, width, l)
        views.append(out[:, offs[l - 1]:offs[l]].view(n_images, h, w, src_components))
    return out, views


def compress_mips_host(compressor, fmt, buffer, height, width, *, levels=None, padding_bytes_per_row=0,
                       etc_strategy=ETC_SMALLER_ERROR, out_size=None, mip_filter=0):
    """Host-buffer mip chain (icamd_compress_mips; icamd_compress_mips_filtered with mip_filter other than 0): bytes of the
    whole chain, or None where the reference's conventions return false."""
    import numpy as np
    if levels is None:
        levels = mip_max_levels(height, width)
    src = _host_u8(buffer)
    if out_size is None:
        codec = {(COMPRESSOR_DXTC, RGB): DXT1, (COMPRESSOR_DXTC, BGR): DXT1, (COMPRESSOR_DXTC, RGBA): DXT5,
                 (COMPRESSOR_DXTC, BGRA): DXT5, (COMPRESSOR_ETC, RGB): ETC1}.get((compressor, fmt))
        out_size = mip_chain_size(codec, height, width, levels)[0] if codec is not None else 0
    out = np.empty(max(out_size, 1), dtype=np.uint8)
    tail = (height, width, padding_bytes_per_row, levels, src.ctypes.data, out.ctypes.data, out_size)
    if mip_filter == 0:
        st = lib().icamd_compress_mips(compressor, etc_strategy, fmt, *tail)
    else:
        st = lib().icamd_compress_mips_filtered(compressor, etc_strategy, fmt, mip_filter, *tail)
    if not _check(st, "icamd_compress_mips"):
        return None
    return out[:out_size].tobytes()


def mip_kernel_name(codec, src_components, mip_filter=0):
    """Name of the mip kernel a configuration launches ("" if refused); codec MIP_PYRAMID: the pixel pyramid's."""
    return lib().icamd_mip_kernel_name(codec, src_components, mip_filter).decode()


# ---- mip chains of the ETC2 family (EXTENSION, include/ic_amd.h): the pixel pyramid, then every level in one encode launch ----
def etc2_mip_chain_size(codec, height, width, levels=None):
    """mip_chain_size for ETC2_RGBA8 / ETC2_RGB8 / ETC2_RGB8A1 / EAC_R11 / EAC_RG11: (bytes of one image's chain, [offset of
    level l for l in 0..levels]); (0, None) where the codec / size / level count is refused."""
    if levels is None:
        levels = mip_max_levels(height, width)
    offs = (ctypes.c_size_t * (max(levels, 0) + 1))()
    n = lib().icamd_etc2_mip_chain_size(codec, height, width, levels, offs)
    return (n, list(offs)) if n else (0, None)


def etc2_mip_workspace_size(codec, src_components, height, width, levels=None, n_images=1):
    if levels is None:
        levels = mip_max_levels(height, width)
    return lib().icamd_etc2_mip_workspace_size(codec, src_components, height, width, levels, n_images)


def encode_etc2_mips_device(codec, src, height, width, src_components, *, levels=None, swap_rb=False,
                            etc_strategy=ETC_SMALLER_ERROR, etc2_modes=0, mip_filter=0, n_images=1, row_stride_bytes=None,
                            src_image_stride_bytes=None, dst_image_stride_bytes=None, out=None, workspace=None, stream=None):
    """Mip-chain encode of the ETC2 family (icamd_encode_etc2_mips_device) of `src` (a torch.uint8 CUDA tensor, contiguous
    bytes): etc2_modes as encode_etc2_device (ETC2_MODES_TH with ETC2_RGB8 only), mip_filter as encode_mips_device
    (MIP_FILTER_NORMAL for EAC_RG11 from two-byte pixels).  Returns (flat, views) as encode_mips_device does: flat is
    [n_images, dst_image_stride] (device), views[l] the blocks of level l.  The workspace is allocated here unless the caller
    passes one (a uint8 CUDA tensor of at least etc2_mip_workspace_size bytes).  No synchronisation."""
    _assert_u8_cuda(src)
    if levels is None:
        levels = mip_max_levels(height, width)
    stride = width * src_components if row_stride_bytes is None else row_stride_bytes
    img_stride = height * stride if src_image_stride_bytes is None else src_image_stride_bytes
    total, offs = etc2_mip_chain_size(codec, height, width, levels)
    per = total if dst_image_stride_bytes is None else dst_image_stride_bytes
    if out is None:
        out = torch.empty((n_images, max(per, 1)), dtype=torch.uint8, device=src.device)
    _check_out(out, n_images, per, "encode_etc2_mips_device")
    ws_bytes = etc2_mip_workspace_size(codec, src_components, height, width, levels, n_images) if total else 0
    if workspace is None and ws_bytes:
        workspace = torch.empty((ws_bytes,), dtype=torch.uint8, device=src.device)
    if workspace is not None and not (workspace.is_cuda and workspace.dtype == torch.uint8 and workspace.is_contiguous()):
        raise ValueError("encode_etc2_mips_device: workspace must be a contiguous uint8 CUDA tensor")
    ws_ptr = _ptr(workspace) if workspace is not None else None
    ws_len = workspace.numel() if workspace is not None else 0
    st = lib().icamd_encode_etc2_mips_device(codec, etc_strategy, etc2_modes, src_components, int(swap_rb), mip_filter, height,
                                             width, stride, levels, n_images, img_stride, per, _ptr(src), _ptr(out), ws_ptr,
                                             ws_len, _stream_handle(stream))
    if not _check(st, "icamd_encode_etc2_mips_device") or offs is None:
        return None
    return out, [out[:, offs[l]:offs[l + 1]] for l in range(levels)]


def etc2_mip_kernel_name(codec, src_components, etc_strategy=ETC_SMALLER_ERROR, etc2_modes=0):
    """Name of the kernel of the chain's encode launch -- with ETC2_MODES_TH of its T / H launch -- ("" if refused)."""
    return lib().icamd_etc2_mip_kernel_name(codec, src_components, etc_strategy, etc2_modes).decode()


def etc2_mip_tune(level_order=1):
    """Measurement knob: 1 = the largest level's workgroups first in the encode launch (default), 0 = the smallest's.  Time
    only, never bytes."""
    _require_ok(lib().icamd_etc2_mip_tune(level_order), "icamd_etc2_mip_tune")


# ---- quality metric (icamd_measure_error_device): compressed blocks against their source pixels

ERROR_STATS_BYTES = 48  # sizeof(icamd_error_stats): uint64 sse[4], uint32 max_abs[4]


def metric_kernel_name(codec, src_components):
    return lib().icamd_metric_kernel_name(codec, src_components).decode()


def _split_stats(raw):
    """[n, 48] uint8 records -> ([n, 4] int64 sse, [n, 4] int32 max_abs); same device, no synchronisation."""
    return raw[:, :32].contiguous().view(torch.int64), raw[:, 32:].contiguous().view(torch.int32)


def measure_error_device(codec, src, blocks, height, width, src_components, *, swap_rb=False, grid_height=None,
                         grid_width=None, row_stride_bytes=None, n_images=1, src_image_stride_bytes=None,
                         blocks_image_stride_bytes=None, out=None, stream=None):
    """icamd_measure_error_device: the error of `blocks` (torch.uint8 CUDA tensor, laid out as encode_device writes them for
    the grid) against the pixels `src` (as encode_device reads them), per image and channel.  Returns ([n, 4] int64 sums of
    squared differences, [n, 4] int32 largest absolute differences) as device tensors, or None where the call answers false.
    `out`: a caller-owned [n_images, 48] uint8 device tensor for the raw records (e.g. under graph capture).  No
    synchronisation; the records are overwritten by stream-ordered work of the call."""
    _assert_u8_cuda(src)
    _assert_u8_cuda(blocks)
    gh = height if grid_height is None else grid_height
    gw = width if grid_width is None else grid_width
    stride = width * src_components if row_stride_bytes is None else row_stride_bytes
    img_stride = height * stride if src_image_stride_bytes is None else src_image_stride_bytes
    blk_stride = encoded_size(codec, max(gh, height), max(gw, width)) if blocks_image_stride_bytes is None \
        else blocks_image_stride_bytes
    if out is None:
        out = torch.empty((n_images, ERROR_STATS_BYTES), dtype=torch.uint8, device=src.device)
    else:
        _check_out(out, n_images, ERROR_STATS_BYTES, "measure_error_device")
    st = lib().icamd_measure_error_device(codec, src_components, int(swap_rb), height, width, gh, gw, stride, n_images,
                                          img_stride, blk_stride, _ptr(src), _ptr(blocks), _ptr(out), _stream_handle(stream))
    if not _check(st, "icamd_measure_error_device"):
        return None
    return _split_stats(out)


def measure_error_host(compressor, fmt, buffer, blocks, height, width, *, padding_bytes_per_row=0):
    """icamd_measure_error (host buffers): (sse, max_abs) as two numpy arrays of 4, or None where the call answers false."""
    import numpy as np
    src, b = _host_u8(buffer), _host_u8(blocks)
    rec = np.zeros(ERROR_STATS_BYTES, np.uint8)
    st = lib().icamd_measure_error(compressor, fmt, height, width, padding_bytes_per_row, src.ctypes.data, b.ctypes.data,
                                   b.size, rec.ctypes.data)
    if not _check(st, "icamd_measure_error"):
        return None
    return rec[:32].view(np.uint64).astype(np.int64), rec[32:].view(np.uint32).astype(np.int64)


def psnr_from_stats(sse, n_pixels, n_channels):
    """10 log10(255^2 N C / SSE) for the summed squared error of N pixels x C channels; inf for a perfect match."""
    import math
    total = float(sse.sum()) if hasattr(sse, "sum") else float(sum(sse))
    return math.inf if total == 0 else 10.0 * math.log10(255.0 ** 2 * n_pixels * n_channels / total)


# ---- 16-bit and signed EAC R11 / RG11 (include/ic_amd.h icamd_encode_eac11_16_device)
# codec: EAC_R11 / EAC_RG11 (uint16 samples) or EAC_SIGNED_R11 / EAC_SIGNED_RG11 (int16 samples).  Pixel tensors may be
# torch.uint16 / torch.int16 (one element per sample) or torch.uint8 (the same memory as little-endian bytes); blocks are
# torch.uint8.  Strides and paddings are always in BYTES.

def _eac11_16_signed(codec):
    return codec in (EAC_SIGNED_R11, EAC_SIGNED_RG11)


def _assert_samples_cuda(t):
    assert t.is_cuda and t.is_contiguous() and t.dtype in (torch.uint8, torch.uint16, torch.int16)


def eac11_16_kernel_name(codec, src_channels, metric=False):
    """icamd_eac11_16_kernel_name, or with metric=True icamd_eac11_16_metric_kernel_name; "" for a refused combination."""
    fn = lib().icamd_eac11_16_metric_kernel_name if metric else lib().icamd_eac11_16_kernel_name
    return fn(codec, src_channels).decode()


def encode_eac11_16_device(codec, src, height, width, src_channels, *, grid_height=None, grid_width=None, row_stride_bytes=None,
                           n_images=1, src_image_stride_bytes=None, out=None, stream=None):
    """icamd_encode_eac11_16_device on `src`: a contiguous CUDA tensor of torch.uint16 (unsigned codecs) / torch.int16 (signed)
    samples, src_channels per pixel, or the same bytes as torch.uint8.  Returns the torch.uint8 blocks [n_images, encoded_size]
    (device), or None where the call answers false.  No synchronisation."""
    _assert_samples_cuda(src)
    gh = height if grid_height is None else max(grid_height, height)
    gw = width if grid_width is None else max(grid_width, width)
    stride = width * src_channels * 2 if row_stride_bytes is None else row_stride_bytes
    img_stride = height * stride if src_image_stride_bytes is None else src_image_stride_bytes
    per = encoded_size(codec, gh, gw)
    if out is None:
        out = torch.empty((n_images, per), dtype=torch.uint8, device=src.device)
    else:
        _check_out(out, n_images, per, "encode_eac11_16_device")
    st = lib().icamd_encode_eac11_16_device(codec, src_channels, height, width, gh, gw, stride, n_images, img_stride, per,
                                            _ptr(src), _ptr(out), _stream_handle(stream))
    return out if _check(st, "icamd_encode_eac11_16_device") else None


def decode_eac11_16_device(codec, blocks, height, width, *, padding_bytes_per_row=0, n_images=1, stream=None):
    """icamd_decode_eac11_16_device: torch.uint8 blocks -> a [n_images, height * (width * channels + padding_bytes_per_row / 2)]
    tensor of torch.uint16 (unsigned codecs) or torch.int16 (signed) samples, channels = 1 (R11) or 2 (RG11, R then G); the
    padding samples are zero.  None where the call answers false.  No synchronisation."""
    _assert_u8_cuda(blocks)
    chans = 2 if codec in (EAC_RG11, EAC_SIGNED_RG11) else 1
    per_out = height * (width * chans * 2 + padding_bytes_per_row)
    out = torch.zeros((n_images, per_out), dtype=torch.uint8, device=blocks.device)
    st = lib().icamd_decode_eac11_16_device(codec, height, width, padding_bytes_per_row, n_images, encoded_size(codec, height, width),
                                            per_out, _ptr(blocks), _ptr(out), _stream_handle(stream))
    if not _check(st, "icamd_decode_eac11_16_device"):
        return None
    return out.view(torch.int16 if _eac11_16_signed(codec) else torch.uint16)


def measure_error_eac11_16_device(codec, src, blocks, height, width, src_channels, *, grid_height=None, grid_width=None,
                                  row_stride_bytes=None, n_images=1, src_image_stride_bytes=None, blocks_image_stride_bytes=None,
                                  out=None, stream=None):
    """icamd_measure_error_eac11_16_device: `blocks` (torch.uint8, as encode_eac11_16_device writes them for the grid) against
    the samples `src` (as encode_eac11_16_device reads them).  Returns ([n, 4] int64 sums of squared 16-bit differences, [n, 4]
    int32 largest absolute differences; entries 0 = R, 1 = G) as device tensors, or None where the call answers false.  `out`: a
    caller-owned [n_images, 48] uint8 device tensor for the raw records.  No synchronisation."""
    _assert_samples_cuda(src)
    _assert_u8_cuda(blocks)
    gh = height if grid_height is None else grid_height
    gw = width if grid_width is None else grid_width
    stride = width * src_channels * 2 if row_stride_bytes is None else row_stride_bytes
    img_stride = height * stride if src_image_stride_bytes is None else src_image_stride_bytes
    blk_stride = encoded_size(codec, max(gh, height), max(gw, width)) if blocks_image_stride_bytes is None \
        else blocks_image_stride_bytes
    if out is None:
        out = torch.empty((n_images, ERROR_STATS_BYTES), dtype=torch.uint8, device=src.device)
    else:
        _check_out(out, n_images, ERROR_STATS_BYTES, "measure_error_eac11_16_device")
    st = lib().icamd_measure_error_eac11_16_device(codec, src_channels, height, width, gh, gw, stride, n_images, img_stride,
                                                   blk_stride, _ptr(src), _ptr(blocks), _ptr(out), _stream_handle(stream))
    if not _check(st, "icamd_measure_error_eac11_16_device"):
        return None
    return _split_stats(out)


def psnr16_from_stats(sse, n_pixels, n_channels, signed=False):
    """10 log10(peak^2 N C / SSE) of 16-bit samples, peak 65535 (unsigned) or 32767 (signed); inf for a perfect match."""
    import math
    total = float(sse.sum()) if hasattr(sse, "sum") else float(sum(sse))
    peak = 32767.0 if signed else 65535.0
    return math.inf if total == 0 else 10.0 * math.log10(peak ** 2 * n_pixels * n_channels / total)


# ---- BC6H (include/ic_amd.h icamd_encode_bc6h_device)
# codec: BC6H_UF16 or BC6H_SF16.  Pixel tensors are torch.float16 (one element per sample), or the same bits as torch.int16 /
# torch.uint16, or the same memory as torch.uint8 (little-endian bytes); all four are accepted.  Blocks are torch.uint8.  Strides
# and paddings are always in BYTES.

def _assert_halves_cuda(t):
    assert t.is_cuda and t.is_contiguous() and t.dtype in (torch.float16, torch.int16, torch.uint16, torch.uint8)


def bc6h_kernel_name(codec, src_channels, metric=False):
    """icamd_bc6h_kernel_name, or with metric=True icamd_bc6h_metric_kernel_name; "" for a refused combination."""
    fn = lib().icamd_bc6h_metric_kernel_name if metric else lib().icamd_bc6h_kernel_name
    return fn(codec, src_channels).decode()


def encode_bc6h_device(codec, src, height, width, src_channels, *, grid_height=None, grid_width=None, row_stride_bytes=None,
                       n_images=1, src_image_stride_bytes=None, out=None, stream=None):
    """icamd_encode_bc6h_device on `src`: a contiguous CUDA tensor of halves (see above), src_channels (3 or 4) per pixel.
    Returns the torch.uint8 blocks [n_images, encoded_size] (device), or None where the call answers false.  No synchronisation."""
    _assert_halves_cuda(src)
    gh = height if grid_height is None else max(grid_height, height)
    gw = width if grid_width is None else max(grid_width, width)
    stride = width * src_channels * 2 if row_stride_bytes is None else row_stride_bytes
    img_stride = height * stride if src_image_stride_bytes is None else src_image_stride_bytes
    per = encoded_size(codec, gh, gw)
    if out is None:
        out = torch.empty((n_images, per), dtype=torch.uint8, device=src.device)
    else:
        _check_out(out, n_images, per, "encode_bc6h_device")
    st = lib().icamd_encode_bc6h_device(codec, src_channels, height, width, gh, gw, stride, n_images, img_stride, per,
                                        _ptr(src), _ptr(out), _stream_handle(stream))
    return out if _check(st, "icamd_encode_bc6h_device") else None


def encode_bc6h_modes_device(codec, src, height, width, src_channels, *, bc6h_modes=BC6H_MODES_DEFAULT, grid_height=None,
                             grid_width=None, row_stride_bytes=None, n_images=1, src_image_stride_bytes=None, out=None, stream=None):
    """icamd_encode_bc6h_modes_device: encode_bc6h_device with a choice of modes -- BC6H_MODES_DEFAULT (encode_bc6h_device itself)
    or BC6H_MODES_EXTENDED (the fused kernel with the two-subset candidate).  Returns the torch.uint8 blocks
    [n_images, encoded_size] (device), or None where the call answers false.  No synchronisation."""
    _assert_halves_cuda(src)
    gh = height if grid_height is None else max(grid_height, height)
    gw = width if grid_width is None else max(grid_width, width)
    stride = width * src_channels * 2 if row_stride_bytes is None else row_stride_bytes
    img_stride = height * stride if src_image_stride_bytes is None else src_image_stride_bytes
    per = encoded_size(codec, gh, gw)
    if out is None:
        out = torch.empty((n_images, per), dtype=torch.uint8, device=src.device)
    else:
        _check_out(out, n_images, per, "encode_bc6h_modes_device")
    st = lib().icamd_encode_bc6h_modes_device(codec, bc6h_modes, src_channels, height, width, gh, gw, stride, n_images, img_stride,
                                              per, _ptr(src), _ptr(out), _stream_handle(stream))
    return out if _check(st, "icamd_encode_bc6h_modes_device") else None


def bc6h_modes_kernel_name(codec, src_channels, bc6h_modes):
    """icamd_bc6h_modes_kernel_name: the kernel that writes the final bytes (BC6H_MODES_DEFAULT: what bc6h_kernel_name answers);
    "" if refused."""
    return lib().icamd_bc6h_modes_kernel_name(codec, src_channels, bc6h_modes).decode()


# ---- half-float pixel pyramid and the mip chains of BC7 and BC6H (EXTENSION, include/ic_amd.h)
def mip_f16_kernel_name(src_channels):
    """icamd_mip_f16_kernel_name: the half-float pyramid's kernel; "" unless src_channels is 3 or 4."""
    return lib().icamd_mip_f16_kernel_name(src_channels).decode()


def mip_pyramid_f16_device(src, height, width, src_channels, *, levels=None, n_images=1, row_stride_bytes=None,
                           src_image_stride_bytes=None, dst_image_stride_bytes=None, out=None, stream=None):
    """icamd_mip_pyramid_f16_device on `src`, a contiguous CUDA tensor of halves (torch.float16, or the same bits as int16 /
    uint16 / uint8).  Returns (flat, views) as mip_pyramid_device does: flat is [n_images, dst_image_stride] torch.uint8, views[l - 1]
    level l as a [n_images, h_l, w_l, src_channels] torch.float16 view, for l = 1 .. levels-1.  No synchronisation."""
    _assert_halves_cuda(src)
    if levels is None:
        levels = mip_max_levels(height, width)
    stride = width * src_channels * 2 if row_stride_bytes is None else row_stride_bytes
    img_stride = height * stride if src_image_stride_bytes is None else src_image_stride_bytes
    total, offs = mip_pyramid_size(src_channels * 2, height, width, levels)
    per = total if dst_image_stride_bytes is None else dst_image_stride_bytes
    if out is None:
        out = torch.empty((n_images, max(per, 1)), dtype=torch.uint8, device=src.device)
    _check_out(out, n_images, per, "mip_pyramid_f16_device")
    st = lib().icamd_mip_pyramid_f16_device(src_channels, height, width, stride, levels, n_images, img_stride, per, _ptr(src),
                                            _ptr(out), _stream_handle(stream))
    if not _check(st, "icamd_mip_pyramid_f16_device"):
        return None
    views = []
    for l in range(1, levels):
        h, w = mip_level_shape(height, width, l)
        views.append(out[:, offs[l - 1]:offs[l]].view(torch.float16).view(n_images, h, w, src_channels))
    return out, views


def bptc_mip_chain_size(codec, height, width, levels=None):
    """mip_chain_size for BC7 / BC6H_UF16 / BC6H_SF16: (bytes of one image's chain, [offset of level l for l in 0..levels]);
    (0, None) where the codec / size / level count is refused."""
    if levels is None:
        levels = mip_max_levels(height, width)
    offs = (ctypes.c_size_t * (max(levels, 0) + 1))()
    n = lib().icamd_bptc_mip_chain_size(codec, height, width, levels, offs)
    return (n, list(offs)) if n else (0, None)


def bptc_mip_workspace_size(codec, src_channels, height, width, levels=None, n_images=1):
    if levels is None:
        levels = mip_max_levels(height, width)
    return lib().icamd_bptc_mip_workspace_size(codec, src_channels, height, width, levels, n_images)


def _encode_bptc_mips(what, call, codec, src, height, width, pixel_bytes, src_channels, levels, n_images, row_stride_bytes,
                      src_image_stride_bytes, dst_image_stride_bytes, out, workspace, stream):
    if levels is None:
        levels = mip_max_levels(height, width)
    stride = width * pixel_bytes if row_stride_bytes is None else row_stride_bytes
    img_stride = height * stride if src_image_stride_bytes is None else src_image_stride_bytes
    total, offs = bptc_mip_chain_size(codec, height, width, levels)
    per = total if dst_image_stride_bytes is None else dst_image_stride_bytes
    if out is None:
        out = torch.empty((n_images, max(per, 1)), dtype=torch.uint8, device=src.device)
    _check_out(out, n_images, per, what)
    ws_bytes = bptc_mip_workspace_size(codec, src_channels, height, width, levels, n_images) if total else 0
    if workspace is None and ws_bytes:
        workspace = torch.empty((ws_bytes,), dtype=torch.uint8, device=src.device)
    if workspace is not None and not (workspace.is_cuda and workspace.dtype == torch.uint8 and workspace.is_contiguous()):
        raise ValueError("%s: workspace must be a contiguous uint8 CUDA tensor" % what)
    ws_ptr = _ptr(workspace) if workspace is not None else None
    ws_len = workspace.numel() if workspace is not None else 0
    st = call(height, width, stride, levels, n_images, img_stride, per, _ptr(src), _ptr(out), ws_ptr, ws_len, _stream_handle(stream))
    if not _check(st, "icamd_" + what) or offs is None:
        return None
    return out, [out[:, offs[l]:offs[l + 1]] for l in range(levels)]


def encode_bc7_mips_device(src, height, width, src_components, *, bc7_modes=BC7_MODES_DEFAULT, levels=None, swap_rb=False,
                           mip_filter=0, n_images=1, row_stride_bytes=None, src_image_stride_bytes=None,
                           dst_image_stride_bytes=None, out=None, workspace=None, stream=None):
    """BC7 mip chain (icamd_encode_bc7_mips_device) of `src` (a torch.uint8 CUDA tensor, contiguous bytes): bc7_modes as
    encode_bc7_device, mip_filter 0 .. 3 as encode_mips_device.  Returns (flat, views) as encode_etc2_mips_device does.  The
    workspace is allocated here unless the caller passes one (at least bptc_mip_workspace_size bytes).  No synchronisation."""
    _assert_u8_cuda(src)
    fn = lib().icamd_encode_bc7_mips_device
    return _encode_bptc_mips("encode_bc7_mips_device", lambda *tail: fn(bc7_modes, src_components, int(swap_rb), mip_filter, *tail),
                             BC7, src, height, width, src_components, src_components, levels, n_images, row_stride_bytes,
                             src_image_stride_bytes, dst_image_stride_bytes, out, workspace, stream)


def encode_bc6h_mips_device(codec, src, height, width, src_channels, *, bc6h_modes=BC6H_MODES_DEFAULT, levels=None, n_images=1,
                            row_stride_bytes=None, src_image_stride_bytes=None, dst_image_stride_bytes=None, out=None,
                            workspace=None, stream=None):
    """BC6H mip chain (icamd_encode_bc6h_mips_device) of `src`, a contiguous CUDA tensor of halves as encode_bc6h_device takes
    them: bc6h_modes as encode_bc6h_modes_device.  Returns (flat, views) as encode_etc2_mips_device does.  No synchronisation."""
    _assert_halves_cuda(src)
    fn = lib().icamd_encode_bc6h_mips_device
    return _encode_bptc_mips("encode_bc6h_mips_device", lambda *tail: fn(codec, bc6h_modes, src_channels, *tail), codec, src,
                             height, width, src_channels * 2, src_channels, levels, n_images, row_stride_bytes,
                             src_image_stride_bytes, dst_image_stride_bytes, out, workspace, stream)


def bptc_mip_kernel_name(codec, src_channels, modes=0):
    """Name of the kernel of the chain's encode launch ("" if refused); modes: BC7_MODES_* / BC6H_MODES_*."""
    return lib().icamd_bptc_mip_kernel_name(codec, src_channels, modes).decode()


def decode_bc6h_device(codec, blocks, height, width, *, padding_bytes_per_row=0, n_images=1, stream=None):
    """icamd_decode_bc6h_device: torch.uint8 blocks -> a [n_images, height * (width * 4 + padding_bytes_per_row / 2)] tensor of
    torch.float16: RGBA16F rows, A = 1; the padding samples are zero.  None where the call answers false.  No synchronisation."""
    _assert_u8_cuda(blocks)
    per_out = height * (width * 8 + padding_bytes_per_row)
    out = torch.zeros((n_images, per_out), dtype=torch.uint8, device=blocks.device)
    st = lib().icamd_decode_bc6h_device(codec, height, width, padding_bytes_per_row, n_images, encoded_size(codec, height, width),
                                        per_out, _ptr(blocks), _ptr(out), _stream_handle(stream))
    if not _check(st, "icamd_decode_bc6h_device"):
        return None
    return out.view(torch.float16)


def measure_error_bc6h_device(codec, src, blocks, height, width, src_channels, *, grid_height=None, grid_width=None,
                              row_stride_bytes=None, n_images=1, src_image_stride_bytes=None, blocks_image_stride_bytes=None,
                              out=None, stream=None):
    """icamd_measure_error_bc6h_device: `blocks` (torch.uint8, as encode_bc6h_device writes them for the grid) against the halves
    `src` (as encode_bc6h_device reads them).  Returns ([n, 4] int64 sums of squared t-domain differences, [n, 4] int32 largest
    absolute differences; entries 0, 1, 2 = R, G, B) as device tensors, or None where the call answers false.  `out`: a
    caller-owned [n_images, 48] uint8 device tensor for the raw records.  No synchronisation."""
    _assert_halves_cuda(src)
    _assert_u8_cuda(blocks)
    gh = height if grid_height is None else grid_height
    gw = width if grid_width is None else grid_width
    stride = width * src_channels * 2 if row_stride_bytes is None else row_stride_bytes
    img_stride = height * stride if src_image_stride_bytes is None else src_image_stride_bytes
    blk_stride = encoded_size(codec, max(gh, height), max(gw, width)) if blocks_image_stride_bytes is None \
        else blocks_image_stride_bytes
    if out is None:
        out = torch.empty((n_images, ERROR_STATS_BYTES), dtype=torch.uint8, device=src.device)
    else:
        _check_out(out, n_images, ERROR_STATS_BYTES, "measure_error_bc6h_device")
    st = lib().icamd_measure_error_bc6h_device(codec, src_channels, height, width, gh, gw, stride, n_images, img_stride,
                                               blk_stride, _ptr(src), _ptr(blocks), _ptr(out), _stream_handle(stream))
    if not _check(st, "icamd_measure_error_bc6h_device"):
        return None
    return _split_stats(out)


def psnr_bc6h_from_stats(sse, n_pixels, n_channels=3):
    """10 log10(peak^2 N C / SSE) in the t domain, peak 31743 (the largest finite half's bit pattern); inf for a perfect match."""
    import math
    total = float(sse.sum()) if hasattr(sse, "sum") else float(sum(sse))
    return math.inf if total == 0 else 10.0 * math.log10(31743.0 ** 2 * n_pixels * n_channels / total)
