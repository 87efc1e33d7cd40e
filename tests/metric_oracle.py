"""The quality metric's definition (include/ic_amd.h, icamd_measure_error_device) computed with numpy from the oracle's
decoders: for every compared channel k, sse[k] = sum over the image of (S - D)^2 and max_abs[k] = max |S - D|, where D is what
the decoder yields for the image's blocks and S the source pixels.  Uncompared channels are 0.

Shared by tests/test_metric_host.py (CPU tier), tests/test_gpu_metric.py (GPU tier) and the scripts that check the metric."""
import numpy as np

import bc45_oracle as B
import ic_testlib as T

DXT1, DXT5, ETC1, PVRTC2, PVRTC4, BC4, BC5 = 0, 1, 2, 3, 4, 5, 6

# (codec, src_components, swap_rb) of every source layout icamd_measure_error_device accepts
BLOCK_LAYOUTS = [(DXT1, 3, 0), (DXT1, 3, 1), (DXT1, 4, 0), (DXT1, 4, 1), (DXT5, 4, 0), (DXT5, 4, 1),
                 (ETC1, 3, 0), (ETC1, 3, 1), (ETC1, 4, 0), (ETC1, 4, 1)] + list(B.LAYOUTS)
PVRTC_LAYOUTS = [(PVRTC2, 4, 0), (PVRTC4, 4, 0)]


def block_bytes(codec):
    return 16 if codec in (DXT5, BC5) else 8


def grid_bytes(codec, gh, gw):
    if codec == PVRTC2:
        return gh * gw // 4
    if codec == PVRTC4:
        return gh * gw // 2
    return ((gh + 3) // 4) * ((gw + 3) // 4) * block_bytes(codec)


def channel_pairs(codec, comps, swap):
    """[(k, source byte, decoded channel)] of the compared channels."""
    if codec in (DXT1, ETC1):
        return [(k, k, k) for k in range(3)]
    if codec in (DXT5, PVRTC2, PVRTC4):
        return [(k, k, k) for k in range(4)]
    r = 2 if (swap and comps >= 3) else 0
    return [(0, r, 0)] if codec == BC4 else [(0, r, 0), (1, 1, 1)]


def image_blocks(codec, blocks, h, w, gh=None, gw=None):
    """The blocks that cover the h x w image out of a row-major grid of max(gh, h) x max(gw, w) pixels."""
    gh = h if gh is None else max(gh, h)
    gw = w if gw is None else max(gw, w)
    b = np.frombuffer(bytes(blocks), np.uint8)
    if codec in (PVRTC2, PVRTC4) or (gh == h and gw == w):
        return b.tobytes()
    bb = block_bytes(codec)
    grid = b.reshape((gh + 3) // 4, (gw + 3) // 4, bb)
    return np.ascontiguousarray(grid[:(h + 3) // 4, :(w + 3) // 4]).tobytes()


def decode(codec, blocks, h, w, swap=0):
    """(h, w, channels) uint8: what icamd_decode_device(codec, swap) yields."""
    if codec in (BC4, BC5):
        return B.oracle_decode(codec, blocks, h, w).reshape(h, w, B.comps_out(codec))
    out = T.oracle_decode(codec, blocks, h, w, swap=0 if codec in (PVRTC2, PVRTC4) else swap)
    assert out is not None
    return out.reshape(h, w, -1)


def stats_of(src, dec, codec, comps, swap=0):
    """(sse int64[4], max_abs int64[4]) of source pixels (h, w, comps) against decoded pixels (h, w, channels)."""
    sse, mx = np.zeros(4, np.int64), np.zeros(4, np.int64)
    for k, sb, dc in channel_pairs(codec, comps, swap):
        d = src[..., sb].astype(np.int64) - dec[..., dc].astype(np.int64)
        sse[k] = int((d * d).sum())
        mx[k] = int(np.abs(d).max())
    return sse, mx


def measure(codec, src, blocks, h, w, comps, swap=0, gh=None, gw=None):
    """The definition: src = the image's pixels, anything that reshapes to (h, w, comps) (no row padding)."""
    src = np.asarray(src, np.uint8).reshape(h, w, comps)
    return stats_of(src, decode(codec, image_blocks(codec, blocks, h, w, gh, gw), h, w, swap), codec, comps, swap)


def psnr(sse, n_pixels, n_channels):
    total = float(np.asarray(sse, np.float64).sum())
    return float("inf") if total == 0 else 10.0 * np.log10(255.0 ** 2 * n_pixels * n_channels / total)
