"""The block-walk cases of the decode and metric kernels: one table of kernel families and one set of case generators, plain
numpy, no GPU.  Every decode and metric kernel cuts a flat block index k with fastdiv into image, block row and block column;
workgroups cover consecutive indices, 256 per workgroup in the decoders (one block per lane) and 1024 in the metrics (lane t holds
blocks t, t + 256, t + 512 and t + 768).  The metric walk exists once (metric_walk of csrc/metric_walk.inc; the kernels of
csrc/metric_kernels.hip, csrc/eac11_16_kernels.hip and csrc/bc6h_kernels.hip bring their accumulators and per-block bodies) and
chooses between one commit per workgroup, one per wave whose lanes agree on the image, and one per lane; the raster decoder
bodies cut their index with raster_block of csrc/ic_launch.h.  The regimes below are the shapes at which those choices and the
last workgroup's occupancy differ.

tests/test_walk_cases_host.py (CPU tier) restates the walk and holds every regime to what it is named for, and runs every
definition once; tests/test_gpu_walk_regimes.py (GPU tier) runs the kernels.  Expected values come from the existing oracles
(tests/*_oracle.py, tests/ic_testlib.py): the blocks of a batch are decoded once per definition and regime, and the layouts of
one definition share the result."""
import functools
from collections import namedtuple

import numpy as np

import bc45_oracle as B45
import bc6h_oracle as B6
import bc7_oracle as B7
import eac11_16_oracle as E16
import eac11_oracle as E11
import etc2_a1_oracle as A1
import etc2_colour_oracle as C
import etc2_oracle as E2
import ic_testlib as T
import metric_oracle as M

DXT1, DXT5, ETC1, PVRTC2, PVRTC4, BC4, BC5 = M.DXT1, M.DXT5, M.ETC1, M.PVRTC2, M.PVRTC4, M.BC4, M.BC5
ETC2_RGBA8, ETC2_RGB8, EAC_R11, EAC_RG11, ETC2_RGB8A1, BC7 = 16, 18, 19, 20, 21, 32
METRIC_BLOCKS_PER_WORKGROUP, DECODE_BLOCKS_PER_WORKGROUP = 1024, 256

# ---- the definitions: what decodes a block stream, shared by every layout that reads it
# name: (block bytes, decoded channels, compared channels (None: as many as the source has), pixel kind)
DEFINITIONS = {
    "dxt1": (8, 3, 3, "rgba8"), "dxt5": (16, 4, 4, "rgba8"), "etc1": (8, 3, 3, "rgba8"),
    "etc2_rgba8": (16, 4, 4, "rgba8"), "etc2_rgb8": (8, 3, 3, "rgba8"), "etc2_rgb8a1": (8, 4, 4, "rgba8"),
    "bc4": (8, 1, 1, "rgba8"), "bc5": (16, 2, 2, "rgba8"), "eac_r11": (8, 1, 1, "rgba8"), "eac_rg11": (16, 2, 2, "rgba8"),
    "bc7": (16, 4, None, "rgba8"),
    "eac16_r11": (8, 1, 1, "u16"), "eac16_rg11": (16, 2, 2, "u16"), "eac16_signed_r11": (8, 1, 1, "s16"),
    "eac16_signed_rg11": (16, 2, 2, "s16"),
    "bc6h_uf16": (16, 4, 3, "half"), "bc6h_sf16": (16, 4, 3, "half"),
    "pvrtc2": (8, 4, 4, "rgba8"), "pvrtc4": (8, 4, 4, "rgba8"),
}
EAC16_CODEC = {"eac16_r11": E16.EAC_R11, "eac16_rg11": E16.EAC_RG11, "eac16_signed_r11": E16.EAC_SIGNED_R11,
               "eac16_signed_rg11": E16.EAC_SIGNED_RG11}

# name: the test id.  kind: "metric" or "decode".  entry: the wrapper of image-compression_amd (metrics: they take every stride
# and `out`) or the C ABI function through pkg.lib() (decoders: the wrappers allocate the output and take no image strides).
# comps, sample_bytes: the source layout of a metric; pixel_bytes: what a decoder writes per pixel.
Family = namedtuple("Family", "name kind entry codec comps sample_bytes pixel_bytes definition")


def _m(name, entry, codec, comps, definition, sample_bytes=1):
    return Family(name, "metric", entry, codec, comps, sample_bytes, 0, definition)


def _d(name, entry, codec, pixel_bytes, definition):
    return Family(name, "decode", entry, codec, 0, 0, pixel_bytes, definition)


_SRC8 = {1: "r8", 2: "rg8", 3: "rgb888", 4: "rgba8"}
_SRC16 = {1: "r16", 2: "rg16", 3: "rgb16", 4: "rgba16"}
METRIC_FAMILIES = (
    # kMetricKernels of csrc/metric_kernels.hip: metric_walk with a workgroup commit through LDS (metric_raster), and the PVRTC
    # raster and tile forms (the shape chooses)
    [_m("metric_%s_%s" % (d, _SRC8[c]), "measure_error_device", codec, c, d) for d, codec, comps in [
        ("dxt1", DXT1, (3, 4)), ("dxt5", DXT5, (4,)), ("etc1", ETC1, (3, 4)), ("etc2_rgba8", ETC2_RGBA8, (4,)),
        ("etc2_rgb8", ETC2_RGB8, (3, 4)), ("etc2_rgb8a1", ETC2_RGB8A1, (4,)), ("bc4", BC4, (1, 2, 3, 4)), ("bc5", BC5, (2, 3, 4)),
        ("eac_r11", EAC_R11, (1, 2, 3, 4)), ("eac_rg11", EAC_RG11, (2, 3, 4)), ("bc7", BC7, (3, 4)), ("pvrtc2", PVRTC2, (4,)),
        ("pvrtc4", PVRTC4, (4,))] for c in comps] +
    # ICAMD_EAC16_METRIC_KERNELS of csrc/eac11_16_kernels.hip: eac11_16_metric, metric_walk with 64-bit sums of 2 channels
    [_m("metric_%s_%s" % (d, _SRC16[c]), "measure_error_eac11_16_device", EAC16_CODEC[d], c, d, sample_bytes=2)
     for d in ("eac16_r11", "eac16_rg11", "eac16_signed_r11", "eac16_signed_rg11") for c in range(DEFINITIONS[d][2], 5)] +
    # ICAMD_BC6H_KERNELS of csrc/bc6h_kernels.hip: bc6h_metric, metric_walk with 64-bit sums of 3 channels
    [_m("metric_%s_%s" % (d, {3: "rgb16f", 4: "rgba16f"}[c]), "measure_error_bc6h_device", codec, c, d, sample_bytes=2)
     for d, codec in (("bc6h_uf16", B6.BC6H_UF16), ("bc6h_sf16", B6.BC6H_SF16)) for c in (3, 4)])
DECODE_FAMILIES = [
    _d("decode_dxt1", "icamd_decode_device", DXT1, 3, "dxt1"), _d("decode_dxt5", "icamd_decode_device", DXT5, 4, "dxt5"),
    _d("decode_etc1", "icamd_decode_device", ETC1, 3, "etc1"), _d("decode_etc2_rgba8", "icamd_decode_device", ETC2_RGBA8, 4, "etc2_rgba8"),
    _d("decode_etc2_rgb8", "icamd_decode_device", ETC2_RGB8, 3, "etc2_rgb8"),
    _d("decode_etc2_rgb8a1", "icamd_decode_device", ETC2_RGB8A1, 4, "etc2_rgb8a1"), _d("decode_bc7", "icamd_decode_device", BC7, 4, "bc7"),
    _d("decode_bc6h_uf16", "icamd_decode_bc6h_device", B6.BC6H_UF16, 8, "bc6h_uf16"),
    _d("decode_bc6h_sf16", "icamd_decode_bc6h_device", B6.BC6H_SF16, 8, "bc6h_sf16"),
    _d("decode_pvrtc2", "icamd_decode_device", PVRTC2, 4, "pvrtc2"), _d("decode_pvrtc4", "icamd_decode_device", PVRTC4, 4, "pvrtc4"),
]
FAMILIES = METRIC_FAMILIES + DECODE_FAMILIES
BY_NAME = {F.name: F for F in FAMILIES}


def is_pvrtc(F):
    return F.definition in ("pvrtc2", "pvrtc4")


def block_bytes(F):
    return DEFINITIONS[F.definition][0]


def compared_channels(F):
    k = DEFINITIONS[F.definition][2]
    return F.comps if k is None else k


# ---- the regimes.  rows x cols: the block grid of one image, B = rows * cols; n images.  padded: the image lies in a larger
# stored grid with garbage around it, its rows are padded, the image strides are larger than an image and the buffers begin at
# the smallest offset the entry point accepts.
Regime = namedtuple("Regime", "name rows cols n padded")
METRIC_REGIMES = [
    Regime("one_short", 33, 31, 1, False),            # 1023 blocks: one workgroup, one lane without a block
    Regime("exact", 32, 32, 1, False),                # one full workgroup
    Regime("one_over", 41, 25, 1, False),             # 1025: the second workgroup holds one block
    Regime("image_per_workgroup", 32, 32, 3, False),  # every workgroup one image, two of them not image 0
    Regime("waves_agree", 12, 16, 7, True),           # both workgroups span images, every wave agrees
    Regime("waves_split", 8, 12, 11, True),           # 11 waves agree, 5 hold two images; then a one-image workgroup of 32
    Regime("straddle", 48, 32, 2, False),             # workgroup 0 one image, workgroup 1 both, workgroup 2 one image
    Regime("lanes_disagree", 3, 5, 300, True),        # up to 6 images a wave; the last wave: two images and 44 empty lanes
    Regime("image_per_lane", 1, 1, 1100, False),      # 64 images a wave, across two workgroups
]
DECODE_REGIMES = [
    Regime("one_short", 15, 17, 1, False),            # 255 blocks
    Regime("exact", 16, 16, 1, False),                # 256
    Regime("one_over", 1, 257, 1, False),             # 257: the second workgroup holds one block
    Regime("image_per_workgroup", 16, 16, 3, False),
    Regime("lanes_disagree", 3, 5, 300, True),
    Regime("image_per_lane", 1, 1, 1100, True),
]
# PVRTC: (size, images).  Block grids below 32 x 8 take the raster form: 8^2, 64^2 and, at 2 bpp (16 x 32 blocks of 8 x 4 pixels),
# 128^2; from 32 x 8 on the tile form, one workgroup per tile of 32 x 8 blocks.  No stored grid, no row padding (the entry points
# refuse them): the padded ones have image strides larger than an image and blocks that begin at an odd address.
PVRTC_SHAPES = [(8, 300, True), (64, 5, True), (128, 3, False), (256, 3, True)]


def pvrtc_grid(F, size):
    """(block rows, block columns) of a size x size PVRTC texture."""
    return size // 4, size // (8 if F.definition == "pvrtc2" else 4)


def pvrtc_takes_tiles(F, size):
    rows, cols = pvrtc_grid(F, size)
    return cols >= 32 and rows >= 8


def regimes(F):
    if is_pvrtc(F):
        return [Regime("pvrtc_%d" % size, *pvrtc_grid(F, size), n, padded) for size, n, padded in PVRTC_SHAPES]
    return METRIC_REGIMES if F.kind == "metric" else DECODE_REGIMES


# h, w: the image; gh, gw: the stored block grid (metrics); stride: source row stride (metrics) or decoded row stride
# (decoders); pixel_image_stride / blocks_image_stride: bytes between images; pixel_lead / blocks_lead: bytes before the buffers.
Layout = namedtuple("Layout", "h w n gh gw stride pixel_image_stride blocks_image_stride pixel_lead blocks_lead")


def image_shape(F, regime):
    """Pixel shapes clip the last block row and column; a one-block image is 3 x 2 pixels."""
    if is_pvrtc(F):
        return regime.rows * 4, regime.rows * 4
    return 4 * regime.rows - 1, 4 * regime.cols - 2


def layout(F, regime):
    h, w = image_shape(F, regime)
    px = F.comps * F.sample_bytes if F.kind == "metric" else F.pixel_bytes
    two = F.sample_bytes == 2 or F.pixel_bytes == 8  # 16-bit samples: even strides and addresses
    per_blocks = regime.rows * regime.cols * block_bytes(F)
    if not regime.padded:
        return Layout(h, w, regime.n, h, w, w * px, h * w * px, per_blocks, 0, 0)
    if is_pvrtc(F):  # (the decoders store 16 bytes at a time: the pixels stay 16-byte aligned)
        return Layout(h, w, regime.n, h, w, w * px, h * w * px + 48, per_blocks + 16, 0 if F.kind == "decode" else 1, 1)
    stride = w * px + (6 if two else 3)
    pixel_image_stride = h * stride + (38 if two else 37)
    if F.kind == "decode":  # a decoder reads the image's own grid
        return Layout(h, w, regime.n, h, w, stride, pixel_image_stride, per_blocks + 24, 2 if two else 1, 1)
    gh, gw = h + 5, w + 10  # one block row and two block columns more than the image has
    return Layout(h, w, regime.n, gh, gw, stride, pixel_image_stride, (regime.rows + 1) * (regime.cols + 2) * block_bytes(F) + 24,
                  2 if two else 1, 1)


# ---- content

def _seed(*parts):
    return T.SEED0 + 0x3A1C + sum(p * m for p, m in zip(parts, (1, 7919, 104729, 1299709)))


@functools.lru_cache(maxsize=None)
def pixels(kind, rows, cols, n, pvrtc=False):
    """(n, h, w, 4) samples of a pixel kind (read-only: shared): noise, and every fourth 4 x 4 block filled with the extremes of
    the sample's range so that max_abs reaches the top of it.  rgba8: uint8; u16 / s16: the 16-bit EAC samples; half: bit
    patterns, every one of them in the noise (NaN, Inf and denormals too), +-65504 and 0 in the extremes."""
    g = np.random.Generator(np.random.PCG64(_seed(rows, cols, n, len(kind))))
    shape = (n, 4 * rows, 4 * cols, 4)
    extreme = (g.integers(0, 4, (n, rows, cols)) == 0).repeat(4, 1).repeat(4, 2)[..., None]
    if kind == "rgba8":
        img = np.where(extreme, 255 * g.integers(0, 2, shape), g.integers(0, 256, shape)).astype(np.uint8)
    elif kind == "u16":
        img = np.where(extreme, 65535 * g.integers(0, 2, shape), g.integers(0, 65536, shape)).astype(np.uint16)
    elif kind == "s16":
        img = np.where(extreme, 65535 * g.integers(0, 2, shape) - 32768, g.integers(-32768, 32768, shape)).astype(np.int16)
    else:
        assert kind == "half"
        ends = np.array([0x7BFF, 0xFBFF, 0x0000])[g.integers(0, 3, shape)]
        img = np.where(extreme, ends, g.integers(0, 65536, shape)).astype(np.uint16)
    h, w = (4 * rows, 4 * rows) if pvrtc else (4 * rows - 1, 4 * cols - 2)
    img = np.ascontiguousarray(img[:, :h, :w])
    img.setflags(write=False)
    return img


def source(F, regime):
    """The family's source pixels: (n, h, w, comps) of its sample type, the first channels of the shared image."""
    cols = regime.rows if is_pvrtc(F) else regime.cols  # (PVRTC: square, whatever the block's width)
    return np.ascontiguousarray(pixels(DEFINITIONS[F.definition][3], regime.rows, cols, regime.n, is_pvrtc(F))[..., :F.comps])


@functools.lru_cache(maxsize=None)
def blocks(definition, rows, cols, n):
    """(n, rows * cols * block bytes) uint8: arbitrary words for the images' own grids, every decode mode among them."""
    seed = _seed(rows, cols, n, len(definition)) % (1 << 31)
    H, W = 4 * rows * n, 4 * cols  # n images as one tall grid
    d = definition
    if d in ("dxt1", "dxt5", "etc1"):
        out = T.random_blocks({"dxt1": DXT1, "dxt5": DXT5, "etc1": ETC1}[d], H, W, seed)
    elif d in ("pvrtc2", "pvrtc4"):
        out = T.random_blocks(PVRTC4, H, W, seed)[:n * rows * cols * 8]
    elif d in ("bc4", "bc5"):
        out = B45.random_words(BC4 if d == "bc4" else BC5, H, W, seed)
    elif d in ("eac_r11", "eac_rg11"):
        out = E11.random_words(EAC_R11 if d == "eac_r11" else EAC_RG11, H, W, seed)
    elif d in EAC16_CODEC:
        out = E16.random_words(EAC16_CODEC[d], H, W, seed)
    elif d == "etc2_rgba8":  # any alpha word, colour words of all five modes
        words = np.frombuffer(E2.random_words(H, W, seed), np.uint8).reshape(-1, 16).copy()
        words[:, 8:] = np.frombuffer(C.random_colour_words(H, W, seed + 1), np.uint8).reshape(-1, 8)
        out = words.tobytes()
    elif d == "etc2_rgb8":
        out = C.random_colour_words(H, W, seed)
    elif d == "etc2_rgb8a1":
        out = A1.random_words(H, W, seed)
    elif d == "bc7":
        out = B7.stratified_blocks(n * rows * cols, seed)
    else:
        assert d in ("bc6h_uf16", "bc6h_sf16")
        out = B6.stratified_blocks(n * rows * cols, seed)
    out = np.frombuffer(bytes(out), np.uint8).reshape(n, -1)
    assert out.shape[1] == rows * cols * DEFINITIONS[d][0]
    out.setflags(write=False)
    return out


def oracle_decode(definition, stream, h, w):
    """The oracle's decode of an h x w image's block stream: (h, w, decoded channels)."""
    d = definition
    if d in ("dxt1", "dxt5", "etc1", "pvrtc2", "pvrtc4"):
        codec = {"dxt1": DXT1, "dxt5": DXT5, "etc1": ETC1, "pvrtc2": PVRTC2, "pvrtc4": PVRTC4}[d]
        out = T.oracle_decode(codec, bytes(stream), h, w)
        assert out is not None
    elif d in ("bc4", "bc5"):
        out = B45.oracle_decode(BC4 if d == "bc4" else BC5, stream, h, w)
    elif d in ("eac_r11", "eac_rg11"):
        out = E11.oracle_decode(EAC_R11 if d == "eac_r11" else EAC_RG11, stream, h, w)
    elif d in EAC16_CODEC:
        out = E16.oracle_decode(EAC16_CODEC[d], stream, h, w)
    elif d == "etc2_rgba8":
        out = C.oracle_decode_rgba8(stream, h, w)
    elif d == "etc2_rgb8":
        out = C.oracle_decode(stream, h, w)
    elif d == "etc2_rgb8a1":
        out = A1.oracle_decode(stream, h, w)
    elif d == "bc7":
        out = B7.decode(stream, h, w)
    else:
        out = B6.decode(stream, h, w, d == "bc6h_sf16")
    return np.asarray(out).reshape(h, w, DEFINITIONS[d][1])


@functools.lru_cache(maxsize=None)
def decoded(definition, rows, cols, n):
    """(n, h, w, decoded channels): what the oracle decodes the blocks of every image to (read-only: shared).  A block decodes
    by itself, so the n streams are decoded as one grid of n * rows block rows and every image is clipped out of its own rows;
    PVRTC blocks read their neighbours, so those images are decoded one by one.  The CPU tier holds a few images of every
    definition to the oracle's call on the image alone."""
    b = blocks(definition, rows, cols, n)
    if definition in ("pvrtc2", "pvrtc4"):
        out = np.stack([oracle_decode(definition, b[i].tobytes(), 4 * rows, 4 * rows) for i in range(n)])
    else:
        tall = oracle_decode(definition, b.tobytes(), 4 * rows * n, 4 * cols)
        out = np.ascontiguousarray(tall.reshape(n, 4 * rows, 4 * cols, -1)[:, :4 * rows - 1, :4 * cols - 2])
    out.setflags(write=False)
    return out


def stats(src, dec, definition, k):
    """(sse [..., 4], max_abs [..., 4]) int64 over the two axes before the last: the first k channels of the source against the
    first k decoded ones, the BC6H definitions through the oracle's texel target."""
    s, d = src[..., :k].astype(np.int64), dec[..., :k].astype(np.int64)
    if definition in ("bc6h_uf16", "bc6h_sf16"):
        signed = definition == "bc6h_sf16"
        s, d = B6.target(s, signed), B6.target(d, signed)
    diff = s - d
    sse = np.zeros(diff.shape[:-3] + (4,), np.int64)
    mx = np.zeros_like(sse)
    sse[..., :k] = (diff * diff).sum(axis=(-3, -2))
    mx[..., :k] = np.abs(diff).max(axis=(-3, -2))
    return sse, mx


def want_metric(F, regime):
    """(sse [n, 4], max_abs [n, 4]) int64: the definition's record of every image."""
    return stats(source(F, regime), decoded(F.definition, regime.rows, regime.cols, regime.n), F.definition, compared_channels(F))


def want_metric_as_the_oracle_measures(F, regime, i):
    """Image i's record through the oracle module's own call on that image alone: what holds the sharing above to the calling
    conventions of the per-family tests (CPU tier)."""
    L = layout(F, regime)
    src = source(F, regime)[i]
    stream = blocks(F.definition, regime.rows, regime.cols, regime.n)[i].tobytes()
    if F.definition in ("dxt1", "dxt5", "etc1", "bc4", "bc5", "pvrtc2", "pvrtc4"):
        sse, mx = M.measure(F.codec, src, stream, L.h, L.w, F.comps)
    elif F.definition in ("bc6h_uf16", "bc6h_sf16"):
        sse, mx = (np.concatenate([np.asarray(v, np.int64), [0]]) for v in B6.metric(src, stream, F.definition == "bc6h_sf16"))
    else:
        sse, mx = stats(src, oracle_decode(F.definition, stream, L.h, L.w), F.definition, compared_channels(F))
    return np.asarray(sse, np.int64), np.asarray(mx, np.int64)


def want_rows(F, regime):
    """(n, h, w * pixel bytes) uint8: the rows a decoder writes."""
    dec = decoded(F.definition, regime.rows, regime.cols, regime.n)
    return np.ascontiguousarray(dec).reshape(dec.shape[0], dec.shape[1], -1).view(np.uint8)


# ---- buffers as they lie in memory

PIXEL_FILL, BLOCK_FILL, CANARY, TAIL = 0x5A, 0xC3, 0xA5, 16


def source_buffer(F, regime):
    """uint8: every image's rows at the layout's strides behind the lead, 0x5A elsewhere."""
    L = layout(F, regime)
    rows = source(F, regime).reshape(L.n, L.h, -1).view(np.uint8)
    buf = np.full(L.pixel_lead + (L.n - 1) * L.pixel_image_stride + L.h * L.stride, PIXEL_FILL, np.uint8)
    for i in range(L.n):
        at = L.pixel_lead + i * L.pixel_image_stride
        buf[at:at + L.h * L.stride].reshape(L.h, L.stride)[:, :rows.shape[2]] = rows[i]
    return buf


def blocks_buffer(F, regime):
    """uint8: every image's stored grid behind the lead: its own blocks in the grid's first rows and columns, arbitrary bytes in
    the blocks outside the image and between the images."""
    L = layout(F, regime)
    bb = block_bytes(F)
    own = blocks(F.definition, regime.rows, regime.cols, regime.n)
    g = np.random.Generator(np.random.PCG64(_seed(regime.rows, regime.cols, regime.n, 99)))
    buf = g.integers(0, 256, L.blocks_lead + L.n * L.blocks_image_stride, dtype=np.uint8) if regime.padded else \
        np.full(L.n * L.blocks_image_stride, BLOCK_FILL, np.uint8)
    grid_rows, grid_cols = (regime.rows, regime.cols) if is_pvrtc(F) else ((L.gh + 3) // 4, (L.gw + 3) // 4)
    for i in range(L.n):
        at = L.blocks_lead + i * L.blocks_image_stride
        grid = buf[at:at + grid_rows * grid_cols * bb].reshape(grid_rows, grid_cols, bb)
        grid[:regime.rows, :regime.cols] = own[i].reshape(regime.rows, regime.cols, bb)
    return buf


def decode_output(F, regime):
    """(canary-filled uint8 buffer for the decoder to write into, what it must hold afterwards): the lead, every image's rows
    at the layout's strides, sixteen bytes after the last image."""
    L = layout(F, regime)
    rows = want_rows(F, regime)
    size = L.pixel_lead + (L.n - 1) * L.pixel_image_stride + L.h * L.stride + TAIL
    want = np.full(size, CANARY, np.uint8)
    for i in range(L.n):
        at = L.pixel_lead + i * L.pixel_image_stride
        want[at:at + L.h * L.stride].reshape(L.h, L.stride)[:, :rows.shape[2]] = rows[i]
    return np.full(size, CANARY, np.uint8), want


def image_of_byte(F, regime, offset):
    """The image whose span (rows, padding and the slack after it) holds byte `offset` of the decoder's buffer."""
    L = layout(F, regime)
    return min(max(offset - L.pixel_lead, 0) // L.pixel_image_stride, L.n - 1)


def measure(pkg, F, regime, src, blk, out):
    """The family's device metric on device buffers (torch.uint8, the leads already skipped)."""
    L = layout(F, regime)
    kw = dict(grid_height=L.gh, grid_width=L.gw, row_stride_bytes=L.stride, n_images=L.n, src_image_stride_bytes=L.pixel_image_stride,
              blocks_image_stride_bytes=L.blocks_image_stride, out=out)
    return getattr(pkg, F.entry)(F.codec, src, blk, L.h, L.w, F.comps, **kw)


def decode_call(pkg, F, h, w, padding, n, blocks_image_stride, pixel_image_stride, blk, out):
    """The family's C ABI decoder on device buffers the caller owns (torch.uint8); returns the status."""
    if F.entry == "icamd_decode_bc6h_device":
        return pkg.lib().icamd_decode_bc6h_device(F.codec, h, w, padding, n, blocks_image_stride, pixel_image_stride,
                                                  blk.data_ptr(), out.data_ptr(), None)
    assert F.entry == "icamd_decode_device"
    return pkg.lib().icamd_decode_device(F.codec, 0, h, w, padding, n, blocks_image_stride, pixel_image_stride, blk.data_ptr(),
                                         out.data_ptr(), None)


def decode(pkg, F, regime, blk, out):
    """decode_call at the regime's layout (the leads already skipped)."""
    L = layout(F, regime)
    return decode_call(pkg, F, L.h, L.w, L.stride - L.w * F.pixel_bytes, L.n, L.blocks_image_stride, L.pixel_image_stride, blk, out)


# ---- the walk restated: which image each lane holds

def walk(B, n, per_workgroup):
    """The image index of every lane: int64 [workgroups, per_workgroup // 256, 4 waves, 64 lanes] and the mask of the lanes that
    hold a block.  Lane t of quarter j of workgroup g holds block k = g * per_workgroup + 256 * j + t; a lane without a block
    carries img_last, the image of the workgroup's last block."""
    total = B * n
    groups = -(-total // per_workgroup)
    k = np.arange(groups * per_workgroup, dtype=np.int64).reshape(groups, per_workgroup // 256, 4, 64)
    have = k < total
    last = np.minimum((np.arange(groups, dtype=np.int64) + 1) * per_workgroup, total) - 1
    img = np.where(have, k // B, (last // B)[:, None, None, None])
    return img, have


def classify(B, n, per_workgroup=METRIC_BLOCKS_PER_WORKGROUP):
    """What the three-way decision of the metric walk does for n images of B blocks, as counts."""
    img, have = walk(B, n, per_workgroup)
    groups = img.shape[0]
    first = np.arange(groups, dtype=np.int64) * per_workgroup // B
    img_last = (np.minimum((np.arange(groups, dtype=np.int64) + 1) * per_workgroup, B * n) - 1) // B
    one_image = first == img_last
    waves = img.reshape(groups, -1, 64)
    wave_have = have.reshape(groups, -1, 64)
    agree = (waves == waves[:, :, :1]).all(axis=2)
    spanning = ~one_image[:, None] & np.ones(agree.shape, bool)  # the waves that go through the per-wave flush
    images_in_wave = np.array([[len(set(w.tolist())) for w in g] for g in waves])
    flat, flat_have = waves.reshape(-1, 64), wave_have.reshape(-1, 64)
    last_wave = int(np.flatnonzero(flat_have.any(axis=1))[-1])  # (images among its blocks, lanes without a block)
    return dict(
        workgroups=groups,
        one_image_workgroups=[int(i) for i in np.flatnonzero(one_image)],
        one_image_workgroup_images=[int(first[i]) for i in np.flatnonzero(one_image)],
        blocks_in_last_workgroup=int(have[-1].sum()),
        quarters_without_a_block_in_last_workgroup=int((~have[-1].any(axis=(1, 2))).sum()),
        waves_that_agree=int((spanning & agree).sum()),
        waves_that_agree_on_another_image_than_img_last=int((spanning & agree & (waves[:, :, 0] != img_last[:, None])).sum()),
        waves_that_disagree=int((spanning & ~agree).sum()),
        waves_that_disagree_by_workgroup=[int(v) for v in (spanning & ~agree).sum(axis=1)],
        empty_waves=int((spanning & ~wave_have.any(axis=2)).sum()),
        waves_with_blocks=int(wave_have.any(axis=2).sum()),
        most_images_in_a_wave=int(images_in_wave.max()),
        last_wave_with_blocks=(len(set(flat[last_wave][flat_have[last_wave]].tolist())), int((~flat_have[last_wave]).sum())),
    )


# ---- more than 2^31 - 1 blocks in one call: overlapping images on a strip
# One strip of STRIP_W pixels and STRIP_IMAGES + STRIP_ROWS - 1 block rows; image i is the STRIP_ROWS block rows from block row i
# on, its last block row clipped to 3 pixel rows: the images are one block row apart.  The content repeats every STRIP_PERIOD
# block rows.  decode_plan.h puts (2^31 - 1) // 64 512 = 33 288 images into the first launch; 33 288 % 5 = 3, so a second launch
# whose pixel, block or record offset is taken from image 0 reads or writes the wrong rows of the period.
STRIP_W, STRIP_ROWS, STRIP_IMAGES, STRIP_PERIOD = 250, 1024, 33291, 5
STRIP_COLS = (STRIP_W + 3) // 4
STRIP_H = 4 * STRIP_ROWS - 1
STRIP_BLOCKS_PER_IMAGE = STRIP_ROWS * STRIP_COLS
STRIP_FIRST_LAUNCH_IMAGES = ((1 << 31) - 1) // STRIP_BLOCKS_PER_IMAGE
STRIP_BLOCK_ROWS = STRIP_IMAGES + STRIP_ROWS - 1
STRIP_ROW_PADDING = 6
STRIP_METRICS = ["metric_dxt1_rgba8", "metric_eac16_r11_r16", "metric_bc6h_uf16_rgb16f"]  # one family per launcher
STRIP_DECODERS = ["decode_dxt1", "decode_bc7", "decode_bc6h_uf16"]
_STRIP_REGIME = Regime("strip_period", STRIP_PERIOD, STRIP_COLS, 1, False)


def strip_period_source(F):
    """(4 * STRIP_PERIOD, STRIP_W, comps): the source pixels of one period (the shared image's columns beyond STRIP_W unused)."""
    assert 4 * STRIP_COLS - 2 == STRIP_W
    full = pixels(DEFINITIONS[F.definition][3], STRIP_PERIOD + 1, STRIP_COLS, 1)[0]  # (one block row more: 4 * PERIOD rows)
    return np.ascontiguousarray(full[:4 * STRIP_PERIOD, :, :F.comps])


def strip_period_blocks(F):
    """(STRIP_PERIOD, STRIP_COLS * block bytes) uint8: the blocks of one period, a block row per row."""
    return blocks(F.definition, STRIP_PERIOD, STRIP_COLS, 1).reshape(STRIP_PERIOD, -1)


def strip_source_stride(F):
    return STRIP_W * F.comps * F.sample_bytes + STRIP_ROW_PADDING


def strip_period_source_rows(F):
    """(4 * STRIP_PERIOD, row stride) uint8: the period's source rows as they lie in memory, the padding 0x5A."""
    src = strip_period_source(F)
    rows = np.full((src.shape[0], strip_source_stride(F)), PIXEL_FILL, np.uint8)
    rows[:, :STRIP_W * F.comps * F.sample_bytes] = src.reshape(src.shape[0], -1).view(np.uint8)
    return rows


def strip_block_row_records(F):
    """(full, clipped): each (sse [PERIOD, 4], max_abs [PERIOD, 4]) -- the oracle's record of every block row of the period as
    an image of its own, 4 pixel rows high and 3."""
    src, blk = strip_period_source(F), strip_period_blocks(F)
    out = []
    for rows in (4, 3):
        recs = [stats(src[4 * p:4 * p + rows], oracle_decode(F.definition, blk[p].tobytes(), rows, STRIP_W), F.definition,
                      compared_channels(F)) for p in range(STRIP_PERIOD)]
        out.append((np.stack([r[0] for r in recs]), np.stack([r[1] for r in recs])))
    return out


def strip_record(F, i, records=None):
    """Image i's record from the block-row records: the sum (max_abs: the maximum) over strip rows i .. i + STRIP_ROWS - 1, the
    last of them clipped.  It depends on i % STRIP_PERIOD alone."""
    (full_sse, full_mx), (clip_sse, clip_mx) = records or strip_block_row_records(F)
    inner = (i + np.arange(STRIP_ROWS - 1)) % STRIP_PERIOD
    last = (i + STRIP_ROWS - 1) % STRIP_PERIOD
    return full_sse[inner].sum(axis=0) + clip_sse[last], np.maximum(full_mx[inner].max(axis=0), clip_mx[last])


def strip_record_table(F):
    """(STRIP_PERIOD, 48) uint8: the icamd_error_stats record of image i at row i % STRIP_PERIOD."""
    records = strip_block_row_records(F)
    table = np.zeros((STRIP_PERIOD, 48), np.uint8)
    for r in range(STRIP_PERIOD):
        sse, mx = strip_record(F, r, records)
        table[r, :32] = sse.astype("<u8").view(np.uint8)
        table[r, 32:] = mx.astype("<u4").view(np.uint8)
    return table


def strip_image_as_the_oracle_measures(F, i):
    """Image i of the strip measured whole: its STRIP_ROWS block rows laid out as one image, through the oracle's decode."""
    which = (i + np.arange(STRIP_ROWS)) % STRIP_PERIOD
    src = strip_period_source(F).reshape(STRIP_PERIOD, 4, STRIP_W, -1)[which].reshape(4 * STRIP_ROWS, STRIP_W, -1)[:STRIP_H]
    stream = strip_period_blocks(F)[which].tobytes()
    return stats(src, oracle_decode(F.definition, stream, STRIP_H, STRIP_W), F.definition, compared_channels(F))


def strip_decoded_stride(F):
    return STRIP_W * F.pixel_bytes + STRIP_ROW_PADDING


def strip_period_decoded_rows(F):
    """(4 * STRIP_PERIOD, decoded row stride) uint8: the oracle's decode of one period, the padding the canary."""
    dec = oracle_decode(F.definition, strip_period_blocks(F).tobytes(), 4 * STRIP_PERIOD, STRIP_W)
    rows = np.full((4 * STRIP_PERIOD, strip_decoded_stride(F)), CANARY, np.uint8)
    rows[:, :STRIP_W * F.pixel_bytes] = np.ascontiguousarray(dec).reshape(4 * STRIP_PERIOD, -1).view(np.uint8)
    return rows


# ---- the divisors fastdiv sees in these launches (tests/wrapper_cases.py probes fastdiv at them)

def fastdiv_grids():
    """block_cols, blocks per image and blocks per launch of every regime, both PVRTC pitches among them, and of the strip."""
    d = {STRIP_COLS, STRIP_BLOCKS_PER_IMAGE, STRIP_FIRST_LAUNCH_IMAGES * STRIP_BLOCKS_PER_IMAGE,
         (STRIP_IMAGES - STRIP_FIRST_LAUNCH_IMAGES) * STRIP_BLOCKS_PER_IMAGE}
    for F in (BY_NAME["metric_dxt1_rgba8"], BY_NAME["decode_dxt1"], BY_NAME["metric_pvrtc2_rgba8"], BY_NAME["metric_pvrtc4_rgba8"]):
        for r in regimes(F):
            d |= {r.cols, r.rows * r.cols, r.rows * r.cols * r.n}
    return d
