"""16-bit and signed EAC R11 / RG11 (include/ic_amd.h, icamd_encode_eac11_16_device) as DEFINED there and in DESIGN.md 3.20,
restated in numpy:

* decode to 16 bits (Khronos EAC), s = 1 if multiplier == 0 else 8 multiplier:
    unsigned  v = clamp(8 base + 4 + M[table][index] s, 0, 2047),  out16 = v << 5 | v >> 6;
    signed    b = int8(byte 0), -128 read as -127;  v = clamp(8 b + M[table][index] s, -1023, 1023),
              out16 = sign(v) ((|v| << 5) + (|v| >> 5));
* encode from 16-bit samples in the 11-bit domain: the 192-candidate search of the header, first smallest sse, smallest index at
  each texel's minimum; grids and clamp-to-edge replication as for the 8-bit codecs (etc2_oracle.block_alphas).

Shared by tests/test_eac11_16_host.py (CPU tier), tests/test_gpu_eac11_16.py (GPU tier) and scripts/bench_eac11_16.py."""
import numpy as np

from etc2_oracle import M, SPAN, block_alphas

EAC_R11, EAC_RG11, EAC_SIGNED_R11, EAC_SIGNED_RG11 = 19, 20, 24, 25
CODECS = (EAC_R11, EAC_RG11, EAC_SIGNED_R11, EAC_SIGNED_RG11)
# (codec, src_channels) of every source layout the C ABI accepts
LAYOUTS = [(c, n) for c in CODECS for n in range(2 if c in (EAC_RG11, EAC_SIGNED_RG11) else 1, 5)]


def is_signed(codec):
    return codec in (EAC_SIGNED_R11, EAC_SIGNED_RG11)


def comps_out(codec):
    return 2 if codec in (EAC_RG11, EAC_SIGNED_RG11) else 1


def block_bytes(codec):
    return 8 * comps_out(codec)


def sample_dtype(codec):
    return np.int16 if is_signed(codec) else np.uint16


def encoded_size(codec, gh, gw):
    return ((gh + 3) // 4) * ((gw + 3) // 4) * block_bytes(codec)


def targets(samples, signed):
    """16-bit samples -> their 11-bit targets (int64)."""
    s = np.asarray(samples).astype(np.int64)
    if not signed:
        return s >> 5
    x = np.maximum(s, -32767)
    return np.sign(x) * (np.abs(x) >> 5)


def search(a, signed):
    """[n, 16] targets (texel i = 4 x + y) -> ([n, 8] uint8 words, [n] sse in the 11-bit domain)."""
    a = np.asarray(a, np.int64)
    n = a.shape[0]
    lo, hi = a.min(axis=1), a.max(axis=1)
    R = hi - lo
    vmin, vmax = (-1023, 1023) if signed else (0, 2047)
    bmin, bmax = (-127, 127) if signed else (0, 255)
    best_sse = np.full(n, np.iinfo(np.int64).max, np.int64)
    best_idx = np.zeros((n, 16), np.int64)
    best_t, best_m, best_b = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    for t in range(16):
        span = int(SPAN[t])
        m0 = (2 * R + 8 * span) // (16 * span)
        for m in (np.zeros(n, np.int64), np.clip(m0 - 1, 1, 15), np.clip(m0, 1, 15), np.clip(m0 + 1, 1, 15)):
            s = np.where(m == 0, 1, 8 * m)
            c2 = lo + hi + s
            b0 = (c2 + 8) >> 4 if signed else c2 >> 4
            for db in (-1, 0, 1):
                b = np.clip(b0 + db, bmin, bmax)
                B = 8 * b if signed else 8 * b + 4
                vals = np.clip(B[:, None] + M[t][None, :] * s[:, None], vmin, vmax)   # [n, 8]
                err = np.abs(vals[:, None, :] - a[:, :, None])                        # [n, 16, 8]
                idx = err.argmin(axis=2)                                              # first (smallest) index of the minimum
                e = err.min(axis=2)
                sse = (e * e).sum(axis=1)
                better = sse < best_sse                                               # strictly: the first candidate stays
                best_sse = np.where(better, sse, best_sse)
                best_idx[better] = idx[better]
                best_t[better], best_m[better], best_b[better] = t, m[better], b[better]
    v = ((best_b & 255).astype(np.uint64) << np.uint64(56)) | (best_m.astype(np.uint64) << np.uint64(52)) | \
        (best_t.astype(np.uint64) << np.uint64(48))
    for i in range(16):
        v |= best_idx[:, i].astype(np.uint64) << np.uint64(45 - 3 * i)
    return v.astype(">u8").view(np.uint8).reshape(n, 8), best_sse


def channel_words(plane, h, w, signed, gh=None, gw=None):
    """[n_blocks, 8] words of the h x w plane of 16-bit samples on the grid max(h, gh) x max(w, gw)."""
    gh = h if gh is None else max(gh, h)
    gw = w if gw is None else max(gw, w)
    return search(block_alphas(targets(np.asarray(plane).reshape(h, w), signed), h, w, gh, gw), signed)[0]


def oracle_encode(codec, img, h, w, chans, gh=None, gw=None):
    """Expected bytes of one image (h, w, chans) of uint16 / int16 samples."""
    img = np.asarray(img).reshape(h, w, chans)
    r = channel_words(img[..., 0], h, w, is_signed(codec), gh, gw)
    if comps_out(codec) == 1:
        return r.tobytes()
    return np.concatenate([r, channel_words(img[..., 1], h, w, is_signed(codec), gh, gw)], axis=1).tobytes()


def decode_v11(words, signed):
    """[n, 8] uint8 words -> [n, 16] 11-bit values (signed: -1023 .. 1023), texel i = 4 x + y."""
    v = np.ascontiguousarray(words, np.uint8).reshape(-1, 8).view(">u8").reshape(-1).astype(np.uint64)
    b = (v >> np.uint64(56)).astype(np.int64)
    m = ((v >> np.uint64(52)) & np.uint64(15)).astype(np.int64)
    t = ((v >> np.uint64(48)) & np.uint64(15)).astype(np.int64)
    s = np.where(m == 0, 1, 8 * m)
    if signed:
        b = np.maximum(np.where(b >= 128, b - 256, b), -127)
    out = np.empty((v.size, 16), np.int64)
    for i in range(16):
        idx = ((v >> np.uint64(45 - 3 * i)) & np.uint64(7)).astype(np.int64)
        out[:, i] = np.clip(8 * b + M[t, idx] * s, -1023, 1023) if signed else np.clip(8 * b + 4 + M[t, idx] * s, 0, 2047)
    return out


def decode16(words, signed):
    """[n, 8] uint8 words -> [n, 16] 16-bit values (int64), texel i = 4 x + y."""
    v = decode_v11(words, signed)
    if signed:
        return np.sign(v) * ((np.abs(v) << 5) + (np.abs(v) >> 5))
    return (v << 5) | (v >> 6)


def _plane(words, h, w, signed):
    rows, cols = (h + 3) // 4, (w + 3) // 4
    a = decode16(words, signed).reshape(rows, cols, 4, 4)  # [brow, bcol, x, y]
    return a.transpose(0, 3, 1, 2).reshape(rows * 4, cols * 4)[:h, :w]


def oracle_decode(codec, blocks, h, w, pad=0):
    """Expected rows: (h, w * comps + pad // 2) uint16 / int16 samples, the padding samples zero.  pad: even bytes."""
    assert pad % 2 == 0
    b = np.frombuffer(bytes(blocks), np.uint8).reshape(-1, block_bytes(codec))
    k = comps_out(codec)
    chans = [_plane(b[:, 8 * c:8 * c + 8], h, w, is_signed(codec)) for c in range(k)]
    out = np.zeros((h, w * k + pad // 2), sample_dtype(codec))
    out[:, :w * k] = np.stack(chans, axis=-1).reshape(h, w * k)
    return out


def random_words(codec, h, w, seed):
    """Arbitrary words for an h x w image.  Of every four words: one with multiplier 0, one with base 0x00 or 0xff and a large
    multiplier (clamps at either end, unsigned), one with base 0x80 or 0x7f and a large multiplier (signed: -128 and the
    clamps at either end), one arbitrary."""
    g = np.random.Generator(np.random.PCG64(seed))
    n = ((h + 3) // 4) * ((w + 3) // 4) * block_bytes(codec) // 8
    al = g.integers(0, 256, size=(n, 8), dtype=np.uint8)
    al[::4, 1] &= 0x0f
    al[1::4, 0] = np.where(g.integers(0, 2, size=al[1::4, 0].shape) == 1, 255, 0)
    al[1::4, 1] |= 0xc0
    al[2::4, 0] = np.where(g.integers(0, 2, size=al[2::4, 0].shape) == 1, 0x80, 0x7f)
    al[2::4, 1] |= 0xc0
    return al.tobytes()


def image(codec, h, w, chans, seed):
    """A test image of 16-bit samples, (h, w, chans): smooth blocks, noisy blocks, flat blocks and the extremes of the range
    (-32768 for the signed codecs), mixed block by block."""
    g = np.random.Generator(np.random.PCG64(7000 + seed))
    lo, hi = (-32768, 32767) if is_signed(codec) else (0, 65535)
    y, x = np.mgrid[0:h, 0:w]
    out = np.empty((h, w, chans), np.int64)
    for c in range(chans):
        smooth = (lo + hi) // 2 + (g.integers(-9000, 9000) + 37 * x * (c + 1) + 11 * y + g.integers(-60, 61, (h, w)))
        noise = g.integers(lo, hi + 1, (h, w))
        flat = np.broadcast_to(g.integers(lo, hi + 1, ((h + 3) // 4, (w + 3) // 4)).repeat(4, 0).repeat(4, 1)[:h, :w], (h, w))
        ends = np.where(g.integers(0, 2, (h, w)) == 1, hi, lo)
        kind = g.integers(0, 5, ((h + 3) // 4, (w + 3) // 4)).repeat(4, 0).repeat(4, 1)[:h, :w]
        near = np.clip(flat + g.integers(-300, 301, (h, w)), lo, hi)
        out[..., c] = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [smooth, noise, flat, ends], near)
    return np.clip(out, lo, hi).astype(sample_dtype(codec))


def with_row_padding(img, pad_bytes):
    """(h, w, c) 16-bit samples -> flat bytes of rows followed by pad_bytes (even) bytes of 0xa5 each."""
    h = img.shape[0]
    rows = np.ascontiguousarray(img).reshape(h, -1).view(np.uint8)
    return np.concatenate([rows, np.full((h, pad_bytes), 0xa5, np.uint8)], axis=1).reshape(-1)


# ---- the quality fixtures of DESIGN.md 3.20 (64 x 64 uint16)

def ramp():
    y, x = np.mgrid[0:64, 0:64]
    return (20000 + 37 * x + 11 * y).astype(np.uint16)


def hills():
    y, x = np.mgrid[0:64, 0:64]
    g = np.random.Generator(np.random.PCG64(20260))
    return (32768 + np.round(9000 * np.sin(x / 9.0) * np.cos(y / 13.0)).astype(np.int64) + g.integers(-40, 41, (64, 64))).astype(np.uint16)


def sse16(plane, words, signed=False):
    """Summed squared error, in the 16-bit domain, of the words of an h x w plane (h, w multiples of 4 here or not)."""
    h, w = plane.shape
    d = _plane(words, h, w, signed) - np.asarray(plane).astype(np.int64)
    return int((d * d).sum())


def existing_route_words(plane):
    """The route a 16-bit source had to take before: source >> 8, the 8-bit EAC R11 search (tests/eac11_oracle.py)."""
    import eac11_oracle as A
    h, w = plane.shape
    return A.channel_words((np.asarray(plane, np.uint16) >> 8).astype(np.uint8), h, w)
