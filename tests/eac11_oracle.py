"""EAC R11 / RG11 (include/ic_amd.h, ICAMD_EAC_R11) as DEFINED in DESIGN.md 3.14, restated in numpy:

* R11 of channel c = the EAC word that the ETC2 RGBA8 definition (tests/etc2_oracle.py: eac_encode on block_alphas) writes for
  the image whose alpha is channel c -- same grid, same clamp-to-edge replication; RG11 = R11(R) then R11(G) per block;
* source channels by the BC4 / BC5 rules: R = byte 0 (byte 2 with swap_rb and 3 or 4 components), G = byte 1;
* decode (Khronos EAC, 11-bit): v11 = clamp(8 base + 4 + M[table][index] * (1 if multiplier == 0 else 8 multiplier), 0, 2047),
  the byte is v11 >> 3.

Shared by tests/test_eac11_host.py (CPU tier), tests/test_gpu_eac11.py (GPU tier) and scripts/bench_eac11.py."""
import numpy as np

from etc2_oracle import M, block_alphas, eac_encode

EAC_R11, EAC_RG11 = 19, 20
# (codec, src_components, swap_rb) of every source layout the C ABI accepts
LAYOUTS = [(EAC_R11, 1, 0), (EAC_R11, 2, 0), (EAC_R11, 3, 0), (EAC_R11, 3, 1), (EAC_R11, 4, 0), (EAC_R11, 4, 1),
           (EAC_RG11, 2, 0), (EAC_RG11, 3, 0), (EAC_RG11, 3, 1), (EAC_RG11, 4, 0), (EAC_RG11, 4, 1)]


def comps_out(codec):
    return 2 if codec == EAC_RG11 else 1


def block_bytes(codec):
    return 16 if codec == EAC_RG11 else 8


def encoded_size(codec, gh, gw):
    return ((gh + 3) // 4) * ((gw + 3) // 4) * block_bytes(codec)


def channel_words(chan, h, w, gh=None, gw=None):
    """[n_blocks, 8] EAC words of the h x w plane `chan` on the grid max(h, gh) x max(w, gw)."""
    gh = h if gh is None else max(gh, h)
    gw = w if gw is None else max(gw, w)
    return eac_encode(block_alphas(chan, h, w, gh, gw))


def oracle_encode(codec, img, h, w, comps, swap=0, gh=None, gw=None):
    """Expected bytes of one image (h, w, comps)."""
    img = np.asarray(img, np.uint8).reshape(h, w, comps)
    rch = 2 if (swap and comps >= 3) else 0
    r = channel_words(img[..., rch], h, w, gh, gw)
    if codec == EAC_R11:
        return r.tobytes()
    return np.concatenate([r, channel_words(img[..., 1], h, w, gh, gw)], axis=1).tobytes()


def eac11_decode_v11(words):
    """[n, 8] uint8 EAC words -> [n, 16] 11-bit values, texel i = 4 x + y."""
    v = np.ascontiguousarray(words, np.uint8).reshape(-1, 8).view(">u8").reshape(-1).astype(np.uint64)
    b = (v >> np.uint64(56)).astype(np.int64)
    m = ((v >> np.uint64(52)) & np.uint64(15)).astype(np.int64)
    t = ((v >> np.uint64(48)) & np.uint64(15)).astype(np.int64)
    scale = np.where(m == 0, 1, 8 * m)
    out = np.empty((v.size, 16), np.int64)
    for i in range(16):
        idx = ((v >> np.uint64(45 - 3 * i)) & np.uint64(7)).astype(np.int64)
        out[:, i] = np.clip(8 * b + 4 + M[t, idx] * scale, 0, 2047)
    return out


def eac11_decode(words):
    """[n, 8] uint8 EAC words -> [n, 16] bytes (v11 >> 3), texel i = 4 x + y."""
    return eac11_decode_v11(words) >> 3


def _plane(words, h, w):
    rows, cols = (h + 3) // 4, (w + 3) // 4
    a = eac11_decode(words).reshape(rows, cols, 4, 4)  # [brow, bcol, x, y]
    return a.transpose(0, 3, 1, 2).reshape(rows * 4, cols * 4)[:h, :w]


def oracle_decode(codec, blocks, h, w, pad=0):
    """Expected R8 / RG8 rows (h rows of w * comps + pad bytes, the pad bytes zero)."""
    b = np.frombuffer(bytes(blocks), np.uint8).reshape(-1, block_bytes(codec))
    chans = [_plane(b[:, :8], h, w)]
    if codec == EAC_RG11:
        chans.append(_plane(b[:, 8:], h, w))
    n = len(chans)
    out = np.zeros((h, w * n + pad), np.uint8)
    out[:, :w * n] = np.stack(chans, axis=-1).reshape(h, w * n)
    return out.reshape(-1)


def random_words(codec, h, w, seed):
    """Arbitrary words for an h x w image: every fourth word gets multiplier 0, the next one base 0 or 255 with a large
    multiplier (as etc2_oracle.random_words does for the alpha half)."""
    g = np.random.Generator(np.random.PCG64(seed))
    n = ((h + 3) // 4) * ((w + 3) // 4) * block_bytes(codec) // 8
    al = g.integers(0, 256, size=(n, 8), dtype=np.uint8)
    al[::4, 1] &= 0x0f
    al[1::4, 0] = np.where(g.integers(0, 2, size=al[1::4, 0].shape) == 1, 255, 0)
    al[1::4, 1] |= 0xc0
    return al.tobytes()
