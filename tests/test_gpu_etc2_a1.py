"""GPU tier for ICAMD_ETC2_RGB8A1, ETC2 RGB8 with punch-through alpha (include/ic_amd.h): the HIP kernels through
the C ABI and the Python wrappers, every case bit-exact against the numpy statement (tests/etc2_a1_oracle.py)."""
import ctypes
import functools
import importlib

import numpy as np
import pytest

import etc2_a1_oracle as A
import ic_testlib as T

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("image-compression_amd")
A1 = A.ETC2_RGB8A1
# 4 x 4, an odd size, one full workgroup (16 x 16 blocks), partial tiles both ways over several workgroups
SHAPES = [(4, 4), (5, 3), (64, 64), (68, 132)]
PADDED = [(30, 30, 40, 48), (5, 3, 16, 16), (1, 1, 9, 13), (64, 61, 64, 64)]
MASKS = ("none", "blobs", "noise")


@pytest.fixture(scope="module")
def dev():
    import torch
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


def _to_dev(buf, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.frombuffer(bytes(buf), np.uint8)).copy()).to(dev)


def _encode(flat, h, w, dev, **kw):
    import torch
    out = pkg.encode_device(A1, _to_dev(flat, dev), h, w, 4, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _decode(words, h, w, dev, **kw):
    import torch
    out = pkg.decode_device(A1, _to_dev(words, dev), h, w, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _image(mask, h, w):
    return A.masked_image("mixed", mask, h, w, index=h + w)


@functools.lru_cache(maxsize=None)
def _want(mask, h, w, gh, gw, strategy):
    return A.oracle_encode(_image(mask, h, w), h, w, 0, strategy, gh=gh, gw=gw)


def _stats(img, dec):
    d = img.astype(np.int64) - dec.astype(np.int64)
    return (d * d).sum(axis=(0, 1)), np.abs(d).max(axis=(0, 1))


# ---- encode

@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("h,w", SHAPES)
def test_encode_every_strategy(dev, h, w, mask):
    img = _image(mask, h, w)
    for strategy in A.STRATEGIES:
        got = _encode(img.tobytes(), h, w, dev, etc_strategy=strategy)
        assert got.tobytes() == _want(mask, h, w, h, w, strategy), (mask, h, w, strategy)


@pytest.mark.parametrize("h,w,gh,gw", PADDED)
def test_encode_padded_grid_every_strategy_and_swap(dev, h, w, gh, gw):
    for mask in ("blobs", "noise"):
        img = _image(mask, h, w)
        for strategy in A.STRATEGIES:
            for swap in (0, 1):  # (bytes 0..2 as they lie in memory, whatever swap_rb)
                got = _encode(img.tobytes(), h, w, dev, etc_strategy=strategy, swap_rb=bool(swap), grid_height=gh, grid_width=gw)
                assert got.tobytes() == _want(mask, h, w, gh, gw, strategy), (mask, h, w, gh, gw, strategy, swap)


def test_encode_batch_with_row_padding_and_image_stride(dev):
    import torch
    h, w, n, pad = 37, 70, 3, 3
    stride = w * 4 + pad
    slot = h * stride + 29
    buf = np.zeros(1 + n * slot, np.uint8)
    imgs = [A.masked_image("mixed", MASKS[i], h, w, index=20 + i) for i in range(n)]
    for i, im in enumerate(imgs):
        buf[1 + i * slot:1 + i * slot + h * stride] = T.with_row_padding(im, pad)
    d = _to_dev(buf.tobytes(), dev)
    per = A.encoded_size(h, w)
    out = torch.zeros(1 + n * (per + 8) + 5, dtype=torch.uint8, device=dev)
    st = pkg.lib().icamd_encode_device(A1, 2, 4, 0, h, w, h, w, stride, n, slot, per + 8, ctypes.c_void_p(d.data_ptr() + 1),
                                       ctypes.c_void_p(out.data_ptr() + 1), None)
    assert st == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got[0] == 0 and not got[1 + n * (per + 8):].any()
    for i, im in enumerate(imgs):
        at = 1 + i * (per + 8)
        assert got[at:at + per].tobytes() == A.oracle_encode(im, h, w), i
        assert not got[at + per:at + per + 8].any()  # the slack between images is left alone


@functools.lru_cache(maxsize=None)
def _wave_vote_image():
    """64 x 64, one workgroup of 16 x 16 blocks: lane l of wave v encodes block (row 4 v + l // 16, column l % 16), so pixel
    rows 16 v .. 16 v + 15 are wave v's."""
    g = np.random.Generator(np.random.PCG64(T.SEED0 + 9900))
    y, x = np.mgrid[0:64, 0:64]
    img = np.empty((64, 64, 4), np.uint8)
    img[..., 0], img[..., 1], img[..., 2], img[..., 3] = 40 + x, 70 + y, 90 + (x + y) // 2, 255
    img[16 + 5, 4 * 9 + 2, 3] = 0                                  # wave 1: one lane, one transparent texel
    img[32:48, :, 3] = np.where(g.integers(0, 3, (16, 64)) == 0, 10, 240)
    img[32:36, 8:24, 3] = 0                                        # wave 2: fully transparent blocks among the masked ones
    img[36:40, 40:44, 3] = 127
    img[48:64, :, :3] = g.integers(0, 256, (16, 64, 3), dtype=np.uint8)
    img[48:64:, :, 3] = g.integers(128, 256, (16, 64), dtype=np.uint8)
    img[52:56, 20:24, :3] = img[4:8, 20:24, :3]                    # wave 3: one smooth lane among the noise
    return img


def test_wave_votes(dev):
    img = _wave_vote_image()
    for strategy in A.STRATEGIES:
        want, info = A.oracle_encode(img, 64, 64, 0, strategy, return_classes=True)
        cls = info["class"].reshape(4, 64)  # [wave, lane]
        n_opq = info["opaque"].sum(axis=(1, 2)).reshape(4, 64)
        e = np.frombuffer(T.oracle_encode(T.ETC1, img, 64, 64, 4, 0, strategy), np.uint8).reshape(4, 64, 8)
        differential = (e[..., 3] & 2) != 0
        # conditions on the input, from the statement alone
        assert (n_opq[0] == 16).all() and differential[0].all()
        assert sorted(n_opq[1].tolist()) == [15] + [16] * 63 and differential[1][n_opq[1] == 16].all()
        assert (n_opq[2] < 16).all() and (n_opq[2] == 0).sum() >= 4 and (cls[2] == A.D_MASKED).sum() >= 32
        assert (n_opq[3] == 16).all() and (~differential[3]).sum() >= 40 and differential[3, 16 + 5]
        assert np.isin(cls[3], (A.D_OPAQUE, A.PLANAR_CHOSEN, A.E_KEPT)).all() and (cls[3] == A.D_OPAQUE).sum() >= 32
        got = _encode(img.tobytes(), 64, 64, dev, etc_strategy=strategy)
        assert got.tobytes() == want, strategy


# ---- decode

@pytest.mark.parametrize("swap", [0, 1])
def test_decode_every_mode_and_opaque_bit_in_every_wave(dev, swap):
    h, w = 4, 1024
    words = A.random_words(h, w, seed=2200)
    per_wave = (A.modes(words) * 2 + A.opaque_bit(words)).reshape(-1, 64)
    assert all((np.bincount(row, minlength=10)[2:] == 8).all() for row in per_wave)  # all eight kinds in every wave
    assert _decode(words, h, w, dev, swap_rb=bool(swap)).tobytes() == A.oracle_decode(words, h, w, swap).tobytes()


@pytest.mark.parametrize("mode", [A.DIFFERENTIAL, A.T_MODE, A.H_MODE, A.PLANAR])
def test_decode_constructed_words_with_op_0(dev, mode):
    h, w = 4, 1024
    words = A.random_words(h, w, seed=2210 + mode, only=mode, op=0)
    assert _decode(words, h, w, dev).tobytes() == A.oracle_decode(words, h, w).tobytes()


@pytest.mark.parametrize("h,w", [(5, 3), (61, 59)])
def test_decode_clipped_edges(dev, h, w):
    for swap in (0, 1):
        for pad in (0, 5):
            words = A.random_words(h, w, seed=2220 + h)
            got = _decode(words, h, w, dev, swap_rb=bool(swap), padding_bytes_per_row=pad)
            assert got.tobytes() == A.oracle_decode(words, h, w, swap, pad).tobytes(), (swap, pad)


@pytest.mark.parametrize("h,w", [(5, 3), (61, 59), (64, 64)])
def test_decode_of_encoder_output(dev, h, w):
    for mask in MASKS:
        img = A.masked_image("mixed", mask, h, w, index=h + w)
        blocks = _encode(img.tobytes(), h, w, dev)
        want = A.oracle_decode(A.oracle_encode(img, h, w), h, w)
        assert _decode(blocks.tobytes(), h, w, dev).tobytes() == want.tobytes(), (mask, h, w)
        dec = want.reshape(h, w, 4)
        assert (dec[..., 3] == np.where(img[..., 3] >= 128, 255, 0)).all()  # alpha is the mask


# ---- metric

def test_metric_equals_decode(dev):
    import torch
    cases = [("blobs", 64, 64, 0), ("noise", 61, 59, 3), ("none", 30, 30, 0), ("noise", 5, 3, 0), ("blobs", 1, 1, 0)]
    for mask, h, w, pad in cases:
        img = A.masked_image("mixed", mask, h, w, index=h + w)
        stride = w * 4 + pad
        d_src = _to_dev(T.with_row_padding(img, pad).tobytes(), dev)
        for strategy in A.STRATEGIES:
            blocks = pkg.encode_device(A1, d_src, h, w, 4, etc_strategy=strategy, row_stride_bytes=stride)
            for swap in (0, 1):
                sse, mx = pkg.measure_error_device(A1, d_src, blocks.reshape(-1), h, w, 4, row_stride_bytes=stride, swap_rb=bool(swap))
                torch.cuda.synchronize()
                dec = A.oracle_decode(blocks.cpu().numpy().tobytes(), h, w, swap).reshape(h, w, 4)
                want_sse, want_max = _stats(img, dec)
                assert (sse[0].cpu().numpy() == want_sse).all() and (mx[0].cpu().numpy() == want_max).all(), (mask, h, w, strategy, swap)


def test_metric_of_arbitrary_words_on_a_padded_grid_and_a_batch(dev):
    import torch
    h, w, gh, gw, n = 30, 30, 40, 48, 3
    imgs = np.stack([A.masked_image("mixed", MASKS[i], h, w, index=60 + i) for i in range(n)])
    d = torch.from_numpy(imgs.reshape(-1)).to(dev)
    words = np.stack([np.frombuffer(A.random_words(gh, gw, seed=2230 + i), np.uint8) for i in range(n)])
    sse, mx = pkg.measure_error_device(A1, d, _to_dev(words.tobytes(), dev), h, w, 4, grid_height=gh, grid_width=gw, n_images=n)
    torch.cuda.synchronize()
    for i in range(n):
        grid = words[i].reshape((gh + 3) // 4, (gw + 3) // 4, 8)
        own = grid[:(h + 3) // 4, :(w + 3) // 4].tobytes()
        want_sse, want_max = _stats(imgs[i], A.oracle_decode(own, h, w).reshape(h, w, 4))
        assert (sse[i].cpu().numpy() == want_sse).all() and (mx[i].cpu().numpy() == want_max).all(), i


def test_17_and_22_are_rejected_with_a_device(dev):
    import torch
    src = torch.zeros(8 * 8 * 4, dtype=torch.uint8, device=dev)
    dst = torch.zeros(64, dtype=torch.uint8, device=dev)
    for codec in (17, 22):
        st = pkg.lib().icamd_encode_device(codec, 2, 4, 0, 8, 8, 8, 8, 32, 1, 0, 0, ctypes.c_void_p(src.data_ptr()),
                                           ctypes.c_void_p(dst.data_ptr()), None)
        assert st == -4
