"""GPU tier for ICAMD_ETC2_RGB8 and the complete ETC2 colour-word decoder (include/ic_amd.h): the HIP kernels
through the C ABI and the Python wrappers, every case bit-exact against the numpy definition (tests/etc2_colour_oracle.py)."""
import ctypes
import functools
import importlib

import numpy as np
import pytest

import bc45_oracle as B
import etc2_colour_oracle as C
import etc2_oracle as E
import ic_testlib as T

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("image-compression_amd")
RGB8, RGBA8 = C.ETC2_RGB8, E.ETC2_RGBA8
PADDED = [(30, 30, 40, 48), (5, 3, 16, 16), (1, 1, 9, 13), (64, 61, 64, 64)]


@pytest.fixture(scope="module")
def dev():
    import torch
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


def _to_dev(buf, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.frombuffer(bytes(buf), np.uint8)).copy()).to(dev)


def _encode(codec, flat, h, w, comps, dev, **kw):
    import torch
    out = pkg.encode_device(codec, _to_dev(flat, dev), h, w, comps, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _decode(codec, words, h, w, dev, **kw):
    import torch
    out = pkg.decode_device(codec, _to_dev(words, dev), h, w, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _rgba8_words(h, w, seed, only=None):
    """ETC2 RGBA8 blocks: any alpha word, colour words of all five modes (or of one)."""
    words = np.frombuffer(E.random_words(h, w, seed), np.uint8).reshape(-1, 16).copy()
    words[:, 8:] = np.frombuffer(C.random_colour_words(h, w, seed + 1, only=only), np.uint8).reshape(-1, 8)
    return words.tobytes()


@functools.lru_cache(maxsize=None)
def _half_and_half(comps):
    return C.smooth_and_noise(comps)


@functools.lru_cache(maxsize=None)
def _want_half_and_half(comps, strategy):
    return C.oracle_encode(_half_and_half(comps), 64, 64, comps, 0, strategy, return_choice=True)


def _stats(img, dec):
    d = img.astype(np.int64) - dec.astype(np.int64)
    return (d * d).sum(axis=(0, 1)), np.abs(d).max(axis=(0, 1))


# ---- decode

@pytest.mark.parametrize("swap", [0, 1])
def test_decode_all_five_modes_in_every_wave(dev, swap):
    h, w = 4, 1024
    words = C.random_colour_words(h, w, seed=900)
    assert (np.bincount(C.modes(words).reshape(-1, 64)[0], minlength=5) >= 12).all()  # every wave of 64 blocks holds all five
    assert _decode(RGB8, words, h, w, dev, swap_rb=bool(swap)).tobytes() == C.oracle_decode(words, h, w).tobytes()
    both = _rgba8_words(h, w, seed=910)
    assert _decode(RGBA8, both, h, w, dev, swap_rb=bool(swap)).tobytes() == C.oracle_decode_rgba8(both, h, w, swap).tobytes()


@pytest.mark.parametrize("mode", [C.INDIVIDUAL, C.DIFFERENTIAL, C.T_MODE, C.H_MODE, C.PLANAR])
def test_decode_one_mode_per_strip(dev, mode):
    h, w = 4, 1024
    words = C.random_colour_words(h, w, seed=920 + mode, only=mode)
    assert _decode(RGB8, words, h, w, dev).tobytes() == C.oracle_decode(words, h, w).tobytes()
    both = _rgba8_words(h, w, seed=930 + mode, only=mode)
    assert _decode(RGBA8, both, h, w, dev).tobytes() == C.oracle_decode_rgba8(both, h, w).tobytes()


@pytest.mark.parametrize("h,w", [(5, 3), (17, 33)])
def test_decode_clipped_edges(dev, h, w):
    for swap in (0, 1):
        for pad in (0, 5):
            words = C.random_colour_words(h, w, seed=940 + h)
            got = _decode(RGB8, words, h, w, dev, swap_rb=bool(swap), padding_bytes_per_row=pad)
            assert got.tobytes() == C.oracle_decode(words, h, w, pad).tobytes(), (swap, pad)
            both = _rgba8_words(h, w, seed=950 + h)
            got = _decode(RGBA8, both, h, w, dev, swap_rb=bool(swap), padding_bytes_per_row=pad)
            assert got.tobytes() == C.oracle_decode_rgba8(both, h, w, swap, pad).tobytes(), (swap, pad)


@pytest.mark.parametrize("codec", [RGB8, RGBA8])
def test_decode_batch_with_row_padding_and_image_strides(dev, codec):
    import torch
    h, w, n, pad = 17, 33, 2, 7
    bb, comps = (8, 3) if codec == RGB8 else (16, 4)
    per_in = ((h + 3) // 4) * ((w + 3) // 4) * bb
    in_slot, out_row = per_in + 24, w * comps + pad
    out_slot = h * out_row + 11
    words = [C.random_colour_words(h, w, seed=960 + i) if codec == RGB8 else _rgba8_words(h, w, seed=970 + 2 * i) for i in range(n)]
    buf = np.zeros(n * in_slot, np.uint8)
    for i, wd in enumerate(words):
        buf[i * in_slot:i * in_slot + per_in] = np.frombuffer(wd, np.uint8)
    d_in = _to_dev(buf.tobytes(), dev)
    d_out = torch.zeros(n * out_slot, dtype=torch.uint8, device=dev)
    st = pkg.lib().icamd_decode_device(codec, 0, h, w, pad, n, in_slot, out_slot, ctypes.c_void_p(d_in.data_ptr()),
                                       ctypes.c_void_p(d_out.data_ptr()), None)
    assert st == 0
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    for i, wd in enumerate(words):
        want = C.oracle_decode(wd, h, w, pad) if codec == RGB8 else C.oracle_decode_rgba8(wd, h, w, 0, pad)
        assert got[i * out_slot:i * out_slot + h * out_row].tobytes() == want.tobytes(), i
        assert not got[i * out_slot + h * out_row:(i + 1) * out_slot].any()


# ---- encode

@pytest.mark.parametrize("comps", [3, 4])
@pytest.mark.parametrize("h,w,gh,gw", PADDED)
def test_encode_padded_grid_every_strategy_and_swap(dev, h, w, gh, gw, comps):
    img = B.image("smooth", h, w, comps, index=h + w)
    for strategy in C.STRATEGIES:
        want = C.oracle_encode(img, h, w, comps, 0, strategy, gh=gh, gw=gw)
        for swap in (0, 1):  # (bytes 0..2 as they lie in memory, whatever swap_rb)
            got = _encode(RGB8, img.tobytes(), h, w, comps, dev, etc_strategy=strategy, swap_rb=bool(swap), grid_height=gh, grid_width=gw)
            assert got.tobytes() == want, (h, w, gh, gw, comps, strategy, swap)
            assert want == C.oracle_encode(img, h, w, comps, swap, strategy, gh=gh, gw=gw)


@pytest.mark.parametrize("comps", [3, 4])
def test_encode_both_outcomes_in_every_wave(dev, comps):
    # 64 x 64, smooth on the left, noise on the right: a wave (16 x 4 blocks) holds planar and ETC1 outcomes side by side
    img = _half_and_half(comps)
    for strategy in C.STRATEGIES:
        want, planar = _want_half_and_half(comps, strategy)
        assert planar.sum() >= 64 and (~planar).sum() >= 64  # a condition on the input, from the definition alone
        per_wave = planar.reshape(4, 4, 16).sum(axis=(1, 2))
        assert (per_wave > 0).all() and (per_wave < 64).all()
        for swap in (0, 1):
            got = _encode(RGB8, img.tobytes(), 64, 64, comps, dev, etc_strategy=strategy, swap_rb=bool(swap))
            assert got.tobytes() == want, (comps, strategy, swap)
        etc1 = _encode(pkg.ETC1, img.tobytes(), 64, 64, comps, dev, etc_strategy=strategy).reshape(-1, 8)
        g8 = np.frombuffer(want, np.uint8).reshape(-1, 8)
        assert (g8[~planar] == etc1[~planar]).all()  # an ETC1 outcome is the ETC1 kernels' word


def test_encode_batch_with_row_padding_and_image_stride(dev):
    import torch
    h, w, n, pad = 37, 70, 3, 3
    for comps in (3, 4):
        stride = w * comps + pad
        slot = h * stride + 29
        buf = np.zeros(1 + n * slot, np.uint8)
        imgs = [B.image("mixed" if i else "smooth", h, w, comps, index=20 + i) for i in range(n)]
        for i, im in enumerate(imgs):
            buf[1 + i * slot:1 + i * slot + h * stride] = T.with_row_padding(im, pad)
        d = _to_dev(buf.tobytes(), dev)
        per = C.encoded_size(h, w)
        out = torch.zeros(1 + n * per + 5, dtype=torch.uint8, device=dev)
        st = pkg.lib().icamd_encode_device(RGB8, 2, comps, 0, h, w, h, w, stride, n, slot, per, ctypes.c_void_p(d.data_ptr() + 1),
                                           ctypes.c_void_p(out.data_ptr() + 1), None)
        assert st == 0
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert got[0] == 0 and not got[1 + n * per:].any()
        for i, im in enumerate(imgs):
            assert got[1 + i * per:1 + (i + 1) * per].tobytes() == C.oracle_encode(im, h, w, comps), (comps, i)


def test_encode_wide_grid_takes_the_same_bytes(dev):
    # more than one tile in both directions, a width that is no multiple of the 16-block tile
    h, w = 72, 200
    img = B.image("smooth", h, w, 3, index=7)
    got = _encode(RGB8, img.tobytes(), h, w, 3, dev)
    assert got.tobytes() == C.oracle_encode(img, h, w, 3)


# ---- metric

@pytest.mark.parametrize("comps", [3, 4])
def test_metric_equals_decode_and_never_exceeds_etc1(dev, comps):
    import torch
    cases = [(_half_and_half(comps), 64, 64, 0)] + [(B.image(g, h, w, comps, index=i), h, w, pad)
                                                   for i, (g, h, w, pad) in enumerate([("smooth", 61, 59, 3), ("mixed", 30, 30, 0),
                                                                                       ("flat", 5, 3, 0), ("noise", 1, 1, 0)])]
    for img, h, w, pad in cases:
        stride = w * comps + pad
        d_src = _to_dev(T.with_row_padding(img, pad).tobytes(), dev)
        for strategy in C.STRATEGIES:
            blocks = pkg.encode_device(RGB8, d_src, h, w, comps, etc_strategy=strategy, row_stride_bytes=stride)
            etc1 = pkg.encode_device(pkg.ETC1, d_src, h, w, comps, etc_strategy=strategy, row_stride_bytes=stride)
            sse, mx = pkg.measure_error_device(RGB8, d_src, blocks.reshape(-1), h, w, comps, row_stride_bytes=stride)
            sse1, _ = pkg.measure_error_device(pkg.ETC1, d_src, etc1.reshape(-1), h, w, comps, row_stride_bytes=stride)
            dec = pkg.decode_device(RGB8, blocks.reshape(-1), h, w)
            torch.cuda.synchronize()
            want = C.oracle_decode(blocks.cpu().numpy().tobytes(), h, w).reshape(h, w, 3)
            assert (dec.cpu().numpy().reshape(h, w, 3) == want).all()
            want_sse, want_max = _stats(img[..., :3], want)
            sse, mx = sse[0].cpu().numpy(), mx[0].cpu().numpy()
            assert (sse[:3] == want_sse).all() and (mx[:3] == want_max).all() and sse[3] == 0 and mx[3] == 0, (h, w, strategy)
            # per block by definition, so for the image; per channel it need not hold
            assert sse[:3].sum() <= sse1[0].cpu().numpy()[:3].sum(), (h, w, comps, strategy)


def test_metric_on_a_padded_grid_and_a_batch(dev):
    import torch
    h, w, gh, gw, n = 30, 30, 40, 48, 3
    imgs = np.stack([B.image("smooth", h, w, 3, index=60 + i) for i in range(n)])
    d = torch.from_numpy(imgs.reshape(-1)).to(dev)
    blocks = pkg.encode_device(RGB8, d, h, w, 3, grid_height=gh, grid_width=gw, n_images=n)
    sse, mx = pkg.measure_error_device(RGB8, d, blocks.reshape(-1), h, w, 3, grid_height=gh, grid_width=gw, n_images=n)
    torch.cuda.synchronize()
    for i in range(n):
        grid = np.frombuffer(blocks[i].cpu().numpy().tobytes(), np.uint8).reshape((gh + 3) // 4, (gw + 3) // 4, 8)
        own = grid[:(h + 3) // 4, :(w + 3) // 4].tobytes()
        want_sse, want_max = _stats(imgs[i], C.oracle_decode(own, h, w).reshape(h, w, 3))
        assert (sse[i].cpu().numpy()[:3] == want_sse).all() and (mx[i].cpu().numpy()[:3] == want_max).all(), i


# ---- ETC2 RGBA8: the decoder's new modes, the encoder unchanged

def test_rgba8_metric_of_t_h_and_planar_words(dev):
    import torch
    for h, w in ((16, 64), (17, 33)):
        img = B.image("mixed", h, w, 4, index=h)
        words = _rgba8_words(h, w, seed=980 + h)
        d_src, d_blk = _to_dev(img.tobytes(), dev), _to_dev(words, dev)
        for swap in (0, 1):
            sse, mx = pkg.measure_error_device(RGBA8, d_src, d_blk, h, w, 4, swap_rb=bool(swap))
            torch.cuda.synchronize()
            want_sse, want_max = _stats(img, C.oracle_decode_rgba8(words, h, w, swap).reshape(h, w, 4))
            assert (sse[0].cpu().numpy() == want_sse).all() and (mx[0].cpu().numpy() == want_max).all(), (h, w, swap)


def test_rgba8_encoder_is_unchanged(dev):
    for h, w, gh, gw in PADDED:
        img = B.image("smooth", h, w, 4, index=h + w)
        for strategy in E.STRATEGIES:
            got = _encode(RGBA8, img.tobytes(), h, w, 4, dev, etc_strategy=strategy, grid_height=gh, grid_width=gw)
            assert got.tobytes() == E.oracle_encode(img, h, w, 0, strategy, gh=gh, gw=gw), (h, w, gh, gw, strategy)
            assert (C.modes(got.reshape(-1, 16)[:, 8:]) <= C.DIFFERENTIAL).all()


def test_17_is_rejected_with_a_device(dev):
    import torch
    src = torch.zeros(8 * 8 * 4, dtype=torch.uint8, device=dev)
    dst = torch.zeros(64, dtype=torch.uint8, device=dev)
    st = pkg.lib().icamd_encode_device(17, 2, 3, 0, 8, 8, 8, 8, 24, 1, 0, 0, ctypes.c_void_p(src.data_ptr()),
                                       ctypes.c_void_p(dst.data_ptr()), None)
    assert st == -4
