"""GPU tier for the T / H encoder of ETC2 RGB8 (include/ic_amd.h icamd_encode_etc2_device, ICAMD_ETC2_MODES_TH):
the HIP kernels through the C ABI and the Python keyword, every case bit-exact against the numpy definition
(tests/etc2_th_oracle.py), and the existing decoder and metric kernels on the T and H words the encoder makes."""
import ctypes
import functools
import importlib

import numpy as np
import pytest

import etc2_colour_oracle as C
import etc2_th_oracle as H
import ic_testlib as T

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("image-compression_amd")
RGB8 = C.ETC2_RGB8
STRATEGIES = C.STRATEGIES + (7,)  # (out of range: kSmallerError)


@pytest.fixture(scope="module")
def dev():
    import torch
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


def _to_dev(buf, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.frombuffer(bytes(buf), np.uint8)).copy()).to(dev)


def _encode(flat, h, w, comps, dev, **kw):
    import torch
    out = pkg.encode_device(RGB8, _to_dev(flat, dev), h, w, comps, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _two_colour_block():
    img = np.empty((4, 4, 3), np.uint8)
    img[:, :2], img[:, 2:] = (200, 40, 30), (30, 60, 200)
    img[1, 1] = (190, 50, 40)
    return img


# name -> (image, h, w, grid_height, grid_width)
SHAPES = {
    "one_block": lambda: (_two_colour_block(), 4, 4, 4, 4),
    "mixed_tile": lambda: (H.mixed(), 64, 64, 64, 64),
    "padded_grid": lambda: (H.edges(6, 61, 59), 61, 59, 64, 64),          # edge replication + a padded grid
    "partial_tiles": lambda: (H.edges(6, 68, 132), 68, 132, 68, 132),     # 33 x 17 blocks: partial tiles in both directions
}


@functools.lru_cache(maxsize=None)
def _shape(name):
    img, h, w, gh, gw = SHAPES[name]()
    img.setflags(write=False)
    return img, h, w, gh, gw


@functools.lru_cache(maxsize=None)
def _want(name, strategy):
    """(bytes, choice) of the definition; the source's fourth byte and swap_rb do not enter."""
    img, h, w, gh, gw = _shape(name)
    return H.oracle_encode(img, h, w, 3, 0, strategy if strategy < 4 else T.SMALLER_ERROR, gh=gh, gw=gw, return_choice=True)


def _source(img, comps):
    if comps == 3:
        return np.ascontiguousarray(img)
    g = np.random.Generator(np.random.PCG64(T.SEED0 + 9730))
    out = g.integers(0, 256, img.shape[:2] + (4,), dtype=np.uint8)  # any alpha: it is ignored
    out[..., :3] = img
    return out


@pytest.mark.parametrize("comps", [3, 4])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_bytes_equal_the_definition(dev, name, comps):
    img, h, w, gh, gw = _shape(name)
    src = _source(img, comps)
    for strategy in STRATEGIES:
        want, choice = _want(name, strategy)
        assert H.changed(choice).any(), (name, strategy)  # a condition on the input: the new kernel has something to write
        if name == "mixed_tile":
            assert all(min(k) >= 4 for k in H.wave_kinds(img, strategy=strategy if strategy < 4 else 2))
        for swap in (0, 1):
            got = _encode(src.tobytes(), h, w, comps, dev, etc_strategy=strategy, swap_rb=bool(swap), grid_height=gh,
                          grid_width=gw, etc2_modes=pkg.ETC2_MODES_TH)
            assert got.tobytes() == want, (name, comps, strategy, swap)


@functools.lru_cache(maxsize=None)
def _batch_image(i):
    img = (H.mixed, lambda: H.edges(6), H.equiluminant)[i]()
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _want_batch(i, strategy):
    return H.oracle_encode(_batch_image(i), 64, 64, 3, 0, strategy if strategy < 4 else T.SMALLER_ERROR)


@pytest.mark.parametrize("comps", [3, 4])
def test_batch_with_padded_strides_leaves_the_gaps_alone(dev, comps):
    import torch
    h = w = 64
    pad, n = 5, 3
    imgs = [_batch_image(i) for i in range(n)]
    stride = w * comps + pad
    slot = h * stride + 29
    buf = np.zeros(1 + n * slot, np.uint8)
    for i, im in enumerate(imgs):
        buf[1 + i * slot:1 + i * slot + h * stride] = T.with_row_padding(_source(im, comps), pad)
    d = _to_dev(buf.tobytes(), dev)
    per = C.encoded_size(h, w)
    out_slot = per + 24
    for strategy in STRATEGIES:
        for swap in (0, 1):
            out = torch.full((1 + n * out_slot + 5,), 0xa5, dtype=torch.uint8, device=dev)
            st = pkg.lib().icamd_encode_etc2_device(RGB8, strategy, 1, comps, swap, h, w, h, w, stride, n, slot, out_slot,
                                                    ctypes.c_void_p(d.data_ptr() + 1), ctypes.c_void_p(out.data_ptr() + 1), None)
            assert st == 0
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert got[0] == 0xa5 and (got[1 + n * out_slot:] == 0xa5).all()
            for i in range(n):
                at = 1 + i * out_slot
                assert got[at:at + per].tobytes() == _want_batch(i, strategy), (comps, strategy, swap, i)
                assert (got[at + per:at + out_slot] == 0xa5).all(), (comps, strategy, swap, i)


@pytest.mark.parametrize("comps", [3, 4])
def test_modes_default_is_icamd_encode_device(dev, comps):
    import torch
    for name in sorted(SHAPES):
        img, h, w, gh, gw = _shape(name)
        src = _to_dev(_source(img, comps).tobytes(), dev)
        per = C.encoded_size(gh, gw)
        for strategy in STRATEGIES:
            plain = pkg.encode_device(RGB8, src, h, w, comps, etc_strategy=strategy, grid_height=gh, grid_width=gw)
            out = torch.zeros((1, per), dtype=torch.uint8, device=dev)
            st = pkg.lib().icamd_encode_etc2_device(RGB8, strategy, 0, comps, 0, h, w, gh, gw, w * comps, 1, 0, per,
                                                    ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(out.data_ptr()), None)
            assert st == 0
            torch.cuda.synchronize()
            assert (out == plain).all(), (name, comps, strategy)
    assert pkg.etc2_kernel_name(RGB8, comps, 0) == pkg.kernel_name(RGB8, comps)  # the kernels of icamd_encode_device, by name


@pytest.mark.parametrize("comps", [3, 4])
def test_round_trip_through_the_decoder_and_the_metric(dev, comps):
    import torch
    for name in ("mixed_tile", "padded_grid", "partial_tiles"):
        img, h, w, _, _ = _shape(name)
        d_src = _to_dev(_source(img, comps).tobytes(), dev)
        blocks = pkg.encode_device(RGB8, d_src, h, w, comps, etc2_modes=pkg.ETC2_MODES_TH)
        plain = pkg.encode_device(RGB8, d_src, h, w, comps)
        dec = pkg.decode_device(RGB8, blocks.reshape(-1), h, w)
        sse, mx = pkg.measure_error_device(RGB8, d_src, blocks.reshape(-1), h, w, comps)
        sse0, _ = pkg.measure_error_device(RGB8, d_src, plain.reshape(-1), h, w, comps)
        torch.cuda.synchronize()
        want = H.oracle_encode(img, h, w, 3)
        assert blocks.cpu().numpy().tobytes() == want
        m = C.modes(want)
        assert (m == C.T_MODE).any() and (m == C.H_MODE).any()  # the decoder and the metric meet encoder-made T and H words
        want_dec = C.oracle_decode(want, h, w).reshape(h, w, 3)
        assert (dec.cpu().numpy().reshape(h, w, 3) == want_dec).all(), name
        diff = img.astype(np.int64) - want_dec.astype(np.int64)
        sse, mx = sse[0].cpu().numpy(), mx[0].cpu().numpy()
        assert (sse[:3] == (diff * diff).sum(axis=(0, 1))).all() and (mx[:3] == np.abs(diff).max(axis=(0, 1))).all(), name
        assert sse[:3].sum() < sse0[0].cpu().numpy()[:3].sum(), name  # (<= by definition; < because blocks changed)


def test_metric_per_image_of_a_batch(dev):
    import torch
    imgs = np.stack([H.mixed(), H.edges(6), H.equiluminant()])
    d = torch.from_numpy(imgs.reshape(-1)).to(dev)
    blocks = pkg.encode_device(RGB8, d, 64, 64, 3, n_images=3, etc2_modes=pkg.ETC2_MODES_TH)
    plain = pkg.encode_device(RGB8, d, 64, 64, 3, n_images=3)
    sse, _ = pkg.measure_error_device(RGB8, d, blocks.reshape(-1), 64, 64, 3, n_images=3)
    sse0, _ = pkg.measure_error_device(RGB8, d, plain.reshape(-1), 64, 64, 3, n_images=3)
    torch.cuda.synchronize()
    for i in range(3):
        want = H.oracle_encode(imgs[i], 64, 64, 3)
        assert blocks[i].cpu().numpy().tobytes() == want, i
        diff = imgs[i].astype(np.int64) - C.oracle_decode(want, 64, 64).reshape(64, 64, 3).astype(np.int64)
        assert sse[i].cpu().numpy()[:3].sum() == (diff * diff).sum(), i
        assert sse[i].cpu().numpy()[:3].sum() <= sse0[i].cpu().numpy()[:3].sum(), i


def test_equiluminant_fixture_is_h_everywhere(dev):
    img = H.equiluminant()
    got = _encode(img.tobytes(), 64, 64, 3, dev, etc2_modes=pkg.ETC2_MODES_TH)
    assert (C.modes(got.reshape(-1, 8)) == C.H_MODE).all()
    assert got.tobytes() == H.oracle_encode(img, 64, 64, 3)


def test_gradient_fixture_is_the_default_encode(dev):
    img = C.gradient(64, 64)
    got = _encode(img.tobytes(), 64, 64, 3, dev, etc2_modes=pkg.ETC2_MODES_TH)
    assert got.tobytes() == _encode(img.tobytes(), 64, 64, 3, dev).tobytes() == C.oracle_encode(img, 64, 64, 3)


def test_other_codecs_and_modes_are_refused_with_a_device(dev):
    import torch
    src = torch.zeros(8 * 8 * 4, dtype=torch.uint8, device=dev)
    dst = torch.full((64,), 0xa5, dtype=torch.uint8, device=dev)
    for codec, modes in ((16, 1), (21, 1), (2, 1), (18, 2), (18, -1)):
        st = pkg.lib().icamd_encode_etc2_device(codec, 2, modes, 4, 0, 8, 8, 8, 8, 32, 1, 0, 0, ctypes.c_void_p(src.data_ptr()),
                                                ctypes.c_void_p(dst.data_ptr()), None)
        assert st == -4, (codec, modes)
    torch.cuda.synchronize()
    assert (dst == 0xa5).all()
