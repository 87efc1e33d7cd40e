"""GPU tier for BC7's opt-in mode-1 / mode-5 candidates (include/ic_amd.h ICAMD_BC7_MODES_EXTENDED): the fused
HIP kernels through icamd_encode_bc7_device and the Python wrapper, byte for byte against the definition's numpy restatement
(tests/bc7_modes_oracle.py); DEFAULT against icamd_encode_device; the device metric against the oracle's claimed sse."""
import functools
import importlib

import numpy as np
import pytest

import bc7_modes_oracle as M
import bc7_oracle as B
import ic_testlib as T

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("image-compression_amd")
BC7 = B.BC7
PAD = 6  # bytes of row padding


@pytest.fixture(scope="module")
def dev():
    import torch
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


@functools.lru_cache(maxsize=None)
def _image(name, h, w, comps, seed=None):
    img = B.content(name, h, w, comps, seed=len(name) if seed is None else seed)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _want(name, h, w, comps, gh=None, gw=None, swap=False, seed=None):
    return M.oracle_encode(_image(name, h, w, comps, seed), gh, gw, swap)


def _encode(dev, img, modes=M.MODES_EXTENDED, **kw):
    import torch
    h, w, comps = img.shape
    pad = kw.pop("pad", 0)
    d = torch.from_numpy(T.with_row_padding(img, pad).copy()).to(dev)
    out = pkg.encode_bc7_device(d, h, w, comps, bc7_modes=modes, row_stride_bytes=w * comps + pad, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy().tobytes()


# ---- device against oracle under EXTENDED

@pytest.mark.parametrize("comps", [3, 4])
@pytest.mark.parametrize("swap", [False, True])
def test_extended_every_shape_and_layout(dev, comps, swap):
    # (4, 32): a 4-row image; (61, 59): clipped blocks; (128, 520): the wide kernel (more than 128 block columns)
    for name, h, w in (("noise", 4, 32), ("noise", 61, 59), ("smooth", 61, 59), ("ramp", 128, 520)):
        img = _image(name, h, w, comps)
        assert _encode(dev, img, swap_rb=swap, pad=PAD) == _want(name, h, w, comps, swap=swap), (name, h, w)


@pytest.mark.parametrize("name", ["two_colour", "varying_alpha", "flat"])
def test_extended_further_contents(dev, name):
    for comps in (3, 4):
        assert _encode(dev, _image(name, 61, 59, comps)) == _want(name, 61, 59, comps), comps


def test_extended_padded_grid(dev):
    for comps, swap in ((3, False), (4, True)):
        got = _encode(dev, _image("smooth", 30, 30, comps), grid_height=40, grid_width=48, swap_rb=swap)
        assert got == _want("smooth", 30, 30, comps, 40, 48, swap)


def test_extended_three_images_with_strides_in_one_launch(dev):
    import torch
    h, w, n, comps = 37, 70, 3, 4
    stride = w * comps + PAD
    slot = h * stride + 30
    buf = np.zeros(6 + n * slot, np.uint8)
    for i in range(n):
        buf[6 + i * slot:6 + i * slot + h * stride] = T.with_row_padding(_image("ramp", h, w, comps, seed=20 + i), PAD)
    d = torch.from_numpy(buf).to(dev)
    per = B.encoded_size(h, w)
    out = torch.zeros(3 + n * (per + 16) + 5, dtype=torch.uint8, device=dev)
    st = pkg.lib().icamd_encode_bc7_device(M.MODES_EXTENDED, comps, 0, h, w, h, w, stride, n, slot, per + 16, d.data_ptr() + 6,
                                           out.data_ptr() + 3, None)
    assert st == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert not got[:3].any() and not got[3 + n * (per + 16):].any()
    for i in range(n):
        at = 3 + i * (per + 16)
        assert got[at:at + per].tobytes() == _want("ramp", h, w, comps, seed=20 + i), i
        assert not got[at + per:at + per + 16].any()


# ---- a mixed wave

def test_extended_a_wave_whose_lanes_disagree_at_every_branch(dev):
    """tests/test_bc7_modes_host.py asserts the image's spread: in every wave some lanes are opaque and some not, some keep
    mode 6, some leave at sse6 = 0, some sub-fits have det = 0, and every flip is taken by some lanes and not by others."""
    img, _ = M.modes_wave_image()
    want = M.oracle_encode(img)
    modes = M.block_modes(want).reshape(64, 64)
    for m in (1, 5, 6):
        assert (modes == m).any(axis=1).all(), m
    assert _encode(dev, img) == want
    img, _ = B.mixed_wave_image()  # the mode-6 encoder's own mixed wave, now under the candidates
    assert _encode(dev, img) == M.oracle_encode(img)


# ---- DEFAULT parity

def test_default_is_icamd_encode_device_byte_for_byte(dev):
    import torch
    for comps in (3, 4):
        for h, w in ((61, 59), (128, 520)):
            img = _image("smooth", h, w, comps)
            d = torch.from_numpy(T.with_row_padding(img, PAD).copy()).to(dev)
            ref = pkg.encode_device(BC7, d, h, w, comps, row_stride_bytes=w * comps + PAD)
            torch.cuda.synchronize()
            assert _encode(dev, img, modes=M.MODES_DEFAULT, pad=PAD) == ref.cpu().numpy().tobytes() == B.oracle_encode(img)
    assert pkg.bc7_kernel_name(4, M.MODES_DEFAULT) == pkg.kernel_name(BC7, 4)


def test_refuses_a_short_row_stride_on_the_device_too(dev):
    import torch
    d = torch.zeros(8 * 8 * 4, dtype=torch.uint8, device=dev)
    out = torch.zeros(64, dtype=torch.uint8, device=dev)
    for modes in (0, 1):
        assert pkg.lib().icamd_encode_bc7_device(modes, 4, 0, 8, 8, 8, 8, 31, 1, 0, 0, d.data_ptr(), out.data_ptr(), None) == -4
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any()


# ---- metric agreement

def test_metric_of_the_extended_blocks_is_the_oracles_claim(dev):
    import torch
    h, w, n = 64, 64, 3
    wave = M.modes_wave_image()[0]
    imgs = [_image("ramp", h, w, 4), _image("noise", h, w, 4), np.ascontiguousarray(wave[:h, 64:64 + w])]
    d_src = torch.from_numpy(np.stack(imgs).reshape(-1).copy()).to(dev)
    sums = {}
    for modes in (M.MODES_DEFAULT, M.MODES_EXTENDED):
        blocks = pkg.encode_bc7_device(d_src, h, w, 4, bc7_modes=modes, n_images=n)
        sse, _ = pkg.measure_error_device(BC7, d_src, blocks.reshape(-1), h, w, 4, n_images=n)
        torch.cuda.synchronize()
        sums[modes] = [int(s.sum()) for s in sse.cpu().numpy()]
        for i, img in enumerate(imgs):
            claimed = M.encode_texels(B.block_texels(img), modes, stages=True)[3]
            assert sums[modes][i] == int(claimed.sum()), (modes, i)
    print("summed sse, default / extended:", sums)
    assert all(e <= d for e, d in zip(sums[M.MODES_EXTENDED], sums[M.MODES_DEFAULT]))


def test_metric_of_the_rgb888_smooth_image_is_strictly_below_defaults(dev):
    import torch
    h, w = 64, 64
    img = _image("smooth", h, w, 3)
    d_src = torch.from_numpy(img.reshape(-1).copy()).to(dev)
    got = {}
    for modes in (M.MODES_DEFAULT, M.MODES_EXTENDED):
        blocks = pkg.encode_bc7_device(d_src, h, w, 3, bc7_modes=modes)
        sse, _ = pkg.measure_error_device(BC7, d_src, blocks.reshape(-1), h, w, 3)
        torch.cuda.synchronize()
        got[modes] = int(sse.cpu().numpy().sum())
        # three channels are measured for a 3-component source; the oracle's decode over the same three
        dec = B.decode(M.oracle_encode(img, modes=modes), h, w).reshape(h, w, 4)[..., :3].astype(np.int64)
        assert got[modes] == int(((dec - img.astype(np.int64)) ** 2).sum()), modes
    print("rgb888 smooth, summed sse default / extended:", got)
    assert got[M.MODES_EXTENDED] < got[M.MODES_DEFAULT]


# ---- graph replay

def test_extended_under_stream_capture_replays_to_the_same_bytes(dev):
    import torch
    h, w = 64, 256
    img = _image("ramp", h, w, 4)
    d = torch.from_numpy(img.reshape(-1).copy()).to(dev)
    out = torch.zeros(B.encoded_size(h, w), dtype=torch.uint8, device=dev)

    def run(stream):
        assert pkg.lib().icamd_encode_bc7_device(M.MODES_EXTENDED, 4, 0, h, w, h, w, w * 4, 1, 0, 0, d.data_ptr(), out.data_ptr(),
                                                 stream) == 0

    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # (the kernel's first launch loads its code: not under capture)
        run(s.cuda_stream)
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            run(torch.cuda.current_stream().cuda_stream)
    out.zero_()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == _want("ramp", h, w, 4)
