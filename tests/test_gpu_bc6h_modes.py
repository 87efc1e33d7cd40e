"""GPU tier for BC6H's opt-in two-subset candidate (include/ic_amd.h ICAMD_BC6H_MODES_EXTENDED): the fused HIP
kernels through icamd_encode_bc6h_modes_device and the Python wrapper, byte for byte against the definition's numpy restatement
(tests/bc6h_modes_oracle.py); DEFAULT against icamd_encode_bc6h_device; the device metric against the oracle's claimed sse.  The
definition's blocks of a test image are computed once and shared by every layout that reads the image."""
import functools
import importlib

import numpy as np
import pytest

import bc6h_modes_oracle as M
import bc6h_oracle as B

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("image-compression_amd")
UF16, SF16 = B.BC6H_UF16, B.BC6H_SF16
SHAPES = [(1, 1), (4, 4), (5, 3), (9, 2), (61, 59)]
PAD = 6  # bytes of row padding
PADDED = [(5, 3, 16, 16), (30, 30, 40, 48)]
EXT = M.MODES_EXTENDED


@pytest.fixture(scope="module")
def dev():
    import torch
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


def _codec(signed):
    return SF16 if signed else UF16


def _halves_to_dev(arr, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int16).reshape(-1).copy()).to(dev)


def _rows(img, pad):
    h, w, chans = img.shape
    rows = np.zeros((h, w * chans + pad // 2), np.uint16)
    rows[:, :w * chans] = img.reshape(h, w * chans)
    return rows


@functools.lru_cache(maxsize=None)
def _image(name, h, w, seed=0):
    img = M.content(name, h, w, 4, seed)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _want(name, h, w, signed, gh=None, gw=None, seed=0):
    return M.oracle_encode(_image(name, h, w, seed), signed, gh, gw)  # (the fourth sample is not read: one answer for 3 and 4)


def _source(name, h, w, chans, seed=0):
    return np.ascontiguousarray(_image(name, h, w, seed)[..., :chans])


def _encode(dev, img, signed, modes=EXT, pad=0, **kw):
    import torch
    h, w, chans = img.shape
    out = pkg.encode_bc6h_modes_device(_codec(signed), _halves_to_dev(_rows(img, pad), dev), h, w, chans, bc6h_modes=modes,
                                       row_stride_bytes=w * chans * 2 + pad, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy().tobytes()


# ---- device against oracle under EXTENDED

@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("chans", [3, 4])
def test_extended_every_shape_on_the_edge_content(dev, signed, chans):
    for h, w in SHAPES:
        assert _encode(dev, _source("edge", h, w, chans), signed, pad=PAD) == _want("edge", h, w, signed), (h, w)


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("name", ["noise", "specials", "exponents", "ldr"])
def test_extended_further_contents(dev, signed, name):
    for chans in (3, 4):
        assert _encode(dev, _source(name, 61, 59, chans), signed) == _want(name, 61, 59, signed), chans


@pytest.mark.parametrize("signed", [False, True])
def test_extended_more_than_128_block_columns(dev, signed):
    for chans in (3, 4):  # (the *_kernel of a wide grid, two block rows)
        assert _encode(dev, _source("edge", 8, 520, chans), signed, pad=PAD) == _want("edge", 8, 520, signed), chans


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("h,w,gh,gw", PADDED)
def test_extended_padded_grid(dev, signed, h, w, gh, gw):
    for chans, name in ((3, "edge"), (4, "noise")):
        got = _encode(dev, _source(name, h, w, chans), signed, grid_height=gh, grid_width=gw)
        assert len(got) == B.encoded_size(gh, gw) and got == _want(name, h, w, signed, gh, gw), (chans, name)


@pytest.mark.parametrize("signed", [False, True])
def test_extended_three_images_with_strides_in_one_launch(dev, signed):
    import torch
    h, w, n, chans = 30, 22, 3, 4
    stride = w * chans * 2 + PAD
    slot = h * stride + 30
    buf = np.zeros(6 + n * slot, np.uint8)
    for i in range(n):
        buf[6 + i * slot:6 + i * slot + h * stride] = _rows(_source("edge", h, w, chans, seed=20 + i), PAD).view(np.uint8).reshape(-1)
    d = torch.from_numpy(buf).to(dev)
    per = B.encoded_size(h, w)
    out = torch.zeros(3 + n * (per + 16) + 5, dtype=torch.uint8, device=dev)
    st = pkg.lib().icamd_encode_bc6h_modes_device(_codec(signed), EXT, chans, h, w, h, w, stride, n, slot, per + 16, d.data_ptr() + 6,
                                                  out.data_ptr() + 3, None)
    assert st == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert not got[:3].any() and not got[3 + n * (per + 16):].any()
    for i in range(n):
        at = 3 + i * (per + 16)
        assert got[at:at + per].tobytes() == _want("edge", h, w, signed, seed=20 + i), i
        assert not got[at + per:at + per + 16].any()


@pytest.mark.parametrize("signed", [False, True])
def test_extended_row_stride_of_4_mib_takes_the_256_x_1_tiles(dev, signed):
    import torch
    h, w, chans, stride = 8, 40, 3, 1 << 22
    img = _source("edge", h, w, chans)
    buf = torch.zeros((h - 1) * stride + w * chans * 2, dtype=torch.uint8, device=dev)
    rows = torch.from_numpy(img.reshape(h, -1).view(np.uint8).copy()).to(dev)
    for y in range(h):
        buf[y * stride:y * stride + w * chans * 2] = rows[y]
    out = pkg.encode_bc6h_modes_device(_codec(signed), buf, h, w, chans, bc6h_modes=EXT, row_stride_bytes=stride)
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == _want("edge", h, w, signed)


# ---- a mixed wave

@pytest.mark.parametrize("signed", [False, True])
def test_extended_a_wave_whose_lanes_disagree(dev, signed):
    """64 blocks, one wave: lanes differ in the ladder's mode (all seven), kept against replaced, each subset's refit taken
    against refused, each anchor exchange, and (signed format) negative against non-negative endpoints."""
    img, flags = M.wave_image(signed)
    for name, f in flags.items():
        if name == "negative endpoint" and not signed:
            continue
        assert f.any() and not f.all(), name
    want = M.oracle_encode(img, signed)
    assert _encode(dev, img, signed) == want


# ---- DEFAULT parity

def test_default_is_icamd_encode_bc6h_device_byte_for_byte(dev):
    import torch
    for signed in (False, True):
        for chans in (3, 4):
            for name, h, w in (("edge", 61, 59), ("noise", 16, 520)):
                img = _source(name, h, w, chans)
                d = _halves_to_dev(_rows(img, PAD), dev)
                ref = pkg.encode_bc6h_device(_codec(signed), d, h, w, chans, row_stride_bytes=w * chans * 2 + PAD)
                torch.cuda.synchronize()
                got = _encode(dev, img, signed, modes=M.MODES_DEFAULT, pad=PAD)
                assert got == ref.cpu().numpy().tobytes() == B.oracle_encode(img, signed), (signed, chans, name)
        assert pkg.bc6h_modes_kernel_name(_codec(signed), 4, M.MODES_DEFAULT) == pkg.bc6h_kernel_name(_codec(signed), 4)


def test_refuses_a_short_row_stride_on_the_device_too(dev):
    import torch
    d = torch.zeros(8 * 8 * 4 * 2, dtype=torch.uint8, device=dev)
    out = torch.zeros(64, dtype=torch.uint8, device=dev)
    for codec in (UF16, SF16):
        for modes in (0, 1):
            assert pkg.lib().icamd_encode_bc6h_modes_device(codec, modes, 4, 8, 8, 8, 8, 62, 1, 0, 0, d.data_ptr(), out.data_ptr(),
                                                            None) == -4
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any()


# ---- metric agreement

@pytest.mark.parametrize("signed", [False, True])
def test_metric_of_the_extended_blocks_is_the_oracles_claim(dev, signed):
    import torch
    h, w, chans = 64, 64, 4
    codec = _codec(signed)
    imgs = [_source("edge", h, w, chans), _source("exponents", h, w, chans), _source("ldr", h, w, chans)]
    d_src = _halves_to_dev(np.stack(imgs), dev)
    sums = {}
    for modes in (M.MODES_DEFAULT, EXT):
        blocks = pkg.encode_bc6h_modes_device(codec, d_src, h, w, chans, bc6h_modes=modes, n_images=len(imgs))
        sse, _ = pkg.measure_error_bc6h_device(codec, d_src, blocks.reshape(-1), h, w, chans, n_images=len(imgs))
        torch.cuda.synchronize()
        sums[modes] = [int(s.sum()) for s in sse.cpu().numpy()]
        for i, img in enumerate(imgs):
            _, st = M.encode_texels(B.block_texels(img, signed), signed, modes, stages=True)
            assert sums[modes][i] == int(st["claimed"].sum()), (modes, i)
    print("summed t-domain sse, default / extended:", sums)
    assert all(e <= d for e, d in zip(sums[EXT], sums[M.MODES_DEFAULT]))
    assert sums[EXT][0] < sums[M.MODES_DEFAULT][0]  # the edge content: strictly below


# ---- graph replay

def test_extended_under_stream_capture_replays_to_the_same_bytes(dev):
    import torch
    h, w, chans = 64, 64, 4
    d = _halves_to_dev(_source("edge", h, w, chans), dev)
    out = torch.zeros(B.encoded_size(h, w), dtype=torch.uint8, device=dev)

    def run(stream):
        assert pkg.lib().icamd_encode_bc6h_modes_device(UF16, EXT, chans, h, w, h, w, w * chans * 2, 1, 0, 0, d.data_ptr(),
                                                        out.data_ptr(), stream) == 0

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
    assert out.cpu().numpy().tobytes() == _want("edge", h, w, False)
