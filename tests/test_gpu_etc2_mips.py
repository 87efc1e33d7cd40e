"""GPU tier of the ETC2-family mip chains (include/ic_amd.h icamd_encode_etc2_mips_device): the chain kernels --
every level of every image in one encode launch -- against the COMPOSITION they replace, byte for byte: the pixel pyramid
(icamd_mip_pyramid_device / _filtered_device), then icamd_encode_device / icamd_encode_etc2_device on every level, all entry
points that exist without the chain.  On 37 x 21 the chain is also held against the CPU oracles of the five codecs on the numpy
pyramid.  Small shapes that still reach every branch:
  37 x 21, 6 levels: clamped edges in both directions, levels narrower than a block, every level one partly filled workgroup;
  8 x 516, 10 levels: 129 block columns (nine 16 x 16 tiles in a row, the last one block wide), a pixel pyramid of two passes with
    a hand-off, seven levels of one block;
  64 x 64 x 3 images, rows and images padded on both sides: the image strides of source, workspace and chain.
Every test runs under a time limit of its own (the process is ended if a step hangs), and after a failed device call nothing more
is launched."""
import ctypes
import faulthandler
import functools
import importlib

import numpy as np
import pytest

import eac11_oracle as E11
import etc2_a1_oracle as A1
import etc2_colour_oracle as C
import etc2_oracle as E2
import etc2_th_oracle as H
import ic_testlib as T
import mip_filter_oracle as F
import mips_oracle as M
import normal_filter_oracle as N

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("image-compression_amd")
RGBA8, RGB8, RGB8A1, R11, RG11 = E2.ETC2_RGBA8, C.ETC2_RGB8, A1.ETC2_RGB8A1, E11.EAC_R11, E11.EAC_RG11
ERR_ARG = -4
STEP_SECONDS = 120
# (codec, source components, [swap_rb], [etc_strategy]) -- every layout each codec accepts; 7 is out of range: kSmallerError
LAYOUTS = [(RGB8, 3, (0, 1), (0, 1, 2, 3, 7)), (RGB8, 4, (0, 1), (0, 1, 2, 3)), (RGBA8, 4, (0, 1), (0, 1, 2, 3, 7)),
           (RGB8A1, 4, (0, 1), (0, 1, 2, 3)), (R11, 1, (0,), (2,)), (R11, 2, (0,), (2,)), (R11, 3, (0, 1), (2,)), (R11, 4, (0, 1), (2,)),
           (RG11, 2, (0,), (2,)), (RG11, 3, (0, 1), (2,)), (RG11, 4, (0, 1), (2,))]
_state = {"faulted": None}


@pytest.fixture(scope="module")
def dev():
    import torch
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


@pytest.fixture(autouse=True)
def one_step(request):
    """The time limit of one test, and no launch after a device call failed in an earlier one."""
    if _state["faulted"]:
        pytest.fail("not run: the device path failed in %s" % _state["faulted"])
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def _guard(request, fn, *a, **kw):
    try:
        return fn(*a, **kw)
    except (pkg.BackendError, RuntimeError):
        _state["faulted"] = request.node.name
        raise


@functools.lru_cache(maxsize=None)
def _img(h, w, comps, index=0):
    """Noise, a smooth ramp, flat areas and a cut-out alpha (4 components), in quadrants that do not line up with blocks."""
    g = np.random.Generator(np.random.PCG64(T.SEED0 + 9900 + index))
    y, x = np.mgrid[0:h, 0:w]
    ramp = ((3 * x + 5 * y + 40 * index) % 256)[..., None] + np.arange(comps) * 37
    img = g.integers(0, 256, (h, w, comps))
    img = np.where((x > w // 2 + 1)[..., None], ramp + g.integers(-4, 5, (h, w, comps)), img)
    img = np.where(((y > h // 2 + 1) & (x <= w // 2 + 1))[..., None], np.array([90, 200, 30, 255])[:comps], img)
    img = np.clip(img, 0, 255).astype(np.uint8)
    if comps == 4:
        img[..., 3] = A1.alpha_blobs(h, w, index)
    img.setflags(write=False)
    return img


def _to_dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).copy()).to(dev)


def _sync():
    import torch
    torch.cuda.synchronize()


def _composition(codec, d_src, h, w, comps, dev, *, levels=None, swap=0, strategy=2, modes=0, mip_filter=0, n=1, row_stride=None,
                 src_image_stride=None):
    """[level][image] -> bytes, through the entry points that exist without the chain; also the pyramid's level views."""
    levels = pkg.mip_max_levels(h, w) if levels is None else levels
    _, pix = pkg.mip_pyramid_device(d_src, h, w, comps, levels=levels, n_images=n, row_stride_bytes=row_stride,
                                    src_image_stride_bytes=src_image_stride, mip_filter=mip_filter)
    out = [pkg.encode_device(codec, d_src, h, w, comps, swap_rb=bool(swap), etc_strategy=strategy, etc2_modes=modes, n_images=n,
                             row_stride_bytes=row_stride, src_image_stride_bytes=src_image_stride)]
    for l in range(1, levels):
        lh, lw = M.level_shape(h, w, l)
        level = pix[l - 1].contiguous().view(-1)  # [n, lh, lw, comps], tight
        out.append(pkg.encode_device(codec, level, lh, lw, comps, swap_rb=bool(swap), etc_strategy=strategy, etc2_modes=modes, n_images=n))
    _sync()
    return [[o[i].cpu().numpy().tobytes() for i in range(n)] for o in out], pix


def _chain(codec, d_src, h, w, comps, **kw):
    flat, views = pkg.encode_etc2_mips_device(codec, d_src, h, w, comps, **kw)
    _sync()
    return flat, views


def _oracle_level(codec, p, comps, swap, strategy, modes=0):
    h, w = p.shape[:2]
    s = strategy if strategy < 4 else T.SMALLER_ERROR
    if codec == RGB8:
        return H.oracle_encode(p, h, w, comps, swap, s, modes=modes) if modes else C.oracle_encode(p, h, w, comps, swap, s)
    if codec == RGBA8:
        return E2.oracle_encode(p, h, w, swap, s)
    if codec == RGB8A1:
        return A1.oracle_encode(p, h, w, swap, s)
    return E11.oracle_encode(codec, p, h, w, comps, swap)


@pytest.mark.parametrize("codec,comps,swaps,strategies", LAYOUTS, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("h,w", [(37, 21), (8, 516)])
def test_chain_is_the_composition_byte_for_byte(dev, request, h, w, codec, comps, swaps, strategies):
    img = _img(h, w, comps, index=codec)
    d_src = _to_dev(img, dev)
    levels = pkg.mip_max_levels(h, w)
    total, offs = pkg.etc2_mip_chain_size(codec, h, w)
    pyramid = M.pyramid(img) if (h, w) == (37, 21) else None
    for swap in swaps:
        for strategy in strategies:
            want, pix = _guard(request, _composition, codec, d_src, h, w, comps, dev, swap=swap, strategy=strategy)
            flat, views = _guard(request, _chain, codec, d_src, h, w, comps, swap_rb=bool(swap), etc_strategy=strategy)
            assert tuple(flat.shape) == (1, total) and len(views) == levels
            for l in range(levels):
                got = views[l][0].cpu().numpy().tobytes()
                assert len(got) == offs[l + 1] - offs[l] == pkg.encoded_size(codec, *M.level_shape(h, w, l))
                assert got == want[l][0], (codec, comps, swap, strategy, "level", l)
                if pyramid is not None:  # and both are the definition: the CPU oracle of the codec on the numpy pyramid
                    if l:
                        assert pix[l - 1][0].cpu().numpy().tobytes() == pyramid[l].tobytes()
                    assert got == _oracle_level(codec, pyramid[l], comps, swap, strategy), (codec, comps, swap, strategy, "oracle", l)


@pytest.mark.parametrize("codec,comps,swap,strategy", [(RGB8, 3, 1, 2), (RGB8, 4, 0, 3), (RGBA8, 4, 0, 2), (RGB8A1, 4, 1, 0), (R11, 1, 0, 2),
                                                       (RG11, 2, 0, 2), (RG11, 4, 1, 2)])
def test_batch_with_padded_rows_and_image_strides(dev, request, codec, comps, swap, strategy):
    import torch
    h = w = 64
    n, levels = 3, 7
    row_stride, gap = w * comps + 5, 40
    src_image_stride = h * row_stride + gap
    g = np.random.Generator(np.random.PCG64(T.SEED0 + 9950 + codec))
    buf = g.integers(0, 256, n * src_image_stride, dtype=np.uint8)  # (the padding is noise: it must not be read as pixels)
    for i in range(n):
        rows = buf[i * src_image_stride:i * src_image_stride + h * row_stride].reshape(h, row_stride)
        rows[:, :w * comps] = _img(h, w, comps, index=20 + i).reshape(h, w * comps)
    d_src = _to_dev(buf, dev)
    total, offs = pkg.etc2_mip_chain_size(codec, h, w, levels)
    per = total + 24
    out = torch.full((n, per), 0xA5, dtype=torch.uint8, device=dev)
    ws_bytes = pkg.etc2_mip_workspace_size(codec, comps, h, w, levels, n)
    ws = torch.zeros((ws_bytes + 64,), dtype=torch.uint8, device=dev)  # (a caller's workspace, larger than needed)
    want, _ = _guard(request, _composition, codec, d_src, h, w, comps, dev, levels=levels, swap=swap, strategy=strategy, n=n,
                     row_stride=row_stride, src_image_stride=src_image_stride)
    flat, views = _guard(request, _chain, codec, d_src, h, w, comps, levels=levels, swap_rb=bool(swap), etc_strategy=strategy, n_images=n,
                         row_stride_bytes=row_stride, src_image_stride_bytes=src_image_stride, dst_image_stride_bytes=per, out=out,
                         workspace=ws)
    assert flat.data_ptr() == out.data_ptr()
    host = out.cpu().numpy()
    for i in range(n):
        for l in range(levels):
            assert host[i, offs[l]:offs[l + 1]].tobytes() == want[l][i] == views[l][i].cpu().numpy().tobytes(), (i, l)
        assert (host[i, total:] == 0xA5).all(), "the gap after image %d's chain was written" % i
    assert (ws[ws_bytes:].cpu().numpy() == 0).all(), "the workspace was written past icamd_etc2_mip_workspace_size"


@pytest.mark.parametrize("comps", [3, 4])
def test_t_and_h_modes_on_hard_edges(dev, request, comps):
    h, w = 61, 59
    img = H.edges(6, h, w, comps)
    d_src = _to_dev(img, dev)
    levels = pkg.mip_max_levels(h, w)
    want, _ = _guard(request, _composition, RGB8, d_src, h, w, comps, dev, modes=pkg.ETC2_MODES_TH)
    _, th = _guard(request, _chain, RGB8, d_src, h, w, comps, etc2_modes=pkg.ETC2_MODES_TH)
    _, plain = _guard(request, _chain, RGB8, d_src, h, w, comps)
    pyramid = M.pyramid(img)
    changed = 0
    for l in range(levels):
        got = th[l][0].cpu().numpy()
        assert got.tobytes() == want[l][0], l
        lh, lw = M.level_shape(h, w, l)
        assert got.tobytes() == H.oracle_encode(pyramid[l], lh, lw, comps, 0, T.SMALLER_ERROR), ("oracle", l)
        changed += int((got.reshape(-1, 8) != plain[l][0].cpu().numpy().reshape(-1, 8)).any(axis=1).sum())
    assert changed > 0, "no block of any level became T or H: the second launch did nothing"


def test_one_filter_per_family(dev, request):
    h, w = 37, 21
    cases = [(RGB8, 3, pkg.MIP_FILTER_SRGB, _img(h, w, 3, index=31)),
             (RGB8A1, 4, pkg.MIP_FILTER_ALPHA_WEIGHTED, _img(h, w, 4, index=32)),  # (a cut-out alpha: A1.alpha_blobs)
             (RG11, 2, pkg.MIP_FILTER_NORMAL, N.normal_image(h, w, 2, index=33))]
    for codec, comps, f, img in cases:
        d_src = _to_dev(img, dev)
        want, _ = _guard(request, _composition, codec, d_src, h, w, comps, dev, mip_filter=f)
        _, views = _guard(request, _chain, codec, d_src, h, w, comps, mip_filter=f)
        _, box = _guard(request, _chain, codec, d_src, h, w, comps)
        pyramid = N.pyramid(img) if f == pkg.MIP_FILTER_NORMAL else F.pyramid(img, f)
        differs = False
        for l in range(len(views)):
            got = views[l][0].cpu().numpy().tobytes()
            assert got == want[l][0], (codec, f, l)
            assert got == _oracle_level(codec, pyramid[l], comps, 0, 2), (codec, f, "oracle", l)
            differs |= got != box[l][0].cpu().numpy().tobytes()
        assert differs, "filter %d changed no level of codec %d" % (f, codec)


@pytest.mark.parametrize("codec,comps", [(RGBA8, 4), (RGB8, 3), (RGB8A1, 4), (R11, 1), (RG11, 2)])
def test_levels_decode_measure_and_frame(dev, request, codec, comps):
    h, w = 37, 21
    img = _img(h, w, comps, index=40 + codec)
    d_src = _to_dev(img, dev)
    levels = pkg.mip_max_levels(h, w)
    _, views = _guard(request, _chain, codec, d_src, h, w, comps)
    pyramid = M.pyramid(img)
    for l in range(levels):
        lh, lw = M.level_shape(h, w, l)
        blocks = views[l][0].contiguous()
        dec = _guard(request, pkg.decode_device, codec, blocks, lh, lw)
        sse, mx = _guard(request, pkg.measure_error_device, codec, _to_dev(pyramid[l], dev), blocks, lh, lw, comps)
        _sync()
        dec = dec.cpu().numpy().reshape(lh, lw, -1)
        assert dec.shape[2] == comps
        diff = pyramid[l].astype(np.int64) - dec.astype(np.int64)
        want_sse, want_max = np.zeros(4, np.int64), np.zeros(4, np.int64)
        want_sse[:comps], want_max[:comps] = (diff * diff).sum(axis=(0, 1)), np.abs(diff).max(axis=(0, 1))
        assert (sse[0].cpu().numpy() == want_sse).all() and (mx[0].cpu().numpy() == want_max).all(), l
    ktx = pkg.container_write(pkg.CONTAINER_KTX, codec, h, w, [v[0].cpu().numpy().tobytes() for v in views])
    assert ktx is not None and len(ktx) == pkg.container_size(pkg.CONTAINER_KTX, codec, h, w, levels)


def test_capture_and_replay_on_one_stream(dev, request):
    import torch
    h, w, comps = 200, 136, 3
    first_img, second_img = H.edges(6, h, w, comps, seed=1), H.edges(9, h, w, comps, seed=2)
    src = _to_dev(first_img, dev)
    kw = dict(etc2_modes=pkg.ETC2_MODES_TH, etc_strategy=3)
    want_first = _guard(request, _chain, RGB8, src, h, w, comps, **kw)[0].cpu().numpy().tobytes()
    want_second = _guard(request, _chain, RGB8, _to_dev(second_img, dev), h, w, comps, **kw)[0].cpu().numpy().tobytes()
    total, _ = pkg.etc2_mip_chain_size(RGB8, h, w)
    out = torch.zeros((1, total), dtype=torch.uint8, device=dev)
    ws = torch.zeros((pkg.etc2_mip_workspace_size(RGB8, comps, h, w),), dtype=torch.uint8, device=dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # the pyramid pass, the encode launch and the T / H launch, in stream order
        pkg.encode_etc2_mips_device(RGB8, src, h, w, comps, out=out, workspace=ws, stream=torch.cuda.current_stream(), **kw)
    g.replay()
    _sync()
    first = out.cpu().numpy().tobytes()
    src.copy_(_to_dev(second_img, dev))
    g.replay()
    _sync()
    assert first == want_first and want_first != want_second
    assert out.cpu().numpy().tobytes() == want_second


def test_the_level_order_inside_the_launch_changes_no_byte(dev, request):
    h, w = 8, 516
    for codec, comps in ((RGB8A1, 4), (RG11, 2)):
        d_src = _to_dev(_img(h, w, comps, index=50 + codec), dev)
        default = _guard(request, _chain, codec, d_src, h, w, comps)[0].cpu().numpy().tobytes()
        pkg.etc2_mip_tune(0)  # the smallest level's workgroups first
        try:
            other = _guard(request, _chain, codec, d_src, h, w, comps)[0].cpu().numpy().tobytes()
        finally:
            pkg.etc2_mip_tune(1)
        assert other == default


def test_refused_combinations_with_a_device_present(dev):
    import torch
    lib = pkg.lib()
    src = torch.zeros((64 * 64 * 4,), dtype=torch.uint8, device=dev)
    out = torch.full((1 << 15,), 0x5A, dtype=torch.uint8, device=dev)
    ws = torch.zeros((1 << 15,), dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(codec, comps, strategy=2, modes=0, swap=0, f=0, levels=7, ws_bytes=1 << 15):
        return lib.icamd_encode_etc2_mips_device(codec, strategy, modes, comps, swap, f, 64, 64, 64 * comps, levels, 1, 0, 0,
                                                 p(src), p(out), p(ws), ws_bytes, None)

    refused = [call(T.ETC1, 3), call(T.DXT1, 4), call(RGBA8, 3), call(RGB8A1, 3), call(RGB8, 2), call(RG11, 1), call(R11, 5),
               call(RGBA8, 4, modes=1), call(R11, 1, modes=1), call(RGB8, 3, modes=2), call(R11, 2, swap=1), call(R11, 1, f=1),
               call(RG11, 3, f=4), call(RGB8, 3, f=2), call(RGB8, 4, f=4), call(RGBA8, 4, f=5), call(RGB8, 3, levels=8),
               call(RGB8, 3, levels=0), call(RGB8, 3, ws_bytes=10)]
    assert refused == [ERR_ARG] * len(refused)
    _sync()
    assert (out.cpu().numpy() == 0x5A).all()
    for codec in (RGBA8, RGB8, RGB8A1, R11, RG11):  # and the old entry points answer what they answered
        assert lib.icamd_encode_mips_device(codec, 2, 4, 0, 64, 64, 256, 7, 1, 0, 0, p(src), p(out), p(ws), 1 << 15, None) == ERR_ARG
        assert pkg.mip_chain_size(codec, 64, 64) == (0, None)
