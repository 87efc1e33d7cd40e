"""GPU tier for 16-bit and signed EAC R11 / RG11 (include/ic_amd.h, icamd_encode_eac11_16_device): the HIP kernels through the
C ABI and the Python wrappers, every case bit-exact against the numpy definition (tests/eac11_16_oracle.py).  The numpy search
is slow per block, so the definition's words of a test image's channel are computed once and shared by every layout that
reads it."""
import ctypes
import functools
import importlib

import numpy as np
import pytest

import eac11_16_oracle as A
import ic_testlib as T

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("image-compression_amd")
R11, RG11, SR11, SRG11 = A.CODECS
SHAPES = [(1, 1), (5, 3), (4, 4), (9, 2), (61, 59), (128, 260)]  # (128, 260): several tiles and workgroups
PAD = 6  # bytes of row padding
PADDED = [(5, 3, 16, 16), (30, 30, 40, 48)]


@pytest.fixture(scope="module")
def dev():
    import torch
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


def _to_dev(buf, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.frombuffer(bytes(buf), np.uint8)).copy()).to(dev)


def _samples_to_dev(arr, dev):
    """A numpy uint16 / int16 array as a torch.uint16 / torch.int16 device tensor."""
    import torch
    flat = _to_dev(np.ascontiguousarray(arr).tobytes(), dev)
    return flat.view(torch.int16 if arr.dtype == np.int16 else torch.uint16)


@functools.lru_cache(maxsize=None)
def _image4(signed, h, w, seed=0):
    img = A.image(SR11 if signed else R11, h, w, 4, seed=h * 100 + w + seed)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _channel_words(signed, h, w, ch, gh=None, gw=None, seed=0):
    return A.channel_words(_image4(signed, h, w, seed)[..., ch], h, w, signed, gh, gw)


def _want(codec, h, w, gh=None, gw=None, seed=0):
    r = _channel_words(A.is_signed(codec), h, w, 0, gh, gw, seed)
    if A.comps_out(codec) == 1:
        return r.tobytes()
    return np.concatenate([r, _channel_words(A.is_signed(codec), h, w, 1, gh, gw, seed)], axis=1).tobytes()


def _source(codec, chans, h, w, seed=0):
    return np.ascontiguousarray(_image4(A.is_signed(codec), h, w, seed)[..., :chans])


def _stats(src, dec):
    """(h, w, k) source samples and decoded samples -> the metric's sums and maxima, padded to 4."""
    d = src.astype(np.int64) - dec.astype(np.int64)
    sse, mx = np.zeros(4, np.int64), np.zeros(4, np.int64)
    sse[:d.shape[2]] = (d * d).sum(axis=(0, 1))
    mx[:d.shape[2]] = np.abs(d).max(axis=(0, 1))
    return sse, mx


@pytest.mark.parametrize("codec,chans", A.LAYOUTS)
def test_encode_every_layout_and_shape(dev, codec, chans):
    import torch
    for h, w in SHAPES:
        img = _source(codec, chans, h, w)
        stride = w * chans * 2 + PAD
        d = _to_dev(A.with_row_padding(img, PAD).tobytes(), dev)
        # the C ABI
        per = A.encoded_size(codec, h, w)
        out = torch.zeros(per + 8, dtype=torch.uint8, device=dev)
        st = pkg.lib().icamd_encode_eac11_16_device(codec, chans, h, w, h, w, stride, 1, 0, 0, d.data_ptr(), out.data_ptr(), None)
        assert st == 0
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert got[:per].tobytes() == _want(codec, h, w), (h, w)
        assert not got[per:].any()
        # the Python wrapper, from the bytes and from a 16-bit tensor
        got = pkg.encode_eac11_16_device(codec, d, h, w, chans, row_stride_bytes=stride)
        tight = pkg.encode_eac11_16_device(codec, _samples_to_dev(img, dev), h, w, chans)
        torch.cuda.synchronize()
        assert got.cpu().numpy().tobytes() == _want(codec, h, w) == tight.cpu().numpy().tobytes(), (h, w)


@pytest.mark.parametrize("h,w,gh,gw", PADDED)
def test_encode_padded_grid(dev, h, w, gh, gw):
    import torch
    for codec, chans in A.LAYOUTS:
        got = pkg.encode_eac11_16_device(codec, _samples_to_dev(_source(codec, chans, h, w), dev), h, w, chans, grid_height=gh,
                                         grid_width=gw)
        torch.cuda.synchronize()
        assert got.cpu().numpy().tobytes() == _want(codec, h, w, gh, gw), (codec, chans)


@pytest.mark.parametrize("codec,chans", [(R11, 1), (SR11, 3), (RG11, 2), (SRG11, 4)])
def test_encode_batch_with_image_stride_and_even_offset(dev, codec, chans):
    # 3 images of 37 x 70, each in a slot larger than the image, the batch starting 6 bytes into the buffer and the output 3
    import torch
    h, w, n = 37, 70, 3
    stride = w * chans * 2 + PAD
    slot = h * stride + 30
    buf = np.zeros(6 + n * slot, np.uint8)
    for i in range(n):
        buf[6 + i * slot:6 + i * slot + h * stride] = A.with_row_padding(_source(codec, chans, h, w, seed=i), PAD)
    d = _to_dev(buf.tobytes(), dev)
    per = A.encoded_size(codec, h, w)
    out = torch.zeros(3 + n * per + 5, dtype=torch.uint8, device=dev)
    st = pkg.lib().icamd_encode_eac11_16_device(codec, chans, h, w, h, w, stride, n, slot, per, d.data_ptr() + 6,
                                                out.data_ptr() + 3, None)
    assert st == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert not got[:3].any() and not got[3 + n * per:].any()
    for i in range(n):
        assert got[3 + i * per:3 + (i + 1) * per].tobytes() == _want(codec, h, w, seed=i), i


@functools.lru_cache(maxsize=None)
def _vote_plane(signed, odd_one_flat):
    """64 x 16 pixels = one wave of 16 x 4 blocks.  odd_one_flat False: every block flat but one noisy block; True: the
    mirror, one flat block among noisy ones.  Returns the plane and its words."""
    g = np.random.Generator(np.random.PCG64(T.SEED0 + 9800 + int(signed)))
    lo, hi = (-32768, 32767) if signed else (0, 65535)
    h, w = 16, 64
    flat = g.integers(lo, hi + 1, (4, 16)).repeat(4, 0).repeat(4, 1)
    noisy = g.integers(lo, hi + 1, (h, w))
    odd = np.zeros((h, w), bool)
    odd[8:12, 36:40] = True  # block (2, 9): lane 41
    plane = np.where(odd ^ odd_one_flat, noisy, flat).astype(np.int16 if signed else np.uint16)
    return plane, A.channel_words(plane, h, w, signed)


@pytest.mark.parametrize("codec", [R11, SR11])
@pytest.mark.parametrize("odd_one_flat", [False, True])
def test_wave_vote_with_one_lane_that_disagrees(dev, codec, odd_one_flat):
    # flat blocks reach sse 0 on the first candidates: the wave may leave the search only when EVERY lane has, so the one
    # noisy block still gets its full search (and one flat block among noisy ones changes nothing for them)
    import torch
    plane, words = _vote_plane(A.is_signed(codec), odd_one_flat)
    got = pkg.encode_eac11_16_device(codec, _samples_to_dev(plane, dev), 16, 64, 1)
    torch.cuda.synchronize()
    got = got.cpu().numpy().reshape(-1, 8)
    assert got.tobytes() == words.tobytes()
    # the odd block is block 2 * 16 + 9
    sse = A.search(A.targets(plane[8:12, 36:40].T.reshape(1, 16), A.is_signed(codec)), A.is_signed(codec))[1][0]
    assert (sse == 0) == odd_one_flat


def test_rg_searches_vote_per_channel(dev):
    # R flat and G noisy in every block of a wave (and the reverse in the next block row): R's early exit must not cut G's search
    import torch
    g = np.random.Generator(np.random.PCG64(T.SEED0 + 9810))
    h, w = 16, 64
    img = np.empty((h, w, 2), np.uint16)
    img[..., 0] = g.integers(0, 65536, (4, 16)).repeat(4, 0).repeat(4, 1)
    img[..., 1] = g.integers(0, 65536, (h, w))
    img[4:8] = img[4:8, :, ::-1]
    got = pkg.encode_eac11_16_device(RG11, _samples_to_dev(img, dev), h, w, 2)
    torch.cuda.synchronize()
    assert got.cpu().numpy().tobytes() == A.oracle_encode(RG11, img, h, w, 2)


@pytest.mark.parametrize("codec", A.CODECS)
def test_decode_random_words_into_padded_rows(dev, codec):
    import torch
    for i, (h, w) in enumerate(SHAPES):
        words = A.random_words(codec, h, w, seed=900 + i)
        got = pkg.decode_eac11_16_device(codec, _to_dev(words, dev), h, w, padding_bytes_per_row=PAD)
        torch.cuda.synchronize()
        assert got.dtype == (torch.int16 if A.is_signed(codec) else torch.uint16)
        got = got.cpu().view(torch.int16).numpy().view(A.sample_dtype(codec))
        assert (got.reshape(h, -1) == A.oracle_decode(codec, words, h, w, PAD)).all(), (h, w)


@pytest.mark.parametrize("codec", A.CODECS)
def test_decode_through_the_c_abi_leaves_the_padding_alone(dev, codec):
    import torch
    h, w, n = 9, 10, 2
    k = A.comps_out(codec)
    row = w * k * 2 + PAD
    slot = h * row + 10
    per = A.encoded_size(codec, h, w) + 24  # the block streams 24 bytes further apart than their size
    words = [A.random_words(codec, h, w, seed=950 + i) for i in range(n)]
    d = _to_dev(b"\0" + b"".join(wd + bytes(24) for wd in words), dev)  # the blocks at an odd address
    out = torch.full((2 + n * slot,), 0x5a, dtype=torch.uint8, device=dev)
    st = pkg.lib().icamd_decode_eac11_16_device(codec, h, w, PAD, n, per, slot, d.data_ptr() + 1, out.data_ptr() + 2, None)
    assert st == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for i in range(n):
        rows = got[2 + i * slot:2 + i * slot + h * row].reshape(h, row)
        assert (rows[:, w * k * 2:] == 0x5a).all()
        want = A.oracle_decode(codec, words[i], h, w)
        assert (np.ascontiguousarray(rows[:, :w * k * 2]).view(A.sample_dtype(codec)) == want).all(), i
        assert (got[2 + i * slot + h * row:2 + (i + 1) * slot] == 0x5a).all()


@pytest.mark.parametrize("codec,chans", A.LAYOUTS)
def test_decode_of_encode_and_metric_agree(dev, codec, chans):
    import torch
    k = A.comps_out(codec)
    for h, w in SHAPES[1:5]:
        img = _source(codec, chans, h, w)
        stride = w * chans * 2 + PAD
        d_src = _to_dev(A.with_row_padding(img, PAD).tobytes(), dev)
        blocks = pkg.encode_eac11_16_device(codec, d_src, h, w, chans, row_stride_bytes=stride)
        sse, mx = pkg.measure_error_eac11_16_device(codec, d_src, blocks.reshape(-1), h, w, chans, row_stride_bytes=stride)
        dec = pkg.decode_eac11_16_device(codec, blocks.reshape(-1), h, w)
        torch.cuda.synchronize()
        want = A.oracle_decode(codec, blocks.cpu().numpy().tobytes(), h, w).reshape(h, w, k)
        got = dec.cpu().view(torch.int16).numpy().view(A.sample_dtype(codec)).reshape(h, w, k)
        assert (got == want).all(), (h, w)
        if A.is_signed(codec):
            assert (np.frombuffer(blocks.cpu().numpy().tobytes(), np.uint8).reshape(-1, 8)[:, 0] != 0x80).all()
        want_sse, want_max = _stats(img[..., :k], want)
        assert (sse[0].cpu().numpy() == want_sse).all() and (mx[0].cpu().numpy() == want_max).all(), (h, w)


@pytest.mark.parametrize("codec,chans", [(R11, 1), (SR11, 4), (RG11, 2), (SRG11, 3)])
def test_metric_on_a_padded_grid_and_a_batch(dev, codec, chans):
    # per image of a batch, counting only the pixels inside the image; the largest differences the format allows (the image
    # generator's blocks of range extremes next to noise) included
    import torch
    h, w, gh, gw, n = 30, 30, 40, 48, 3
    k, bb = A.comps_out(codec), A.block_bytes(codec)
    imgs = np.stack([_source(codec, chans, h, w, seed=60 + i) for i in range(n)])
    d = _samples_to_dev(imgs, dev)
    blocks = pkg.encode_eac11_16_device(codec, d, h, w, chans, grid_height=gh, grid_width=gw, n_images=n)
    sse, mx = pkg.measure_error_eac11_16_device(codec, d, blocks.reshape(-1), h, w, chans, grid_height=gh, grid_width=gw,
                                                n_images=n)
    torch.cuda.synchronize()
    for i in range(n):
        grid = np.frombuffer(blocks[i].cpu().numpy().tobytes(), np.uint8).reshape((gh + 3) // 4, (gw + 3) // 4, bb)
        own = grid[:(h + 3) // 4, :(w + 3) // 4].tobytes()
        want_sse, want_max = _stats(imgs[i][..., :k], A.oracle_decode(codec, own, h, w).reshape(h, w, k))
        assert (sse[i].cpu().numpy() == want_sse).all() and (mx[i].cpu().numpy() == want_max).all(), i


def test_metric_of_arbitrary_words_reaches_the_largest_difference(dev):
    # random words against a source of range extremes: differences up to 65535, squared below 2^32, summed in 64 bits
    import torch
    h, w = 61, 59
    for codec in (RG11, SRG11):
        lo, hi = (-32768, 32767) if A.is_signed(codec) else (0, 65535)
        g = np.random.Generator(np.random.PCG64(T.SEED0 + 9820))
        img = np.where(g.integers(0, 2, (h, w, 2)) == 1, hi, lo).astype(A.sample_dtype(codec))
        words = A.random_words(codec, h, w, seed=970)
        sse, mx = pkg.measure_error_eac11_16_device(codec, _samples_to_dev(img, dev), _to_dev(words, dev), h, w, 2)
        torch.cuda.synchronize()
        want_sse, want_max = _stats(img, A.oracle_decode(codec, words, h, w).reshape(h, w, 2))
        assert want_sse.max() > 1 << 40 and want_max.max() >= 65534
        assert (sse[0].cpu().numpy() == want_sse).all() and (mx[0].cpu().numpy() == want_max).all()


def test_ramp_quality_condition_by_the_device_metric(dev):
    # the 16-bit sse of the new encode is at most 1/4 of the existing route's (source >> 8, icamd_encode_device(EAC_R11)),
    # both measured by the device metric on device-encoded blocks; every ramp block chooses multiplier 0
    import torch
    plane = A.ramp()
    d16 = _samples_to_dev(plane, dev)
    new = pkg.encode_eac11_16_device(R11, d16, 64, 64, 1)
    old = pkg.encode_device(pkg.EAC_R11, _to_dev((plane >> 8).astype(np.uint8).tobytes(), dev), 64, 64, 1)
    sse_new, _ = pkg.measure_error_eac11_16_device(R11, d16, new.reshape(-1), 64, 64, 1)
    sse_old, _ = pkg.measure_error_eac11_16_device(R11, d16, old.reshape(-1), 64, 64, 1)
    torch.cuda.synchronize()
    a, b = int(sse_new[0, 0]), int(sse_old[0, 0])
    print("ramp: 16-bit sse new", a, "existing route", b, "ratio", a / b)
    assert a == A.sse16(plane, np.frombuffer(new.cpu().numpy().tobytes(), np.uint8).reshape(-1, 8))
    assert 4 * a <= b
    assert ((new.cpu().numpy().reshape(-1, 8)[:, 1] >> 4) == 0).all()
    assert pkg.psnr16_from_stats(sse_new[0].cpu().numpy(), 64 * 64, 1) > pkg.psnr16_from_stats(sse_old[0].cpu().numpy(), 64 * 64, 1)


def test_encode_decode_and_metric_under_stream_capture(dev):
    # one encode + decode + metric captured into a graph (a single chain of nodes: no parallel branches), replayed once
    import torch
    codec, chans, h, w = SRG11, 2, 61, 59
    img = _source(codec, chans, h, w)
    src = _samples_to_dev(img, dev)
    per = A.encoded_size(codec, h, w)
    blocks = torch.zeros((1, per), dtype=torch.uint8, device=dev)
    pixels = torch.zeros(h * w * 4, dtype=torch.uint8, device=dev)
    stats = torch.zeros((1, 48), dtype=torch.uint8, device=dev)
    lib = pkg.lib()

    def run(stream):
        s = ctypes.c_void_p(stream)
        assert lib.icamd_encode_eac11_16_device(codec, chans, h, w, h, w, w * 4, 1, 0, 0, src.data_ptr(), blocks.data_ptr(), s) == 0
        assert lib.icamd_decode_eac11_16_device(codec, h, w, 0, 1, 0, 0, blocks.data_ptr(), pixels.data_ptr(), s) == 0
        assert lib.icamd_measure_error_eac11_16_device(codec, chans, h, w, h, w, w * 4, 1, 0, 0, src.data_ptr(), blocks.data_ptr(),
                                                       stats.data_ptr(), s) == 0

    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # (the kernels' first launch loads their code: not under capture)
        run(s.cuda_stream)
    s.synchronize()
    first = (blocks.cpu().numpy().tobytes(), pixels.cpu().numpy().tobytes(), stats.cpu().numpy().tobytes())
    blocks.zero_()
    pixels.zero_()
    stats.fill_(0xff)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            run(torch.cuda.current_stream().cuda_stream)
    graph.replay()
    torch.cuda.synchronize()
    want = _want(codec, h, w)
    assert blocks.cpu().numpy().tobytes() == want == first[0]
    dec = A.oracle_decode(codec, want, h, w)
    assert pixels.cpu().numpy().tobytes() == dec.tobytes() == first[1]
    assert stats.cpu().numpy().tobytes() == first[2]
    want_sse, want_max = _stats(img, dec.reshape(h, w, 2))
    rec = stats.cpu().numpy().reshape(-1)
    assert (rec[:32].view(np.int64) == want_sse).all() and (rec[32:].view(np.int32) == want_max).all()
