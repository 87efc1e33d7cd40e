"""GPU tier for BC6H (include/ic_amd.h icamd_encode_bc6h_device): the HIP kernels through the C ABI and the Python wrappers.  The
decoder against the two committed fixtures (what an independent decoder makes of the blocks) and the numpy restatement, the
encoder byte for byte against the numpy definition, the metric against numpy on the oracle's decode (tests/bc6h_oracle.py).
The definition's blocks of a test image are computed once and shared by every layout that reads the image."""
import functools
import importlib
import struct

import numpy as np
import pytest

import bc6h_oracle as B

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("image-compression_amd")
UF16, SF16 = B.BC6H_UF16, B.BC6H_SF16
SHAPES = [(1, 1), (4, 4), (5, 3), (9, 2), (61, 59)]
PAD = 6  # bytes of row padding
PADDED = [(5, 3, 16, 16), (30, 30, 40, 48)]
KAT = B.__file__.replace("bc6h_oracle.py", "golden/bc6h_decode_kat.bin")
BITS = B.__file__.replace("bc6h_oracle.py", "golden/bc6h_bits_kat.bin")


@pytest.fixture(scope="module")
def dev():
    import torch
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


def _codec(signed):
    return SF16 if signed else UF16


def _to_dev(buf, dev):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(buf), np.uint8).copy()).to(dev)


def _halves_to_dev(arr, dev, dtype=None):
    """A numpy uint16 array of half bits as a device tensor of `dtype` (default torch.float16) over the same bits."""
    import torch
    return _to_dev(np.ascontiguousarray(arr).tobytes(), dev).view(dtype or torch.float16)


def _rows(img, pad):
    h, w, chans = img.shape
    rows = np.zeros((h, w * chans + pad // 2), np.uint16)
    rows[:, :w * chans] = img.reshape(h, w * chans)
    return rows


@functools.lru_cache(maxsize=None)
def _image(name, h, w, seed=0):
    img = B.content(name, h, w, 4, seed)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _want(name, h, w, signed, gh=None, gw=None, seed=0):
    return B.oracle_encode(_image(name, h, w, seed), signed, gh, gw)  # (the fourth sample is not read: one answer for 3 and 4)


def _source(name, h, w, chans, seed=0):
    return np.ascontiguousarray(_image(name, h, w, seed)[..., :chans])


# ---- decoder

def _decode_as_row(dev, blocks, signed):
    """n blocks as a 4-row image through the device decoder -> [n, 16, 3] uint16 half bits."""
    import torch
    n = len(blocks) // 16
    out = pkg.decode_bc6h_device(_codec(signed), _to_dev(blocks, dev), 4, 4 * n)
    torch.cuda.synchronize()
    rows = out.view(torch.int16).cpu().numpy().view(np.uint16).reshape(4, n, 4, 4)
    assert (rows[..., 3] == 0x3C00).all()
    return rows.transpose(1, 0, 2, 3).reshape(n, 16, 4)[..., :3]


@pytest.mark.parametrize("signed", [False, True])
def test_decode_both_fixtures(dev, signed):
    rec = np.fromfile(KAT, np.uint8).reshape(-1, 65)
    raw = open(BITS, "rb").read()
    n_partners, n_cells = struct.unpack_from("<2I", raw)
    partners = np.frombuffer(raw, np.uint8, n_partners * 65, 8).reshape(n_partners, 65)
    cells = np.frombuffer(raw, np.uint8, n_cells * 27, 8 + n_partners * 65).reshape(n_cells, 27)
    for r in (rec[rec[:, 16] == int(signed)], partners[partners[:, 16] == int(signed)]):
        got = B.half_to_byte(_decode_as_row(dev, r[:, :16].tobytes(), signed)).reshape(-1, 48)
        bad = np.flatnonzero((got != r[:, 17:]).any(axis=1))
        assert len(bad) == 0, bad[:8]
    c = cells[cells[:, 16] == int(signed)]
    assert len(c) == 1728
    blocks = c[:, :16].tobytes()
    half = _decode_as_row(dev, blocks, signed)
    got = B.half_to_byte(half).reshape(-1, 48)
    bad = [i for i in range(len(c)) if B.digest(got[i]) != bytes(c[i, 19:])]
    assert not bad, bad[:8]
    assert (half == B.decode_blocks(blocks, signed)).all()  # and in half bits, which is finer than the fixture


@pytest.mark.parametrize("signed", [False, True])
def test_decode_clipped_with_row_padding_and_as_a_batch(dev, signed):
    import torch
    h, w, n = 61, 59, 3
    per = B.encoded_size(h, w)
    streams = [B.stratified_blocks(per // 16, 40 + i) for i in range(n)]
    for pad in (0, PAD):
        out = pkg.decode_bc6h_device(_codec(signed), _to_dev(streams[0], dev), h, w, padding_bytes_per_row=pad)
        torch.cuda.synchronize()
        got = out.view(torch.int16).cpu().numpy().view(np.uint16).reshape(h, -1)
        assert (got == B.decode(streams[0], h, w, signed, pad)).all(), pad  # (the padding samples stay zero)
    # a batch of three in oversized slots, pixels starting 2 bytes into their buffer; what lies between is left alone
    stride = w * 8 + PAD
    slot_in, slot_out = per + 48, h * stride + 34
    src = np.zeros(n * slot_in, np.uint8)
    for i in range(n):
        src[i * slot_in:i * slot_in + per] = np.frombuffer(streams[i], np.uint8)
    out = torch.full((2 + n * slot_out,), 0xA5, dtype=torch.uint8, device=dev)
    st = pkg.lib().icamd_decode_bc6h_device(_codec(signed), h, w, PAD, n, slot_in, slot_out, _to_dev(src, dev).data_ptr(),
                                            out.data_ptr() + 2, None)
    assert st == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:2] == 0xA5).all()
    for i in range(n):
        s = got[2 + i * slot_out:2 + (i + 1) * slot_out]
        rows = s[:h * stride].reshape(h, stride)
        want = B.decode(streams[i], h, w, signed)
        assert (rows[:, :w * 8].copy().view(np.uint16) == want).all(), i
        assert (rows[:, w * 8:] == 0xA5).all() and (s[h * stride:] == 0xA5).all()


# ---- encoder

@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("chans", [3, 4])
def test_encode_every_shape_and_content(dev, signed, chans):
    import torch
    codec = _codec(signed)
    for h, w in SHAPES:
        for name in B.CONTENTS:
            img = _source(name, h, w, chans)
            want = _want(name, h, w, signed)
            stride = w * chans * 2 + PAD
            d = _to_dev(_rows(img, PAD).tobytes(), dev)
            per = B.encoded_size(h, w)
            out = torch.zeros(per + 8, dtype=torch.uint8, device=dev)
            st = pkg.lib().icamd_encode_bc6h_device(codec, chans, h, w, h, w, stride, 1, 0, 0, d.data_ptr(), out.data_ptr(), None)
            assert st == 0
            tight = pkg.encode_bc6h_device(codec, _halves_to_dev(img, dev), h, w, chans)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert got[:per].tobytes() == want == tight.cpu().numpy().tobytes(), (name, h, w)
            assert not got[per:].any()


@pytest.mark.parametrize("h,w,gh,gw", PADDED)
def test_encode_padded_grid(dev, h, w, gh, gw):
    import torch
    for signed in (False, True):
        for chans in (3, 4):
            for name in ("noise", "specials", "gradient"):
                got = pkg.encode_bc6h_device(_codec(signed), _halves_to_dev(_source(name, h, w, chans), dev), h, w, chans,
                                             grid_height=gh, grid_width=gw)
                torch.cuda.synchronize()
                assert got.cpu().numpy().tobytes() == _want(name, h, w, signed, gh, gw), (signed, chans, name)


@pytest.mark.parametrize("signed", [False, True])
def test_encode_wide_grid_runs_both_tile_forms(dev, signed):
    # 520 block columns: two 256 x 1-block tiles and a clipped third per block row (the wide kernel); the shapes above are narrow
    import torch
    h, w = 8, 2080
    for chans, name in ((3, "noise"), (4, "exponents")):
        got = pkg.encode_bc6h_device(_codec(signed), _halves_to_dev(_source(name, h, w, chans), dev), h, w, chans)
        torch.cuda.synchronize()
        assert got.cpu().numpy().tobytes() == _want(name, h, w, signed), (chans, name)


@pytest.mark.parametrize("signed,chans", [(False, 3), (True, 4)])
def test_encode_batch_with_image_stride_and_even_offset(dev, signed, chans):
    # 3 images of 37 x 70, each in a slot larger than the image, the batch starting 6 bytes into the buffer and the output 3
    import torch
    h, w, n = 37, 70, 3
    stride = w * chans * 2 + PAD
    slot = h * stride + 30
    buf = np.zeros(6 + n * slot, np.uint8)
    for i in range(n):
        buf[6 + i * slot:6 + i * slot + h * stride] = _rows(_source("noise", h, w, chans, seed=i), PAD).view(np.uint8).reshape(-1)
    d = _to_dev(buf, dev)
    per = B.encoded_size(h, w)
    out = torch.zeros(3 + n * per + 5, dtype=torch.uint8, device=dev)
    st = pkg.lib().icamd_encode_bc6h_device(_codec(signed), chans, h, w, h, w, stride, n, slot, per, d.data_ptr() + 6,
                                            out.data_ptr() + 3, None)
    assert st == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert not got[:3].any() and not got[3 + n * per:].any()
    for i in range(n):
        assert got[3 + i * per:3 + (i + 1) * per].tobytes() == _want("noise", h, w, signed, seed=i), i


def test_every_accepted_tensor_dtype(dev):
    import torch
    h, w = 9, 14
    img = _source("gradient", h, w, 3)
    want = _want("gradient", h, w, False)
    blocks = _to_dev(want, dev)
    ref = None
    for dtype in (torch.float16, torch.int16, torch.uint16, torch.uint8):
        t = _halves_to_dev(img, dev, dtype)
        got = pkg.encode_bc6h_device(UF16, t, h, w, 3)
        stats = pkg.measure_error_bc6h_device(UF16, t, blocks, h, w, 3)
        torch.cuda.synchronize()
        assert got.cpu().numpy().tobytes() == want, dtype
        s = (stats[0].cpu().numpy().tolist(), stats[1].cpu().numpy().tolist())
        ref = ref or s
        assert s == ref, dtype
    dec = pkg.decode_bc6h_device(UF16, blocks, h, w)
    assert dec.dtype == torch.float16 and dec.shape == (1, h * w * 4)
    assert pkg.psnr_bc6h_from_stats(np.array(ref[0]), h * w) > 40


# ---- metric

def _metric_want(img, blocks, signed, gw=None):
    sse, mx = B.metric(img, blocks, signed, gw)
    return list(sse) + [0], list(mx) + [0]


@pytest.mark.parametrize("signed", [False, True])
def test_metric_matches_numpy_on_the_oracles_decode(dev, signed):
    import torch
    codec = _codec(signed)
    for (h, w, gh, gw) in [(61, 59, 61, 59), (5, 3, 16, 16), (30, 30, 40, 48), (128, 260, 128, 260)]:
        for chans, name in ((3, "noise"), (4, "gradient")):
            img = _source(name, h, w, chans)
            # the encoder's own blocks in the first rows, blocks of every mode in the rest
            blocks = np.frombuffer(B.stratified_blocks(B.encoded_size(gh, gw) // 16, h + chans), np.uint8).copy()
            enc = np.frombuffer(_want(name, h, w, signed, gh, gw), np.uint8)
            blocks[:len(enc) // 2] = enc[:len(enc) // 2]
            sse, mx = pkg.measure_error_bc6h_device(codec, _halves_to_dev(img, dev), _to_dev(blocks, dev), h, w, chans,
                                                    grid_height=gh, grid_width=gw)
            torch.cuda.synchronize()
            want = _metric_want(img, blocks.tobytes(), signed, gw)
            assert (sse.cpu().numpy()[0].tolist(), mx.cpu().numpy()[0].tolist()) == want, (h, w, chans)


@pytest.mark.parametrize("signed", [False, True])
def test_metric_batch_of_small_images_with_strides(dev, signed):
    # 5 images of 9 x 14 (12 blocks each: the lanes of one wave hold blocks of several images), slots larger than the data
    import torch
    h, w, n, chans = 9, 14, 5, 4
    stride = w * chans * 2 + PAD
    slot, per = h * stride + 10, B.encoded_size(h, w)
    bslot = per + 16
    src = np.zeros(n * slot, np.uint8)
    blk = np.zeros(n * bslot, np.uint8)
    want = []
    for i in range(n):
        img = _source("specials" if i % 2 else "noise", h, w, chans, seed=i)
        src[i * slot:i * slot + h * stride] = _rows(img, PAD).view(np.uint8).reshape(-1)
        b = B.stratified_blocks(per // 16, 90 + i)
        blk[i * bslot:i * bslot + per] = np.frombuffer(b, np.uint8)
        want.append(_metric_want(img, b, signed))
    sse, mx = pkg.measure_error_bc6h_device(_codec(signed), _to_dev(src, dev), _to_dev(blk, dev), h, w, chans, row_stride_bytes=stride,
                                            n_images=n, src_image_stride_bytes=slot, blocks_image_stride_bytes=bslot)
    torch.cuda.synchronize()
    for i in range(n):
        assert (sse.cpu().numpy()[i].tolist(), mx.cpu().numpy()[i].tolist()) == want[i], i
