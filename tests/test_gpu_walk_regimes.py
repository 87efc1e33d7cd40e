"""GPU tier of the block-walk cases (tests/walk_cases.py): every metric kernel and every raster decoder in every regime of the
walk -- a last workgroup one block short, full and one block over, workgroups of one image other than image 0, workgroups that
span images with waves that agree, waves that hold two images, waves that hold many -- and calls of more than 2^31 - 1 blocks,
which decode_pieces / metric_pieces of csrc/ic_capi.hip cut into two launches.  tests/test_walk_cases_host.py (CPU tier) holds
each case to the regime it is named for.  Every comparison is == on integers or bytes against the oracles' decode.

A metric writes its records into the first n rows of an [n + 1, 48] tensor whose last row must keep its 0xA5.  A decoder
writes into a buffer of 0xA5 the test owns, through the C ABI: row padding, the slack between images and the sixteen bytes
after the last image must keep theirs.

The calls of more than 2^31 - 1 blocks lay 33 291 overlapping images on one strip of 250 pixels by 34 314 block rows (about
140 MB of source): image i is the 1024 block rows from block row i on.  Nothing in include/ic_amd.h forbids images that
overlap; overlapping decoded images write the same bytes to the same places."""
import importlib
import time

import numpy as np
import pytest

import walk_cases as K

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("image-compression_amd")


@pytest.fixture(scope="module")
def dev():
    import torch
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


def _to_dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(dev)


# ---- the regimes

@pytest.mark.parametrize("F", K.METRIC_FAMILIES, ids=[F.name for F in K.METRIC_FAMILIES])
def test_metric_in_every_regime(dev, F):
    import torch
    for regime in K.regimes(F):
        L = K.layout(F, regime)
        src, blk = _to_dev(K.source_buffer(F, regime), dev), _to_dev(K.blocks_buffer(F, regime), dev)
        records = torch.full((L.n + 1, pkg.ERROR_STATS_BYTES), K.CANARY, dtype=torch.uint8, device=dev)
        got = K.measure(pkg, F, regime, src[L.pixel_lead:], blk[L.blocks_lead:], records[:L.n])
        assert got is not None, (F.name, regime.name)
        torch.cuda.synchronize()
        sse, mx = got[0].cpu().numpy().astype(np.int64), got[1].cpu().numpy().astype(np.int64)
        want_sse, want_mx = K.want_metric(F, regime)
        bad = np.flatnonzero((sse != want_sse).any(axis=1) | (mx != want_mx).any(axis=1))
        if len(bad):
            i = int(bad[0])
            pytest.fail("%s, %s: %d of %d records differ, first image %d: sse %s max_abs %s, expected %s %s"
                        % (F.name, regime.name, len(bad), L.n, i, sse[i].tolist(), mx[i].tolist(), want_sse[i].tolist(),
                           want_mx[i].tolist()))
        assert bool((records[L.n] == K.CANARY).all()), (F.name, regime.name, "the record after the last image was written")


@pytest.mark.parametrize("F", K.DECODE_FAMILIES, ids=[F.name for F in K.DECODE_FAMILIES])
def test_decode_in_every_regime(dev, F):
    import torch
    for regime in K.regimes(F):
        L = K.layout(F, regime)
        start, want = K.decode_output(F, regime)
        blk, out = _to_dev(K.blocks_buffer(F, regime), dev), _to_dev(start, dev)
        assert K.decode(pkg, F, regime, blk[L.blocks_lead:], out[L.pixel_lead:]) == 0, (F.name, regime.name)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        bad = np.flatnonzero(got != want)
        if len(bad):
            at = int(bad[0])
            i = K.image_of_byte(F, regime, at)
            inside = at - L.pixel_lead - i * L.pixel_image_stride
            pytest.fail("%s, %s: %d bytes differ, first in image %d of %d at row %d, byte %d of the row (%d bytes of pixels a row): "
                        "0x%02x, expected 0x%02x" % (F.name, regime.name, len(bad), i, L.n, inside // L.stride, inside % L.stride,
                                                     L.w * F.pixel_bytes, got[at], want[at]))


# ---- more than 2^31 - 1 blocks in one call

def _periodic(total, piece, dev):
    """A device tensor of `total` bytes: `piece` repeated, the last repeat cut."""
    import torch
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    p = _to_dev(piece, dev)
    n = total // p.numel()
    out[:n * p.numel()].view(n, p.numel()).copy_(p.view(1, -1).expand(n, -1))
    out[n * p.numel():] = p[:total - n * p.numel()]
    return out


def _strip_blocks(F, dev):
    row_bytes = K.STRIP_COLS * K.block_bytes(F)
    return _periodic(K.STRIP_BLOCK_ROWS * row_bytes, K.strip_period_blocks(F), dev), row_bytes


@pytest.mark.parametrize("name", K.STRIP_METRICS)
def test_metric_of_more_than_2_31_blocks(dev, name):
    """33 288 images in the first launch (block indices up to 2^31 - 8 193), three in the second, which begins in the middle of
    the content's period: every record against the 5-periodic table of the CPU tier."""
    import torch
    F = K.BY_NAME[name]
    n, stride = K.STRIP_IMAGES, K.strip_source_stride(F)
    src = _periodic(K.STRIP_BLOCK_ROWS * 4 * stride, K.strip_period_source_rows(F), dev)
    blk, row_bytes = _strip_blocks(F, dev)
    records = torch.full((n + 1, pkg.ERROR_STATS_BYTES), K.CANARY, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = getattr(pkg, F.entry)(F.codec, src, blk, K.STRIP_H, K.STRIP_W, F.comps, row_stride_bytes=stride, n_images=n,
                                src_image_stride_bytes=4 * stride, blocks_image_stride_bytes=row_bytes, out=records[:n])
    assert got is not None
    torch.cuda.synchronize()
    print("%s: %d blocks in %.3f s" % (name, n * K.STRIP_BLOCKS_PER_IMAGE, time.perf_counter() - t0))
    want = _to_dev(K.strip_record_table(F), dev).view(K.STRIP_PERIOD, -1)[torch.arange(n, device=dev) % K.STRIP_PERIOD]
    bad = (records[:n] != want).any(dim=1).nonzero()
    if bad.numel():
        i = int(bad[0])
        pytest.fail("%s: %d of %d records differ, first image %d (the second launch begins at image %d): %s, expected %s"
                    % (name, bad.numel(), n, i, K.STRIP_FIRST_LAUNCH_IMAGES, records[i].cpu().numpy().tobytes().hex(),
                       want[i].cpu().numpy().tobytes().hex()))
    assert bool((records[n] == K.CANARY).all()), (name, "the record after the last image was written")


@pytest.mark.parametrize("name", K.STRIP_DECODERS)
def test_decode_of_more_than_2_31_blocks(dev, name):
    """The strip decodes to the oracle's decode of one period, repeated.  The fourth pixel row of the strip's last block row is
    written by no image (every image's last block row is clipped to three rows) and keeps its canary, as all row padding does."""
    import torch
    F = K.BY_NAME[name]
    n, stride = K.STRIP_IMAGES, K.strip_decoded_stride(F)
    blk, row_bytes = _strip_blocks(F, dev)
    size = K.STRIP_BLOCK_ROWS * 4 * stride
    out = torch.full((size + K.TAIL,), K.CANARY, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    status = K.decode_call(pkg, F, K.STRIP_H, K.STRIP_W, K.STRIP_ROW_PADDING, n, row_bytes, 4 * stride, blk, out)
    assert status == 0
    torch.cuda.synchronize()
    print("%s: %d blocks in %.3f s" % (name, n * K.STRIP_BLOCKS_PER_IMAGE, time.perf_counter() - t0))
    want = _periodic(size + K.TAIL, K.strip_period_decoded_rows(F), dev)
    want[size - stride:] = K.CANARY
    bad = (out != want).nonzero()
    if bad.numel():
        at = int(bad[0])
        row = at // stride
        pytest.fail("%s: %d bytes differ, first at pixel row %d of the strip (block row %d: the first image to write it is %d, the "
                    "second launch begins at image %d), byte %d of the row: 0x%02x, expected 0x%02x"
                    % (name, bad.numel(), row, row // 4, max(row // 4 - K.STRIP_ROWS + 1, 0), K.STRIP_FIRST_LAUNCH_IMAGES, at % stride,
                       int(out[at]), int(want[at])))
