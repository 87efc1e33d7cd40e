"""Writes tests/golden/bc1a_bc2_decode_kat.bin: BC1 and BC2 blocks with the texels an INDEPENDENT decoder gives them (Pillow's DDS
reader, through FourCC DXT1 -- which it reads as RGBA, with the transparent index -- and FourCC DXT3).  Layout: "BC1A2KAT", uint32
n, uint32 m, n 8-byte BC1 blocks, n x 64 expected bytes, m 16-byte BC2 blocks, m x 64 expected bytes (texel i = 4 y + x, R G B A).
From a fixed seed:

* BC1: 256 blocks, a quarter each as drawn, forced to c0 == c1, to c0 < c1 (with every index in the block) and to c0 > c1;
* BC2: 256 blocks with random alpha words, their colour words drawn the same way -- so half of them have c0 <= c1 and must still
  decode in four-colour mode.

tests/bc1a_bc2_oracle.py must agree with Pillow on every byte before anything is written.  Run from the repository root:
    python tests/golden/make_bc1a_bc2_golden.py"""
import io
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bc1a_bc2_oracle as O  # noqa: E402

SEED = 0xBC1A
N_BC1 = N_BC2 = 256


def dds(fourcc, h, w, blocks, flags=0x4):
    """A legacy DDS file (no DX10 header) around a block stream."""
    head = b"DDS " + struct.pack("<7I", 124, 0x1 | 0x2 | 0x4 | 0x1000 | 0x80000, h, w, len(blocks), 0, 1) + bytes(44) + \
        struct.pack("<2I4s5I", 32, flags, fourcc, 0, 0, 0, 0, 0) + struct.pack("<5I", 0x1000, 0, 0, 0, 0)
    assert len(head) == 128
    return head + blocks


def pillow_decode(fourcc, blocks, size):
    """[n, 64] uint8: the texels Pillow decodes for n blocks (laid out as a 4-row image)."""
    from PIL import Image
    n = len(blocks) // size
    im = Image.open(io.BytesIO(dds(fourcc, 4, 4 * n, blocks)))
    im.load()
    return np.asarray(im.convert("RGBA")).reshape(4, n, 4, 4).transpose(1, 0, 2, 3).reshape(n, 64)


def main():
    bc1 = O.random_bc1_blocks(N_BC1, SEED)
    bc2 = O.random_bc2_blocks(N_BC2, SEED + 16)
    c0, c1, idx = O.colour_words(bc1)
    assert (c0 == c1).sum() >= N_BC1 // 4 and (c0 < c1).sum() >= N_BC1 // 4 and (c0 > c1).sum() >= N_BC1 // 4
    assert all(((idx == k) & (c0 < c1)[:, None]).any() for k in range(4))
    d0, d1, _ = O.colour_words(bc2[:, 8:])
    assert (d0 <= d1).sum() >= N_BC2 // 4 and (d0 > d1).sum() >= N_BC2 // 4
    want1 = pillow_decode(b"DXT1", bc1.tobytes(), 8)
    want2 = pillow_decode(b"DXT3", bc2.tobytes(), 16)
    assert (O.decode_bc1a_blocks(bc1).reshape(-1, 64) == want1).all(), "bc1a_bc2_oracle disagrees with Pillow on BC1"
    assert (O.decode_bc2_blocks(bc2).reshape(-1, 64) == want2).all(), "bc1a_bc2_oracle disagrees with Pillow on BC2"
    with open(O.GOLDEN, "wb") as f:
        f.write(b"BC1A2KAT" + struct.pack("<2I", N_BC1, N_BC2))
        f.write(bc1.tobytes() + want1.tobytes() + bc2.tobytes() + want2.tobytes())
    print("wrote %s: %d + %d blocks, %d bytes" % (O.GOLDEN, N_BC1, N_BC2, os.path.getsize(O.GOLDEN)))


if __name__ == "__main__":
    main()
