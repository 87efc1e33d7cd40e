"""Writes tests/golden/bc7_decode_kat.bin: BC7 blocks with the texels an INDEPENDENT decoder gives them (Pillow's DDS reader, through
a DX10 DDS header), 80-byte records of 16 block bytes + 64 expected bytes (texel i = 4 y + x, R G B A).  From a fixed seed:

* every (mode, partition) cell of modes 0 (16 partitions) and 1, 2, 3, 7 (64 each): two blocks, remaining bits random;
* mode 4: every rotation x index-selection pair; mode 5: every rotation; 32 mode-6 blocks;
* per mode one block whose bits after the mode bit are all ones;
* four reserved blocks (byte 0 = 0, the rest random): expected all zero by the specification, whatever Pillow does there.

tests/bc7_oracle.py must agree on every block before anything is written.  Run from the repository root:
    python tests/golden/make_bc7_golden.py"""
import io
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bc7_oracle as B  # noqa: E402

SEED = 0xBC7
OUT = os.path.join(HERE, "bc7_decode_kat.bin")


def dx10_dds(blocks, h, w):
    """A DDS file with the DX10 extension header (dxgiFormat 98) around a BC7 block stream."""
    head = b"DDS " + struct.pack("<7I", 124, 0x1 | 0x2 | 0x4 | 0x1000 | 0x80000, h, w, len(blocks), 0, 1) + bytes(44) + \
        struct.pack("<2I4s5I", 32, 0x4, b"DX10", 0, 0, 0, 0, 0) + struct.pack("<5I", 0x1000, 0, 0, 0, 0) + \
        struct.pack("<5I", 98, 3, 0, 1, 0)
    assert len(head) == 148
    return head + blocks


def pillow_decode(blocks):
    """[n, 16, 4] uint8: the texels Pillow decodes for n BC7 blocks (laid out as a 4-row image)."""
    from PIL import Image
    n = len(blocks) // 16
    im = Image.open(io.BytesIO(dx10_dds(blocks, 4, 4 * n)))
    im.load()
    return np.asarray(im.convert("RGBA")).reshape(4, n, 4, 4).transpose(1, 0, 2, 3).reshape(n, 16, 4)


def fixture_blocks():
    g = np.random.Generator(np.random.PCG64(SEED))
    blocks = []
    for mode in (0, 1, 2, 3, 7):
        for part in range(1 << B.MODES[mode][1]):
            blocks += [B.random_block(g, mode, partition=part) for _ in range(2)]
    blocks += [B.random_block(g, 4, rotation=r, sel=s) for r in range(4) for s in range(2)]
    blocks += [B.random_block(g, 5, rotation=r) for r in range(4)]
    blocks += [B.random_block(g, 6) for _ in range(32)]
    blocks += [B.random_block(g, mode, ones=True) for mode in range(8)]
    n_decoded = len(blocks)
    blocks += [B.random_block(g, 8) for _ in range(4)]
    return b"".join(blocks), n_decoded


def main():
    blocks, n_decoded = fixture_blocks()
    n = len(blocks) // 16
    assert n == 2 * (16 + 4 * 64) + 8 + 4 + 32 + 8 + 4
    want = np.zeros((n, 16, 4), np.uint8)
    want[:n_decoded] = pillow_decode(blocks[:16 * n_decoded])
    mine = B.decode_blocks(blocks)
    bad = [i for i in range(n) if not (mine[i] == want[i]).all()]
    assert not bad, "bc7_oracle.decode disagrees on blocks %s" % bad[:8]
    rec = np.concatenate([np.frombuffer(blocks, np.uint8).reshape(n, 16), want.reshape(n, 64)], axis=1)
    with open(OUT, "wb") as f:
        f.write(rec.tobytes())
    print("wrote %s: %d blocks, %d bytes" % (OUT, n, rec.size))


if __name__ == "__main__":
    main()
