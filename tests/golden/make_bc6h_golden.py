"""Writes the two BC6H fixtures from what an INDEPENDENT decoder (Pillow's DDS reader, DX10 header with dxgiFormat 95 = UF16 /
96 = SF16) makes of blocks drawn from a fixed seed.  Pillow hands back 8-bit RGB: byte = 0 for f < 0, 255 for f > 1, else
trunc(255 f) (bc6h_oracle.half_to_byte); that is coarse, so the second fixture proves bit by bit that it still pins the format.

tests/golden/bc6h_decode_kat.bin -- records of 65 bytes: block[16] | signed flag | the 48 bytes Pillow decodes (texel i = 4 y + x,
R G B).  Every (mode, partition) cell of the ten two-subset modes, 16 blocks per one-subset mode, per mode one block with every
bit after the mode field set, one block per reserved mode field; each block under both formats.  CONDITION (asserted; the blocks
are redrawn from the next seed until it holds): at least a fifth of the unsigned records' bytes and an eighth of the signed
records' bytes lie strictly between 0 and 255.

tests/golden/bc6h_bits_kat.bin -- the bit sweep.  uint32 n_partners, uint32 n_cells; n_partners records of 65 bytes as above; then
n_cells records of 27 bytes: block[16] | signed flag | partner index (uint16) | the first 8 bytes of SHA-256 of Pillow's 48 bytes.
A cell is (format, mode, bit above the mode field); its block is its partner with that ONE bit flipped, and Pillow's output for
the two differs.  CONDITION (asserted; the draw count per mode is doubled until it holds): NO cell is left without such a pair.
Partners are shared between cells (a greedy cover).

tests/bc6h_oracle.py must agree with Pillow on all 48 bytes of every stored block before anything is written.  Run from the
repository root:
    python tests/golden/make_bc6h_golden.py"""
import io
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bc6h_oracle as B  # noqa: E402

SEED = 0xBC6
OUT_KAT = os.path.join(HERE, "bc6h_decode_kat.bin")
OUT_BITS = os.path.join(HERE, "bc6h_bits_kat.bin")
CHUNK = 1 << 16  # blocks per Pillow image


def dx10_dds(blocks, h, w, signed):
    head = b"DDS " + struct.pack("<7I", 124, 0x1 | 0x2 | 0x4 | 0x1000 | 0x80000, h, w, len(blocks), 0, 1) + bytes(44) + \
        struct.pack("<2I4s5I", 32, 0x4, b"DX10", 0, 0, 0, 0, 0) + struct.pack("<5I", 0x1000, 0, 0, 0, 0) + \
        struct.pack("<5I", 96 if signed else 95, 3, 0, 1, 0)
    assert len(head) == 148
    return head + blocks


def pillow_decode(blocks, signed):
    """[n, 48] uint8: what Pillow decodes for n BC6H blocks (laid out as 4-row images)."""
    from PIL import Image
    blocks = bytes(blocks)
    out = []
    for at in range(0, len(blocks), 16 * CHUNK):
        part = blocks[at:at + 16 * CHUNK]
        n = len(part) // 16
        im = Image.open(io.BytesIO(dx10_dds(part, 4, 4 * n, signed)))
        im.load()
        assert im.mode == "RGB"
        out.append(np.asarray(im).reshape(4, n, 4, 3).transpose(1, 0, 2, 3).reshape(n, 48))
    return np.concatenate(out) if out else np.zeros((0, 48), np.uint8)


def oracle_bytes(blocks, signed):
    return B.half_to_byte(B.decode_blocks(bytes(blocks), signed)).reshape(-1, 48)


def records(blocks, signed):
    """65-byte records; the oracle is held to Pillow on every byte."""
    want = pillow_decode(blocks, signed)
    mine = oracle_bytes(blocks, signed)
    bad = np.flatnonzero((want != mine).any(axis=1))
    assert len(bad) == 0, "bc6h_oracle disagrees with Pillow on blocks %s (signed %d)" % (bad[:8], signed)
    b = np.frombuffer(bytes(blocks), np.uint8).reshape(-1, 16)
    return np.concatenate([b, np.full((len(b), 1), int(signed), np.uint8), want], axis=1)


def kat_blocks(seed):
    g = np.random.Generator(np.random.PCG64(seed))
    blocks = []
    for mode in range(10):
        blocks += [B.random_block(g, mode, partition=p) for p in range(32)]
    for mode in range(10, 14):
        blocks += [B.random_block(g, mode) for _ in range(16)]
    blocks += [B.random_block(g, mode, ones=True) for mode in range(14)]
    blocks += [B.random_block(g, mode) for mode in range(14, 18)]
    return b"".join(blocks)


def make_kat():
    for attempt in range(64):
        blocks = kat_blocks(SEED + attempt)
        assert len(blocks) == 16 * (320 + 64 + 14 + 4)
        recs = [records(blocks, s) for s in (False, True)]
        inner = [float(((r[:, 17:] > 0) & (r[:, 17:] < 255)).mean()) for r in recs]
        assert not recs[0][-4:, 17:].any() and not recs[1][-4:, 17:].any()  # reserved mode fields: zeros
        if inner[0] >= 1 / 5 and inner[1] >= 1 / 8:
            return np.concatenate(recs), inner, attempt
    raise AssertionError("no draw met the interior-byte condition")


def sweep_mode(g, mode, signed):
    """(partners [k, 16] uint8, cells [(bit, partner index)]) covering every bit above the mode field of `mode`."""
    mbits = B.MODES[mode][1]
    bits = list(range(mbits, 128))
    open_bits = set(bits)
    partners, cells = [], []
    draws = 1024
    while open_bits:
        cand = np.frombuffer(b"".join(B.random_block(g, mode) for _ in range(draws)), np.uint8).reshape(draws, 16)
        base = pillow_decode(cand.tobytes(), signed)
        todo = sorted(open_bits)
        visible = np.zeros((draws, len(todo)), bool)
        for j, bit in enumerate(todo):
            flipped = cand.copy()
            flipped[:, bit // 8] ^= 1 << (bit % 8)
            visible[:, j] = (pillow_decode(flipped.tobytes(), signed) != base).any(axis=1)
        while True:  # greedy cover among this draw
            live = [j for j, bit in enumerate(todo) if bit in open_bits]
            if not live:
                break
            gain = visible[:, live].sum(axis=1)
            best = int(gain.argmax())
            if gain[best] == 0:
                break
            partners.append(cand[best])
            for j in live:
                if visible[best, j]:
                    cells.append((todo[j], len(partners) - 1))
                    open_bits.discard(todo[j])
        draws *= 2
        assert draws <= 1 << 20, "mode %d: bits %s stay invisible" % (mode, sorted(open_bits))
    assert sorted(b for b, _ in cells) == bits  # zero cells without a visible pair
    return np.stack(partners), sorted(cells)


def make_bits():
    g = np.random.Generator(np.random.PCG64(SEED ^ 0xB175))
    partner_recs, cell_recs = [], []
    for signed in (False, True):
        for mode in range(14):
            partners, cells = sweep_mode(g, mode, signed)
            first = sum(len(p) for p in partner_recs)
            prec = records(partners.tobytes(), signed)
            partner_recs.append(prec)
            flipped = partners[[pi for _, pi in cells]].copy()
            for row, (bit, _) in zip(flipped, cells):
                row[bit // 8] ^= 1 << (bit % 8)
            frec = records(flipped.tobytes(), signed)
            for (bit, pi), r in zip(cells, frec):
                assert (r[17:] != prec[pi][17:]).any()
                cell_recs.append(bytes(r[:17]) + struct.pack("<H", first + pi) + B.digest(r[17:]))
    partners = np.concatenate(partner_recs)
    assert len(cell_recs) == 2 * (2 * 126 + 12 * 123)
    return struct.pack("<2I", len(partners), len(cell_recs)) + partners.tobytes() + b"".join(cell_recs), len(partners)


def main():
    kat, inner, attempt = make_kat()
    bits, n_partners = make_bits()
    with open(OUT_KAT, "wb") as f:
        f.write(kat.tobytes())
    with open(OUT_BITS, "wb") as f:
        f.write(bits)
    print("wrote %s: %d records, %d bytes; interior bytes %.3f unsigned, %.3f signed (seed + %d)"
          % (OUT_KAT, len(kat), kat.size, inner[0], inner[1], attempt))
    print("wrote %s: %d partners, %d bytes" % (OUT_BITS, n_partners, len(bits)))


if __name__ == "__main__":
    main()
