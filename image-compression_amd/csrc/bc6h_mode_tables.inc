/* BC6H (BPTC float) mode layouts, typed from the BPTC specification (ARB_texture_compression_bptc, "Block descriptions for
 * floating-point formats"; Direct3D 11 "BC6H format", mode table).  DATA ONLY: csrc/bc6h_block.h packs these rows at compile time
 * for the kernels and for their host twin, so there is one table; tests/bc6h_oracle.py states the layouts a second time, and
 * tests/test_bc6h_host.py holds both to an independent decoder bit by bit.
 * One row per mode, in the order: the two modes with a 2-bit mode field, the eight other two-subset modes, the four one-subset
 * modes.  Row = mode field, width of the mode field, endpoint bits, delta bits of R, G, B, transformed (1: endpoints 1..3 are
 * deltas to endpoint 0), subsets, then the block's bits after the mode field in stream order as runs {field, first bit, count}:
 * the next `count` stream bits are bits first, first + 1, ... of the field.  Fields: RW GW BW = endpoint 0, RX GX BX = endpoint 1,
 * RY.. and RZ.. = the second subset's two endpoints, D = the partition.  (A field's bits that the stream holds in DESCENDING
 * order -- the high bits of endpoint 0 in mode fields 01011 and 01111 -- are runs of one.)  The indices follow the last run: at
 * bit 82 in the two-subset modes, at bit 65 in the one-subset modes.  Mode fields 10011, 10111, 11011, 11111 are reserved. */
#ifdef ICAMD_BC6H_TABLE_MODES
{0x00, 2, 10, {5,5,5}, 1, 2, {{GY,4,1}, {BY,4,1}, {BZ,4,1}, {RW,0,10}, {GW,0,10}, {BW,0,10}, {RX,0,5}, {GZ,4,1}, {GY,0,4}, {GX,0,5}, {BZ,0,1}, {GZ,0,4}, {BX,0,5}, {BZ,1,1}, {BY,0,4}, {RY,0,5}, {BZ,2,1}, {RZ,0,5}, {BZ,3,1}, {D,0,5}}},
{0x01, 2,  7, {6,6,6}, 1, 2, {{GY,5,1}, {GZ,4,2}, {RW,0,7}, {BZ,0,2}, {BY,4,1}, {GW,0,7}, {BY,5,1}, {BZ,2,1}, {GY,4,1}, {BW,0,7}, {BZ,3,1}, {BZ,5,1}, {BZ,4,1}, {RX,0,6}, {GY,0,4}, {GX,0,6}, {GZ,0,4}, {BX,0,6}, {BY,0,4}, {RY,0,6}, {RZ,0,6}, {D,0,5}}},
{0x02, 5, 11, {5,4,4}, 1, 2, {{RW,0,10}, {GW,0,10}, {BW,0,10}, {RX,0,5}, {RW,10,1}, {GY,0,4}, {GX,0,4}, {GW,10,1}, {BZ,0,1}, {GZ,0,4}, {BX,0,4}, {BW,10,1}, {BZ,1,1}, {BY,0,4}, {RY,0,5}, {BZ,2,1}, {RZ,0,5}, {BZ,3,1}, {D,0,5}}},
{0x06, 5, 11, {4,5,4}, 1, 2, {{RW,0,10}, {GW,0,10}, {BW,0,10}, {RX,0,4}, {RW,10,1}, {GZ,4,1}, {GY,0,4}, {GX,0,5}, {GW,10,1}, {GZ,0,4}, {BX,0,4}, {BW,10,1}, {BZ,1,1}, {BY,0,4}, {RY,0,4}, {BZ,0,1}, {BZ,2,1}, {RZ,0,4}, {GY,4,1}, {BZ,3,1}, {D,0,5}}},
{0x0a, 5, 11, {4,4,5}, 1, 2, {{RW,0,10}, {GW,0,10}, {BW,0,10}, {RX,0,4}, {RW,10,1}, {BY,4,1}, {GY,0,4}, {GX,0,4}, {GW,10,1}, {BZ,0,1}, {GZ,0,4}, {BX,0,5}, {BW,10,1}, {BY,0,4}, {RY,0,4}, {BZ,1,2}, {RZ,0,4}, {BZ,4,1}, {BZ,3,1}, {D,0,5}}},
{0x0e, 5,  9, {5,5,5}, 1, 2, {{RW,0,9}, {BY,4,1}, {GW,0,9}, {GY,4,1}, {BW,0,9}, {BZ,4,1}, {RX,0,5}, {GZ,4,1}, {GY,0,4}, {GX,0,5}, {BZ,0,1}, {GZ,0,4}, {BX,0,5}, {BZ,1,1}, {BY,0,4}, {RY,0,5}, {BZ,2,1}, {RZ,0,5}, {BZ,3,1}, {D,0,5}}},
{0x12, 5,  8, {6,5,5}, 1, 2, {{RW,0,8}, {GZ,4,1}, {BY,4,1}, {GW,0,8}, {BZ,2,1}, {GY,4,1}, {BW,0,8}, {BZ,3,2}, {RX,0,6}, {GY,0,4}, {GX,0,5}, {BZ,0,1}, {GZ,0,4}, {BX,0,5}, {BZ,1,1}, {BY,0,4}, {RY,0,6}, {RZ,0,6}, {D,0,5}}},
{0x16, 5,  8, {5,6,5}, 1, 2, {{RW,0,8}, {BZ,0,1}, {BY,4,1}, {GW,0,8}, {GY,5,1}, {GY,4,1}, {BW,0,8}, {GZ,5,1}, {BZ,4,1}, {RX,0,5}, {GZ,4,1}, {GY,0,4}, {GX,0,6}, {GZ,0,4}, {BX,0,5}, {BZ,1,1}, {BY,0,4}, {RY,0,5}, {BZ,2,1}, {RZ,0,5}, {BZ,3,1}, {D,0,5}}},
{0x1a, 5,  8, {5,5,6}, 1, 2, {{RW,0,8}, {BZ,1,1}, {BY,4,1}, {GW,0,8}, {BY,5,1}, {GY,4,1}, {BW,0,8}, {BZ,5,1}, {BZ,4,1}, {RX,0,5}, {GZ,4,1}, {GY,0,4}, {GX,0,5}, {BZ,0,1}, {GZ,0,4}, {BX,0,6}, {BY,0,4}, {RY,0,5}, {BZ,2,1}, {RZ,0,5}, {BZ,3,1}, {D,0,5}}},
{0x1e, 5,  6, {6,6,6}, 0, 2, {{RW,0,6}, {GZ,4,1}, {BZ,0,2}, {BY,4,1}, {GW,0,6}, {GY,5,1}, {BY,5,1}, {BZ,2,1}, {GY,4,1}, {BW,0,6}, {GZ,5,1}, {BZ,3,1}, {BZ,5,1}, {BZ,4,1}, {RX,0,6}, {GY,0,4}, {GX,0,6}, {GZ,0,4}, {BX,0,6}, {BY,0,4}, {RY,0,6}, {RZ,0,6}, {D,0,5}}},
{0x03, 5, 10, {10,10,10}, 0, 1, {{RW,0,10}, {GW,0,10}, {BW,0,10}, {RX,0,10}, {GX,0,10}, {BX,0,10}}},
{0x07, 5, 11, {9,9,9}, 1, 1, {{RW,0,10}, {GW,0,10}, {BW,0,10}, {RX,0,9}, {RW,10,1}, {GX,0,9}, {GW,10,1}, {BX,0,9}, {BW,10,1}}},
{0x0b, 5, 12, {8,8,8}, 1, 1, {{RW,0,10}, {GW,0,10}, {BW,0,10}, {RX,0,8}, {RW,11,1}, {RW,10,1}, {GX,0,8}, {GW,11,1}, {GW,10,1}, {BX,0,8}, {BW,11,1}, {BW,10,1}}},
{0x0f, 5, 16, {4,4,4}, 1, 1, {{RW,0,10}, {GW,0,10}, {BW,0,10}, {RX,0,4}, {RW,15,1}, {RW,14,1}, {RW,13,1}, {RW,12,1}, {RW,11,1}, {RW,10,1}, {GX,0,4}, {GW,15,1}, {GW,14,1}, {GW,13,1}, {GW,12,1}, {GW,11,1}, {GW,10,1}, {BX,0,4}, {BW,15,1}, {BW,14,1}, {BW,13,1}, {BW,12,1}, {BW,11,1}, {BW,10,1}}},
#endif
