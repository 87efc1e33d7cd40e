"""Operand sets and plain definitions for the instruction wrappers of image-compression_amd/csrc (the list of
tests/device_probe/wrapper_ops.h).  Plain numpy, deterministic.  Shared by tests/test_wrappers_host.py (the twins, everywhere)
and tests/test_gpu_wrappers.py (the device forms, on an MI355X).

Per op:
  definition(a, b, c)  the operation in 64-bit numpy integers, written from the comment in the header that defines the wrapper
                       -- never from the host twin; evaluated on in-domain cases only;
  in_domain(a, b, c)   the precondition as the header states it (all true where it states none);
  into_domain(a, b, c) the masking that brings random operands into the domain;
  control              the op's small operand, exhaustively.
An op's cases are edges + control + random, in that order (uint32 [n, 3]); the recorded hashes of
tests/golden/gfx950_wrapper_hashes.json cover edges + control.
"""
import functools
import hashlib
import itertools
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OPS_H = os.path.join(HERE, "device_probe", "wrapper_ops.h")
GOLDEN = os.path.join(HERE, "golden", "gfx950_wrapper_hashes.json")

EDGE_VALUES = [0, 1, 0x7f, 0x80, 0xff, 0x100, 0x7fff, 0x8000, 0xffff, 0x10000, 0x7fffff, 0x800000, 0xffffff, 0x1000000,
               0x7fffffff, 0x80000000, 0xffffffff]
N_RANDOM = 1 << 18
M32 = np.uint64(0xffffffff)
U = np.uint64


# ---- the list

def parse_ops_header(text=None):
    """{list macro: [(id, wrapper, arity, header)]} from the X(...) / Y(...) lines of wrapper_ops.h, in the file's order."""
    if text is None:
        with open(OPS_H) as f:
            text = f.read()
    lists = {}
    for m in re.finditer(r"#define (ICAMD_WRAPPER_\w+)\([XY]\)((?:.*\\\n)*.*\n)", text):
        rows = re.findall(r'^\s*[XY]\((\w+), "(\w+)", (\d), "([\w.]+)"', m.group(2), flags=re.M)
        lists[m.group(1)] = [(i, w, int(n), h) for i, w, n, h in rows]
    return lists


def op_list():
    """[(id, wrapper, arity, header)]: position = the op's number in the probe's files and in wrapper_emul_apply."""
    lists = parse_ops_header()
    return lists["ICAMD_WRAPPER_OPS"] + lists["ICAMD_WRAPPER_SCAN_OPS"]


def op_numbers():
    """{id: number}, the second build of the scan (scan_plain_b0 ..) after the list."""
    ids = [row[0] for row in op_list()]
    numbers = {name: i for i, name in enumerate(ids)}
    for k in range(4):
        numbers["scan_plain_b%d" % k] = len(ids) + k
    return numbers


# ---- helpers on uint64 arrays that hold 32-bit values

def _bytes(v):
    return [(v >> U(8 * i)) & U(0xff) for i in range(4)]


def _halves(v):
    return v & U(0xffff), v >> U(16)


def _absdiff(x, y):
    return np.where(x > y, x - y, y - x)


def _signed(v):
    return v.astype(np.int64) - ((v >> U(31)).astype(np.int64) << 32)


def _wrap(v):
    """a signed or unsigned 64-bit result modulo 2^32"""
    return (np.asarray(v).astype(np.int64) & np.int64(0xffffffff)).astype(np.uint64)


def _pack16(lo, hi):
    return (lo & U(0xffff)) | (hi & U(0xffff)) << U(16)


def _popcount(v):
    n = np.zeros(v.shape, np.uint64)
    for i in range(32):
        n += (v >> U(i)) & U(1)
    return n


def _everywhere(a, b, c):
    return np.ones(a.shape, bool)


def _as_is(a, b, c):
    return a, b, c


class Op:
    def __init__(self, definition, in_domain=_everywhere, into_domain=_as_is, control=None, domain=""):
        self.definition, self.in_domain, self.into_domain = definition, in_domain, into_domain
        self.control = control  # () -> uint32 [n, 3]
        self.domain = domain    # the precondition in words ("" = every operand)
        self.has_precondition = in_domain is not _everywhere


# ---- definitions, from the headers' comments

def _udot4(a, b, c):  # a.b0*b.b0 + a.b1*b.b1 + a.b2*b.b2 + a.b3*b.b3 + c
    return (sum(x * y for x, y in zip(_bytes(a), _bytes(b))) + c) & M32


def _sad_u16x2(a, b, c):  # |a.lo16 - b.lo16| + |a.hi16 - b.hi16| + c
    (al, ah), (bl, bh) = _halves(a), _halves(b)
    return (_absdiff(al, bl) + _absdiff(ah, bh) + c) & M32


def _sad_u8(a, b, c):  # sum over the 4 bytes of |a.b - b.b|, plus c
    return (sum(_absdiff(x, y) for x, y in zip(_bytes(a), _bytes(b))) + c) & M32


def _perm(hi, lo, sel):  # byte i of the result = byte sel.b[i] of the 8-byte value {hi,lo}; 0x0c -> 0x00
    data = _bytes(lo) + _bytes(hi)
    out = np.zeros(hi.shape, np.uint64)
    for i, s in enumerate(_bytes(sel)):
        picked = np.zeros(hi.shape, np.uint64)
        for k in range(8):
            picked = np.where(s == U(k), data[k], picked)
        out |= picked << U(8 * i)
    return out


def _perm_ok(hi, lo, sel):
    ok = np.ones(hi.shape, bool)
    for s in _bytes(sel):
        ok &= (s <= U(7)) | (s == U(0x0c))
    return ok


def _perm_mask(hi, lo, sel):
    out = np.zeros(hi.shape, np.uint64)
    for i, s in enumerate(_bytes(sel)):
        out |= np.where(s & U(8) != 0, U(0x0c), s & U(7)) << U(8 * i)
    return hi, lo, out


def _mask24s(v):
    """any 32-bit pattern -> a signed value of magnitude below 2^23 (as a 32-bit pattern)"""
    s = (v & U(0xffffff)).astype(np.int64)
    s = np.where(s >= 1 << 23, s - (1 << 24), s)
    return _wrap(np.where(s == -(1 << 23), 0, s))


def _in24s(v):
    return np.abs(_signed(v)) < (1 << 23)


def _fastdiv_mask(n, d, c):
    d = d & U(0x7fffffff)
    return n & U(0x7fffffff), np.where(d == 0, U(1), d), c


def _scan_value(a, b):
    (d0, d1), (d2, d3) = _halves(a), _halves(b)
    s1 = d1 < d0
    s2 = s1 & (d2 < d1)
    s3 = s2 & (d3 < d2)
    return s1.astype(np.uint64) + s2.astype(np.uint64) + s3.astype(np.uint64)


def _scan(k):
    byte = U(0xff) << U(8 * k)

    def definition(a, b, c):  # the value (0..3) is ADDED into acc at the byte whose unit is 2^(8 k)
        return (c + (_scan_value(a, b) << U(8 * k))) & M32

    def in_domain(a, b, c):  # the byte is zero on entry; with unit 1 the whole of acc
        return (c == 0) if k == 0 else (c & byte) == 0

    def into_domain(a, b, c):
        return a, b, (np.zeros_like(c) if k == 0 else c & ~byte & M32)

    def control():
        vals = (0, 1, 510, 1020)
        accs = [0, 0x100 if k == 0 else 0xffffffff & ~(0xff << 8 * k), 1 << 8 * k, 0xff << 8 * k, 0xffffffff, 0x04030201]
        rows = [(d[0] | d[1] << 16, d[2] | d[3] << 16, acc) for d in itertools.product(vals, repeat=4) for acc in accs]
        return np.array(rows, np.uint32)

    return Op(definition, in_domain, into_domain, control,
              "byte %d of acc is zero%s" % (k, "; the whole of acc" if k == 0 else ""))


# ---- control sets

PAIRS8 = [(0x00000000, 0x00000000), (0xffffffff, 0xffffffff), (0x03020100, 0x07060504), (0x80808080, 0x7f7f7f7f),
          (0x7f7f7f7f, 0x80808080), (0x80ff7f01, 0x017fff80), (0x12345678, 0x9abcdef0), (0xdeadbeef, 0x00c0ffee)]


def _perm_control():
    rows = []
    for pos in range(4):
        for s in range(256):
            sel = (0x03020100 & ~(0xff << 8 * pos)) | s << 8 * pos
            rows += [(hi, lo, sel) for hi, lo in PAIRS8]
    return np.array(rows, np.uint32)


def _bfe_control():
    return np.array([(v, off, w) for v in (0xffffffff, 0x80000001, 0x12345678, 0xdeadbeef) for off in range(41)
                     for w in range(41)], np.uint32)


def _alignbit_control():
    return np.array([(hi, lo, sh) for hi, lo in PAIRS8 for sh in range(64)], np.uint32)


def _bit_mask_control():
    values = [1 << k for k in range(32)] + [0xffffffff ^ (1 << k) for k in range(32)] + [0, 0xffffffff]
    return np.array([(v, bit, 0) for v in values for bit in range(41)], np.uint32)


def _pk_lshr16_control():
    values = [0xffffffff, 0x80008000, 0x00018000, 0x7fff0001, 0x12345678, 0xdeadbeef, 0x0000ffff, 0xffff0000]
    return np.array([(v, sh, 0) for v in values for sh in range(32)], np.uint32)


# (grid height, grid width, images) of every launch tests/test_gpu_metric.py measures.  Its _measure() asserts that the launch
# it is about to make is listed here, so a shape added there without a line here fails on the GPU box.
METRIC_GRIDS = {(64, 64, 1), (8, 8, 1), (256, 256, 1), (61, 59, 1), (5, 3, 1), (1, 1, 1), (257, 1023, 1), (70, 72, 1), (14, 16, 1),
                (10, 14, 1), (266, 1036, 1), (61, 59, 5), (64, 128, 3), (64, 64, 5), (256, 256, 3), (8, 8, 37), (12, 20, 300),
                (4096, 4096, 1), (2048, 2048, 1), (128, 128, 1), (128, 128, 3), (37, 130, 1)}


def fastdiv_divisors():
    """The issue's divisors, and block_cols, blocks_per_image and the blocks of the whole batch of every metric launch; the same
    of every launch of the walk table (tests/walk_cases.py), the launches of more than 2^31 - 1 blocks among them."""
    import walk_cases  # (here: this module stays plain numpy for those who only want the operand sets)
    d = {1, 2, 3, 5, 7, 255, 256, 257, 1023, 65535, 65536, (1 << 31) - 1} | walk_cases.fastdiv_grids()
    for h, w, n in METRIC_GRIDS:
        rows = (h + 3) // 4
        for cols in ((w + 3) // 4, (w + 7) // 8):  # (PVRTC 2 bpp: blocks of 8 x 4 pixels)
            d |= {cols, rows * cols, rows * cols * n}
    return sorted(d)


def _fastdiv_control():
    rows = []
    for d in fastdiv_divisors():
        ns = {0, 1, d - 1, d, d + 1, 2 * d - 1, 2 * d, 1000 * d - 1, 1000 * d, (1 << 31) - d - 1, (1 << 31) - d, (1 << 31) - 2,
              (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 31) + d - 1, (1 << 31) + d, (1 << 32) - d, (1 << 32) - 2, (1 << 32) - 1}
        q = ((1 << 31) - 1) // d
        ns |= {q * d - 1, q * d, ((1 << 32) - 1) // d * d - 1, ((1 << 32) - 1) // d * d}
        rows += [(n, d, 0) for n in sorted(ns) if 0 <= n < 1 << 32]
    return np.array(rows, np.uint32)


# ---- the table

def _pk2(f):
    def definition(a, b, c):
        (al, ah), (bl, bh), (cl, ch) = _halves(a), _halves(b), _halves(c)
        return _pack16(f(al, bl, cl), f(ah, bh, ch))
    return definition


def _pk_lane(lane):
    def definition(a, w, c):  # lane k of the result = a.lane[k] * w.lane[L] + c.lane[k]  (mod 2^16)
        (al, ah), (cl, ch), ww = _halves(a), _halves(c), _halves(w)[lane]
        return _pack16(al * ww + cl, ah * ww + ch)
    return definition


def _wide(a, b, c):
    return ((b << U(32) | a) + c)  # modulo 2^64 (uint64 wraps)


OPS = {
    "umulhi32": Op(lambda a, b, c: (a * b) >> U(32)),
    "udot4": Op(_udot4),
    "sad_u32": Op(lambda a, b, c: (_absdiff(a, b) + c) & M32, lambda a, b, c: (a < 65536) & (b < 65536),
                  lambda a, b, c: (a & U(0xffff), b & U(0xffff), c), domain="a, b < 65536"),
    "sad_u16x2": Op(_sad_u16x2),
    "sad_u8": Op(_sad_u8),
    "sad_hi_u8": Op(lambda a, b, c: ((_sad_u8(a, b, np.zeros_like(c)) << U(16)) + c) & M32),
    "alignbit": Op(lambda hi, lo, sh: ((hi << U(32) | lo) >> sh) & M32, lambda hi, lo, sh: sh < 32,
                   lambda hi, lo, sh: (hi, lo, sh & U(31)), _alignbit_control, "sh < 32"),
    "avg_u8": Op(lambda a, b, c: sum(((x + y) >> U(1)) << U(8 * i) for i, (x, y) in enumerate(zip(_bytes(a), _bytes(b))))),
    "perm": Op(_perm, _perm_ok, _perm_mask, _perm_control, "every selector byte is 0..7 or 0x0c"),
    "bfe": Op(lambda v, off, w: (v >> off) & ((U(1) << w) - U(1)), lambda v, off, w: (off < 32) & (w < 32),
              lambda v, off, w: (v, off & U(31), w & U(31)), _bfe_control, "off < 32, w < 32"),
    "bit_mask": Op(lambda v, bit, c: ((v >> bit) & U(1)) * M32, lambda v, bit, c: bit < 32,
                   lambda v, bit, c: (v, bit & U(31), c), _bit_mask_control, "bit < 32"),
    "imad24": Op(lambda a, b, c: _wrap(_signed(a) * _signed(b) + _signed(c)), lambda a, b, c: _in24s(a) & _in24s(b),
                 lambda a, b, c: (_mask24s(a), _mask24s(b), c), domain="|a|, |b| < 2^23"),
    "umad24": Op(lambda a, b, c: (a * b + c) & M32, lambda a, b, c: (a < 1 << 24) & (b < 1 << 24),
                 lambda a, b, c: (a & U(0xffffff), b & U(0xffffff), c), domain="a, b < 2^24"),
    "umin": Op(lambda a, b, c: np.minimum(a, b)),
    "umax": Op(lambda a, b, c: np.maximum(a, b)),
    "imin": Op(lambda a, b, c: _wrap(np.minimum(_signed(a), _signed(b)))),
    "imax": Op(lambda a, b, c: _wrap(np.maximum(_signed(a), _signed(b)))),
    "fastdiv": Op(lambda n, d, c: n // d, lambda n, d, c: (n < 1 << 31) & (d >= 1) & (d <= 1 << 31), _fastdiv_mask,
                  _fastdiv_control, "n < 2^31, 1 <= d <= 2^31"),
    "pk_addsat_u16": Op(_pk2(lambda x, y, z: np.minimum(x + y, U(0xffff)))),
    "pk_subsat_u16": Op(_pk2(lambda x, y, z: np.where(x > y, x - y, U(0)))),
    "udot2_u16": Op(lambda a, b, c: (_halves(a)[0] * _halves(b)[0] + _halves(a)[1] * _halves(b)[1] + c) & M32),
    "pk_sub_u16": Op(_pk2(lambda x, y, z: x + U(0x10000) - y)),
    "pk_min_u16": Op(_pk2(lambda x, y, z: np.minimum(x, y))),
    "pk_max_u16": Op(_pk2(lambda x, y, z: np.maximum(x, y))),
    "pk_lshr16": Op(lambda v, sh, c: _pack16(_halves(v)[0] >> sh, _halves(v)[1] >> sh), lambda v, sh, c: sh < 16,
                    lambda v, sh, c: (v, sh & U(15), c), _pk_lshr16_control, "sh < 16"),
    "pk_mad_u16": Op(_pk2(lambda x, y, z: x * y + z)),
    "pk_mad_u16_lane0": Op(_pk_lane(0)),
    "pk_mad_u16_lane1": Op(_pk_lane(1)),
    "popcount_u32": Op(lambda a, b, c: _popcount(a)),
    "pack64": Op(lambda lo, hi, c: ((hi << U(32) | lo) >> (c & U(63))) & M32),
    "lo32": Op(lambda a, b, c: _wide(a, b, c) & M32),
    "hi32": Op(lambda a, b, c: _wide(a, b, c) >> U(32)),
    "popc32": Op(lambda a, b, c: _popcount(a)),
}
for _k in range(4):
    OPS["scan_b%d" % _k] = _scan(_k)
    OPS["scan_plain_b%d" % _k] = _scan(_k)  # the second device build: no twin of its own, held to the definition in domain


# ---- the cases

@functools.lru_cache(maxsize=None)
def edges():
    return np.array(list(itertools.product(EDGE_VALUES, repeat=3)), np.uint32)


def _seed(name):
    return int.from_bytes(hashlib.sha256(name.replace("scan_plain", "scan").encode()).digest()[:8], "little")


@functools.lru_cache(maxsize=None)
def cases(name):
    """(operands uint32 [n, 3] in the order edges, control, random; the number of edge + control cases)"""
    op = OPS[name]
    control = op.control() if op.control else np.zeros((0, 3), np.uint32)
    rnd = np.random.Generator(np.random.PCG64(_seed(name))).integers(0, 1 << 32, size=(N_RANDOM, 3), dtype=np.uint64)
    a, b, c = op.into_domain(rnd[::2, 0], rnd[::2, 1], rnd[::2, 2])  # every other one: masked into the domain
    rnd[::2, 0], rnd[::2, 1], rnd[::2, 2] = a, b, c
    out = np.concatenate([edges(), control, rnd.astype(np.uint32)])
    out.setflags(write=False)
    return out, len(edges()) + len(control)


def split(operands):
    o = operands.astype(np.uint64)
    return o[:, 0], o[:, 1], o[:, 2]


def domain_mask(name, operands):
    return np.asarray(OPS[name].in_domain(*split(operands)), bool)


def expected(name, operands):
    """The plain definition on (in-domain) operands, as uint32."""
    a, b, c = split(operands)
    with np.errstate(over="ignore"):
        return np.asarray(OPS[name].definition(a, b, c)).astype(np.uint64).astype(np.uint32)


def digest(results_edges_and_control):
    return hashlib.sha256(np.ascontiguousarray(results_edges_and_control, dtype="<u4").tobytes()).hexdigest()


def first_difference(name, operands, got, want, what):
    """None, or a message with the first case at which got != want."""
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    if not len(bad):
        return None
    i = int(bad[0])
    return "%s: %s differ at %d of %d cases, first at case %d: operands (0x%x, 0x%x, 0x%x): 0x%x != 0x%x" % (
        name, what, len(bad), len(got), i, operands[i, 0], operands[i, 1], operands[i, 2], got[i], want[i])


# ---- the lane forms (one wave of 64)

def vote_cases():
    """[(exit mask, predicate mask)] as 64-bit integers: every exit mask with every kind of predicate."""
    full = (1 << 64) - 1
    exits = [0, 1 << 17, (1 << 32) - 1, 0xaaaaaaaaaaaaaaaa, full ^ (1 << 40)]
    out = []
    for ex in exits:
        active = full ^ ex
        one_active = active & -active if ex != 0xaaaaaaaaaaaaaaaa else 1 << 42
        assert one_active & active
        out.append((ex, active))               # true in all active lanes (and false in the exited ones)
        out.append((ex, full))                 # true everywhere
        out.append((ex, full ^ one_active))    # false in exactly one active lane
        out.append((ex, active | (ex >> 1 & ex)))  # false only in (some) exited lanes
        out.append((ex, 0x0123456789abcdef))   # a mixture
        out.append((ex, 0))
    return out


def vote_expected(ex, pred):
    """(all [64], count [64]) as the active lanes see them; 0xffffffff in the lanes that returned early."""
    active = [not (ex >> l) & 1 for l in range(64)]
    p = [bool((pred >> l) & 1) for l in range(64)]
    all_ = int(all(p[l] for l in range(64) if active[l]))
    count = sum(p[l] for l in range(64) if active[l])
    return (np.array([all_ if active[l] else 0xffffffff for l in range(64)], np.uint32),
            np.array([count if active[l] else 0xffffffff for l in range(64)], np.uint32))


def quad_values():
    return np.random.Generator(np.random.PCG64(0x9AD)).integers(0, 1 << 32, size=64, dtype=np.uint64).astype(np.uint32)


# ---- the float first guesses of mip_normal.h: everything the filter can form

LS_FIRST, LS_LAST, A_LAST = 16, 28267, 1020
GUESS_SETS = ["isqrt_z", "isqrt_length", "div_code"]


def guess_count(which):
    return {"isqrt_z": 65025 + 1, "isqrt_length": 3 * 1020 * 1020 + 1,
            "div_code": (A_LAST + 1) * (LS_LAST - LS_FIRST + 1)}[which]


def guess_operands(which, first, count):
    """(n, d) as int64 arrays for the set's cases first .. first + count - 1 (d is None for the square roots)."""
    i = np.arange(first, first + count, dtype=np.int64)
    if which == "isqrt_z":
        return 4 * i, None
    if which == "isqrt_length":
        return i << 8, None
    n_ls = LS_LAST - LS_FIRST + 1
    a, ls = i // n_ls, LS_FIRST + i % n_ls
    return 4080 * a + (ls >> 1), ls


def exact_floor(n, d):
    """floor(sqrt(n)) (d is None) or floor(n / d), in 64-bit integers."""
    if d is not None:
        return n // d
    s = np.sqrt(n.astype(np.float64)).astype(np.int64)  # n < 2^30: within one of the floor; settled in integers
    s -= (s * s > n)
    s += ((s + 1) * (s + 1) <= n)
    return s
