"""CPU tier: the host twins of the instruction wrappers (image-compression_amd/csrc/*.h under -DICAMD_HOST_EMULATION), op by op.

tests/host_emul/wrapper_emul.cc compiles the list of tests/device_probe/wrapper_ops.h with the twins.  Checked here, everywhere:
the twins equal the plain definitions of tests/wrapper_cases.py wherever the stated domain holds; their results over the edge
and control cases hash to what an MI355X returned for them (tests/golden/gfx950_wrapper_hashes.json, recorded by
tests/test_gpu_wrappers.py, which compares case by case); the violation counter rises on exactly the cases outside the domain;
and no wrapper of csrc/*.h is missing from the list.  The tests here feed operands outside the domains on purpose: twin_apply
puts the library's counter back to where it was, and the fixture asserts a zero count at teardown like every other."""
import ctypes
import glob
import json
import os
import re
import subprocess

import numpy as np
import pytest

import ic_testlib as T
import wrapper_cases as W

CSRC = os.path.join(T.ROOT, "image-compression_amd", "csrc")
EMUL_DIR = os.path.join(T.ROOT, "tests", "host_emul")
LIST_IDS = [row[0] for row in W.op_list()]


def build_wrapper_emul(directory):
    so = os.path.join(str(directory), "libwrapper_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DICAMD_HOST_EMULATION", "-I" + CSRC,
                           "-I" + os.path.join(T.ROOT, "include"), "-o", so, os.path.join(EMUL_DIR, "wrapper_emul.cc")])
    L = ctypes.CDLL(so)
    L.wrapper_emul_op_id.restype = ctypes.c_char_p
    L.wrapper_emul_op_id.argtypes = [T.ci]
    L.wrapper_emul_apply.restype = T.ci
    L.wrapper_emul_apply.argtypes = [T.ci, T.u32, T.vp, T.vp]
    L.wrapper_emul_flags.restype = T.ci
    L.wrapper_emul_flags.argtypes = [T.ci, T.u32, T.vp, T.vp]
    L.wrapper_emul_isqrt.restype = None
    L.wrapper_emul_isqrt.argtypes = [T.u32, T.vp, T.vp, T.vp]
    L.wrapper_emul_div.restype = None
    L.wrapper_emul_div.argtypes = [T.u32, T.vp, T.vp, T.vp, T.vp]
    L.icamd_emul_violations.restype = ctypes.c_ulonglong
    L.icamd_emul_violations.argtypes = [ctypes.c_char_p, T.sz]
    L.icamd_emul_violations_restore.restype = None
    L.icamd_emul_violations_restore.argtypes = [ctypes.c_ulonglong, ctypes.c_char_p]
    return L


def violations(L):
    """(count, first) of the library's counter."""
    first = ctypes.create_string_buffer(256)
    return L.icamd_emul_violations(first, len(first)), first.value


def twin_apply(L, name, operands, keep_count=False):
    """The op's twin on every case.  The cases lie outside the domains on purpose, so the counter is put back afterwards."""
    ops = np.ascontiguousarray(operands, np.uint32)
    out = np.zeros(len(ops), np.uint32)
    before = violations(L)
    assert L.wrapper_emul_apply(W.op_numbers()[name], len(ops), ops.ctypes.data, out.ctypes.data) == 1, name
    if not keep_count:
        L.icamd_emul_violations_restore(*before)
    return out


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    L = build_wrapper_emul(tmp_path_factory.mktemp("wrappers"))
    yield L
    T.assert_no_emul_violations(L, "test_wrappers_host")


def test_the_python_parse_of_the_list_is_the_compiled_list(emul):
    assert emul.wrapper_emul_op_count() == len(LIST_IDS)
    assert [emul.wrapper_emul_op_id(i).decode() for i in range(len(LIST_IDS))] == LIST_IDS
    assert sorted(W.OPS) == sorted(LIST_IDS + ["scan_plain_b%d" % k for k in range(4)])
    assert emul.wrapper_emul_apply(len(LIST_IDS), 0, None, None) == 0 and emul.wrapper_emul_apply(-1, 0, None, None) == 0


@pytest.mark.parametrize("name", sorted(W.OPS))
def test_the_sets_hold_enough_cases_on_both_sides_of_the_domain(name):
    operands, n_fixed = W.cases(name)
    assert (operands[:len(W.edges())] == W.edges()).all() and len(W.edges()) == 17 ** 3
    assert len(operands) == n_fixed + W.N_RANDOM and W.N_RANDOM == 1 << 18
    inside = W.domain_mask(name, operands)
    assert inside.sum() >= 1000, (name, inside.sum())
    assert inside[n_fixed::2].all(), name  # the masked half of the random cases
    if W.OPS[name].has_precondition:
        assert (~inside).sum() >= 100 and W.OPS[name].domain, (name, (~inside).sum())
    else:
        assert inside.all()


def test_the_control_sets_are_exhaustive_where_the_issue_names_them():
    def column(name, k):
        return set(W.OPS[name].control()[:, k].tolist())
    sel = W.OPS["perm"].control()[:, 2]
    for pos in range(4):
        assert {int(s) >> 8 * pos & 0xff for s in sel} == set(range(256))
    assert len(W.OPS["perm"].control()) == 4 * 256 * 8
    bfe = W.OPS["bfe"].control()
    assert {(int(o), int(w)) for o, w in bfe[:, 1:]} == {(o, w) for o in range(41) for w in range(41)}
    assert column("alignbit", 2) == set(range(64)) and column("bit_mask", 1) == set(range(41))
    assert column("pk_lshr16", 1) == set(range(32))
    fd = W.OPS["fastdiv"].control()
    assert {1, 2, 3, 5, 7, 255, 256, 257, 1023, 65535, 65536, (1 << 31) - 1} <= column("fastdiv", 1)
    for h, w, n in W.METRIC_GRIDS:  # block_cols, blocks_per_image and the batch's blocks of every metric launch
        rows, cols = (h + 3) // 4, (w + 3) // 4
        assert {cols, (w + 7) // 8, rows * cols, rows * ((w + 7) // 8), rows * cols * n} <= column("fastdiv", 1), (h, w, n)
    assert (8, 8, 37) in W.METRIC_GRIDS and 4 * 37 in column("fastdiv", 1)
    for d in W.fastdiv_divisors():
        ns = fd[fd[:, 1] == d][:, 0]
        assert (ns < 1 << 31).any() and (ns >= 1 << 31).any(), d
    for k in range(4):
        c = W.OPS["scan_b%d" % k].control()
        orderings = {(int(a) & 0xffff, int(a) >> 16, int(b) & 0xffff, int(b) >> 16) for a, b in c[:, :2]}
        assert len(orderings) == 4 ** 4, k


@pytest.mark.parametrize("name", LIST_IDS)
def test_the_twin_equals_the_plain_definition_in_the_domain(emul, name):
    operands, _ = W.cases(name)
    inside = W.domain_mask(name, operands)
    got = twin_apply(emul, name, operands)
    msg = W.first_difference(name, operands[inside], got[inside], W.expected(name, operands[inside]), "twin and definition")
    assert msg is None, msg


def golden():
    with open(W.GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", LIST_IDS)
def test_the_twin_hashes_to_what_the_device_returned(emul, name):
    operands, n_fixed = W.cases(name)
    assert W.digest(twin_apply(emul, name, operands[:n_fixed])) == golden()["ops"][name], name


def test_the_golden_file_covers_the_list_and_nothing_else():
    assert sorted(golden()["ops"]) == sorted(W.OPS)


@pytest.mark.parametrize("name", LIST_IDS)
def test_the_counter_rises_on_exactly_the_cases_outside_the_domain(emul, name):
    operands, _ = W.cases(name)
    ops = np.ascontiguousarray(operands, np.uint32)
    flags = np.full(len(ops), 7, np.uint8)
    assert emul.wrapper_emul_flags(W.op_numbers()[name], len(ops), ops.ctypes.data, flags.ctypes.data) == 1
    outside = ~W.domain_mask(name, operands)
    msg = W.first_difference(name, operands, flags, outside.astype(np.uint8), "counted and outside the domain")
    assert msg is None, msg


def test_the_count_and_the_first_violation_are_reported(emul):
    assert violations(emul) == (0, b"")
    cases = np.array([[1, 2, 3], [0x1000000, 5, 6], [7, 0xffffffff, 8]], np.uint32)
    twin_apply(emul, "umad24", cases)
    assert violations(emul) == (0, b"")  # put back
    twin_apply(emul, "umad24", cases, keep_count=True)
    count, first = violations(emul)
    text = first.decode()
    assert count == 2 and text.startswith("umad24(0x1000000, 0x5, 0x6) at ") and "wrapper_ops.h:" in text, (count, text)
    twin_apply(emul, "fastdiv", np.array([[1 << 31, 7, 0]], np.uint32))
    assert violations(emul) == (2, first)  # an earlier state is restored whole, not reset
    emul.icamd_emul_violations_restore(0, b"")
    twin_apply(emul, "fastdiv", np.array([[5, 0, 0]], np.uint32), keep_count=True)  # d = 0 runs as mul 0, shift 32
    assert violations(emul)[0] == 1 and violations(emul)[1].startswith(b"fastdiv(0x5, 0x0, 0x20) at "), violations(emul)
    emul.icamd_emul_violations_restore(0, b"")
    assert violations(emul) == (0, b"")


def test_each_emulation_library_has_a_counter_of_its_own(emul, tmp_path):
    """Two host-emulation libraries in one process: a violation in one is not seen in the other (the counter of ic_device.h has
    internal linkage; a shared one would fail the teardown of whichever host module runs after an out-of-domain case)."""
    so = str(tmp_path / "libbc45_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DICAMD_HOST_EMULATION", "-I" + CSRC, "-o", so,
                           os.path.join(EMUL_DIR, "bc45_emul.cc")])
    other = ctypes.CDLL(so)
    other.icamd_emul_violations.restype = ctypes.c_ulonglong
    other.icamd_emul_violations.argtypes = [ctypes.c_char_p, T.sz]
    second = build_wrapper_emul(tmp_path)  # and a second copy of the same library
    assert violations(emul) == (0, b"") and violations(other) == (0, b"") and violations(second) == (0, b"")
    twin_apply(emul, "umad24", np.array([[0x1000000, 5, 6]], np.uint32), keep_count=True)
    assert violations(emul)[0] == 1 and violations(other) == (0, b"") and violations(second) == (0, b"")
    twin_apply(second, "bfe", np.array([[1, 32, 1], [1, 1, 32]], np.uint32), keep_count=True)
    assert violations(emul)[0] == 1 and violations(other) == (0, b"") and violations(second)[0] == 2
    emul.icamd_emul_violations_restore(0, b"")
    assert violations(emul) == (0, b"") and violations(second)[0] == 2
    T.assert_no_emul_violations(other, "bc45_emul next to wrapper_emul")


def test_the_probe_is_built_with_the_flags_of_the_library():
    """tests/cxx/Makefile repeats three lines of image-compression_amd/Makefile; they stay the same lines."""
    def lines(path):
        with open(path) as f:
            return {l.split()[0]: l.rstrip("\n") for l in f if l.startswith(("HIPCC ", "ARCH ", "HIPFLAGS "))}
    product = lines(os.path.join(T.ROOT, "image-compression_amd", "Makefile"))
    probe = lines(os.path.join(T.ROOT, "tests", "cxx", "Makefile"))
    assert sorted(product) == ["ARCH", "HIPCC", "HIPFLAGS"] and probe == product, (probe, product)
    with open(os.path.join(T.ROOT, "tests", "cxx", "Makefile")) as f:
        text = f.read()
    assert "CSRC     := $(PKG)/csrc\n" in text and "PKG  := $(ROOT)/image-compression_amd\n" in text  # what the lines expand over


def test_the_float_twins_settle_to_the_exact_values(emul):
    """The host's own first guesses (sqrtf, 1.0f / d) over everything the filter can form: within one of the exact floor, and
    settled exactly -- what tests/test_gpu_wrappers.py asserts of v_sqrt_f32 and v_rcp_f32."""
    assert violations(emul) == (0, b"")
    for which in W.GUESS_SETS:
        total, chunk = W.guess_count(which), 1 << 22
        for first in range(0, total, chunk):
            count = min(chunk, total - first)
            n, d = W.guess_operands(which, first, count)
            n32, guess, settled = n.astype(np.uint32), np.zeros(count, np.uint32), np.zeros(count, np.uint32)
            if d is None:
                emul.wrapper_emul_isqrt(count, n32.ctypes.data, guess.ctypes.data, settled.ctypes.data)
            else:
                d32 = d.astype(np.uint32)
                emul.wrapper_emul_div(count, n32.ctypes.data, d32.ctypes.data, guess.ctypes.data, settled.ctypes.data)
            exact = W.exact_floor(n, d)
            assert (np.abs(guess.astype(np.int64) - exact) <= 1).all() and (settled == exact).all(), (which, first)
    assert emul.icamd_emul_violations(None, 0) == 0  # every one of them inside normal_isqrt's and normal_div's domains


# ---- completeness: every wrapper of csrc/*.h is in the list

# Collected by the scan below but no instruction wrapper of three operands, with the reason:
EXEMPT = {
    "opaque": "an optimisation barrier (an empty asm): returns its operand",
    "opaque64": "the same barrier on a register pair",
    "load_stream": "a memory access (non-temporal load), not arithmetic",
    "encode_etc1_block_quad": "the quad encoder: four lanes on the device, a loop on the host; quad_xor1 / quad_xor2 are listed",
    "etc1_pad_block_quad": "its two arms differ only in the quad encoder's signature",
}
LISTED = ({row[1] for row in W.op_list()} | {row[1] for key in ("ICAMD_WRAPPER_FLOAT_OPS", "ICAMD_WRAPPER_LANE_OPS")
                                             for row in W.parse_ops_header()[key]})
TRIGGERS = re.compile(r"__builtin_amdgcn_|__builtin_elementwise_|__mul24|__umul24|__umulhi|__popc|\basm\s*(?:volatile\s*)?\(\s*(?!\"\"\s*:)")
DEFINITION = re.compile(r"(?:ICAMD_DEV|__device__\s+__forceinline__)\s+[\w:<>\*& ]+?\b(\w+)\s*\(")


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n"), text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _function_bodies(text):
    """[(name, start offset, body text)] of every device function definition."""
    out = []
    for m in DEFINITION.finditer(text):
        i, depth = m.end(), 1
        while depth and i < len(text):  # the parameter list
            depth += {"(": 1, ")": -1}.get(text[i], 0)
            i += 1
        j = i
        while j < len(text) and text[j] in " \t\n":
            j += 1
        if j >= len(text) or text[j] != "{":
            continue  # a declaration
        k, depth = j + 1, 1
        while depth and k < len(text):
            depth += {"{": 1, "}": -1}.get(text[k], 0)
            k += 1
        out.append((m.group(1), m.start(), text[j:k]))
    return out


def _defined_in_both_arms(text):
    """Names of device functions defined in more than one arm of a conditional on ICAMD_HOST_EMULATION (a function whose
    BODY holds such a conditional is collected by collect_wrappers)."""
    names, stack, offset = set(), [], 0
    defs = [(name, start) for name, start, _ in _function_bodies(text)]
    for line in text.split("\n"):
        s = line.strip()
        if re.match(r"#\s*if", s):
            stack.append({"emul": "ICAMD_HOST_EMULATION" in s, "arm": 0, "start": offset, "seen": {}})
        elif re.match(r"#\s*(else|elif)", s) and stack:
            top = stack[-1]
            top["emul"] = top["emul"] or "ICAMD_HOST_EMULATION" in s
            for name, start in defs:
                if top["start"] <= start < offset:
                    top["seen"].setdefault(name, set()).add(top["arm"])
            top["arm"], top["start"] = top["arm"] + 1, offset
        elif re.match(r"#\s*endif", s) and stack:
            top = stack.pop()
            for name, start in defs:
                if top["start"] <= start < offset:
                    top["seen"].setdefault(name, set()).add(top["arm"])
            if top["emul"]:
                names |= {name for name, arms in top["seen"].items() if len(arms) > 1}
        offset += len(line) + 1
    return names


def collect_wrappers(text):
    text = _strip_comments(text)
    return _defined_in_both_arms(text) | {name for name, _, body in _function_bodies(text)
                                          if TRIGGERS.search(body) or "ICAMD_HOST_EMULATION" in body}


def test_the_scan_finds_a_wrapper_that_is_added_later():
    sample = """
    #if defined(ICAMD_HOST_EMULATION)
    ICAMD_DEV uint32_t brand_new(uint32_t a) { return a; }
    #else
    ICAMD_DEV uint32_t brand_new(uint32_t a) { return a + 0u; }
    #endif
    ICAMD_DEV uint32_t other_new(uint32_t a) { return __builtin_amdgcn_readfirstlane(a); }
    ICAMD_DEV uint32_t third_new(uint32_t a) { asm("v_not_b32 %0, %0" : "+v"(a)); return a; }
    ICAMD_DEV uint32_t barrier(uint32_t a) { asm volatile("" : "+v"(a)); return a; }
    ICAMD_DEV uint32_t plain(uint32_t a) { return a * 3u; }  // __builtin_amdgcn_ in a comment
    """
    assert collect_wrappers(sample) == {"brand_new", "other_new", "third_new"}


def test_every_wrapper_of_the_headers_is_in_the_list_or_exempt():
    found = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.h"))):
        with open(path) as f:
            for name in collect_wrappers(f.read()):
                found.setdefault(name, []).append(os.path.basename(path))
    assert len(found) >= 40, sorted(found)
    missing = {n: h for n, h in found.items() if n not in LISTED and n not in EXEMPT}
    assert not missing, "wrappers without a line in tests/device_probe/wrapper_ops.h: %s" % missing
    assert not set(EXEMPT) & LISTED and set(EXEMPT) <= set(found), sorted(set(EXEMPT) - set(found))
    # the list names the header that defines each wrapper
    for ident, name, arity, header in W.op_list() + [r for k in ("ICAMD_WRAPPER_FLOAT_OPS", "ICAMD_WRAPPER_LANE_OPS")
                                                      for r in W.parse_ops_header()[k]]:
        assert header in found.get(name, []), (ident, name, header, found.get(name))
