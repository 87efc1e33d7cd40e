"""GPU tier: the host twins of the instruction wrappers are pinned to the device, op by op.

One run of tests/device_probe/wrapper_probe (a stand-alone HIP program, built by tests/cxx/Makefile) applies the DEVICE form of
every wrapper of tests/device_probe/wrapper_ops.h to the operand sets of tests/wrapper_cases.py.  Per op: device == twin on all
cases, inside and outside the stated domain, bit for bit; device == plain definition inside the domain; and the SHA-256 of the
device's results over edges + control is the entry of tests/golden/gfx950_wrapper_hashes.json, which lets the CPU tier
(tests/test_wrappers_host.py) hold the twins to the hardware's answers everywhere.  The same run returns the float first
guesses of the normal-map filter (v_sqrt_f32, v_rcp_f32) over everything the filter can form, and the lane forms (wave_all,
wave_count, quad_xor1, quad_xor2) in one wave of 64.

tests/golden/record_wrapper_hashes.py records the golden file from one probe run; this test only ever compares."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import ic_testlib as T
import wrapper_cases as W
from test_wrappers_host import build_wrapper_emul, twin_apply

pytestmark = pytest.mark.gpu

CXX_DIR = os.path.join(T.ROOT, "tests", "cxx")
PROBE = os.path.join(CXX_DIR, "build", "wrapper_probe")
CSRC = os.path.join(T.ROOT, "image-compression_amd", "csrc")


def probe_binary():
    """The probe, rebuilt when it is missing or older than its sources and hipcc is on PATH."""
    sources = [os.path.join(T.ROOT, "tests", "device_probe", f) for f in ("wrapper_probe.hip", "wrapper_ops.h")]
    sources += [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".inc"))]
    stale = not os.path.exists(PROBE) or os.path.getmtime(PROBE) < max(os.path.getmtime(s) for s in sources)
    if stale and shutil.which("hipcc"):
        subprocess.check_call(["make", "-C", CXX_DIR, PROBE], stdout=subprocess.DEVNULL)
    elif not os.path.exists(PROBE):
        pytest.fail("tests/cxx/build/wrapper_probe is not built and there is no hipcc on PATH to build it", pytrace=False)
    return PROBE


def write_input(path):
    numbers = W.op_numbers()
    with open(path, "wb") as f:
        def put(*words):
            np.array(words, "<u4").tofile(f)
        for name in sorted(W.OPS, key=numbers.get):
            operands, _ = W.cases(name)
            put(1, numbers[name], len(operands))
            operands.astype("<u4").tofile(f)
        votes = W.vote_cases()
        put(2, len(votes))
        for ex, pred in votes:
            put(ex & 0xffffffff, ex >> 32, pred & 0xffffffff, pred >> 32)
        put(3)
        W.quad_values().astype("<u4").tofile(f)
        put(4)
        put(0)


def read_output(path):
    """{"ops": {number: results}, "votes": [n, 2, 64], "quad": [2, 64], "guess": {set: (guess, settled)}}; the large float
    sections stay memory-mapped."""
    words = np.memmap(path, dtype="<u4", mode="r")
    out, at = {"ops": {}, "guess": {}}, 0
    while True:
        tag = int(words[at])
        at += 1
        if tag == 0:
            break
        if tag == 1:
            op, n = int(words[at]), int(words[at + 1])
            out["ops"][op] = np.array(words[at + 2:at + 2 + n])
            at += 2 + n
        elif tag == 2:
            n = int(words[at])
            out["votes"] = np.array(words[at + 1:at + 1 + 128 * n]).reshape(n, 2, 64)
            at += 1 + 128 * n
        elif tag == 3:
            out["quad"] = np.array(words[at:at + 128]).reshape(2, 64)
            at += 128
        elif tag == 4:
            for which in W.GUESS_SETS:
                n = int(words[at])
                assert n == W.guess_count(which), (which, n)
                out["guess"][which] = (words[at + 1:at + 1 + n], words[at + 1 + n:at + 1 + 2 * n])
                at += 1 + 2 * n
        else:
            raise AssertionError("unknown section %d in the probe's output" % tag)
    assert at == len(words)
    return out


def run_probe(directory):
    exe = probe_binary()
    src, dst = os.path.join(str(directory), "in.bin"), os.path.join(str(directory), "out.bin")
    write_input(src)
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout.decode()[-2000:], r.stderr.decode()[-4000:])
    os.remove(src)
    return read_output(dst)


@pytest.fixture(scope="module")
def device(tmp_path_factory):
    """The one probe run.  A non-zero exit or a timeout fails here, and nothing else is started."""
    return run_probe(tmp_path_factory.mktemp("wrapper_probe"))


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return build_wrapper_emul(tmp_path_factory.mktemp("wrappers_gpu"))


def test_every_op_device_twin_definition_and_recorded_hash(device, emul):
    numbers = W.op_numbers()
    hashes, problems = {}, []
    for name in sorted(W.OPS, key=numbers.get):
        operands, n_fixed = W.cases(name)
        got = device["ops"][numbers[name]]
        assert len(got) == len(operands), name
        inside = W.domain_mask(name, operands)
        if name.startswith("scan_plain"):  # the second device build has no twin: the twin models the build the kernels run
            twin, where = twin_apply(emul, name.replace("scan_plain", "scan"), operands), inside
        else:
            twin, where = twin_apply(emul, name, operands), np.ones(len(operands), bool)
        problems.append(W.first_difference(name, operands[where], got[where], twin[where], "device and twin"))
        problems.append(W.first_difference(name, operands[inside], got[inside], W.expected(name, operands[inside]),
                                           "device and definition (in domain)"))
        hashes[name] = W.digest(got[:n_fixed])
        print("%-18s %7d cases, %7d in domain, edges + control %s" % (name, len(operands), inside.sum(), hashes[name][:16]))
    with open(W.GOLDEN) as f:
        golden = json.load(f)["ops"]
    problems += ["%s: the device's hash %s is not the recorded %s" % (n, h, golden.get(n)) for n, h in hashes.items()
                 if golden.get(n) != h]
    problems = [p for p in problems if p]
    assert not problems, "\n".join(problems)


def test_the_float_first_guesses_are_within_one_and_settle_exactly(device):
    """mip_normal.h: "the truncated guess is the floor or its neighbour", over everything the filter can form."""
    for which in W.GUESS_SETS:
        guess, settled = device["guess"][which]
        total, chunk = W.guess_count(which), 1 << 22
        hist, wrong = {-1: 0, 0: 0, 1: 0}, 0
        for first in range(0, total, chunk):
            count = min(chunk, total - first)
            n, d = W.guess_operands(which, first, count)
            exact = W.exact_floor(n, d)
            err = np.asarray(guess[first:first + count]).astype(np.int64) - exact
            bad = np.flatnonzero(np.abs(err) > 1)
            assert not len(bad), (which, "guess", int(n[bad[0]]), None if d is None else int(d[bad[0]]), int(err[bad[0]]))
            for e in hist:
                hist[e] += int((err == e).sum())
            bad = np.flatnonzero(np.asarray(settled[first:first + count]).astype(np.int64) != exact)
            assert not len(bad), (which, "settled", int(n[bad[0]]), None if d is None else int(d[bad[0]]))
        assert sum(hist.values()) == total
        print("guess error %-13s %9d cases: -1: %d, 0: %d, +1: %d" % (which, total, hist[-1], hist[0], hist[1]))


def test_votes_with_lanes_that_returned_early(device):
    votes = W.vote_cases()
    assert device["votes"].shape == (len(votes), 2, 64)
    for i, (ex, pred) in enumerate(votes):
        want_all, want_count = W.vote_expected(ex, pred)
        assert (device["votes"][i, 0] == want_all).all(), ("wave_all", hex(ex), hex(pred), device["votes"][i, 0], want_all)
        assert (device["votes"][i, 1] == want_count).all(), ("wave_count", hex(ex), hex(pred), device["votes"][i, 1], want_count)


def test_quad_permutes_in_full_quads(device):
    v = W.quad_values()
    lanes = np.arange(64)
    assert (device["quad"][0] == v[lanes ^ 1]).all(), ("quad_xor1", device["quad"][0], v[lanes ^ 1])
    assert (device["quad"][1] == v[lanes ^ 2]).all(), ("quad_xor2", device["quad"][1], v[lanes ^ 2])
