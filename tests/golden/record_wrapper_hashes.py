"""Records tests/golden/gfx950_wrapper_hashes.json on an MI355X: one run of tests/device_probe/wrapper_probe over the operand
sets of tests/wrapper_cases.py, the SHA-256 of the device's results over each op's edge and control cases.  Run it when an op
or a set changes; tests/test_gpu_wrappers.py and tests/test_wrappers_host.py only ever compare with the file.

Some of the hashed cases lie outside the wrappers' stated domains, and the device forms of two ops reach them through C++
whose behaviour the language leaves undefined: `fastdiv` shifts by 32 for d = 0 and d > 2^31, `pk_lshr16` shifts 16-bit lanes
by 16 .. 31.  What is recorded for those is what hipcc's lowering to v_lshrrev_b32 / v_pk_lshrrev_b16 with a run-time count
gives; a compiler upgrade may legally change it, so read a mismatch on exactly these two ops with that in mind.

    python tests/golden/record_wrapper_hashes.py
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import wrapper_cases as W  # noqa: E402
import test_gpu_wrappers as G  # noqa: E402


def main():
    numbers = W.op_numbers()
    with tempfile.TemporaryDirectory() as d:
        device = G.run_probe(d)
        hashes = {name: W.digest(device["ops"][numbers[name]][:W.cases(name)[1]]) for name in W.OPS}
    with open(W.GOLDEN, "w") as f:
        json.dump({"device": "gfx950", "what": "SHA-256 of the device form's uint32 results (little-endian) over the edge and "
                   "control cases of tests/wrapper_cases.py; outside the stated domains fastdiv and pk_lshr16 rest on hipcc's "
                   "lowering of shifts C++ leaves undefined (tests/golden/record_wrapper_hashes.py)", "ops": hashes},
                  f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d ops in %s" % (len(hashes), W.GOLDEN))


if __name__ == "__main__":
    main()
