"""CPU: the worklist digest's argument check (check_digest_idx, csrc/api_args.hpp)
under ASan + UBSan.

crdt_awset_digest_idx_async refuses a bad argument tuple on the host, before it
touches the device; the check reads descriptors only, so
tests/cpp/test_api_args_digest_idx.cpp drives it with addresses taken from one
static buffer: in both modes, with and without tombstones, at n_max = 2 and 0,
an accepted baseline, every required pointer NULL, R and mode out of range, the
document-count rule of each mode, and the digest and the list on every input
array.  host/Makefile builds it (build/test_api_args_digest_idx, host code only,
no libcrdtgpu.so); any sanitizer report aborts with a non-zero exit."""

import os
import re
import subprocess

import crdtgpu


def test_digest_idx_argument_check_under_sanitizers():
    exe = os.path.join(os.path.dirname(crdtgpu.__file__), "..", "host", "build", "test_api_args_digest_idx")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(os.path.dirname(exe)),
                               "build/test_api_args_digest_idx"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    m = re.fullmatch(r"ok: (\d+) cases in (\d+) families\n", r.stdout)
    assert m, r.stdout[-2000:]
    # the table as committed: a case that silently drops out changes these
    assert (int(m.group(1)), int(m.group(2))) == (496, 4)
