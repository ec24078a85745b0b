"""CPU: the C ABI's argument checks (csrc/api_args.hpp) under ASan + UBSan.

Every *_async entry point refuses a bad argument tuple on the host, before it
touches the device; the checks read descriptors only, so
tests/cpp/test_api_args.cpp drives them with addresses taken from one static
buffer: per check_* family an accepted baseline, every required / optional
pointer NULL, every two written arrays at one address, sized arrays one
element inside each other and exactly adjacent, every written array on every
input array, at n_docs = 1 and n_docs = 0, plus the differences between the
families pinned as they are.  host/Makefile builds it (build/test_api_args,
host code only, no libcrdtgpu.so); any sanitizer report aborts with a
non-zero exit."""

import os
import re
import subprocess

import crdtgpu


def test_argument_checks_under_sanitizers():
    exe = os.path.join(os.path.dirname(crdtgpu.__file__), "..", "host", "build", "test_api_args")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(os.path.dirname(exe)), "build/test_api_args"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    m = re.fullmatch(r"ok: (\d+) cases in (\d+) families\n", r.stdout)
    assert m, r.stdout[-2000:]
    # the table as committed: a row or a case that silently drops out changes these
    assert (int(m.group(1)), int(m.group(2))) == (21031, 43)
