"""CPU: the digest tree's argument checks (check_digest_tree,
check_digest_tree_children, check_digest_tree_diff; csrc/api_args.hpp) and its
layout arithmetic (csrc/digest_hash.hpp) under ASan + UBSan.

The three device calls refuse a bad argument tuple on the host, before they touch
the device; the checks read arguments only, so
tests/cpp/test_api_args_digest_tree.cpp drives them with addresses taken from one
static buffer: accepted baselines, every required pointer NULL, every optional one
NULL, the mask range, each written array on each input and on each other written
array, and the identity form's n_max against the level.  host/Makefile builds it
(build/test_api_args_digest_tree, host code only, no libcrdtgpu.so); any sanitizer
report aborts with a non-zero exit."""

import os
import re
import subprocess

import crdtgpu


def test_digest_tree_argument_checks_under_sanitizers():
    exe = os.path.join(os.path.dirname(crdtgpu.__file__), "..", "host", "build", "test_api_args_digest_tree")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(os.path.dirname(exe)),
                               "build/test_api_args_digest_tree"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    m = re.fullmatch(r"ok: (\d+) cases in (\d+) families\n", r.stdout)
    assert m, r.stdout[-2000:]
    # the table as committed: a case that silently drops out changes these
    assert (int(m.group(1)), int(m.group(2))) == (CASES, 4)


CASES = 193
