"""kbg_node_why is part of the C ABI (include/kbgpu.h): the header compiles as
C, the struct's size from a compiled C snippet is 128 bytes and equals the
ctypes struct's with the same offsets, the addition left KBG_ABI_VERSION at
13, and the call refuses what it must: a session without kbg_options.reasons,
a node index out of range, nodes == NULL with another count than the
session's (through the CPU library of the hostsim tests, in a child process
of its own: the refusals need a session, and a session needs a stream). No
other ABI test opens a session over a communicator, and this one does not
either."""
import ctypes
import json
import os
import shutil
import subprocess
import sys

import pytest

from helpers import build_hostsim
from kbgpu import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SNIPPET = r"""
#include <stdio.h>
#include <stddef.h>
#include "kbgpu.h"
int main(void) {
  kbg_status (*fn)(kbg_session*, const int32_t*, int32_t, kbg_node_why*) = kbg_node_reasons;
  (void)fn;
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(kbg_node_why), offsetof(kbg_node_why, pending),
         offsetof(kbg_node_why, count), offsetof(kbg_node_why, first_task), offsetof(kbg_node_why, idle_short),
         offsetof(kbg_node_why, open_idle), offsetof(kbg_node_why, idle_best_effort), offsetof(kbg_node_why, reserved),
         KBG_ABI_VERSION);
  return 0;
}
"""


def test_struct_size_matches_ctypes(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler: build() needs one too")
    src, exe = tmp_path / "t.c", tmp_path / "t"
    src.write_text(SNIPPET)
    lib_dir = os.path.dirname(_abi.lib()._name)
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", lib_dir,
                    "-l:" + os.path.basename(_abi.lib()._name), "-Wl,-rpath," + lib_dir], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    size, *offsets, version = map(int, out)
    T = _abi.kbg_node_why
    assert size == ctypes.sizeof(T) == 128
    assert offsets == [T.pending.offset, T.count.offset, T.first_task.offset, T.idle_short.offset, T.open_idle.offset,
                       T.idle_best_effort.offset, T.reserved.offset]
    assert version == 13


def test_abi_version_is_still_13():
    assert _abi.lib().kbg_abi_version() == 13


CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1])
import node_why_session as ns
import node_why_worker as nw
print(json.dumps(ns.check_refusals(nw.session_fixture("kat_task_why"))))
"""


def test_refusals():
    here = os.path.dirname(os.path.abspath(__file__))
    p = subprocess.run([sys.executable, "-c", CHILD, here], capture_output=True, text=True,
                       env=dict(os.environ, KBG_LIB_PATH=build_hostsim()))
    assert p.returncode == 0, p.stderr[-3000:]
    errs = json.loads(p.stdout.strip().splitlines()[-1])
    assert not errs, "\n".join(errs)
