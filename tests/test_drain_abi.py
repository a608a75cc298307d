"""kbg_node_drain is part of the C ABI (include/kbgpu.h): the header compiles
as C, the row's size from a compiled C snippet is 64 bytes (16 x int32) and
equals the ctypes struct's with the same offsets, the addition left
KBG_ABI_VERSION at 13, and the call refuses what it must: a session without
kbg_options.reasons, a limit outside 1..512, a node or cordon index out of
range, nodes == NULL with another count than the session's, cordon == NULL
with a count, places == NULL with a capacity, too small a places_cap with the
need reported (through the CPU library of the hostsim tests, in a child process
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
  kbg_status (*fn)(kbg_session*, const int32_t*, int32_t, const int32_t*, int32_t, int32_t, kbg_node_drain_row*,
                   kbg_fit_place*, int32_t, int32_t*) = kbg_node_drain;
  (void)fn;
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(kbg_node_drain_row), offsetof(kbg_node_drain_row, tasks),
         offsetof(kbg_node_drain_row, unplaced), offsetof(kbg_node_drain_row, other_pods),
         offsetof(kbg_node_drain_row, jobs_moved), offsetof(kbg_node_drain_row, jobs_short),
         offsetof(kbg_node_drain_row, panic_nodes), offsetof(kbg_node_drain_row, place_off),
         offsetof(kbg_node_drain_row, reserved), KBG_ABI_VERSION);
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
    T = _abi.kbg_node_drain
    assert size == ctypes.sizeof(T) == 64
    assert offsets == [T.tasks.offset, T.unplaced.offset, T.other_pods.offset, T.jobs_moved.offset, T.jobs_short.offset,
                       T.panic_nodes.offset, T.place_off.offset, T.reserved.offset]
    assert version == 13


def test_abi_version_is_still_13():
    assert _abi.lib().kbg_abi_version() == 13


def test_message():
    from kbgpu.fixture import drain_message
    row = dict(valid=True, tasks=20, walked=20, placed_idle=16, placed_releasing=2, unplaced=2, first_unplaced=7713,
               nodes_used=5, other_pods=1, jobs_moved=4, jobs_short=1, affinity_now=False)
    assert drain_message(row) == ("18 of 20 pods find room (2 on releasing resources, 5 nodes); 2 do not, "
                                  "first task 7713; breaks 1 gang")
    assert drain_message(dict(row, valid=False)) == "not a live node"
    assert drain_message(dict(row, tasks=0, walked=0)).startswith("no pods to move")
    assert drain_message(dict(row, tasks=30)).endswith("; 10 not walked")


CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1])
import drain_session as ds
print(json.dumps(ds.check_refusals(ds.drain_fixture(ports=False))))
"""


def test_refusals():
    here = os.path.dirname(os.path.abspath(__file__))
    p = subprocess.run([sys.executable, "-c", CHILD, here], capture_output=True, text=True,
                       env=dict(os.environ, KBG_LIB_PATH=build_hostsim()))
    assert p.returncode == 0, p.stderr[-3000:]
    errs = json.loads(p.stdout.strip().splitlines()[-1])
    assert not errs, "\n".join(errs)
