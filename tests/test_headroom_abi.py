"""kbg_task_room is part of the C ABI (include/kbgpu.h): its size and field
offsets from a compiled C snippet equal the ctypes struct's, and the addition
left KBG_ABI_VERSION at 13."""
import ctypes
import os
import shutil
import subprocess

import pytest

from kbgpu import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("valid", "task", "best_effort", "queue_overused", "limit", "nodes_pass", "copies_idle", "copies_releasing",
          "nodes_idle", "nodes_releasing_only", "first_node", "max_node_copies", "limit_hit", "affinity_now",
          "panic_nodes", "reserved")

SNIPPET = r"""
#include <stdio.h>
#include <stddef.h>
#include "kbgpu.h"
int main(void) {
  kbg_status (*fn)(kbg_session*, const int32_t*, int32_t, int32_t, kbg_task_room*) = kbg_task_headroom;
  (void)fn;
  printf("%zu %d", sizeof(kbg_task_room), KBG_ABI_VERSION);
""" + "".join(f'  printf(" %zu", offsetof(kbg_task_room, {f}));\n' for f in FIELDS) + r"""
  printf("\n");
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
    size, version, *offsets = map(int, out)
    T = _abi.kbg_task_room
    assert size == ctypes.sizeof(T) == 16 * 4 and version == 13
    assert [f for f, _ in T._fields_] == list(FIELDS)
    assert offsets == [getattr(T, f).offset for f in FIELDS] == [4 * i for i in range(16)]
    assert _abi.ROOM_MAX_LIMIT == 1024


def test_abi_version_is_still_13():
    assert _abi.lib().kbg_abi_version() == 13
