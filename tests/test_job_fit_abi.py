"""kbg_job_fit's row and place structs are part of the C ABI (include/
kbgpu.h): their sizes and field offsets from a compiled C snippet equal the
ctypes structs', and the addition left KBG_ABI_VERSION at 13."""
import ctypes
import os
import shutil
import subprocess

import pytest

from kbgpu import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("valid", "job", "pending", "walked", "placed_idle", "placed_releasing", "first_unplaced", "nodes_used",
          "ready_num", "min_available", "ready_after", "queue_overused", "affinity_now", "panic_nodes", "place_off",
          "reserved")
PLACE = ("task", "node", "kind", "reserved")

SNIPPET = r"""
#include <stdio.h>
#include <stddef.h>
#include "kbgpu.h"
int main(void) {
  kbg_status (*fn)(kbg_session*, const int32_t*, int32_t, int32_t, struct kbg_job_fit*, kbg_fit_place*, int32_t,
                   int32_t*) = kbg_job_fit;
  kbg_job_fit_row row;
  (void)fn;
  (void)row;
  printf("%zu %zu %d %d", sizeof(struct kbg_job_fit), sizeof(kbg_fit_place), KBG_ABI_VERSION, KBG_FIT_MAX_LIMIT);
""" + "".join(f'  printf(" %zu", offsetof(struct kbg_job_fit, {f}));\n' for f in FIELDS) + \
    "".join(f'  printf(" %zu", offsetof(kbg_fit_place, {f}));\n' for f in PLACE) + r"""
  printf("\n");
  return 0;
}
"""


def test_struct_sizes_match_ctypes(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler: build() needs one too")
    src, exe = tmp_path / "t.c", tmp_path / "t"
    src.write_text(SNIPPET)
    lib_dir = os.path.dirname(_abi.lib()._name)
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", lib_dir,
                    "-l:" + os.path.basename(_abi.lib()._name), "-Wl,-rpath," + lib_dir], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    size, place, version, limit, *offsets = map(int, out)
    T, Q = _abi.kbg_job_fit, _abi.kbg_fit_place
    assert size == ctypes.sizeof(T) == 64 and place == ctypes.sizeof(Q) == 16 and version == 13
    assert [f for f, _ in T._fields_] == list(FIELDS) and [f for f, _ in Q._fields_] == list(PLACE)
    assert offsets[:16] == [getattr(T, f).offset for f in FIELDS] == [4 * i for i in range(16)]
    assert offsets[16:] == [getattr(Q, f).offset for f in PLACE] == [0, 4, 8, 12]
    assert limit == _abi.FIT_MAX_LIMIT == 512


def test_abi_version_is_still_13():
    assert _abi.lib().kbg_abi_version() == 13
