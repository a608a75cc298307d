"""kbg_task_why is part of the C ABI (include/kbgpu.h): its size from a
compiled C snippet equals the ctypes struct's, the cause codes agree, and the
addition left KBG_ABI_VERSION at 13."""
import ctypes
import os
import shutil
import subprocess

import pytest

from kbgpu import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SNIPPET = r"""
#include <stdio.h>
#include <stddef.h>
#include "kbgpu.h"
int main(void) {
  kbg_status (*fn)(kbg_session*, const int32_t*, int32_t, kbg_task_why*) = kbg_task_reasons;
  (void)fn;
  printf("%zu %zu %zu %zu %d %d %d %d %d %d\n", sizeof(kbg_task_why), offsetof(kbg_task_why, count),
         offsetof(kbg_task_why, first_node), offsetof(kbg_task_why, idle_short), KBG_TWHY_FITS_IDLE,
         KBG_TWHY_FITS_RELEASING, KBG_TWHY_SHORT, KBG_TWHY_PANIC, KBG_TWHY_COUNT, KBG_ABI_VERSION);
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
    size, o_count, o_first, o_short, *codes = map(int, out)
    T = _abi.kbg_task_why
    assert size == ctypes.sizeof(T) == 31 * 4
    assert (o_count, o_first, o_short) == (T.count.offset, T.first_node.offset, T.idle_short.offset)
    assert codes == [_abi.TWHY_FITS_IDLE, _abi.TWHY_FITS_RELEASING, _abi.TWHY_SHORT, _abi.TWHY_PANIC, _abi.TWHY_COUNT, 13]


def test_abi_version_is_still_13():
    assert _abi.lib().kbg_abi_version() == 13
