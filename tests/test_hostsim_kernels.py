"""The host launchers of hostsim (kube-arbitrator_amd/tools/hostsim_kernels.cpp:
a per-node, per-row restatement of every kbg::launch_*, the preempt / reclaim
victim scan and its prep included) against the references the GPU kernels are
held to: the seeded cases of tests/kernel_cases.py and tests/victim_ref.py
through the same probes (tools/kernel_probe.cpp, compiled against the
simulated HIP runtime), compared bit for bit by tests/kernel_ref.py's and
tests/victim_ref.py's comparators — covered words, info words, stop / panic
words, row_out bytes, prepped tables, sentinels and guards. CPU only: no test
here is marked gpu.

The probes run in one child process that loads no other kbg library
(tests/hostsim_worker.py), under the lazy schedule, where a launch runs only
when the probe synchronises its stream."""
import json
import os
import subprocess
import sys

import pytest

import kernel_cases as kc
import reasons_kernel_ref as rr
import victim_ref as vr
from helpers import build_hostsim
from test_victim_kernels_gpu import ILLEGAL

HERE = os.path.dirname(os.path.abspath(__file__))

IDS = (["firstfit/" + n for n in kc.FF_NAMES] +
       ["reject/" + k for k in ("rows0", "rows17", "complete1", "w_hi1000000", "tab_n1000000", "mw3", "split_words1")] +
       [f"scan_select/{n}-{m}" for n in sorted(kc.SCAN_CASES) for m in ("int", "gen")] +
       ["fitdelta/" + n for n in sorted(kc.FIT_CASES)] + ["apply", "mask_apply", "copy16"] +
       [f"stage_mask/n{n}" for n in rr.NODE_COUNTS] + ["reasons/" + n for n in sorted(rr.REASON_CASES)] +
       [f"victim/{n}-{m}" for n in vr.NAMES for m in ("mapped", "device")] +
       [f"victim_reject/{i:02d}-{what.replace(' ', '_')}" for i, (_, _, _, what) in enumerate(ILLEGAL)])


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    build_hostsim()
    out = str(tmp_path_factory.mktemp("hostsim") / "kernels.json")
    env = dict(os.environ, KBG_HOSTSIM_SCHEDULE="lazy")
    subprocess.run([sys.executable, os.path.join(HERE, "hostsim_worker.py"), "kernels", out], check=True, env=env)
    with open(out) as f:
        return json.load(f)


def test_every_case_ran(results):
    assert sorted(results) == sorted(IDS)


@pytest.mark.parametrize("case", IDS)
def test_host_launcher(results, case):
    """No difference from the reference (firstfit, scan_select, fitdelta,
    apply, mask_apply, copy16; stage_mask with launch_build_class_mask on the
    same tables, reasons, victim: the stop / panic words, row_out bytes and
    prepped tables of tests/victim_ref.py), or -2 without a byte written
    (reject, victim_reject)."""
    assert not results[case], "\n".join(results[case])
