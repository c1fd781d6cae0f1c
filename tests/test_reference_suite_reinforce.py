"""Runs the REFERENCE's own tests/agents_tests/test_reinforce.py against pfrl_amd through
tools/run_reference_tests.py (``import pfrl`` -> ``pfrl_amd``), as test_reference_suite_trpo.py does for
TRPO: the host route of ``pfrl_amd.agents.REINFORCE`` (feed-forward and recurrent, discrete and
continuous, ``batchsize`` 1 and 10, with and without ``backward_separately``) under
``train_agent_with_evaluation``.  Only where the reference is mounted (the build container); skipped on
the GPU box."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("PFRL_REFERENCE", "/root/reference")


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "tests")),
                    reason="the reference is not mounted here")
def test_reference_reinforce_tests_pass_against_pfrl_amd(tmp_path):
    log = tmp_path / "reference_reinforce_tests.log"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "run_reference_tests.py"), "--timeout", "300",
           "-m", "not slow and not gpu", "tests/agents_tests/test_reinforce.py"]
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    with open(log, "w") as out:       # a file, not a pipe: see the runner's docstring
        proc = subprocess.run(cmd, stdout=out, stderr=subprocess.STDOUT, env=env, cwd=str(tmp_path),
                              timeout=600, start_new_session=True)
    text = open(log).read()
    summary = [line for line in text.splitlines() if re.search(r"\d+ (passed|failed)", line)]
    assert summary, text[-3000:]
    assert proc.returncode == 0 and "failed" not in summary[-1] and " error" not in summary[-1], \
        text[-4000:]
    # test_abc_fast_cpu x {discrete, continuous} x {LSTM, feed-forward} x {batchsize 1, 10} x
    # {backward_separately or not}: the same selection run against the reference itself reports
    # "16 passed, 48 deselected"
    assert int(re.search(r"(\d+) passed", summary[-1]).group(1)) == 16, summary[-1]
