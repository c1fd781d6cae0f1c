"""Runs the REFERENCE's own tests/agents_tests/test_trpo.py against pfrl_amd through
tools/run_reference_tests.py (``import pfrl`` -> ``pfrl_amd``), as test_reference_suite.py does for
the other agents: the Hessian-vector product helpers and the host route of ``pfrl_amd.agents.TRPO``
(feed-forward and recurrent, discrete and continuous, with and without a normaliser).  Only where the
reference is mounted (the build container); skipped on the GPU box."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("PFRL_REFERENCE", "/root/reference")


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "tests")),
                    reason="the reference is not mounted here")
def test_reference_trpo_tests_pass_against_pfrl_amd(tmp_path):
    log = tmp_path / "reference_trpo_tests.log"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "run_reference_tests.py"), "--timeout", "300",
           "-m", "not slow and not gpu", "tests/agents_tests/test_trpo.py"]
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    with open(log, "w") as out:       # a file, not a pipe: see the runner's docstring
        proc = subprocess.run(cmd, stdout=out, stderr=subprocess.STDOUT, env=env, cwd=str(tmp_path),
                              timeout=1500, start_new_session=True)
    text = open(log).read()
    summary = [line for line in text.splitlines() if re.search(r"\d+ (passed|failed)", line)]
    assert summary, text[-3000:]
    assert proc.returncode == 0 and "failed" not in summary[-1] and " error" not in summary[-1], \
        text[-4000:]
    # 2 Hessian-vector product tests + (96 + 4) parameter sets x (single env, batch of envs)
    assert int(re.search(r"(\d+) passed", summary[-1]).group(1)) == 202, summary[-1]
