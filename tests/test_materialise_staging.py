"""What fx_materialise_candidates_batch hands to the list launcher for 129 agents, without a GPU: a
stand-alone program (tests/materialise_staging.cpp, built the way tests/test_batch_staging.py builds its program) links the library's
host sources against malloc-backed fakes of the HIP runtime that count their calls and a stub of fx_launch_eval_list that keeps its
arguments, creates a context of 129 agents, uploads and "evaluates" 129 select-only problems, and makes the call over all agents
and over a list given out of order, at 1 and at 32 lanes.  It holds the launches' variants, the row table, each clone's C, ld,
n_blocks and mode bits, every clone's outputs to the agent's ONE live device block, the uploaded lists to ascending and
de-duplicated, fx_device_bytes to the fakes' table, a refused call to changing nothing, and the runtime calls of a repeated call
to the same count for 3 agents as for 129."""
import re
import subprocess

from tests.test_context_owners import build_host_program


def test_materialise_staging(tmp_path):
    run = subprocess.run([build_host_program("materialise_staging", tmp_path)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok (129 agents, "), run.stdout[-4000:] + run.stderr[-2000:]
    # one wait, one upload, and per launch nothing the fakes see (the launcher is a stub here): the count DESIGN.md section 22 gives
    calls = int(re.search(r"(\d+) runtime calls per repeated call", run.stdout).group(1))
    assert calls == 3, run.stdout
