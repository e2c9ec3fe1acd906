"""What the four batched entries beside the plan step hand to their launchers for 129 agents, without a GPU (DESIGN.md section 2,
"Beyond one wave of agents"): a stand-alone program (tests/batch_staging.cpp, built the way tests/test_context_owners.py builds its
program) links the library's host sources against malloc-backed fakes of the HIP runtime and launcher stubs that keep their
argument, creates a context of 129 agents, uploads and "evaluates" 129 problems, and calls fx_eval_prediction_prob_batch,
fx_eval_responsibility_cost_batch, fx_eval_risk_batch and fx_eval_risk_costs_batch over all agents and over a list given out of
order.  It holds agent_row[], the rows, item0[] / fin0[], blk0[] (by agent, and compact over the agents with cost parameters) and
seg_blk0[] to their expected values, every table and every row's memory to ONE live device block, and fx_device_bytes to the
fakes' table."""
import subprocess

from tests.test_context_owners import build_host_program


def test_batch_staging(tmp_path):
    run = subprocess.run([build_host_program("batch_staging", tmp_path)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok (129 agents, 8 batched launches)"), run.stdout[-4000:] + run.stderr[-2000:]
