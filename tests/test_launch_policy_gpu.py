"""The wiring of the launch policy: for every row of the recorded table (profiles/policy/step_info_parent.json, tools/dump_step_info.py)
a real context reports, through fx_step_info_ex, what the contexts of the recording reported -- the one-launch rows in full, the
refusals with their codes and messages.  The contexts are reused from row to row (the recording took a fresh one per row), so a
field of the launch record that kept an earlier step's value would show as well."""
import pytest

from tests.test_launch_policy import dump_step_info, recorded_rows


@pytest.mark.gpu
def test_every_row_on_a_real_context():
    recorded = {r["name"]: r for r in recorded_rows()}
    table = dump_step_info.table()
    assert [r["name"] for r in table] == list(recorded), "the table of tools/dump_step_info.py is not the recorded one"
    runner = dump_step_info.Runner(reuse=True)
    wrong = []
    try:
        for row in table:
            got, want = runner.run(row), recorded[row["name"]]
            for key in ("agents", "info", "error", "last_live", "info_second", "occupancy"):
                if got.get(key) != want.get(key):
                    wrong.append((row["name"], key, want.get(key), got.get(key)))
    finally:
        runner.close()
    assert not wrong, f"{len(wrong)} differences (row, what, recorded, reported): {wrong[:12]}"
