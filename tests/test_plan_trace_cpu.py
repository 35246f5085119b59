"""The transformer plans' launch sequence against tests/golden/plan_traces.json (tools/plan_trace.py: every C-ABI call of
every tier, tuning switch, data-parallel flush order and sampler tier, in dry-run on CPU tensors).  A refactor of plans.py
must leave every trace as it is; a change that moves a launch on purpose regenerates the golden file with
`python tools/plan_trace.py --write` and says so."""
import pytest

from tools import plan_trace


@pytest.fixture(scope="module")
def golden():
    return plan_trace.load_golden()


def test_golden_lists_every_case(golden):
    assert list(golden) == list(plan_trace.cases())


@pytest.mark.parametrize("case", list(plan_trace.cases()))
def test_plan_trace(case, golden):
    got = plan_trace.summary(plan_trace.trace_case(case))
    want = golden[case]
    for i, (g, w) in enumerate(zip(got["names"], want["names"])):
        assert g == w, f"{case}: entry {i} is {g}, the golden has {w} (after {got['names'][max(0, i - 3):i]})"
    assert len(got["names"]) == len(want["names"])
    # same names, another hash: an argument or the buffer-reuse pattern moved -- `tools/plan_trace.py --dump` shows where
    assert got["sha256"] == want["sha256"]


def test_data_parallel_cases_flush_and_report(golden):
    """what the data-parallel cases are there to pin: 12 gradients per layer + 9 of the ends, twice; a flush per layer
    boundary + the ends when every layer reports itself, fewer when the layers' launches lag a layer"""
    for name, flushes in (("ddp_whole_layer_lagged", 6), ("ddp_whole_layer+no_lag_group", 10),
                          ("ddp_token_panels_lagged", 6), ("ddp_token_panels+no_lag_group", 10)):
        names = golden[name]["names"]
        assert sum(n.startswith("ready:") for n in names) == 90 and names.count("flush") == flushes
