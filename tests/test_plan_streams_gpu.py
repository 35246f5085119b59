"""What the CPU trace of the transformer plans (tests/test_plan_trace_cpu.py) cannot see: on the GPU, every launch issued
inside a Branch.run goes to that branch's stream, everything else to the stream the step runs on, no two enabled branches
share a stream -- and the entry points an eager step calls are the ones the golden trace lists for the same case."""
import pytest
import torch

from tools import plan_trace

pytestmark = pytest.mark.gpu

# the dry-run wrapper of the grouped weight-gradient launch always names the plain entry; on the GPU the same launch
# carries the bias partial sums or the time-MLP rider (hip.linear_wgrad_slabs_multi)
SAME_LAUNCH = {"ib_linear_wgrad_slabs_multi_bias": "ib_linear_wgrad_slabs_multi",
               "ib_linear_wgrad_slabs_multi_tb": "ib_linear_wgrad_slabs_multi"}
# entry points that may refuse a shape (IB_E_UNSUPPORTED: nothing launched, no kernel family recorded) and the launch their
# wrapper's caller falls back to.  The dry-run library accepts every call, so the golden lists the attempt and no fallback:
# on the GPU the fallback right behind a refused attempt is taken out before the comparison, nothing else
FALLBACK = {"ib_linear_dgrad_wt": "ib_linear_dgrad", "ib_linear_panel_fwd": "ib_linear_fwd"}


def without_fallbacks(calls, paths):
    names, refused = [], None
    for (name, _), path in zip(calls, paths):
        if refused is not None and name == FALLBACK[refused]:
            refused = None
            continue
        refused = name if (name in FALLBACK and path == 0) else None
        names.append(SAME_LAUNCH.get(name, name))
    return names


def record(fn):
    """(the C-ABI calls of fn(), [(enabled branch, first call, end call)] of every Branch.run inside it)"""
    from inferbiomechanics_amd import hip, plans
    spans, run = [], plans.Branch.run
    with hip.record_launches() as rec:
        def marked_run(br, issue):
            if not br.on:                   # inline: on whatever stream the caller is on
                return run(br, issue)

            def marked():
                first = len(rec.calls)
                try:
                    issue()
                finally:
                    spans.append((br, first, len(rec.calls)))
            return run(br, marked)
        plans.Branch.run = marked_run
        try:
            fn()
            torch.cuda.synchronize()
        finally:
            plans.Branch.run = run
    return list(zip(rec.calls, rec.paths)), spans


def check(calls, spans, step_stream: int, branches, case: str, begin: str):
    assert calls and spans
    owner = [None] * len(calls)
    for br, first, end in spans:
        owner[first:end] = [br] * (end - first)
    for i, ((name, args), _) in enumerate(calls):
        stream = getattr(args[-1], "value", args[-1]) or 0
        want = owner[i].stream.cuda_stream if owner[i] is not None else step_stream
        assert stream == want, f"{case}: call {i} {name} on stream {stream:#x}, expected {want:#x} " \
                               f"({'branch ' + owner[i].name if owner[i] is not None else 'the step stream'})"
    on = {id(b): b for b in list(branches) + [br for br, _, _ in spans] if b.on}
    streams = [b.stream.cuda_stream for b in on.values()]
    assert len(set(streams)) == len(streams) and step_stream not in streams
    want = plan_trace.launch_names(plan_trace.load_golden()[case]["names"], begin)
    got = without_fallbacks([c for c, _ in calls], [p for _, p in calls])
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{case}: launch {i} is {g}, the golden has {w} (after {got[max(0, i - 3):i]})"
    assert len(got) == len(want)


@pytest.mark.parametrize("case", ["train_whole_layer", "train_token_panels"])
def test_training_step_streams_and_names(case):
    from inferbiomechanics_amd.engine import HipTrainer
    c, dev = plan_trace.TRAIN_CASES[case], torch.device("cuda", 0)
    torch.manual_seed(0)
    tr = HipTrainer(plan_trace._model(c, dev), "diffusion", "adam", 1e-3, use_graph=False)
    batch = plan_trace._batch(c, dev)
    tr.step(batch)
    calls, spans = record(lambda: tr.step(batch))
    assert any(br.name == "layer" for br, _, _ in spans) and any(br.name == "tr_wt" for br, _, _ in spans)
    check(calls, spans, tr.stream.cuda_stream, tr.plan.branches(), case, "begin:step")


def test_sampler_side_split_streams_and_names():
    from inferbiomechanics_amd.diffusion.sampler import DDIMSampler
    case = "sample_B84_side_split"
    c, dev = plan_trace.SAMPLER_CASES[case], torch.device("cuda", 0)
    torch.manual_seed(0)
    m = plan_trace._model(c, dev)
    sampler = DDIMSampler(m, num_sample_steps=4, use_graph=False)
    x = torch.randn(c["B"], c["T"], c["D"], generator=torch.Generator().manual_seed(2)).to(dev)
    sampler.sample(x)
    plan = m._get_plan(dev)
    assert plan.br_side.on
    calls, spans = record(lambda: sampler.sample(x))
    assert [br.name for br, _, _ in spans] == ["tr_side"] * 4            # one fork per denoise step
    check(calls, spans, sampler._stream.cuda_stream, plan.branches(), case, "begin:sample")
