"""The samplers' launch sequence, signature and buffers against tests/golden/sampler_traces.json (tools/sampler_trace.py:
every C-ABI call of the four sampler classes and of DiffusionLabelPredictor's paths, in dry-run on CPU tensors, with the
sampler's `_sig` and `_bufs` after every call).  A refactor of diffusion/sampler.py must leave every trace as it is; a change
that moves a launch on purpose regenerates the golden file with `python tools/sampler_trace.py --write` and says so.

And what a refused call leaves behind: nothing -- the next good call's trace is a fresh sampler's first."""
import pytest
import torch

from tools import sampler_trace
from tools.plan_trace import _Trace, summary


@pytest.fixture(scope="module")
def golden():
    return sampler_trace.load_golden()


def test_golden_lists_every_case(golden):
    assert list(golden) == list(sampler_trace.cases())


@pytest.mark.parametrize("case", list(sampler_trace.cases()))
def test_sampler_trace(case, golden):
    got = summary(sampler_trace.trace_case(case))
    want = golden[case]
    for i, (g, w) in enumerate(zip(got["names"], want["names"])):
        assert g == w, f"{case}: entry {i} is {g}, the golden has {w} (after {got['names'][max(0, i - 3):i]})"
    assert len(got["names"]) == len(want["names"])
    # same names, another hash: an argument, the buffer-reuse pattern, the signature or a buffer moved --
    # `tools/sampler_trace.py --dump` shows where
    assert got["sha256"] == want["sha256"]


T, D, F = sampler_trace.SMALL["T"], sampler_trace.SMALL["D"], 17


def _samplers():
    """(name, make(model), good call, refused calls) per class: the refusals come mid-way, after the call has begun"""
    from inferbiomechanics_amd.diffusion import sampler as S
    mask = torch.zeros(T, D, dtype=torch.bool)
    mask[:, :20] = True
    cols = mask[0].clone()
    x, o = torch.zeros(3, T, D), torch.ones(3, T, D)
    z, q = torch.zeros(2, F, D), torch.ones(2, F, D)
    return [
        ("DDIMSampler", lambda m: S.DDIMSampler(m, 5, eta=0.5, seed=1),
         lambda s: s.sample(x), [lambda s: s.sample(x, window_ids=[1, 2])]),
        ("ConditionalDDIMSampler", lambda m: S.ConditionalDDIMSampler(m, 5, eta=0.5, seed=1),
         lambda s: s.sample(x, o, mask), [lambda s: s.sample(x, o, mask, window_ids=[1, 2]),
                                          lambda s: s.sample(x, o[:2], mask)]),
        ("StitchedDDIMSampler", lambda m: S.StitchedDDIMSampler(m, 5, hop=3),
         lambda s: s.sample(z, q, cols), [lambda s: s.sample(z, q[:, :9], cols)]),
        ("StochasticStitchedSampler", lambda m: S.StochasticStitchedSampler(m, 5, eta=0.5, hop=3, seed=1),
         lambda s: s.sample(z, q, cols), [lambda s: s.sample(z, q, cols, trial_ids=[1, 2, 3]),
                                          lambda s: s.sample(z, q[:, :9], cols)]),
    ]


@pytest.mark.parametrize("which", range(4), ids=[s[0] for s in _samplers()])
def test_a_refused_call_leaves_the_sampler_as_it_was(which):
    """a wrong id count (the stochastic classes) and an `observed` of the wrong shape (the masked ones) are refused after
    the call has begun; the good call that follows issues exactly what a fresh sampler's first call issues, and ends with
    the same signature and buffers"""
    _, make, good, refused = _samplers()[which]

    def first_good_call(after_refusals: bool):
        with _Trace() as tr, sampler_trace.Run(tr) as r:
            sampler = make(r.model(torch.bfloat16, D, T))
            if after_refusals:
                for bad in refused:
                    with pytest.raises(ValueError):
                        bad(sampler)
                del tr.log[:]
            good(sampler)
            return tr.canonical()
    fresh, after = first_good_call(False), first_good_call(True)
    assert [e for e in fresh if e[0] == "state:sig"] and fresh[0] == "begin:sample"
    assert after == fresh
