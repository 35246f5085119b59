#!/usr/bin/env python3
"""The launch sequence of the samplers, pinned as tools/plan_trace.py pins the plans': for a fixed list of cases (the four
sampler classes of diffusion/sampler.py over their solvers, grids, eta, observation kinds, dtypes and trial lengths, and
DiffusionLabelPredictor's four paths) the canonical trace of every C-ABI call, taken on CPU tensors in dry-run mode.

The entries are plan_trace's (its _Trace, canonical and summary are reused).  "begin:sample" stands before every call of a
sampler's sample(), and after every sample() that returns come two entries of the sampler's state:
  * ["state:sig", ...]   the sampler's `_sig`, element by element: every address as its "p<k>", dtypes and strings as text;
  * ["state:bufs", [key, shape, dtype], ...]  the `_bufs` in key order (a tuple of tensors: a list of [shape, dtype]).
Tests index `_sig` from its end and read `_bufs` by key: the golden file makes that layout a stated contract.

Every case runs, on ONE sampler object: a call, a second call of the same shape with new data (the buffers are reused),
where eta > 0 a third with explicit ids, a call with another batch size (a new signature), one sample_noise call.

tests/golden/sampler_traces.json holds, per case, the names in full and the sha256 of the whole canonical trace;
tests/test_sampler_trace_cpu.py holds diffusion/sampler.py to it.  A refactor of the samplers leaves the file alone.
The cases repeat the same few runs of names (a denoise step, a call's head) thousands of times, so the file keeps every
distinct run once ("chunks") and a case's names as indices into them (pack / unpack).

  python tools/sampler_trace.py            # compare with the golden file, print the cases that differ
  python tools/sampler_trace.py --write    # rewrite tests/golden/sampler_traces.json
  python tools/sampler_trace.py --dump DIR # one <case>.json per case with the full canonical trace
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.plan_trace import _Trace, summary  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "sampler_traces.json")

S = 5                                       # sampling steps of every case
SMALL = dict(D=44, T=8)                     # the plumbing tests' small denoiser; bf16 pitches its state (Dp = 64), fp32 does not
LABELS = dict(D=177, T=10)                  # DiffusionLabelPredictor's row: 147 input columns + 30 label columns
DTYPES = (("bf16", torch.bfloat16), ("fp32", torch.float32))
SETTINGS = (("ddim", "time", 0.0), ("ddim", "time", 0.5), ("dpmpp2m", "logsnr", 0.0), ("dpmpp2m_sde", "logsnr", 0.5),
            ("dpmpp2m_sde", "logsnr", 0.0))
COND_COLS = 14
N_TRIALS, HOP = 2, 3
TRIAL_FRAMES = (17, 8)                      # four windows with a ragged last one; one window (F == T)


class Run:
    """How the cases run: on which device, with or without the captured step, and who hears of it.  `tr` gets the markers
    and the state entries (a _Trace; None: nobody), `sink` every sample()'s result (the A/B job hashes them)."""

    def __init__(self, tr=None, device=None, use_graph=False, sink=None):
        self.tr, self.device, self.use_graph, self.sink = tr, device, use_graph, sink
        self.gen = torch.Generator().manual_seed(7)
        self._depth = 0

    def randn(self, *shape):
        return torch.randn(*shape, generator=self.gen)

    def model(self, dtype, D, T, cond_cols=0):
        from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
        torch.manual_seed(0)
        m = DiffusionTransformer(D, T, d_model=64, num_heads=4, dim_feedforward=128, num_layers=2, compute_dtype=dtype,
                                 device=self.device)
        m.cond_cols = cond_cols
        return m

    def __enter__(self):
        """every OUTERMOST sample() of the four classes is marked, and the sampler's state recorded when it returns"""
        from inferbiomechanics_amd.diffusion import sampler as mod
        self._saved = [(c, c.__dict__["sample"]) for c in (mod.DDIMSampler, mod.ConditionalDDIMSampler,
                                                             mod.StitchedDDIMSampler, mod.StochasticStitchedSampler)
                       if "sample" in c.__dict__]
        for cls, fn in self._saved:
            cls.sample = self._watched(fn)
        return self

    def __exit__(self, *exc):
        for cls, fn in self._saved:
            cls.sample = fn
        return False

    def _watched(self, fn):
        def sample(sampler, *a, **kw):
            if self._depth:
                return fn(sampler, *a, **kw)
            if self.tr is not None:
                self.tr.mark("begin:sample")
            self._depth += 1
            try:
                out = fn(sampler, *a, **kw)
            finally:
                self._depth -= 1
            if self.tr is not None:
                self.tr.log.append(("state:sig", list(sampler._sig)))
                self.tr.log.append(("state:bufs", [[k] + _shape(b) for k, b in sorted(sampler._bufs.items())]))
            if self.sink is not None:
                self.sink(out)
            return out
        return sample


def _shape(b):
    if isinstance(b, torch.Tensor):
        return [list(b.shape), b.dtype]
    return [[list(t.shape), t.dtype] for t in b]


def _sequence(r, eta, call, noise, batches=(3, 2)):
    """the calls of one case: call(batch, ids) / noise(batch) run the sampler's sample / sample_noise"""
    B, other = batches
    call(B, None)
    call(B, None)
    if eta > 0.0:
        call(B, [9, 4, 11][:B])
    call(other, None)
    noise(other)


def _window(r, cls_name, dtype, solver, spacing, eta):
    from inferbiomechanics_amd.diffusion import sampler as mod
    m = r.model(dtype, **SMALL)
    D, T = SMALL["D"], SMALL["T"]
    sampler = getattr(mod, cls_name)(m, S, use_graph=r.use_graph, eta=eta, seed=5, solver=solver, spacing=spacing)
    if cls_name == "DDIMSampler":
        _sequence(r, eta, lambda B, ids: sampler.sample(r.randn(B, T, D), window_ids=ids),
                  lambda B: sampler.sample_noise(B, T, D, seed=3, draw=1))
    else:
        mask = torch.zeros(T, D, dtype=torch.bool)
        mask[:, :20] = True
        mask[2, 30] = True
        _sequence(r, eta, lambda B, ids: sampler.sample(r.randn(B, T, D), r.randn(B, T, D), mask, window_ids=ids),
                  lambda B: sampler.sample_noise(B, T, D, r.randn(B, T, D), mask, seed=3, draw=1))


def _clean_then_noised(r, dtype):
    """observations = 'clean' on a model trained with cond_cols, then the same object switched to 'noised'"""
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler
    m = r.model(dtype, cond_cols=COND_COLS, **SMALL)
    D, T = SMALL["D"], SMALL["T"]
    sampler = ConditionalDDIMSampler(m, S, use_graph=r.use_graph, observations="clean")
    mask = torch.zeros(T, D, dtype=torch.bool)
    mask[:, :COND_COLS] = True
    call = lambda B, ids: sampler.sample(r.randn(B, T, D), r.randn(B, T, D), mask, window_ids=ids)
    noise = lambda B: sampler.sample_noise(B, T, D, r.randn(B, T, D), mask, seed=3, draw=1)
    _sequence(r, 0.0, call, noise)
    sampler.observations = "noised"
    _sequence(r, 0.0, call, noise)


def _trial(r, dtype, F, observed, solver, spacing, eta=None):
    """StitchedDDIMSampler (eta None) or StochasticStitchedSampler over trials of F frames"""
    from inferbiomechanics_amd.diffusion.sampler import StitchedDDIMSampler, StochasticStitchedSampler
    m = r.model(dtype, **SMALL)
    D = SMALL["D"]
    if eta is None:
        sampler = StitchedDDIMSampler(m, S, hop=HOP, use_graph=r.use_graph, solver=solver, spacing=spacing, seed=5)
        ids = lambda i: {}
    else:
        sampler = StochasticStitchedSampler(m, S, eta=eta, hop=HOP, use_graph=r.use_graph, spacing=spacing, seed=5,
                                            solver=solver)
        ids = lambda i: {"trial_ids": i}
    cols = torch.zeros(D, dtype=torch.bool)
    cols[:20] = True
    obs = lambda N: (r.randn(N, F, D), cols) if observed else (None, None)
    _sequence(r, eta or 0.0, lambda N, i: sampler.sample(r.randn(N, F, D), *obs(N), **ids(i)),
              lambda N: sampler.sample_noise(N, F, D, *obs(N), seed=3, draw=1), batches=(N_TRIALS, 3))


def _label_inputs(r, n, frames):
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import SyntheticWindowDataset
    ds = SyntheticWindowDataset(4, 50, 5)                              # windows of 10 frames
    items = [ds[i] for i in range(4)]
    if frames == 10:
        return {k: torch.stack([it[0][k] for it in items[:n]]) for k in items[0][0]}
    return {k: torch.cat([it[0][k] for it in items[:2]]).unsqueeze(0).repeat(n, 1, 1) for k in items[0][0]}   # [n, 20, c]


def _predictor(r, path, **kw):
    from inferbiomechanics_amd.models.DiffusionLabelPredictor import DiffusionLabelPredictor
    pred = DiffusionLabelPredictor(r.model(torch.bfloat16, **LABELS), S, seed=11, use_graph=r.use_graph, **kw)
    for n in (2, 2, 3):                     # a call, the same shape again, another batch size
        if path == "call":
            out = pred(_label_inputs(r, n, 10), draw=1 if pred.num_samples > 1 else 0)
        else:
            out = getattr(pred, path)(_label_inputs(r, n, 20), hop=4)
        if r.sink is not None:
            for k in sorted(out):
                r.sink(out[k])
                if pred.last_std is not None:
                    r.sink(pred.last_std[k])


def cases():
    """{case name: fn(run)} in the order of the golden file"""
    out = {}
    for cls in ("DDIMSampler", "ConditionalDDIMSampler"):
        for solver, spacing, eta in SETTINGS:
            for dn, dt in DTYPES:
                out[f"{cls}_{solver}_{spacing}_eta{eta}_{dn}"] = \
                    lambda r, a=(cls, dt, solver, spacing, eta): _window(r, *a)
    for dn, dt in DTYPES:
        out[f"ConditionalDDIMSampler_clean_then_noised_{dn}"] = lambda r, dt=dt: _clean_then_noised(r, dt)
    for observed in (False, True):
        for solver, spacing in (("ddim", "time"), ("dpmpp2m", "logsnr")):
            for F in TRIAL_FRAMES:
                for dn, dt in DTYPES:
                    out[f"StitchedDDIMSampler_{solver}_F{F}_{'obs' if observed else 'free'}_{dn}"] = \
                        lambda r, a=(dt, F, observed, solver, spacing): _trial(r, *a)
    for observed in (False, True):
        for eta in (0.0, 0.5):
            for solver, spacing in (("ddim", "time"), ("dpmpp2m_sde", "logsnr")):
                for dn, dt in DTYPES:
                    out[f"StochasticStitchedSampler_{solver}_eta{eta}_{'obs' if observed else 'free'}_{dn}"] = \
                        lambda r, a=(dt, TRIAL_FRAMES[0], observed, solver, spacing, eta): _trial(r, *a)
    out["predictor_call_K1_eta0"] = lambda r: _predictor(r, "call")
    out["predictor_call_K3_eta1_draw1"] = lambda r: _predictor(r, "call", eta=1.0, num_samples=3)
    out["predictor_predict_trial"] = lambda r: _predictor(r, "predict_trial")
    out["predictor_trial_ensemble_ddim"] = lambda r: _predictor(r, "predict_trial_ensemble", eta=1.0, num_samples=3)
    out["predictor_trial_ensemble_dpmpp2m_sde"] = \
        lambda r: _predictor(r, "predict_trial_ensemble", eta=0.5, num_samples=3, solver="dpmpp2m_sde", spacing="logsnr")
    return out


def trace_case(name: str):
    """the full canonical trace of one case"""
    with _Trace() as tr, Run(tr) as r:
        cases()[name](r)
        return tr.canonical()


def _runs(names):
    """the names cut into runs: a denoise step's launches, its update + counter pair, what ends with a state entry"""
    cur = []
    for e in names:
        cur.append(e)
        if e == "ib_counter_add":
            yield cur[:-2]
            yield cur[-2:]
            cur = []
        elif e == "state:bufs":
            yield cur
            cur = []
    yield cur


def pack(summaries: dict) -> dict:
    """{case: summary} -> the golden file's form: every distinct run of names once, the cases as indices into them"""
    chunks, cases = {}, {}
    for name, s in summaries.items():
        idx = [chunks.setdefault(tuple(r), len(chunks)) for r in _runs(s["names"]) if r]
        cases[name] = {"chunks": idx, "sha256": s["sha256"]}
    return {"chunks": [list(c) for c in chunks], "cases": cases}


def unpack(packed: dict) -> dict:
    return {name: {"names": [e for i in c["chunks"] for e in packed["chunks"][i]], "sha256": c["sha256"]}
            for name, c in packed["cases"].items()}


def load_golden() -> dict:
    """{case: {"names": [...], "sha256": ...}}"""
    with open(GOLDEN) as f:
        return unpack(json.load(f))


def main(argv):
    dump = argv[argv.index("--dump") + 1] if "--dump" in argv else None
    if dump:
        os.makedirs(dump, exist_ok=True)
    got = {}
    for name in cases():
        trace = trace_case(name)
        got[name] = summary(trace)
        if dump:
            with open(os.path.join(dump, name + ".json"), "w") as f:
                f.write("\n".join(json.dumps(e) for e in trace) + "\n")
    if "--write" in argv:
        packed = pack(got)
        assert unpack(packed) == got
        lines = lambda items: ",\n".join(json.dumps(i, separators=(",", ":")) for i in items)
        with open(GOLDEN, "w") as f:
            f.write('{"chunks": [\n' + lines(packed["chunks"]) + '\n],\n"cases": {\n'
                    + ",\n".join(f"{json.dumps(n)}: {json.dumps(c, separators=(',', ':'))}" for n, c in packed["cases"].items())
                    + "\n}}\n")
        print(f"wrote {GOLDEN}: {len(got)} cases")
        return 0
    golden = load_golden()
    bad = [n for n in got if got[n] != golden.get(n)] + [n for n in golden if n not in got]
    for n in bad:
        print("differs:", n)
    print(f"{len(got) - len(bad)} of {len(got)} cases agree with {os.path.relpath(GOLDEN, ROOT)}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
