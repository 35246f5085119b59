#!/usr/bin/env python3
"""The launch sequence of the transformer plans, pinned: for a fixed list of cases (every tier of
TransformerLayerPlan / DenoiserTransformerPlan at the smallest shape that takes it, every tuning switch that moves a launch,
the data-parallel flush order, the sampler tiers, the standalone layer with and without dropout) the canonical trace of
every C-ABI call the host side issues, taken on CPU tensors with the library in dry-run mode (no GPU needed).

A canonical trace is a list of entries in issue order:
  * ["ib_<entry>", arg, ...]  one per C-ABI call: integer and float scalars as passed, ctypes arrays expanded element by
    element, every pointer replaced by "p<k>", k = the order of its first appearance in the trace (the pattern of buffer
    reuse is compared, not addresses);
  * ["operands:linear_wgrad_slabs_multi", "p<k>", ...]  in front of a grouped weight-gradient launch: per problem dz, x,
    workspace, then the bias partial-sum buffers and the time-MLP rider's operands (the dry-run wrapper of that one launch
    passes no operands to the C-ABI, so the call itself would not show them);
  * ["state:<what>", value, ...]  host-side state a case records (tools/sampler_trace.py: a sampler's signature and
    buffers): nested tuples as lists, every integer that is an address taken during the trace as its "p<k>", dtypes as text;
  * "begin:step" / "begin:round" / "begin:sample" / "begin:layer"   where a repetition of the case starts;
  * "fork:<branch>:<on>" ... "endfork:<branch>" around what a Branch.run issues, "join:<branch>" for every Branch.join
    (<branch> = the branch's name + "#k" for the k-th distinct branch of that name in the case: the layers' branches are
    all called "layer");
  * "ready:<param>" / "flush" from the ParamSource of the data-parallel cases.

tests/golden/plan_traces.json holds, per case, the names and markers in full and the sha256 of the whole canonical trace;
tests/test_plan_trace_cpu.py holds plans.py to it.  A refactor of the plans leaves the file alone.  A change that moves,
adds or removes a launch ON PURPOSE regenerates it (`--write`) and says so in its description.

  python tools/plan_trace.py            # compare with the golden file, print the cases that differ
  python tools/plan_trace.py --write    # rewrite tests/golden/plan_traces.json
  python tools/plan_trace.py --dump DIR # one <case>.json per case with the full canonical trace (diff two trees' dumps)
"""
import ctypes
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from inferbiomechanics_amd import hip, plans  # noqa: E402
from inferbiomechanics_amd._tuning import tuning as TU  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_traces.json")

WHOLE = dict(B=128, T=32, D=48, d=512, heads=8, ffn=1024, layers=3, dtype=torch.bfloat16)      # whole-layer tier
PANELS = dict(WHOLE, heads=4)             # token-count panels, QKV tail / head, the last layer's split tail
TRAIN_CASES = {
    "train_whole_layer": WHOLE,
    "train_token_panels": PANELS,
    "train_padded_D300": dict(B=128, T=32, D=300, d=512, heads=8, ffn=2048, layers=2, dtype=torch.bfloat16),
    "train_per_op_bf16": dict(WHOLE, B=8, layers=2),
    "train_fp32": dict(B=6, T=10, D=44, d=64, heads=4, ffn=128, layers=3, dtype=torch.float32),
    "train_d256": dict(B=128, T=32, D=48, d=256, heads=4, ffn=512, layers=2, dtype=torch.bfloat16),
}
SWITCHES = ("no_attn_fuse", "no_qkv_fuse", "no_ffn_chain", "no_head_merge", "no_layer_group", "no_nt", "no_early_opt",
            "no_opt_fuse")
SAMPLER = dict(T=200, D=300, d=512, heads=8, ffn=2048, layers=2, dtype=torch.bfloat16)
SAMPLER_CASES = {
    "sample_B4_row_panels": dict(SAMPLER, B=4),
    "sample_B24_no_qkv_panel": dict(SAMPLER, B=24),
    "sample_B48_chain": dict(SAMPLER, B=48),
    "sample_B84_side_split": dict(SAMPLER, B=84, side=True),
    "sample_fp32": dict(B=3, T=10, D=44, d=64, heads=4, ffn=128, layers=3, dtype=torch.float32),
}


class _Trace:
    """Dry-run library + Branch markers for the duration of one case.  Every tensor whose address is taken while the trace
    runs is kept alive until the trace is canonicalised: a freed temporary's address handed out again would make two
    buffers one pointer index in one run and two in the next."""

    def __enter__(self):
        hip.set_dry_run(True)
        torch.manual_seed(0)
        self.log = hip.lib().args
        self._keep = keep = []
        self._addr = addr = set()           # every address taken: what a "state:" entry may hold as a plain integer
        self._seen = {}                     # branch name -> [Branch, ...] in first-use order
        self._saved = (plans.Branch.run, plans.Branch.join, hip.linear_wgrad_slabs_multi)
        data_ptr = torch.Tensor.data_ptr
        trace = self

        def kept_ptr(t):
            keep.append(t)
            addr.add(data_ptr(t))
            return data_ptr(t)

        def run(br, fn):
            nm = trace._name(br)
            trace.log.append((f"fork:{nm}:{br.on}", None))
            fn()
            trace.log.append((f"endfork:{nm}", None))

        def join(br):
            trace.log.append((f"join:{trace._name(br)}", None))

        def grouped(problems, bias_parts=None, time_bwd=None, launch=hip.linear_wgrad_slabs_multi):
            ops = [t for pr in problems for t in pr] + list(bias_parts or ()) + list(time_bwd or ())
            trace.log.append(("operands:linear_wgrad_slabs_multi", [None if t is None else t.data_ptr() for t in ops]))
            return launch(problems, bias_parts=bias_parts, time_bwd=time_bwd)
        plans.Branch.run, plans.Branch.join, hip.linear_wgrad_slabs_multi = run, join, grouped
        torch.Tensor.data_ptr = kept_ptr
        return self

    def __exit__(self, *exc):
        plans.Branch.run, plans.Branch.join, hip.linear_wgrad_slabs_multi = self._saved
        del torch.Tensor.data_ptr           # the inherited method again
        hip.set_dry_run(False)
        return False

    def _name(self, br) -> str:
        same = self._seen.setdefault(br.name, [])
        if not any(b is br for b in same):
            same.append(br)
        return f"{br.name}#{[b is br for b in same].index(True)}"

    def mark(self, text: str):
        self.log.append((text, None))

    def canonical(self):
        """the trace so far as JSON-able entries (see the module docstring)"""
        index = {}

        def ptr(v):
            if not v:
                return None
            return "p%d" % index.setdefault(int(v), len(index))

        def arg(v, argtype):
            if v is None or isinstance(v, (bool, str)):
                return v
            if isinstance(v, int):
                return ptr(v) if argtype is ctypes.c_void_p else v
            if isinstance(v, float):
                return v
            if isinstance(v, ctypes.Array):
                return [ptr(e) if v._type_ is ctypes.c_void_p else e for e in v]
            if isinstance(v, ctypes.c_void_p):
                held = [o for o in (v._objects or {}).values() if isinstance(o, ctypes.Array)]
                if held:                    # ctypes.cast(array, c_void_p): a host array of pointers / sizes
                    return arg(held[0], None)
                if v._objects:              # a pointer to a host scalar the call writes
                    return "host"
                return ptr(v.value)
            if hasattr(v, "value"):
                return v.value
            return "host"                   # byref(...)

        def state(v):
            if isinstance(v, (tuple, list)):
                return [state(e) for e in v]
            if v is None or isinstance(v, (bool, str, float)):
                return v
            if isinstance(v, int):
                return ptr(v) if v in self._addr else v
            return str(v)                   # a dtype
        out = []
        for name, a in self.log:
            if a is None:
                out.append(name)
            elif name.startswith("operands:"):
                out.append([name] + [ptr(v) for v in a])
            elif name.startswith("state:"):
                out.append([name] + state(a))
            else:
                out.append([name] + [arg(v, t) for v, t in zip(a, hip._sig(name)[1])])
        return out


def _model(c, device=None):
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    return DiffusionTransformer(c["D"], c["T"], d_model=c["d"], num_heads=c["heads"], dim_feedforward=c["ffn"],
                                num_layers=c["layers"], compute_dtype=c["dtype"], device=device)


def _batch(c, device=None):
    """(x0, t, eps) of a training step, the same numbers on every device"""
    g = torch.Generator().manual_seed(1)
    shape = (c["B"], c["T"], c["D"])
    x0, t, eps = torch.randn(shape, generator=g), torch.randint(0, 1000, (c["B"],), generator=g), torch.randn(shape, generator=g)
    return x0.to(device), t.to(device), eps.to(device)


def _train(tr, c, switches=()):
    from inferbiomechanics_amd.engine import HipTrainer
    for s in switches:
        setattr(TU, s, True)
    try:
        trainer = HipTrainer(_model(c), "diffusion", "adam", 1e-3, use_graph=False)
        batch = _batch(c)
        for _ in range(2):
            tr.mark("begin:step")
            trainer.step(batch)
        return trainer
    finally:
        for s in switches:
            delattr(TU, s)


def _data_parallel(tr, c, no_lag: bool):
    """the overlapped data-parallel backward, driven at plan level (the launch order needs no process group)"""
    trainer = _train(tr, c)
    del tr.log[:]
    if no_lag:
        TU.no_lag_group = True
    try:
        plan, m = trainer.plan, trainer.model
        plan.flush_each_layer(True)
        plan.fuse_reduce_into_optimizer, plan.early_optimizer = False, None
        src = trainer._psrc()
        P = plans.ParamSource(src.w, src.v, src.g, ready=lambda name: tr.mark("ready:" + name),
                              flush=lambda: tr.mark("flush"))
        B, T, D, dt = c["B"], c["T"], c["D"], c["dtype"]
        Dp = plan.train_pitch(D, B * T)
        xt, pred, dpred = (plan.buf.get(n, (B * T, Dp), dt, zero=True)[:, :D] for n in ("tr.xt", "tr.pred", "tr.dpred"))
        t = _batch(c)[1]
        for _ in range(2):
            tr.mark("begin:round")
            plan.forward(xt, t, m.tables(xt.device).temb, P, out=pred, BT=(B, T))
            plan.backward(dpred, P, accumulate=False)
    finally:
        if no_lag:
            del TU.no_lag_group


def _sample(tr, c):
    from inferbiomechanics_amd.diffusion.sampler import DDIMSampler
    m = _model(c)
    sampler = DDIMSampler(m, num_sample_steps=4, use_graph=False)
    x = torch.randn(c["B"], c["T"], c["D"], generator=torch.Generator().manual_seed(2))
    m.ensure_packed()
    if c.get("side"):
        m._get_plan(m._flat.device).br_side.on = True      # off the GPU every branch is off: side_windows() needs this one on
    for _ in range(2):
        tr.mark("begin:sample")
        sampler.sample(x)


def _layer(tr, p: float, dtype):
    from inferbiomechanics_amd.models.TransformerBaseline import TransformerLayer
    layer = TransformerLayer(64, 4, 128, p, dtype=dtype, seed=1234)
    layer.train()
    x = torch.randn(2, 9, 64, generator=torch.Generator().manual_seed(3)).requires_grad_()
    for _ in range(2):
        tr.mark("begin:layer")
        layer(x).float().sum().backward()


def cases():
    """{case name: fn(trace)} in the order of the golden file"""
    out = {}
    for name, c in TRAIN_CASES.items():
        out[name] = lambda tr, c=c: _train(tr, c)
    for s in SWITCHES:
        out[f"train_whole_layer+{s}"] = lambda tr, s=s: _train(tr, WHOLE, (s,))
    out["train_token_panels+no_tail_split"] = lambda tr: _train(tr, PANELS, ("no_tail_split",))
    for name, c in (("whole_layer", WHOLE), ("token_panels", PANELS)):
        out[f"ddp_{name}_lagged"] = lambda tr, c=c: _data_parallel(tr, c, False)
        out[f"ddp_{name}+no_lag_group"] = lambda tr, c=c: _data_parallel(tr, c, True)
    for name, c in SAMPLER_CASES.items():
        out[name] = lambda tr, c=c: _sample(tr, c)
    for p in (0.0, 0.1):
        for dtype, dn in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            out[f"layer_p{p}_{dn}"] = lambda tr, p=p, dtype=dtype: _layer(tr, p, dtype)
    return out


def trace_case(name: str):
    """the full canonical trace of one case"""
    with _Trace() as tr:
        cases()[name](tr)
        return tr.canonical()


def summary(trace) -> dict:
    """what the golden file keeps of a trace: names and markers in order, and the hash of everything"""
    text = json.dumps(trace, separators=(",", ":"))
    return {"names": [e if isinstance(e, str) else e[0] for e in trace], "sha256": hashlib.sha256(text.encode()).hexdigest()}


def load_golden() -> dict:
    with open(GOLDEN) as f:
        return json.load(f)


def launch_names(names, begin: str):
    """the entry names of a case's LAST repetition (after the last `begin` marker), markers removed"""
    last = len(names) - 1 - names[::-1].index(begin)
    return [n for n in names[last + 1:] if n.startswith("ib_")]


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
        with open(GOLDEN, "w") as f:
            f.write("{\n" + ",\n".join(f"{json.dumps(n)}: {json.dumps(s)}" for n, s in got.items()) + "\n}\n")
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
