"""hip.optim_step's call table without a GPU: for every combination of (sources, ema, lr_schedule, weight_decay / decay_origin,
max_grad_norm, step form) the C entry it calls and every argument it passes, and for every refusal the HipError's message,
equal to tests/golden/optim_calls.json.  The fixture was recorded once, by this module's --write mode, at the commit BEFORE
optim_step's nine calls became one table-driven call (`python tests/test_optim_call_table_cpu.py --write`); the case builder
below is what recorded it, so a case cannot be left out on one side only.

Scalars are recorded by value, pointers as null or "<buffer name>+<byte offset>" (the stream, 0 in the dry run, as 0), the
seven arrays behind the sources pointers as lists (their base pointers named like any other), the dry run's ema_ranges
beside them."""
import ctypes
import itertools
import json
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "optim_calls.json")
N_PLAIN, N_SOURCES = 67, 72
SRC_ARRAYS = {13: ctypes.c_int64, 14: ctypes.c_int64, 15: ctypes.c_int32, 16: ctypes.c_void_p, 17: ctypes.c_int64,
              18: ctypes.c_int32, 19: ctypes.c_float}          # start, len, kind, base, stride, count, scale of the sources entries

SOURCES = ("none", "sources")
EMA = (False, True)
SCHED = ("none", "constant", "cosine")
DECAY = ("0", "0.01@0", "0.01@8")
CLIP = (0.0, 1.0, float("inf"))
STEP = ("host", "step_dev", "ticket")


class Buffers:
    """the named CPU tensors of one case; a pointer inside one of them is recorded as name+offset"""

    def __init__(self, hip, n):
        self.n = n
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt)
        self.t = {"p": z(n), "g": z(n), "s1": z(n), "s2": z(n), "shadow": z(n, dt=torch.bfloat16), "ema": z(n),
                  "step_dev": z(1, dt=torch.int32), "ticket": z(hip.optim_ticket_words(), dt=torch.int32),
                  "norm_slots": z(1, dt=torch.float64), "norm_stats": z(4), "ws": z(2, 16), "part": z(4, 24), "loss": z(4)}
        self.table = hip.DecayTable([(0, 16), (32, 6)], "cpu")
        self.t["table"] = self.table.buf

    def __getattr__(self, k):
        return self.t[k]

    def name(self, ptr):
        if ptr is None:
            return None
        ptr = int(ptr)
        for k, t in self.t.items():
            if t.data_ptr() <= ptr < t.data_ptr() + max(t.numel() * t.element_size(), 1):
                return f"{k}+{ptr - t.data_ptr()}"
        return ptr                                             # 0: the dry run's stream

    def sources(self):
        """one slab item, one column-sum segment, the loss scalar, one done range"""
        g = self.g
        return ([(self.ws, 2, g[16:32])], self.part, 4, [(4, 8, g[48:56], None, 0.5), (0, 1, self.loss[:1], None, 0.25)], [g[32:48]])


def scalar(v):
    if isinstance(v, float) and not math.isfinite(v):
        return repr(v)                                         # "inf" / "nan": JSON has no spelling for them
    return v


def record(hip, B, fn):
    """what one optim_step call did: {"entry", "args", "ema_ranges"} or {"error": the HipError's message}"""
    lib = hip.lib()
    del lib.args[:], lib.calls[:], lib.ema_ranges[:]
    try:
        fn()
    except hip.HipError as e:
        assert not lib.calls, "a refused call launches nothing"
        return {"error": str(e)}
    assert len(lib.args) == 1, lib.calls
    name, a = lib.args[0]
    types = hip._sig(name)[1]
    out = []
    for i, (v, t) in enumerate(zip(a, types)):
        v = v.value if isinstance(v, ctypes.c_void_p) else v
        if "_sources" in name and i in SRC_ARRAYS and v is not None:
            arr = ctypes.cast(ctypes.c_void_p(v), ctypes.POINTER(SRC_ARRAYS[i]))
            vals = [arr[j] for j in range(int(a[12]))]
            out.append({"array": [B.name(x) if i == 16 else scalar(x) for x in vals]})
        elif t is hip._vp:
            out.append(B.name(v))
        else:
            out.append(scalar(v))
    ranges = [[B.name(p), n, [[int(s), int(l)] for s, l in done]] for p, n, done in lib.ema_ranges]
    return {"entry": name, "args": out, "ema_ranges": ranges}


def product_cases(hip):
    """(case id, Buffers, thunk) over the whole product of the six factors"""
    from inferbiomechanics_amd.lr_schedule import LrSchedule
    for src, ema, sch, dec, clip, form in itertools.product(SOURCES, EMA, SCHED, DECAY, CLIP, STEP):
        B = Buffers(hip, N_SOURCES if src == "sources" else N_PLAIN)
        kw = {"shadow": B.shadow, "grad_scale": 0.5}
        if src == "sources":
            kw["sources"] = B.sources()
        if ema:
            kw.update(ema=B.ema, ema_decay=0.9, ema_warmup=False)
        if sch != "none":
            kw["lr_schedule"] = LrSchedule("constant", 0, 0, 1.0) if sch == "constant" else LrSchedule("cosine", 5, 15, 0.1)
        if dec != "0":
            kw.update(weight_decay=0.01, decay_table=B.table, decay_origin=int(dec.split("@")[1]))
        if clip:
            kw.update(max_grad_norm=clip, norm_slots=B.norm_slots, norm_stats=B.norm_stats)
        if form == "host":
            kw["step"] = 3
        elif form == "step_dev":
            kw.update(step=1, step_dev=B.step_dev)
        else:
            kw.update(step_dev=B.step_dev, ticket=B.ticket)
        cid = f"{src}|ema={int(ema)}|sched={sch}|decay={dec}|clip={clip!r}|{form}"
        yield cid, B, (lambda B=B, kw=kw: hip.optim_step("adam", B.p, B.g, B.s1, B.s2, 1e-3, **kw))


def error_cases(hip):
    """one case per refusal of optim_step that the product does not reach, then pairs that pin the order of the refusals"""
    from inferbiomechanics_amd.lr_schedule import LrSchedule
    B = Buffers(hip, N_SOURCES)
    n = B.n
    clip = dict(max_grad_norm=1.0, norm_slots=B.norm_slots, norm_stats=B.norm_stats)
    dec = dict(weight_decay=0.01, decay_table=B.table)
    meta = lambda dt: torch.zeros(4, dtype=dt, device="meta")
    off_table = hip.DecayTable.__new__(hip.DecayTable)
    off_table.buf, off_table.n = meta(torch.int64), 1
    g = B.g
    two_loss = ([], B.part, 4, [(0, 1, B.loss[:1], None, 1.0), (1, 1, B.loss[1:2], None, 1.0)])
    cases = {
        "clip negative": dict(clip, max_grad_norm=-1.0),
        "clip nan": dict(clip, max_grad_norm=float("nan")),
        "clip without slots": dict(max_grad_norm=1.0, norm_stats=B.norm_stats),
        "clip without stats": dict(max_grad_norm=1.0, norm_slots=B.norm_slots),
        "clip slots dtype": dict(clip, norm_slots=torch.zeros(1)),
        "clip stats dtype": dict(clip, norm_stats=torch.zeros(4, dtype=torch.float64)),
        "clip slots 2-D": dict(clip, norm_slots=torch.zeros(1, 1, dtype=torch.float64)),
        "clip stats short": dict(clip, norm_stats=B.norm_stats[:2]),
        "clip slots strided": dict(clip, norm_slots=torch.zeros(4, dtype=torch.float64)[::2]),
        "clip slots device": dict(clip, norm_slots=meta(torch.float64)),
        "decay negative": dict(dec, weight_decay=-0.5),
        "decay nan": dict(dec, weight_decay=float("nan")),
        "decay table type": dict(weight_decay=0.01, decay_table=[(0, 16)]),
        "decay table missing": dict(weight_decay=0.01),
        "decay origin negative": dict(dec, decay_origin=-4),
        "decay origin odd": dict(dec, decay_origin=6),
        "decay table device": dict(weight_decay=0.01, decay_table=off_table),
        "schedule type": dict(lr_schedule="cosine"),
        "p dtype": dict(_p=torch.zeros(n, dtype=torch.float64)),
        "p 2-D": dict(_p=torch.zeros(n // 8, 8)),
        "g dtype": dict(_g=torch.zeros(n, dtype=torch.bfloat16)),
        "g length": dict(_g=torch.zeros(n + 4)),
        "p strided": dict(_p=torch.zeros(2 * n)[::2]),
        "s1 dtype": dict(_s1=torch.zeros(n, dtype=torch.float64)),
        "s1 length": dict(_s1=torch.zeros(n - 4)),
        "s2 length": dict(_s2=torch.zeros(n + 4)),
        "shadow dtype": dict(shadow=torch.zeros(n)),
        "shadow length": dict(shadow=torch.zeros(n - 1, dtype=torch.bfloat16)),
        "ema dtype": dict(ema=torch.zeros(n, dtype=torch.float64), ema_decay=0.9),
        "ema length": dict(ema=torch.zeros(n + 1), ema_decay=0.9),
        "ema strided": dict(ema=torch.zeros(2 * n)[::2], ema_decay=0.9),
        "ema decay above": dict(ema=B.ema, ema_decay=1.5),
        "ema decay nan": dict(ema=B.ema, ema_decay=float("nan")),
        "step_dev dtype": dict(step_dev=torch.zeros(1, dtype=torch.int64)),
        "ticket dtype": dict(step_dev=B.step_dev, ticket=torch.zeros(2048, dtype=torch.int64)),
        "ticket short": dict(step_dev=B.step_dev, ticket=B.ticket[:8]),
        "sources part dtype": dict(sources=([], torch.zeros(4, 24, dtype=torch.float64), 4, [])),
        "sources dw outside g": dict(sources=([(B.ws, 2, torch.zeros(16))], None, 0, [])),
        "sources dw misaligned": dict(sources=([(B.ws, 2, g[18:34])], None, 0, [])),
        "sources dst misaligned": dict(sources=([], B.part, 4, [(0, 8, g[2:10], None, 1.0)])),
        "sources done strided": dict(sources=([], None, 0, [], [g[0:32:2]])),
        "sources two scalars": dict(sources=two_loss),
        "sources wide scalar": dict(sources=([], B.part, 4, [(0, 2, B.loss[:2], None, 1.0)])),
        "sources part_i dtype": dict(sources=([], None, 0, [(0, 8, g[0:8], None, 1.0, torch.zeros(4, 24, dtype=torch.float64), 4)])),
        "unknown optimizer": dict(_opt="lion"),
        # the order of the refusals: the first of each pair is the one that is raised
        "order clip < decay": dict(clip, max_grad_norm=-1.0, weight_decay=-0.5),
        "order clip sources < clip slots": dict(max_grad_norm=1.0, sources=B.sources()),
        "order decay < schedule": dict(weight_decay=-0.5, lr_schedule="cosine"),
        "order schedule < p": dict(lr_schedule="cosine", _p=torch.zeros(n, dtype=torch.float64)),
        "order g length < s1": dict(_g=torch.zeros(n + 4), _s1=torch.zeros(n - 4)),
        "order s1 < shadow": dict(_s1=torch.zeros(n - 4), shadow=torch.zeros(n)),
        "order shadow < ema": dict(shadow=torch.zeros(n), ema=B.ema, ema_decay=1.5),
        "order ema < step_dev": dict(ema=B.ema, ema_decay=1.5, step_dev=torch.zeros(1, dtype=torch.int64)),
        "order ticket < sources": dict(step_dev=B.step_dev, ticket=B.ticket[:8], sources=two_loss),
        "order sources < optimizer": dict(sources=two_loss, _opt="lion"),
        "order sched ok, constant": dict(lr_schedule=LrSchedule("constant", 0, 0, 1.0), _g=torch.zeros(n + 4)),
    }
    for cid, kw in cases.items():
        kw = dict(kw)
        pos = [kw.pop("_opt", "adam")] + [kw.pop("_" + k, B.t[k]) for k in ("p", "g", "s1", "s2")]

        def call(pos=pos, kw=kw):
            try:
                hip.optim_step(*pos, 1e-3, **kw)
            except KeyError as e:                              # the unknown optimizer: OPT[opt], no HipError
                raise hip.HipError(f"KeyError: {e}")
        yield "error|" + cid, B, call


def all_cases(hip):
    yield from product_cases(hip)
    yield from error_cases(hip)


def run_all():
    from inferbiomechanics_amd import hip
    hip.set_dry_run(True)
    try:
        return {cid: record(hip, B, fn) for cid, B, fn in all_cases(hip)}
    finally:
        hip.set_dry_run(False)


@pytest.fixture(scope="module")
def recorded():
    return run_all()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_no_case_is_left_out(recorded, golden):
    n = len(SOURCES) * len(EMA) * len(SCHED) * len(DECAY) * len(CLIP) * len(STEP)
    assert n == 324 and len([k for k in recorded if not k.startswith("error|")]) == n
    assert sorted(recorded) == sorted(golden), "the fixture and the case builder name the same cases"
    errors = [k for k in recorded if k.startswith("error|")]
    assert len(errors) >= 40 and all("error" in recorded[k] for k in errors), [k for k in errors if "error" not in recorded[k]]


def test_every_call_is_what_it_was(recorded, golden):
    bad = [k for k in golden if json.loads(json.dumps(recorded[k])) != golden[k]]
    assert not bad, (len(bad), bad[0], recorded[bad[0]], golden[bad[0]])


def test_sources_with_a_clip_are_refused_and_nothing_else_of_the_product(recorded):
    for k, v in recorded.items():
        if k.startswith("error|"):
            continue
        refused = k.startswith("sources|") and "|clip=0.0|" not in k
        assert ("error" in v) == refused, (k, v)
        if refused:
            assert v["error"] == "max_grad_norm needs the materialised gradient: it cannot be combined with sources"


def test_ema_ranges_follow_the_ema_argument(recorded):
    """one rule: a launch with an EMA pointer is recorded with its n and its kind-3 ranges, a launch without is not"""
    for k, v in recorded.items():
        if "error" in v:
            continue
        if "|ema=1|" in k:
            done = [[128 // 4, 16]] if k.startswith("sources|") else []
            assert v["ema_ranges"] == [["ema+0", N_SOURCES if k.startswith("sources|") else N_PLAIN, done]], (k, v["ema_ranges"])
        else:
            assert v["ema_ranges"] == [], k


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_optim_call_table_cpu.py --write     (at the commit the fixture pins)")
    with open(GOLDEN, "w") as f:
        json.dump(run_all(), f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"wrote {GOLDEN}: {os.path.getsize(GOLDEN)} bytes")
