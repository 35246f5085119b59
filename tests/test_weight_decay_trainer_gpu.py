"""Decoupled weight decay in the fused trainer (HipTrainer(weight_decay=...)) on the GPU, 6 steps, bitwise.

The yardstick takes its decay from torch: a trainer with weight_decay = 0 and use_graph=False whose `hip.optim_step` the test
wraps -- before the original call the wrapper multiplies, with a torch fp32 multiply on the current stream, the decayed
ranges of that launch's slice by f = decay_factor(rate of the step, wd), leaving alone the ranges the launch names as done.
The rate is the host's, or the device probe's value for that step under a schedule.

  * the decayed trainer, replayed from its captured hipGraph and in use_graph=False form, equals the yardstick in loss, flat
    parameters and EMA after every step: MLP and transformer denoiser, Adam, with and without a cosine schedule + EMA;
  * weight_decay = 0 is the trainer without the argument: the same launch names, bitwise the same steps;
  * a checkpoint taken mid-run and loaded into a fresh trainer continues bitwise; another decay is refused;
  * with SGD the parameters with ndim < 2 are bitwise those of the weight_decay = 0 run after step 1 while every decayed
    one differs (later steps see other gradients, so the comparison ends there).  -m gpu."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
STEPS = 6
WD = 0.1


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def sched():
    from inferbiomechanics_amd.lr_schedule import LrSchedule
    return LrSchedule("cosine", 2, 5, 0.1)               # six steps: warmup, peak, decay, floor


def _diff_batches(B, T, D, dt):
    def make(n, seed=5):
        g = torch.Generator().manual_seed(seed)
        return [(torch.randn(B, T, D, generator=g).to(DEV, dt), torch.randint(0, 1000, (B,), generator=g).to(DEV),
                 torch.randn(B, T, D, generator=g).to(DEV, dt)) for _ in range(n)]
    return make


def _model(name):
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionMLP, DiffusionTransformer
    torch.manual_seed(7)
    if name == "mlp_perop_fp32":
        return DiffusionMLP(44, [64, 96], temb_dim=32, temb_hidden=48, device=DEV), _diff_batches(8, 10, 44, torch.float32)
    assert name == "transformer_small_bf16"
    return DiffusionTransformer(48, 32, d_model=512, num_heads=8, dim_feedforward=512, num_layers=2, device=DEV,
                                compute_dtype=torch.bfloat16), _diff_batches(128, 32, 48, torch.bfloat16)


MODELS = ["mlp_perop_fp32", "transformer_small_bf16"]


def _trainer(name, opt="adam", use_graph=True, **kw):
    from inferbiomechanics_amd.engine import HipTrainer
    model, mk = _model(name)
    lr = 1e-2 if opt == "sgd" else 1e-3
    return HipTrainer(model, "diffusion", opt, lr, use_graph=use_graph, **kw), mk, lr


def _bits(t):
    return t.view(torch.int32)


def _run(tr, batches, before=None):
    losses, flats, emas = [], [], []
    for k, b in enumerate(batches):
        if before is not None:
            before(k)
        tr.step(b)
        torch.cuda.synchronize()
        losses.append(tr.loss_value())
        flats.append(tr.flat.detach().cpu().clone())
        emas.append(None if tr.ema is None else tr.ema.detach().cpu().clone())
    return losses, flats, emas


def _same(a, b, what):
    (la, fa, ea), (lb, fb, eb) = a, b
    assert la == lb, (what, la, lb)
    for k in range(len(fa)):
        assert torch.equal(_bits(fa[k]), _bits(fb[k])), (what, "parameters after step", k + 1,
                                                         int((_bits(fa[k]) != _bits(fb[k])).sum()))
        assert (ea[k] is None) == (eb[k] is None)
        if ea[k] is not None:
            assert torch.equal(_bits(ea[k]), _bits(eb[k])), (what, "ema after step", k + 1)


def yardstick(name, batches, opt="adam", first=1, **kw):
    """the run of a trainer without decay whose optimizer launches are preceded by torch's multiply of the decayed ranges"""
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.weight_decay import decay_factor, decay_ranges, decayed_names
    ref, _, lr = _trainer(name, opt, use_graph=False, **kw)
    shapes = {k: tuple(v.shape) for k, v in ref.model.named_parameters()}
    ranges = decay_ranges(ref.layout, decayed_names({k: shapes[k] for k in ref.layout}))
    sch = kw.get("lr_schedule")
    rates = None
    if sch is not None:
        steps = torch.arange(first, first + len(batches), dtype=torch.int32, device=DEV)
        rates = [float(v) for v in hip.lr_schedule_eval(lr, sch, steps).cpu()]
    cur = {"k": 0, "launches": 0}
    real = hip.optim_step

    def wrapped(opt_, p, g, *a, **k):
        lo = (p.data_ptr() - ref.flat.data_ptr()) // 4
        hi = lo + p.numel()
        assert 0 <= lo and hi <= ref.flat.numel() and k.get("weight_decay", 0.0) == 0.0
        src = k.get("sources")
        done = [] if src is None or len(src) < 5 else [((d.data_ptr() - g.data_ptr()) // 4 + lo, d.numel()) for d in src[4]]
        keep = torch.ones(hi - lo, dtype=torch.bool, device=DEV)
        for a0, n0 in done:
            keep[a0 - lo:a0 - lo + n0] = False
        f = torch.tensor(decay_factor(rates[cur["k"]] if rates is not None else lr, WD), dtype=torch.float32, device=DEV)
        for a0, n0 in ranges:
            s, e = max(a0, lo), min(a0 + n0, hi)
            if s < e:
                v = p[s - lo:e - lo]
                v.copy_(torch.where(keep[s - lo:e - lo], v * f, v))
        cur["launches"] += 1
        return real(opt_, p, g, *a, **k)
    hip.optim_step = wrapped
    try:
        out = _run(ref, batches, before=lambda k: cur.__setitem__("k", k))
    finally:
        hip.optim_step = real
    assert cur["launches"] >= len(batches)
    return out, ranges


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("variant", ["adam", "adam_cosine_ema"])
def test_decayed_trainer_is_torchs_multiply_before_every_launch(name, variant):
    kw = {} if variant == "adam" else {"lr_schedule": sched(), "ema_decay": 0.999}
    _, mk = _model(name)
    batches = mk(STEPS)
    want, ranges = yardstick(name, batches, **kw)
    assert ranges, "something is decayed"
    for use_graph in (True, False):
        tr, _, _ = _trainer(name, use_graph=use_graph, weight_decay=WD, **kw)
        assert tr.decay_ranges == ranges
        got = _run(tr, batches)
        assert (tr._rec is not None) == use_graph, "the later steps were replays of the captured graph"
        _same(got, want, (name, variant, use_graph))
    # the decay did something: the same run without it differs from the first step on
    plain, _, _ = _trainer(name, **kw)
    plain.step(batches[0])
    torch.cuda.synchronize()
    assert not torch.equal(plain.flat.cpu(), want[1][0]), name


@pytest.mark.parametrize("name", MODELS)
def test_weight_decay_zero_is_todays_trainer(name):
    from inferbiomechanics_amd import hip

    def run(**kw):
        tr, mk, _ = _trainer(name, **kw)
        batches = mk(STEPS)
        with hip.record_launches() as rec:
            tr.step(batches[0])
        torch.cuda.synchronize()
        names = [n for n, _ in rec.calls]
        first = (tr.loss_value(), tr.flat.detach().cpu().clone())
        losses, flats, emas = _run(tr, batches[1:])
        assert tr._rec is not None
        return names, ([first[0]] + losses, [first[1]] + flats, [None] + emas)
    names_today, today = run()
    assert not any("decay" in n for n in names_today) and any(n.startswith("ib_optim_step") for n in names_today)
    for off in (dict(weight_decay=0.0), dict(weight_decay=0.0, decay_filter=lambda n, s: True)):
        names, got = run(**off)
        assert names == names_today, (name, off)
        _same(got, today, (name, sorted(off)))
    names_on, _ = run(weight_decay=WD)
    strip = lambda n: n[:-len("_decay")] if n.endswith("_decay") else n
    assert [strip(n) for n in names_on] == names_today, "the same launches, decayed"
    assert sum(n.endswith("_decay") for n in names_on) == sum(n.startswith("ib_optim_step") for n in names_today)


def test_checkpoint_mid_run_continues_bitwise(tmp_path):
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.cli.abstract_command import AbstractCommand
    from inferbiomechanics_amd.cli.train import save_checkpoint
    name, kw = "mlp_perop_fp32", {"lr_schedule": sched(), "ema_decay": 0.999, "weight_decay": WD}
    whole, mk, _ = _trainer(name, **kw)
    batches = mk(STEPS)
    want = _run(whole, batches)
    first, _, _ = _trainer(name, **kw)
    _run(first, batches[:3])
    d = str(tmp_path / "ck")
    save_checkpoint(d, 0, 2, first.model, first)
    saved = torch.load(f"{d}/epoch_0_batch_2.pt", map_location="cpu")["optimizer_state_dict"]
    assert saved["weight_decay"] == first.weight_decay and saved["decayed"] == first.decayed and saved["step"] == 3
    resumed, _, _ = _trainer(name, **kw)
    assert AbstractCommand().load_latest_checkpoint(resumed.model, optimizer=resumed, checkpoint_dir=d) == (0, 2)
    got = _run(resumed, batches[3:])
    (lw, fw, ew), (lg, fg, eg) = want, got
    assert lg == lw[3:]
    for k in range(3):
        assert torch.equal(_bits(fg[k]), _bits(fw[3 + k])), ("parameters after step", 4 + k)
    other, _, _ = _trainer(name, **dict(kw, weight_decay=0.2))
    with pytest.raises(hip.HipError, match="weight decay"):
        AbstractCommand().load_latest_checkpoint(other.model, optimizer=other, checkpoint_dir=d)


@pytest.mark.parametrize("name", MODELS)
def test_sgd_leaves_vectors_alone_and_decays_every_matrix(name):
    _, mk = _model(name)
    batch = mk(1)[0]
    out = {}
    for wd in (0.0, WD):
        tr, _, _ = _trainer(name, "sgd", weight_decay=wd)
        init = tr.flat.detach().cpu().clone()
        tr.step(batch)
        torch.cuda.synchronize()
        out[wd] = tr.flat.detach().cpu().clone()
    shapes = {k: tuple(v.shape) for k, v in tr.model.named_parameters()}
    seen = {1: 0, 2: 0}
    for k, (off, n) in tr.layout.items():
        a, b = out[0.0][off:off + n], out[WD][off:off + n]
        if len(shapes[k]) < 2:
            assert torch.equal(_bits(a), _bits(b)), (name, k, "a vector was decayed")
            seen[1] += 1
        elif bool(init[off:off + n].any()):                  # a matrix of zeros stays what its gradient makes of it
            assert not torch.equal(a, b), (name, k, "a matrix was not")
            seen[2] += 1
    assert seen[1] > 0 and seen[2] > 0 and tr.decayed == [k for k in tr.layout if len(shapes[k]) >= 2]
