"""The head of the transformer denoiser's training step as two merged launches (round 7):
  launch A  ib_tr_head_prep (csrc/chain.hip): time-MLP forward + q_sample + frame-embedding projection + padded in-projection
            copy as block ranges of one grid, against ib_time_mlp_fwd, ib_q_sample, ib_tiny_matmul and ib_cast2d;
  launch B  ib_ffn_chain_pack_ex (csrc/ffn_chain.hip): weight packing + transposed copies + padded out-projection copies,
            against ib_ffn_chain_pack + 2 x ib_cast2d + ib_transpose_multi.
The merged launches call the device bodies of the stand-alone kernels (csrc/head_jobs.h), so EVERY comparison is bitwise
(torch.equal on the raw buffers, pad columns and untouched outputs included).  Then HipTrainer with the merged head against
the old launch sequence (tuning.no_head_merge), eager and graph-replayed, and the launch shape of the head.  -m gpu."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from inferbiomechanics_amd._tuning import tuning as TU  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
T, D, DP, DM, PD, TEMB, HID, STEPS = 5, 300, 320, 512, 30, 128, 512, 1000
FILL = 7.0          # what every output buffer holds before a launch: columns / buffers a launch must not touch keep it


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _mt4_batch():
    """the smallest batch on the far side of the time-MLP launcher's MT = 1 / 4 switch (csrc/chain.hip: time_fwd_mt1), read
    from the library: ib_tr_head_prep_supported is that rule"""
    from inferbiomechanics_amd import hip
    b = 1
    while hip.tr_head_prep_supported(TEMB, HID, DM, b):
        b += 1
        assert b < 1 << 16
    return b


@pytest.fixture(scope="module")
def weights():
    g = torch.Generator().manual_seed(11)
    q = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(DEV, BF)
    f = lambda *s, sc=0.1: (torch.randn(*s, generator=g) * sc).to(DEV)
    steps = torch.arange(STEPS, dtype=torch.float64)
    ab = torch.cos(steps / STEPS * 1.5) ** 2
    return dict(table=f(STEPS, TEMB, sc=1.0), w1=q(HID, TEMB, sc=TEMB ** -0.5), b1=f(HID), w2=q(DM, HID, sc=HID ** -0.5), b2=f(DM),
                w_in=q(DM, D + PD, sc=0.05), pos=q(64, PD)[:T], sqrt_ab=ab.sqrt().float().to(DEV),
                sqrt_1mab=(1 - ab).sqrt().float().to(DEV))


def _head_inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, T, D, generator=g).to(DEV, BF), torch.randn(B, T, D, generator=g).to(DEV, BF),
            torch.randint(0, STEPS, (B,), generator=g).to(DEV))


def _head_outputs(B):
    full = lambda *s: torch.full(s, FILL, dtype=BF, device=DEV)
    return dict(s=full(B, TEMB), zu=full(B, HID), u=full(B, HID), e=full(B, DM), xt=full(B * T, DP), posproj=full(T, DM),
                w_in_pad=full(DM, DP))


def _run_head(w, x0, eps, t, merged, jobs=("q_sample", "posproj", "cast")):
    from inferbiomechanics_amd import hip
    o = _head_outputs(x0.shape[0])
    qs = (x0, eps, w["sqrt_ab"], w["sqrt_1mab"], o["xt"][:, :D])
    pp = (w["pos"], w["w_in"][:, D:].t(), o["posproj"])
    cs = (w["w_in"][:, :D], o["w_in_pad"][:, :D])
    tm = (w["table"], t, w["w1"], w["b1"], w["w2"], w["b2"], o["s"], o["zu"], o["u"], o["e"])
    if merged:
        hip.tr_head_prep(*tm, q_sample=qs if "q_sample" in jobs else None, posproj=pp if "posproj" in jobs else None,
                         cast=cs if "cast" in jobs else None)
    else:
        hip.time_mlp_fwd(*tm)
        if "q_sample" in jobs:
            hip.q_sample(x0, eps, t, w["sqrt_ab"], w["sqrt_1mab"], qs[4])
        if "posproj" in jobs:
            hip.tiny_matmul(*pp)
        if "cast" in jobs:
            hip.cast2d(*cs)
    torch.cuda.synchronize()
    return o


def _same(got, want, what):
    for k in want:
        assert torch.equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()))


@pytest.mark.parametrize("B", [3, 17, "mt4"])
def test_head_launch_equals_the_four_separate_entries(weights, B):
    """B = 3: one 16-window row group; 17: two; the third batch takes the 64-window time kernel (MT = 4)"""
    from inferbiomechanics_amd import hip
    B = _mt4_batch() if B == "mt4" else B
    assert hip.tr_head_prep_supported(TEMB, HID, DM, B) == (B <= 17)
    x0, eps, t = _head_inputs(B, 100 + B)
    want = _run_head(weights, x0, eps, t, merged=False)
    got = _run_head(weights, x0, eps, t, merged=True)
    assert bool((want["xt"][:, D:] == FILL).all()) and bool((want["w_in_pad"][:, D:] == FILL).all())     # pad columns untouched
    assert not bool((want["xt"][:, :D] == FILL).all()) and not bool((want["posproj"] == FILL).all())
    _same(got, want, f"B={B}")


@pytest.mark.parametrize("absent", ["q_sample", "posproj", "cast", "all"])
def test_head_launch_with_a_job_absent(weights, absent):
    """each optional job absent in turn: its output keeps what it held, the others do not change; all three absent: the
    launch IS ib_time_mlp_fwd"""
    jobs = tuple(j for j in ("q_sample", "posproj", "cast") if j != absent and absent != "all")
    x0, eps, t = _head_inputs(17, 7)
    want = _run_head(weights, x0, eps, t, merged=False, jobs=jobs)
    got = _run_head(weights, x0, eps, t, merged=True, jobs=jobs)
    for k, j in (("xt", "q_sample"), ("posproj", "posproj"), ("w_in_pad", "cast")):
        if j not in jobs:
            assert bool((got[k] == FILL).all()), k
    _same(got, want, f"without {absent}")


@pytest.mark.parametrize("layers,ffn", [(1, 512), (2, 1024)])
@pytest.mark.parametrize("extra", ["both", "transposes", "casts", "none"])
def test_pack_launch_equals_pack_casts_and_transposes(layers, ffn, extra):
    from inferbiomechanics_amd import hip
    g = torch.Generator().manual_seed(3 + layers)
    q = lambda *s: torch.randn(*s, generator=g).to(DEV, BF)
    ws = [(q(ffn, DM), q(DM, ffn), q(DM, DM), q(3 * DM, DM)) for _ in range(layers)]
    w_out, b_out = q(D, DM), torch.randn(D, generator=g).to(DEV)

    def run(merged):
        full = lambda *s, dt=BF: torch.full(s, FILL, dtype=dt, device=DEV)
        o = dict(w_outT=full(DM, DP), w_out_pad=full(DP, DM), b_out_pad=full(DP, dt=torch.float32))
        items = []
        for l, (w1, w2, wo, wq) in enumerate(ws):
            o[f"pk{l}"] = full(hip.ffn_chain_packed_elems(DM, ffn))
            o[f"wqT{l}"] = full(DM, 3 * DM)
            items.append((w1, w2, o[f"pk{l}"], wo, wq))
        # whole 64 x 64 tiles on the 16-byte path (the layer weights) and a 300-row matrix into a pitched buffer on the other
        tr = [(ws[l][3], o[f"wqT{l}"]) for l in range(layers)] + [(w_out, o["w_outT"][:, :D])]
        ca = [(w_out, o["w_out_pad"][:D]), (b_out.view(1, D), o["b_out_pad"].view(1, -1)[:, :D])]
        tr = tr if extra in ("both", "transposes") else []
        ca = ca if extra in ("both", "casts") else []
        if merged:
            hip.ffn_chain_pack(items, transposes=tr, casts=ca)
        else:
            hip.ffn_chain_pack(items)
            for src, dst in ca:
                hip.cast2d(src, dst)
            hip.transpose_multi(tr)
        torch.cuda.synchronize()
        return o
    want, got = run(False), run(True)
    if extra == "both":
        assert bool((want["w_outT"][:, D:] == FILL).all()) and not bool((want["w_outT"][:, :D] == FILL).all())
        assert bool((want["b_out_pad"][D:] == FILL).all()) and torch.equal(want["b_out_pad"][:D], b_out)
    _same(got, want, f"{layers} layers, ffn {ffn}, {extra}")


def _trainer_run(no_merge, use_graph, batches):
    from inferbiomechanics_amd.engine import HipTrainer
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    TU.no_head_merge = no_merge
    try:
        torch.manual_seed(0)
        m = DiffusionTransformer(D, T, d_model=512, num_heads=8, dim_feedforward=1024, num_layers=2, device=DEV, compute_dtype=BF)
        tr = HipTrainer(m, "diffusion", "rmsprop", 1e-3, use_graph=use_graph)
        losses = []
        for b in batches:
            tr.step(b)
            losses.append(tr.loss_value())
        torch.cuda.synchronize()
        state = {"flat": tr.flat.clone(), "s1": None if tr.s1 is None else tr.s1.clone(),
                 "s2": None if tr.s2 is None else tr.s2.clone()}
        return losses, {k: v.detach().clone() for k, v in m.state_dict().items()}, state
    finally:
        del TU.no_head_merge


@pytest.fixture(scope="module")
def trainer_reference():
    g = torch.Generator().manual_seed(5)
    batches = [(torch.randn(3, T, D, generator=g).to(DEV, BF), torch.randint(0, 1000, (3,), generator=g).to(DEV),
                torch.randn(3, T, D, generator=g).to(DEV, BF)) for _ in range(3)]
    return batches, _trainer_run(True, False, batches)        # the old launch sequence, eager: computed once


@pytest.mark.parametrize("no_merge,use_graph", [(False, False), (False, True), (True, True)])
def test_trainer_steps_are_bit_equal_to_the_old_sequence(trainer_reference, no_merge, use_graph):
    batches, (l0, p0, s0) = trainer_reference
    l1, p1, s1 = _trainer_run(no_merge, use_graph, batches)
    assert l1 == l0, (l1, l0)
    for k in p0:
        assert torch.equal(p1[k], p0[k]), k
    for k in s0:
        assert (s0[k] is None) == (s1[k] is None) and (s0[k] is None or torch.equal(s1[k], s0[k])), k


def test_head_launch_shape():
    """one eager step at whole-layer-launch size: at most 6 launches and exactly one fork ahead of the first whole-layer launch"""
    from inferbiomechanics_amd import hip, plans
    from inferbiomechanics_amd.engine import HipTrainer
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    Bt, Tt, Dt = 128, 32, 40
    g = torch.Generator().manual_seed(9)
    batch = (torch.randn(Bt, Tt, Dt, generator=g).to(DEV, BF), torch.randint(0, 1000, (Bt,), generator=g).to(DEV),
             torch.randn(Bt, Tt, Dt, generator=g).to(DEV, BF))
    torch.manual_seed(3)
    m = DiffusionTransformer(Dt, Tt, d_model=512, num_heads=8, dim_feedforward=512, num_layers=2, device=DEV, compute_dtype=BF)
    tr = HipTrainer(m, "diffusion", "sgd", 1e-2, use_graph=False)
    forks, real_run = [], plans.Branch.run

    def counting_run(self, fn):
        if self.on:
            forks.append((self.name, len(rec.calls)))
        return real_run(self, fn)
    plans.Branch.run = counting_run
    try:
        with hip.record_launches() as rec:
            tr.step(batch)
    finally:
        plans.Branch.run = real_run
    torch.cuda.synchronize()
    names = [n for n, _ in rec.calls]
    first = names.index("ib_ffn_chain_fwd_attn")
    head = names[:first]
    assert len(head) <= 6, head
    assert "ib_tr_head_prep" in head and "ib_ffn_chain_pack_ex" in head, head
    assert not {"ib_tiny_matmul", "ib_cast2d", "ib_transpose_multi", "ib_time_mlp_fwd", "ib_ffn_chain_pack"} & set(head), head
    assert [n for n, at in forks if at < first] == ["tr_wt"], forks
