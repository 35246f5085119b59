"""HipTrainer(cond_drop = p): condition dropout in the training step (ib_q_sample_cond_drop in place of ib_q_sample_cond, nothing
else moves), on the 2-layer transformer denoiser (d_model 128) and the MLP denoiser of tests/test_cond_trainer_gpu.py at
B = 8, T = 12, D = 44, C = 14, three SGD steps.  Everything is held bit for bit: p = 0 is the cond_cols trainer; p = 1 is that
trainer fed batches whose conditioning columns are zero; p = 0.5 follows the restated per-step masks, replays from the
captured graph exactly as it runs eagerly, and is reproducible.  -m gpu."""
import pytest
import torch

from tests import cfg_restatement as CR
from tests.test_cond_trainer_gpu import BF, DEV, LR, batches, make

pytestmark = pytest.mark.gpu

B, T, D, C, STEPS = 8, 12, 44, 14, 3
KINDS = [("transformer", BF), ("mlp", BF), ("transformer", torch.float32)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def live_seed():
    """a noise seed under which the restated p = 0.5 mask of each of the three steps drops 2 .. 6 of the 8 windows"""
    for seed in range(1, 1000):
        if all(2 <= int(CR.drop_mask(B, 0.5, seed, s, 0).sum()) <= 6 for s in range(STEPS)):
            return seed
    raise AssertionError("no seed found")


def run(kind, dtype, use_graph, bs, seed=1, watch=None, **kw):
    """three SGD steps -> (losses, parameters, trainer); watch(step index, trainer) runs after every step"""
    from inferbiomechanics_amd.engine import HipTrainer
    model, _ = make(kind, dtype, D, T)
    torch.manual_seed(seed)                                  # the trainer's noise seed is torch's
    tr = HipTrainer(model, "diffusion", "sgd", LR, use_graph=use_graph, cond_cols=C, **kw)
    assert tr.noise_seed == seed
    losses = []
    for i in range(STEPS):
        x0, t, eps = bs[i % len(bs)]
        tr.step((x0.to(DEV), t.to(DEV), eps.to(DEV)))
        losses.append(tr.loss_value())
        if watch is not None:
            watch(i, tr)
    torch.cuda.synchronize()
    return losses, tr.flat.detach().clone(), tr


@pytest.mark.parametrize("kind,dtype", KINDS)
def test_cond_drop_zero_is_the_cond_cols_trainer_bitwise(kind, dtype):
    from inferbiomechanics_amd import hip
    bs = batches(3, B, T, D, dtype, seed=7)
    a = run(kind, dtype, False, bs)
    with hip.record_launches() as rec:
        b = run(kind, dtype, False, bs, cond_drop=0.0)
    names = [n for n, _ in rec.calls]
    assert names.count("ib_q_sample_cond") == STEPS and "ib_q_sample_cond_drop" not in names
    assert a[0] == b[0] and torch.equal(a[1], b[1])
    assert not any(k[0] == "cond_drop" for k in b[2]._sig if isinstance(k, tuple) and k), "p = 0 adds nothing to the signature"


@pytest.mark.parametrize("kind,dtype", KINDS)
def test_cond_drop_one_is_training_on_zeroed_conditions_bitwise(kind, dtype):
    from inferbiomechanics_amd import hip
    bs = batches(3, B, T, D, dtype, seed=7)
    zeroed = []
    for x0, t, eps in bs:
        z = x0.clone()
        z[..., :C] = 0
        zeroed.append((z, t, eps))
    with hip.record_launches() as rec:
        a = run(kind, dtype, False, bs, cond_drop=1.0)
    names = [n for n, _ in rec.calls]
    assert names.count("ib_q_sample_cond_drop") == STEPS and "ib_q_sample_cond" not in names and "ib_q_sample" not in names
    b = run(kind, dtype, False, zeroed)
    assert a[0] == b[0] and torch.equal(a[1], b[1])
    c = run(kind, dtype, False, bs)
    assert a[0] != c[0], "dropping every condition must change the loss"


@pytest.mark.parametrize("kind,dtype", KINDS)
def test_cond_drop_half_is_live_under_graph_replay(kind, dtype):
    bs = batches(3, B, T, D, dtype, seed=7)
    seed = live_seed()
    seen = []

    def watch(i, tr):
        # the step's x_t: the conditioning columns of a window are x0's or all zero, by the restated mask of step i
        torch.cuda.synchronize()
        Dp = tr.plan.train_pitch(D, B * T) if hasattr(tr.plan, "train_pitch") else (D + 7) // 8 * 8
        xt = tr.plan.buf.get("tr.xt", (B * T, Dp), dtype)[:, :C].reshape(B, T, C).cpu()
        x0 = bs[i % len(bs)][0][..., :C]
        mask = CR.drop_mask(B, 0.5, seed, i, 0)
        assert 2 <= int(mask.sum()) <= 6
        for b in range(B):
            assert torch.equal(xt[b], torch.zeros_like(xt[b]) if mask[b] else x0[b]), (i, b, mask.tolist())
        seen.append(mask.tolist())

    eager = run(kind, dtype, False, bs, seed=seed, watch=watch, cond_drop=0.5)
    graph = run(kind, dtype, True, bs, seed=seed, watch=watch, cond_drop=0.5)
    assert graph[2]._rec is not None, "the step was never captured"
    assert ("cond_drop", 0.5) in graph[2]._sig
    assert seen[:STEPS] == seen[STEPS:] and len({tuple(m) for m in seen}) > 1, "every step draws its own mask"
    assert eager[0] == graph[0] and torch.equal(eager[1], graph[1]), "captured and uncaptured runs must agree bit for bit"
    again = run(kind, dtype, True, bs, seed=seed, cond_drop=0.5)
    assert again[0] == graph[0] and torch.equal(again[1], graph[1]), "the run must be reproducible"
    plain = run(kind, dtype, True, bs, seed=seed)
    assert plain[0][STEPS - 1] != graph[0][STEPS - 1], "the replayed step's loss must feel the mask"
    assert plain[0] != graph[0]
