"""Equivariance of the label predictor under per-column standardisation, with no trained model: a random-weight
diffusion-transformer with statistics, given raw inputs, equals bit for bit the restated de-standardisation
(tests/standardize_restatement.py) of the same denoiser without statistics given host-standardised inputs.  The sampler runs
on the same bits either way, so nothing but the two affine launches is under test.  For an ensemble the members of the
plain run are de-standardised on the host and the existing ensemble kernels run over them: that is what the predictor with
statistics does on the device."""
import numpy as np
import pytest
import torch

from tests import standardize_restatement as SR

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
T, D, S, B = 8, 40, 10, 2
LW = 30                                  # the label block


@pytest.fixture(scope="module")
def setup():
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import INPUT_KEY_ORDER, LOSS_KEY_ORDER, LOSS_KEY_WIDTHS
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    torch.manual_seed(0)
    model = DiffusionTransformer(D, T, d_model=64, num_heads=4, dim_feedforward=128, num_layers=2, compute_dtype=BF, device="cuda")
    g = torch.Generator().manual_seed(9)
    mean = torch.randn(D, generator=g) * 3
    mean[3], mean[D - LW + 8] = 900.0, -250.0                          # an offset input column and an offset label column
    scale = torch.rand(D, generator=g) * 3 + 0.2
    stats = torch.stack([mean, scale], dim=1).to(torch.float32)
    from inferbiomechanics_amd import hip
    inv = hip.inv_scale(stats[:, 1].contiguous())

    def batch(F):
        raw = stats[:, 0] + stats[:, 1] * torch.randn(B, F, D, generator=g)
        raw = raw.to(torch.float32)
        z = torch.from_numpy(SR.affine(raw.numpy(), stats[:, 0].numpy(), inv.numpy(), SR.STANDARDIZE))
        assert len(INPUT_KEY_ORDER) == D - LW                           # one column per input key
        split_in = lambda m: {k: m[:, :, i:i + 1].contiguous() for i, k in enumerate(INPUT_KEY_ORDER)}
        labels, c = {}, D - LW
        for k, w in zip(LOSS_KEY_ORDER, LOSS_KEY_WIDTHS):
            labels[k] = raw[:, :, c:c + w].contiguous()
            c += w
        return split_in(raw), split_in(z), labels
    return model, stats, batch


def label_stats(stats):
    return stats[D - LW:, 0].numpy(), stats[D - LW:, 1].numpy()


def block(out):
    """the four-key layout back as one [B, F, 30] array"""
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import LOSS_KEY_ORDER
    return np.concatenate([out[k].detach().cpu().numpy() for k in LOSS_KEY_ORDER], axis=2)


def predictors(model, **kw):
    from inferbiomechanics_amd.models.DiffusionLabelPredictor import DiffusionLabelPredictor
    return DiffusionLabelPredictor(model, S, seed=3, **kw), DiffusionLabelPredictor(model, S, seed=3, **kw)


@pytest.mark.parametrize("what", ["window", "trial"])
def test_single_trajectory_is_the_destandardised_plain_one(setup, what):
    model, stats, batch = setup
    raw_in, z_in, _ = batch(T if what == "window" else T + 7)
    plain, with_stats = predictors(model)
    call = (lambda p, x: p(x, draw=4)) if what == "window" else (lambda p, x: p.predict_trial(x, draw=4))
    model.column_stats = None
    z_out = block(call(plain, z_in))
    model.column_stats = stats
    try:
        got = call(with_stats, raw_in)
    finally:
        model.column_stats = None
    m, s = label_stats(stats)
    want = SR.affine(z_out, m, s, SR.DESTANDARDIZE)
    assert all(v.dtype == torch.float32 for v in got.values())
    assert np.array_equal(SR.bits(block(got)), SR.bits(want))
    assert not np.array_equal(SR.bits(SR.bf16_round(want)), SR.bits(want)), "fp32 out: bf16 would quantise the offset column"
    assert with_stats.last_std is None


def test_ensemble_statistics_are_taken_over_raw_members(setup):
    from inferbiomechanics_amd import hip
    model, stats, batch = setup
    raw_in, z_in, labels = batch(T)
    K = 3
    plain, with_stats = predictors(model, eta=1.0, num_samples=K, interval=0.8)
    members = []
    orig = plain.sampler.sample

    def spy(*a, **kw):
        x = orig(*a, **kw)
        members.append(x.detach().clone())
        return x
    plain.sampler.sample = spy
    model.column_stats = None
    plain(z_in, draw=4)
    (x,) = members
    assert tuple(x.shape) == (B * K, T, D) and x.dtype == BF
    model.column_stats = stats
    try:
        got = with_stats(raw_in, labels, draw=4)
    finally:
        model.column_stats = None
    raw_members = torch.from_numpy(SR.affine(SR.widen(x), stats[:, 0].numpy(), stats[:, 1].numpy(), SR.DESTANDARDIZE))
    x4 = raw_members.to("cuda").view(B, K, T, D).contiguous()
    mean, std = hip.ensemble_stats(x4)
    truth = torch.cat([labels[k] for k in labels], dim=2).contiguous().to("cuda")
    order = hip.ensemble_order(x4, (D - LW, LW), 0.8, truth)
    torch.cuda.synchronize()
    same = lambda a, b: np.array_equal(SR.bits(a), SR.bits(b))
    assert same(block(got), mean[:, :, D - LW:].cpu().numpy()), "mean"
    assert same(block(with_stats.last_std), std[:, :, D - LW:].cpu().numpy()), "last_std"
    for k in ("lo", "median", "hi"):
        assert same(block(with_stats.last_interval[k]), order[k].cpu().numpy()), k
    assert np.array_equal(block(with_stats.last_rank), order["rank"].cpu().numpy()), "last_rank"
    assert block(with_stats.last_rank).dtype == np.uint8 and (block(with_stats.last_std) > 0).any()
