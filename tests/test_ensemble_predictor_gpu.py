"""DiffusionLabelPredictor(interval=L) and `analyze --interval L` on the GPU.  -m gpu.

The K = 3 members of an ensemble are reproduced one by one with single-sample predictors (a K = 1 call returns its member's
values exactly); the restatement (tests/ensemble_restatement.py) over their stack must equal last_interval, last_crps,
last_rank and last_inside, on windows and on stitched trials, and the outputs and last_std must not change by a bit against
the same predictor without the interval."""
import os
import re

import numpy as np
import pytest
import torch

from tests import ensemble_restatement as ER
from tools import sampler_trace

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
S, K, L = sampler_trace.S, 3, 0.5


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from inferbiomechanics_amd import hip
    hip.lib()


@pytest.fixture(scope="module")
def model():
    return sampler_trace.Run(device=DEV).model(BF, **sampler_trace.LABELS)


def _labels(n, frames):
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import LOSS_KEY_ORDER, LOSS_KEY_WIDTHS
    g = torch.Generator().manual_seed(3)
    return {k: torch.randn(n, frames, w, generator=g) * 0.5 for k, w in zip(LOSS_KEY_ORDER, LOSS_KEY_WIDTHS)}


def _block(d):
    """the four-key layout -> [B, F, 30] on the host"""
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import LOSS_KEY_ORDER
    return torch.cat([d[k].detach().cpu() for k in LOSS_KEY_ORDER], dim=2)


@pytest.mark.parametrize("path", ["windows", "trials"])
def test_order_statistics_of_the_reproduced_members(model, path):
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import LOSS_KEY_ORDER
    from inferbiomechanics_amd.diffusion.ensemble import interval_levels, quantile_position
    from inferbiomechanics_amd.models.DiffusionLabelPredictor import DiffusionLabelPredictor
    frames, draw, B = (10, 2, 2) if path == "windows" else (20, 1, 2)
    r = sampler_trace.Run(device=DEV)
    inputs = {k: v.to(DEV) for k, v in sampler_trace._label_inputs(r, B, frames).items()}
    labels = _labels(B, frames)

    def run(pred, inp, d, lab=None):
        if path == "windows":
            return pred(inp, lab, draw=d)
        return pred.predict_trial_ensemble(inp, hop=4, draw=d, labels=lab)

    pred = DiffusionLabelPredictor(model, S, seed=3, eta=1.0, num_samples=K, interval=L)
    out = run(pred, inputs, draw, labels)
    plain = DiffusionLabelPredictor(model, S, seed=3, eta=1.0, num_samples=K)
    want_out = run(plain, inputs, draw, labels)
    assert plain.last_interval is None and plain.last_crps is None and plain.last_rank is None and plain.last_inside is None
    for k in LOSS_KEY_ORDER:
        assert torch.equal(out[k], want_out[k]) and torch.equal(pred.last_std[k], plain.last_std[k]), k
        assert bool((pred.last_std[k] > 0).any()), "the members differ"

    single = DiffusionLabelPredictor(model, S, seed=3, eta=1.0)
    members = []
    for b in range(B):
        one = {k: v[b:b + 1] for k, v in inputs.items()}
        members.append(torch.stack([_block(run(single, one, (draw + b) * K + j)) for j in range(K)], dim=1))
    stack = torch.cat(members)                                          # [B, K, F, 30]
    assert tuple(stack.shape) == (B, K, frames, 30) and stack.dtype == torch.float32
    pos = [quantile_position(q, K) for q in interval_levels(L)]
    want = ER.restate(ER.members_of(stack, 0, 30), pos, _block(labels).numpy().reshape(-1))
    got = {"lo": pred.last_interval["lo"], "median": pred.last_interval["median"], "hi": pred.last_interval["hi"],
           "crps": pred.last_crps, "rank": pred.last_rank, "inside": pred.last_inside}
    for k, d in got.items():
        g = _block(d).numpy().reshape(-1)
        assert g.dtype == want[k].dtype and np.array_equal(g == want[k], np.ones_like(g, dtype=bool)), k
    hist = np.bincount(want["rank"], minlength=K + 1)
    print(f"{path}: rank histogram {hist.tolist()}, coverage {float(want['inside'].mean()):.3f}")
    assert bool((_block(pred.last_interval["lo"]) <= _block(pred.last_interval["median"])).all())
    assert bool((_block(pred.last_interval["median"]) <= _block(pred.last_interval["hi"])).all())

    # without labels: the interval alone, and the score of the call before is gone
    run(pred, inputs, draw)
    assert pred.last_crps is None and pred.last_rank is None and pred.last_inside is None
    for k in ("lo", "median", "hi"):
        assert torch.equal(_block(pred.last_interval[k]), _block(got[k])), k


def test_analyze_reports_calibration(tmp_path, capsys):
    from inferbiomechanics_amd.diffusion.ensemble import calibrated_coverage
    from inferbiomechanics_amd.main import main
    ck = str(tmp_path / "ck")
    common = ['--no-wandb', '--checkpoint-dir', ck, '--data-loading-workers', '0', '--model-type', 'diffusion-mlp',
              '--hidden-dims', '64', '64']
    assert main(['train', '--synthetic-windows', '16', '--feat-dim', '177', '--epochs', '1', '--max-steps', '2',
                 '--batch-size', '8'] + common)
    ens = ['analyze', '--synthetic-windows', '6', '--sample-steps', '10', '--sample-seed', '3', '--num-samples', '4',
           '--sample-eta', '1'] + common
    capsys.readouterr()
    assert main(ens)
    plain = capsys.readouterr().out
    assert 'Ensemble calibration' not in plain and 'Rank histogram' not in plain and plain.count('Ensemble spread (') == 2
    assert main(ens + ['--interval', '0.8'])
    out = capsys.readouterr().out
    new = [l for l in out.splitlines() if l.startswith(('Ensemble calibration (', 'Rank histogram ('))]
    assert [re.match(r'[\w ]+\((\w+)', l).group(1) for l in new] == ['dev', 'dev', 'train', 'train']
    kept = [l for l in out.splitlines(keepends=True) if not l.startswith(('Ensemble calibration (', 'Rank histogram ('))]
    assert ''.join(kept) == plain, "without the new lines the output is the run without the flag"
    lines = out.splitlines()
    for split in ('dev', 'train'):
        at = next(i for i, l in enumerate(lines) if l.startswith(f'Ensemble spread ({split}, '))
        assert lines[at + 1].startswith(f'Ensemble calibration ({split}, 4 samples per window, level 0.8): cop: coverage ')
        assert lines[at + 2].startswith(f'Rank histogram ({split}): cop: [')
        assert lines[at + 1].count(f'(calibrated ensemble: {calibrated_coverage(0.8, 4):.4f})') == 4
        assert f'{calibrated_coverage(0.8, 4):.4f}' == '0.6000'
        names = re.findall(r'(\w+): \[([0-9 ]+)\]', lines[at + 2])
        assert [n for n, _ in names] == ['cop', 'force', 'torque', 'wrench']
        for (name, counts), width in zip(names, (6, 6, 6, 12)):
            counts = [int(c) for c in counts.split()]
            assert len(counts) == 5 and sum(counts) == 6 * 10 * width, (name, "six windows of ten frames are scored")
        cov = [float(c) for c in re.findall(r'coverage ([0-9.]+) \(', lines[at + 1])]
        assert len(cov) == 4 and all(0.0 <= c <= 1.0 for c in cov)
    assert main(ens + ['--interval', '0.8', '--sample-batch', '3'])
    assert capsys.readouterr().out == out, "--sample-batch does not change the report"
    with pytest.raises(SystemExit, match="--num-samples >= 2"):
        main(['analyze', '--synthetic-windows', '6', '--sample-steps', '10', '--interval', '0.8'] + common)
    assert os.path.exists(os.path.join(ck, 'diffusion-mlp', 'dev_analysis.csv'))
