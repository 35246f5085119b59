"""`main.py analyze --use-ema` on a diffusion-mlp checkpoint written by `train --ema-decay` (EMA different from the last
weights): the report and the inferred labels equal those of a plain run on a checkpoint whose model_state_dict is the
EMA weights, and differ from the run without the flag; without the flag the output is that of the same checkpoint with
the EMA keys removed (what the loader read before the EMA existed).  -m gpu."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def test_analyze_use_ema(tmp_path, monkeypatch, capsys):
    from inferbiomechanics_amd.main import main
    from inferbiomechanics_amd.models.DiffusionLabelPredictor import DiffusionLabelPredictor
    mt = 'diffusion-mlp'
    model_args = ['--no-wandb', '--data-loading-workers', '0', '--model-type', mt, '--hidden-dims', '64', '64']
    src = str(tmp_path / "src")
    assert main(['train', '--synthetic-windows', '32', '--feat-dim', '177', '--epochs', '1', '--max-steps', '4',
                 '--batch-size', '8', '--checkpoint-dir', src, '--ema-decay', '0.5', '--no-ema-warmup',
                 '--learning-rate', '1e-2'] + model_args)
    (name,) = [f for f in os.listdir(os.path.join(src, mt)) if f.endswith('.pt')]
    ck = torch.load(os.path.join(src, mt, name), map_location='cpu')
    assert any(not torch.equal(ck['ema_state_dict'][k], v) for k, v in ck['model_state_dict'].items())
    swapped = dict(ck, model_state_dict=ck['ema_state_dict'])
    stripped = {k: ck[k] for k in ('epoch', 'model_state_dict', 'optimizer_state_dict')}
    for d, payload in (("a", ck), ("b", ck), ("swapped", swapped), ("stripped", stripped)):   # analyze appends to its CSVs
        os.makedirs(str(tmp_path / d / mt))
        torch.save(payload, str(tmp_path / d / mt / name))

    outs = []
    orig = DiffusionLabelPredictor.__call__

    def spy(self, inputs, labels=None, draw=0):
        out = orig(self, inputs, labels, draw)
        outs.append({k: v.detach().cpu().clone() for k, v in out.items()})
        return out
    monkeypatch.setattr(DiffusionLabelPredictor, '__call__', spy)

    def analyze(d, *extra):
        outs.clear()
        capsys.readouterr()
        assert main(['analyze', '--synthetic-windows', '4', '--sample-steps', '10', '--checkpoint-dir', str(tmp_path / d)]
                    + model_args + list(extra))
        report = capsys.readouterr().out
        assert 'Final dev results:' in report and 'Force Avg Err' in report
        rows = [open(os.path.join(str(tmp_path / d), mt, f)).read() for f in ('dev_analysis.csv', 'train_analysis.csv')]
        return report, rows, list(outs)

    def same(a, b):
        return a[0] == b[0] and a[1] == b[1] and len(a[2]) == len(b[2]) and \
            all(torch.equal(x[k], y[k]) for x, y in zip(a[2], b[2]) for k in x)

    with_ema = analyze("a", "--use-ema")
    on_swapped = analyze("swapped")
    plain = analyze("b")
    on_stripped = analyze("stripped")
    assert same(with_ema, on_swapped)
    assert same(plain, on_stripped)
    assert not same(with_ema, plain) and with_ema[0] != plain[0]
    with pytest.raises(ValueError, match="no EMA"):
        analyze("stripped", "--use-ema")
