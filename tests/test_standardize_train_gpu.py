"""`train --standardize` on the GPU, in process: the checkpoint carries the statistics the cache was built with, a resumed
run keeps them, a resume without the flag is refused; and the --eager loop's batch, standardised on the device from the
DataLoader's fp32 windows, is the batch the window cache holds -- both are the fp32 affine rounded to bf16 once, so they
agree bit for bit."""
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def args(ck, *more):
    return ['--no-wandb', '--batch-size', '8', '--data-loading-workers', '0', '--model-type', 'diffusion-mlp', '--feat-dim', '24',
            '--hidden-dims', '32', '32', '--stride', '1', '--history-len', '6', '--compute-dtype', 'bf16', '--seed', '7',
            '--checkpoint-dir', ck] + list(more)


def latest(ck):
    return torch.load(sorted(glob.glob(os.path.join(ck, "diffusion-mlp", "*.pt")), key=os.path.getmtime)[-1], map_location="cpu")


def test_checkpoint_statistics_resume_and_refusal(tmp_path):
    from inferbiomechanics_amd.main import main
    ck = str(tmp_path / "ck")
    run = ['--synthetic-windows', '2048', '--window-cache', 'hbm', '--standardize', '--max-steps', '4']
    assert main(['train', '--epochs', '1'] + args(ck, *run))
    first = latest(ck)
    st = first["column_stats"]
    assert tuple(st.shape) == (24, 2) and st.dtype == torch.float32 and torch.isfinite(st).all() and (st[:, 1] > 0).all()
    # the synthetic table is N(0, 1): 2048 x 6 rows put every mean within 6 / sqrt(12288) of 0 and every scale near 1
    assert st[:, 0].abs().max() < 0.06 and (st[:, 1] - 1).abs().max() < 0.06
    assert main(['train', '--epochs', '2'] + args(ck, *run))
    second = latest(ck)
    assert second["epoch"] == 1 and torch.equal(second["column_stats"].view(torch.int32), st.view(torch.int32))
    with pytest.raises(SystemExit, match="--standardize"):
        main(['train', '--epochs', '3'] + args(ck, '--synthetic-windows', '2048', '--window-cache', 'hbm', '--max-steps', '4'))


def test_eager_loop_draws_the_batch_the_cache_holds(tmp_path, monkeypatch):
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.data.WindowCache import DeviceMotionCache
    from inferbiomechanics_amd.main import main
    ck, path = str(tmp_path / "ck"), str(tmp_path / "motion.npy")
    common = ['--synthetic-windows', '64', '--standardize', '--max-steps', '1', '--max-dev-steps', '1']
    assert main(['train', '--epochs', '1', '--window-cache', path] + args(ck, *common))
    stats = latest(ck)["column_stats"]
    cache = DeviceMotionCache(torch.from_numpy(np.load(path)), "cuda", BF, stats=stats)
    seen = []
    real = hip.q_sample

    def spy(x0, *a, **kw):
        seen.append(x0.detach().clone())
        return real(x0, *a, **kw)
    monkeypatch.setattr(hip, "q_sample", spy)
    assert main(['train', '--epochs', '2', '--eager'] + args(ck, *common))
    train_batch = seen[-1]                                             # the dev batch comes first, the one training step last
    assert tuple(train_batch.shape) == (8, 6, 24) and train_batch.dtype == BF
    rows = cache.table[:8, :6 * 24].reshape(8, 6, 24)
    assert torch.equal(train_batch.view(torch.int16), rows.view(torch.int16))
    raw = torch.from_numpy(np.load(path))[:8].to("cuda", BF)
    assert not torch.equal(train_batch, raw), "it is not the raw batch"
