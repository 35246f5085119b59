"""The EMA of the weights under data parallelism with real kernels: two fresh processes share this one GPU over gloo (the
pattern of test_ddp_numerics_gpu.py), each trains a few graph-replayed steps on its shard with HipTrainer(ema_decay=...),
and the EMA -- advanced by the one-bucket policy's single launch, or by the overlapped policy's per-bucket launches plus
the step's last launch -- ends bitwise equal on both ranks, as do the parameters; the EMA also matches a float64
recurrence over the rank's parameter trajectory.  -m gpu."""
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = {
    # name: (model kind, overlap_comm)
    "mlp_one_bucket": ("mlp", False),
    "mlp_overlap": ("mlp", True),
    "transformer_overlap": ("transformer", True),
    "transformer_one_bucket": ("transformer", False),
}
B2, T, D, STEPS, DECAY = 8, 10, 44, 5, 0.8


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, case, q):
    try:
        import sys
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          HSA_ENABLE_IPC_MODE_LEGACY="0")
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from inferbiomechanics_amd.engine import HipTrainer
        from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionMLP, DiffusionTransformer
        kind, overlap = CASES[case]
        torch.manual_seed(100 + rank)                   # different initialisation per rank: the broadcast equalises
        if kind == "transformer":
            model = DiffusionTransformer(D, T, d_model=64, num_heads=2, dim_feedforward=128, num_layers=2,
                                         temporal_embedding_dim=6, temb_dim=16, temb_hidden=32, device="cuda")
        else:
            model = DiffusionMLP(D, [64, 96], temb_dim=32, temb_hidden=48, device="cuda")
        tr = HipTrainer(model, "diffusion", "adam", 1e-3, bucket_mb=0.02, overlap_comm=overlap, ema_decay=DECAY)
        assert tr.world == world and tr.ddp and tr.overlap_comm == overlap
        g = torch.Generator().manual_seed(123)
        e = tr.ema.detach().cpu().double().clone()
        err = 0.0
        for k in range(STEPS):
            x0, t, eps = torch.randn(B2, T, D, generator=g), torch.randint(0, 1000, (B2,), generator=g), \
                torch.randn(B2, T, D, generator=g)
            rows = slice(rank, None, world)
            tr.step((x0[rows].cuda().contiguous(), t[rows].cuda().contiguous(), eps[rows].cuda().contiguous()))
            torch.cuda.synchronize()
            d = float(np.float32(min(DECAY, (2.0 + k) / (11.0 + k))))
            e = d * e + float(np.float32(1.0) - np.float32(d)) * tr.flat.detach().cpu().double()
            err = max(err, float((tr.ema.detach().cpu().double() - e).abs().max()) / float(tr.flat.abs().max()))
        assert tr._rec is not None
        out = {"flat": tr.flat.detach().cpu().numpy().copy(), "ema": tr.ema.detach().cpu().numpy().copy(), "err": err,
               "bucket_opt": tr.bucket_opt, "buckets": len(tr.buckets.ranges)}
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok", out))
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, "FAIL: " + traceback.format_exc(), None))


@pytest.mark.parametrize("case", list(CASES))
def test_ema_is_bitwise_equal_on_both_ranks(case):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, case, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=120)
    assert all(r[1] == "ok" for r in res), [r[1] for r in res]
    a, b = res[0][2], res[1][2]
    assert np.array_equal(a["flat"].view(np.int32), b["flat"].view(np.int32))
    assert np.array_equal(a["ema"].view(np.int32), b["ema"].view(np.int32))
    assert not np.array_equal(a["ema"], a["flat"])
    assert a["err"] <= 1e-6 and b["err"] <= 1e-6, (a["err"], b["err"])
    if CASES[case] == ("transformer", True):
        assert a["bucket_opt"] and a["buckets"] > 1            # the per-bucket optimizer launches carried the EMA
