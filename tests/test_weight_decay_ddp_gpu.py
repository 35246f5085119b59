"""Decoupled weight decay under data parallelism over REAL RCCL on a one-rank group (a fresh process: `nccl` backend,
IB_DDP_SELFTEST=1 makes the trainer issue its collectives although world == 1, as in tests/test_ddp_rccl_gpu.py): the
overlapped transformer step, whose optimizer runs per bucket behind that bucket's all-reduce plus a last self-counting
launch that names the buckets' ranges as done.  Every one of those launches carries the one decay table and its slice's
origin, each parameter is decayed exactly once per step, and after each of 4 steps the parameters equal BITWISE those of
the single-GPU fused trainer with the same decay -- in the cut-graph form (the per-bucket launches are host actions of the
replay) and in the captured form (one graph per step; forced through IB_GRAPH_COLLECTIVES as that test does).  -m gpu."""
import os
import socket

import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS, WD, BASE = 4, 0.1, 1e-3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(port, q):
    try:
        import faulthandler
        import sys
        import tempfile
        root_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        _fh = open(os.path.join(tempfile.gettempdir(), f"weight_decay_ddp_hang_{os.getpid()}.txt"), "w")
        faulthandler.dump_traceback_later(150, exit=True, file=_fh)      # a hang shows where, and ends the process
        sys.path.insert(0, root_)
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1",
                          HSA_ENABLE_IPC_MODE_LEGACY="0", IB_DDP_SELFTEST="1",
                          TORCH_NCCL_CUDA_EVENT_CACHE=os.environ.get("TORCH_NCCL_CUDA_EVENT_CACHE", "0"),
                          TORCH_NCCL_TRACE_BUFFER_SIZE=os.environ.get("TORCH_NCCL_TRACE_BUFFER_SIZE", "2000"),
                          TORCH_FR_BUFFER_SIZE=os.environ.get("TORCH_FR_BUFFER_SIZE", "2000"))
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        from inferbiomechanics_amd import hip
        from inferbiomechanics_amd.engine import HipTrainer
        from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
        B, T, D, dt = 128, 32, 48, torch.bfloat16              # B * T = 4096 rows: the fused layer launches' threshold
        g = torch.Generator().manual_seed(3)
        batches = [(torch.randn(B, T, D, generator=g).to("cuda", dt), torch.randint(0, 1000, (B,), generator=g).cuda(),
                    torch.randn(B, T, D, generator=g).to("cuda", dt)) for _ in range(STEPS)]

        def run(ddp: bool, wd: float, captured: bool = False):
            os.environ["IB_GRAPH_COLLECTIVES"] = "1" if captured else "0"
            os.environ["IB_DDP_SELFTEST"] = "1" if ddp else "0"
            print(f"[arm] ddp={ddp} wd={wd} captured={captured}", file=sys.stderr, flush=True)
            torch.manual_seed(7)
            model = DiffusionTransformer(D, T, d_model=512, num_heads=8, dim_feedforward=1024, num_layers=3,
                                         temporal_embedding_dim=6, temb_dim=32, temb_hidden=64, device="cuda", compute_dtype=dt)
            tr = HipTrainer(model, "diffusion", "adam", BASE, bucket_mb=0.5, overlap_comm=True if ddp else None,
                            weight_decay=wd)
            seen, real = [], hip.optim_step

            def counted(*a, **k):
                lo = (a[1].data_ptr() - tr.flat.data_ptr()) // 4
                seen.append((k.get("weight_decay", 0.0), k.get("decay_table") is tr.decay_table, k.get("decay_origin", 0) == lo,
                             k.get("ticket") is not None))
                return real(*a, **k)
            hip.optim_step = counted
            losses, flats = [], []
            try:
                for b in batches:
                    tr.step(b)
                    torch.cuda.synchronize()
                    losses.append(tr.loss_value())
                    flats.append(tr.flat.detach().cpu().numpy().copy())
            finally:
                hip.optim_step = real
            info = {"ddp": tr.ddp, "overlap": tr.overlap_comm, "buckets": len(tr.buckets.ranges), "bucket_opt": tr.bucket_opt,
                    "recorded": tr._rec is not None, "first_step": seen[:len(tr.buckets.ranges) + 1] if ddp else seen[:1],
                    "graph_cuts": sum(1 for kk, _ in tr._rec.actions if kk == "host") if tr._rec is not None else -1,
                    "table_n": tr.decay_table.n if tr.decay_table is not None else -1, "wd": tr.weight_decay}
            return losses, flats, info

        out = {"single": run(False, WD), "cut": run(True, WD), "captured": run(True, WD, captured=True)}
        dist.barrier()
        dist.destroy_process_group()
        faulthandler.cancel_dump_traceback_later()
        _fh.close()
        os.unlink(_fh.name)                           # no hang: nothing to hand back
        q.put(("ok", out))
    except Exception:  # pragma: no cover
        import traceback
        q.put(("FAIL: " + traceback.format_exc(), None))


def test_per_bucket_optimizer_decays_once_and_equals_the_fused_trainer_bitwise():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import numpy as np
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_worker, args=(_free_port(), q))
    p.start()
    status, out = q.get(timeout=200)
    p.join(timeout=120)
    assert status == "ok", status
    ls, fs, i_s = out["single"]
    assert not i_s["ddp"] and i_s["recorded"] and i_s["table_n"] >= 1, i_s
    assert all(s[0] == i_s["wd"] and s[1] and s[2] for s in i_s["first_step"]), i_s["first_step"]
    for arm in ("cut", "captured"):
        l, f, i = out[arm]
        assert i["ddp"] and i["overlap"] and i["bucket_opt"] and i["recorded"] and i["buckets"] > 1, (arm, i)
        # every optimizer launch of a step carries the decay, the one table and its own origin: one per bucket, then the last
        assert len(i["first_step"]) == i["buckets"] + 1, (arm, i["first_step"])
        assert all(s[0] == i["wd"] and s[1] and s[2] for s in i["first_step"]), (arm, i["first_step"])
        assert [s[3] for s in i["first_step"]] == [False] * i["buckets"] + [True], (arm, i["first_step"])
        assert (i["graph_cuts"] >= i["buckets"]) if arm == "cut" else (i["graph_cuts"] == 0), (arm, i["graph_cuts"])
        assert l == ls, (arm, l, ls)
        for k in range(STEPS):
            assert np.array_equal(f[k].view(np.int32), fs[k].view(np.int32)), (arm, "parameters after step", k + 1)
