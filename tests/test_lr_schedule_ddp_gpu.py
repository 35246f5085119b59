"""The learning-rate schedule under data parallelism over REAL RCCL on a one-rank group (a fresh process: `nccl` backend,
IB_DDP_SELFTEST=1 makes the trainer issue its collectives although world == 1, as in tests/test_ddp_rccl_gpu.py): the
overlapped transformer step, whose optimizer runs per bucket behind that bucket's all-reduce plus a last self-counting
launch.  12 steps of a cosine schedule with w = 3, T = 9, m = 0.1, in the cut-graph form (the per-bucket launches are host
actions of the replay) and in the captured form (one graph per step; forced through IB_GRAPH_COLLECTIVES as that test does:
no start-up probe in a test), each bitwise against the same data-parallel trainer run eagerly, without a schedule, with
its `lr` set on the host to LrSchedule.lr_at(base, k) before step k.  -m gpu."""
import os
import socket

import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS, W, T_TOTAL, M, BASE = 12, 3, 9, 0.1, 1e-3


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
        _fh = open(os.path.join(tempfile.gettempdir(), f"lr_schedule_ddp_hang_{os.getpid()}.txt"), "w")
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
        from inferbiomechanics_amd.lr_schedule import LrSchedule
        from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
        sch = LrSchedule("cosine", W, T_TOTAL, M)
        B, T, D, dt = 128, 32, 48, torch.bfloat16              # B * T = 4096 rows: the fused layer launches' threshold
        g = torch.Generator().manual_seed(3)
        batches = [(torch.randn(B, T, D, generator=g).to("cuda", dt), torch.randint(0, 1000, (B,), generator=g).cuda(),
                    torch.randn(B, T, D, generator=g).to("cuda", dt)) for _ in range(STEPS)]

        def run(scheduled: bool, use_graph: bool, captured: bool = False):
            os.environ["IB_GRAPH_COLLECTIVES"] = "1" if captured else "0"
            print(f"[arm] scheduled={scheduled} use_graph={use_graph} captured={captured}", file=sys.stderr, flush=True)
            torch.manual_seed(7)
            model = DiffusionTransformer(D, T, d_model=512, num_heads=8, dim_feedforward=1024, num_layers=3,
                                         temporal_embedding_dim=6, temb_dim=32, temb_hidden=64, device="cuda", compute_dtype=dt)
            tr = HipTrainer(model, "diffusion", "adam", BASE, bucket_mb=0.5, overlap_comm=True, use_graph=use_graph,
                            lr_schedule=sch if scheduled else None)
            names, real = [], hip.optim_step

            def counted(*a, **k):
                names.append(("sched" if k.get("lr_schedule") is not None else "plain", k.get("ticket") is not None))
                return real(*a, **k)
            hip.optim_step = counted
            losses, flats = [], []
            try:
                for k, b in enumerate(batches):
                    if not scheduled:
                        tr.lr = sch.lr_at(BASE, k + 1)
                    tr.step(b)
                    torch.cuda.synchronize()
                    losses.append(tr.loss_value())
                    flats.append(tr.flat.detach().cpu().numpy().copy())
            finally:
                hip.optim_step = real
            info = {"ddp": tr.ddp, "overlap": tr.overlap_comm, "buckets": len(tr.buckets.ranges), "bucket_opt": tr.bucket_opt,
                    "recorded": tr._rec is not None, "first_step": names[:len(tr.buckets.ranges) + 1],
                    "graph_cuts": sum(1 for kk, _ in tr._rec.actions if kk == "host") if tr._rec is not None else -1,
                    "next_lr": tr.current_lr()}
            return losses, flats, info

        out = {"yardstick": run(False, False), "cut": run(True, True), "captured": run(True, True, captured=True)}
        dist.barrier()
        dist.destroy_process_group()
        faulthandler.cancel_dump_traceback_later()
        _fh.close()
        os.unlink(_fh.name)                           # no hang: nothing to hand back
        q.put(("ok", out))
    except Exception:  # pragma: no cover
        import traceback
        q.put(("FAIL: " + traceback.format_exc(), None))


def test_scheduled_per_bucket_optimizer_is_the_host_set_rate_bitwise():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import numpy as np
    import torch.multiprocessing as mp
    from inferbiomechanics_amd.lr_schedule import LrSchedule
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_worker, args=(_free_port(), q))
    p.start()
    status, out = q.get(timeout=200)
    p.join(timeout=120)
    assert status == "ok", status
    ly, fy, iy = out["yardstick"]
    assert iy["ddp"] and iy["overlap"] and iy["buckets"] > 1 and iy["bucket_opt"] and not iy["recorded"], iy
    assert iy["first_step"] == [("plain", False)] * iy["buckets"] + [("plain", True)], iy["first_step"]
    floor = LrSchedule("cosine", W, T_TOTAL, M).lr_at(BASE, T_TOTAL)
    for arm in ("cut", "captured"):
        l, f, i = out[arm]
        assert i["ddp"] and i["overlap"] and i["bucket_opt"] and i["recorded"] and i["buckets"] == iy["buckets"], (arm, i)
        # every optimizer launch of a step carries the schedule: one per bucket and the last, self-counting one
        assert i["first_step"] == [("sched", False)] * i["buckets"] + [("sched", True)], (arm, i["first_step"])
        assert (i["graph_cuts"] >= i["buckets"]) if arm == "cut" else (i["graph_cuts"] == 0), (arm, i["graph_cuts"])
        assert i["next_lr"] == floor, (arm, i["next_lr"])
        assert l == ly, (arm, l, ly)
        for k in range(STEPS):
            assert np.array_equal(f[k].view(np.int32), fy[k].view(np.int32)), (arm, "parameters after step", k + 1)
    # the rate reached the update.  Adam moves a parameter by at most rate * sqrt(1 - 0.999^s) / sqrt(1 - 0.999) < 3.5 rate
    # at s = 12 (|m| <= (1 - 0.9^s) max|g|, v >= 0.001 * 0.999^(s-1) max|g|^2): step 12 ran at the floor, 0.1 lr, step 3 at lr
    move = lambda k: float(np.abs(fy[k] - fy[k - 1]).max())
    assert move(11) <= 4.0 * floor < move(2), (move(2), move(11), floor)
