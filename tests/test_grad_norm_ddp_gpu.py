"""Clipping to a global gradient norm under data parallelism over REAL RCCL on a one-rank group (a fresh process: `nccl`
backend, IB_DDP_SELFTEST=1 makes the trainer issue its collectives although world == 1, as in tests/test_ddp_rccl_gpu.py): the
overlapped transformer step.  Without the clip its optimizer runs per bucket behind that bucket's all-reduce; with it there are
no per-bucket launches -- the coefficient needs every bucket -- and the step ends in one ib_grad_sumsq and one clipped launch
over the whole flat buffer behind the last all-reduce.  After each of 4 steps the parameters equal BITWISE those of the
single-process clipped trainer, in the cut-graph form (the collectives are host actions between graph segments) and in the
captured form (one graph per step; forced through IB_GRAPH_COLLECTIVES as that test does).  -m gpu."""
import os
import socket

import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS, BASE = 4, 1e-3


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
        _fh = open(os.path.join(tempfile.gettempdir(), f"grad_norm_ddp_hang_{os.getpid()}.txt"), "w")
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

        def run(ddp: bool, mgn: float, captured: bool = False, steps: int = STEPS):
            os.environ["IB_GRAPH_COLLECTIVES"] = "1" if captured else "0"
            os.environ["IB_DDP_SELFTEST"] = "1" if ddp else "0"
            print(f"[arm] ddp={ddp} max_grad_norm={mgn} captured={captured}", file=sys.stderr, flush=True)
            torch.manual_seed(7)
            model = DiffusionTransformer(D, T, d_model=512, num_heads=8, dim_feedforward=1024, num_layers=3,
                                         temporal_embedding_dim=6, temb_dim=32, temb_hidden=64, device="cuda", compute_dtype=dt)
            tr = HipTrainer(model, "diffusion", "adam", BASE, bucket_mb=0.5, overlap_comm=True if ddp else None,
                            max_grad_norm=mgn)
            order, real_opt, real_sq, real_launch = [], hip.optim_step, hip.grad_sumsq, tr.buckets.launch

            def opt(*a, **k):
                order.append(("optim", a[1].numel() == tr.flat.numel(), k.get("max_grad_norm", 0.0), k.get("ticket") is not None))
                return real_opt(*a, **k)

            def sq(*a, **k):
                order.append(("sumsq", a[0].numel() == tr.flat.numel()))
                return real_sq(*a, **k)

            def launch(b, *a, **k):
                order.append(("allreduce", b))
                return real_launch(b, *a, **k)
            hip.optim_step, hip.grad_sumsq, tr.buckets.launch = opt, sq, launch
            losses, flats, coefs, norms, first = [], [], [], [], None
            try:
                for b in batches[:steps]:
                    tr.step(b)
                    torch.cuda.synchronize()
                    if first is None:
                        first = list(order)
                    losses.append(tr.loss_value())
                    flats.append(tr.flat.detach().cpu().numpy().copy())
                    coefs.append(tr.clip_coef())
                    norms.append(tr.grad_norm())
            finally:
                hip.optim_step, hip.grad_sumsq = real_opt, real_sq
            info = {"ddp": tr.ddp, "overlap": tr.overlap_comm, "buckets": len(tr.buckets.ranges), "bucket_opt": tr.bucket_opt,
                    "recorded": tr._rec is not None, "first_step": first, "coefs": coefs, "norms": norms,
                    "graph_cuts": sum(1 for kk, _ in tr._rec.actions if kk == "host") if tr._rec is not None else -1}
            return losses, flats, info

        norm0 = run(False, float("inf"), steps=1)[2]["norms"][0]
        mgn = 0.5 * norm0
        out = {"mgn": mgn, "single": run(False, mgn), "cut": run(True, mgn), "captured": run(True, mgn, captured=True)}
        dist.barrier()
        dist.destroy_process_group()
        faulthandler.cancel_dump_traceback_later()
        _fh.close()
        os.unlink(_fh.name)                           # no hang: nothing to hand back
        q.put(("ok", out))
    except Exception:  # pragma: no cover
        import traceback
        q.put(("FAIL: " + traceback.format_exc(), None))


def test_one_clipped_launch_behind_the_last_all_reduce_equals_the_single_process_trainer_bitwise():
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
    mgn = float(np.float32(out["mgn"]))
    ls, fs, i_s = out["single"]
    assert not i_s["ddp"] and i_s["recorded"] and i_s["coefs"][0] < 1.0, i_s
    assert i_s["first_step"] == [("sumsq", True), ("optim", True, mgn, True)], i_s["first_step"]
    for arm in ("cut", "captured"):
        l, f, i = out[arm]
        assert i["ddp"] and i["overlap"] and i["recorded"] and i["buckets"] > 1, (arm, i)
        assert not i["bucket_opt"], "no per-bucket optimizer launches under the clip"
        # every bucket's all-reduce, then the norm of the whole reduced gradient, then the one clipped launch
        seq = i["first_step"]
        assert sorted(s[1] for s in seq[:-2]) == list(range(i["buckets"])) and all(s[0] == "allreduce" for s in seq[:-2]), (arm, seq)
        assert seq[-2:] == [("sumsq", True), ("optim", True, mgn, True)], (arm, seq)
        assert (i["graph_cuts"] >= i["buckets"]) if arm == "cut" else (i["graph_cuts"] == 0), (arm, i["graph_cuts"])
        assert l == ls and i["coefs"] == i_s["coefs"] and i["norms"] == i_s["norms"], (arm, l, ls, i["coefs"], i_s["coefs"])
        for k in range(STEPS):
            assert np.array_equal(f[k].view(np.int32), fs[k].view(np.int32)), (arm, "parameters after step", k + 1)
