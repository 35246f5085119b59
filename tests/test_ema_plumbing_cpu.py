"""Host-side plumbing of the EMA of the weights (`train --ema-decay`), on CPU tensors with the C-ABI in dry-run mode: the
two `_ema` entry points are exported and declared; over one step the EMA launches of a trainer cover the flat buffer
exactly once (source kind 3 excluded) on every step structure -- per-op MLP, chain-kernel MLP, the transformer's per-layer
launches and the data-parallel per-bucket launches; with the EMA off the launches are those of a trainer built without
it; the CLI flags, refusals and checkpoint keys; and the optimizer kernel's register budget."""
import argparse
import os
import socket

import pytest
import torch


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.fixture()
def dry():
    from inferbiomechanics_amd import hip
    hip.set_dry_run(True)
    yield hip
    hip.set_dry_run(False)


def ema_cover(tr, ranges):
    """how often one step's EMA launches touched each element of tr.ema (kind-3 ranges of a launch do not count)"""
    n = tr.ema.numel()
    cover = torch.zeros(n, dtype=torch.int32)
    for ptr, ln, skips in ranges:
        lo = (ptr - tr.ema.data_ptr()) // 4
        assert (ptr - tr.ema.data_ptr()) % 16 == 0 and 0 <= lo and lo + ln <= n
        c = torch.ones(ln, dtype=torch.int32)
        for s, l in skips:
            c[s:s + l] = 0
        cover[lo:lo + ln] += c
    return cover


def one_step(hip, tr, batch):
    lib = hip.lib()
    lib.calls.clear()
    lib.ema_ranges.clear()
    tr.step(batch)
    return list(lib.calls), list(lib.ema_ranges)


def diffusion_batch(B, T, D, dtype, seed=1):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, T, D, generator=g).to(dtype), torch.randint(0, 1000, (B,), generator=g),
            torch.randn(B, T, D, generator=g).to(dtype))


def test_ema_entries_are_exported_and_declared():
    from inferbiomechanics_amd import hip
    lib = hip.lib()
    for name in ("ib_optim_step_ema", "ib_optim_step_sources_ema"):
        assert name in hip.declared_symbols() and name in hip._SIGS and hasattr(lib, name)
    # the old entries keep their argument lists; the new ones add (ema, decay, warmup) in front of the stream
    assert hip._SIGS["ib_optim_step_ema"][1] == hip._SIGS["ib_optim_step"][1][:-1] + [hip._vp, hip._f32, hip._c.c_int, hip._vp]
    assert hip._SIGS["ib_optim_step_sources_ema"][1] == \
        hip._SIGS["ib_optim_step_sources"][1][:-1] + [hip._vp, hip._f32, hip._c.c_int, hip._vp]
    # argument errors are reported before anything is launched
    assert lib.ib_optim_step_ema(0, None, None, None, None, 0, 0.0, 1.0, 1, None, None, None, None, 0.5, 1, None) == -1


def _models():
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionMLP, DiffusionTransformer
    return [
        ("per-op MLP", lambda: DiffusionMLP(30, [32, 48], temb_dim=16, temb_hidden=24), (3, 7, 30, torch.float32)),
        ("chain MLP", lambda: DiffusionMLP(48, [128, 128], temb_dim=32, temb_hidden=128, compute_dtype=torch.bfloat16),
         (5, 16, 48, torch.bfloat16)),
        ("transformer", lambda: DiffusionTransformer(48, 32, d_model=512, num_heads=4, dim_feedforward=1024, num_layers=3,
                                                     compute_dtype=torch.bfloat16), (128, 32, 48, torch.bfloat16)),
    ]


@pytest.mark.parametrize("which", range(3), ids=["per-op MLP", "chain MLP", "transformer"])
def test_one_step_updates_every_ema_element_exactly_once(dry, which):
    from inferbiomechanics_amd.engine import HipTrainer
    name, make, (B, T, D, dt) = _models()[which]
    batch = diffusion_batch(B, T, D, dt)
    torch.manual_seed(0)
    plain = HipTrainer(make(), "diffusion", "adam", 1e-3, use_graph=False)
    names_plain, ranges = one_step(dry, plain, batch)
    assert ranges == [] and plain.ema is None
    torch.manual_seed(0)
    off = HipTrainer(make(), "diffusion", "adam", 1e-3, use_graph=False, ema_decay=0.0)
    assert one_step(dry, off, batch) == (names_plain, [])
    torch.manual_seed(0)
    tr = HipTrainer(make(), "diffusion", "adam", 1e-3, use_graph=False, ema_decay=0.999)
    assert tr.ema is not None and torch.equal(tr.ema, tr.flat) and tr.ema.data_ptr() != tr.flat.data_ptr()
    for _ in range(2):
        names, ranges = one_step(dry, tr, batch)
        assert [n.replace("_ema", "") for n in names] == names_plain      # the same launches, no new ones
        assert ranges and sum(n.endswith("_ema") for n in names) == len(ranges)
        assert torch.equal(ema_cover(tr, ranges), torch.ones(tr.ema.numel(), dtype=torch.int32)), name
    if which == 2:
        assert len(ranges) > 1                          # the per-layer launches from the backward carry the EMA too


def test_trainer_ema_state_dict_roundtrip(dry):
    from inferbiomechanics_amd.engine import HipTrainer
    from inferbiomechanics_amd.models.FeedForwardRegressionBaseline import FeedForwardBaseline
    m = FeedForwardBaseline(23, 2, 50, 'all_frames', 'sigmoid', 5, 10, hidden_dims=[16], batchnorm=True)
    args = argparse.Namespace(predict_grf_components=list(range(6)), predict_cop_components=list(range(6)),
                              predict_moment_components=list(range(6)), predict_wrench_components=list(range(12)))
    tr = HipTrainer(m, "regression", "sgd", 1e-2, args=args, use_graph=False, ema_decay=0.9)
    sd = tr.ema_state_dict()
    ref = m.state_dict()
    assert list(sd) == list(ref)                        # parameters AND buffers (BatchNorm running statistics)
    assert all(sd[k].shape == ref[k].shape and torch.equal(sd[k], ref[k].cpu()) for k in ref)
    sd2 = {k: v + 1.0 if k in tr.layout else v for k, v in sd.items()}
    tr.load_ema_state_dict(sd2)
    k0 = next(iter(tr.layout))
    assert torch.equal(tr.ema_state_dict()[k0], sd[k0] + 1.0)
    tr.reset_ema()
    assert torch.equal(tr.ema, tr.flat)
    with pytest.raises(Exception):
        tr.load_ema_state_dict({k0: sd[k0]})           # incomplete
    with pytest.raises(ValueError):
        HipTrainer(m, "regression", "sgd", 1e-2, args=args, use_graph=False, ema_decay=1.0)
    plain = HipTrainer(m, "regression", "sgd", 1e-2, args=args, use_graph=False)
    with pytest.raises(Exception, match="no EMA"):
        plain.ema_state_dict()


def _gloo_worker(rank, world, port, q):
    try:
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        import sys
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from inferbiomechanics_amd import hip
        from inferbiomechanics_amd.engine import HipTrainer
        from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionMLP, DiffusionTransformer
        hip.set_dry_run(True)
        lib = hip.lib()
        # (model, bucket MiB, overlapped buckets, optimizer per bucket): one all-reduce + one launch; buckets overlapped with
        # the backward + one launch; per-bucket launches on the side stream + the last launch over what is left
        cases = [(lambda: DiffusionMLP(12, [16, 24], temb_dim=8, temb_hidden=16), 0.001, False, False),
                 (lambda: DiffusionMLP(12, [16, 24], temb_dim=8, temb_hidden=16), 0.001, True, False),
                 (lambda: DiffusionTransformer(12, 5, d_model=16, num_heads=2, dim_feedforward=32, num_layers=3), 0.004, True,
                  True)]
        for make, mb, overlap, per_bucket in cases:
            torch.manual_seed(rank)                   # different init per rank: the EMA must start from the broadcast weights
            tr = HipTrainer(make(), "diffusion", "adam", 1e-3, bucket_mb=mb, overlap_comm=overlap, ema_decay=0.99)
            ref = tr.ema.clone()
            dist.broadcast(ref, src=0)
            assert torch.equal(ref, tr.ema) and torch.equal(tr.ema, tr.flat)
            for _ in range(2):
                lib.calls.clear()
                lib.ema_ranges.clear()
                tr.step((torch.randn(2, 5, 12), torch.tensor([1, 2]), torch.randn(2, 5, 12)))
                assert torch.equal(ema_cover(tr, list(lib.ema_ranges)), torch.ones(tr.ema.numel(), dtype=torch.int32)), \
                    (overlap, tr.bucket_opt, lib.ema_ranges)
            assert tr.bucket_opt == per_bucket
            if per_bucket:
                assert len(lib.ema_ranges) > 2              # the per-bucket launches carry the EMA
        hip.set_dry_run(False)
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, "FAIL: " + traceback.format_exc()))


def test_ddp_world2_gloo_ema_coverage():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert all(r[1] == "ok" for r in res), res


def _parse(argv):
    from inferbiomechanics_amd.cli.analyze import AnalyzeCommand
    from inferbiomechanics_amd.cli.train import TrainCommand
    from inferbiomechanics_amd.cli.visualize import VisualizeCommand
    parser = argparse.ArgumentParser()
    sub = parser.add_subparsers(dest="command")
    for c in (TrainCommand(), VisualizeCommand(), AnalyzeCommand()):
        c.register_subcommand(sub)
    return parser.parse_args(argv)


def test_cli_flags_parse_and_refusals(dry, tmp_path):
    from inferbiomechanics_amd.main import main
    a = _parse(['train', '--ema-decay', '0.9999', '--no-ema-warmup'])
    assert a.ema_decay == 0.9999 and a.no_ema_warmup
    a = _parse(['train'])
    assert a.ema_decay == 0.0 and not a.no_ema_warmup
    assert _parse(['analyze', '--use-ema']).use_ema and not _parse(['analyze']).use_ema
    assert _parse(['visualize', '--use-ema']).use_ema and not _parse(['visualize']).use_ema
    base = ['--no-wandb', '--synthetic-windows', '8', '--batch-size', '4', '--checkpoint-dir', str(tmp_path),
            '--data-loading-workers', '0', '--epochs', '1', '--max-steps', '1']
    for bad in (['--ema-decay', '-0.1'], ['--ema-decay', '1.0'], ['--ema-decay', '1.5'], ['--ema-decay', '0.99', '--eager']):
        with pytest.raises(SystemExit, match="ema-decay"):
            main(['train'] + base + bad)
    assert not os.path.exists(os.path.join(str(tmp_path), 'feedforward'))      # refused before anything was written


def test_checkpoint_keys_and_use_ema(dry, tmp_path):
    from inferbiomechanics_amd.cli.abstract_command import AbstractCommand
    from inferbiomechanics_amd.main import main
    from inferbiomechanics_amd.models.FeedForwardRegressionBaseline import FeedForwardBaseline
    base = ['--no-wandb', '--synthetic-windows', '16', '--batch-size', '8', '--data-loading-workers', '0',
            '--max-steps', '1', '--hidden-dims', '16']
    plain, ema = str(tmp_path / "plain"), str(tmp_path / "ema")
    assert main(['train', '--epochs', '1', '--checkpoint-dir', plain] + base)
    assert main(['train', '--epochs', '1', '--checkpoint-dir', ema, '--ema-decay', '0.999', '--no-ema-warmup'] + base)
    sp = torch.load(os.path.join(plain, 'feedforward', 'epoch_0_batch_0.pt'))
    se = torch.load(os.path.join(ema, 'feedforward', 'epoch_0_batch_0.pt'))
    assert set(sp) == {'epoch', 'model_state_dict', 'optimizer_state_dict'}
    assert set(se) == {'epoch', 'model_state_dict', 'optimizer_state_dict', 'ema_state_dict', 'ema'}
    assert se['ema'] == {'decay': 0.999, 'warmup': False}
    assert list(se['ema_state_dict']) == list(se['model_state_dict'])
    assert all(se['ema_state_dict'][k].shape == v.shape for k, v in se['model_state_dict'].items())
    assert set(se['optimizer_state_dict']) == set(sp['optimizer_state_dict'])
    # use_ema: the EMA weights go into the model; a checkpoint without them is an error, not a silent fall-back
    m = FeedForwardBaseline(23, 2, 50, 'all_frames', 'sigmoid', 5, 10, hidden_dims=[16])
    marked = {k: v + 7.0 for k, v in se['ema_state_dict'].items()}
    se['ema_state_dict'] = marked
    d = str(tmp_path / "marked")
    os.makedirs(d)
    torch.save(se, os.path.join(d, 'epoch_0_batch_0.pt'))
    AbstractCommand().load_latest_checkpoint(m, checkpoint_dir=d, use_ema=True)
    assert all(torch.equal(m.state_dict()[k].cpu(), v) for k, v in marked.items())
    AbstractCommand().load_latest_checkpoint(m, checkpoint_dir=d)
    assert all(torch.equal(m.state_dict()[k].cpu(), v) for k, v in se['model_state_dict'].items())
    with pytest.raises(ValueError, match="no EMA"):
        AbstractCommand().load_latest_checkpoint(m, checkpoint_dir=os.path.join(plain, 'feedforward'), use_ema=True)
    with pytest.raises(ValueError, match="no EMA"):
        main(['analyze', '--no-wandb', '--synthetic-windows', '3', '--checkpoint-dir', plain, '--data-loading-workers', '0',
              '--hidden-dims', '16', '--use-ema'])
    assert main(['analyze', '--no-wandb', '--synthetic-windows', '3', '--checkpoint-dir', ema, '--data-loading-workers', '0',
                 '--hidden-dims', '16', '--use-ema'])
    assert main(['visualize', '--synthetic-windows', '3', '--checkpoint-dir', ema, '--num-frames', '1', '--hidden-dims',
                 '16', '--use-ema'])
    # resuming an EMA run from a checkpoint without EMA starts the EMA from the loaded weights; the next file has it
    assert main(['train', '--epochs', '2', '--checkpoint-dir', plain, '--ema-decay', '0.99'] + base)
    s1 = torch.load(os.path.join(plain, 'feedforward', 'epoch_1_batch_0.pt'))
    assert 'ema_state_dict' in s1 and s1['ema'] == {'decay': 0.99, 'warmup': True}


def test_optim_kernel_forms_do_not_spill():
    """every optim_kernel<SRC, EMA> instantiation compiles without spills or scratch (compile only, about 3 s)"""
    from tools import kernel_resources as kr
    if kr.hipcc() is None:
        pytest.skip("hipcc not installed")
    res = {k["kernel"]: k for k in kr.resources("optim.hip")}
    forms = ["optim_kernel<0,0>", "optim_kernel<0,1>", "optim_kernel<1,0>", "optim_kernel<1,1>"]
    for f in forms:
        assert f in res, f"{f} not compiled (found {sorted(res)})"
        k = res[f]
        assert not k["vgpr_spill"] and not k["sgpr_spill"] and not k["scratch"], k
    # the EMA costs registers, not occupancy
    assert res["optim_kernel<0,1>"]["occupancy"] == res["optim_kernel<0,0>"]["occupancy"]
    assert res["optim_kernel<1,1>"]["occupancy"] == res["optim_kernel<1,0>"]["occupancy"]
