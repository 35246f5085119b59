"""In-kernel phase profile of the whole-layer launches HOT and COLD (measurement build; thread 0 of every workgroup stamps the
100 MHz wall clock at phase boundaries, as tools/layer_prof.py):
  hot   back-to-back launches of one layer, the packed image resident in the caches (what layer_prof.py measures);
  cold  ONE chosen launch inside the captured graph of a real training step of the headline workload: the stamp buffer is
        handed to the library only while that launch is captured, so every replay of the step stamps that launch alone.  Between
        two uses of a layer's image the step moves gigabytes through HBM: the launch meets its weights cold.
The three forms: the three-layer forward (layer 1's), the top-layer forward, the backward (the top layer's, which runs with
nothing beside it, and layer 1's, which runs beside the weight-gradient launches).
Run once as is and once with IB_NO_IMAGE_SWEEP=1 (the switch is read once per process) for the two arms; both arms are stamped.
Usage: python tools/sweep_prof.py [hot|cold|both]"""
import ctypes
import os
import sys

import torch

sys.path.insert(0, ".")
import tools._ab  # noqa: E402,F401
import bench  # noqa: E402
from inferbiomechanics_amd import hip  # noqa: E402
from inferbiomechanics_amd.engine import HipTrainer  # noqa: E402

NC = 4
FWD = ["x, attn rows -> LDS; out-proj GEMM; LayerNorm1"]
for _c in range(NC):
    FWD += [f"c{_c}.gemm1", f"c{_c}.sync(skew)", f"c{_c}.relu+mask+sync", f"c{_c}.gemm2(+f1 rows)"]
FWD += ["s2 exchange, LayerNorm2 rows"]
TAIL = ["Q gemm", "Q epilogue", "K gemm (+Q rows out)", "K epilogue + S^T + softmax", "V gemm (+K rows out)", "V epilogue",
        "P.V, attn + V rows out"]
BWD = ["LayerNorm2 backward (+dgamma/dbeta)", "feed-forward dgrads (8 GEMM phases)", "dx1 -> image D, LayerNorm1 backward",
       "out-projection dgrad GEMM", "barrier", "dO -> SB, q/k/v loads, K -> SA", "attention phase 1 (dQ)",
       "attention phase 2 (dK, dV)", "barrier", "in-projection dgrad (3 GEMM phases) + ds1", "dx rows out"]
ARM = "no sweep" if os.environ.get("IB_NO_IMAGE_SWEEP") else "sweep"


def row_of(stamps, n):
    s = stamps.cpu().double()
    dd = (s[:, 1:n + 1] - s[:, :n]) * 0.01
    return torch.cat([dd.mean(0), ((s[:, n] - s[:, 0]) * 0.01).mean().view(1), ((s[:, n].max() - s[:, 0].min()) * 0.01).view(1)])


def show(title, names, acc):
    print(f"---- {title} [{ARM}]")
    for nm, val in zip(names, acc[:len(names)].tolist()):
        print(f"{nm:52s} {val:7.2f} us")
    print(f"{'per-WG mean':52s} {acc[-2]:7.2f} us")
    print(f"{'first start -> last end':52s} {acc[-1]:7.2f} us", flush=True)


def hot(B=256, T=50):
    M, d, ffn, dev, bf = B * T, 512, 512 * NC, "cuda", torch.bfloat16
    g = torch.Generator().manual_seed(0)
    q = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(dev, bf)
    v = lambda n: (0.1 * torch.randn(n, generator=g)).to(dev)
    x, attn, dy = q(M, d), q(M, d), q(M, d)
    w1, w2, wo, wq = q(ffn, d, sc=d ** -0.5), q(d, ffn, sc=ffn ** -0.5), q(d, d, sc=d ** -0.5), q(3 * d, d, sc=2 * d ** -0.5)
    b1, b2, bo, bq = v(ffn), v(d), v(d), v(3 * d)
    g1, be1, g2, be2 = 1 + v(d), v(d), 1 + v(d), v(d)
    packed = torch.zeros(hip.ffn_chain_packed_elems(d, ffn), dtype=bf, device=dev)
    hip.ffn_chain_pack([(w1, w2, packed, wo, wq)])
    e = lambda *s: torch.empty(*s, dtype=bf, device=dev)
    f1, s2, y, s1, x1o, qkv, ao = e(M, ffn), e(M, d), e(M, d), e(M, d), e(M, d), e(M, 3 * d), e(M, d)
    lse = torch.empty(B, 8, T, device=dev)
    mean, rstd, mean1, rstd1 = (torch.empty(M, device=dev) for _ in range(4))
    mask = torch.zeros(hip.ffn_chain_mask_bytes(M, d, ffn, T), dtype=torch.uint8, device=dev)
    nwg = hip.ffn_chain_workgroups(M, d, ffn, T)
    ds2, dz1, ds1, dqkv, dx = e(M, d), e(M, ffn), e(M, d), e(M, 3 * d), e(M, d)
    part = torch.empty(4 * nwg, d, device=dev)
    a_out = (attn, bo, g1, be1, s1, x1o, mean1, rstd1)
    fwd = lambda: hip.ffn_chain_fwd(x, packed, b1, b2, g2, be2, f1, s2, y, mean, rstd, mask, attn_out=a_out,
                                    qkv_next=(packed, bq, qkv), attn_next=(ao, lse, T), panel_T=T)
    top = lambda: hip.ffn_chain_fwd(x, packed, b1, b2, g2, be2, f1, s2, y, mean, rstd, mask, attn_out=a_out, panel_T=T)
    bwd = lambda: hip.ffn_chain_bwd(dy, s2, mean, rstd, g2, packed, mask, ds2, dz1, None, part,
                                    attn_out=(s1, mean1, rstd1, g1, ds1, None), attn_bwd=(qkv, lse, dqkv, dx, T))
    for name, launch, names in (("three-layer forward", fwd, FWD + TAIL), ("top-layer forward", top, FWD), ("backward", bwd, BWD)):
        stamps = torch.zeros(nwg, 64, dtype=torch.int64, device=dev)
        for _ in range(20):
            fwd(); bwd()
        torch.cuda.synchronize()
        hip.lib().ib_debug_set_ffn_prof(ctypes.c_void_p(stamps.data_ptr()))
        acc = None
        for _ in range(8):
            for _ in range(30):
                launch()
            torch.cuda.synchronize()
            row = row_of(stamps, len(names))
            acc = row if acc is None else acc + row
        hip.lib().ib_debug_set_ffn_prof(None)
        show(f"HOT {name} (B = {B}, T = {T}, {nwg} workgroups; back-to-back launches, wave 0's timeline)", names, acc / 8)


def cold(kind, index, title, names, reps=32, skip=2):
    wl_kind, T, D, B = bench.WORKLOADS["transformer_denoiser_T50"]
    dev = torch.device("cuda", 0)
    model = bench.build_model(wl_kind, T, D, torch.bfloat16, dev)
    batches = bench.make_batches(8, B, T, D, torch.bfloat16, dev, seed=0)
    nwg = hip.ffn_chain_workgroups(B * T, 512, 512 * NC, T)
    stamps = torch.zeros(nwg, 64, dtype=torch.int64, device=dev)
    calls, armed, orig = {"fwd": 0, "bwd": 0}, [False], {"fwd": hip.ffn_chain_fwd, "bwd": hip.ffn_chain_bwd}

    def wrap(k):
        def f(*a, **kw):
            i, calls[k] = calls[k], calls[k] + 1
            on = armed[0] and k == kind and i == index
            if on:
                hip.lib().ib_debug_set_ffn_prof(ctypes.c_void_p(stamps.data_ptr()))
            try:
                return orig[k](*a, **kw)
            finally:
                if on:
                    hip.lib().ib_debug_set_ffn_prof(None)
        return f

    hip.ffn_chain_fwd, hip.ffn_chain_bwd = wrap("fwd"), wrap("bwd")
    try:
        tr = HipTrainer(model, "diffusion", "rmsprop", 1e-4, use_graph=True)
        for i in range(2):
            tr.step(batches[i])                    # eager warm-ups
        armed[0] = True
        calls.update(fwd=0, bwd=0)
        tr.step(batches[2])                        # capture (+ first replay): the chosen launch takes the stamp buffer
        armed[0] = False
        assert calls[kind] > index, f"the step made {calls[kind]} {kind} launches"
        acc, n = None, 0
        for i in range(reps):
            stamps.zero_()
            torch.cuda.synchronize()
            tr.step(batches[i % 8])                # a replay of the captured step
            torch.cuda.synchronize()
            assert int(stamps[0, len(names)]) != 0, "the chosen launch did not stamp: is the step a graph replay?"
            if i >= skip:
                row = row_of(stamps, len(names))
                acc, n = (row if acc is None else acc + row), n + 1
        show(f"COLD {title} (inside the captured step of transformer_denoiser_T50, B = {B}, {nwg} workgroups; {n} replays)",
             names, acc / n)
    finally:
        hip.ffn_chain_fwd, hip.ffn_chain_bwd = orig["fwd"], orig["bwd"]


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "both"
    if not hip.measurement_build():
        raise SystemExit("the phase stamps need the measurement build of the library")
    if what in ("hot", "both"):
        hot()
    if what in ("cold", "both"):
        cold("fwd", 1, "three-layer forward, layer 1", FWD + TAIL)
        cold("fwd", 3, "top-layer forward, layer 3", FWD)
        cold("bwd", 0, "backward, layer 3 (runs first, nothing beside it)", BWD)
        cold("bwd", 2, "backward, layer 1 (beside the weight-gradient launches)", BWD)


if __name__ == "__main__":
    main()
