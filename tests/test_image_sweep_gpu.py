"""The image sweep of the whole-layer kernels only loads (csrc/ffn_chain.hip, csrc/ffn_chain_bwd.hip): every output buffer of the
forward and backward entries is bitwise what the kernels without the sweep write.  The reference is the same call made ONCE in a
fresh child process on the measurement build with IB_NO_IMAGE_SWEEP=1 (the switch is read once per process), at the smallest
shapes where the sweep can go wrong: one panel, short last rows, one chunk, the form without QKV parts, the forms with every
part, the plain forms, and a grid of 257 panels (one more than the chip has CUs).  That no slice leaves its part is checked
without a launch, exhaustively, in tests/test_image_sweep_cpu.py."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 512
# name: (B, T, ffn, mode) -- "att": one-window panels, forward <1,1,1> (every part) and backward <1,0,1> (every part);
# "top": one-window panels, forward <1,0,0> (the top layer: no QKV parts); "tokens": the token-count panels (16 rows here),
# forward <1,1,0> and <0,0,0>, backward <1,1,0> (the QKV head's part first), <1,0,0> and <0,0,0>
CASES = {
    "one_panel": (1, 50, 2048, "att"),
    "short_last_rows": (3, 7, 2048, "tokens"),
    "one_chunk": (2, 50, 512, "att"),
    "top_layer": (2, 50, 2048, "top"),
    "grid_257": (257, 16, 512, "att"),
}


def run_case(name):
    """every output buffer of the case's launches, on the CPU: {buffer name: tensor}"""
    from inferbiomechanics_amd import hip
    B, T, ffn, mode = CASES[name]
    M, dev, bf = B * T, "cuda", torch.bfloat16
    g = torch.Generator().manual_seed(11)
    q = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(dev, bf)
    v = lambda n: (0.1 * torch.randn(n, generator=g)).to(dev)
    x, attn, dy, dqn, ds1n = q(M, D), q(M, D), q(M, D), q(M, 3 * D, sc=0.25), q(M, D)
    w1, w2, wo, wq = q(ffn, D, sc=D ** -0.5), q(D, ffn, sc=ffn ** -0.5), q(D, D, sc=D ** -0.5), q(3 * D, D, sc=2 * D ** -0.5)
    b1, b2, bo, bq = v(ffn), v(D), v(D), v(3 * D)
    g1, be1, g2, be2 = 1 + v(D), v(D), 1 + v(D), v(D)
    packed = torch.zeros(hip.ffn_chain_packed_elems(D, ffn), dtype=bf, device=dev)
    hip.ffn_chain_pack([(w1, w2, packed, wo, wq)])
    out = {}

    def z(tag, *s, dtype=bf):
        out[tag] = torch.zeros(*s, dtype=dtype, device=dev)
        return out[tag]

    def forward(tag, Tp, with_out, with_qkv, with_att):
        f = lambda n, *s, **k: z(f"{tag}.{n}", *s, **k)
        mask = f("mask", hip.ffn_chain_mask_bytes(M, D, ffn, Tp), dtype=torch.uint8)
        f1, s2, y = f("f1", M, ffn), f("s2", M, D), f("y", M, D)
        mean, rstd = f("mean", M, dtype=torch.float32), f("rstd", M, dtype=torch.float32)
        ao = qn = an = None
        if with_out:
            ao = (attn, bo, g1, be1, f("s1", M, D), f("x1", M, D), f("mean1", M, dtype=torch.float32),
                  f("rstd1", M, dtype=torch.float32))
        if with_qkv:
            qn = (packed, bq, f("qkv", M, 3 * D))
        if with_att:
            an = (f("attn_next", M, D), f("lse", B, 8, T, dtype=torch.float32), T)
        hip.ffn_chain_fwd(x, packed, b1, b2, g2, be2, f1, s2, y, mean, rstd, mask, attn_out=ao, qkv_next=qn, attn_next=an,
                          panel_T=Tp)
        return f1, s2, mean, rstd, mask, ao, qn, an

    def backward(tag, Tp, fw, with_out, with_head, with_att):
        f = lambda n, *s, **k: z(f"{tag}.{n}", *s, **k)
        _, s2, mean, rstd, mask, ao, qn, an = fw
        nwg = hip.ffn_chain_workgroups(M, D, ffn, Tp)
        part = f("partial", (4 if with_out else 2) * nwg, D, dtype=torch.float32)
        ds2, dz1 = f("ds2", M, D), f("dz1", M, ffn)
        a_out = head = a_bwd = dx1 = None
        if with_out:
            a_out = (ao[4], ao[6], ao[7], g1, f("ds1", M, D), None if with_att else f("dattn", M, D))
        else:
            dx1 = f("dx1", M, D)
        if with_head:
            head = (packed, dqn, ds1n)
        if with_att:
            a_bwd = (qn[2], an[1], f("dqkv", M, 3 * D), f("dx", M, D), Tp)
        hip.ffn_chain_bwd(None if with_head else dy, s2, mean, rstd, g2, packed, mask, ds2, dz1, dx1, part, attn_out=a_out,
                          qkv_head=head, attn_bwd=a_bwd)

    if mode == "att":
        backward("bwd_att", T, forward("fwd_att", T, True, True, True), True, False, True)
    elif mode == "top":
        forward("fwd_top", T, True, False, False)
    else:
        fw = forward("fwd_tail", 0, True, True, False)
        backward("bwd_head", 0, fw, True, True, False)
        backward("bwd_out", 0, fw, True, False, False)
        backward("bwd_plain", 0, forward("fwd_plain", 0, False, False, False), False, False, False)
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in out.items()}


def child_main(path):
    torch.save({name: run_case(name) for name in CASES}, path)


@pytest.fixture(scope="module")
def without_sweep(tmp_path_factory):
    """every case's outputs from the kernels without the sweep: one child process for all cases"""
    from inferbiomechanics_amd import hip
    assert os.path.exists(hip.AB_LIB_PATH), f"{hip.AB_LIB_PATH} is not built"
    path = str(tmp_path_factory.mktemp("image_sweep") / "reference.pt")
    env = dict(os.environ, IB_HIP_LIB=hip.AB_LIB_PATH, IB_NO_IMAGE_SWEEP="1")
    code = "import sys; sys.path.insert(0, sys.argv[1]); from tests import test_image_sweep_gpu as m; m.child_main(sys.argv[2])"
    r = subprocess.run([sys.executable, "-c", code, ROOT, path], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return torch.load(path)


@pytest.mark.parametrize("name", sorted(CASES))
def test_outputs_are_bitwise_those_without_the_sweep(name, without_sweep):
    assert "IB_NO_IMAGE_SWEEP" not in os.environ, "this process runs the kernels that sweep"
    got, ref = run_case(name), without_sweep[name]
    assert sorted(got) == sorted(ref) and len(got) >= 10
    for k in sorted(got):
        a, b = got[k], ref[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"{name}: {k} differs"
        if a.is_floating_point():
            assert torch.isfinite(a.float()).all(), f"{name}: {k} is not finite"
    assert any(t.float().abs().sum() > 0 for t in got.values())
