"""The fused MLP-denoiser chain kernel (csrc/chain.hip) on the GPU, at every edge of tests/chain_cases.py.

Every case: the weights are packed into an image pre-filled with NaN (every element must have been overwritten, and the
image must equal the one built in Python), the kernel is launched through the C entry point on sentinel-filled buffers with
guard rows and guard columns, and check() holds every output elementwise to its stage-held float64 reference and the bound
counted from the code (tests/test_chain_bounds_cpu.py shows that the bound admits an fp32 emulation of the kernel and
rejects eighteen one-line mutants), asserts the exact values (the zero-variance rows, the zero pad columns, de_lp) and that
nothing outside the outputs was written.  For L <= 2 a second launch hands over NO u buffers: every other output must be
bitwise what the first launch produced.  The path the launcher recorded must be IB_PATH_CHAIN2.  The float64 references
are per-stage matrix products on the device.  The worst error / bound per stage is printed (pytest -rP)."""
import ctypes

import pytest
import torch

from tests.chain_cases import (BF, BY_NAME, CASES, GR, IB_E_ARG, IB_E_UNSUPPORTED, IB_OK, LN_EPS, PATH_CHAIN2, REFUSED, SENT,
                               TABLE_ROWS, alloc, case_id, check, expected_pack, geometry, layout, make_inputs, packed_elems)

pytestmark = pytest.mark.gpu

DEV = "cuda"
WORST = {}


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from inferbiomechanics_amd import hip as h
    h.lib()
    return h


def _ptrs(tensors):
    arr = (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def _dev(inp):
    return {k: ([a.to(DEV) for a in v] if isinstance(v, list) else v.to(DEV)) for k, v in inp.items()}


def _pack(hip, c, W):
    packed = torch.full((packed_elems(c.D, c.H, c.L),), float("nan"), dtype=BF, device=DEV)
    hip.mlp_chain_pack(W, packed, c.D, c.H)
    return packed


def _launch(hip, c, di, packed, outs, with_u=True, null_u=None, ld_part=None, de_lp="case", dims=None):
    """ib_mlp_chain_train on the buffers of alloc(): -> the return code.  di: the inputs on the device"""
    g = geometry(c)
    lay = layout(c)
    base = lambda name: outs[name][GR:, lay[name][1]:]
    keep = []
    slots = None
    x0, eps, t = di["x0"], di["eps"], di["t"]
    if c.slots:                                                      # the kernel must read the slots, not these
        slots = torch.zeros(4, dtype=torch.int64, device=DEV)
        hip.set_ptrs(slots, [di["x0"], di["eps"], di["t"]])
        x0, eps, t = di["x0_decoy"], di["eps_decoy"], di["t_decoy"]
    arrays = []
    for lst in (di["bias"], di["gamma"], di["beta"],
                [base(f"u{i}") if with_u and i != null_u else None for i in range(c.L)],
                [base(f"h{i}") for i in range(c.L)], [base(f"dz{i}") for i in range(c.L)]):
        k, p = _ptrs(lst)
        keep.append(k)
        arrays.append(p)
    pb, pg, pbe, pu, ph, pdz = arrays
    de = (base("de_lp") if c.de_lp else None) if isinstance(de_lp, str) else de_lp
    D, H, L = dims or (c.D, c.H, c.L)
    ptr = lambda a: None if a is None else a.data_ptr()
    return hip.lib().ib_mlp_chain_train(
        ptr(x0), ptr(eps), ptr(t), ptr(di["sab"]), ptr(di["s1m"]), TABLE_ROWS, ptr(di["e"]), di["e"].stride(0), ptr(packed), pb, pg,
        pbe, ptr(base("xt")), lay["xt"][3], pu, ph, pdz, ptr(base("dpred")), lay["dpred"][3], ptr(base("partial")),
        lay["partial"][3] if ld_part is None else ld_part, ptr(de), de.stride(0) if de is not None else 0, ptr(slots), g.M, c.T,
        D, H, L, LN_EPS, hip.stream_ptr())


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_chain_edges(hip, c):
    inp = make_inputs(c)
    di = _dev(inp)
    packed = _pack(hip, c, di["W"])
    outs = alloc(c, DEV)
    assert _launch(hip, c, di, packed, outs) == IB_OK
    assert hip.lib().ib_debug_last_path() == PATH_CHAIN2
    torch.cuda.synchronize()
    assert torch.equal(packed.cpu(), expected_pack(inp["W"], c.D, c.H, c.L))      # no NaN left, every block in its place
    worst = check(c, inp, outs)
    print(c.name, " ".join(f"{k}={v:.3g}" for k, v in worst.items()))
    for k, v in worst.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    assert all(v < 1 for v in worst.values()), worst
    if c.L <= 2:
        # no u buffers (the pre-activations stay in registers): bitwise the same outputs, and the u buffers untouched
        outs2 = alloc(c, DEV)
        assert _launch(hip, c, di, packed, outs2, with_u=False) == IB_OK
        assert hip.lib().ib_debug_last_path() == PATH_CHAIN2
        torch.cuda.synchronize()
        for name in outs:
            if name.startswith("u"):
                assert bool((outs2[name] == SENT).all()), name
            elif name == "partial":                                  # the three unwritten floats of a row hold the sentinel in both
                assert torch.equal(outs2[name], outs[name]), name
            else:
                assert torch.equal(outs2[name].view(torch.int16), outs[name].view(torch.int16)), name


def test_worst_ratio_per_stage():
    """the largest error / bound per stage over the cases that ran in this session"""
    print("worst error / bound per stage over all cases (GPU):")
    for k, v in WORST.items():
        print(f"  {k:10s} {v:.3g}")
    assert all(v < 1 for v in WORST.values())


@pytest.mark.parametrize("D,H,L,pitched", [(512, 512, 2, False), (300, 512, 3, True), (4, 128, 4, False), (300, 256, 1, False)])
def test_pack_layout_is_exact(hip, D, H, L, pitched):
    """ib_mlp_chain_pack: forward blocks, head, transposed blocks 1 .. L-1, head^T, fragment-major, zero beyond D in both roles
    (columns D .. DP-1 of a reduction, rows D .. DN-1 of an output); D = 512 fills DP and DN exactly, D = 300 and 4 do not"""
    g = torch.Generator().manual_seed(7 * D + H + L)
    dims = [D] + [H] * L
    shapes = [(dims[i + 1], dims[i]) for i in range(L)] + [(D, H)]
    W = []
    for n, k in shapes:                                              # values that are never 0: a zero in the image is padding
        w = (torch.rand(n, k, generator=g) + 0.5) * (torch.randint(0, 2, (n, k), generator=g) * 2 - 1)
        W.append(w.to(BF))
    if pitched:                                                      # rows of pitch K + 8, NaN in the pitch padding
        Wd = []
        for w in W:
            buf = torch.full((w.shape[0], w.shape[1] + 8), float("nan"), dtype=BF, device=DEV)
            buf[:, :w.shape[1]] = w.to(DEV)
            Wd.append(buf[:, :w.shape[1]])
    else:
        Wd = [w.to(DEV) for w in W]
    n = packed_elems(D, H, L)
    assert n == hip.mlp_chain_packed_elems(D, H, L)
    buf = torch.full((n + 1024,), float("nan"), dtype=BF, device=DEV)
    buf[n:] = SENT
    hip.mlp_chain_pack(Wd, buf[:n], D, H)
    torch.cuda.synchronize()
    want = expected_pack(W, D, H, L)
    assert int((want == 0).sum()) == n - sum(2 * a * b for a, b in shapes[1:]) - shapes[0][0] * shapes[0][1]
    assert torch.equal(buf[:n].cpu(), want)
    assert bool((buf[n:] == SENT).all())


def test_refusals(hip):
    """a refused call returns its code and writes nothing"""
    c = BY_NAME["h512_d64_m15"]                                      # L = 3, panel == window
    inp = make_inputs(c)
    di = _dev(inp)
    packed = _pack(hip, c, di["W"])
    outs = alloc(c, DEV)
    for D, H, L in REFUSED:
        assert _launch(hip, c, di, packed, outs, dims=(D, H, L)) == IB_E_UNSUPPORTED, (D, H, L)
        assert not hip.mlp_chain_supported(D, H, L)
    assert _launch(hip, c, di, packed, outs, null_u=1) == IB_E_ARG                  # KEEP off needs every u buffer
    assert _launch(hip, c, di, packed, outs, with_u=False) == IB_E_ARG
    w = geometry(c).width
    assert _launch(hip, c, di, packed, outs, ld_part=w - 1) == IB_E_ARG
    assert _launch(hip, c, di, packed, outs, ld_part=w - 4) == IB_E_ARG
    c2 = BY_NAME["h512_d68_m16"]                                     # P = 16, T = 2: de_lp is not defined
    di2 = _dev(make_inputs(c2))
    packed2 = _pack(hip, c2, di2["W"])
    outs2 = alloc(c2, DEV)
    de = torch.full((c2.B, c2.L * c2.H), SENT, dtype=BF, device=DEV)
    assert _launch(hip, c2, di2, packed2, outs2, de_lp=de) == IB_E_ARG
    torch.cuda.synchronize()
    for o in list(outs.values()) + list(outs2.values()) + [de]:
        assert bool((o == SENT).all())
    # the same buffers are accepted when nothing is wrong
    assert _launch(hip, c, di, packed, outs) == IB_OK and _launch(hip, c2, di2, packed2, outs2) == IB_OK
    torch.cuda.synchronize()
    check(c, inp, outs)
