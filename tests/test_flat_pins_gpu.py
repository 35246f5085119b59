"""The flat masked sampler updates hold their spelled rounding forms exactly (csrc/diffusion.hip: masked_update over
csrc/sampler_elem.h).  -m gpu.

ib_ddim_cond_init, ib_ddim_cond_step, ib_dpmpp_cond_step (a C == 0 row and a C != 0 row) and ib_ddim_cond_step_noise at a
sigma == 0 row, fp32 and bf16, column and checker masks, on windows of T = 8 frames, B = 2:
  (D, ld) = (12, 16)                    the 8-wide kernels
  (5, 5)                                8-wide too (T * ld = 40), keyed by flat offset: a vector straddles rows
  (5, 5), every buffer one element off  element-wise, lone-element forms (mix8 = 0)
  (5, 5), x0 and z one element off      element-wise, the free elements in the 8-wide form at e & 7 (mix8 = 1)
Every element of the state is compared with torch.equal against tests/exact_fp32.py, the forms restated in rational
arithmetic: an observed element is obs_pin8 at position e & 7 of its vector or obs_pin1 alone, a free one ddim_mix keyed the
same way (plus the one fused C h of a DPM row, and its history fmaf(hx, x, he eps)); INIT leaves free elements as they were.
Pad columns stay 0, the sentinels behind every buffer stay, and z is not written."""
import pytest
import torch

from tests.exact_fp32 import fused, mixed, pinned
from tests.test_stitch_kernels_gpu import checker_mask, col_mask, guarded, sentinels_ok

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
B, T, S = 2, 8, 6
GEOMS = [(12, 16, "aligned"), (5, 5, "aligned"), (5, 5, "all_off"), (5, 5, "x0z_off")]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from inferbiomechanics_amd import hip
    hip.lib()


@pytest.fixture(scope="module")
def tabs():
    from inferbiomechanics_amd.diffusion.schedule import DiffusionTables
    t = DiffusionTables(torch.device(DEV), num_sample_steps=10)
    t.set_sampler(S, 0.0, "dpmpp2m", "logsnr")
    c5 = t.dpmpp_coef.cpu()
    assert float(c5[0, 2]) == 0.0 and float(c5[2, 2]) != 0.0
    return t


def operands(D, ld, dt, how, seed):
    """x, eps, hist, x0, z [B, T, ld] with pad columns 0, each at the end of a flat buffer that ends in sentinels"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, dtype, scale in (("x", dt, 1.0), ("eps", dt, 1.0), ("hist", torch.float32, 3.0), ("x0", dt, 1.0), ("z", dt, 1.0)):
        shift = 1 if how == "all_off" or (how == "x0z_off" and name in ("x0", "z")) else 0
        v = torch.zeros(B, T, ld)
        v[:, :, :D] = scale * torch.randn(B, T, D, generator=g)
        out[name + "_flat"], out[name] = guarded((B, T, ld), dtype, shift)
        out[name].copy_(v.to(dtype).to(DEV))
    return out


def expected(op, mask, row, obs, vec, mix8, bf16, init=False):
    """(state, history) [B, T, ld] float32 of one update: row = (cx, ce, ch, hx, he), obs = (ox, oz); history None for DDIM"""
    x, eps, hist, x0, z = (op[k].float().cpu() for k in ("x", "eps", "hist", "x0", "z"))
    ld = x.shape[-1]
    cx, ce, ch, hx, he = row
    out, hout, mask = x.clone(), hist.clone(), mask.tolist()
    for b in range(B):
        for t in range(T):
            for c in range(ld):
                k, i = ((b * T + t) * ld + c) & 7, (b, t, c)
                if mask[t][c]:
                    out[i] = float(pinned(obs[0], x0[i], obs[1], z[i], k, vec))
                elif not init:
                    o = mixed(cx, x[i], ce, eps[i], k, vec or mix8, bf16)
                    out[i] = float(fused(ch, hist[i], o) if ch != 0.0 else o)
                    hout[i] = float(pinned(hx, x[i], he, eps[i], 0, True))       # fmaf(hx, x, he * eps), at either width
    return out, hout


@pytest.mark.parametrize("dt", [torch.float32, BF])
@pytest.mark.parametrize("D,ld,how", GEOMS)
def test_masked_updates_equal_their_spelled_forms(tabs, dt, D, ld, how):
    from inferbiomechanics_amd import hip
    op = operands(D, ld, dt, how, 300 + D + (dt == BF))
    vec, mix8, bf16 = how == "aligned", how != "all_off", dt == BF
    c2, c5, oc = tabs.ddim_coef.cpu(), tabs.dpmpp_coef.cpu(), tabs.obs_coef.cpu()
    zero3 = torch.cat([tabs.ddim_coef, torch.zeros(S, 1, device=DEV)], dim=1).contiguous()       # sigma == 0 in every row
    keep = torch.tensor([[1.0, 0.0]] * S, device=DEV)
    win = torch.arange(B, dtype=torch.int64, device=DEV)
    ddim_row = lambda s: (float(c2[s, 0]), float(c2[s, 1]), 0.0, 0.0, 0.0)
    dpm_row = lambda s: tuple(float(v) for v in c5[s])
    obs_row = lambda r: (float(oc[r, 0]), float(oc[r, 1]))
    for mask in (col_mask(D, ld), checker_mask(D, ld)):
        md, mb = mask.to(DEV), mask.bool()

        def run(entry, s):
            """one launch on fresh copies of x and hist (same alignment) -> (x, hist, their flat buffers)"""
            shift = op["x"].storage_offset()
            xf, x = guarded((B, T, ld), dt, shift)
            hf, h = guarded((B, T, ld), torch.float32, shift)
            x.copy_(op["x"])
            h.copy_(op["hist"])
            if entry == "init":
                hip.ddim_cond_init(x, op["x0"], op["z"], md, tabs.obs_coef, D=D)
            elif entry == "ddim":
                hip.ddim_cond_step(x, op["eps"], op["x0"], op["z"], md, tabs.ddim_coef, tabs.obs_coef, tabs.ddim_t, step=s, D=D)
            elif entry == "noise":
                hip.ddim_cond_step_noise(x, op["eps"], op["x0"], op["z"], md, zero3, tabs.obs_coef, keep, tabs.ddim_t, win, 7,
                                         step=s, D=D)
            else:
                hip.dpmpp_cond_step(x, op["eps"], h, op["x0"], op["z"], md, tabs.dpmpp_coef, tabs.obs_coef, tabs.ddim_t,
                                    step=s, D=D)
            torch.cuda.synchronize()
            return x, h, xf, hf

        z_before = op["z"].clone()
        for entry, s, row, obs in (("init", 0, ddim_row(0), obs_row(0)), ("ddim", 2, ddim_row(2), obs_row(3)),
                                   ("noise", 2, ddim_row(2), obs_row(3)), ("dpmpp", 0, dpm_row(0), obs_row(1)),
                                   ("dpmpp", 2, dpm_row(2), obs_row(3))):
            x, h, xf, hf = run(entry, s)
            want, want_h = expected(op, mb, row, obs, vec, mix8, bf16, init=entry == "init")
            got, want = x.cpu(), want.to(dt)
            print(f"{dt} D={D} ld={ld} {how} {entry} s={s}: {int((got[:, mb] != want[:, mb]).sum())} observed and "
                  f"{int((got[:, ~mb] != want[:, ~mb]).sum())} free elements differ from the spelled forms")
            assert torch.equal(got[:, mb], want[:, mb]), (entry, s, "observed elements are not the pinned form")
            assert torch.equal(got[:, ~mb], want[:, ~mb]), (entry, s, "free elements are not ddim_mix's form")
            assert not got[:, :, D:].any(), "pad columns must stay 0"
            if entry == "dpmpp":
                assert torch.equal(h.cpu()[:, ~mb], want_h[:, ~mb]), (entry, s, "history of the free elements")
                assert not h.cpu()[:, :, D:].any(), "pad columns of the history must stay 0"
            else:
                assert torch.equal(h, op["hist"]), "only the DPM update has a history"
            assert sentinels_ok(xf) and sentinels_ok(hf), "wrote past the state or the history"
        assert torch.equal(op["z"], z_before), "a deterministic row must not write z"
        assert all(sentinels_ok(op[k + "_flat"]) for k in ("x", "eps", "hist", "x0", "z"))
