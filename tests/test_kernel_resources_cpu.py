"""Register plan of the whole-layer kernels (csrc/ffn_chain.hip, csrc/ffn_chain_bwd.hip): every training instantiation
compiles for gfx950 with no VGPR spill, no scratch and two waves per SIMD.  A spill in these kernels lands in scratch
traffic inside the layer's phases; this catches a change that pushes the plan over the 256-register budget.
Compiles both translation units with hipcc (about 8 s each); skips where hipcc is not installed."""
import pytest

from tools import kernel_resources as kr

pytestmark = pytest.mark.skipif(kr.hipcc() is None, reason="hipcc not installed")

# <OUT, QKV, ATT, INFER> and <OUT, QKVH, ATT>: the forms the training step launches
TRAINING = {
    "ffn_chain.hip": ["ffn_chain_fwd_kernel<1,1,1,0>", "ffn_chain_fwd_kernel<1,1,0,0>", "ffn_chain_fwd_kernel<1,0,0,0>",
                      "ffn_chain_fwd_kernel<0,0,0,0>"],
    "ffn_chain_bwd.hip": ["ffn_chain_bwd_kernel<1,0,1>", "ffn_chain_bwd_kernel<1,1,0>", "ffn_chain_bwd_kernel<1,0,0>",
                          "ffn_chain_bwd_kernel<0,0,0>"],
}


@pytest.fixture(scope="module", params=sorted(TRAINING))
def source_resources(request):
    return request.param, {k["kernel"]: k for k in kr.resources(request.param)}


def test_short_names():
    assert kr.short_name("_ZN12_GLOBAL__N_120ffn_chain_fwd_kernelILb1ELb1ELb1ELb0EEEvNS_12FfnFwdParamsE") == \
        "ffn_chain_fwd_kernel<1,1,1,0>"
    assert kr.short_name("_ZN12_GLOBAL__N_120ffn_chain_bwd_kernelILb1ELb0ELb1EEEvNS_12FfnBwdParamsE") == \
        "ffn_chain_bwd_kernel<1,0,1>"


def test_training_forms_do_not_spill(source_resources):
    src, res = source_resources
    bad = []
    for name in TRAINING[src]:
        assert name in res, f"{src}: {name} not compiled (found {sorted(res)})"
        k = res[name]
        if k["vgpr_spill"] or k["scratch"] or k["vgpr"] > 256 or k["occupancy"] < 2:
            bad.append(f"{name}: {k['vgpr']} VGPRs, {k['vgpr_spill']} spilled, {k['scratch']} B/lane scratch, "
                       f"{k['occupancy']} waves/SIMD")
    assert not bad, "\n".join(bad)


def test_scratch_free_ffn_chain_forms(source_resources):
    # the INFER forms of the forward (DDIM sampler) as well: none of them may touch scratch
    src, res = source_resources
    forms = [k for k in res.values() if k["kernel"].startswith("ffn_chain_")]
    assert forms
    assert not [k["kernel"] for k in forms if k["scratch"] or k["vgpr_spill"]]
