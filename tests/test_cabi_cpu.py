"""CPU-side checks: the C-ABI library loads and exports every symbol include/ib_hip.h declares (no
compute calls without a GPU), host-side logic (flat layout, schedule tables bit-exact vs the oracle,
component weights), the drop-in surface (state_dict names, registry), and loud failure off-GPU."""
import argparse
import ctypes

import pytest
import torch

from oracle import ref_cpu as R


def test_library_loads_and_exports_every_declared_symbol():
    from inferbiomechanics_amd import hip
    lib = hip.lib()
    names = hip.declared_symbols()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), f"libib_hip.so does not export {n}"
        assert n in hip._SIGS, f"{n} has no ctypes signature"
    assert lib.ib_version() >= 100
    assert b"workspace" in lib.ib_error_string(-4)


# ---------------------------------------------------------------------------------------------------------------------
# the ctypes signatures are parsed from the header (hip._parse_header): the parser on texts written here
# ---------------------------------------------------------------------------------------------------------------------
HEADER_TEXT = """
#ifndef X_H
#define X_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef void* ib_stream_t; /* a stream */
enum { IB_A = 0, IB_B = 1 /* ib_not_a_call(int) */ };
int ib_scalars(int a, int32_t b, int64_t c, uint32_t d, uint64_t e, float f, size_t g, ib_stream_t s);
const char* ib_text(const int code);   // ib_in_a_comment(double x);
size_t ib_bytes(const int64_t n, const float* p, const void *q, int64_t unnamed_follows, int);
int64_t ib_arrays(void** out, const void* const* in, float* const* dst, const uint8_t* mask);
int ib_nothing(void);
int ib_split(const void* x,   /* the input,
                                 described over two lines; with a semicolon */
             int64_t n,
             ib_stream_t stream);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_maps_every_declaration_form():
    from inferbiomechanics_amd import hip
    c = ctypes
    vp = c.c_void_p
    assert hip._parse_header(HEADER_TEXT) == {
        "ib_scalars": (c.c_int, [c.c_int, c.c_int32, c.c_int64, c.c_uint32, c.c_uint64, c.c_float, c.c_size_t, vp]),
        "ib_text": (c.c_char_p, [c.c_int]),
        "ib_bytes": (c.c_size_t, [c.c_int64, vp, vp, c.c_int64, c.c_int]),
        "ib_arrays": (c.c_int64, [vp, vp, vp, vp]),
        "ib_nothing": (c.c_int, []),
        "ib_split": (c.c_int, [vp, c.c_int64, vp]),
    }
    assert hip._parse_header("") == {}


@pytest.mark.parametrize("text,words", [
    ("int ib_ok(int a);\nint ib_bad_type(int64_t n, double x, float y);", ("ib_bad_type", "double x")),
    ("int ib_unsigned(unsigned int n);", ("ib_unsigned", "unsigned int n")),
    ("int ib_array(int n[4]);", ("ib_array", "n[4]")),
    ("int ib_empty();", ("ib_empty",)),
    ("int ib_callback(int n, void (*done)(int), ib_stream_t s);", ("ib_callback", "done")),
    ("int ib_unclosed(int n;\nint ib_next(void);", ("ib_unclosed",)),
    ("double ib_ret(int n);", ("ib_ret", "double")),
    ("void* ib_ret_ptr(int n);", ("ib_ret_ptr",)),
    ("int ib_twice(int a);\nint ib_other(void);\nint ib_twice(int a);", ("ib_twice", "twice")),
])
def test_parser_refuses_what_it_cannot_map(text, words):
    from inferbiomechanics_amd import hip
    with pytest.raises(hip.HipError) as e:
        hip._parse_header(text)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_missing_header_is_a_hip_error_that_names_the_path(monkeypatch, tmp_path):
    from inferbiomechanics_amd import hip
    gone = str(tmp_path / "include" / "ib_hip.h")
    monkeypatch.setattr(hip, "HEADER_PATH", gone)
    with pytest.raises(hip.HipError) as e:
        hip._read_header()
    assert "missing" in str(e.value) and gone in str(e.value)


# the entry points that are not pure host queries and still do not take the stream last, as the header shows them: a new one
# has to be added here by name (time_recorded_call and the stamping proxy put the stream into the last argument)
NO_TRAILING_STREAM = {
    "ib_debug_set_ablate", "ib_debug_set_chain_prof", "ib_debug_set_ffn_prof", "ib_debug_set_gemm_prof", "ib_debug_set_nt_prof",
    "ib_event_create", "ib_event_destroy", "ib_event_elapsed_ms", "ib_graph_destroy", "ib_graph_end", "ib_stream_create",
    "ib_stream_destroy",
}


def test_real_header_gives_one_signature_per_declared_symbol():
    import re
    from inferbiomechanics_amd import hip
    c = ctypes
    assert len(hip._SIGS) == len(hip.declared_symbols()) == 127
    assert hip.declared_symbols() == sorted(hip._SIGS)
    src = re.sub(r"/\*.*?\*/", "", open(hip.HEADER_PATH).read(), flags=re.S)
    assert set(hip._SIGS) == set(re.findall(r"\b(ib_[a-z0-9_]+)\s*\(", src))        # the rule declared_symbols() had
    for name, (res, args) in hip._SIGS.items():
        assert res in (c.c_int, c.c_size_t, c.c_int64, c.c_char_p), name
        if name.endswith(hip._HOST_ONLY) or name in ("ib_version", "ib_error_string"):
            continue                                                              # pure host queries: no stream
        last = re.search(rf"\b{name}\s*\(([^)]*)\)", src).group(1).split(",")[-1].split()
        assert (last[0] != "ib_stream_t") == (name in NO_TRAILING_STREAM), (name, last)
        if name not in NO_TRAILING_STREAM:
            assert args[-1] is c.c_void_p, name
    # every out-parameter is a plain c_void_p like the other pointers (ctypes takes byref() there), not a POINTER(...) type
    assert hip._SIGS["ib_graph_end"][1] == [c.c_void_p, c.c_void_p]
    assert hip._SIGS["ib_stream_create"][1] == hip._SIGS["ib_event_create"][1] == [c.c_void_p]
    assert hip._SIGS["ib_event_elapsed_ms"][1] == [c.c_void_p] * 3
    lib = hip.lib()
    for name, (res, args) in hip._SIGS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    h, ms = c.c_void_p(), c.c_float()
    for fn, a in ((lib.ib_graph_end, (None, c.byref(h))), (lib.ib_event_elapsed_ms, (None, None, c.byref(ms)))):
        fn.argtypes[-1].from_param(a[-1])                                         # byref() marshals into a c_void_p parameter


# ---------------------------------------------------------------------------------------------------------------------
# which entry points the four proxies take over (hip._is_launch): the sets of the code before the predicate was shared
# ---------------------------------------------------------------------------------------------------------------------
HOST_QUERIES = {
    "ib_debug_last_path", "ib_error_string", "ib_ffn_chain_attn_mask_bytes", "ib_ffn_chain_attn_workgroups",
    "ib_ffn_chain_mask_bytes", "ib_ffn_chain_packed_elems", "ib_ffn_chain_supported", "ib_ffn_chain_workgroups",
    "ib_ffn_infer_workgroups", "ib_ffn_infer_workspace", "ib_layernorm_bwd_workspace", "ib_linear_ln_fwd_workspace",
    "ib_linear_ln_panel_workgroups", "ib_linear_panel_workgroups", "ib_linear_wgrad_slabs_workspace",
    "ib_linear_wgrad_workspace", "ib_mlp_chain_packed_elems", "ib_mlp_chain_partial_width", "ib_mlp_chain_supported",
    "ib_mlp_chain_workgroups", "ib_mse_loss_workspace", "ib_optim_ticket_words", "ib_regression_loss_workspace",
    "ib_time_mlp_bwd_slab_count", "ib_time_mlp_bwd_supported", "ib_time_mlp_fwd_supported", "ib_version",
}
EVENTS_AND_GRAPHS = {"ib_event_create", "ib_event_destroy", "ib_event_elapsed_ms", "ib_event_record", "ib_graph_begin",
                     "ib_graph_destroy", "ib_graph_end", "ib_graph_launch"}
DEBUG_HOOKS = {"ib_debug_set_ablate", "ib_debug_set_chain_prof", "ib_debug_set_ffn_prof", "ib_debug_set_gemm_prof",
               "ib_debug_set_nt_prof", "ib_debug_stamp"}
PASSED_THROUGH = {                       # proxy -> the names it hands to the library untouched; it wraps every other one
    "_DryRunLib": HOST_QUERIES,          # ... so no event, graph or stream call of a dry run reaches the real library
    "_TimingLib": HOST_QUERIES | EVENTS_AND_GRAPHS,
    "_RecordingLib": HOST_QUERIES | EVENTS_AND_GRAPHS,
    "_StampLib": HOST_QUERIES | EVENTS_AND_GRAPHS | DEBUG_HOOKS,
}


class _StubLib:
    """stands where the loaded library does: one distinct function per name, nothing behind it"""

    def __getattr__(self, name):
        fn = self.__dict__[name] = lambda *a: 0
        return fn


def _proxy_over_stub(cls, **attrs):
    proxy = object.__new__(cls)          # not __init__: _StampLib's allocates its stamp buffer on the device
    proxy._real = _StubLib()
    proxy.__dict__.update(attrs)
    return proxy


@pytest.mark.parametrize("cls", sorted(PASSED_THROUGH))
def test_each_proxy_takes_over_exactly_the_entry_points_it_did(cls):
    from inferbiomechanics_amd import hip
    proxy = _proxy_over_stub(getattr(hip, cls), only=None)
    passed = {n for n in hip._SIGS if getattr(proxy, n) is getattr(proxy._real, n)}
    assert passed == PASSED_THROUGH[cls]
    assert len(hip._SIGS) - len(passed) == {"_DryRunLib": 100, "_TimingLib": 92, "_RecordingLib": 92, "_StampLib": 86}[cls]
    if cls != "_DryRunLib":              # (the dry-run stand-in looks every name up in _SIGS)
        assert proxy.some_attribute is proxy._real.some_attribute


def test_stamp_proxy_honours_only():
    from inferbiomechanics_amd import hip
    proxy = _proxy_over_stub(hip._StampLib, only={"ib_cast", "ib_debug_stamp", "ib_event_record", "ib_version"})
    wrapped = {n for n in hip._SIGS if getattr(proxy, n) is not getattr(proxy._real, n)}
    assert wrapped == {"ib_cast"}


def test_predicate_is_the_one_rule_behind_the_proxies():
    from inferbiomechanics_amd import hip
    names = set(hip._SIGS)
    assert {n for n in names if not hip._is_launch(n)} == HOST_QUERIES | EVENTS_AND_GRAPHS
    assert {n for n in names if not hip._is_launch(n, handed_through=())} == HOST_QUERIES
    assert not hip._is_launch("calls") and not hip._is_launch("_real")
    assert hip._RecordingLib.SKIP == ("ib_optim_step", "ib_optim_step_ema", "ib_counter_add")


def test_launch_context_managers_install_their_proxy_and_restore_the_library():
    from inferbiomechanics_amd import hip
    hip.set_dry_run(True)
    try:
        base = hip.lib()
        with hip.record_launches() as rec:
            assert isinstance(rec, hip._RecordingLib) and hip.lib() is rec and rec._real is base
            assert (rec.calls, rec.paths, rec.notes) == ([], [], {})
            hip.cast(torch.zeros(4), torch.zeros(4, dtype=torch.bfloat16))
            assert [n for n, _ in rec.calls] == ["ib_cast"] and base.calls[-1] == "ib_cast"
        assert hip.lib() is base
        with hip.time_launches() as tl:
            assert isinstance(tl, hip._TimingLib) and hip.lib() is tl and tl.summary() == {}
        assert hip.lib() is base
        with pytest.raises(KeyError):
            with hip.record_launches():
                raise KeyError("left through an exception")
        assert hip.lib() is base
        assert callable(hip.time_recorded_call) and issubclass(hip.stamp_launches, hip._proxy_installed)
    finally:
        hip.set_dry_run(False)


def test_null_arguments_return_error_codes_not_crashes():
    from inferbiomechanics_amd import hip
    lib = hip.lib()
    assert lib.ib_linear_fwd(None, 0, None, 0, None, None, 0, None, 0, 0, 0, None, 0, None, 0, 4, 4, 4, 0, None) == -1
    assert lib.ib_optim_step(9, None, None, None, None, 0, 0.0, 1.0, 1, None, None, None, None) == -1
    assert lib.ib_linear_wgrad_workspace(12800, 512, 512) > 0
    assert lib.ib_linear_wgrad_workspace(4, 8, 8) == 0


def test_whole_layer_launches_validate_their_arguments():
    """round 5: the launches with the attention inside check shape, panel geometry and pointers on the host and return error
    codes -- a NULL `mask` would have been a device fault (the forward stores its ReLU bit words through it)"""
    from inferbiomechanics_amd import hip
    lib = hip.lib()
    assert lib.ib_ffn_chain_attn_workgroups(12800, 512, 2048, 50) == 256
    assert lib.ib_ffn_chain_attn_workgroups(4096, 512, 1024, 64) == 64
    for M, d, ffn, T in ((12800, 512, 2048, 8), (12800, 512, 2048, 65), (12800, 512, 2048, 48), (12800, 256, 2048, 50),
                         (12800, 512, 2000, 50), (12800, 512, 2048, 0)):
        assert lib.ib_ffn_chain_attn_workgroups(M, d, ffn, T) == 0, (M, d, ffn, T)
    assert lib.ib_ffn_chain_attn_mask_bytes(12800, 512, 2048, 50) == 256 * 4 * 512 * 8
    buf = ctypes.create_string_buffer(4096)
    a = ctypes.cast(buf, ctypes.c_void_p).value // 16 * 16 + 16          # any aligned non-NULL address: nothing is launched
    P = lambda ok=True: ctypes.c_void_p(a) if ok else None
    fwd = lambda **k: lib.ib_ffn_chain_fwd_attn(*[P(k.get(f"a{i}", True)) for i in range(25)], k.get("T", 50), k.get("M", 12800),
                                                k.get("d", 512), k.get("ffn", 2048), 1e-5, None)
    assert fwd(T=0) == -1                                         # IB_E_ARG: no panel geometry
    assert fwd(T=48) == -5 and fwd(d=256) == -5                   # IB_E_UNSUPPORTED: M % T != 0 / d != 512
    assert fwd(a11=False) == -1                                   # mask
    assert fwd(a24=False) == -1                                   # attention tail without lse
    assert fwd(a22=False) == -1                                   # attention tail without the QKV tail
    assert lib.ib_ffn_chain_fwd(*[P(i != 11) for i in range(23)], 12800, 512, 2048, 1e-5, None) == -1       # mask NULL
    bwd = lambda **k: lib.ib_ffn_chain_bwd_attn(*[P(k.get(f"a{i}", True)) for i in range(19)], k.get("T", 50), k.get("M", 12800),
                                                512, 2048, None)
    assert bwd(T=0) == -1 and bwd(T=48) == -5
    for i in (0, 6, 10, 15, 16, 17, 18):                          # dy, mask, s1, qkv, lse, dqkv, dx
        assert bwd(**{f"a{i}": False}) == -1, i
    inf = lambda **k: lib.ib_ffn_chain_fwd_infer(*[P(k.get(f"a{i}", True)) for i in range(14)], k.get("M", 51200), k.get("d", 512),
                                                 2048, 1e-5, None)
    assert inf(d=256) == -5 and inf(a6=False) == -1 and inf(a7=False) == -1 and inf(a13=True, a11=False) == -1


def test_schedule_tables_bit_exact_vs_oracle():
    from inferbiomechanics_amd.diffusion import schedule as S
    ab = S.alphas_cumprod(1000)
    assert torch.equal(ab, R.alphas_cumprod(R.linear_beta_schedule(1000)))
    assert abs(ab[499].item() - 0.078587242881778235) < 1e-15
    assert torch.equal(S.ddim_timesteps(1000, 100), R.ddim_timesteps(1000, 100))
    assert torch.equal(S.ddim_coefficients(1000, 100), R.ddim_coeffs(1000, 100))
    t = torch.arange(1000)
    assert torch.equal(S.timestep_embedding_table(1000, 128), R.timestep_embedding(t, 128))
    tabs = S.DiffusionTables(torch.device("cpu"))
    assert tabs.sqrt_ab.dtype == torch.float32 and tabs.ddim_t.dtype == torch.int64
    assert torch.equal(tabs.sqrt_ab, R.schedule_tables()["sqrt_ab"].to(torch.float32))


def test_flat_layout_alignment():
    from collections import OrderedDict
    from inferbiomechanics_amd.module import flat_layout
    lay, total = flat_layout(OrderedDict(a=(3, 5), b=(7,), c=(64, 2)))
    assert lay["a"] == (0, 15) and lay["b"] == (64, 7) and lay["c"] == (128, 128) and total == 256


def test_component_weights():
    from inferbiomechanics_amd.loss.RegressionLossEvaluator import component_weights
    a = argparse.Namespace(predict_grf_components=[1], predict_cop_components=[], predict_moment_components=[],
                           predict_wrench_components=[])
    w = component_weights(a)
    assert sum(w) == 1.0 and w[1] == 1.0
    a = argparse.Namespace(predict_grf_components=list(range(6)), predict_cop_components=list(range(6)),
                           predict_moment_components=list(range(6)), predict_wrench_components=list(range(12)))
    assert component_weights(a) == [1.0] * 30


def test_drop_in_surface_names_match_reference():
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionMLP, DiffusionTransformer
    from inferbiomechanics_amd.models.FeedForwardRegressionBaseline import FeedForwardBaseline
    from inferbiomechanics_amd.models.TransformerBaseline import TransformerLayer
    m = FeedForwardBaseline(23, 2, 50, 'all_frames', 'sigmoid', 5, 10)
    assert list(m.state_dict().keys()) == ['net.0.weight', 'net.0.bias', 'net.2.weight', 'net.2.bias',
                                           'net.4.weight', 'net.4.bias']
    assert m.input_size == 1470 and m.output_size == 300          # FeedForwardRegressionBaseline.py:52,63
    assert sum(p.numel() for p in m.parameters()) == 1169708
    assert list(TransformerLayer(512, 8, 2048).state_dict().keys()) == R.TL_KEYS
    d = DiffusionMLP()
    assert {k: tuple(v.shape) for k, v in d.state_dict().items()} == R.denoiser_mlp_param_shapes(300, [512, 512])
    d2 = DiffusionTransformer()
    assert {k: tuple(v.shape) for k, v in d2.state_dict().items()} == R.denoiser_transformer_param_shapes(300, 50)


def test_no_cpu_fallback():
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.loss.RegressionLossEvaluator import RegressionLossEvaluator
    from inferbiomechanics_amd.models.FeedForwardRegressionBaseline import FeedForwardBaseline
    from oracle.fixture_inputs import ff_inputs
    m = FeedForwardBaseline(23, 2, 50, 'all_frames', 'sigmoid', 5, 10)
    with pytest.raises(hip.HipError):
        m(ff_inputs(2, 10, 23, 5))
    with pytest.raises(hip.HipError):
        hip.linear_fwd(torch.zeros(2, 2), torch.zeros(2, 2), None, torch.zeros(2, 2))
    ev = RegressionLossEvaluator(None, 'train', device='cpu')
    with pytest.raises(hip.HipError):
        ev({}, {}, {}, [], [], argparse.Namespace())


def test_shipping_library_reads_no_environment_and_has_no_profiling_hooks():
    """no global mutable state in the C-ABI.  The A/B switches (IB_NO_NT, IB_TN_TARGET, ...) and the in-kernel
    stamp hooks are compiled only into the measurement build (lib/ab/libib_hip_ab.so, -DIB_AB); the shipping library imports
    no getenv at all, answers IB_E_UNSUPPORTED to every ib_debug_set_* call, and both builds export the same symbols"""
    import os
    import subprocess
    from inferbiomechanics_amd import hip
    assert os.path.basename(hip.LIB_PATH) == "libib_hip.so" and not hip.measurement_build()
    und = subprocess.run(["nm", "-D", "--undefined-only", hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in und
    lib = hip.lib()
    for setter in ("ib_debug_set_chain_prof", "ib_debug_set_gemm_prof", "ib_debug_set_nt_prof"):
        assert getattr(lib, setter)(None) == -5, setter
    assert lib.ib_debug_set_ablate(1) == -5
    assert os.path.exists(hip.AB_LIB_PATH), "the measurement build was not built (make -C inferbiomechanics_amd/csrc)"
    ab = ctypes.CDLL(hip.AB_LIB_PATH)
    for n in hip.declared_symbols():
        assert hasattr(ab, n), f"libib_hip_ab.so does not export {n}"
    assert "getenv" in subprocess.run(["nm", "-D", "--undefined-only", hip.AB_LIB_PATH], capture_output=True, text=True,
                                      check=True).stdout
