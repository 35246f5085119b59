"""The refusals of the diffusion entry points (csrc/diffusion.hip), and which refusal wins where a call has two defects.
Every call here carries at least one defect, so nothing is ever launched and no GPU is needed; the pointers are addresses
inside a live ctypes buffer.  The expected codes are what the library returned before its launchers were folded onto one
width rule and one dtype dispatch (csrc/launch_geom.h, csrc/launch.h): each entry point keeps its own order."""
import ctypes

import pytest

OK, ARG, DTYPE, UNSUPPORTED = 0, -1, -2, -5
F32, BF16, BAD = 0, 1, 7

_buf = ctypes.create_string_buffer(1 << 16)
P = ctypes.cast(_buf, ctypes.c_void_p).value // 64 * 64 + 64          # aligned, non-null, alive for the whole module
HUGE_T, HUGE_LD = 1 << 20, 1 << 11                                    # T * ld = 2^31: offsets inside a window are 32-bit

# entry -> its parameters in header order with a valid value each (stream = None)
VALID = {
    "ib_gather_rows": dict(table=P, idx=P, out=P, B=2, dim=8, table_rows=10, dtype_out=F32, stream=None),
    "ib_q_sample": dict(x0=P, eps=P, t=P, sqrt_ab=P, sqrt_1mab=P, x_t=P, ld_xt=8, B=2, T=3, D=8, table_rows=10, dtype=F32,
                        stream=None),
    "ib_q_sample_cond": dict(x0=P, eps=P, t=P, sqrt_ab=P, sqrt_1mab=P, x_t=P, ld_xt=8, B=2, T=3, D=8, table_rows=10,
                             cond_cols=3, dtype=F32, stream=None),
    "ib_ddim_step": dict(x=P, eps=P, coef=P, timesteps=P, num_steps=4, step=0, step_dev=None, t_out=P, B=2, n=48,
                         dtype=F32, stream=None),
    "ib_ddim_cond_step": dict(x=P, eps=P, x0=P, z=P, mask=P, coef=P, obs_coef=P, timesteps=P, num_steps=4, step=0,
                              step_dev=None, t_out=P, B=2, T=3, D=8, ld=8, dtype=F32, stream=None),
    "ib_ddim_cond_init": dict(x=P, x0=P, z=P, mask=P, obs_coef=P, B=2, T=3, D=8, ld=8, dtype=F32, stream=None),
    "ib_ddim_step_noise": dict(x=P, eps=P, coef=P, timesteps=P, num_steps=4, step=0, step_dev=None, t_out=P, win_id=P,
                               seed=5, B=2, T=3, D=8, ld=8, dtype=F32, stream=None),
    "ib_ddim_cond_step_noise": dict(x=P, eps=P, x0=P, z=P, mask=P, coef=P, obs_coef=P, obs_noise_coef=P, timesteps=P,
                                    num_steps=4, step=0, step_dev=None, t_out=P, win_id=P, seed=5, B=2, T=3, D=8, ld=8,
                                    dtype=F32, stream=None),
    "ib_dpmpp_step": dict(x=P, eps=P, hist=P, coef=P, timesteps=P, num_steps=4, step=0, step_dev=None, t_out=P, B=2, n=48,
                          dtype=F32, stream=None),
    "ib_dpmpp_cond_step": dict(x=P, eps=P, hist=P, x0=P, z=P, mask=P, coef=P, obs_coef=P, timesteps=P, num_steps=4, step=0,
                               step_dev=None, t_out=P, B=2, T=3, D=8, ld=8, dtype=F32, stream=None),
    "ib_ensemble_stats": dict(x=P, mean=P, std_out=P, B=2, K=3, n=8, dtype=F32, stream=None),
}

_PTRS_Q = ("x0", "eps", "t", "sqrt_ab", "sqrt_1mab", "x_t")
_WINDOW = (dict(win_id=None), dict(B=0), dict(T=0), dict(D=0), dict(ld=7))
_TOO_LONG = dict(T=HUGE_T, ld=HUGE_LD, D=8)

# (entry, defects, expected code).  One defect: the code of that refusal.  Two: the one the entry point answers first.
CASES = []


def _add(entry, code, *defects):
    for d in defects:
        CASES.append((entry, d, code))


_add("ib_gather_rows", ARG, dict(table=None), dict(idx=None), dict(out=None), dict(B=0), dict(dim=0), dict(table_rows=0),
     dict(table=None, dtype_out=BAD), dict(B=-1, dtype_out=BAD))
_add("ib_gather_rows", DTYPE, dict(dtype_out=BAD), dict(dtype_out=2), dict(dtype_out=-1))

for e in ("ib_q_sample", "ib_q_sample_cond"):
    _add(e, ARG, *[{p: None} for p in _PTRS_Q], dict(B=0), dict(T=0), dict(D=0), dict(table_rows=0), dict(ld_xt=7),
         dict(x0=None, dtype=BAD), dict(ld_xt=7, dtype=BAD), dict(table_rows=0, dtype=BAD))
    _add(e, DTYPE, dict(dtype=BAD), dict(dtype=2), dict(dtype=-1), dict(dtype=BAD, ld_xt=9), dict(dtype=BAD, D=7, ld_xt=7))
# cond_cols out of range is refused before anything else; cond_cols == 0 is ib_q_sample, refusals included
_add("ib_q_sample_cond", ARG, dict(cond_cols=-1), dict(cond_cols=8), dict(cond_cols=9), dict(cond_cols=8, dtype=BAD),
     dict(cond_cols=-1, dtype=BAD), dict(cond_cols=-1, x0=None), dict(cond_cols=0, x0=None), dict(cond_cols=0, ld_xt=7),
     dict(cond_cols=0, x_t=None, dtype=BAD), dict(cond_cols=0, D=0))
_add("ib_q_sample_cond", DTYPE, dict(cond_cols=0, dtype=BAD), dict(cond_cols=7, dtype=BAD))

for e in ("ib_ddim_step", "ib_dpmpp_step"):
    hist = [dict(hist=None), dict(hist=None, dtype=BAD)] if e == "ib_dpmpp_step" else []
    _add(e, ARG, dict(x=None), dict(eps=None), dict(coef=None), dict(num_steps=0), dict(n=0), dict(timesteps=None),
         dict(B=0), dict(x=None, dtype=BAD), dict(n=0, dtype=BAD), dict(timesteps=None, dtype=BAD), dict(B=0, dtype=BAD),
         dict(num_steps=-1, dtype=BAD), *hist)
    # without t_out neither timesteps nor B is looked at: only the dtype is left to refuse
    _add(e, DTYPE, dict(dtype=BAD), dict(dtype=2), dict(dtype=BAD, n=47), dict(dtype=BAD, x=P + 4),
         dict(dtype=BAD, t_out=None, timesteps=None, B=0))

for e in ("ib_ddim_cond_step", "ib_dpmpp_cond_step"):
    hist = [dict(hist=None), dict(hist=None, dtype=BAD)] if e == "ib_dpmpp_cond_step" else []
    _add(e, ARG, dict(x=None), dict(eps=None), dict(x0=None), dict(z=None), dict(mask=None), dict(coef=None),
         dict(obs_coef=None), dict(num_steps=0), dict(B=0), dict(T=0), dict(D=0), dict(ld=7), dict(timesteps=None),
         dict(mask=None, dtype=BAD), dict(ld=7, dtype=BAD), dict(B=0, dtype=BAD), dict(timesteps=None, dtype=BAD), *hist)
    _add(e, DTYPE, dict(dtype=BAD), dict(dtype=2), dict(dtype=BAD, t_out=None, timesteps=None), dict(dtype=BAD, T=5, ld=9),
         dict(dtype=BAD, mask=P + 1))

_add("ib_ddim_cond_init", ARG, dict(x=None), dict(x0=None), dict(z=None), dict(mask=None), dict(obs_coef=None), dict(B=0),
     dict(T=0), dict(D=0), dict(ld=7), dict(z=None, dtype=BAD), dict(ld=7, dtype=BAD))
_add("ib_ddim_cond_init", DTYPE, dict(dtype=BAD), dict(dtype=2), dict(dtype=BAD, mask=P + 1), dict(dtype=BAD, T=5, ld=9))

# the stochastic updates: pointers and tables, then the dtype, then the window arguments, then the window's length
for e in ("ib_ddim_step_noise", "ib_ddim_cond_step_noise"):
    first = [dict(x=None), dict(eps=None), dict(coef=None), dict(num_steps=0), dict(timesteps=None)]
    if e == "ib_ddim_cond_step_noise":
        first += [dict(x0=None), dict(z=None), dict(mask=None), dict(obs_coef=None), dict(obs_noise_coef=None)]
    _add(e, ARG, *first, *[dict(d, dtype=BAD) for d in first], *[dict(d, **_TOO_LONG) for d in first], *_WINDOW,
         *[dict(d, **_TOO_LONG) for d in _WINDOW if "win_id" in d or "B" in d])
    _add(e, DTYPE, dict(dtype=BAD), dict(dtype=2), *[dict(d, dtype=BAD) for d in _WINDOW], dict(_TOO_LONG, dtype=BAD),
         dict(dtype=BAD, t_out=None, timesteps=None))
    _add(e, UNSUPPORTED, _TOO_LONG, dict(_TOO_LONG, dtype=BF16), dict(_TOO_LONG, t_out=None, timesteps=None),
         dict(T=1 << 31, ld=8, D=8))

_add("ib_ensemble_stats", ARG, dict(x=None), dict(mean=None), dict(std_out=None), dict(B=0), dict(K=0), dict(n=0),
     dict(x=None, dtype=BAD), dict(K=0, dtype=BAD))
_add("ib_ensemble_stats", DTYPE, dict(dtype=BAD), dict(dtype=2), dict(dtype=-1))


def _id(case):
    entry, defects, code = case
    return f"{entry[3:]}-{'+'.join(f'{k}={v}' if not isinstance(v, int) or abs(v) < 100 else k for k, v in defects.items())}->{code}"


def test_every_touched_entry_point_is_covered_and_two_defect_calls_pin_each_pair():
    assert {c[0] for c in CASES} == set(VALID)
    for entry in VALID:
        codes = {c[2] for c in CASES if c[0] == entry}
        assert {ARG, DTYPE} <= codes, entry
        assert any(len(c[1]) >= 2 and "dtype" in "".join(c[1]) for c in CASES if c[0] == entry), entry
    assert all(c[2] != OK and c[1] for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_refusal(case):
    from inferbiomechanics_amd import hip
    entry, defects, code = case
    args = dict(VALID[entry])
    assert set(defects) <= set(args), (entry, defects)
    args.update(defects)
    assert len(args) == len(hip._SIGS[entry][1])
    assert getattr(hip.lib(), entry)(*args.values()) == code
