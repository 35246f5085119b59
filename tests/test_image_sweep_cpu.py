"""The image sweep of the whole-layer kernels (csrc/image_sweep.h, used by csrc/ffn_chain.hip and csrc/ffn_chain_bwd.hip): the
slice rule, exhaustively, through the probe entry of include/ib_hip_sweep.h -- the same function the kernels call.  Every
workgroup's slice of every part is 16-byte aligned and inside its part, slices of different workgroups are disjoint, their
union is a prefix of the parts laid end to end (all of them once the grid is at least 256), and no workgroup exceeds the cap.
This is the check against an out-of-range read of the sweep: no GPU test is arranged in which an overrun would fault."""
import ctypes
import os
import re
import subprocess

import pytest

W = 512 * 512 * 2                 # bytes of one packed [512 x 512] bf16 weight image
CAP = 3 * 512 * 16                # three 16-byte loads per thread of 512
GRIDS = (1, 2, 3, 31, 32, 33, 255, 256, 257, 800)
# (backward, out, qkv, att): the forms that exist -- forward <OUT, QKV, ATT>, backward <OUT, QKVH, ATT>
FORMS = [(0, 1, 1, 1), (0, 1, 1, 0), (0, 1, 0, 0), (0, 0, 0, 0), (1, 1, 0, 1), (1, 1, 1, 0), (1, 1, 0, 0), (1, 0, 0, 0)]


def expected_parts(backward, out, qkv, att, nc):
    """bytes of the parts in the order the form consumes them (0: it does not stream that part)"""
    if backward:      # wqkvtp (the QKV head comes first), w2tp, w1tp, wotp, wqkvtp_own
        return [3 * W * qkv, nc * W, nc * W, W * out, 3 * W * att]
    return [W * out, nc * W, nc * W, 3 * W * qkv, 0]        # wop, w1p, w2p, wqkvp


@pytest.mark.parametrize("form", FORMS, ids=lambda f: "%s<%d,%d,%d>" % ("bwd" if f[0] else "fwd", *f[1:]))
@pytest.mark.parametrize("nchunk", [1, 2, 3, 4])
def test_slices_are_aligned_inside_disjoint_and_a_prefix(form, nchunk):
    from inferbiomechanics_amd import hip
    parts = expected_parts(*form, nchunk)
    total = sum(parts)
    base = [sum(parts[:k]) for k in range(5)]
    assert total <= 256 * CAP, "a grid of 256 covers every image of these widths"
    for grid in GRIDS:
        spans = []                                  # (start, end) on the line of parts laid end to end
        for wg in range(grid):
            nbytes, rows = hip.image_sweep_slices(*form, 512, 512 * nchunk, grid, wg)
            assert [r[0] for r in rows] == parts, (form, nchunk)
            assert 0 <= nbytes <= CAP and nbytes == sum(r[2] for r in rows), (grid, wg, nbytes)
            for k, (pb, off, ln) in enumerate(rows):
                assert off % 16 == 0 and ln % 16 == 0 and 0 <= off and 0 <= ln and off + ln <= pb, (grid, wg, k, pb, off, ln)
                if ln:
                    spans.append((base[k] + off, base[k] + off + ln))
                else:
                    assert off == 0
        spans.sort()
        at = 0
        for a, b in spans:                          # sorted and each starting where the last ended: disjoint, a prefix
            assert a == at, (grid, a, at)
            at = b
        assert at <= total
        if grid >= 256:
            assert at == total, (grid, at, total)
        else:
            assert at == min(total, grid * min(CAP, -(-(-(-total // grid)) // 16) * 16)), (grid, at)


def test_the_headline_launch_sweeps_three_loads_per_thread():
    from inferbiomechanics_amd import hip
    for form in ((0, 1, 1, 1), (1, 1, 0, 1)):       # the three-layer forward form, the backward form: 12 images = 6 MB
        for wg in (0, 100, 255):
            assert hip.image_sweep_slices(*form, 512, 2048, 256, wg)[0] == CAP
    assert hip.image_sweep_slices(0, 1, 0, 0, 512, 2048, 256, 255)[0] == 9 * W // 256       # the top-layer form: 4.5 MB


def test_argument_errors():
    """IB_E_ARG = -1, IB_E_UNSUPPORTED = -3: a form that does not exist, a workgroup outside the grid, a null array, a width
    the kernels do not take"""
    from inferbiomechanics_amd import hip
    lib = hip.lib()
    a = [(ctypes.c_int64 * 5)() for _ in range(3)]
    ok = (0, 1, 1, 1, 512, 2048, 256, 0)
    assert lib.ib_image_sweep_slices(*ok, *a) == CAP
    for form in ((0, 0, 0, 1), (0, 0, 1, 0), (0, 1, 0, 1), (1, 0, 1, 0), (1, 0, 0, 1), (1, 1, 1, 1)):
        assert lib.ib_image_sweep_slices(*form, 512, 2048, 256, 0, *a) == -1, form
    for grid, wg in ((0, 0), (-1, 0), (4, 4), (4, -1)):
        assert lib.ib_image_sweep_slices(0, 1, 1, 1, 512, 2048, grid, wg, *a) == -1, (grid, wg)
    for k in range(3):
        b = list(a)
        b[k] = None
        assert lib.ib_image_sweep_slices(*ok, *b) == -1
    unsupported = lib.ib_image_sweep_slices(0, 1, 1, 1, 256, 2048, 256, 0, *a)
    assert unsupported < 0 and unsupported == lib.ib_image_sweep_slices(0, 1, 1, 1, 512, 2000, 256, 0, *a)
    with pytest.raises(hip.HipError):
        hip.image_sweep_slices(0, 0, 0, 1, 512, 2048, 256, 0)


def test_twelfth_header_has_its_own_table_and_is_built():
    from inferbiomechanics_amd import hip
    assert os.path.basename(hip.SWEEP_HEADER_PATH) == "ib_hip_sweep.h" and os.path.exists(hip.SWEEP_HEADER_PATH)
    assert hip.sweep_decls() == ["ib_image_sweep_slices"] == sorted(hip._SWEEP_SIGS)
    assert "ib_image_sweep_slices" not in hip._LOADED and len(hip._ENTRIES) == len(hip._LOADED) + 1
    assert not hip._is_launch("ib_image_sweep_slices"), "a host query: no proxy brackets, records or fakes it"
    c = ctypes
    assert hip._sig("ib_image_sweep_slices") == (c.c_int, [c.c_int] * 4 + [c.c_int64] * 2 + [c.c_int] * 2 + [c.c_void_p] * 3)
    mk = open(os.path.join(os.path.dirname(hip.__file__), "csrc", "Makefile")).read()
    sweep = re.search(r"^SWEEP_HDRS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert sweep == ["image_sweep.h", "../../include/ib_hip_sweep.h"]
    assert len(re.findall(r"^build(?:_ab)?/%\.o: %\.hip \$\(HDRS\) \$\(SWEEP_HDRS\)$", mk, flags=re.M)) == 2
    for path in (hip.LIB_PATH, hip.AB_LIB_PATH):
        if not os.path.exists(path):
            pytest.fail(f"{path} is not built")
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        assert "ib_image_sweep_slices" in {line.split()[-1] for line in out.splitlines() if line.strip()}, path
    root = os.path.dirname(os.path.dirname(hip.__file__))
    for doc in ("README.md", "INTEGRATION.md"):
        assert "ib_hip_sweep.h" in open(os.path.join(root, doc)).read(), doc
    assert "sweep_decls" in open(os.path.join(root, "__graft_entry__.py")).read(), "build() checks the twelfth header's exports"
