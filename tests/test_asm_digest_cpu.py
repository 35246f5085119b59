"""tools/kernel_resources.py --digest hashes each source's normalised device assembly, so that a refactor which only moves
text can show that it moved no instruction (same digests in both trees).  The normaliser is checked here on a canned
listing, no compiler: it drops what differs between two compilations of the same code and nothing else."""
import hashlib

from tools import kernel_resources as kr

LISTING = """\
\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"
\t.amdhsa_code_object_version 6
\t.text
\t.file\t"gemm_tn.hip"
\t.globl\t_ZN12_GLOBAL__N_114gemm_tn_kernelILb1EEEvNS_8TnParamsE ; -- Begin function
\t.p2align\t8
_ZN12_GLOBAL__N_114gemm_tn_kernelILb1EEEvNS_8TnParamsE:
; %bb.0:
\ts_load_dwordx2 s[2:3], s[0:1], 0x0
\t;;#ASMSTART
\tv_mbcnt_lo_u32_b32 v1, -1, 0
\t;;#ASMEND
\ts_waitcnt lgkmcnt(0)   \t
\ts_endpgm

\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel _ZN12_GLOBAL__N_114gemm_tn_kernelILb1EEEvNS_8TnParamsE
\t\t.amdhsa_next_free_vgpr 252
\t\t.amdhsa_accum_offset 252
\t.end_amdhsa_kernel
; NumVgprs: 252
\t.type\t__hip_cuid_94e6d6c2d3f0f1a2,@object
\t.globl\t__hip_cuid_94e6d6c2d3f0f1a2
__hip_cuid_94e6d6c2d3f0f1a2:
\t.byte\t0
\t.size\t__hip_cuid_94e6d6c2d3f0f1a2, 1
\t.ident\t"AMD clang version 20.0.0git"
"""


def test_normaliser_drops_comments_ident_file_and_cuid_only():
    out = kr.normalise_asm(LISTING).splitlines()
    assert not [l for l in out if l.lstrip().startswith((";", ".ident", ".file")) or "__hip_cuid_" in l or not l.strip()]
    # every instruction, label, directive and descriptor field stays, in order, without trailing blanks
    assert out == [
        '\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"',
        "\t.amdhsa_code_object_version 6",
        "\t.text",
        "\t.globl\t_ZN12_GLOBAL__N_114gemm_tn_kernelILb1EEEvNS_8TnParamsE ; -- Begin function",
        "\t.p2align\t8",
        "_ZN12_GLOBAL__N_114gemm_tn_kernelILb1EEEvNS_8TnParamsE:",
        "\ts_load_dwordx2 s[2:3], s[0:1], 0x0",
        "\tv_mbcnt_lo_u32_b32 v1, -1, 0",
        "\ts_waitcnt lgkmcnt(0)",
        "\ts_endpgm",
        '\t.section\t.rodata,"a",@progbits',
        "\t.amdhsa_kernel _ZN12_GLOBAL__N_114gemm_tn_kernelILb1EEEvNS_8TnParamsE",
        "\t\t.amdhsa_next_free_vgpr 252",
        "\t\t.amdhsa_accum_offset 252",
        "\t.end_amdhsa_kernel",
        "\t.byte\t0",
    ]


def test_digest_ignores_what_the_normaliser_drops_and_nothing_else():
    def digest(text):
        return hashlib.sha256(kr.normalise_asm(text).encode()).hexdigest()

    other_tu = LISTING.replace("94e6d6c2d3f0f1a2", "0123456789abcdef").replace('"gemm_tn.hip"', '"copy/gemm_tn.hip"') \
                      .replace("20.0.0git", "20.0.1") + "; a trailing remark\n"
    assert digest(other_tu) == digest(LISTING)
    assert digest(LISTING.replace("lgkmcnt(0)", "lgkmcnt(1)")) != digest(LISTING)                  # an instruction
    assert digest(LISTING.replace("next_free_vgpr 252", "next_free_vgpr 256")) != digest(LISTING)  # a descriptor field
    swapped = LISTING.replace("\ts_waitcnt lgkmcnt(0)   \t\n\ts_endpgm", "\ts_endpgm\n\ts_waitcnt lgkmcnt(0)")
    assert digest(swapped) != digest(LISTING)                                                      # instruction order


def test_digest_default_sources_are_the_makefile_list():
    srcs = kr.makefile_sources()
    assert len(srcs) == len(set(srcs)) >= 21 and all(s.endswith(".hip") for s in srcs)
    assert {"gemm.hip", "gemm_nt.hip", "gemm_tn.hip", "ffn_chain.hip", "diffusion.hip"} <= set(srcs)


# --digest --kernels: one digest per kernel.  KERNEL is one kernel as the compiler lays it out, {sym} its mangled name and
# {n} its ordinal in the file; NOTE is the metadata note at the end of a listing, which names every kernel again
KERNEL = """\
\t.section\t.text.{sym},"axG",@progbits,{sym},comdat
\t.globl\t{sym} ; -- Begin function {sym}
\t.p2align\t8
\t.type\t{sym},@function
{sym}: ; @{sym}
; %bb.0:
\ts_load_dwordx2 s[2:3], s[0:1], 0x0
\ts_cbranch_scc1 .LBB{n}_2
\ts_waitcnt lgkmcnt(0)
.LBB{n}_2:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel {sym}
\t\t.amdhsa_next_free_vgpr 52
\t\t.amdhsa_kernarg_size 192
\t.end_amdhsa_kernel
\t.section\t.text.{sym},"axG",@progbits,{sym},comdat
.Lfunc_end{n}:
\t.size\t{sym}, .Lfunc_end{n}-{sym}
\t.set {sym}.num_vgpr, 52
\t.set {sym}.private_seg_size, 0
\t.section\t.AMDGPU.csdata,"",@progbits
; Kernel info:
"""
NOTE = """\
\t.amdgpu_metadata
---
amdhsa.kernels:
  - .name:           {a}
    .symbol:         {a}.kd
  - .name:           {b}
    .symbol:         {b}.kd
...
\t.end_amdgpu_metadata
"""
STEP = "_ZN12_GLOBAL__N_118stitch_step_kernelIfLi8ELb1ELi{mode}ELb0EEEvNS_10StitchArgsE"
SDE = "_ZN12_GLOBAL__N_115sde_step_kernelIfLi8ELb1ELb0EEEvNS_7SdeArgsE"


def _kernels(first, second, edit=lambda text: text):
    text = KERNEL.format(sym=first, n=0) + edit(KERNEL.format(sym=second, n=1)) + NOTE.format(a=first, b=second)
    return kr.kernel_digests(kr.normalise_asm(text))


def test_kernel_digests_follow_the_kernel_not_its_name_or_place():
    base = _kernels(STEP.format(mode=1), STEP.format(mode=2))
    assert [k for k, _ in base] == ["stitch_step_kernel<float,8,1,1,0>", "stitch_step_kernel<float,8,1,2,0>"]
    assert base[0][1] == base[1][1] and len(base[0][1]) == 64          # the same text under two names and two ordinals
    # renamed (another template, another argument list in the mangled name) and moved to the other place in the file
    moved = _kernels(SDE, STEP.format(mode=1))
    assert [k for k, _ in moved] == ["sde_step_kernel<float,8,1,0>", "stitch_step_kernel<float,8,1,1,0>"]
    assert {d for _, d in moved} == {base[0][1]}
    # a symbol that another kernel's name begins with is not taken for that kernel
    assert {d for _, d in _kernels(STEP.format(mode=1), STEP.format(mode=1) + "x")} == {base[0][1]}


SMALLM = "_ZN12_GLOBAL__N_16smallm17fwd_smallm_kernelILi{act}ELi1EEEvPKDF16blS3_lPKfS3_lS3_liPDF16bliii"
SKINNY = "_ZN6skinny19dgrad_skinny_kernelILi0EEEvPKDF16blS2_lS2_lPDF16blPfiii"


def test_short_name_walks_nested_namespaces():
    assert kr.short_name(SMALLM.format(act=1)) == "smallm::fwd_smallm_kernel<1,1>"
    assert kr.short_name(SKINNY) == "skinny::dgrad_skinny_kernel<0>"
    assert kr.short_name("_ZN6wsmall19wgrad_smallm_kernelEPKDF16blS2_lPflS3_iiii") == "wsmall::wgrad_smallm_kernel"
    # two kernels of one nested namespace keep separate names, and the same text still hashes the same under both
    got = _kernels(SMALLM.format(act=1), SMALLM.format(act=2))
    assert [k for k, _ in got] == ["smallm::fwd_smallm_kernel<1,1>", "smallm::fwd_smallm_kernel<2,1>"]
    assert got[0][1] == got[1][1] == _kernels(STEP.format(mode=1), SKINNY)[1][1]


def test_kernel_digests_ignore_the_file_wide_count_of_long_branches():
    def long_branch(k):     # a branch relaxed out of range: its anchor label counts through the whole file, not the kernel
        return lambda t: t.replace("\ts_waitcnt lgkmcnt(0)\n", f"\ts_getpc_b64 s[4:5]\n.Lpost_getpc{k}:\n"
                                   f"\ts_add_u32 s4, s4, (.LBB1_2-.Lpost_getpc{k})&4294967295\n\ts_waitcnt lgkmcnt(0)\n")

    a = _kernels(STEP.format(mode=1), STEP.format(mode=2), long_branch(28))
    assert a[0][1] != a[1][1]                                          # the added instructions are seen
    assert _kernels(STEP.format(mode=1), STEP.format(mode=2), long_branch(175)) == a
    assert _kernels(STEP.format(mode=1), STEP.format(mode=2), long_branch(1)) == a      # a count equal to the kernel's ordinal
    other = _kernels(STEP.format(mode=1), STEP.format(mode=2), lambda t: long_branch(28)(t).replace("(.LBB1_2-", "(.LBB1_3-"))
    assert other[0] == a[0] and other[1][1] != a[1][1]                 # the branch's target still counts


def test_kernel_digests_see_instructions_descriptor_registers_and_order():
    base = _kernels(STEP.format(mode=1), STEP.format(mode=2))
    swap = ("\ts_load_dwordx2 s[2:3], s[0:1], 0x0\n\ts_cbranch_scc1 .LBB1_2\n",
            "\ts_cbranch_scc1 .LBB1_2\n\ts_load_dwordx2 s[2:3], s[0:1], 0x0\n")
    for old, new in (("lgkmcnt(0)", "lgkmcnt(1)"),                     # an instruction
                     ("kernarg_size 192", "kernarg_size 200"),         # a descriptor field
                     (".num_vgpr, 52", ".num_vgpr, 64"),               # a resource .set line
                     ("s_cbranch_scc1 .LBB1_2", "s_cbranch_scc1 .LBB1_3"),   # a branch target
                     swap):                                            # instruction order
        got = _kernels(STEP.format(mode=1), STEP.format(mode=2), lambda t: t.replace(old, new))
        assert old in KERNEL.format(sym="s", n=1) and got[0] == base[0] and got[1][0] == base[1][0], old
        assert got[1][1] != base[1][1], old
    # the file-level listing of the other tests: one kernel, no resource lines, no local labels
    (name, digest), = kr.kernel_digests(kr.normalise_asm(LISTING))
    assert name == "gemm_tn_kernel<1>"
    (_, other), = kr.kernel_digests(kr.normalise_asm(LISTING.replace("lgkmcnt(0)", "lgkmcnt(1)")))
    assert other != digest


# a loop header's label as the compiler writes it: the comment behind it names the kernel's ordinal again, without ".L"
def _loop_label(n, blanks):
    return lambda t: t.replace(f".LBB{n}_2:\n", f".LBB{n}_2:{blanks}; in Loop: Header=BB{n}_1 Depth=1\n")


def _loop_kernels(edit=lambda text: text):
    text = _loop_label(0, "   ")(KERNEL.format(sym=STEP.format(mode=1), n=0)) + \
        edit(_loop_label(1, "\t\t\t\t")(KERNEL.format(sym=STEP.format(mode=2), n=1))) + \
        NOTE.format(a=STEP.format(mode=1), b=STEP.format(mode=2))
    assert "Header=BB0_1 Depth=1" in text and "Header=BB1_1 Depth=1" in text
    return kr.kernel_digests(kr.normalise_asm(text))


def test_kernel_digests_ignore_trailing_comments_that_name_the_ordinal():
    base = _loop_kernels()
    assert base[0][1] == base[1][1]                  # ordinals 0 and 1, different blank widths before the comment
    assert base[0][1] == _kernels(STEP.format(mode=1), STEP.format(mode=2))[0][1]      # and the same as with no comment


def test_kernel_digests_still_see_the_code_in_front_of_a_trailing_comment():
    base = _loop_kernels()
    # the label itself, on the line that carries the loop comment
    relabelled = _loop_kernels(lambda t: t.replace(".LBB1_2:\t", ".LBB1_3:\t"))
    assert relabelled[0] == base[0] and relabelled[1][1] != base[1][1]
    # an instruction on a line that also carries a trailing comment: the comment alone changes nothing, the instruction does
    commented = _loop_kernels(lambda t: t.replace("s_waitcnt lgkmcnt(0)\n", "s_waitcnt lgkmcnt(0) ; 8-byte Folded Reload\n"))
    changed = _loop_kernels(lambda t: t.replace("s_waitcnt lgkmcnt(0)\n", "s_waitcnt lgkmcnt(1) ; 8-byte Folded Reload\n"))
    assert commented == base
    assert changed[0] == base[0] and changed[1][1] != base[1][1]
