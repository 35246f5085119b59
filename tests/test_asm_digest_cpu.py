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
