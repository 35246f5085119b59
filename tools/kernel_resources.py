"""Register and scratch budget of every kernel in csrc/ sources: compiles each source with the Makefile's flags plus
-Rpass-analysis=kernel-resource-usage (device side only, no object kept) and prints, per kernel, VGPRs, AGPRs, SGPRs,
VGPR / SGPR spills, scratch bytes per lane, occupancy (waves per SIMD) and LDS bytes.  Runs without a GPU.
Usage: python tools/kernel_resources.py [--filter SUBSTR] [--json] [file.hip ...]     (default: ffn_chain.hip ffn_chain_bwd.hip)
       python tools/kernel_resources.py --digest [-D IB_AB] [file.hip ...]            (default: every source of the Makefile)
--digest prints, per source, the sha256 of its normalised device assembly (normalise_asm): a refactor that only moves
text leaves every line as it was; run it on both checkouts, once per build flavour, and diff the two outputs.  A source
given by absolute path is compiled where it lies, so one checkout's tool can digest another checkout's csrc/.
--digest --kernels prints one line per kernel instead (kernel_digests): its short name and the sha256 of its own text, so a
kernel that was renamed or moved to another place in its file, and is otherwise the same, keeps its line: neither its
ordinal in the file nor the compiler's trailing comments (which repeat the ordinal on loop labels) enter the hash."""
import argparse
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "inferbiomechanics_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function"]   # csrc/Makefile CXXFLAGS
KEYS = {"TotalSGPRs": "sgpr", "VGPRs": "vgpr", "AGPRs": "agpr", "ScratchSize [bytes/lane]": "scratch",
        "Occupancy [waves/SIMD]": "occupancy", "SGPRs Spill": "sgpr_spill", "VGPRs Spill": "vgpr_spill",
        "LDS Size [bytes/block]": "lds"}
_REMARK = re.compile(r"remark:\s+(Function Name|[A-Za-z][A-Za-z \[\]/]*?):\s+(\S+)\s+\[-Rpass-analysis")


def hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return None


def short_name(mangled):
    """_ZN12_GLOBAL__N_120ffn_chain_fwd_kernelILb1ELb1ELb1ELb0EEEvNS_12FfnFwdParamsE -> ffn_chain_fwd_kernel<1,1,1,0>
    _ZN12_GLOBAL__N_16smallm17fwd_smallm_kernelILi1ELi1EEEvPKDF16bl... -> smallm::fwd_smallm_kernel<1,1>
    (nested namespaces are walked and joined with "::", the anonymous one left out; template arguments that are float /
    bf16 element types, bools or ints; anything else keeps the mangled tail)"""
    m = re.match(r"_ZN(?:12_GLOBAL__N_1)?(?=\d)", mangled)
    if not m:
        return mangled
    parts, pos = [], m.end()
    while (d := re.match(r"\d+", mangled[pos:])):
        n = int(d.group())
        parts.append(mangled[pos + d.end():pos + d.end() + n])
        pos += d.end() + n
    name, rest = "::".join(parts), mangled[pos:]
    if rest.startswith("I"):
        # leading element types (f = float, DF16b = bf16), then bool / int literals
        types, body = [], rest[1:]
        while body.startswith(("f", "DF16b")):
            types.append("float" if body[0] == "f" else "bf16")
            body = body[1 if body[0] == "f" else 5:]
        args = re.findall(r"L[bij](-?\d+|n\d+)E", body[: body.find("EE") + 1] if "EE" in body else body)
        if types or args:
            return f"{name}<{','.join(types + [a.replace('n', '-') for a in args])}>"
    return name


def resources(src, extra=()):
    """[{kernel, mangled, vgpr, agpr, sgpr, vgpr_spill, sgpr_spill, scratch, occupancy, lds}] of one source"""
    cc = hipcc()
    if cc is None:
        raise RuntimeError("hipcc not found")
    path = src if os.path.isabs(src) else os.path.join(CSRC, src)
    with tempfile.TemporaryDirectory() as td:
        cmd = [cc, *FLAGS, *extra, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", path,
               "-o", os.path.join(td, "dev.o")]
        r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed:\n{r.stderr[-4000:]}")
    out, cur = [], None
    for line in r.stderr.splitlines():
        m = _REMARK.search(line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = {"source": os.path.basename(path), "kernel": short_name(val), "mangled": val}
            out.append(cur)
        elif cur is not None and key in KEYS:
            cur[KEYS[key]] = int(val) if val.lstrip("-").isdigit() else val
    return out


def normalise_asm(text):
    """device assembly without what differs between two compilations of the same code: comment lines, the compiler's
    .ident, the .file line, and every line that names the translation unit's __hip_cuid_<hash> symbol"""
    keep = []
    for line in text.splitlines():
        t = line.strip()
        if not t or t.startswith(";") or t.startswith((".ident", ".file")) or "__hip_cuid_" in t:
            continue
        keep.append(line.rstrip())
    return "\n".join(keep) + "\n"


def device_asm(src, extra=()):
    """normalised device assembly of one source, built with the Makefile's flags"""
    cc = hipcc()
    if cc is None:
        raise RuntimeError("hipcc not found")
    path = src if os.path.isabs(src) else os.path.join(CSRC, src)
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "dev.s")
        cmd = [cc, *FLAGS, *extra, "--cuda-device-only", "-S", path, "-o", out]
        r = subprocess.run(cmd, cwd=os.path.dirname(path), capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"{' '.join(cmd)} failed:\n{r.stderr[-4000:]}")
        with open(out) as f:
            return normalise_asm(f.read())


def kernel_digests(asm):
    """[(short name, sha256)] of the kernels of a normalised listing, in the listing's order.  A kernel's text is every line
    from the first to the last that names its symbol outside the metadata note -- its section, label and code, its
    .amdhsa_kernel descriptor and its resource .set lines -- with its own symbol replaced by "<kernel>", any other kernel's
    by that kernel's short name, the kernel's ordinal in the file taken out of its local labels (.LBB<n>_,
    .Lfunc_end<n>), the file-wide count of long branches out of their anchors (.Lpost_getpc<k>), and the comment the compiler puts behind a line's code cut off with the blanks before it (on a loop's
    label it names the ordinal again: "; in Loop: Header=BB<n>_80 Depth=1"; a line with a string in it is left whole):
    what remains is the instructions, the descriptor and the register counts"""
    lines = asm.split(".amdgpu_metadata")[0].splitlines()
    syms = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)
    names = re.compile("|".join(rf"(?<![\w$]){re.escape(s)}(?![\w$])" for s in sorted(syms, key=len, reverse=True)) or "$^")
    out = []
    for sym in syms:
        at = [i for i, l in enumerate(lines) if any(m.group() == sym for m in names.finditer(l))]
        text = "\n".join(l if '"' in l else re.sub(r"\s*;.*$", "", l) for l in lines[at[0]:at[-1] + 1]) + "\n"
        seen = {}      # .Lpost_getpc<k> (a long branch's anchor) counts through the whole file: renumbered per kernel, as #0, #1, ...
        text = re.sub(r"\.Lpost_getpc(\d+)", lambda m: f".Lpost_getpc#{seen.setdefault(m.group(1), len(seen))}", text)
        n = re.search(r"^\.Lfunc_end(\d+):", text, re.M)
        if n:
            text = re.sub(rf"(\.L[A-Za-z_]+){n.group(1)}(?!\d)", r"\1", text)
        text = names.sub(lambda m: "<kernel>" if m.group() == sym else short_name(m.group()), text)
        out.append((short_name(sym), hashlib.sha256(text.encode()).hexdigest()))
    return out


def makefile_sources():
    with open(os.path.join(CSRC, "Makefile")) as f:
        return re.search(r"^SRCS\s*=\s*(.+)$", f.read(), re.M).group(1).split()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sources", nargs="*")
    ap.add_argument("--filter", default="", help="only kernels whose short name contains this")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--digest", action="store_true", help="sha256 of each source's normalised device assembly")
    ap.add_argument("--kernels", action="store_true", help="with --digest: one line per kernel, under its short name")
    ap.add_argument("-D", action="append", default=[], help="extra -D definitions (e.g. -D IB_AB)")
    a = ap.parse_args()
    extra = [f"-D{d}" for d in a.D]
    if a.digest:
        srcs = a.sources or makefile_sources()
        with ThreadPoolExecutor(max_workers=min(8, len(srcs))) as ex:
            for s, asm in zip(srcs, ex.map(lambda s: device_asm(s, extra), srcs)):
                if a.kernels:
                    for k, d in kernel_digests(asm):
                        print(f"{os.path.basename(s):14s} {k:40s} {d}")
                else:
                    print(f"{os.path.basename(s):22s} {hashlib.sha256(asm.encode()).hexdigest()}")
        return 0
    a.sources = a.sources or ["ffn_chain.hip", "ffn_chain_bwd.hip"]
    with ThreadPoolExecutor(max_workers=min(4, len(a.sources))) as ex:
        rows = [k for ks in ex.map(lambda s: resources(s, extra), a.sources) for k in ks]
    rows = [k for k in rows if a.filter in k["kernel"]]
    if a.json:
        print(json.dumps(rows, indent=1))
        return 0
    cols = ("vgpr", "agpr", "sgpr", "vgpr_spill", "sgpr_spill", "scratch", "occupancy", "lds")
    print(f"{'source':18s} {'kernel':40s} " + " ".join(f"{c:>10s}" for c in cols))
    for k in rows:
        print(f"{k['source']:18s} {k['kernel']:40s} " + " ".join(f"{str(k.get(c, '?')):>10s}" for c in cols))
    return 0


if __name__ == "__main__":
    sys.exit(main())
