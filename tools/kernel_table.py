"""Per-kernel resource table of one HIP translation unit, as the build compiles it (no GPU needed).

Compiles csrc/<unit> with build.py's flags (plus any extra flags), takes the gfx950 code object out of the object file and
prints one row per kernel: registers, scratch, spills, occupancy, LDS (hipcc's kernel-resource-usage remarks), code bytes
and a digest of the disassembly with addresses and encodings stripped.  Two trees compile the same device code exactly
when their tables are equal, digests included; a register regression shows as a changed column.

usage: python tools/kernel_table.py gemm.hip [-DPM_DIAG=1 ...] [--asm DIR]   (--asm: also write DIR/<symbol>.s)"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from open_pandora_amd import build as _b  # noqa: E402

LLVM = "/opt/rocm/lib/llvm/bin"
FIELDS = (("TotalSGPRs", "sgpr"), ("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "occ"), ("SGPRs Spill", "sspill"), ("VGPRs Spill", "vspill"), ("LDS Size [bytes/block]", "lds"))


def resources(stderr):
    """{mangled name: {column: value}} from the -Rpass-analysis=kernel-resource-usage remarks"""
    out, cur = {}, None
    for line in stderr.splitlines():
        m = re.search(r"remark:\s+(.*?):\s+(\S+)\s+\[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = out.setdefault(m.group(2), {})
        elif cur is not None:
            for key, col in FIELDS:
                if m.group(1) == key:
                    cur[col] = m.group(2)
    return out


def disassembly(code_object):
    """{symbol: [instruction lines]} of .text, comments (address + encoding) stripped"""
    txt = subprocess.run([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", code_object],
                         check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in txt.splitlines():
        m = re.match(r"^<(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(line.split("//")[0].strip())
    return out


def sizes(code_object):
    txt = subprocess.run([LLVM + "/llvm-objdump", "-t", code_object], check=True, capture_output=True, text=True).stdout
    out = {}
    for line in txt.splitlines():
        p = line.split()
        if len(p) >= 5 and "F" in p[1:3] and ".text" in p:
            out[p[-1]] = int(p[p.index(".text") + 1], 16)
    return out


def main():
    args = sys.argv[1:]
    asm_dir = None
    if "--asm" in args:
        i = args.index("--asm")
        asm_dir = args[i + 1]
        del args[i:i + 2]
    unit, extra = args[0], args[1:]
    src = unit if os.path.exists(unit) else os.path.join(_b.CSRC, unit)
    flags = _b.CFLAGS + _b.PER_FILE_FLAGS.get(os.path.basename(src), []) + extra
    with tempfile.TemporaryDirectory() as tmp:
        obj, fat, co = (os.path.join(tmp, n) for n in ("u.o", "u.fatbin", "u.co"))
        r = subprocess.run([_b._hipcc()] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", obj],
                           capture_output=True, text=True)
        if r.returncode:
            sys.exit(r.stderr)
        subprocess.run([LLVM + "/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
        subprocess.run([LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fat,
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True)
        res, dis, size = resources(r.stderr), disassembly(co), sizes(co)
    print(f"# {os.path.basename(src)}  flags: {' '.join(flags)}")
    print(f"# {'vgpr':>4} {'agpr':>4} {'sgpr':>4} {'scratch':>7} {'vspill':>6} {'sspill':>6} {'occ':>3} {'lds':>6} {'bytes':>7} {'insns':>6}  digest        kernel")
    rows = []
    for sym, lines in dis.items():
        r = res.get(sym, {})
        if asm_dir:
            os.makedirs(asm_dir, exist_ok=True)
            with open(os.path.join(asm_dir, sym[:200] + ".s"), "w") as f:
                f.write("\n".join(lines) + "\n")
        dig = hashlib.sha256("\n".join(lines).encode()).hexdigest()[:12]
        g = lambda c: r.get(c, "-")
        rows.append((sym, f"  {g('vgpr'):>4} {g('agpr'):>4} {g('sgpr'):>4} {g('scratch'):>7} {g('vspill'):>6} {g('sspill'):>6} {g('occ'):>3} "
                                  f"{g('lds'):>6} {size.get(sym, 0):>7} {len(lines):>6}  {dig}  {sym}"))
    for _, row in sorted(rows):
        print(row)


if __name__ == "__main__":
    main()
