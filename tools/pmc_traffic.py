"""HBM-side bytes per launch of the kernel families of ONE U-Net forward, from two rocprofv3 --pmc passes of
tools/fwd_only.py (FETCH_SIZE and WRITE_SIZE cannot share a pass: MI355X guide, counters table), corrected as the
guide's HBM section prescribes for gfx950 (FETCH_SIZE counts 64 B per 128-B request of a wide coalesced read: x2;
WRITE_SIZE is exact for 16-B-per-lane stores; both in KiB).  Writes profiles/<round>/pmc_traffic.json, which bench.py
quotes as roofline.traffic only while the library sources are the ones measured (lib_digest).
usage: python tools/pmc_traffic.py <out.json> <res>=<fetch_dir>,<write_dir> [...] [attention=<fetch_dir>,<write_dir>]"""
import collections
import csv
import glob
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from open_pandora_amd import build  # noqa: E402


def family(name):
    """kernel name -> family of bench.py's roofline.families (mangled or demangled spelling)"""
    m = re.search(r"gemm_(?:ringw?_)?kernelI\w+?Li(\d)E", name) or re.search(r"gemm_(?:ringw?_)?kernel<[^,]+, (\d)", name)
    if "ln_gemm_kernel" in name or "gemm_wide" in name:
        return "gemm"
    if m:
        return {"0": "gemm", "1": "conv3x3", "3": "conv3x3", "2": "conv_t3"}[m.group(1)]
    if "splitk_reduce" in name or "split16" in name:
        return "gemm_side"
    if "attn_self_kernel" in name or "attn_self16_kernel" in name or "attn_kernel" in name or "attn_fp8" in name:
        return "attention"
    if "pm" in name:
        return "other"
    return None


def counters(d, counter):
    per = collections.defaultdict(lambda: [0.0, 0])
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if r["Counter_Name"] != counter:
                continue
            fam = family(r["Kernel_Name"])
            if fam is None:
                continue
            per[fam][0] += float(r["Counter_Value"])
            per[fam][1] += 1
    return per


def main():
    out = {"lib_digest": build._digest(), "unit": "bytes per launch (FETCH_SIZE x 2 + WRITE_SIZE, KiB -> bytes)",
           "method": "rocprofv3 --kernel-trace --pmc FETCH_SIZE | WRITE_SIZE in separate passes over tools/fwd_only.py "
                     "(eager forwards, bf16); sums over every launch of the family, divided by the launches"}
    for arg in sys.argv[2:]:
        key, dirs = arg.split("=")
        fdir, wdir = dirs.split(",")
        fe, wr = counters(fdir, "FETCH_SIZE"), counters(wdir, "WRITE_SIZE")
        row = {}
        for fam in sorted(set(fe) | set(wr)):
            n = fe[fam][1] or wr[fam][1]
            fetch, write = 2.0 * fe[fam][0] * 1024, wr[fam][0] * 1024
            row[fam] = {"launches": n, "fetch_bytes_per_launch": fetch / max(n, 1), "write_bytes_per_launch": write / max(n, 1),
                        "bytes_per_launch": (fetch + write) / max(n, 1)}
        out[key] = row
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
