"""Two builds of the library's device code compared kernel by kernel (profiles/*/kernels.tsv).

  python tools/isa_compare.py parent.s new.s OUTDIR

Both files from `hipcc -O3 --offload-arch=gfx950 -std=c++17 -Iinclude --cuda-device-only -S` of
one unit of turtle_kv_amd/csrc/ (tkv_amq_kernels.hip, tkv_amq_read.hip, ...), or of several units
with their .s files concatenated: kernels are matched by name, wherever they were compiled.
Per kernel: the instruction text with comments and directives stripped, local labels without
their function number (`.LBB12_3` as `.LBB_3`), and the `.amdhsa_*` resource lines.  Writes
OUTDIR/kernels.tsv (every kernel) and OUTDIR/differing.txt; needs c++filt for the names."""
from __future__ import annotations

import re
import subprocess
import sys


def parse(path):
    ks, name, body, hsa = {}, None, None, None
    for ln in open(path):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            name, body = m.group(1), []
            ks[name] = {"ins": body, "hsa": {}}
            continue
        m = re.match(r"^\s+\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            hsa = m.group(1)
            continue
        if ln.startswith("\t.end_amdhsa_kernel"):
            hsa = None
            continue
        if hsa is not None:
            m = re.match(r"^\s+\.amdhsa_(\S+)\s+(\S+)", ln)
            if m and hsa in ks:
                ks[hsa]["hsa"][m.group(1)] = m.group(2)
            continue
        if ln.startswith(".Lfunc_end"):
            name = None
            continue
        if name is None or ln.lstrip().startswith(";;#"):
            continue
        t = ln.split(";")[0].strip()
        if t and (not t.startswith(".") or re.match(r"^\.LBB\d+_\d+:", t)):
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    return {k: v for k, v in ks.items() if v["hsa"]}  # kernels only, not device functions


def figures(k):
    h = k["hsa"]
    return (sum(not i.endswith(":") for i in k["ins"]), h.get("next_free_vgpr"), h.get("next_free_sgpr"),
            h.get("group_segment_fixed_size"), h.get("private_segment_fixed_size"))


def main():
    p, n, out = parse(sys.argv[1]), parse(sys.argv[2]), sys.argv[3]
    names = sorted(set(p) | set(n))
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True,
                           check=True).stdout.split("\n")
    rows = []
    for k, d in zip(names, plain):
        if k not in p or k not in n:
            rows.append((d, *(["-"] * 10), "only in " + ("new" if k not in p else "parent")))
        else:
            same = p[k]["ins"] == n[k]["ins"] and p[k]["hsa"] == n[k]["hsa"]
            rows.append((d, *figures(p[k]), *figures(n[k]), "same" if same else "differs"))
    head = ("kernel", *(f"{c}_{s}" for s in ("parent", "new") for c in ("insns", "vgpr", "sgpr", "lds", "scratch")), "result")
    with open(out + "/kernels.tsv", "w") as fh:
        for r in [head] + rows:
            fh.write("\t".join(str(x) for x in r) + "\n")
    with open(out + "/differing.txt", "w") as fh:
        for r in rows:
            if r[-1] != "same":
                fh.write("\t".join(str(x) for x in r) + "\n")
    print(len(rows), "kernels,", sum(r[-1] != "same" for r in rows), "differ")


if __name__ == "__main__":
    main()
