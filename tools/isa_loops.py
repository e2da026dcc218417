"""VALU instructions per loop of a kernel's gfx950 ISA (profiles/leaf_loop/README.md).

  hipcc -O3 --offload-arch=gfx950 -std=c++17 -Iinclude --cuda-device-only -S -o kernels.s \
      turtle_kv_amd/csrc/tkv_amq_kernels.hip
  python tools/isa_loops.py kernels.s bloom_build_ldsILi0ELj256 [more mangled-name substrings]

Per kernel whose mangled name holds one of the substrings: every loop (a label and a later
branch back to it) that sets at least `--min-ds-or` LDS bits, with its instructions, its v_*
instructions, global loads, ds_or, exec saves and v_mov counted from the label to the back-edge.
A Bloom leaf loop is found by its ds_or count: keys per iteration x hash count."""
from __future__ import annotations

import argparse
import re


def kernels(path):
    out, name, body = {}, None, []
    for ln in open(path):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            name, body = m.group(1), []
            out[name] = body
        elif ln.startswith("\t.end_amdhsa_kernel") or ln.startswith(".Lfunc_end"):
            name = None
        elif name is not None:
            body.append(ln.rstrip("\n"))
    return out


def loops(body):
    labels = {}
    for i, ln in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            labels[m.group(1)] = i
    for i, ln in enumerate(body):
        m = re.match(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", ln)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            yield labels[m.group(1)], i, m.group(1)


def stats(body, a, b):
    ins = [ln.split(";")[0].strip() for ln in body[a:b + 1]]
    ins = [x for x in ins if x and not x.endswith(":") and not x.startswith(".")]
    n = lambda *p: sum(x.startswith(p) for x in ins)
    return dict(insns=len(ins), valu=n("v_"), loads=n("global_load", "buffer_load", "flat_load"),
                ds_or=n("ds_or"), saveexec=sum("saveexec" in x for x in ins), v_mov=n("v_mov"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("names", nargs="+")
    ap.add_argument("--min-ds-or", type=int, default=14)
    a = ap.parse_args()
    for name, body in kernels(a.asm).items():
        if not any(s in name for s in a.names):
            continue
        print(name)
        for lo, hi, label in loops(body):
            s = stats(body, lo, hi)
            if s["ds_or"] >= a.min_ds_or:
                print(f"  {label} lines {lo}-{hi}: {s}")


if __name__ == "__main__":
    main()
