#!/usr/bin/env python3
"""Compare the kernels' resources of two builds (DESIGN.md §3.12's table), no GPU needed.

Each input is the stderr of
    for f in rust-raytrace_amd/csrc/*.hip; do
    hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -Iinclude \\
          -Irust-raytrace_amd/csrc -c $f -o /dev/null -Rpass-analysis=kernel-resource-usage; done 2> LOG
on one checkout: the remark logs of all its translation units, one after the other (the parser
goes line by line; a checkout from before the split has trace_kernel.hip and path_kernel.hip).  Kernels are matched
by demangled name (c++filt); a trailing `false` template argument of wf_nearest / wf_fold / wf_tail / wf_shade /
trace_frame_kernel / wf_compose / wf_aa_compose / dn_pack / dn_pass in the second build (a parameter the first build
does not have; a kernel the first build has as a plain function loses its `<false>`) is dropped
before matching.  Prints every kernel of the first build whose
VGPRs, AGPRs, scratch, LDS or occupancy differ in the second (exit status 1 if any), then the
kernels only the second build has.

    python tools/kernel_resources.py parent.log head.log
"""
import re
import subprocess
import sys

KEYS = ["VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]"]


def parse(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: (.*?)(?: \[-Rpass-analysis=kernel-resource-usage\])?$", line.rstrip())
        if not m:
            continue
        text = m.group(1).strip()
        if text.startswith("Function Name:"):
            cur = text.split(":", 1)[1].strip()
            out[cur] = {}
        elif cur and ":" in text:
            k, v = text.split(":", 1)
            out[cur][k.strip()] = v.strip()
    names = list(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    res = {}
    for n, d in zip(names, dem):
        d = re.sub(r"rtamd::\(anonymous namespace\)::", "", d)
        res[re.sub(r"\(.*$", "", d).replace("void ", "")] = out[n]
    return res


def first_build_name(n):
    m = re.match(r"(wf_nearest|wf_fold|wf_tail|wf_shade|trace_frame_kernel|wf_compose|wf_aa_compose|dn_pack|dn_pass)<(.*)>$", n)
    if not m:
        return n
    args = [a.strip() for a in m.group(2).split(",")]
    if args[-1] != "false":
        return None
    return f"{m.group(1)}<{', '.join(args[:-1])}>" if len(args) > 1 else m.group(1)


def main():
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    seen, new, diffs = set(), [], 0
    for n, r in b.items():
        pn = n if n in a else first_build_name(n)
        if pn is None or pn not in a:
            new.append(n)
            continue
        seen.add(pn)
        for k in KEYS:
            if a[pn].get(k) != r.get(k):
                print(f"DIFF {pn}: {k} {a[pn].get(k)} -> {r.get(k)}")
                diffs += 1
    for n in a:
        if n not in seen:
            print(f"MISSING in the second build: {n}")
            diffs += 1
    print(f"{len(a)} kernels in the first build, {len(b)} in the second, {diffs} differences")
    for n in new:
        print("NEW", n, " ".join(f"{k.split()[0]}={b[n].get(k)}" for k in KEYS))
    return 1 if diffs else 0


if __name__ == "__main__":
    sys.exit(main())
