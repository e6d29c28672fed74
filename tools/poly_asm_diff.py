#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of csrc/twostage.hip instruction by instruction.

    hipcc ... -save-temps=obj -Rpass-analysis=kernel-resource-usage -c twostage.hip -o A/t.o 2> A/log   (parent; same for B)
    python tools/poly_asm_diff.py A/twostage-hip-amdgcn-amd-amdhsa-gfx950.s B/twostage-hip-amdgcn-amd-amdhsa-gfx950.s [B/log]

Kernels are matched by demangled name (c++filt), with a trailing defaulted `, false` template argument dropped — the equal-length
instances of k_poly gained `bool RAGGED = false`.  Every kernel of A must be in B with the same instruction text (labels and
their numbers normalised, comments and directives dropped).  Kernels only in B are listed, with VGPRs, scratch and occupancy from
the remarks log when one is given.  Exit status 1 on any difference."""
import re
import subprocess
import sys


def kernels(path):
    out, name, body = {}, None, []
    for ln in open(path):
        m = re.match(r"^(_Z\w+):\s", ln)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        s = ln.split(";")[0].strip()
        if s.startswith(".Lfunc_end"):
            out[name], name = body, None
            continue
        if not s or s.startswith(".") and not s.startswith(".LBB"):
            continue
        body.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return out


def demangle(names):
    txt = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return {n: re.sub(r", false>$", ">", d.split("(")[0]) for n, d in zip(names, txt)}  # (the argument list: PolyArgs / PolyArgsOf<false>::type)


def remarks(path):
    """-> {mangled name: {field: value}} from -Rpass-analysis=kernel-resource-usage"""
    out, cur = {}, None
    for ln in open(path):
        m = re.search(r"remark: .*Function Name: (\S+)", ln)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r":\s{2,}(.+?): (\S+) \[-Rpass", ln)
        if m and cur is not None:
            cur[m.group(1).split(" [")[0]] = m.group(2)
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    da, db = demangle(sorted(a)), demangle(sorted(b))
    by_name_b = {d: n for n, d in db.items()}
    bad = 0
    for n, d in sorted(da.items(), key=lambda t: t[1]):
        if d not in by_name_b:
            print("MISSING in the second build:", d)
            bad += 1
        elif a[n] != b[by_name_b[d]]:
            print("DIFFERENT (%d vs %d instructions): %s" % (len(a[n]), len(b[by_name_b[d]]), d))
            bad += 1
    print("%d kernels of the first build compared, %d differ or are missing" % (len(da), bad))
    rem = remarks(sys.argv[3]) if len(sys.argv) > 3 else {}
    new = sorted((d, n) for n, d in db.items() if d not in set(da.values()))
    print("%d new kernels" % len(new))
    for d, n in new:
        r = rem.get(n, {})
        print("  %-60s VGPRs %s AGPRs %s scratch %s occupancy %s LDS %s" % (d, r.get("VGPRs"), r.get("AGPRs"), r.get("ScratchSize"),
                                                                       r.get("Occupancy"), r.get("LDS Size")))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
