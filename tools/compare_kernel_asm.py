#!/usr/bin/env python
"""Two device assemblies of one source (hipcc --offload-arch=gfx950 -O3 -std=c++17 --offload-device-only -S, the library's flags), kernel by
kernel: registers and LDS from the .amdhsa_kernel block, whether the instruction streams are identical, and whether the opcode sequence
from the first to the last v_mfma is.  How profiles/wino_f43_registers.txt was made:
    python tools/compare_kernel_asm.py parent_stream1x1_f32.s change_stream1x1_f32.s
Kernels are matched by mangled name; --strip TEXT removes TEXT from the names of the second file first (a template parameter added at the
end of a parameter list shows up as one more 'Lb0E' in front of the argument types)."""
import re
import sys


def kernels(path, strip):
    txt = open(path).read()
    norm = (lambda k: k.replace(strip[0], strip[1])) if strip else (lambda k: k)
    body = {norm(m.group(1)): m.group(2) for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M)}
    meta = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", txt, re.S):
        d = []
        for k in ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size"):
            mm = re.search(r"\.amdhsa_%s (\S+)" % k, m.group(2))
            d.append(mm.group(1) if mm else "-")
        meta[norm(m.group(1))] = d
    return body, meta


def ops(b):
    out = []
    for ln in b.split("\n"):
        ln = ln.split(";")[0].strip()
        if ln and not ln.startswith(".") and not ln.endswith(":"):
            out.append(ln)
    return out


def mfma_span(o):
    idx = [i for i, x in enumerate(o) if x.startswith("v_mfma")]
    return [x.split()[0] for x in o[idx[0]:idx[-1] + 1]] if idx else []


if __name__ == "__main__":
    args = sys.argv[1:]
    strip = None
    if "--strip" in args:
        i = args.index("--strip")
        strip = (args[i + 1], args[i + 2])
        del args[i:i + 3]
    a, am = kernels(args[0], None)
    b, bm = kernels(args[1], strip)
    print("%-86s %-22s %-22s %-10s %-12s" % ("kernel", "parent VGPR SGPR scr LDS", "change VGPR SGPR scr LDS", "body", "MFMA span"))
    for k in sorted(set(a) | set(b)):
        if k in a and k in b:
            oa, ob = ops(a[k]), ops(b[k])
            print("%-86s %-22s %-22s %-10s %-12s" % (k[:86], " ".join(am[k]), " ".join(bm[k]), "identical" if oa == ob else "DIFFERS",
                                                     ("identical (%d)" % len(mfma_span(oa))) if mfma_span(oa) == mfma_span(ob) else "DIFFERS"))
        else:
            print("%-86s %-22s %-22s %-10s" % (k[:86], " ".join(am[k]) if k in a else "-", " ".join(bm[k]) if k in b else "-", "new" if k in b else "gone"))
