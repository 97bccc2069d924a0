#!/usr/bin/env python
"""Two device assemblies of one source (hipcc --offload-arch=gfx950 -O3 -std=c++17 --offload-device-only -S, the library's flags), kernel by
kernel: registers and LDS from the .amdhsa_kernel block, whether the instruction streams are identical, and whether the opcode sequence
from the first to the last v_mfma is.  How profiles/wino_f43_registers.txt was made:
    python tools/compare_kernel_asm.py parent_stream1x1_f32.s change_stream1x1_f32.s
--step adds, per kernel, the instruction counts of the steady-state step (the loop with the most matrix instructions), per step: how
profiles/ws1x1f_step_isa.txt was made.  Kernels are matched by mangled name; --strip TEXT removes TEXT from the names of the second file first (a template parameter added at the
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


FP32_VALU = re.compile(r"v_(pk_)?(add|sub|mul|fma|fmac|mac|mad|max|min)_(legacy_)?f32")
NOT_SALU = ("s_waitcnt", "s_nop", "s_barrier", "s_cbranch", "s_branch", "s_endpgm", "s_setprio", "s_sleep")


def steady_step(body):
    """The steady-state step of a kernel: the loop (a label up to a branch back to it, whatever blocks lie between) that holds the most
    matrix instructions; among equals the shortest -> its instructions, or [] where there is no loop"""
    best, at, o = [], {}, []
    for ln in body.split("\n"):
        m = re.match(r"^(\.L\w+):", ln)
        if m:
            at[m.group(1)] = len(o)
            continue
        ln = ln.split(";")[0].strip()
        if not ln or ln.startswith("."):
            continue
        o.append(ln)
        if ln.startswith(("s_cbranch", "s_branch")) and ln.split()[-1] in at:
            cur = o[at[ln.split()[-1]]:]
            n, nb = sum(x.startswith("v_mfma") for x in cur), sum(x.startswith("v_mfma") for x in best)
            if n > nb or (n == nb and n and len(cur) < len(best)):
                best = cur
    return best


def step_counts(o):
    """Of a step's instructions: matrix, VALU as accumulator reads / integer, select and compare / fp32 arithmetic, vector memory, LDS, SALU"""
    c = dict.fromkeys(("mfma", "acc_read", "int_valu", "fp32_valu", "vmem", "ds", "salu"), 0)
    for x in o:
        op = x.split()[0]
        if op.startswith("v_mfma"):
            c["mfma"] += 1
        elif op.startswith("v_accvgpr_read"):
            c["acc_read"] += 1
        elif FP32_VALU.match(op):
            c["fp32_valu"] += 1
        elif op.startswith("v_"):
            c["int_valu"] += 1
        elif op.startswith(("buffer_", "global_", "flat_", "scratch_")):
            c["vmem"] += 1
        elif op.startswith("ds_"):
            c["ds"] += 1
        elif op.startswith("s_") and not op.startswith(NOT_SALU):
            c["salu"] += 1
    return c


def per_step(o):
    """(steps the loop holds — the compiler unrolls it —, counts per step): a step has one s_barrier; without barriers the loop is one step"""
    n = max(1, sum(x.startswith("s_barrier") for x in o))
    return n, {k: v / float(n) for k, v in step_counts(o).items()}


def step_table(a, b):
    """--step: the steady-state step of every kernel both files have, parent / change, per step"""
    keys = ("mfma", "acc_read", "int_valu", "fp32_valu", "vmem", "ds", "salu")
    print("steady-state step: the loop with the most v_mfma, its counts divided by the steps it holds (one s_barrier each; `unroll`), parent / change.")
    print("acc_read = v_accvgpr_read; fp32_valu = fp32 add / mul / fma / max, packed or not; int_valu = every other VALU instruction (addresses, selects,")
    print("compares, moves); vmem = buffer / global instructions; salu = scalar ALU instructions (waits, nops, barriers and branches not counted).")
    print("%-86s %-7s %s  %s" % ("kernel", "unroll", " ".join("%-11s" % k for k in keys), "MFMA opcodes of a step"))
    fmt = lambda v: ("%d" % v) if v == int(v) else ("%.1f" % v)  # noqa: E731
    for k in sorted(set(a) & set(b)):
        sa, sb = steady_step(a[k]), steady_step(b[k])
        (na, ca), (nb, cb) = per_step(sa), per_step(sb)
        ma, mb = [x.split()[0] for x in sa if x.startswith("v_mfma")], [x.split()[0] for x in sb if x.startswith("v_mfma")]
        same = len(ma) % na == 0 and len(mb) % nb == 0 and ma[:len(ma) // na] == mb[:len(mb) // nb]
        print("%-86s %-7s %s  %s" % (k[:86], "%d/%d" % (na, nb), " ".join("%-11s" % ("%s/%s" % (fmt(ca[q]), fmt(cb[q]))) for q in keys), "identical" if same else "DIFFER"))


if __name__ == "__main__":
    args = sys.argv[1:]
    step = "--step" in args
    if step:
        args.remove("--step")
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
    if step:
        print()
        step_table(a, b)
