"""Static issue-cost model of a sampler kernel's step loop (no GPU): extracts the kernel's gfx950 ISA from a
libdmip.so and prices every MFMA gap as max(MFMA cycles, 8 + the issue costs of the instructions placed in
it), with MI355X_MICROARCH.md's per-instruction constants (transcendental 8, other VALU / s_nop / LDS / VMEM
issue 4, SALU 1). Prints the modelled cycles between consecutive s_barriers (one per ring chunk), then the whole
step loop (the innermost backward branch enclosing every MFMA of the kernel) with its scratch accesses.
    python scripts/isa_issue_model.py <libdmip.so> <kernel-symbol-substring> [mfma_cycles=16]
--hist prints the step loop's instruction histogram instead (count and issue cycles per mnemonic, then one summary line:
MFMAs, transcendentals, AGPR copies, s_nop statements and wait states, barriers, scratch accesses):
    python scripts/isa_issue_model.py --hist <libdmip.so> <kernel-symbol-substring>"""
import functools
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_isa  # noqa: E402


@functools.lru_cache(maxsize=4)
def _disassemble(so, i):
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, f"co{i}.o")
        open(p, "wb").write(check_isa.code_objects(so)[i])
        return subprocess.run([check_isa.LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", p],
                              capture_output=True, text=True).stdout.splitlines()


def kernel_lines(so, sym):
    """The instruction lines of the first kernel whose symbol holds `sym`: only code objects that name it are
    disassembled, once per library and object."""
    for i, o in enumerate(check_isa.code_objects(so)):
        if sym.encode() not in o:
            continue
        L = _disassemble(so, i)
        for k, line in enumerate(L):
            if sym in line and line.endswith(">:"):
                out = []
                for l in L[k + 1:]:
                    if l.endswith(">:"):
                        break
                    out.append(l)
                return out
    raise SystemExit(f"{sym} not found")


def cost(op):
    if op.startswith("v_mfma"):
        return None
    if re.match(r"v_(exp|rcp|log|sqrt|rsq|sin|cos)_f32", op):
        return 8
    if op.startswith(("v_", "ds_", "buffer_", "global_", "scratch_")) or op == "s_nop":
        return 4
    return 1


def model(lines, mc):
    gap, tot, pre, n = None, 0, 0, 0
    for l in lines:
        m = re.match(r"\s+([a-z_0-9]+)", l)
        if not m:
            continue
        c = cost(m.group(1))
        if c is None:
            if gap is not None:
                tot += max(mc, gap)
            gap, n = 8, n + 1
        elif gap is None:
            pre += c
        else:
            gap += c
    if gap is not None:
        tot += max(mc, gap)
    return n, tot + pre


def step_loop(L, mc):
    """(MFMAs, modelled cycles, scratch instructions) of the innermost loop that holds every MFMA."""
    loop = loop_lines(L)
    if loop is None:
        return None
    n, c = model(loop[:-1], mc)
    return n, c, sum(1 for l in loop[:-1] if "scratch_" in l)


def loop_lines(L):
    """The step loop's instruction lines (step_loop's extent), or None."""
    addr = []
    for l in L:
        mm = re.search(r"//\s*([0-9A-F]{12}):", l)
        addr.append(int(mm.group(1), 16) if mm else None)
    mf = [i for i, l in enumerate(L) if "v_mfma" in l]
    best = None
    for i, l in enumerate(L):
        mm = re.match(r"\s+s_(cbranch_\w+|branch)\s+(\d+)", l)
        if not mm or addr[i] is None:
            continue
        off = int(mm.group(2))
        off = off - 65536 if off >= 32768 else off
        tgt = addr[i] + 4 + off * 4
        if tgt < addr[i] and tgt in addr:
            j = addr.index(tgt)
            if all(j <= x <= i for x in mf) and (best is None or i - j < best[1] - best[0]):
                best = (j, i)
    return None if best is None else L[best[0]:best[1] + 1]


def histogram(L):
    """Mnemonic -> count over the step loop, the s_nop wait states (sum of N + 1) and the MFMAs whose C / D operand is
    a VGPR."""
    loop = loop_lines(L)
    if loop is None:
        raise SystemExit("no loop holds every MFMA")
    hist, nop_states, mfma_vgpr = {}, 0, 0
    for l in loop:
        m = re.match(r"\s+([a-z_0-9]+)\s*(.*?)\s*(//.*)?$", l)
        if not m:
            continue
        op, args = m.group(1), m.group(2)
        hist[op] = hist.get(op, 0) + 1
        if op == "s_nop":
            nop_states += int(args.split()[0], 0) + 1
        if op.startswith("v_mfma") and args.lstrip().startswith("v"):
            mfma_vgpr += 1
    return hist, nop_states, mfma_vgpr


def print_histogram(L):
    hist, nop_states, mfma_vgpr = histogram(L)
    total = sum(hist.values())
    print(f"step loop: {total} instructions")
    print(f"{'instruction':32s} {'count':>6s} {'issue cycles':>12s}")
    issue_total = 0
    for op, n in sorted(hist.items(), key=lambda kv: (-kv[1], kv[0])):
        c = cost(op)
        cyc = n * (8 if c is None else c)
        if op == "s_nop":
            cyc = max(cyc, nop_states)
        issue_total += cyc
        print(f"{op:32s} {n:6d} {cyc:12d}")
    g = lambda *pre: sum(n for op, n in hist.items() if op.startswith(pre))
    print(f"summary: mfma {g('v_mfma')} (C/D in VGPRs: {mfma_vgpr}), "
          f"transcendental {sum(n for op, n in hist.items() if cost(op) == 8)}, "
          f"accvgpr_read {g('v_accvgpr_read')}, accvgpr_write {g('v_accvgpr_write')}, "
          f"s_nop {hist.get('s_nop', 0)} ({nop_states} wait states), ds_read_b128 {hist.get('ds_read_b128', 0)}, "
          f"s_barrier {hist.get('s_barrier', 0)}, s_waitcnt {hist.get('s_waitcnt', 0)}, scratch {g('scratch_')}, "
          f"issue cycles {issue_total}")


def main():
    if "--hist" in sys.argv:  # isa_issue_model.py --hist <libdmip.so> <kernel-symbol-substring>
        a = [x for x in sys.argv[1:] if x != "--hist"]
        print_histogram(kernel_lines(a[0], a[1]))
        return
    so, sym = sys.argv[1], sys.argv[2]
    mc = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    L = kernel_lines(so, sym)
    bars = [i for i, l in enumerate(L) if "s_barrier" in l]
    tot = 0
    for a, b in zip(bars[1:-1], bars[2:]):
        n, c = model(L[a:b], mc)
        tot += c
        print(f"{a:6d} mfma {n:4d} modelled {c:6d} (floor {n * mc})")
    print("chunks total", tot)
    sl = step_loop(L, mc)
    if sl:
        print(f"step loop: {sl[0]} MFMAs, modelled {sl[1]} cycles, {sl[2]} scratch instructions")


if __name__ == "__main__":
    main()
