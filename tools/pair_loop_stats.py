#!/usr/bin/env python3
"""What a plane step of cheby_pair_kernel executes, read from the gfx950 assembly (needs the compiler, no GPU).

usage: tools/pair_loop_stats.py [--asm FILE.s [--before-edgew | --before-ua] | --src FILE.hip] [INSTANCE ...]
  INSTANCE: the template arguments <V,NW,C32,SM,NARROW,INTERP,REMOTE,FORM[,EDGEW[,UA]]>, e.g. 0,10,false,0,false,false,false,true (EDGEW, UA: false when left out)
  default:  the config-2 instance of the pre-pass path, its NARROW twin, its INTERP twin and the 12-wave instance, then the EDGEW twins (an eleventh wave
            forms the tile-edge columns; the loop reported is the main waves' segment step, the edge wave's own loop is the smaller one), then the UA twin of each
            (alpha from the arguments: the EDGEW ones are what config 2 runs)
Without --asm, hpgmg_amd/csrc/kernels/pair.hip (or --src) is compiled to device assembly with the flags of the Makefile.

Per instance: the kernel's VGPR / SGPR counts and spill counts, and for its largest INNERMOST loop (natural loops of the control-flow graph; the one that holds no
other loop and the most instructions is the steady-state step of the march -- the parent's single march loop) the instructions by category, the marks of address work (integer-division sequences,
64-bit LDS reads = box-table lookups, lane reads = SGPR-spill restores) and the global loads in blocks that a step may skip, by the kind of branch that decides.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = ["0,10,false,0,false,false,false,true", "0,10,false,0,true,false,false,true", "0,10,false,0,false,true,false,true", "0,12,false,0,false,false,false,true",
           "0,10,false,0,false,false,false,true,true", "0,10,false,0,false,true,false,true,true"]
DEFAULT = DEFAULT + [d + (",false,true" if d.count(",") == 7 else ",true") for d in DEFAULT]


BEFORE_EDGEW = False      # --before-edgew: the assembly is of a commit whose kernel has eight template parameters
BEFORE_UA = False         # --before-ua: ... nine (no UA)


def mangled(inst):
    parts = [a.strip() for a in inst.split(",")]
    assert len(parts) in (8, 9, 10), "eight template arguments, nine with EDGEW, ten with UA"
    want = 8 if BEFORE_EDGEW else (9 if BEFORE_UA else 10)
    if len(parts) > want:
        return "cheby_pair_kernel_has_no_such_instance"
    parts += ["false"] * (want - len(parts))
    enc = "".join("Lb%dE" % (a == "true") if a in ("true", "false") else "Li%sE" % a for a in parts)
    return "cheby_pair_kernelI" + enc + "E"


def compile_asm(src):
    out = os.path.join(tempfile.mkdtemp(prefix="pair_loop_stats_"), "pair.s")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "hpgmg_amd", "csrc", "kernels"), "-S", "--cuda-device-only", "-o", out, src]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    return out


def kernel_body(lines, frag):
    """(name, [(label or None, mnemonic, operands)]) of the kernel whose symbol holds `frag`."""
    start = next((i for i, l in enumerate(lines) if re.match(r"^_Z\w*%s\w*:" % re.escape(frag), l)), None)
    if start is None:
        return None, []
    name, body, label = lines[start].split(":")[0], [], None
    for l in lines[start + 1:]:
        s = l.split(";")[0].strip()
        if s.startswith(".Lfunc_end") or s.startswith(".section"):
            break
        m = re.match(r"^(\.LBB\w+):", s)
        if m:
            label = m.group(1)
            continue
        if not s or s.startswith("."):
            continue
        tok = s.split(None, 1)
        body.append((label, tok[0], tok[1] if len(tok) > 1 else ""))
        label = None
    return name, body


def metadata(lines, name):
    out, on = {}, False
    for l in lines:
        if ".name:" in l:
            on = l.split()[-1] == name
        m = re.match(r"\s*\.(vgpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s*(\d+)", l)
        if on and m:
            out[m.group(1)] = int(m.group(2))
    return out


def category(op):
    if op == "s_waitcnt":
        return "wait"
    if op == "s_barrier":
        return "barrier"
    if op.startswith("s_cbranch") or op == "s_branch":
        return "branch"
    if op.startswith(("s_load", "s_buffer_load")):
        return "scalar load"
    if op.startswith("s_"):
        return "SALU"
    if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
        return "lane read/write"
    if op.startswith("v_") and "_f64" in op:
        return "fp64"
    if op.startswith("v_"):
        return "other VALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_load", "flat_load")):
        return "global load"
    if op.startswith(("global_store", "flat_store")):
        return "global store"
    if op.startswith("scratch_"):
        return "scratch (VGPR spill)"
    return "other"


def cfg(body):
    """Basic blocks [(first, last)] of the instruction list and their successor lists."""
    pos = {lab: i for i, (lab, _, _) in enumerate(body) if lab}
    heads = {0} | set(pos.values())
    for i, (_, op, _) in enumerate(body):
        if category(op) == "branch" or op in ("s_endpgm", "s_setpc_b64"):
            heads.add(i + 1)
    heads = sorted(h for h in heads if h < len(body))
    blocks = [(h, (heads[n + 1] if n + 1 < len(heads) else len(body)) - 1) for n, h in enumerate(heads)]
    at = {h: n for n, (h, _) in enumerate(blocks)}
    succ = []
    for n, (h, t) in enumerate(blocks):
        _, op, args = body[t]
        out = []
        if category(op) == "branch" and args.strip() in pos:
            out.append(at[pos[args.strip()]])
        if op not in ("s_branch", "s_endpgm", "s_setpc_b64") and n + 1 < len(blocks):
            out.append(n + 1)
        succ.append(out)
    return blocks, succ


def dominators(succ):
    n = len(succ)
    pred = [[] for _ in range(n)]
    for u, out in enumerate(succ):
        for v in out:
            pred[v].append(u)
    dom = [set(range(n)) for _ in range(n)]
    dom[0] = {0}
    changed = True
    while changed:
        changed = False
        for v in range(1, n):
            ps = [dom[u] for u in pred[v]]
            new = (set.intersection(*ps) if ps else set()) | {v}
            if new != dom[v]:
                dom[v], changed = new, True
    return dom, pred


def natural_loops(succ, dom, pred):
    """header -> set of blocks (the loops of all back edges to one header merged)."""
    loops = {}
    for u, out in enumerate(succ):
        for h in out:
            if h in dom[u]:
                body, work = {h, u}, [u]
                while work:
                    x = work.pop()
                    if x == h:
                        continue
                    for q in pred[x]:
                        if q not in body:
                            body.add(q); work.append(q)
                loops.setdefault(h, set()).update(body)
                loops[h].add(("latch", u))
    return loops


def report(lines, inst):
    name, body = kernel_body(lines, mangled(inst))
    print("== cheby_pair_kernel<%s>" % inst)
    if not body:
        print("   not in this assembly")
        return
    md = metadata(lines, name)
    print("   kernel: %d instructions, VGPRs %s (spilled %s), SGPRs %s (spilled %s), scratch %s bytes" % (
        len(body), md.get("vgpr_count"), md.get("vgpr_spill_count"), md.get("sgpr_count"), md.get("sgpr_spill_count"), md.get("private_segment_fixed_size")))
    blocks, succ = cfg(body)
    dom, pred = dominators(succ)
    loops = natural_loops(succ, dom, pred)
    latches = {h: [x[1] for x in l if isinstance(x, tuple)] for h, l in loops.items()}
    loops = {h: {x for x in l if not isinstance(x, tuple)} for h, l in loops.items()}
    inner = {h: l for h, l in loops.items() if not any(o != h and o in l for o in loops)}
    if not inner:
        print("   no loop")
        return
    size = lambda l: sum(blocks[x][1] - blocks[x][0] + 1 for x in l)
    h, l = max(inner.items(), key=lambda kv: size(kv[1]))
    loop = [body[i] for x in sorted(l) for i in range(blocks[x][0], blocks[x][1] + 1)]
    counts = {}
    for _, op, _ in loop:
        counts[category(op)] = counts.get(category(op), 0) + 1
    print("   largest innermost loop: %d instructions in %d basic blocks (%d innermost loops in the kernel)" % (len(loop), len(l), len(inner)))
    for k in ("fp64", "other VALU", "SALU", "scalar load", "LDS", "global load", "global store", "scratch (VGPR spill)", "lane read/write", "wait", "branch", "barrier", "other"):
        if counts.get(k):
            print("     %-22s %4d" % (k, counts[k]))
    ops = [op for _, op, _ in loop]
    n = lambda pre: sum(1 for o in ops if o.startswith(pre))
    print("   address work: v_mov_b64 %d, v_lshl_add_u64 %d, s_mul_i32 %d, mul_hi (integer division) %d, v_rcp_iflag_f32 %d, ds_read_b64 (table lookups) %d, v_readlane_b32 (SGPR-spill restores) %d"
          % (n("v_mov_b64"), n("v_lshl_add_u64"), n("s_mul_i32"), n("s_mul_hi") + n("v_mul_hi_u32"), n("v_rcp_iflag"), n("ds_read_b64") + n("ds_read2_b64"), n("v_readlane")))
    waits = [args for _, op, args in loop if op == "s_waitcnt"]
    print("   waits: vmcnt(0) %d, other vmcnt %d, lgkmcnt-only %d" % (sum(1 for w in waits if "vmcnt(0)" in w), sum(1 for w in waits if "vmcnt" in w and "vmcnt(0)" not in w),
                                                                         sum(1 for w in waits if "vmcnt" not in w)))
    # loads in blocks that not every iteration passes (they do not dominate the latch), by the branch that decides: the nearest dominating block of the loop ending in one
    always = set.intersection(*[dom[u] for u in latches[h]])
    behind = {}
    for x in sorted(l):
        loads = sum(1 for i in range(blocks[x][0], blocks[x][1] + 1) if category(body[i][1]) == "global load")
        if not loads or x in always:
            continue
        guards = [d for d in dom[x] if d != x and d in l and body[blocks[d][1]][1].startswith("s_cbranch")]
        guard = max(guards, key=lambda d: len(dom[d])) if guards else None
        kind = "?" if guard is None else ("exec mask (lanes)" if "exec" in body[blocks[guard][1]][1] else "scalar / vcc condition (%s)" % body[blocks[guard][1]][1])
        behind[kind] = behind.get(kind, 0) + loads
    print("   global loads in blocks a step may skip: %s" % (", ".join("%d under %s" % (v, k) for k, v in sorted(behind.items())) or "none"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--asm", help="device assembly of pair.hip, already compiled")
    ap.add_argument("--src", default=os.path.join(ROOT, "hpgmg_amd", "csrc", "kernels", "pair.hip"))
    ap.add_argument("--before-edgew", action="store_true", help="the assembly (--asm) comes from a commit before the EDGEW template parameter: eight arguments in the symbol")
    ap.add_argument("--before-ua", action="store_true", help="the assembly (--asm) comes from a commit before the UA template parameter: nine arguments in the symbol")
    ap.add_argument("instances", nargs="*", default=DEFAULT)
    args = ap.parse_args()
    global BEFORE_EDGEW, BEFORE_UA
    BEFORE_EDGEW, BEFORE_UA = args.before_edgew, args.before_ua
    lines = open(args.asm or compile_asm(args.src)).read().splitlines()
    for inst in args.instances:
        report(lines, inst)
    return 0


if __name__ == "__main__":
    sys.exit(main())
