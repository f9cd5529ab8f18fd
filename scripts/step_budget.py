#!/usr/bin/env python3
"""Per-segment instruction budget of the path kernel's step, from an IPT_MARK
listing (hipcc -S with -DIPT_AB_BUILD -DIPT_DIAGNOSTIC_BUILD -DIPT_C2_ONLY=1
-DIPT_MARK=1): the ;@STAMP comments mark the step's segments in source order,
but the listing's block layout does not follow source order, so instructions
are attributed by basic block: the control-flow graph is rebuilt from the
labels and branches, and the marks are propagated forward through it (a block
belongs to the segment whose opening mark reaches its entry).

Cold blocks are counted apart: the out-of-table frame angle (f64 division /
rsq), the non-power-of-two res/n divisions of the pop, the sqrt tie of
longer_sq in resolve, and every block reachable only through them.

The `cycles` column weighs the counts by what a wave64 instruction of each
class costs the SIMD's issue (scripts/ubench_valu.hip, measured on the MI355X:
profiles/round1_ubench_valu.jsonl and round1_ubench_path.jsonl, the
cycles_per_wave_op of v_add_f32 / v_fma_f32, "u32*u32->u64 + xor", v_rcp_f32,
v_mul_f64 / v_fma_f64): a plain VALU instruction 2.5 cycles, v_mad_u64_u32 (the
Philox multiplies) 7.8, a transcendental (rcp, rsq, sqrt, exp, log, sin, cos)
8, an f64 instruction 4.2 (the f64 transcendentals of the cold blocks count
as transcendentals). SALU, LDS and memory instructions are not in it: the
column prices the VALU pipe alone, so it ranks VALU-for-VALU rewrites; a trade
between VALU and scalar instructions or branches, which take the wave's issue
slot too, still needs an A/B.

usage: step_budget.py listing.s [--instance REGEX] [--blocks]
--instance: a regular expression searched in the mangled kernel names; the
default is the product (COUNT = false) 4-level box instance, in range where
the range form is an instance parameter.
"""
import re
import sys
from collections import defaultdict

SEG = {  # opening mark -> the segment it opens (ipt_kernels.hip, IPT_STAMP_AT)
    7: "loop top", 0: "refill", 1: "(pop at step top: empty)", 2: "frame need", 3: "prologue + Philox + gathers + frame",
    4: "exit test", 5: "new path + direction", 8: "light trace + pdf", 9: "mixture + geometry",
    10: "resolve + push", 11: "pre-skip + pop", 6: "frame prefetch",
}
ORDER = [7, 0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 6]
TRANS = ("v_rcp", "v_rsq", "v_sqrt", "v_exp", "v_log", "v_sin", "v_cos")
LANE = ("v_readlane", "v_writelane", "v_readfirstlane", "ds_bpermute", "ds_permute", "v_permlane")
# cycles per wave64 instruction (profiles/round1_ubench_valu.jsonl)
CYC_PLAIN, CYC_MAD64, CYC_TRANS, CYC_F64 = 2.5, 7.8, 8.0, 4.2
COLD_F64 = ("v_rsq_f64", "v_div_scale_f64", "v_rcp_f64", "v_div_fmas_f64", "v_div_fixup_f64")


def body_of(txt, inst):
    for m in re.finditer(r"\n(_Z\S*path_kernel\S*):[^\n]*\n(.*?)\n\.Lfunc_end", txt, re.S):
        if re.search(inst, m.group(1)):
            return m.group(2)
    raise SystemExit(f"no path_kernel instance matching {inst}")


def blocks_of(body):
    """[(labels, [op lines], mark or None)] -- a block also ends at a mark, so
    that a mark is always the first thing of its block."""
    blocks, cur = [], dict(labels=[], ops=[], mark=None, depth2=False)

    def flush():
        nonlocal cur
        if cur["labels"] or cur["ops"] or cur["mark"] is not None:
            blocks.append(cur)
        cur = dict(labels=[], ops=[], mark=None, depth2=False)

    for line in body.split("\n"):
        m = re.match(r"(\.LBB\d+_\d+):", line)
        if m:
            if cur["ops"] or cur["mark"] is not None:
                flush()
            cur["labels"].append(m.group(1))
            cur["depth2"] = "Depth=2" in line or "Inner Loop" in line
            continue
        if line.startswith("; %bb."):
            if cur["ops"] or cur["mark"] is not None:
                flush()
            cur["depth2"] = "Depth=2" in line
            continue
        if "Depth=2" in line:
            cur["depth2"] = True
        m = re.match(r"\s*;@STAMP (\d+)", line)
        if m:
            flush()
            cur["mark"] = int(m.group(1))
            continue
        s = line.strip()
        if not line.startswith("\t") or not s or s[0] in ".;":
            continue
        cur["ops"].append(s)
        if s.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc")):
            flush()
    flush()
    return blocks


def analyse(blocks):
    index = {l: i for i, b in enumerate(blocks) for l in b["labels"]}
    succ = defaultdict(list)
    for i, b in enumerate(blocks):
        last = b["ops"][-1] if b["ops"] else ""
        op = last.split()[0] if last else ""
        if op.startswith(("s_cbranch", "s_branch")):
            succ[i].append(index[last.split()[-1]])
        if not op.startswith(("s_branch", "s_endpgm", "s_setpc")) and i + 1 < len(blocks):
            succ[i].append(i + 1)
    pred = defaultdict(list)
    for i, ss in succ.items():
        for s in ss:
            pred[s].append(i)
    # forward propagation of the opening mark
    seg_in = [set() for _ in blocks]
    out = [None] * len(blocks)
    work = [0]
    seen = set()
    while work:
        i = work.pop()
        o = {blocks[i]["mark"]} if blocks[i]["mark"] is not None else set(seg_in[i])
        if i in seen and o == out[i]:
            continue
        seen.add(i)
        out[i] = o
        for s in succ[i]:
            if not o <= seg_in[s]:
                seg_in[s] |= o
            work.append(s)
    seg = []
    for i, b in enumerate(blocks):
        s = {b["mark"]} if b["mark"] is not None else seg_in[i]
        seg.append(tuple(sorted(s)))
    # cold seeds, then everything reachable only through cold blocks
    cold = [False] * len(blocks)
    for i, b in enumerate(blocks):
        ops = [o.split()[0] for o in b["ops"]]
        if any(o.startswith(COLD_F64) for o in ops):
            cold[i] = True
        if seg[i] == (11,) and any(o.startswith("v_div_scale_f32") for o in ops):
            cold[i] = True
        if seg[i] == (10,) and any(o.startswith("v_sqrt_f32") for o in ops) and len(ops) < 12:
            cold[i] = True
    changed = True
    while changed:
        changed = False
        for i in range(1, len(blocks)):
            if not cold[i] and pred[i] and all(cold[p] for p in pred[i]):
                cold[i] = changed = True
    return seg, cold


def count(ops):
    c = defaultdict(int)
    for s in ops:
        o = s.split()[0]
        if o.startswith("v_"):
            c["valu"] += 1
            if o.startswith(TRANS):
                c["cycles"] += CYC_TRANS
            elif o.startswith("v_mad_u64_u32") or o.startswith("v_mad_i64_i32"):
                c["cycles"] += CYC_MAD64
            elif "f64" in o:
                c["cycles"] += CYC_F64
            else:
                c["cycles"] += CYC_PLAIN
            if o.startswith("v_mov") or o.startswith("v_accvgpr"):
                c["mov"] += 1
            elif o.startswith("v_cndmask"):
                c["cnd"] += 1
            elif o.startswith(LANE):
                c["lane"] += 1
            elif o.startswith(TRANS):
                c["trans"] += 1
            if "f64" in o:
                c["f64"] += 1
        elif o.startswith("s_"):
            c["salu"] += 1
            if o.startswith(("s_cbranch", "s_branch")):
                c["br"] += 1
            if "saveexec" in o:
                c["sx"] += 1
            if o.startswith("s_nop"):
                c["nop"] += 1
        elif o.startswith("ds_"):
            c["lds"] += 1
        elif o.startswith(("global_", "buffer_", "flat_", "scratch_")):
            c["vmem"] += 1
    return c


COLS = ("cycles", "valu", "mov", "cnd", "lane", "trans", "f64", "salu", "br", "sx", "nop", "lds", "vmem")


def fmt(v):
    return f"{v:7.0f}"


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    inst = r"path_kernelILi4ELb0ELi\d+ELi0E(Lb1E){0,2}EEvNS"
    if "--instance" in sys.argv:
        inst = sys.argv[sys.argv.index("--instance") + 1]
        args.remove(inst)
    blocks = blocks_of(body_of(open(args[0]).read(), inst))
    seg, cold = analyse(blocks)
    rows = defaultdict(lambda: defaultdict(int))
    for i, b in enumerate(blocks):
        if not seg[i]:
            key = "setup / exit (outside the step loop)"
        elif len(seg[i]) > 1:
            key = "shared by segments " + ",".join(map(str, seg[i]))
        else:
            key = SEG[seg[i][0]]
            if seg[i] == (11,) and b["depth2"] and not cold[i]:
                key = "pop: levels past the first two (loop)"
        if cold[i]:
            key = "COLD " + key
        for k, v in count(b["ops"]).items():
            rows[key][k] += v
        if "--blocks" in sys.argv:
            print(i, b["labels"], seg[i], "cold" if cold[i] else "", dict(count(b["ops"])))
    names = [SEG[s] for s in ORDER] + ["pop: levels past the first two (loop)"]
    names += sorted(k for k in rows if k not in names and not k.startswith(("COLD", "setup")))
    hot = defaultdict(int)
    print(f"{'segment':52s}" + "".join(f"{c:>7s}" for c in COLS))
    for n in names:
        if n in rows:
            print(f"{n:52s}" + "".join(fmt(rows[n][c]) for c in COLS))
            if not n.startswith("pop: levels"):
                for c in COLS:
                    hot[c] += rows[n][c]
    print(f"{'HOT STEP (every wave-step; without the pop loop)':52s}" + "".join(fmt(hot[c]) for c in COLS))
    for n in sorted(rows):
        if n.startswith(("COLD", "setup")):
            print(f"{n:52s}" + "".join(fmt(rows[n][c]) for c in COLS))
    print("columns: cycles = VALU issue cycles per wave (plain 2.5, v_mad_u64_u32 7.8, trans 8, f64 4.2);")
    print("         valu = all VALU, of which mov (v_mov), cnd (v_cndmask), lane (read/writelane), trans, f64;")
    print("         salu = all SALU, of which br (branches), sx (saveexec), nop (s_nop); lds; vmem")


if __name__ == "__main__":
    main()
