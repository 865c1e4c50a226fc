"""What the compiler put between consecutive MFMAs of the split NeRF kernels' K-steps, from a `hipcc -S` file.

  hipcc -O3 -std=c++17 -ffp-contract=off --offload-arch=gfx950 -S --cuda-device-only -Inerfmatch_amd/csrc -Iinclude \
      nerfmatch_amd/csrc/nerf_fwd_bf16.hip -o nerf_fwd_bf16.s
  python scripts/kstep_gaps.py nerf_fwd_bf16.s nerf_fwd_fp16x3_kernel [--all]

A half slot is 12 consecutive MFMAs on the same four accumulator blocks; two halves in a row are one K-step (slot_step8: different blocks,
slot_step4x2: the same blocks), a half on its own is a slot_step4.  "odd" K-steps hold the ring barrier, "even" ones the eight LDS-DMA
pieces of the weight request.  Per gap (the instructions behind MFMA k of a half, up to the next MFMA) the mix is printed as
  <n> ds_read, <n> VALU (accumulator reads included), <n> s_nop, <n> SALU, DMA pieces, waits and barriers.
A scalar ALU instruction takes an issue turn of the wavefront's one in-order stream like a VALU one and is COUNTED like one (round 11,
scripts/ubench/fillers.hip, profiles/r11_ubench_fillers_salu.log: 3 or 6 independent SALU per gap hide behind the MFMA, 10 cost 12 cycles
per gap -- 3.6 cycles each against the 24 an MFMA leaves; beside an LDS-DMA piece 1 or 3 are free, 10 cost 50 cycles); `s_waitcnt` and
`s_barrier` are listed and not counted.  The gap is marked `OVER` unless it is one of (nerf_split_chain.h, "Per-gap schedule"):
  one DMA piece and nothing else but at most one scalar write of M0 (the LDS base of the pieces that follow)  |  <= 2 ds_read + <= 3
  VALU/SALU/s_nop  |  <= 5 VALU/SALU/s_nop  |  <= 4 ds_read and nothing else (the bias
  reads of a views-layer unit)  |  one global store and nothing else (a row of the tapped layer stored from inside a K-loop: DESIGN
  section 3.1, round 10).
`--m0` instead lists every instruction of the kernel that names M0 and every LDS-DMA instruction, and exits non-zero unless the kernel
owns M0 (nerf_split_chain.h, dma_slot): every one of them stands in an inline-asm block of the project, and M0 is only ever written there,
as `s_mov_b32 m0, <sgpr>` or `s_add_u32 m0, m0, <constant>` -- never read, never saved, never set by the compiler.
K-steps with the same mix in every gap are printed once, with their count and the line of the first (--all: every K-step).  The gap behind
a K-step's last MFMA is the hand-over to whatever follows when no K-step follows directly (or only across a branch); it is printed but not judged.
"""
import argparse
import re
import sys
from collections import OrderedDict

MFMA = re.compile(r"^\s+v_mfma_\S+\s+(a\[\d+:\d+\]|v\[\d+:\d+\])")
INSN = re.compile(r"^\s+([a-z_][a-z0-9_]*)\b")
M0_WRITE = re.compile(r"^(s_mov_b32 m0, (s\d+|vcc_lo|vcc_hi)|s_add_u32 m0, m0, (0x[0-9a-f]+|\d+))\s*(;.*)?$")
M0_NAMED = re.compile(r"\bm0\b")


def m0_report(lines, start, end, name):
    """Every instruction that names M0 and every LDS-DMA, with whether it stands in an inline-asm block; the number that break the rule."""
    in_asm, bad, rows = False, 0, []
    for i in range(start, end):
        t = lines[i].strip()
        if t.startswith(";;#ASMSTART"):
            in_asm = True
        elif t.startswith(";;#ASMEND"):
            in_asm = False
        m = INSN.match(lines[i])
        if not m or t.startswith((";", ".")):
            continue
        code = t.split(";")[0].strip()
        dma = classify(m.group(1)) == "dma"
        if not (dma or M0_NAMED.search(code)):
            continue
        ok = in_asm and (dma or bool(M0_WRITE.match(code)))
        bad += not ok
        rows.append((code, in_asm, ok, i + 1))
    kinds = OrderedDict()
    for code, ia, ok, ln in rows:
        key = (re.sub(r"\b(s|v)\d+\b", r"\1N", re.sub(r"\[\d+:\d+\]", "[N:N]", re.sub(r"offset:\d+", "offset:K", code))), ia, ok)
        kinds.setdefault(key, []).append(ln)
    print(f"{name}: {len(rows)} instructions name M0 or are LDS-DMA; {bad} not of the project's own pattern")
    for (code, ia, ok), lns in kinds.items():
        print(f"  {len(lns):4d} x  {code:60s} {'inline asm' if ia else 'COMPILER'}  {'ok' if ok else 'NOT OWNED'}  (first at line {lns[0]})")
    return bad


def kernel_lines(path, name):
    lines = open(path).read().split("\n")
    start = next((i for i, l in enumerate(lines) if re.match(r"^\S*" + re.escape(name) + r"\S*:", l)), None)
    if start is None:
        sys.exit(f"no kernel matching {name!r} in {path}")
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    return lines, start, end


def classify(op):
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("ds_read") or op.startswith("ds_load"):
        return "ds"
    if op.startswith("ds_"):
        return "ds_other"
    if op.startswith("global_load_lds") or (op.startswith("buffer_load") and op.endswith("lds")):
        return "dma"
    if op.startswith(("global_store", "buffer_store")):
        return "store"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op == "s_nop":
        return "nop"
    if op == "s_waitcnt":
        return "wait"
    if op == "s_barrier":
        return "barrier"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_"):
        return "salu"
    return "other"


class Gap:
    def __init__(self):
        self.n = dict(ds=0, ds_other=0, dma=0, vmem=0, store=0, nop=0, wait=0, barrier=0, valu=0, salu=0, m0=0, other=0)
        self.ops = []

    def add(self, op, text):
        kind = classify(op)
        if kind == "salu" and M0_WRITE.match(text):
            kind = "m0"
        self.n[kind] += 1
        self.ops.append(text)

    def vector(self):  # issue turns of 4 cycles: VALU, s_nop and (round 11) scalar ALU
        return self.n["valu"] + self.n["nop"] + self.n["salu"] + self.n["m0"]

    def over(self):
        n = self.n
        if n["dma"]:
            return n["dma"] > 1 or n["valu"] or n["nop"] or n["salu"] or n["m0"] > 1 or n["ds"] or n["ds_other"] or n["vmem"] or n["store"]
        if n["store"]:
            return n["store"] > 1 or self.vector() or n["ds"] or n["ds_other"] or n["vmem"]
        if n["ds"] or n["ds_other"]:
            if n["ds"] <= 4 and not (n["ds_other"] or self.vector() or n["vmem"]):
                return False
            return n["ds"] + n["ds_other"] > 2 or self.vector() > 3 or n["vmem"]
        return self.vector() > 5 or n["vmem"]

    def mix(self, salu=True):
        n, parts = self.n, []
        for key, label in (("dma", "DMA piece"), ("ds", "ds_read"), ("ds_other", "other ds"), ("vmem", "vmem"), ("store", "store"), ("valu", "VALU"), ("nop", "s_nop"),
                           ("salu", "SALU"), ("m0", "M0 write"),
                           ("wait", "s_waitcnt"), ("barrier", "s_barrier"), ("other", "other")):
            if n[key] and (salu or key != "salu"):
                parts.append(f"{n[key]} {label}")
        return ", ".join(parts) if parts else "nothing"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("kernel", help="substring of the kernel's symbol")
    ap.add_argument("--all", action="store_true", help="print every K-step, not one per distinct mix")
    ap.add_argument("--ops", action="store_true", help="list the instructions of the gaps marked OVER")
    ap.add_argument("--m0", action="store_true", help="list what touches M0 instead; exit 1 unless the kernel owns it")
    a = ap.parse_args()
    lines, start, end = kernel_lines(a.asm, a.kernel)
    if a.m0:
        sys.exit(1 if m0_report(lines, start, end, a.kernel) else 0)
    # the MFMA stream with the gap behind each
    mf = []  # (line, accumulator, Gap)
    for i in range(start, end):
        l = lines[i]
        m = MFMA.match(l)
        if m:
            mf.append((i + 1, m.group(1), Gap()))
            continue
        m = INSN.match(l)
        if m and mf and not l.lstrip().startswith((";", ".")):
            mf[-1][2].add(m.group(1), l.strip())
    # halves: 12 MFMAs on the same four accumulator blocks, each block three times
    halves, i = [], 0
    while i + 12 <= len(mf):
        accs = [x[1] for x in mf[i:i + 12]]
        if len(set(accs[:4])) == 4 and accs[4:8] == accs[:4] and accs[8:12] == accs[:4]:
            halves.append(i)
            i += 12
        else:
            i += 1
    steps, k = [], 0
    while k < len(halves):
        if k + 1 < len(halves) and halves[k + 1] == halves[k] + 12 and len(mf[halves[k] + 11][2].ops) < 60:
            steps.append((halves[k], 2))
            k += 2
        else:
            steps.append((halves[k], 1))
            k += 1
    nm = sum(12 * h for _, h in steps)
    vm = [lines[i].strip() for i in range(mf[0][0], mf[-1][0]) if INSN.match(lines[i]) and INSN.match(lines[i]).group(1) == "s_waitcnt" and "vmcnt" in lines[i]] if mf else []
    print(f"s_waitcnt with vmcnt between the first and the last MFMA: {len(vm)}: " + ", ".join(f"{vm.count(t)} x {t}" for t in sorted(set(vm))))
    print(f"{a.asm}: {a.kernel}: {len(mf)} MFMAs, {nm} of them in {len(steps)} K-steps; s_barrier {sum(1 for i in range(start, end) if INSN.match(lines[i]) and INSN.match(lines[i]).group(1) == 's_barrier')}")
    groups = OrderedDict()
    for idx, (h0, nh) in enumerate(steps):
        gaps = [mf[h0 + j][2] for j in range(12 * nh)]
        follows = (idx + 1 < len(steps) and steps[idx + 1][0] == h0 + 12 * nh and len(gaps[-1].ops) < 60
                   and not any(t.startswith(("s_cbranch", "s_branch")) for t in gaps[-1].ops))
        same = nh == 2 and mf[h0][1] == mf[h0 + 12][1]
        kind = ("slot_step4x2" if same else "slot_step8") if nh == 2 else "slot_step4"
        parity = "odd" if any(g.n["barrier"] for g in gaps[:-1] + ([gaps[-1]] if follows else [])) else ("even" if any(g.n["dma"] for g in gaps) else "plain")
        rows = []
        for j, g in enumerate(gaps):
            last = j == len(gaps) - 1 and not follows
            where = ("first half " if j < 12 else "second half ") + str(j % 12) if nh == 2 else f"gap {j}"
            rows.append((where, g.mix() if not last else f"hand-over, not judged: {len(g.ops)} instructions", (not last) and bool(g.over()), None if last else g))
        sig = (kind, parity, tuple((r[0], r[1] if r[3] is None else r[3].mix(salu=False), r[2]) for r in rows))  # (scalar ALU does not tell K-steps apart)
        if a.all:
            sig = sig + (idx,)
        groups.setdefault(sig, []).append((mf[h0][0], rows))
    total_over = 0
    for sig, inst in groups.items():
        kind, parity = sig[0], sig[1]
        n_over = sum(1 for r in inst[0][1] if r[2])
        total_over += n_over * len(inst)
        print(f"\n{kind}, {parity} K-step: {len(inst)} x, first at line {inst[0][0]}" + (f"; {n_over} gap(s) over budget" if n_over else "; every gap within budget"))
        print("| gap (behind MFMA) | between it and the next MFMA | |")
        print("|---|---|---|")
        for where, mix, over, g in inst[0][1]:
            print(f"| {where} | {mix} | {'OVER' if over else ''} |")
            if over and a.ops and g is not None:
                for t in g.ops:
                    print(f"|   | `{t}` | |")
    print(f"\ngaps over budget, all K-steps: {total_over}")


if __name__ == "__main__":
    main()
