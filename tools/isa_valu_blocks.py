"""Developer helper: VALU instructions per basic block of one kernel in a hipcc -S listing, split into the scan's
essential set (v_xor, v_bcnt, v_fmaak, v_min_u16) and the rest, with the LDS instructions beside them.
    python tools/isa_valu_blocks.py <listing.s> <mangled-name-prefix> [--min N]"""
import collections, re, sys
t = open(sys.argv[1]).read().splitlines()
name = sys.argv[2]
least = int(sys.argv[sys.argv.index("--min") + 1]) if "--min" in sys.argv else 1
s = next(i for i, l in enumerate(t) if l.startswith(name) and ":" in l)
e = next(i for i in range(s, len(t)) if "s_endpgm" in t[i])
ESSENTIAL = ("v_xor_b32", "v_bcnt_u32_b32", "v_fmaak_f32", "v_min_u16")
blocks, cur = [], ["entry", collections.Counter()]
for l in t[s + 1:e + 1]:
    m = re.match(r"(\.LBB\d+_\d+):", l) or re.match(r"; %bb\.(\d+):", l)
    if m:
        blocks.append(cur)
        cur = [m.group(1) if l.startswith(".") else "bb." + m.group(1), collections.Counter()]
        continue
    w = l.split()
    if l.startswith("\t") and w and not w[0].startswith((";", ".")):
        cur[1][w[0]] += 1
blocks.append(cur)
tot_e = tot_o = 0
print(f"{'block':12s} {'essential':>9s} {'other VALU':>10s} {'LDS':>4s}  other VALU by opcode")
for label, h in blocks:
    ess = sum(n for k, n in h.items() if k in ESSENTIAL)
    oth = {k: n for k, n in h.items() if k.startswith("v_") and k not in ESSENTIAL}
    lds = sum(n for k, n in h.items() if k.startswith("ds_"))
    tot_e += ess; tot_o += sum(oth.values())
    if ess + sum(oth.values()) + lds >= least:
        print(f"{label:12s} {ess:9d} {sum(oth.values()):10d} {lds:4d}  " + " ".join(f"{k}:{n}" for k, n in sorted(oth.items())))
print(f"{'total':12s} {tot_e:9d} {tot_o:10d}")
