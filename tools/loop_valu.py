"""VALU instruction counts of the loop bodies of one kernel in a device ISA listing (hipcc -S --cuda-device-only).
A loop is a backward branch to a label of the same function; its body is the text from the label to the branch
(inner loops are counted with the loops that contain them).  Prints, for every loop with at least MIN VALU
instructions, the fp64 VALU count (v_*_f64), the other VALU count, LDS and scalar-memory counts.
Usage: python tools/loop_valu.py file.s 'k_blkseg_evalILi2ELi3ELi8ELi0ELb0' [MIN=40]

These are sums over the whole text of a body: a loop that holds two variants of a step behind a branch (the select
and the no-select variant of the segmented eval's slice-steps before they were peeled apart) counts both, although one
iteration runs one of them.  For what one iteration issues, follow one path:
  python tools/loop_valu.py file.s KERNEL --path .LBB20_1091 [DECISIONS]
walks from the label to the first branch back to it.  An unconditional forward branch is followed; at a conditional
one the next letter of DECISIONS decides (t: taken, n: not taken; not taken once the letters run out).  Every
conditional branch met is printed with its line in the function and the decision used, so that the letters can be
fitted to the path wanted (compare the counts of the variants: the select variant has the v_cndmask).  Counts along
the path: fp64 VALU, v_mov_b64, v_readlane, other VALU, DS, SALU, branches, s_waitcnt, and the s_waitcnt lgkmcnt that
stand directly behind the DS read they wait for (exposed LDS latency)."""
import re
import sys

path, pat = sys.argv[1], sys.argv[2]
lines = open(path).read().splitlines()
start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*%s\w*:" % re.escape(pat), l))
end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
body = lines[start:end + 1]
labels = {}
for i, l in enumerate(body):
    m = re.match(r"^(\.LBB\d+_\d+):", l)
    if m:
        labels[m.group(1)] = i


def walk(head, decisions):
    """Instruction mnemonics along one path from label head to the first branch back to it."""
    i, ins, log, d = labels[head] + 1, [], [], list(decisions)
    for _ in range(100000):
        s = body[i]
        i += 1
        if not re.match(r"^\s+[a-z]", s):
            continue
        op = s.split()[0]
        ins.append(op)
        m = re.match(r"^\s+(s_c?branch\w*)\s+(\.LBB\d+_\d+)", s)
        if not m:
            if op == "s_endpgm":
                break
            continue
        tgt = m.group(2)
        if m.group(1) == "s_branch":
            if tgt == head:
                return ins, log
            i = labels[tgt] + 1
            continue
        take = (d.pop(0) if d else "n") == "t"
        log.append((i - 1, m.group(1), tgt, "taken" if take else "not taken"))
        if take:
            if tgt == head:
                return ins, log
            i = labels[tgt] + 1
    raise SystemExit("the path does not return to " + head)


if len(sys.argv) > 3 and sys.argv[3] == "--path":
    head = sys.argv[4]
    ins, log = walk(head, sys.argv[5] if len(sys.argv) > 5 else "")
    for ln, op, tgt, how in log:
        print(f"  line {ln:6d} {op} {tgt}: {how}")
    f64 = sum(1 for s in ins if s.startswith("v_") and "_f64" in s)
    mov64 = sum(1 for s in ins if s.startswith("v_mov_b64"))
    rdl = sum(1 for s in ins if s.startswith("v_readlane") or s.startswith("v_writelane"))
    valu = sum(1 for s in ins if s.startswith("v_")) - f64 - mov64 - rdl
    ds = sum(1 for s in ins if s.startswith("ds_"))
    br = sum(1 for s in ins if re.match(r"s_c?branch", s))
    wt = ins.count("s_waitcnt")
    salu = sum(1 for s in ins if s.startswith("s_")) - br - wt
    exposed = sum(1 for a, b in zip(ins, ins[1:]) if a.startswith("ds_read") and b == "s_waitcnt")
    print(f"path {head}: fp64 VALU {f64}  v_mov_b64 {mov64}  v_readlane/writelane {rdl}  other VALU {valu}  ds {ds}  "
          f"salu {salu}  branches {br}  s_waitcnt {wt} (directly behind a ds_read: {exposed})  total {len(ins)}")
    sys.exit(0)

minv = int(sys.argv[3]) if len(sys.argv) > 3 else 40
print(lines[start][:-1], "instructions:", sum(1 for l in body if re.match(r"^\s+[sv]_|^\s+ds_|^\s+global_|^\s+buffer_", l)))
for i, l in enumerate(body):
    m = re.match(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
    if not m or m.group(1) not in labels or labels[m.group(1)] >= i:
        continue
    seg = body[labels[m.group(1)]:i]
    ins = [s.split()[0] for s in seg if re.match(r"^\s+[a-z]", s)]
    f64 = sum(1 for s in ins if s.startswith("v_") and "_f64" in s)
    valu = sum(1 for s in ins if s.startswith("v_")) - f64
    if f64 + valu >= minv:
        print(f"  loop {m.group(1):12s} fp64 VALU {f64:4d}  other VALU {valu:4d}  ds {sum(1 for s in ins if s.startswith('ds_')):3d}"
              f"  scalar {sum(1 for s in ins if s.startswith('s_')):3d}  total {len(ins):4d}")
