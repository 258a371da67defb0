"""VALU instruction counts of the loop bodies of one kernel in a device ISA listing (hipcc -S --cuda-device-only).
A loop is a backward branch to a label of the same function; its body is the text from the label to the branch
(inner loops are counted with the loops that contain them).  Prints, for every loop with at least MIN VALU
instructions, the fp64 VALU count (v_*_f64), the other VALU count, LDS and scalar-memory counts.
Usage: python tools/loop_valu.py file.s 'k_blkseg_evalILi2ELi3ELi8ELi0ELb0' [MIN=40]"""
import re
import sys

path, pat = sys.argv[1], sys.argv[2]
minv = int(sys.argv[3]) if len(sys.argv) > 3 else 40
lines = open(path).read().splitlines()
start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*%s\w*:" % re.escape(pat), l))
end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
body = lines[start:end + 1]
labels = {}
for i, l in enumerate(body):
    m = re.match(r"^(\.LBB\d+_\d+):", l)
    if m:
        labels[m.group(1)] = i
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
