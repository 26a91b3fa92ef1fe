"""What the dense factorisation's schedule does around its bulk update, from a timeline written by tools/trace_timeline.py
(all rows: `trace_timeline.py results.db 2000 > timeline.txt`):
  - k_ldl_update launches of the fused zone (each follows a k_ldl_pairtrsm and runs beside the hoisted workgroup): average
    duration, and that of the other bulk launches;
  - the tail: wall time from the start of the last k_ldl_pairtrsm (the last fused pair) to the end of the factorisation;
  - the look-ahead below the fused zone: per k_ldl_update_part (the rest of a pair's update, second queue), how much of
    it ran beside kernels of the main queue.
usage: ldl_schedule_report.py timeline.txt"""
import re
import sys

rows = []
for line in open(sys.argv[1]):
    m = re.match(r"(k_\w+)\s+start\s+([\d.]+) end\s+([\d.]+) dur\s+([\d.]+) us q(\S+)", line)
    if m:
        rows.append((m.group(1), float(m.group(2)), float(m.group(3)), m.group(5)))
main_q = rows[0][3]
main = [r for r in rows if r[3] == main_q]
fused, other = [], []
for a, b in zip(main, main[1:]):
    if b[0] == "k_ldl_update":
        (fused if a[0] == "k_ldl_pairtrsm" else other).append(b[2] - b[1])
end = max(r[2] for r in rows)
print("span of the factorisation: %.1f us, %d kernels" % (end - rows[0][1], len(rows)))
if fused:
    print("k_ldl_update beside the hoisted workgroup (fused zone): n %d  avg %.1f us" % (len(fused), sum(fused) / len(fused)))
if other:
    print("k_ldl_update, other launches: n %d  avg %.1f us" % (len(other), sum(other) / len(other)))
last = [r for r in main if r[0] == "k_ldl_pairtrsm"]
if last:
    print("tail, from the last fused pair's panel kernel to the end: %.1f us" % (end - last[-1][1]))
rests = [r for r in rows if r[0] == "k_ldl_update_part"]
tot = hid = 0.0
for r in rests:
    o = sum(max(0.0, min(r[2], m[2]) - max(r[1], m[1])) for m in main)
    tot += r[2] - r[1]
    hid += o
    print("  rest start %9.1f dur %6.1f us, %5.1f us beside the main queue's kernels" % (r[1], r[2] - r[1], o))
if rests:
    print("rests: n %d  sum %.1f us, %.1f us of it beside the main queue's kernels" % (len(rests), tot, hid))
