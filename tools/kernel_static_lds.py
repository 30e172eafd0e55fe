#!/usr/bin/env python3
"""Static LDS of every instantiation of k_trace, k_shade_pool, k_bounce_carry and k_bounce against the bounds check_static_lds
(csrc/ptx_api.inc) applies on a kernel's first launch -- a kernel over its bound aborts the process there, so this is read before
a kernel nobody has launched is launched.  Runs without a GPU.
usage: tools/kernel_static_lds.py [FILE]   FILE: a saved table of tools/kernel_resources.py (default: the tool is run)"""
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
RESERVE_TRACE = 1024                       # launch_trace's `reserve`
RESERVE_BOUNCE = 2 * 256 * 4 + 512         # PT_LDS_CU_BYTES - PT_LDS_BOUNCE_LIMIT (PT_SOLO_MAX_BLOCKS = 256)
STATIC_MAX = (2048 + 92 - 1) & ~63         # PT_LDS_STATIC_MAX (PT_SWZ_NODE_BYTES = 92)

text = open(sys.argv[1]).read() if len(sys.argv) > 1 else subprocess.run([sys.executable, os.path.join(HERE, "kernel_resources.py")],
                                                                        capture_output=True, text=True, check=True).stdout
rows = []
for line in text.splitlines():
    m = re.match(r"\s*(?:\d+\s+){6}(\d+)\s+(k_trace|k_shade_pool|k_bounce_carry|k_bounce)<(.*)>\s*$", line)
    if not m:
        continue
    lds, fam, args = int(m.group(1)), m.group(2), [a.strip() for a in m.group(3).split(",")]
    if fam == "k_trace":  # <MODE, COUNT, PRIMARY, LDS_SCENE, PACKET>
        reserve, lds_scene = RESERVE_TRACE, args[3] == "true"
    elif fam == "k_bounce":  # <MODE, COUNT, EMIT, PRIMARY, LDS_SCENE, SOLO_T, LIT, LANE_WALK, IMG>
        reserve, lds_scene = RESERVE_BOUNCE, args[4] == "true"
    elif fam == "k_bounce_carry":  # <MODE, COUNT, EMIT, PRIMARY, LANE_WALK, LOCT, TILE>: the per-octant image is not the shared one
        reserve, lds_scene = RESERVE_BOUNCE, not (len(args) > 5 and args[5] == "true")
    else:  # launch_shade_pool applies no check
        reserve, lds_scene = None, False
    bound = None if reserve is None else (min(reserve, STATIC_MAX) if lds_scene else reserve)
    rows.append((fam, "%s<%s>" % (fam, ", ".join(args)), lds, bound))
for fam in ("k_trace", "k_shade_pool", "k_bounce_carry", "k_bounce"):
    rs = [r for r in rows if r[0] == fam]
    print("%s: %d instantiations, static LDS %s" % (fam, len(rs), ", ".join("%d B x %d" % (v, sum(r[2] == v for r in rs)) for v in sorted({r[2] for r in rs}))))
print()
print("%6s %6s %4s  kernel" % ("LDS", "bound", "ok"))
bad = 0
for fam, name, lds, bound in rows:
    ok = bound is None or lds <= bound
    bad += not ok
    print("%6d %6s %4s  %s" % (lds, "-" if bound is None else bound, "yes" if ok else "NO", name))
print()
print("%d instantiations, %d over their bound." % (len(rows), bad))
sys.exit(1 if bad else 0)
