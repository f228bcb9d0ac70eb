"""Debug: per-basic-block instruction counts of one kernel in the device
assembly of the translation unit that holds it.
usage: asm_blocks.py NAME-SUBSTRING [TU.hip | FILE.s]
TU.hip defaults to pvvote.hip, the fused vote/count kernels alone (k_vote_mfma,
k_vote_count, k_hyp_gen); k_vote_bytes and the other API kernels are pvapi.hip's.
A TU is read from csrc/TU.gfx950.s, which pvnet_amd.build.asm(TU) writes; it is
compiled again only if that file is older than the sources."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pvnet_amd import build as B  # noqa: E402

tu = sys.argv[2] if len(sys.argv) > 2 else "pvvote.hip"
path = tu if tu.endswith(".s") else os.path.join(B.CSRC, os.path.splitext(tu)[0] + ".gfx950.s")
if not tu.endswith(".s") and B.older(path, (*B.closure([os.path.join(B.CSRC, tu)]), B.__file__)):
    B.asm(tu)
s = open(path).read().split("\n")
key = sys.argv[1]
start = next(i for i, l in enumerate(s) if l.startswith("_Z") and key in l and l.split(":")[0].endswith("E"))
blocks, cur = [], ["entry", 0, 0, 0, 0, []]
for l in s[start + 1:]:
    t = l.split(";")[0].strip()
    if t.startswith(".Lfunc_end"):
        break
    if not t or (t.startswith(".") and not t.endswith(":")):
        continue
    if t.endswith(":"):
        blocks.append(cur)
        cur = [t[:-1], 0, 0, 0, 0, []]
        continue
    op = t.split()[0]
    cur[1] += 1
    cur[2] += op.startswith("v_")
    cur[3] += op.startswith(("ds_", "global_", "buffer_", "flat_"))
    if op.startswith(("s_cbranch", "s_branch")):
        cur[5].append(t.split()[-1])
blocks.append(cur)
names = [b[0] for b in blocks]
tot = 0
for k, b in enumerate(blocks):
    tot += b[1]
    back = [x for x in b[5] if x in names and names.index(x) <= k]
    print(f"{b[0]:14s} n={b[1]:4d} valu={b[2]:4d} mem={b[3]:3d} cum={tot:5d}" + (f"  LOOP->{back}" if back else ""))
