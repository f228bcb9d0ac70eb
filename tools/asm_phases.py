"""Debug: the vector instructions of the pipeline's k_vote_mfma by source phase, from the
device assembly with line tables (-gline-tables-only: every instruction carries the source
line it was made from; an inlined helper's instruction carries the helper's line, and is
given to the named phase of that helper or, for the shared ones (exact_vote, the wave
reductions, the math headers), to the phase of the kernel line last seen before it).
usage: asm_phases.py [CSRC_DIR]      (default: this tree's pvnet_amd/csrc)
Static counts.  The phases outside the hot loop, the band phase and the rare passes are
straight-line code that a wave runs once per segment or per sub-chunk (one of each on the
bench's frames), so there the static count is what a wave executes up to the branches it
skips; v_readlane / v_writelane are the spilled scalar registers' reloads and spills, each
a vector-issue slot."""
import collections
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pvnet_amd import build as B  # noqa: E402

csrc = sys.argv[1] if len(sys.argv) > 1 else B.CSRC
src = os.path.join(csrc, "pvvote.hip")
text = open(src).read().split("\n")
k0 = next(i for i, l in enumerate(text) if "void k_vote_mfma(" in l) + 1


def at(s, after=k0):
    return next(i for i in range(after - 1, len(text)) if s in text[i]) + 1


# (phase, first line) inside k_vote_mfma, in source order; a phase runs to the next one's first line
MARKS = [("work split", k0),
         ("pixel load", at("// ---- segment:")),
         ("hypothesis load + classify", at("// hypotheses: lane ")),
         ("counts + tail", at("int cnt[kMSet]")),
         ("pixel prep (prep_compacted, exact slab)", at("for (int s0 = ts; s0 < te; s0 += kMChunk)")),
         ("box", at("if (wid * kWave < np) {")),
         ("put_rows", at("auto put_rows")),
         ("pixel load", at("// next sub-chunk's loads")),
         ("box", at("float cxl = kBig, cxh = -kBig")),
         ("put_rows", at("put_rows(ox, oy, slow);")),
         ("hscale + B fragments", at("if (!slow) {", at("put_rows(ox, oy, slow);"))),
         ("hot loop", at("uint32_t neg[kMSet]")),
         ("counts + tail", at("// positives = slots")),
         ("band phase", at("// ---- band pairs")),
         ("exact-only pass / slow sub-chunk", at("// exact-only hypotheses (rare")),
         ("counts + tail", at("// the reference pass's corrections")),
         ("end", at("// The matrix-core vote (k_vote_mfma): its own fast-path constant"))]
# inlined helpers outside the kernel's lines, by function
HELPERS = {"even_share": "work split", "round_share": "work split", "tn_at": "work split",
           "pixel_exact": "pixel load", "item_hyp": "hypothesis load + classify",
           "prep_compacted": "pixel prep (prep_compacted, exact slab)", "form_row": "put_rows", "pack_h2": "put_rows"}


def helper_ranges():
    out = []
    for name, ph in HELPERS.items():
        for i, l in enumerate(text):
            if re.search(r"\b" + name + r"\(", l) and "__device__" in l:
                j = next(k for k in range(i, len(text)) if text[k] == "}")
                out.append((i + 1, j + 1, ph))
    return out


HR = helper_ranges()


def phase_of(fname, line):
    base = os.path.basename(fname)
    if base == "pv_hypclass.h":
        return "hypothesis load + classify"
    if base != "pvvote.hip":                       # pv_common.h (exact_vote, reductions), HIP's math headers:
        return None                                # the phase of the kernel line last seen before it
    if MARKS[0][1] <= line < MARKS[-1][1]:
        ph = MARKS[0][0]
        for name, first in MARKS:
            if line >= first:
                ph = name
        return ph
    for a, b, ph in HR:
        if a <= line <= b:
            return ph
    return None                                    # (ExactSlab's put / get: staging, or a reference pass)


with tempfile.TemporaryDirectory() as td:
    out = os.path.join(td, "k.s")
    subprocess.check_call([B.hipcc(), *[f for f in B.HIPCC_FLAGS if f not in ("-shared", "-fPIC", "-Wall")],
                           "-gline-tables-only", "-I", B.CSRC, "--cuda-device-only", "-S", "-o", out, src],
                          stderr=subprocess.DEVNULL)
    s = open(out).read().split("\n")
files = {}
for l in s:
    m = re.match(r"\s*\.file\s+(\d+)\s+\"([^\"]*)\"(?:\s+\"([^\"]*)\")?", l)
    if m:
        files[int(m.group(1))] = m.group(3) or m.group(2)
start = next(i for i, l in enumerate(s) if l.startswith("_Z") and "k_vote_mfmaILb1" in l and l.split(":")[0].endswith("E"))
valu, lanes, cur, last = collections.Counter(), collections.Counter(), ("", 0), "work split"
for l in s[start + 1:]:
    t = l.split(";")[0].strip()
    if t.startswith(".Lfunc_end"):
        break
    m = re.match(r"\.loc\s+(\d+)\s+(\d+)", t)
    if m:
        cur = (files.get(int(m.group(1)), ""), int(m.group(2)))
        continue
    if not t or t.startswith(".") or t.endswith(":"):
        continue
    op = t.split()[0]
    ph = phase_of(*cur) or last
    last = ph
    if op.startswith(("v_readlane", "v_writelane")):
        lanes[ph] += 1
    elif op.startswith("v_"):
        valu[ph] += 1
print(f"{'phase':52s} {'VALU':>6s} {'readlane/writelane':>20s}")
for ph in sorted(set(valu) | set(lanes), key=lambda p: -valu[p]):
    print(f"{ph:52s} {valu[ph]:6d} {lanes[ph]:20d}")
print(f"{'total':52s} {sum(valu.values()):6d} {sum(lanes.values()):20d}")
