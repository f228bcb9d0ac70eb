"""Is every device function of the working tree the same code as in git revision REV?

    python tools/kernel_asm_diff.py REV

Exports pvnet_amd/csrc and include/ of REV to a temporary directory, compiles
every translation unit of both trees to gfx950 assembly with build.HIPCC_FLAGS
and compares the function bodies, keyed by demangled symbol across all
translation units of a tree (so a kernel may move between files).  Comments,
the per-file function index in .LBB<n>_ labels and the namespace a symbol's
types moved to do not count.  Prints each function as same / different /
only-old / only-new; exit status 0 only if all are "same".  Not part of the
product: the check a refactor of the kernels' files has to pass."""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pvnet_amd import build as B  # noqa: E402

CXXFILT = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")   # either demangles symbols inside text


def functions(src: str, tmp: str) -> dict:
    """{demangled symbol: normalised body} of one translation unit"""
    s = B.asm(src, os.path.join(tmp, os.path.basename(src) + ".s"))
    text = subprocess.run([CXXFILT], input=open(s).read(), capture_output=True, text=True, check=True).stdout
    text = re.sub(r"\(anonymous namespace\)::|pvv::", "", text)
    out = {}
    for m in re.finditer(r"^\t\.type\t([^\n]+),@function\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S):
        body = [re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0].rstrip()) for ln in m.group(2).split("\n")]
        # What is left: labels, instructions and, for a kernel, its descriptor -- llvm emits the
        # .amdhsa_kernel block (register and LDS sizes) after the code and before .Lfunc_end, so it
        # is compared too.  The .section lines around it carry mangled names and are dropped.
        out[m.group(1)] = "\n".join(ln for ln in body if ln and not ln.startswith("\t.section\t"))
    return out


def merged(parts: list) -> dict:
    """One tree's functions; one name with two different bodies in two translation units (anonymous
    namespaces allow it) is an error, not a silent overwrite"""
    out = {}
    for part in parts:
        dup = sorted(k for k in set(out) & set(part) if out[k] != part[k])
        if dup:
            sys.exit("one name, different code in two translation units of one tree: " + ", ".join(dup))
        out.update(part)
    return out


def tree(csrc: str, tmp: str) -> dict:
    os.makedirs(tmp)
    with ThreadPoolExecutor(4) as ex:
        parts = list(ex.map(lambda p: functions(p, tmp), sorted(glob.glob(os.path.join(csrc, "*.hip")))))
    return merged(parts)


def main(rev: str) -> int:
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", B.REPO, "archive", rev, "pvnet_amd/csrc", "include"], capture_output=True,
                             check=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        old = tree(os.path.join(tmp, "pvnet_amd", "csrc"), os.path.join(tmp, "old_s"))
        new = tree(B.CSRC, os.path.join(tmp, "new_s"))
    verdicts = {k: "same" if old.get(k) == new.get(k) else "only-old" if k not in new else "only-new" if k not in old
                else "different" for k in sorted(set(old) | set(new))}
    for k, v in verdicts.items():
        print(f"{v:9s} {k}")
    n = sum(v == "same" for v in verdicts.values())
    print(f"{n} of {len(verdicts)} functions same")
    return 0 if n == len(verdicts) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
