"""Compare two hipcc -S --offload-device-only outputs kernel by kernel, instruction lines only.

  python tools/asm_diff.py OLD.s NEW.s [MORE_NEW.s ...] [--map OLDNAME=NEWNAME ...]

Directive and comment lines are dropped, the per-function number of .LBB<n>_ labels is removed and
the __hip_cuid_* symbol is ignored, so a kernel that only moved within its file, or to another
file, compares equal. Several NEW files are read as one (a translation unit that was split). --map
replaces a substring of the OLD kernel names first (a kernel that was renamed, e.g. de-templated).
Prints the kernels that differ with their line counts and those present on one side only; exit
status 1 if there are any."""
import argparse
import re
import sys


def kernels(path):
    """{kernel symbol: [instruction and label lines]} of one device assembly file"""
    lines = open(path).read().split("\n")
    names = {m.group(1) for ln in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln))}
    out, cur = {}, None
    for ln in lines:
        s = ln.split(";")[0].strip()
        if s.endswith(":") and s[:-1] in names:
            cur = out.setdefault(s[:-1], [])
        elif s.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and s and "__hip_cuid_" not in s and (not s.startswith(".") or s.endswith(":")):
            cur.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return out


ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("old")
ap.add_argument("new", nargs="+")
ap.add_argument("--map", action="append", default=[], metavar="OLD=NEW")
args = ap.parse_args()
old = kernels(args.old)
for m in args.map:
    a, b = m.split("=", 1)
    old = {k.replace(a, b): v for k, v in old.items()}
new = {}
for p in args.new:
    new.update(kernels(p))
both = sorted(set(old) & set(new))
differ = [k for k in both if old[k] != new[k]]
for k in differ:
    print(f"DIFFERS  {k}: {len(old[k])} -> {len(new[k])} lines")
for k in sorted(set(old) - set(new)):
    print(f"OLD ONLY {k}: {len(old[k])} lines")
for k in sorted(set(new) - set(old)):
    print(f"NEW ONLY {k}: {len(new[k])} lines")
print(f"{len(both) - len(differ)} identical, {len(differ)} differ, {len(set(old) - set(new))} only in old, "
      f"{len(set(new) - set(old))} only in new")
sys.exit(1 if differ or set(old) ^ set(new) else 0)
