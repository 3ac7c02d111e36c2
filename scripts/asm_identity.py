"""Development aid: are the kernels of two gfx950 assembly files the same machine code?

    hipcc --offload-arch=gfx950 <the library's flags> --cuda-device-only -S x.hip -o old.s   (and new.s)
    python scripts/asm_identity.py old.s new.s [renames.txt]

A kernel's body runs from its `_Z...:` label to `.Lfunc_end`; `;` comments are dropped and the
labels that carry the function's ordinal in the file (.LBB<n>_, .Ltmp<n>, .Lfunc_*<n>) are
renumbered, so a kernel compares equal wherever it stands in its file.  renames.txt holds one
`old_mangled_name new_mangled_name` pair per line for kernels whose template parameters changed.
Prints the kernels only in one file and those whose bodies differ; exit status 1 if any differ.
The comparison is of text only."""
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
        elif name and line.startswith(".Lfunc_end"):
            out[name] = normalise(name, body)
            name = None
        elif name:
            body.append(line)
    return out


def normalise(name, body):
    text = "\n".join(s for s in (re.sub(r";.*", "", ln).rstrip() for ln in body) if s).replace(name, "SELF")
    text = re.sub(r"\.LBB\d+_", ".LBB_", text)
    text = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", text)
    tmps = {}  # .Ltmp<n> counts through the whole file: number them by first use in this body
    return re.sub(r"\.Ltmp\d+", lambda m: tmps.setdefault(m.group(0), f".Ltmp_{len(tmps)}"), text)


def main(old_s, new_s, renames=None):
    old, new = kernels(old_s), kernels(new_s)
    ren = dict(ln.split() for ln in open(renames) if ln.strip()) if renames else {}
    old = {ren.get(k, k): (k, v) for k, v in old.items()}
    same = [k for k in old if k in new and old[k][1] == new[k]]
    differ = [k for k in old if k in new and old[k][1] != new[k]]
    print(f"{len(old)} kernels in {old_s}, {len(new)} in {new_s}: {len(same)} identical, {len(differ)} differ")
    for k, (was, _) in old.items():
        if k in new and was != k:
            print(f"renamed    {was} -> {k}" + ("  (DIFFERS)" if k in differ else ""))
    for k in differ:
        print(f"differs    {k}")
    for k in old:
        if k not in new:
            print(f"only old   {old[k][0]}")
    for k in new:
        if k not in old:
            print(f"only new   {k}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:4]))
