"""Compare the instruction bodies of every kernel in two `make asm` outputs (build/*.s of two trees): a change that must not touch the
existing kernels (a new template instance beside them, a host-side refactor) shows an empty diff here.  Labels are renumbered, comments,
blank lines and section directives dropped, and demangled names normalised (`void f<>(P)` == `f(P)`: an empty template pack), so
only the instructions and their operands are compared.  usage: python tools/asm_kernel_diff.py OLD_BUILD_DIR NEW_BUILD_DIR"""
import os
import re
import subprocess
import sys


def kernels(path):
    """{mangled name: normalised body} of the functions in one .s file"""
    out, name, body = {}, None, []
    for ln in open(path).read().split("\n"):
        if name is None:
            m = re.match(r"^([A-Za-z_][\w$.]*):", ln)
            if m and m.group(1).startswith("_Z"):
                name, body = m.group(1), []
            continue
        if re.match(r"^\.Lfunc_end\d+:", ln):
            out[name] = body
            name = None
            continue
        ln = re.sub(r";.*$", "", ln).strip()
        if not ln or ln.startswith((".section", ".text")):
            continue
        ln = re.sub(r"\s+", " ", ln)
        ln = re.sub(r"\.LBB\d+_", ".LBB_", ln)
        body.append(ln.replace(name, "SELF"))
    return out


def demangle(names):
    res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    # (PointLightShape<L> became PointLightShape<L, ANY = 0x7F>: the instance of the full mask is the old one under a longer name)
    return {n: re.sub(r"(PointLightShape<\d+), 127u>", r"\1>", re.sub(r"^void ", "", d).replace("<>", "")) for n, d in zip(names, res)}


def main():
    old_dir, new_dir = sys.argv[1], sys.argv[2]
    changed = compared = 0
    for f in sorted(x for x in os.listdir(old_dir) if x.endswith(".s")):
        old, new = kernels(os.path.join(old_dir, f)), kernels(os.path.join(new_dir, f))
        dn = demangle(list(new))
        by_name = {dn[k]: v for k, v in new.items()}
        for k, body in old.items():
            d = demangle([k])[k]
            compared += 1
            if by_name.get(d) != body:
                changed += 1
                print("%s: %s %s" % (f, d, "missing" if d not in by_name else "differs"))
        print("%s: %d functions compared, %d new ones" % (f, len(old), len(set(by_name) - set(demangle(list(old)).values()))))
    print("%d functions compared, %d differ" % (compared, changed))
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
