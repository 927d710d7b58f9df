#!/usr/bin/env python3
"""Compare the gfx950 ISA of named kernels between two builds of the library.

Both builds are made with `--save-temps`; the device assembly is the `*-gfx950.s` each leaves behind. A kernel's body is the text between
its label and its `.Lfunc_end`; debug-line directives are dropped and the numbers of the local labels are renumbered in order of
appearance, so that a kernel which merely moved in the file compares equal.

    python tools/isa_diff.py OLD.s NEW.s k_flat_lane k_addp_size k_flat_parse k_flat_sizeILb0E=k_flat_sizeILi0E

A name is a substring of the mangled names to compare; OLD=NEW compares kernels whose mangled names differ between the builds (a template
parameter that changed its type).
"""
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    with open(path) as fh:
        for ln in fh:
            m = re.match(r"^(_Z\w+):\s", ln)
            if m and name is None:
                name, body = m.group(1), []
                continue
            if name is not None:
                if ln.startswith(".Lfunc_end"):
                    out[name] = body
                    name = None
                    continue
                s = ln.split(";")[0].rstrip() if not ln.lstrip().startswith(";") else ""
                if not s or re.match(r"\s*\.(loc|file|cfi|p2align)", s):
                    continue
                body.append(s)
    return out


def normal(body):
    ids = {}

    def sub(m):
        return ".L%d" % ids.setdefault(m.group(0), len(ids))

    return [re.sub(r"\.L\w+", sub, s) for s in body]


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    rc = 0
    for want in sys.argv[3:]:
        want, _, other = want.partition("=")
        names = sorted(n for n in old if want in n)
        if not names:
            print(want, "not found")
            rc = 2
        for n in names:
            a, b = normal(old[n]), normal(new.get(n.replace(want, other) if other else n, []))
            if other:  # symbols named after the kernel (its LDS)
                a = [x.replace(want, other) for x in a]
            same = a == b
            print("%-60s %6d -> %6d lines  %s" % (n, len(a), len(b), "identical" if same else "DIFFERENT"))
    return rc


if __name__ == "__main__":
    sys.exit(main())
