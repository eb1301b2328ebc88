"""The instructions of one kernel out of a `hipcc --save-temps` assembly file, for comparing a kernel between two builds.

    python tools/isa_body.py FILE.s MANGLED_NAME

Prints the lines from the kernel's label to its .Lfunc_end with comments, blank lines and section directives dropped, its own name replaced by KERNEL and
its basic-block labels (.LBB<function number>_<n>) by .LBBk_<n>: what remains is the same text for two builds exactly when the
kernel's code is, whatever the kernel is called and wherever it sits in the file.

    hipcc --offload-arch=gfx950 <the Makefile's flags> --save-temps -c kernels_lk.hip        # in each of the two trees
    diff <(python tools/isa_body.py parent/kernels_lk-hip-amdgcn-amd-amdhsa-gfx950.s _Z10k_lk_track11LkTrackArgs) \\
         <(python tools/isa_body.py this/kernels_lk-hip-amdgcn-amd-amdhsa-gfx950.s _Z10k_lk_trackI7LkPlainEvNT_4ArgsE)
"""
import re
import sys


def body(path: str, name: str) -> str:
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
    out = []
    for l in lines[start + 1:]:
        if l.startswith(".Lfunc_end"):
            break
        l = l.split(";")[0].rstrip()
        if l.strip() and l.split()[0] not in (".text", ".section"):        # a template's code sits in a COMDAT section of its own
            out.append(l)
    txt = "\n".join(out).replace(name, "KERNEL")
    return re.sub(r"\.LBB\d+_", ".LBBk_", txt)


if __name__ == "__main__":
    print(body(sys.argv[1], sys.argv[2]))
