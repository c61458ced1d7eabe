#!/usr/bin/env python3
"""Are the kernels of two builds the same device code?  Both builds made with --save-temps
(make FLAGS='... --save-temps' in two copies of csrc/): for every translation unit the device assembly files are compared
kernel by kernel - the text from a kernel's label to its end label and its .amdhsa_kernel block -, sorted by name, because
the order in the file follows the order of instantiation.  The labels of basic blocks carry the function's number in the
file (.LBB12_3): that number is dropped on both sides, and so are the assembler's comments (they number the compiler's
temporaries through the whole file), the blanks in front of them and the lines they leave empty; no instruction, operand or directive is touched.

    tools/isa_identity.py PARENT_DIR BRANCH_DIR [--drop-arg KERNEL:N ...] [--retired REGEX ...]

--drop-arg pair_cull_kernel:4   the parent's template argument N (counted from 1) of KERNEL is deleted from its mangled names
                                before the comparison (a template parameter the branch removed);
--retired REGEX                 parent kernels whose (original) mangled name matches are expected to be absent from the branch.
Prints one line per translation unit and every difference; exit status 1 if anything differs."""
import glob
import os
import re
import sys

ARG = re.compile(r"L[a-z]n?\d+E")


def drop_arg(text, kernel, n):
    def fix(m):
        args = ARG.findall(m.group(2))
        assert "".join(args) == m.group(2), m.group(0)
        del args[n - 1]
        return m.group(1) + "".join(args) + "E"
    return re.sub(r"(\d+%sI)((?:L[a-z]n?\d+E)+)E" % re.escape(kernel), fix, text)


def kernels(path, drops, retired):
    """{name: (body, descriptor)} of one assembly file, and the names of the retired kernels (left out of the dict)"""
    text = open(path).read()
    text = re.sub(r"\.LBB\d+_", ".LBB_", text)
    text = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", text)
    text = re.sub(r"[ \t]*;.*$", "", text, flags=re.M)
    text = re.sub(r"\n+", "\n", text)
    out, gone = {}, set()
    for nm in re.findall(r"^\t\.amdhsa_kernel (\S+)$", text, re.M):
        if any(re.search(r, nm) for r in retired):      # (taken out BEFORE the renaming: a retired name may become a kept one)
            gone.add(nm)
            continue
        body = re.search(r"^%s:.*?^\.Lfunc_end:" % re.escape(nm), text, re.M | re.S).group(0)
        desc = re.search(r"^\t\.amdhsa_kernel %s$.*?^\t\.end_amdhsa_kernel$" % re.escape(nm), text, re.M | re.S).group(0)
        for kernel, n in drops:
            nm, body, desc = drop_arg(nm, kernel, n), drop_arg(body, kernel, n), drop_arg(desc, kernel, n)
        assert nm not in out, nm
        out[nm] = (body, desc)
    return out, gone


def figures(k):
    """instruction lines and the descriptor's registers, scratch and LDS of one kernel"""
    body, desc = k
    n = sum(1 for ln in body.split("\n") if ln.startswith("\t") and not ln.startswith("\t."))
    get = lambda key: re.search(r"\.amdhsa_%s (\S+)" % key, desc).group(1)
    return "%d instructions, %s VGPRs, %s SGPRs, %s B scratch, %s B LDS" % (
        n, get("next_free_vgpr"), get("next_free_sgpr"), get("private_segment_fixed_size"), get("group_segment_fixed_size"))


def main(argv):
    pos = [a for a in argv if not a.startswith("--")]
    drops, retired = [], []
    it = iter(argv)
    for a in it:
        if a == "--drop-arg":
            k, n = next(it).split(":")
            drops.append((k, int(n)))
            pos.remove("%s:%d" % (k, int(n)))
        elif a == "--retired":
            r = next(it)
            retired.append(r)
            pos.remove(r)
    parent, branch = pos
    bad = 0
    for pa in sorted(glob.glob(os.path.join(parent, "*-hip-amdgcn-amd-amdhsa-gfx950.s"))):
        unit = os.path.basename(pa).split("-hip-")[0]
        br = os.path.join(branch, os.path.basename(pa))
        if open(pa).read() == open(br).read():
            print("%-20s device assembly identical (whole file)" % unit)
            continue
        kp, gone = kernels(pa, drops, retired)
        kb, _ = kernels(br, [], [])
        kept = sorted(kp)
        print("%-20s parent %d kernels, retired %d, kept %d; branch %d kernels" % (unit, len(kp) + len(gone), len(gone), len(kept), len(kb)))
        for nm in sorted(gone):
            print("    retired  %s" % nm)
        for nm in sorted(set(kb) - set(kept)):
            print("    NEW IN THE BRANCH  %s" % nm)
            bad += 1
        same = 0
        for nm in kept:
            if nm not in kb:
                print("    MISSING FROM THE BRANCH  %s" % nm)
                bad += 1
            elif kp[nm] != kb[nm]:
                print("    DIFFERS  %s (%s)" % (nm, "code" if kp[nm][0] != kb[nm][0] else "descriptor"))
                print("             parent %s\n             branch %s" % (figures(kp[nm]), figures(kb[nm])))
                bad += 1
            else:
                same += 1
        print("    %d of %d kept kernels: code and descriptor identical" % (same, len(kept)))
    print("RESULT: %s" % ("identical" if bad == 0 else "%d differences" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
