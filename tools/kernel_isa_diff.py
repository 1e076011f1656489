"""Compare the kernels of two compilations, kernel by kernel: `python tools/kernel_isa_diff.py OLD.s [OLD2.s ...] -- NEW.s [NEW2.s ...]`.

For a refactor that moves or re-expresses device code and must leave every kernel's machine code alone.  The inputs are hipcc's
assembly listings (`hipcc -x hip <build.FLAGS> -S --cuda-device-only -o X.s X.hip`); the kernels of each side are pooled, so a
file may be split or merged between the two.  One line per kernel:

    same                 the .amdhsa_kernel descriptor block is equal verbatim, and so is the instruction text from the kernel's label
                         to its .Lfunc_end once `;` comments are dropped and the local .L labels are renumbered in order of appearance
                         (their numbers count the functions of the file before them)
    descriptor differs   registers, LDS, scratch, kernarg size ... changed (a changed body is not looked at then)
    code differs         same descriptor, other instructions
    only in OLD / NEW    the kernel is missing from one side

Exit status 0 only when every kernel is `same`.  It compares two compilations and nothing else: no opinion on what the code holds."""
import re
import subprocess
import sys


def kernels(paths):
    """{mangled name: (descriptor text, normalised body lines)} over the listings"""
    out = {}
    for path in paths:
        asm = open(path).read()
        for m in re.finditer(r"^[ \t]*\.amdhsa_kernel[ \t]+(\S+)\n(.*?)^[ \t]*\.end_amdhsa_kernel", asm, re.S | re.M):
            name, desc = m.group(1), m.group(2)
            body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), asm, re.S | re.M)
            if body is None:
                sys.exit("%s: no body for kernel %s" % (path, name))
            if name in out:
                sys.exit("%s: kernel %s appears twice on one side" % (path, name))
            labels = {}
            lines = []
            for line in body.group(1).split("\n"):
                line = line.split(";", 1)[0].strip()
                if line:
                    lines.append(re.sub(r"\.L\w+", lambda l: labels.setdefault(l.group(0), ".L%d" % len(labels)), line))
            out[name] = (desc, lines)
    return out


def demangled(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        short = [re.sub(r"\(anonymous namespace\)::|\(.*", "", s) for s in r.stdout.split("\n")[:len(names)]]
        return dict(zip(names, short))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main(argv):
    if "--" not in argv or argv[0] == "--" or argv[-1] == "--":
        sys.exit(__doc__)
    i = argv.index("--")
    old, new = kernels(argv[:i]), kernels(argv[i + 1:])
    names = sorted(set(old) | set(new))
    show = demangled(names)
    bad = 0
    for n in sorted(names, key=lambda n: show[n].replace("void ", "")):
        if n not in old or n not in new:
            verdict = "only in NEW" if n in new else "only in OLD"
        elif old[n][0] != new[n][0]:
            verdict = "descriptor differs"
        elif old[n][1] != new[n][1]:
            first = next((j for j, (a, b) in enumerate(zip(old[n][1], new[n][1])) if a != b), min(len(old[n][1]), len(new[n][1])))
            verdict = "code differs (%d / %d instructions and labels, first at %d)" % (len(old[n][1]), len(new[n][1]), first)
        else:
            verdict = "same"
        bad += verdict != "same"
        print("%-60s %s" % (show[n], verdict))
    print("%d kernels, %d not the same" % (len(names), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
