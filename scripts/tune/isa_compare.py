"""Per-kernel comparison of two hipcc gfx950 assembly files of one source (profiles/attn_refactor_isa.txt,
profiles/gemm_refactor_isa.txt).

    hipcc -O3 --offload-arch=gfx950 <the build's flags of pghip/build.py, with its preload flags for the sources that
          take them> --cuda-device-only -S csrc/SOURCE.hip -o SOURCE.s                                (both trees)
    python scripts/tune/isa_compare.py parent/SOURCE.s new/SOURCE.s [--allow REGEX] [--rename REGEX REPL]

For a refactor that removes kernel instances, whole-text comparison fails on the renumbered function-indexed local
labels alone.  This compares, per kernel symbol: the symbol sets, each body (label line to the end of the function's
text, the function index in local labels dropped) and each .amdhsa_kernel descriptor block.  It reports set and text
differences only and looks at no instruction.  For a kernel that differs it prints the body line counts and the
descriptor lines that differ (the register counts are there).  Exit status 1 if a kernel outside --allow (a regex on
the demangled-ish short name) differs or a symbol was added.

--rename REGEX REPL: a refactor that drops a template parameter renames every instance of that kernel.  The parent's
mangled symbols are rewritten with re.sub(REGEX, REPL) before the sets are compared, so such an instance is compared
with its successor instead of being counted once as removed and once as added; the renamed count is printed.
"""
import hashlib
import re
import sys


def short_name(mangled):
    """_Z11attn_kernelILi32ELi1ELb0EEv8AttnArgs -> attn_kernel<32,1,0>"""
    m = re.match(r"_Z(\d+)", mangled)
    if not m:
        return mangled
    n = int(m.group(1))
    name, rest = mangled[m.end():m.end() + n], mangled[m.end() + n:]
    args = []
    if rest.startswith("I"):
        for a in re.finditer(r"L([ib])(n?)(\d+)E", rest.split("EEv")[0] + "E"):
            args.append(("-" if a.group(2) else "") + a.group(3))
    return name + ("<" + ",".join(args) + ">" if args else "")


LOCAL = re.compile(r"\.L([A-Za-z_]+?)(\d+)(_\d+)?\b")


def norm(line):
    # .LBB20_3 -> .LBB_3, .Lfunc_end20 -> .Lfunc_end: the function's index in the file, not its code; the assembler's
    # comments (loop headers named by that index, padded to a column) are dropped
    line = re.sub(r"\s*;.*$", "", line.rstrip("\n"))
    return LOCAL.sub(lambda m: ".L" + m.group(1) + (m.group(3) or ""), line) + "\n"


def kernels(path):
    """symbol -> (body lines, descriptor lines), for the symbols that have a descriptor (the kernels)"""
    body, desc, cur, dcur = {}, {}, None, None
    with open(path) as f:
        for line in f:
            if "__hip_cuid_" in line:
                continue
            m = re.match(r"^(\w+):", line)
            if m and dcur is None and not line.startswith(".L"):
                cur = m.group(1)
                body[cur] = []
                continue
            if line.startswith("\t.amdhsa_kernel "):
                dcur = line.split()[1]
                desc[dcur] = []
                continue
            if line.startswith("\t.end_amdhsa_kernel"):
                dcur = None
                continue
            if dcur is not None:
                desc[dcur].append(line)
            elif cur is not None:
                if line.startswith("\t.section") or line.startswith(".Lfunc_end"):
                    cur = None
                elif norm(line).strip():
                    body[cur].append(norm(line))
    return {k: (body[k], desc[k]) for k in desc}


def sha(lines):
    return hashlib.sha256("".join(lines).encode()).hexdigest()


def main():
    args = sys.argv[1:]
    allow = None
    if "--allow" in args:
        i = args.index("--allow")
        allow = re.compile(args[i + 1])
        del args[i:i + 2]
    rename = None
    if "--rename" in args:
        i = args.index("--rename")
        rename = (re.compile(args[i + 1]), args[i + 2])
        del args[i:i + 3]
    old, new = kernels(args[0]), kernels(args[1])
    if rename:
        n = len(old)
        renamed = {rename[0].sub(rename[1], k): v for k, v in old.items()}
        assert len(renamed) == n, "--rename maps two parent symbols onto one"
        print(f"renamed {sum(k not in old for k in renamed)} parent symbols: s/{rename[0].pattern}/{rename[1]}/")
        old = renamed
    gone, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    both = sorted(set(old) & set(new))
    print(f"kernels: {len(old)} -> {len(new)}; removed {len(gone)}, added {len(added)}, in both {len(both)}")
    for k in gone:
        print(f"  removed  {short_name(k)}")
    for k in added:
        print(f"  ADDED    {short_name(k)}")
    nb = nd = bad = 0
    for k in both:
        (b0, d0), (b1, d1) = old[k], new[k]
        if b0 == b1 and d0 == d1:
            continue
        nb += b0 != b1
        nd += d0 != d1
        ok = allow is not None and allow.search(short_name(k)) is not None
        bad += not ok
        print(f"  {'differs (allowed)' if ok else 'DIFFERS'}  {short_name(k)}  {k}: body {len(b0)} -> {len(b1)} lines")
        for x, y in zip(d0, d1):
            if x != y:
                print(f"      {x.strip()}  ->  {y.strip().split()[-1]}")
    print(f"bodies that differ: {nb} of {len(both)}; descriptor blocks that differ: {nd} of {len(both)}")
    same = [k for k in both if old[k] == new[k]]
    print(f"sha256 over the {len(same)} identical kernels (bodies and descriptors, sorted by symbol): "
          f"{sha([l for k in same for l in new[k][0] + new[k][1]])}")
    return 1 if bad or added else 0


if __name__ == "__main__":
    sys.exit(main())
