"""What each block decode of the 12-bit GEMV forms without a prologue waits for, from hipcc's gfx950 assembly
(profiles/w12b_isa.txt).

    hipcc -O3 --offload-arch=gfx950 <the build's flags> --cuda-device-only -S csrc/gemm_gemv.hip -o gemv.s
    python scripts/tune/w12b_isa.py LABEL gemv.s

The straight-line PG_W_FRAG12 forms that read x from memory (gemv_hot_kernel<EPI, NT, 2, DEPTH, PRO 0 | 4, 3, CPW>: down,
the finalising down, the lm_head) are meant to issue every vector load outside the decode's branches, so the text order
of the loads is their issue order, and `s_waitcnt vmcnt(N)` lets the N youngest loads stay in flight: after k loads it
waits for the oldest k - N.  The kernel's text is cut at every fourth MFMA (one tile of one block).  In each piece,
everything in front of the piece's first branch runs whatever the block is; of the basic blocks behind it, those that
hold the fifth-bit mask 0x8000800, and those that load, belong to the wide decodes.  Per piece:
  k        vector loads in the text up to the piece's first MFMA
  narrow   the smallest N the narrow path has waited for by then, and k - N
  wide     the smallest N of the wide decodes, and k - N
  +s       vector loads issued INSIDE the branches (a fifth-plane load the compiler sank to its only reader: the
           kernel's youngest load, a full round trip in front of that decode, and the wait behind it is vmcnt(0))
The lm_head (PRO 4) loads its sums of squares in wave 0 only, in one of three branches (4 + 8 + 8 loads in the text): k
counts the 4 that M <= 2 issues.  The compiler's N allows for the longest branch, so for the lm_head k - N is a lower
bound of what the wait covers, short by at most 4.
"""
import re
import sys

from karg_isa import kernels, short_name

WANT = re.compile(r"gemv_hot_kernel<\d+,[12],2,\d+,[04],3,[48]>")
VEC = re.compile(r"^\t(global_load|buffer_load|flat_load)")
WIDE = "0x8000800"


def real_entry(lines):
    for i, l in enumerate(lines[:40]):
        if ".p2align\t8" in l or ".p2align 8" in l:
            return i + 1
    return 0


def pieces(lines):
    """[[basic block = list of lines]] -- one list per four MFMAs; a block ends with a branch or in front of a label"""
    out, blocks, cur, nm = [], [], [], 0
    for l in lines[real_entry(lines):]:
        if re.match(r"^\.LBB", l):
            blocks.append(cur)
            cur = []
        cur.append(l)
        if l.startswith("\ts_cbranch") or l.startswith("\ts_branch"):
            blocks.append(cur)
            cur = []
        if l.startswith("\tv_mfma"):
            nm += 1
            if nm % 4 == 0:
                blocks.append(cur)
                out.append(blocks)
                blocks, cur = [], []
    return out


def analyse(lines, pro):
    rows, issued, first = [], 0, True
    for blocks in pieces(lines):
        n = {"narrow": None, "wide": None}
        sunk, branched, k = 0, False, None
        for b in blocks:
            loads = sum(bool(VEC.match(l)) for l in b)
            mask = any(WIDE in l for l in b)
            # the kernel's first piece also holds the fill and, in the lm_head, wave 0's sums-of-squares loads in three
            # branches: the 4 of M <= 2 are counted as issued, the 8 + 8 of the M > 2 branches are not
            sums = first and pro == 4 and branched and not mask and loads >= 4
            if sums and loads >= 8:
                continue
            kind = "wide" if branched and not sums and (loads or mask) else "narrow"
            for l in b:
                if l.startswith("\tv_mfma") and k is None:
                    k = issued
                if VEC.match(l):
                    issued += 1
                    if k is None:
                        sunk += kind == "wide"
                        if kind == "narrow":
                            n["narrow"] = None    # (a wait in front of a load of the fill is the fill's own: the table words)
                m = re.match(r"^\ts_waitcnt.*vmcnt\((\d+)\)", l)
                if m and k is None and not sums:
                    v = int(m.group(1))
                    n[kind] = v if n[kind] is None else min(n[kind], v)
                if l.startswith("\ts_cbranch"):
                    branched = True
        rows.append((k, n["narrow"], n["wide"], sunk))
        first = False
    return rows


def main():
    label, path = sys.argv[1], sys.argv[2]
    print(f"# {label}")
    print("# kernel | per block (b) and tile (t): k: narrow N (k - N) / wide N (k - N) [+s sunk loads]; "
          "- = no further wait on that path")
    ks = kernels(path)
    for name in sorted(ks):
        short = short_name(name)
        if not WANT.fullmatch(short):
            continue
        a = short.split("<")[1].rstrip(">").split(",")
        nt, pro = int(a[1]), int(a[4])
        cells = []
        for i, (k, n, w, s) in enumerate(analyse(ks[name][0], pro)):
            f = lambda v: "-" if v is None else f"{v} ({k - v})"
            cells.append(f"b{i // nt}" + (f"t{i % nt}" if nt > 1 else "") + f" {k}: {f(n)} / {f(w)}" + (f" +{s}" if s else ""))
        print(f"{short} | " + " | ".join(cells))


if __name__ == "__main__":
    main()
