"""Entry-code counts of the batch-1 decode kernels from hipcc's gfx950 assembly (profiles/karg_isa.txt).

    hipcc -O3 --offload-arch=gfx950 <the build's flags> --cuda-device-only -S csrc/gemm_gemv.hip -o gemv.s
    python scripts/tune/karg_isa.py LABEL gemv.s attn.s misc.s [--only REGEX]

Per kernel: the kernarg preload length (dwords the firmware puts into SGPRs before the wave starts), then, counted
from the kernel's real entry (behind the compatibility prologue that a preloading kernel carries for firmware that
does not preload):
  pre_sload / pre_wait   scalar loads and `s_waitcnt lgkmcnt(0)` in front of the first vector memory load
  post_sload / post_wait scalar loads behind it, and the lgkmcnt(0) waits behind it that retire a scalar load (a wait
                         with no scalar load issued since the previous one only drains LDS traffic and is not counted)
  first_post_wait        vector memory loads issued before the first such wait (the ring's first fill is in front of it
                         when this is at least the ring's load count)
"""
import re
import sys

WANT = r"gemv_(hot_)?kernel|attn_decode_(hot_)?kernel|argmax_partial_kernel|argmax_final_embed_kernel"


def short_name(mangled):
    """_Z11gemv_kernelILi2ELi2E...EEv... -> gemv_kernel<2,2,...> (the integer / bool template arguments only)"""
    m = re.match(r"_Z(\d+)", mangled)
    n = int(m.group(1))
    name, rest = mangled[m.end():m.end() + n], mangled[m.end() + n:]
    args = []
    if rest.startswith("I"):
        for a in re.finditer(r"L([ib])(n?)(\d+)E", rest.split("EEv")[0] + "E"):
            args.append(("-" if a.group(2) else "") + a.group(3))
    return name + ("<" + ",".join(args) + ">" if args else "")


def kernels(path):
    """name -> (body lines, preload length)"""
    body, pre, cur = {}, {}, None
    desc = None
    with open(path) as f:
        for line in f:
            m = re.match(r"^(_Z\w+):", line)
            if m:
                cur = m.group(1)
                body[cur] = []
                continue
            if line.startswith("\t.amdhsa_kernel "):
                desc = line.split()[1]
                cur = None
                continue
            if desc and ".amdhsa_user_sgpr_kernarg_preload_length" in line:
                pre[desc] = int(line.split()[-1])
            if line.startswith("\t.end_amdhsa_kernel"):
                desc = None
            if cur is not None:
                body[cur].append(line)
            if line.startswith(".Lfunc_end"):
                cur = None
    return {k: (v, pre.get(k, 0)) for k, v in body.items() if k in pre}


def counts(lines):
    # the real entry: behind `.p2align 8` when the function opens with the compatibility prologue
    start = 0
    for i, l in enumerate(lines[:40]):
        if ".p2align\t8" in l or ".p2align 8" in l:
            start = i + 1
            break
    vec = re.compile(r"^\t(global_load|buffer_load|flat_load)")
    pre_s = pre_w = post_s = post_w = nvec = 0
    first_post = None
    pending = False
    seen = False
    for l in lines[start:]:
        if vec.match(l):
            seen = True
            nvec += 1
        elif l.startswith("\ts_load") or l.startswith("\ts_buffer_load"):
            pending = True
            if seen:
                post_s += 1
            else:
                pre_s += 1
        elif l.startswith("\ts_waitcnt") and "lgkmcnt(0)" in l:
            if not seen:
                pre_w += 1
            elif pending:
                post_w += 1
                if first_post is None:
                    first_post = nvec
            pending = False
    return pre_s, pre_w, post_s, post_w, first_post


def main():
    args = sys.argv[1:]
    only = None
    if "--only" in args:
        i = args.index("--only")
        only = re.compile(args[i + 1])
        del args[i:i + 2]
    label, files = args[0], args[1:]
    print(f"# {label}: preload dwords | pre_sload pre_wait | post_sload post_wait first_post_wait | kernel")
    for path in files:
        ks = kernels(path)
        names = sorted(ks)
        for name in names:
            short = short_name(name)
            if not re.search(WANT, short) or (only and not only.search(short)):
                continue
            body, pre = ks[name]
            a, b, c, d, e = counts(body)
            print(f"{pre:2d} | {a:2d} {b:2d} | {c:2d} {d:2d} {'-' if e is None else e:>3} | {short}")


if __name__ == "__main__":
    main()
