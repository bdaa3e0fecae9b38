"""Did a change touch device code?  Per-kernel comparison of two directories of
`hipcc -S --cuda-device-only` output (one .s per translation unit, same file
names in both): the set of kernel symbols, and each kernel's instructions and
.amdhsa descriptor.  Compared per kernel with comments dropped and block labels
renumbered, so the order in which a unit instantiates its kernels does not matter.
usage: python tools/isa_kernels_cmp.py DIR_A DIR_B   (exit status 1 on a difference)"""
import hashlib
import os
import re
import sys


def kernels(path):
    """{symbol: (instructions, descriptor)} of one .s file."""
    lines = open(path).read().split("\n")
    exported = {m.group(1) for ln in lines for m in [re.match(r"\s*\.(?:globl|weak)\s+(\S+)", ln)] if m}
    body, desc = {}, {}
    cur, buf, dcur, dbuf = None, [], None, []
    for ln in lines:
        m = re.match(r"^(\w+):\s*(;.*)?$", ln)
        if m and cur is None and m.group(1) in exported:
            cur, buf = m.group(1), []
            continue
        if cur is not None:
            if re.match(r"^\.Lfunc_end\d+:", ln):
                body[cur] = "\n".join(buf)
                cur = None
                continue
            ln = re.sub(r"\s*;.*$", "", ln)  # comments name blocks by the function's number in the unit
            ln = re.sub(r"\.LBB\d+_", ".LBB_", ln)
            ln = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", ln)
            buf.append(re.sub(r"\.Ltmp\d+", ".Ltmp", ln))
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            dcur, dbuf = m.group(1), []
        elif dcur is not None and ".end_amdhsa_kernel" in ln:
            desc[dcur] = "\n".join(dbuf)
            dcur = None
        elif dcur is not None:
            dbuf.append(ln)
    return {k: (v, desc.get(k, "")) for k, v in body.items()}


def main(a, b):
    bad = 0
    for f in sorted(x for x in os.listdir(a) if x.endswith(".s")):
        ka, kb = kernels(os.path.join(a, f)), kernels(os.path.join(b, f))
        odd = sorted(set(ka) ^ set(kb)) + [k for k in ka if k in kb and ka[k] != kb[k]]
        sha = hashlib.sha256("".join(k + "".join(ka[k]) for k in sorted(ka)).encode()).hexdigest()[:12]
        print(f"{f}: {len(ka)} / {len(kb)} kernels, {sum(v[0].count(chr(10)) for v in ka.values())} lines, "
              f"missing or differing: {len(odd)}, sha256 of A {sha}")
        for k in odd:
            print("   ", k)
        bad += len(odd)
    print("IDENTICAL" if bad == 0 else f"{bad} DIFFERENCES")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
