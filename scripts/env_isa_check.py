"""Compare the kernels of two gfx950 assembly listings of one source file (csrc/macjd_env.hip, csrc/macjd_episode.hip).

    hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -std=c++17 --cuda-device-only -S -o before.s macjd_env.hip
    python scripts/env_isa_check.py before.s after.s

Each body is normalised (symbol names, basic-block / temporary / long-branch label numbers) and hashed together with
its kernel descriptor (.amdhsa_kernel: registers, LDS, scratch); instruction count, VGPRs and scratch bytes are printed
next to the hashes.  A kernel whose name is in both listings is matched by name.  The kernels whose names are in one
listing only (a changed template parameter list changes the name) are paired by digest and reported as `same (renamed)`
with both names; what is left over is `DIFF` (a kernel of `before.s` without a counterpart of its digest) or `new`.
Exits non-zero when any kernel of `before.s` has no counterpart with the same digest, or the two listings differ in
their number of kernels."""
import hashlib
import re
import sys


def kernels(path):
    txt = open(path).read()
    body = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\S*macjd\S*):[^\n]*$(.*?)^\.Lfunc_end\d+:", txt, re.M | re.S)}
    desc = {m.group(1): m.group(2) for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)$(.*?)\.end_amdhsa_kernel", txt, re.M | re.S)}
    return {n: (b, desc[n]) for n, b in body.items() if "desc" not in n}


def digest(body, desc):
    b = re.sub(r"\.?LBB\d+_|BB\d+_", "BB_", body)
    b = re.sub(r"\.Ltmp\d+", ".Ltmp", b)
    b = re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", b)   # long-branch labels: numbered per module, like the blocks
    b = re.sub(r"_Z\S+", "SYM", b)
    b = re.sub(r"[ \t]*;[^\n]*", "", b)   # assembler comments (their padding follows the label numbers)
    return hashlib.sha256((b + "\n--\n" + desc).encode()).hexdigest()[:16]


def stats(body, desc):
    n = sum(1 for ln in body.splitlines() if re.match(r"^\s+[sv]_|^\s+(global|buffer|ds|flat|scratch)_", ln))
    vg = re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc)
    sc = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc)
    return f"insts={n} vgpr={vg.group(1) if vg else '?'} scratch={sc.group(1) if sc else '?'}"


def main(before, after):
    bk, ak = kernels(before), kernels(after)
    bad = 0
    for name in sorted(set(bk) & set(ak)):
        h_old, h_new = digest(*bk[name]), digest(*ak[name])
        bad += h_old != h_new
        print(f"{'same' if h_old == h_new else 'DIFF'}  {h_old}  {h_new}  {stats(*bk[name])} -> {stats(*ak[name])}  {name}")
    # names on one side only: pair by digest
    unpaired = {}
    for name in sorted(set(ak) - set(bk)):
        unpaired.setdefault(digest(*ak[name]), []).append(name)
    n_renamed = 0
    for old in sorted(set(bk) - set(ak)):
        h = digest(*bk[old])
        if unpaired.get(h):
            new = unpaired[h].pop(0)
            n_renamed += 1
            print(f"same (renamed)  {h}  {h}  {stats(*bk[old])} -> {stats(*ak[new])}  {old} -> {new}")
        else:
            bad += 1
            print(f"DIFF  {h}  {'-' * 16}  {stats(*bk[old])} -> (no kernel with this digest)  {old}")
    n_new = 0
    for h, names in sorted(unpaired.items()):
        for name in names:
            n_new += 1
            print(f"new   {'-' * 16}  {h}  {stats(*ak[name])}  {name}")
    print(f"{len(bk)} kernels before, {len(ak)} after; {len(bk) - bad} of before's have a counterpart of the same digest "
          f"({n_renamed} renamed), {bad} do not; {n_new} new")
    return 1 if bad or len(bk) != len(ak) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
