"""Compare the env-step kernels of two gfx950 assembly listings of csrc/macjd_env.hip.

    hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -std=c++17 --cuda-device-only -S -o before.s macjd_env.hip
    python scripts/env_isa_check.py before.s after.s

Kernels are matched by name.  When `before.s` is from a tree without the SCAN template parameter (the last template
argument of env_step_kernel), the instantiations of `after.s` with that argument false are matched to the kernel of the
same name in `before.s` without it.  Each body is normalised (symbol names, basic-block / temporary / long-branch label numbers) and hashed together with
its kernel descriptor (.amdhsa_kernel: registers, LDS, scratch); instruction count, VGPRs and scratch bytes are printed
next to the hashes.  Exits non-zero when any existing kernel differs."""
import hashlib
import re
import sys


def kernels(path):
    txt = open(path).read()
    body = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\S*macjd\S*):[^\n]*$(.*?)^\.Lfunc_end\d+:", txt, re.M | re.S)}
    desc = {m.group(1): m.group(2) for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)$(.*?)\.end_amdhsa_kernel", txt, re.M | re.S)}
    return body, desc


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
    bb, bd = kernels(before)
    ab, ad = kernels(after)
    bad = n_old = n_scan = 0
    for name in sorted(ab):
        if "desc" in name:
            continue
        # (a kernel of the same name in both listings is matched by name: both trees have the SCAN parameter)
        m = None if name in bb else re.match(r"(_ZN5macjd15env_step_kernel.*)Lb([01])E(EEv.*)$", name)
        if m and m.group(2) == "1":
            n_scan += 1
            print(f"scan  {stats(ab[name], ad[name])}  {name}")
            continue
        old = m.group(1) + m.group(3) if m else name
        if old not in bb:
            print(f"new   {stats(ab[name], ad[name])}  {name}")
            continue
        n_old += 1
        h_old = digest(bb[old], bd[old])
        h_new = digest(ab[name], ad[name])
        same = h_old == h_new
        bad += not same
        s_old = stats(bb[old], bd[old])
        print(f"{'same' if same else 'DIFF'}  {h_old}  {h_new}  {s_old} -> {stats(ab[name], ad[name])}  {old}")
    print(f"{len(bb)} kernels before; {n_old} matched after ({bad} differ); {n_scan} SCAN instantiations added")
    return 1 if bad or n_old != len(bb) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
