"""Show that kernels both trees have compile to the same gfx950 code, from two assembly listings of one source file.

    hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -std=c++17 --cuda-device-only -S -o before.s csrc/macjd_wgrad.hip
    (the same in the other tree -> after.s)
    python scripts/kernel_isa_check.py before.s after.s

Every kernel of `before.s` is looked up by its mangled name in `after.s`.  A body is normalised (basic-block and
temporary label numbers, symbol names) and hashed together with its kernel descriptor (.amdhsa_kernel: registers, LDS,
scratch) — the normalisation of scripts/mixer_isa_check.py, for any file.  Prints one line per kernel of `before.s`, then
the kernels only `after.s` has with their scratch size, and exits non-zero when a shared kernel differs, one is missing
or a new one uses scratch."""
import hashlib
import re
import sys


def kernels(path):
    txt = open(path).read()
    desc = {m.group(1): m.group(2) for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)$(.*?)\.end_amdhsa_kernel", txt, re.M | re.S)}
    body = {}
    for name in desc:
        m = re.search(r"^" + re.escape(name) + r":[^\n]*$(.*?)^\.Lfunc_end\d+:", txt, re.M | re.S)
        body[name] = m.group(1)
    return body, desc


def digest(body, desc):
    b = re.sub(r"\.?LBB\d+_|BB\d+_", "BB_", body)
    b = re.sub(r"\.Ltmp\d+", ".Ltmp", b)
    b = re.sub(r"_Z\S+", "SYM", b)
    return hashlib.sha256((b + "\n--\n" + desc).encode()).hexdigest()[:16]


def scratch(desc):
    m = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc)
    return int(m.group(1)) if m else -1


def main(before, after):
    bb, bd = kernels(before)
    ab, ad = kernels(after)
    bad = 0
    for name in sorted(bb):
        h_old = digest(bb[name], bd[name])
        h_new = digest(ab[name], ad[name]) if name in ab else "missing"
        bad += h_old != h_new
        print(f"{'same' if h_old == h_new else 'DIFF'}  {h_old}  {h_new}  {name}")
    for name in sorted(set(ab) - set(bb)):
        bad += scratch(ad[name]) != 0
        print(f"new   scratch {scratch(ad[name])} bytes  {name}")
    print(f"{len(bb)} kernels before, {len(ab)} after; {bad} differ, are missing or use scratch")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
