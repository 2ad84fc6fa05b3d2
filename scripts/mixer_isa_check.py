"""Compare the f32 fused-mixer kernels of two gfx950 assembly listings of csrc/macjd_mixer.hip.

    hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -std=c++17 --cuda-device-only -S -o before.s macjd_mixer.hip
    python scripts/mixer_isa_check.py before.s after.s

`after.s` is from a tree with the operand-type template parameter (the last template argument of every mixer kernel);
its instantiations with that argument false are matched to the kernel of the same name in `before.s` without it.  Each
body is normalised (symbol names, basic-block / temporary label numbers) and hashed together with its kernel descriptor
(.amdhsa_kernel: registers, LDS, scratch).  Prints one line per kernel and exits non-zero when any differs."""
import hashlib
import re
import sys


def kernels(path):
    txt = open(path).read()
    body = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\S*mixer\S*):[^\n]*$(.*?)^\.Lfunc_end\d+:", txt, re.M | re.S)}
    desc = {m.group(1): m.group(2) for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)$(.*?)\.end_amdhsa_kernel", txt, re.M | re.S)}
    return body, desc


def digest(body, desc):
    b = re.sub(r"\.?LBB\d+_|BB\d+_", "BB_", body)
    b = re.sub(r"\.Ltmp\d+", ".Ltmp", b)
    b = re.sub(r"_Z\S+", "SYM", b)
    return hashlib.sha256((b + "\n--\n" + desc).encode()).hexdigest()[:16]


def main(before, after):
    bb, bd = kernels(before)
    ab, ad = kernels(after)
    bad = 0
    for name in sorted(ab):
        m = re.match(r"(.*)Lb([01])E(EEv.*|Ev.*)$", name)
        if not m or m.group(2) == "1":
            continue
        old = m.group(1) + m.group(3)
        h_old = digest(bb[old], bd[old]) if old in bb else "missing"
        h_new = digest(ab[name], ad[name])
        same = h_old == h_new
        bad += not same
        print(f"{'same' if same else 'DIFF'}  {h_old}  {h_new}  {old}")
    print(f"{len(bb)} mixer kernels before; {sum(1 for n in ab if re.search(r'Lb0E(EEv|Ev)', n))} f32 instantiations after; "
          f"{bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
