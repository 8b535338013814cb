#!/usr/bin/env python3
"""Static instruction counts of conv3x3_wino_kernel's prologue and epilogue, from the compiler's assembly (documentation only:
docs/rounds/r07.md).  No device needed.

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off --cuda-device-only -S multipathnet_amd/csrc/dense.hip -o dense.s
  python tools/wino_epilogue_count.py dense.s

For each production instantiation (ABL = 0, TC = 8 / 16): the instructions before the first MFMA and after the last one, grouped
by mnemonic family, and the kernel's private segment / spill figures from its metadata block."""
import collections
import re
import sys

FAMILIES = [("accvgpr_read", r"v_accvgpr_read"), ("accvgpr_write", r"v_accvgpr_write"), ("pk_add", r"v_pk_add_f32"),
            ("max3", r"v_max3_f32"), ("max", r"v_max_f32"), ("cndmask", r"v_cndmask"), ("other valu", r"v_"),
            ("store", r"(global|flat|scratch|buffer)_store"), ("load", r"(global|flat|scratch|buffer|s)_load"),
            ("saveexec/exec", r"s_(and|or|xor|andn2)_saveexec|s_(or|and|andn2|mov)_b64 exec"), ("branch", r"s_cbranch|s_branch"),
            ("waitcnt/nop", r"s_waitcnt|s_nop"), ("other scalar", r"s_"), ("lds", r"ds_")]


def family(mn):
    for name, pat in FAMILIES:
        if re.match(pat, mn):
            return name
    return "other"


def kernels(path):
    name, body, out = None, [], {}
    for line in open(path):
        m = re.match(r"^(_ZN3mpn19conv3x3_wino_kernelILi0ELi(\d+)EEEvNS_8ConvArgsE):", line)
        if m:
            name, body = "TC=%s" % m.group(2), []
            continue
        if name is None:
            continue
        if line.startswith("\t.amdhsa_kernel") or line.startswith(".Lfunc_end"):
            out.setdefault(name, {})["body"] = body
            body = []
        s = line.strip()
        for key in (".amdhsa_private_segment_fixed_size", "; ScratchSize:", "; NumVgprs:", "; NumAgprs:", "; codeLenInByte"):
            if s.startswith(key):
                out.setdefault(name, {}).setdefault("meta", []).append(s)
        if s.startswith(".end_amdhsa_kernel"):
            name = None
            continue
        if s and not s.startswith((";", ".", "//")) and not s.endswith(":"):
            body.append(s.split()[0])
    return out


def main():
    for name, k in sorted(kernels(sys.argv[1]).items()):
        body = k["body"]
        mf = [i for i, mn in enumerate(body) if mn.startswith("v_mfma")]
        print("== conv3x3_wino_kernel<0, %s>: %d instructions, %d MFMA" % (name[3:], len(body), len(mf)))
        for m in k.get("meta", []):
            print("   " + m)
        for what, part in (("prologue (before the first MFMA)", body[:mf[0]]), ("epilogue (after the last MFMA)", body[mf[-1] + 1:])):
            c = collections.Counter(family(mn) for mn in part)
            print("   %s: %d" % (what, len(part)))
            print("      " + ", ".join("%s %d" % kv for kv in c.most_common()))


if __name__ == "__main__":
    main()
