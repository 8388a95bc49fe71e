#!/usr/bin/env python3
"""Same row kernels before and after the SUM / BF16 / F16 / UNDO flags became one RowKind?  (profiles/r19/README.md)

Reads the gfx950 assembly of saf_fuse.hip, saf_window.hip and saf_brick.hip of two builds (hipcc -save-temps leaves
<unit>-hip-amdgcn-amd-amdhsa-gfx950.s beside the objects), pairs every row-kernel instantiation of the build that spells the
flags with the one of the build that spells the kind, and compares the instruction stream with the kernel descriptor behind it --
symbol names and the number a function's local labels carry replaced by placeholders, comments dropped, nothing else -- and the
resources the compiler reports.  Prints one markdown table row per instantiation of either build; exit status 1 if a pair differs
in code or resources, or a 176-register kernel reports more.

    python tools/rowkind_asm_table.py <csrc of the flags build> <csrc of the kinds build>
"""
import hashlib
import re
import subprocess
import sys

UNITS = ["saf_fuse", "saf_window", "saf_brick"]
KINDS = ["MeanF32", "SumF32", "MeanBf16", "SumBf16", "MeanF16", "UndoF32"]  # enum class RowKind, in order
ROW = re.compile(r"(fuse_rows_kernel|fuse_window_kernel(?:_of176)?(?:_f16)?|window_unfuse_kernel(?:_of176)?|fuse_brick_kernel)(?:<(.*?)>)?\(")
FIELDS = {"vgpr": "NumVgprs", "sgpr": "TotalNumSgprs", "lds": "LDSByteSize", "scratch": "ScratchSize"}


def kind_of(sum_, b16, f16="false", undo="false"):
    flags = (sum_ == "true", b16 == "true", f16 == "true", undo == "true")
    return {(False, False, False, False): "MeanF32", (True, False, False, False): "SumF32", (False, True, False, False): "MeanBf16",
            (True, True, False, False): "SumBf16", (False, True, True, False): "MeanF16", (False, False, False, True): "UndoF32"}[flags]


def key_of(name, args):
    """One spelling for both builds: 'kernel<numbers and bools..., Kind>'."""
    a = [x.strip() for x in args.split(",")] if args else []
    enum = [KINDS[int(x.rsplit(")", 1)[1])] if "RowKind" in x else None for x in a]
    if any(enum):  # the kinds build
        rest = [x for x, e in zip(a, enum) if not e]
        if name == "fuse_window_kernel_of176":
            rest = ["2"]
        return "%s<%s>" % (name, ", ".join(rest + [e for e in enum if e]))
    if name == "fuse_rows_kernel":
        return "%s<%s>" % (name, ", ".join(a[:4] + [kind_of(*a[4:])]))
    if name == "fuse_window_kernel":
        return "%s<%s>" % (name, ", ".join([a[0], a[3], kind_of(a[1], a[2])]))
    if name == "fuse_window_kernel_f16":
        return "fuse_window_kernel<%s, %s, MeanF16>" % (a[0], a[1])
    if name == "fuse_window_kernel_of176":
        return "%s<2, %s>" % (name, kind_of(a[1], a[2]))
    if name == "fuse_window_kernel_of176_f16":
        return "fuse_window_kernel_of176<2, MeanF16>"
    if name == "fuse_brick_kernel":
        return "%s<%s>" % (name, ", ".join([a[0], a[3], a[4], kind_of(a[1], a[2])]))
    return "%s<%s>" % (name, ", ".join(a)) if a else name  # window_unfuse_kernel<CPL>, window_unfuse_kernel_of176


def kernels(csrc):
    out = {}
    for unit in UNITS:
        text = open("%s/%s-hip-amdgcn-amd-amdhsa-gfx950.s" % (csrc, unit)).read()
        syms = re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M)
        names = subprocess.run(["c++filt"] + syms, capture_output=True, text=True, check=True).stdout.split("\n")
        for sym, dem in zip(syms, names):
            m = ROW.search(dem)
            if not m:
                continue
            body = text[text.index("\n%s:" % sym):]
            end = re.search(r"^\.Lfunc_end\d+:", body, re.M).start()
            tail = body[end:body.index("; Occupancy:", end)]  # the "; Kernel info:" comments behind the function
            code = re.sub(r"_Z\w+", "SYM", body[:end])
            code = re.sub(r"\.LBB\d+_", ".LBB_", code)
            code = "\n".join(l for l in (l.split(";")[0].rstrip() for l in code.split("\n")) if l)  # (no string in these holds a ';')
            key = key_of(m.group(1), m.group(2))
            res = {f: int(re.search(r"; %s: (\d+)" % tag, tail).group(1)) for f, tag in FIELDS.items()}
            assert key not in out, key
            out[key] = dict(res, lines=code.count("\n") + 1, sha=hashlib.sha256(code.encode()).hexdigest()[:12])
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    print("| kernel | instructions + labels | stream | VGPRs | SGPRs | LDS bytes | scratch bytes |")
    print("|---|---|---|---|---|---|---|")
    for k in sorted(set(a) | set(b)):
        x, y = a.get(k), b.get(k)
        if x is None or y is None:
            print("| `%s` | %s | only in the %s build | | | | |" % (k, (x or y)["lines"], "flags" if x else "kinds"))
            continue
        same = x["sha"] == y["sha"]
        res = [("%d" % x[f]) if x[f] == y[f] else ("%d -> %d" % (x[f], y[f])) for f in FIELDS]
        bad += (not same) or any(x[f] != y[f] for f in FIELDS)
        print("| `%s` | %d | %s | %s |" % (k, x["lines"], "identical" if same else "DIFFERS (%d lines)" % y["lines"], " | ".join(res)))
    for k, y in b.items():
        if "of176" in k and y["vgpr"] > 176:
            bad += 1
            print("`%s`: %d VGPRs" % (k, y["vgpr"]))
    print("\n%d row-kernel instantiations in the flags build, %d in the kinds build, %d in both" % (len(a), len(b), len(set(a) & set(b))))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
