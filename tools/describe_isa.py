#!/usr/bin/env python3
"""The gfx950 listing of orient_describe8_kernel, read on a machine without a GPU: tools/describe_isa.py [-D...] [--dump FILE] [--asm LISTING]

Compiles describe_kernels.hip to assembly with the Makefile's flags (or reads a listing made that way, --asm), cuts the kernel out and reports, as one JSON line,
  * the register budget (VGPRs, SGPRs, scratch bytes),
  * its two per-keypoint loops (the innermost loops that request windows: phase 1, the moments, and phase 3, BRIEF): the static
    instruction count, and the EXECUTED PATH of one full iteration, taken as the longest way through the loop body from its header
    back to it (every conditional branch is followed both ways, loop exits are not; `s_cbranch_execz` around a store falls through,
    the wide window's third load round is on the way) with its split into vector, scalar, LDS and memory instructions,
  * what must not be in the loops: scalar loads, waits for them,
  * every write of M0 outside an inline-asm block (the LDS-DMA statements write M0 and do not restore it: the compiler must not keep
    anything there).
The count needs no knowledge of the source, so the same count can be made of any build: it is the figure
profiles/r07_describe.md quotes for the parent and for this kernel.
"""
import json, os, re, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "refactored_orb_slam2_amd", "csrc")
FLAGS = ["-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950",
         "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-gpu-rdc", "--cuda-device-only", "-S"]
KERNEL = "_Z23orient_describe8_kernel14DescribeParams"


def listing(extra=()):
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    r = subprocess.run([hipcc] + FLAGS + list(extra) + ["describe_kernels.hip", "-o", "-"], capture_output=True, text=True, cwd=CSRC, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    return r.stdout


def kernel_text(asm):
    a = asm.index(KERNEL + ":")
    b = asm.index(".amdhsa_kernel " + KERNEL)
    return asm[a:b], asm[b:]


def parse(body):
    """-> list of (kind, text, in_asm): kind 'label' | 'inst'"""
    out, in_asm = [], False
    for line in body.splitlines():
        t = line.strip()
        if t.startswith(";;#ASMSTART"):
            in_asm = True
            continue
        if t.startswith(";;#ASMEND"):
            in_asm = False
            continue
        t = t.split(";")[0].strip()
        if not t:
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", t)
        if m:
            out.append(("label", m.group(1), False))
        elif not t.startswith(".") and not t.endswith(":"):
            out.append(("inst", t, in_asm))
    return out


def loop_span(body, header):
    """all line indices of `body` (parsed items) that the compiler marks as part of the loop of `header`"""
    short = header.replace(".L", "")
    items, idx, cur_in = [], [], False
    in_asm = False
    for line in body.splitlines():
        t = line.strip()
        if t.startswith(";;#ASMSTART"):
            in_asm = True
            continue
        if t.startswith(";;#ASMEND"):
            in_asm = False
            continue
        m = re.match(r"^(\.LBB\d+_\d+):(.*)$", t)
        if m:
            cur_in = m.group(1) == header or ("Header=" + short + " ") in m.group(2) + " "
            items.append(("label", m.group(1), False, cur_in))
            continue
        if t.startswith("; %bb."):
            cur_in = ("Header=" + short + " ") in t + " "
            continue
        c = t.split(";")[0].strip()
        if not c or c.startswith(".") or c.endswith(":"):
            continue
        items.append(("inst", c, in_asm, cur_in))
    return items


def longest_path(items, header):
    """Instructions on the longest way through the loop body from `header` back to it (exits are not followed) -> (count, per class)."""
    sys.setrecursionlimit(20000)
    pos = {it[1]: i for i, it in enumerate(items) if it[0] == "label"}
    memo = {}

    def cls(op):
        return ("salu" if op.startswith("s_") else "lds" if op.startswith("ds_") else
                "vmem" if op.startswith(("global_", "flat_", "buffer_")) else "valu")

    def best(i, first=False):
        # -> (count, classes) of the longest way from item i to the header, None if every way from i leaves the loop
        while i < len(items) and items[i][0] == "label":
            if items[i][1] == header and not first:
                return (0, {})
            first = False
            i += 1
        if i >= len(items) or not items[i][3]:
            return None
        if i in memo:
            return memo[i]
        t = items[i][1]
        op = t.split()[0]
        nxt = []
        if op == "s_branch":
            nxt = [pos[t.split()[1]]]
        elif op.startswith("s_cbranch"):
            nxt = [pos[t.split()[1]], i + 1]
        elif op != "s_endpgm":
            nxt = [i + 1]
        cands = [r for r in (best(j) for j in nxt) if r is not None]
        if not cands:
            memo[i] = None
            return None
        c, k = max(cands, key=lambda r: r[0])
        k = dict(k)
        k[cls(op)] = k.get(cls(op), 0) + 1
        memo[i] = (c + 1, k)
        return memo[i]

    return best(pos[header], first=True)


def report(extra=(), asm=None):
    asm = asm if asm is not None else listing(extra)
    body, tail = kernel_text(asm)
    res = {}
    for key, pat in (("vgprs", r"\.amdhsa_next_free_vgpr (\d+)"), ("sgprs", r"\.amdhsa_next_free_sgpr (\d+)"),
                     ("scratch_bytes", r"\.amdhsa_private_segment_fixed_size (\d+)")):
        m = re.search(pat, tail)
        res[key] = int(m.group(1)) if m else None
    heads = re.findall(r"^(\.LBB\d+_\d+):\s*;\s*=>This Inner Loop Header", body, re.M)
    dma_loops = []
    for h in heads:
        items = loop_span(body, h)
        inside = [it for it in items if it[0] == "inst" and it[3]]
        if any("global_load_lds" in it[1] or "global_load_dwordx4" in it[1] for it in inside):
            dma_loops.append((h, items, inside))
    res["loops"] = []
    for h, items, inside in dma_loops:
        res["loops"].append({
            "header": h,
            "static_instructions": len(inside),
            "s_load": sum(1 for it in inside if it[1].startswith(("s_load_", "s_buffer_load_"))),
            "s_nop": sum(1 for it in inside if it[1].startswith("s_nop")),
            "v_readlane": sum(1 for it in inside if it[1].startswith("v_readlane")),
            "lds_dma": sum(1 for it in inside if "global_load_lds" in it[1]),
            "branches": sum(1 for it in inside if it[1].startswith(("s_branch", "s_cbranch"))),
            "longest_path": longest_path(items, h),
        })
    allitems = parse(body)
    res["m0_writes_outside_asm"] = [t for k, t, a in allitems if k == "inst" and not a and re.match(r"^\S+\s+m0\b", t)]
    return res, body


if __name__ == "__main__":
    extra = [a for a in sys.argv[1:] if a.startswith("-D")]
    res, body = report(extra, open(sys.argv[sys.argv.index("--asm") + 1]).read() if "--asm" in sys.argv else None)
    if "--dump" in sys.argv:
        open(sys.argv[sys.argv.index("--dump") + 1], "w").write(body)
    print(json.dumps(res))
