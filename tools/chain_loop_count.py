#!/usr/bin/env python3
"""Instruction counts of the batch-1 chain loop (attention.hip fx1_chain_body)
from compiled ISA.

  hipcc <the Makefile's HIPFLAGS> -S --cuda-device-only csrc/attention.hip -o attention.s
  python tools/chain_loop_count.py attention.s [--path]

For qkv_attn1_kernel<64> and <128>: the function is cut into basic blocks (at
every label and after every branch); for each loop whose blocks hold chain
instructions (v_fma_mix_f32 / v_cvt_f16_f32) the script takes, among the
simple paths from the loop header back to the header that stay inside the
loop, never enter a block of the slow path (one with a v_mul_f32: fx8_slow)
and run every buffer they load exactly once (16 chain instructions per 16-B
V^T load), the one with the fewest instructions a buffer -- the all-fast
iteration.  An iteration covers one or two 64-key buffers; the figures are
per buffer (chain instructions / 128): 128 chain instructions and the others
by class."""
import collections
import re
import sys

CHAIN = ("v_fma_mix_f32", "v_cvt_f16_f32")


def classify(op):
    if op in CHAIN:
        return "chain"
    if op.startswith(("global_load", "buffer_load", "flat_load")):
        return "vmem load"
    if op.startswith("ds_read"):
        return "ds_read"
    if op in ("s_waitcnt", "s_nop"):
        return op
    if op.startswith("s_cbranch") or op == "s_branch":
        return "branch"
    return "salu" if op.startswith("s_") else "valu" if op.startswith("v_") else "other"


def blocks_of(lines, name):
    """basic blocks of function `name`: dict(label, ops, loop, succ)"""
    start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
    bl, loop = [dict(label="<entry>", ops=[], loop=None)], None
    for l in lines[start + 1:]:
        if l.startswith(".Lfunc_end"):
            break
        m = re.match(r"^(\.LBB\d+_\d+):(.*)", l) or re.match(r"^(; %bb\.\d+):(.*)", l)
        if m:
            hdr = re.search(r"Header=(BB\d+_\d+)", m.group(2))
            loop = m.group(1) if "Loop Header" in m.group(2) else ".L" + hdr.group(1) if hdr else None
            bl.append(dict(label=m.group(1), ops=[], loop=loop))
            continue
        t = l.strip()
        if not t or t[0] in ";." or t.endswith(":"):
            continue
        op = t.split(";")[0].split()
        bl[-1]["ops"].append(op)
        if op[0].startswith("s_cbranch") or op[0] == "s_branch":
            bl.append(dict(label=None, ops=[], loop=loop))
    idx = {b["label"]: i for i, b in enumerate(bl) if b["label"]}
    for i, b in enumerate(bl):
        t = b["ops"][-1] if b["ops"] else None
        b["succ"] = []
        if t and t[0] == "s_branch":
            b["succ"] = [idx[t[1]]]
        else:
            if i + 1 < len(bl):
                b["succ"].append(i + 1)
            if t and t[0].startswith("s_cbranch"):
                b["succ"].append(idx[t[1]])
    return bl, idx


def report(lines, name, show):
    bl, idx = blocks_of(lines, name)
    loops = collections.Counter()
    for b in bl:
        if b["loop"]:
            loops[b["loop"]] += sum(o[0] in CHAIN for o in b["ops"])
    print(name)
    for hdr, nchain in loops.items():
        if nchain < 128:
            continue
        h = idx[hdr]
        ok = lambda j: bl[j]["loop"] == hdr and not any(o[0] == "v_mul_f32" for o in bl[j]["ops"])
        # every simple header -> header path over such blocks that runs each
        # buffer it loads once (16 chain instructions per 16-B V^T load); of
        # those the one with the fewest instructions
        best, stack = None, [(h, [h])]
        while stack:
            j, p = stack.pop()
            for s in bl[j]["succ"]:
                if s == h:
                    ops = [o[0] for k in p for o in bl[k]["ops"]]
                    nch, nld = sum(o in CHAIN for o in ops), sum(classify(o) == "vmem load" for o in ops)
                    if nch and nch == 16 * nld and (best is None or len(ops) / nch < best[0]):
                        best = (len(ops) / nch, p)
                elif ok(s) and s not in p:
                    stack.append((s, p + [s]))
        if best is None:
            continue
        path = best[1]
        cls = collections.Counter(classify(o[0]) for j in path for o in bl[j]["ops"])
        if cls["chain"] == 0:
            continue
        nbuf = cls["chain"] / 128.0
        tot = sum(cls.values())
        print(f"  loop {hdr}: the all-fast iteration holds {cls['chain']} chain instructions = {nbuf:g} buffer(s) of 64 keys")
        print(f"    per buffer: {tot / nbuf:g} instructions = 128 chain + {(tot - cls['chain']) / nbuf:g} others")
        print("    others per buffer: " + ", ".join(f"{k} {v / nbuf:g}" for k, v in sorted(cls.items()) if k != "chain"))
        if show:
            for j in path:
                print(f"      {bl[j]['label'] or '(after branch)'}: " + " ".join(o[0] for o in bl[j]["ops"] if o[0] not in CHAIN))


def main():
    lines = open(sys.argv[1]).read().split("\n")
    for spl in (64, 128):
        name = next(l.split(":")[0] for l in lines if re.match(rf"^_ZN4qasr16qkv_attn1_kernelILi{spl}E.*:", l))
        report(lines, name, "--path" in sys.argv)
        i = next(k for k, l in enumerate(lines) if l.startswith(f"    .symbol:") and name + ".kd" in l)
        meta = [l.strip() for l in lines[i - 40:i + 8] if re.search(r"vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size", l)]
        print("    " + "  ".join(meta))


if __name__ == "__main__":
    main()
