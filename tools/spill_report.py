#!/usr/bin/env python3
"""Scalar and vector spill traffic of the node pipeline's two hot kernels, per loop nest, from `make asm`'s outputs (no GPU involved).

For every instantiation of skr_leaf_kernel2 and skr_trace_kernel in build/render_nodes.s: code bytes, VGPRs, occupancy, spilled SGPRs and
VGPRs and scratch (build/resource_usage.txt), then one line per loop nest — a nest is a basic block's innermost loop header and its depth,
from the assembler's `; in Loop: Header=... Depth=...` comments; `-` is the code outside every loop — with the instructions that matter
for spills: VALU in all, v_readlane / v_writelane (a spilled SGPR travels through a lane of a carrier VGPR), scratch loads and stores
(spilled VGPRs) and s_nop (the hazard slots behind lane operations).  `below` sums a nest and every nest inside it.
usage: python tools/spill_report.py [BUILD_DIR]      (default: build)"""
import os
import re
import subprocess
import sys

KERNELS = ("skr_leaf_kernel2", "skr_trace_kernel")
COLS = ("valu", "readlane", "writelane", "scr_load", "scr_store", "s_nop")
PAT = {"valu": r"v_", "readlane": r"v_readlane_b32", "writelane": r"v_writelane_b32", "scr_load": r"scratch_load", "scr_store": r"scratch_store",
       "s_nop": r"s_nop"}


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {n: re.sub(r"^void ", "", d).replace("(RenderParams)", "") for n, d in zip(names, out)}


def resources(path):
    """{mangled name: {remark field: value}} of -Rpass-analysis=kernel-resource-usage"""
    res, cur = {}, None
    for ln in open(path):
        m = re.search(r"remark:\s+Function Name: (\S+)", ln)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][\w /\[\]]*?): (\S+) \[-Rpass", ln)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return res


def functions(path):
    """{mangled name: lines of the function} of one listing"""
    out, name, body = {}, None, []
    for ln in open(path).read().split("\n"):
        if name is None:
            m = re.match(r"^(_Z[\w$.]*):", ln)
            if m:
                name, body = m.group(1), []
            continue
        body.append(ln)
        if "; codeLenInByte" in ln:  # (the kernel's info block, behind its .Lfunc_end)
            out[name] = body
            name = None
    return out


def nests(body):
    """the blocks of one function: ({(header, depth): counts}, {header: parent header}, order of first appearance, code bytes)"""
    counts, parent, order = {}, {}, []
    key, label, pending = ("-", 0), None, False  # pending: in a block's comment lines, before its first instruction
    code, ended = None, False
    for ln in body:
        ended = ended or re.match(r"^\.Lfunc_end\d+:", ln) is not None
        m = re.search(r"; codeLenInByte = (\d+)", ln)
        if m:
            code = int(m.group(1))
        blk = re.match(r"^(?:\.L(BB\d+_\d+):|; %bb\.\d+:)(.*)$", ln)
        if blk:
            label, key, pending = blk.group(1), ("-", 0), True
            ln = ";" + blk.group(2)
        s = ln.strip()
        if pending and s.startswith(";"):
            m = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", s)
            if m:
                key = (m.group(1), int(m.group(2)))
            m = re.search(r"Parent Loop (BB\d+_\d+) Depth=(\d+)", s)
            if m and label:
                parent.setdefault(label, []).append((int(m.group(2)), m.group(1)))
            m = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", s)
            if m and label:
                key = (label, int(m.group(1)))
            continue
        if ended or not s or s.startswith((";", ".")) or s.endswith(":"):
            continue
        pending = False
        if key not in counts:
            counts[key] = dict.fromkeys(COLS, 0)
            counts[key]["insts"] = counts[key]["hdr_readlane"] = 0
            order.append(key)
        c = counts[key]
        c["insts"] += 1
        for k in COLS:
            if re.match(PAT[k], s):
                c[k] += 1
        if label == key[0] and re.match(PAT["readlane"], s):
            c["hdr_readlane"] += 1  # (in the loop's header block itself)
    up = {h: max(ps)[1] for h, ps in parent.items()}  # the innermost enclosing loop: the deepest parent
    return counts, up, order, code


def report(build):
    res = resources(os.path.join(build, "resource_usage.txt"))
    fns = functions(os.path.join(build, "render_nodes.s"))
    names = sorted(n for n in fns if any(k in n for k in KERNELS))
    dm = demangle(names)
    for n in sorted(names, key=lambda x: dm[x]):
        counts, up, order, code = nests(fns[n])
        r = res.get(n, {})
        print("== %s" % dm[n])
        print("   code %s bytes, VGPRs %s, occupancy %s, SGPR spills %s, VGPR spills %s, scratch %s B/lane, SGPRs %s" % (
            code, r.get("VGPRs"), r.get("Occupancy [waves/SIMD]"), r.get("SGPRs Spill"), r.get("VGPRs Spill"), r.get("ScratchSize [bytes/lane]"),
            r.get("TotalSGPRs")))

        def inside(h, top):
            while h is not None:
                if h == top:
                    return True
                h = up.get(h)
            return False

        print("   %-10s %5s %6s | %6s %8s %9s %8s %9s %6s | below: %8s %9s %8s %9s | %s" % (
            "nest", "depth", "insts", "valu", "readlane", "writelane", "scr_load", "scr_store", "s_nop", "readlane", "writelane", "scr_load", "scr_store", "header-block readlane"))
        tot = dict.fromkeys(COLS + ("insts",), 0)
        for key in order:
            c = counts[key]
            for k in tot:
                tot[k] += c[k]
            sub = dict.fromkeys(COLS, 0)
            for k2, c2 in counts.items():
                if key[0] != "-" and inside(k2[0], key[0]):
                    for k in COLS:
                        sub[k] += c2[k]
            below = "%8d %9d %8d %9d | %d" % (sub["readlane"], sub["writelane"], sub["scr_load"], sub["scr_store"], c["hdr_readlane"]) if key[0] != "-" else ""
            print("   %-10s %5d %6d | %6d %8d %9d %8d %9d %6d |        %s" % (
                key[0], key[1], c["insts"], c["valu"], c["readlane"], c["writelane"], c["scr_load"], c["scr_store"], c["s_nop"], below))
        print("   %-10s %5s %6d | %6d %8d %9d %8d %9d %6d |" % (
            "total", "", tot["insts"], tot["valu"], tot["readlane"], tot["writelane"], tot["scr_load"], tot["scr_store"], tot["s_nop"]))
        print()


if __name__ == "__main__":
    report(sys.argv[1] if len(sys.argv) > 1 else "build")
