#!/usr/bin/env python3
"""Static instruction counts per phase of one segment of k_encode_local, from an ISA listing with line tables.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -DAEC_ENC_PART=16 -gline-tables-only -S --cuda-device-only \
          -o /tmp/aec_enc16_g.s libaec_amd/csrc/aec_enc.hip
    python tests/isa_phases_enc.py /tmp/aec_enc16_g.s [--symbol k_encode_localILi16ELi2ELb0EE] [--src <csrc of the listing>]

Every instruction of the kernel goes to the source line its `.loc` names (the innermost inlined frame, as in
tests/isa_phases.py) and the line to a phase: feed, option analysis, unary region, second extension, field region,
placement, copy-out, bookkeeping.  The segment body exists twice in the kernel: for segments whose blocks the lanes hold
from the load on (the DIRECT path, which the benchmark's shape runs) and for the others, fed through the LDS rows.  The
second copy is the one that reads rows (`ds_read_b128`).  Each copy ends with its copy-out, so the main loop is cut behind
the stores of the first copy-out in the listing; the part without a row read is the direct copy, and its figures are
printed beside those of the whole loop.  The counts are STATIC: a branch that few wavefronts take (the second
extension loop, emit_block for lanes that are not eligible, the fourth and fifth word of a placement) counts as much as
the straight path; emit_block's text is listed apart -- everything from the first to the last basic block that holds one of
its lines, which takes in the bit writer's flush branches inlined into it and, where the compiler moved them into that
stretch, blocks of its neighbours (in the parent's listing the copy-out lies inside it).  The dynamic figure (SQ_INSTS_VALU per segment) is in
profiles/r19/README.md.  Works on the sources of a tree with either small-block emitter (emit_small / emit_small_pairs)."""
import argparse
import collections
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_phases import CSRC, find  # noqa: E402

FEED, OPT, UNARY, SE, FIELDS, PLACE, COPY, BOOK, SLOW = (
    "feed (loads, byte order, predictor)", "option analysis", "unary region", "second extension", "field region",
    "placement (header, shifts, LDS or)", "copy-out (LDS image to the slot)", "bookkeeping (loop, geometry, scans, kept values)",
    "(emit_block: lanes that are not eligible)")
ORDER = [FEED, OPT, UNARY, SE, FIELDS, PLACE, COPY, BOOK, SLOW]


def function_span(lines, start_pat):
    a = find(lines, start_pat)
    depth, seen = 0, False
    for i in range(a - 1, len(lines)):
        depth += lines[i].count("{") - lines[i].count("}")
        seen = seen or "{" in lines[i]
        if seen and depth == 0:
            return a, i + 1
    raise SystemExit(f"no end of {start_pat}")


def table(src_dir):
    """[(file, first line, last line, phase)], the first match wins"""
    enc = open(os.path.join(src_dir, "aec_enc.hip")).read().split("\n")
    lane = open(os.path.join(src_dir, "aec_lane.h")).read().split("\n")
    t = []

    def whole(lines, fname, pat, phase):
        try:
            a, b = function_span(lines, pat)
        except SystemExit:
            return
        t.append((fname, a, b, phase))

    # the small-block emitter, line by line: which register a line builds
    for pat in (r"AEC_HD void emit_small_pairs\(", r"AEC_HD void emit_small\("):
        try:
            a, b = function_span(lane, pat)
        except SystemExit:
            continue
        se0 = find(lane, r"if \(AEC_ANY\(is_se\)\)", a)
        tail = find(lane, r"if \(!live\) return;|// header: option id", se0)
        for i in range(a, b + 1):
            text = lane[i - 1]
            if i >= tail:
                ph = PLACE
            elif i >= se0:
                ph = SE
            elif re.search(r"\bfa\b", text) and not re.search(r"\bua\b", text):
                ph = FIELDS
            else:
                ph = UNARY                # (the packed shift and add, the chain, the masks of k)
            t.append(("aec_lane.h", i, i, ph))
    whole(lane, "aec_lane.h", r"^struct BitWriter \{", PLACE)
    whole(lane, "aec_lane.h", r"AEC_HD bool small_eligible\(", PLACE)
    whole(lane, "aec_lane.h", r"AEC_HD bool pairs_eligible\(", PLACE)
    whole(lane, "aec_lane.h", r"AEC_HD uint32_t pair_shr\(", UNARY)
    whole(lane, "aec_lane.h", r"AEC_HD void emit_block\(", SLOW)
    whole(lane, "aec_lane.h", r"AEC_HD void emit_split_groups\(", SLOW)
    for pat in (r"AEC_HD void assess_split_with\(", r"AEC_HD BlockChoice choose_from\(", r"AEC_HD uint32_t zero_run_at\("):
        whole(lane, "aec_lane.h", pat, OPT)
    for pat in (r"void pp_words_pk\(", r"uint32_t pp_unsigned_pk\(", r"void fast_issue\(", r"void fast_finish\(",
                r"void direct_issue\(", r"void direct_finish\(", r"void load_segment_generic\(", r"^struct Feeder \{",
                r"uint32_t load_sample_raw\(", r"uint32_t sample_byte_order\("):
        whole(enc, "aec_enc.hip", pat, FEED)
    for pat in (r"BlockChoice choose_option_pk\(", r"bool block_is_zero\(", r"uint32_t analyze_segment\("):
        whole(enc, "aec_enc.hip", pat, OPT)
    # emit_segment: its own lines are the prefix sum of the lengths, the block's k and the control of the emission
    whole(enc, "aec_enc.hip", r"void emit_segment\(", BOOK)
    # the kernel: the copy-out inside do_segment, everything else bookkeeping
    ka, kb = function_span(enc, r"^k_encode_local\(const Cfg c")
    c0 = find(enc, r"const uint32_t nwords = \(lead \+ total \+ 31u\) >> 5", ka)
    c1 = find(enc, r"pos \+= total;", c0)
    t.append(("aec_enc.hip", c0, c1, COPY))
    t.append(("aec_enc.hip", ka, kb, BOOK))
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("--symbol", default="k_encode_localILi16ELi2ELb0EE")
    ap.add_argument("--src", default=CSRC, help="directory of the sources the listing was compiled from")
    args = ap.parse_args()
    files, body, inside = {}, [], False
    with open(args.asm) as f:
        for l in f:
            m = re.match(r'\s*\.file\s+(\d+)\s+"[^"]*"\s+"([^"]+)"', l)
            if m:
                files[int(m.group(1))] = os.path.basename(m.group(2))
            if not inside and re.match(r"^[A-Za-z_].*" + re.escape(args.symbol) + r".*:\s*(;.*)?$", l):
                inside = True
            if inside:
                body.append(l.rstrip("\n"))
                if re.match(r"\s*\.size\s", l):
                    break
    if not body:
        raise SystemExit("kernel not found")
    tab = table(args.src)

    def phase_of(loc):
        for fn, lo, hi, ph in tab:
            if loc[0] == fn and lo <= loc[1] <= hi:
                return ph
        return BOOK                        # (runtime headers: lane reads, ballots, DPP moves)

    instr = re.compile(r"^\t([vsd]_[a-z0-9_]+|ds_[a-z0-9_]+|global_[a-z0-9_]+|buffer_[a-z0-9_]+|flat_[a-z0-9_]+)\s")
    blocks, blk, cur, depth = [], [], ("?", 0), 0
    for l in body:
        m = re.match(r"\s*\.loc\s+(\d+)\s+(\d+)", l)
        if m:
            cur = (files.get(int(m.group(1)), "?"), int(m.group(2)))
            continue
        if l.startswith(".LBB") or l.startswith("; %bb"):
            if blk:
                blocks.append((depth, blk))
            blk = []
            d = re.search(r"Depth[= ](\d+)", l)
            depth = int(d.group(1)) if d else 0
            continue
        m = instr.match(l)
        if m:
            op = m.group(1)
            kind = "VALU" if op.startswith("v_") else "SALU" if op.startswith("s_") else "LDS" if op.startswith("ds_") else "VMEM"
            blk.append((cur, kind, op))
    if blk:
        blocks.append((depth, blk))
    loop = [(d, b) for d, b in blocks if d >= 1]
    # each copy of the segment body ends with its copy-out (stores to the slot): the loop is cut behind the first one
    stores = [i for i, (d, b) in enumerate(loop) if any(phase_of(loc) == COPY and kind == "VMEM" for loc, kind, _ in b)]
    if len(stores) < 2:
        raise SystemExit("the copy-outs of the two copies of the segment body were not found")
    gap = max(range(len(stores) - 1), key=lambda j: stores[j + 1] - stores[j])
    cut = stores[gap] + 1
    parts = [loop[:cut], loop[cut:]]
    rows = [any(op == "ds_read_b128" for _, b in p for _, _, op in b) for p in parts]
    if rows[0] == rows[1]:
        raise SystemExit("both parts of the loop, or neither, read LDS rows: the copies could not be told apart")
    direct_part = parts[1 if rows[0] else 0]

    def count(part):
        c = collections.Counter()
        # emit_block is inlined once per copy, as one stretch of the listing: every basic block from the first to the last
        # that holds one of its lines belongs to it, the bit writer's flush branches between them included
        own = [i for i, (_, b) in enumerate(part) if any(phase_of(loc) == SLOW for loc, _, _ in b)]
        for i, (_, b) in enumerate(part):
            slow = bool(own) and own[0] <= i <= own[-1]
            for loc, kind, _ in b:
                c[(SLOW if slow else phase_of(loc), kind)] += 1
        return c

    direct, whole = count(direct_part), count(loop)
    print(f"{args.symbol}: main loop {len(loop)} basic blocks, cut behind block {cut}; the direct copy is the "
          f"{'second' if rows[0] else 'first'} part ({len(direct_part)} blocks)")
    print(f"{'phase':62s} {'direct copy: VALU':>18s} {'SALU':>6s} {'LDS':>5s} {'VMEM':>5s} | {'whole loop: VALU':>17s} {'SALU':>6s} {'LDS':>5s} {'VMEM':>5s}")
    tot_d, tot_w = collections.Counter(), collections.Counter()
    for ph in ORDER:
        d = [direct[(ph, k)] for k in ("VALU", "SALU", "LDS", "VMEM")]
        w = [whole[(ph, k)] for k in ("VALU", "SALU", "LDS", "VMEM")]
        print(f"{ph:62s} {d[0]:18d} {d[1]:6d} {d[2]:5d} {d[3]:5d} | {w[0]:17d} {w[1]:6d} {w[2]:5d} {w[3]:5d}")
        if ph != SLOW:
            tot_d.update(dict(zip("vslm", d)))
            tot_w.update(dict(zip("vslm", w)))
    print(f"{'all but emit_block':62s} {tot_d['v']:18d} {tot_d['s']:6d} {tot_d['l']:5d} {tot_d['m']:5d} | "
          f"{tot_w['v']:17d} {tot_w['s']:6d} {tot_w['l']:5d} {tot_w['m']:5d}")


if __name__ == "__main__":
    sys.exit(main())
