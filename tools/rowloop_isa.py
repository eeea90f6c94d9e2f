"""Row-loop ISA report of the fused block-matching pass (csrc/dsx_bm.hip).

Cross-compiles one radius unit with -S (as tools/valu_roofline.py does) and prints, for every row
loop of an instantiation (the unaligned-dword copy and the clamped-byte copy of bm2_segment):

  * the VALU instruction count;
  * counts of ds_read2_b64, ds_read_b64, v_mad_u64_u32 and s_waitcnt vmcnt(..);
  * where each vmcnt wait sits in the step, counted from the step's first global load: how many
    of the loop's global loads and global_store_* / global_atomic_* precede it (a wait behind all
    of the stores is in the step's tail or at the next step's header), and, for the waits on the
    store-taking path of a step, how many of the step's stores each one drains (store_drains below);
  * the ds_* instructions by opcode and the LDS-path cycles per wave they amount to (LDS_CYCLES below:
    cycles per wave-instruction for conflict-free accesses; a store's cycles are those of moving its
    address and data dwords to the LDS).  Static counts over every block of the loop, the branches a
    benchmark step does not take included (odd-D overwrite, uniqueness re-reads, edge overwrites);
  * the SAD, add / sub, add3, byte-permute and DPP-move counts (column update, box phase, staging);
  * the kernel's VGPRs, scratch bytes and LDS bytes per block (Geo in dsx_bm.hip, restated here);
  * a segment-start table (segstart_report below): LDS drains of the init SAD loop, loads, vmcnt waits and global
    round trips of the init rows, memory waits in front of the segment loop.

It reports; it gates nothing.

usage:
  python tools/rowloop_isa.py [c2 c2r c4 c5 c1 c3 sad0 .. sad7 ...] [--src <dsx_bm.hip>] [--tag <text>]
  (sad<R>: bm2<R, SAD, 1, 0>, the plain left pass of the pair layout at radius R)
"""
from __future__ import annotations

import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from valu_roofline import BENCH_KERNELS, ROOT, blocks, function_body, kernel_label, row_loops, symbol  # noqa: E402

ORDER = ["c2", "c2r", "c4", "c5", "c1", "c3"]


# LDS cycles per wave64 instruction, conflict-free (measured on MI355X; stores: 2 cycles per source
# dword moved to the LDS, the 12- and 16-byte forms more; ds_write_addtid_b32 has no address dword)
LDS_CYCLES = {
    "ds_read_u8": 2, "ds_read_i8": 2, "ds_read_u16": 2, "ds_read_i16": 2, "ds_read_u16_d16": 2, "ds_read_u16_d16_hi": 2,
    "ds_read_b32": 2, "ds_read_b64": 2, "ds_read_b96": 8, "ds_read_b128": 4, "ds_read2_b32": 4, "ds_read2_b64": 8,
    "ds_write_b8": 4, "ds_write_b16": 4, "ds_write_b32": 4, "ds_write_b64": 6, "ds_write2_b32": 6,
    "ds_write_b96": 10, "ds_write_b128": 13, "ds_write2_b64": 13, "ds_write_addtid_b32": 2,
}


def lds_report(ops):
    """(text, cycles) for the ds_* instructions of a loop; opcodes without a table entry are listed at 0."""
    cnt = {}
    for _, op, _ in ops:
        if op.startswith("ds_"):
            cnt[op] = cnt.get(op, 0) + 1
    cyc = sum(n * LDS_CYCLES.get(op, 0) for op, n in cnt.items())
    txt = ", ".join(f"{op} {n}" + ("" if op in LDS_CYCLES else " (no table entry)") for op, n in sorted(cnt.items()))
    return txt, cyc


def rnd16(v):
    return (v + 15) & ~15


def lds_bytes(r, ssd, nw, side):
    """Geo<R, SSD, NW>::SMEM plus the SAD LR pass's exit region (launch_bm2_side)."""
    tx, nc, kd = 32, 32 + 2 * r, (1 if ssd else 2)
    dp = nw * 64 * kd
    pitch = dp * (4 if ssd else 2) + 16
    slot = rnd16((nc + dp) * 4 + 16) + rnd16(4 * (nc + 8))
    smem = max(4 * slot + tx * pitch, (2 * r + 1) * slot)
    return smem + (128 * nw if side == 3 and not ssd else 0)


def meta(asm, sym):
    m = re.search(r"\.amdhsa_kernel " + re.escape(sym) + r"\n(.*?)\.end_amdhsa_kernel", asm, re.S)
    d = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)", m.group(1))} if m else {}
    return d.get("next_free_vgpr"), d.get("private_segment_fixed_size"), d.get("accum_offset")


def lines_of(body):
    """[(block label, op, operands)] in layout order."""
    out, lab = [], "entry"
    for line in body.split("\n"):
        if line.startswith(".LBB"):
            lab = line.split(":")[0]
        elif line.startswith("\t"):
            t = line.strip()
            if t and not t.startswith((".", ";")):
                p = t.split(None, 1)
                out.append((lab, p[0], p[1] if len(p) > 1 else ""))
    return out


def store_drains(ops, head):
    """{op index: (k, text)} for the vmcnt waits on the store-taking path of one step of a row loop.

    ops are the loop's (label, op, operands) in layout order, the header block included.  The step is walked from its
    first global load (the first one the header reaches) round to that load again.  At a branch the walk takes the
    side that still holds more global_store_* / global_atomic_* - the store-taking path - and between sides that hold
    equally many the longer one (the work of a full step: a side that only skips something is not taken).  Inner
    loops are passed once.  vmcnt counts loads and stores in order, so a vmcnt(n) wait retires all but the youngest n
    of them: the wait is there for the youngest load it retires, and it drains the k stores issued behind that load
    that it retires with it (every store it retires, where it retires no load).  The walk goes round twice and
    reports the second time, when the stores of the previous step's tail are in the queue.  Static: a side that the
    kernel only takes on steps without stores (a first step's staging behind the box phase, where the build has one)
    is not known to be such, is walked behind the stores and reported as draining them."""
    at = {}
    for k, (lab, _, _) in enumerate(ops):
        at.setdefault(lab, k)
    n = len(ops)
    is_load = lambda k: ops[k][1].startswith("global_load")  # noqa: E731
    is_store = lambda k: ops[k][1].startswith(("global_store", "global_atomic"))  # noqa: E731

    def succ(k):
        _, op, arg = ops[k]
        s = []
        if op != "s_branch" and op != "s_endpgm" and k + 1 < n:
            s.append(k + 1)
        if op.startswith(("s_cbranch", "s_branch")):
            t = re.search(r"(\.LBB\d+_\d+)", arg)
            if t and t.group(1) in at:
                s.append(at[t.group(1)])
        return s

    if head not in at:
        return {}
    seen, todo, first = set(), [at[head]], []
    while todo:
        k = todo.pop()
        if k in seen:
            continue
        seen.add(k)
        if is_load(k):
            first.append(k)
            continue
        todo.extend(succ(k))
    if not first:
        return {}
    start = min(first)
    # value of the best way on from op k: (stores ahead, length), ways into the start or out of the loop end
    val, state, stack = {}, {}, [(start, iter(succ(start)))]
    better = lambda a, b: a > b  # noqa: E731  (stores ahead, then length)
    best_of, acc = {start: None}, {start: None}
    state[start] = 1
    while stack:
        k, it = stack[-1]
        nxt = next(it, None)
        if nxt is None:
            stack.pop()
            a = acc[k] or (0, 0)
            val[k] = (a[0] + (1 if is_store(k) else 0), a[1] + 1)
            state[k] = 2
            if stack:
                p = stack[-1][0]
                if acc[p] is None or better(val[k], acc[p]):
                    acc[p], best_of[p] = val[k], k
            continue
        if nxt == start or state.get(nxt) == 1:  # round the step, or an inner loop's back edge
            if nxt == start and (acc[k] is None or better((0, 0), acc[k])):
                acc[k], best_of[k] = (0, 0), start
            continue
        if state.get(nxt) == 2:
            if acc[k] is None or better(val[nxt], acc[k]):
                acc[k], best_of[k] = val[nxt], nxt
            continue
        state[nxt] = 1
        acc[nxt], best_of[nxt] = None, None
        stack.append((nxt, iter(succ(nxt))))
    path, k = [], start
    while k is not None and (k != start or not path) and len(path) <= n:
        path.append(k)
        k = best_of.get(k)
    found, queue = {}, []
    for lap in range(2):
        for k in path:
            if is_load(k):
                queue.append("L")
            elif is_store(k):
                queue.append("S")
            elif ops[k][1] == "s_waitcnt" and "vmcnt" in ops[k][2]:
                v = int(re.search(r"vmcnt\((\d+)\)", ops[k][2]).group(1))
                gone = queue[:max(0, len(queue) - v)]
                queue = queue[len(gone):]
                if lap:
                    if "L" in gone:
                        d = gone[len(gone) - gone[::-1].index("L"):].count("S")
                        found[k] = (d, f"drains {d} stores")
                    else:
                        d = gone.count("S")
                        found[k] = (d, f"drains {d} stores (retires no load)")
    return found


def report(asm, name, out):
    r, ssd, nw, side, abs_ = BENCH_KERNELS[name]
    sym = symbol(r, ssd, nw, side, abs_)
    body = function_body(asm, sym)
    bl = blocks(body)
    loops, nvalu = row_loops(bl)
    vg, scratch, acc = meta(asm, sym)
    out(f"{name} {kernel_label(r, ssd, nw, side, abs_)}: VGPRs {vg} (accum offset {acc}), scratch {scratch} B, "
        f"LDS {lds_bytes(r, ssd, nw, side)} B per block")
    ln = lines_of(body)
    for i, j in loops:
        labs = {bl[k][0] for k in range(i, j + 1)}
        ops = [(lab, op, arg) for lab, op, arg in ln if lab in labs]
        cnt = lambda p: sum(1 for _, op, _ in ops if op.startswith(p))  # noqa: E731
        out(f"  loop {bl[i][0]} .. {bl[j][0]}: VALU {nvalu((i, j))}, ds_read2_b64 {cnt('ds_read2_b64')}, "
            f"ds_read_b64 {cnt('ds_read_b64')}, v_mad_u64_u32 {cnt('v_mad_u64_u32')}, "
            f"global loads {cnt('global_load')}, global stores/atomics {cnt('global_store') + cnt('global_atomic')}")
        txt, cyc = lds_report(ops)
        out(f"    LDS: {txt}")
        out(f"    LDS-path cycles per wave (static): {cyc}; s_nop {cnt('s_nop')}, v_readfirstlane {cnt('v_readfirstlane')}, "
            f"v_lshl_add_u64 {cnt('v_lshl_add_u64')}")
        # the column update and the box phase by opcode (the pair layout's byte SADs, their subtractions, the box sums)
        out(f"    sums: v_sad_u8 {cnt('v_sad_u8')}, v_sad_hi_u8 {cnt('v_sad_hi_u8')}, v_sub_u32 {cnt('v_sub_u32')}, "
            f"v_add_u32 {cnt('v_add_u32')}, v_add3_u32 {cnt('v_add3_u32')}, v_perm_b32 {cnt('v_perm_b32')}, "
            f"v_mov_b32_dpp {cnt('v_mov_b32_dpp')}")
        # the tail's block keys by opcode: block minima (packed, then low against high half), key forms, running key
        out(f"    keys: v_pk_min_u16 {cnt('v_pk_min_u16')}, v_pk_minimum3_f16 {cnt('v_pk_minimum3_f16')}, "
            f"v_min_u16 {cnt('v_min_u16')}, v_lshl_or_b32 {cnt('v_lshl_or_b32')}, v_min_u32 {cnt('v_min_u32')}, "
            f"v_min3_u32 {cnt('v_min3_u32')}")
        # The compiler lays the blocks of a step out of program order (the column update and the
        # box phase sit behind the stores in the listing), so positions are taken from the control
        # flow: op k leads to op k + 1 (unless it is s_branch) and to its branch target.  The step
        # is cut at its global loads (the prefetch).  A wait "follows a store" when a store reaches
        # it without crossing a load - tail of the step or header of the next one - and is "at the
        # header" when the loop's header block reaches it before any load or LDS operation.
        at = {}
        for k, (lab, _, _) in enumerate(ops):
            at.setdefault(lab, k)
        loads = {k for k, (_, op, _) in enumerate(ops) if op.startswith("global_load")}
        lds = {k for k, (_, op, _) in enumerate(ops) if op.startswith("ds_")}

        def reach(starts, cut):
            seen, todo = set(), list(starts)
            while todo:
                k = todo.pop()
                if k in seen or k >= len(ops):
                    continue
                seen.add(k)
                if k in cut:
                    continue
                _, op, arg = ops[k]
                if op.startswith(("s_cbranch", "s_branch")):
                    t = re.search(r"(\.LBB\d+_\d+)", arg)
                    if t and t.group(1) in at:
                        todo.append(at[t.group(1)])
                if op != "s_branch" and k + 1 < len(ops) and (ops[k + 1][0] == ops[k][0] or ops[k + 1][0] in at):
                    todo.append(k + 1)
            return seen

        hdr = re.findall(r"in Loop: Header=(BB\d+_\d+) Depth=2", "\n".join(
            b for b in re.split(r"\n(?=\.LBB\d+_\d+:)", body) if b.split(":")[0] in labs))
        head = ".L" + max(set(hdr), key=hdr.count) if hdr else ops[0][0]
        after_store = reach([k + 1 for k, (_, op, _) in enumerate(ops) if op.startswith(("global_store", "global_atomic"))], loads)
        at_header = reach([at[head]], loads | lds) if head in at else set()
        # "follows a store" is positional.  What costs is a wait that retires a store of the step with the load it is
        # there for: store_drains walks the store-taking path of a step, over the whole loop - the blocks above plus
        # every block that names the header as its loop (a rotated loop's header and latch lie outside the range).
        texts = {b.split(":")[0]: b for b in re.split(r"\n(?=\.LBB\d+_\d+:)", body)}
        mine = re.compile(r"(Header=|Parent Loop )" + re.escape(head[2:]) + r"\b")
        wlabs = labs | {b[0] for b in bl if b[0] == head or mine.search(texts.get(b[0], ""))}
        wops = [(g, lab, op, arg) for g, (lab, op, arg) in enumerate(ln) if lab in wlabs]
        found = {wops[k][0]: v for k, v in store_drains([w[1:] for w in wops], head).items()}
        gidx = [g for g, (lab, _, _) in enumerate(ln) if lab in labs]
        waits = []
        for k, (lab, op, arg) in enumerate(ops):
            if op == "s_waitcnt" and "vmcnt" in arg:
                v = re.search(r"vmcnt\((\d+)\)", arg).group(1)
                where = [w for w, c in (("at the loop header", k in at_header), ("follows a store of the step", k in after_store)) if c]
                d = found.get(gidx[k])
                waits.append(f"    vmcnt({v}) in {lab}: {', '.join(where) or 'between the prefetch and the stores'}; "
                             + (d[1] if d else "not on the store-taking path"))
        out(f"    s_waitcnt vmcnt: {len(waits)}")
        for w in waits:
            out(w)
        extra = [(g, lab, arg) for g, lab, op, arg in wops if g in found and lab not in labs]
        for g, lab, arg in extra:
            out(f"    {arg.strip()} in {lab} (a block of the loop outside the range above): {found[g][1]}")
        worst = max((d for d, _ in found.values()), default=0)
        out(f"    store-taking path: {len(found)} vmcnt waits, " + (f"the worst drains {worst} stores" if worst else "none drains a store"))


def segstart_report(asm, name, out):
    """Segment-start table of one instantiation: what a block waits for between kernel entry and a segment's
    first row step.  Per copy of bm2_segment (unaligned-dword, clamped):

      * the init SAD loop - the innermost loop outside the row loops that holds v_sad_* and LDS reads and no global
        memory operation (one iteration per row group of the transposed init, per row of the row-by-row init): its
        s_waitcnt lgkmcnt(0) (full LDS drains) and all lgkmcnt waits per iteration;
      * the init row loads - the blocks from which that loop is reached without crossing a global store (the previous
        segment's row loop) or the head of the segment loop: global loads, vmcnt waits, and the global round trips they add up to
        (a loop over row groups that holds loads: one per group; straight-line code: the runs of loads that a vmcnt
        wait separates from the next load);
      * the memory waits (vmcnt / lgkmcnt) in front of the segment loop, from kernel entry.
    """
    r, ssd, nw, side, abs_ = BENCH_KERNELS[name]
    sym = symbol(r, ssd, nw, side, abs_)
    body = function_body(asm, sym)
    bl = blocks(body)
    loops, _ = row_loops(bl)
    ln = lines_of(body)
    index = {lab: i for i, (lab, _, _) in enumerate(bl)}
    ops_of = {}
    for lab, op, arg in ln:
        ops_of.setdefault(lab, []).append((op, arg))
    in_row = set()
    for i, j in loops:
        in_row |= set(range(i, j + 1))
    back = sorted({(index[t], j) for j, (_, _, tg) in enumerate(bl) for t in tg if t in index and index[t] <= j})
    rng_ops = lambda i, j: [o for k in range(i, j + 1) for o in ops_of.get(bl[k][0], [])]  # noqa: E731
    has = lambda ops, p: any(op.startswith(p) for op, _ in ops)  # noqa: E731
    vg, scratch, _ = meta(asm, sym)
    out(f"{name} {kernel_label(r, ssd, nw, side, abs_)} segment start: VGPRs {vg}, scratch {scratch} B")
    if loops:
        seg0 = min(i for i, j in back if any(i <= a and b <= j for a, b in loops))
        waits = [f"{op} {arg}" for k in range(seg0) for op, arg in ops_of.get(bl[k][0], [])
                 if op == "s_waitcnt" and ("vmcnt" in arg or "lgkmcnt" in arg)]
        out(f"  kernel entry to the segment loop ({bl[seg0][0]}): {len(waits)} memory waits: {'; '.join(waits) or '-'}")
    # successors in the control flow (fall-through unless the block ends in s_branch)
    succ = {}
    for k, (lab, ops, tg) in enumerate(bl):
        s = {index[t] for t in tg if t in index}
        if k + 1 < len(bl) and not (ops and ops[-1] == "s_branch"):
            s.add(k + 1)
        succ[k] = s
    pred = {}
    for k, s in succ.items():
        for t in s:
            pred.setdefault(t, set()).add(k)
    ngr = (2 * r + 1 + 3) // 4
    for i, j in back:
        ops = rng_ops(i, j)
        if (i in in_row or not has(ops, "v_sad_") or not has(ops, "ds_read") or has(ops, "global_")
                or any((a, b) != (i, j) and i <= a and b <= j for a, b in back)):
            continue
        n = lambda p: sum(1 for op, _ in ops if op.startswith(p))  # noqa: E731
        full = sum(1 for op, arg in ops if op == "s_waitcnt" and "lgkmcnt(0)" in arg)
        anyw = sum(1 for op, arg in ops if op == "s_waitcnt" and "lgkmcnt" in arg)
        out(f"  init SAD loop {bl[i][0]}: v_sad {n('v_sad_')}, LDS reads {n('ds_read')}, s_waitcnt lgkmcnt(0) {full} "
            f"of {anyw} lgkmcnt waits per iteration")
        # backwards from the loop, not through global stores, row loops or the loop itself
        reg, todo = set(), [p for p in pred.get(i, ()) if not i <= p <= j]
        while todo:
            k = todo.pop()
            if k in reg or k in in_row or (loops and k <= seg0) or has(ops_of.get(bl[k][0], []), "global_store") or has(ops_of.get(bl[k][0], []), "global_atomic"):
                continue
            reg.add(k)
            todo.extend(pred.get(k, ()))
        rops = [o for k in sorted(reg) for o in ops_of.get(bl[k][0], [])]
        loads = sum(1 for op, _ in rops if op.startswith("global_load"))
        vmw = [arg for op, arg in rops if op == "s_waitcnt" and "vmcnt" in arg]
        looped = any(all(k in reg for k in range(a, b + 1)) and has(rng_ops(a, b), "global_load") for a, b in back)
        if looped:
            trips = f"{ngr} (a loop over the {ngr} row groups holds the loads)" if has(rops, "v_perm") else "one per loop iteration"
        else:
            t, pending, waited = 0, False, True
            for k in sorted(reg):
                for op, arg in ops_of.get(bl[k][0], []):
                    if op.startswith("global_load"):
                        if waited:
                            t, waited = t + 1, False
                        pending = True
                    elif op == "s_waitcnt" and "vmcnt" in arg and pending:
                        waited = True
            trips = str(t)
        out(f"    init row loads in front of it: global loads {loads}, vmcnt waits {len(vmw)}, global round trips {trips}")


def main(argv):
    src = os.path.join(ROOT, "depthestimation_amd", "csrc", "dsx_bm.hip")
    tag = None
    names = []
    it = iter(argv)
    for a in it:
        if a == "--src":
            src = next(it)
        elif a == "--tag":
            tag = next(it)
        else:
            names.append(a)
    names = names or ORDER
    for n in names:  # sad<R>: the plain left pass of the pair layout at radius R, bm2<R, SAD, 1, 0>
        if re.fullmatch(r"sad[0-7]", n):
            BENCH_KERNELS.setdefault(n, (int(n[3]), False, 1, 0, False))
    out = print
    if tag:
        out(f"== {tag} ==")
    tmp = tempfile.mkdtemp(prefix="dsx_rowloop_")
    asm = {}
    procs = {}
    for r in sorted({BENCH_KERNELS[n][0] for n in names}):
        procs[r] = subprocess.Popen(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", f"-DDSX_RADIUS={r}",
                                     "-I", os.path.dirname(src), "--cuda-device-only", "-S", "-o",
                                     os.path.join(tmp, f"r{r}.s"), src], stderr=subprocess.DEVNULL)
    for r, p in procs.items():
        if p.wait() != 0:
            raise SystemExit(f"hipcc failed for radius {r}")
        asm[r] = open(os.path.join(tmp, f"r{r}.s")).read()
    for n in names:
        report(asm[BENCH_KERNELS[n][0]], n, out)
        segstart_report(asm[BENCH_KERNELS[n][0]], n, out)


if __name__ == "__main__":
    main(sys.argv[1:])
