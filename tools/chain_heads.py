#!/usr/bin/env python3
"""tools/chain_heads.py FILE.s KERNEL_SUBSTRING [FIRST_REQUEST_REGEX] [--row REGEX] [--max N] [--groups G] [--ends] [--avoid B,B..] [--distinct]

The head of a wavefront's dependent chain, read from the emitted code: for every distinct way through the kernel's basic blocks
from its entry down to the first ROW request, the waits and memory requests on the way, in order.  One line per way:

    way 3  waits before first request 0 | wait groups first request -> row request 1 | blocks 0 381 594 600
           sl2 sl4 sl8 ... SL8* sl4 [lgkmcnt(0)] br g g G4!

FIRST_REQUEST_REGEX: the instruction that is the first request of the chain (default: a `s_load_dwordx8` whose base is not the kernel-argument
pointer s[0:1] - the update kernel's plan record; e.g. `global_load_dword ` for an id load).  It is marked `*`; ways that never reach it are printed with `-` in its column.
--row: the row request the way ends at (default `global_load_dwordx4`), marked `!`.
Tokens: slN = scalar load of N dwords, gN / g = global load of N dwords / one dword, S = store, A = atomic, r / w = LDS,
[..] = s_waitcnt, BAR = barrier, br = a branch taken or fallen through.  A "wait group" is a run of s_waitcnt with no request
between them.  The first 256 bytes of a kernel with preloaded arguments (s_load + s_waitcnt + s_branch, then .p2align 8) are the
compatibility header for firmware without preload: they are skipped.

Ways are told apart by their tokens only: two ways with the same tokens print once (the first block list found).  Loops are
followed once.  A way with more than G (default 4) wait groups behind its first request is no head and is not listed (the
sampler tail of update_kernel_reg has hundreds of them); --ends also lists the ways that end the program without a row request.
--distinct: one line per distinct sequence of requests and waits (branches dropped) with the number of ways that share it.
--max N (default 40): stop after N distinct ways.  A way that has passed 64 blocks without meeting FIRST_REQUEST_REGEX is given up.
--avoid: blocks no way may enter, by the names the block lists show (a block is
cut behind every branch: 0' is what follows block 0's first branch) - `--avoid "0'"` keeps the walk out of update_kernel_reg's
sampler tail, which starts there.

FILE.s from:  hipcc -O3 -std=c++17 --offload-arch=gfx950 -mllvm -amdgpu-kernarg-preload-count=16 -S --cuda-device-only X.hip
(profiles/r10_update_heads.txt)."""
import re
import sys

# the update kernel's plan record: a 32-byte scalar load whose base is NOT the kernel-argument pointer s[0:1]
RECORD = r's_load_dwordx8 s\[\d+:\d+\], s\[(?!0:1\])'
LOADW = {"dword": 1, "dwordx2": 2, "dwordx3": 3, "dwordx4": 4, "dwordx8": 8, "dwordx16": 16}


def kernel_body(text, pat):
    for m in re.finditer(r'^(\S+):\s*; @\1\n(.*?)\.end_amdhsa_kernel', text, re.S | re.M):
        if pat in m.group(1):
            yield m.group(1), m.group(2)


def blocks_of(body):
    """[(label, [instruction lines])] in layout order, cut behind every branch (a label's later pieces are label', label'', ..);
    the preload compatibility header is dropped"""
    lines = body.split("\n")
    for i, ln in enumerate(lines[:12]):
        if ln.strip().replace("\t", " ") == ".p2align 8":
            lines = lines[i + 1:]
            break
    out, cur, name = [], [], "entry"
    for ln in lines:
        t = ln.strip()
        m = re.match(r'^(\.LBB\d+_\d+):', t)
        if m:
            out.append((name, cur)); name, cur = m.group(1), []
        elif t and not t.startswith((";", ".")):
            cur.append(t)
            if t.startswith(("s_cbranch", "s_branch", "s_endpgm")):
                out.append((name, cur)); name, cur = name + "'", []
    out.append((name, cur))
    return [(n, c) for n, c in out if c or not n.endswith("'")]


def token(t, first_rx, row_rx):
    op = t.split()[0]
    tok = None
    if op.startswith("s_load_") or op.startswith("s_buffer_load_"):
        tok = "sl%d" % LOADW.get(op.split("_")[-1], 0)
    elif op.startswith(("global_load", "buffer_load", "flat_load")):
        w = LOADW.get(op.split("_")[-1], 1)
        tok = "g" if w == 1 else "g%d" % w
    elif op.startswith(("global_store", "buffer_store", "flat_store")): tok = "S"
    elif op.startswith(("global_atomic", "buffer_atomic", "flat_atomic")): tok = "A"
    elif op.startswith(("ds_read", "ds_load")): tok = "r"
    elif op.startswith(("ds_write", "ds_store")): tok = "w"
    elif op.startswith("ds_"): tok = "ds"
    elif op == "s_waitcnt": tok = "[" + t[len("s_waitcnt"):].strip().replace(" ", "") + "]"
    elif op == "s_barrier": tok = "BAR"
    if tok is None:
        return None
    if row_rx.match(t): tok = tok.upper() + "!"
    elif first_rx.match(t): tok = tok.upper() + "*"
    return tok


def short(name):
    return re.sub(r'^\.LBB\d+_', '', name)


def ways(blocks, first_rx, row_rx, limit, max_groups, ends=False, avoid=()):
    """distinct token sequences entry -> first row request (or the end of the program): depth first, not-taken before taken,
    no block twice on one way; a way with more than max_groups wait groups behind its first request is no head and is dropped
    (states from which every way was dropped are remembered: the walk stays polynomial in a kernel with a long tail)"""
    index = {n: i for i, (n, _) in enumerate(blocks)}
    seen, out, dead = set(), [], set()

    def emit(toks, path):
        if tuple(toks) not in seen:
            seen.add(tuple(toks)); out.append((toks, path))
        return True

    def walk(i, toks, path, onpath, groups, inwait):
        if len(out) >= limit or i >= len(blocks) or i in onpath or (groups < 0 and len(onpath) > 64):
            return False          # (64 blocks without the first request: not a head - and the walk must end)
        state = (i, groups, inwait)
        if state in dead:
            return False
        name, ins = blocks[i]
        if short(name) in avoid:
            return False
        path = path + [name]
        toks, onpath = list(toks), onpath | {i}
        for t in ins:
            tok = token(t, first_rx, row_rx)
            if tok:
                toks.append(tok)
                if tok.endswith("!"):
                    return emit(toks, path)
                if groups >= 0 or tok.endswith("*"):           # counting starts at the first request
                    if tok.startswith("["):
                        groups += 0 if inwait else 1; inwait = True
                    else:
                        groups, inwait = max(groups, 0), False
                    if groups > max_groups:
                        dead.add(state)
                        return False
        last = ins[-1].split() if ins else [""]
        if last[0] == "s_endpgm":
            return emit(toks + ["end"], path) if ends else False
        live = False
        if last[0] != "s_branch":
            live = walk(i + 1, toks, path, onpath, groups, inwait) or live
        if last[0].startswith(("s_cbranch", "s_branch")) and last[-1] in index:
            live = walk(index[last[-1]], toks + ["br"], path, onpath, groups, inwait) or live
        if not live and len(out) < limit:
            dead.add(state)
        return live

    sys.setrecursionlimit(20000)
    walk(0, [], [], frozenset(), -1, False)
    return out


def summary(toks):
    """(waits before the first request or None, wait groups between it and the row request or None)"""
    first = next((i for i, t in enumerate(toks) if t.endswith("*")), None)
    row = next((i for i, t in enumerate(toks) if t.endswith("!")), None)
    if first is None:
        return None, None
    before = sum(1 for t in toks[:first] if t.startswith("["))
    if row is None:
        return before, None
    groups, inwait = 0, False
    for t in toks[first + 1:row]:
        if t.startswith("["):
            groups += 0 if inwait else 1; inwait = True
        elif t != "br":
            inwait = False
    return before, groups


def heads(src, pat, first=RECORD, row=r"global_load_dwordx4", limit=40, max_groups=4, ends=False, avoid=()):
    """[(kernel, [(tokens, blocks, waits_before_first, groups_first_to_row)])] - what the command line prints, for a test"""
    first_rx, row_rx = re.compile(first), re.compile(row)
    res = []
    for name, body in kernel_body(open(src).read(), pat):
        w = ways(blocks_of(body), first_rx, row_rx, limit, max_groups, ends, avoid)
        res.append((name, [(t, p) + summary(t) for t, p in w]))
    return res


def main(argv):
    pos = [a for a in argv if not a.startswith("--")]
    opt = lambda k, d: argv[argv.index(k) + 1] if k in argv else d
    if "--row" in argv: pos.remove(opt("--row", None))
    if "--max" in argv: pos.remove(opt("--max", None))
    if "--groups" in argv: pos.remove(opt("--groups", None))
    if "--avoid" in argv: pos.remove(opt("--avoid", None))
    if len(pos) < 2:
        raise SystemExit(__doc__)
    first = pos[2] if len(pos) > 2 else RECORD
    for name, ws in heads(pos[0], pos[1], first, opt("--row", r"global_load_dwordx4"), int(opt("--max", "40")), int(opt("--groups", "4")), "--ends" in argv,
                          tuple(opt("--avoid", "").split(","))):
        print("==", name)
        if "--distinct" in argv:         # one line per distinct sequence of requests and waits (branches dropped), most frequent first
            seqs = {}
            for toks, path, before, groups in ws:
                key = " ".join(t for t in toks if t != "br")
                n, b, g, blk = seqs.get(key, (0, before, groups, short(path[-1])))
                seqs[key] = (n + 1, b, g, blk)
            for key, (n, b, g, blk) in sorted(seqs.items(), key=lambda kv: -kv[1][0]):
                print("%3d ways  waits before %s  wait groups behind %s  (e.g. to block %s)\n          %s"
                      % (n, "-" if b is None else b, "-" if g is None else g, blk, key))
            continue
        for k, (toks, path, before, groups) in enumerate(ws):
            lab = [short(p) for p in path]
            print("way %-3d waits before first request %s | wait groups first request -> row request %s | blocks %s"
                  % (k, "-" if before is None else before, "-" if groups is None else groups, " ".join(lab)))
            print("        " + " ".join(toks))


if __name__ == "__main__":
    main(sys.argv[1:])
