#!/usr/bin/env python
"""Static figures of the k_walk_slice instantiations in a gfx950 assembly file of csrc/aggregate.hip
(build.py's flags plus `--cuda-device-only -S`):

    python tools/walk_isa_report.py AGGREGATE.s [AGGREGATE.s ...]

Per kernel: VGPRs, SGPRs, scratch, instructions in all, and for the PER-SET LOOP (the outermost loop that holds the
ticket's LDS atomic of the light sets: from the target of the last backward branch behind that atomic to the branch;
it holds the ticket, the wave-walked medium rows handed out by the same ticket stream, the row-pointer and first-pair
requests and the walk of a set) the instruction total and the counts of the addressing and predication instructions.
"drained loads": the global loads of the loop (row pointers: dword, or dwordx2 where the compiler fetches a node's two
neighbouring entries at once; pairs: dwordx2) whose next wait, with no other load in between, is `s_waitcnt vmcnt(0)` -
what a request made a set ahead must not have behind it - by width.
"""
import re
import sys

COUNTED = ["v_lshl_add_u64", "v_ashrrev_i32", "v_mul_lo_u32", "v_mad_u64_u32", "s_and_saveexec_b64", "s_cbranch_execz",
           "s_or_b64 exec", "global_load_dwordx2", "global_load_dword ", "global_load_dwordx4", "global_store",
           "v_cndmask_b32", "v_min_u32", "ds_read_b128", "v_pk_fma_f32", "s_waitcnt vmcnt(0)"]


def kernel_text(lines, name):
    beg = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
    end = next(i for i in range(beg, len(lines)) if lines[i].startswith(".Lfunc_end"))
    d0 = lines.index(".amdhsa_kernel " + name)
    d1 = next(i for i in range(d0, len(lines)) if lines[i] == ".end_amdhsa_kernel")
    body = [l.split(";")[0].strip() for l in lines[beg + 1:end]]
    desc = dict(l.split()[:2] for l in lines[d0 + 1:d1] if l.startswith(".amdhsa_") and len(l.split()) >= 2)
    return [l for l in body if l], desc


def is_inst(l):
    return not l.endswith(":") and not l.startswith(".")


def counts(body):
    out = {k: 0 for k in COUNTED}
    for l in body:
        if not is_inst(l):
            continue
        for k in COUNTED:
            if k == "s_waitcnt vmcnt(0)":
                out[k] += bool(re.match(r"s_waitcnt\b.*vmcnt\(0\)", l))
            elif k == "s_or_b64 exec":
                out[k] += bool(re.match(r"s_or_b64 exec,", l))
            elif l.startswith(k):
                out[k] += 1
    return out


def set_loop(body):
    labels = {l[:-1]: i for i, l in enumerate(body) if l.endswith(":")}
    atom = [i for i, l in enumerate(body) if l.startswith("ds_add_rtn_u32")]
    best = None
    for i, l in enumerate(body):
        m = re.match(r"s_(?:cbranch_\w+|branch)\s+(\S+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            lo = labels[m.group(1)]
            if any(lo < a < i for a in atom) and (best is None or i - lo > best[1] - best[0]):
                best = (lo, i)
    return body[best[0]:best[1] + 1] if best else []


def drained_loads(loop, width):
    n = 0
    for i, l in enumerate(loop):
        if l.startswith("global_load_" + width + " "):
            for k in loop[i + 1:]:
                if k.startswith("global_load") or k.startswith("buffer_load"):
                    break
                if k.startswith("s_waitcnt") and "vmcnt" in k:
                    n += bool(re.search(r"vmcnt\(0\)", k))
                    break
    return n


def main():
    for path in sys.argv[1:]:
        lines = [l.strip() for l in open(path).read().splitlines()]
        names = sorted(l.split()[1] for l in lines if l.startswith(".amdhsa_kernel ") and "k_walk_slice" in l)
        print("== %s" % path)
        for name in names:
            body, desc = kernel_text(lines, name)
            loop = set_loop(body)
            print("%s" % name)
            print("  vgpr %s  sgpr %s  scratch %s  instructions %d  per-set loop %d" % (
                desc.get(".amdhsa_next_free_vgpr"), desc.get(".amdhsa_next_free_sgpr"),
                desc.get(".amdhsa_private_segment_fixed_size"), sum(map(is_inst, body)), sum(map(is_inst, loop))))
            ck, cl = counts(body), counts(loop)
            print("  %-26s %8s %8s" % ("", "kernel", "loop"))
            for k in COUNTED:
                print("  %-26s %8d %8d" % (k.strip(), ck[k], cl[k]))
            print("  drained loads in the loop: dword %d, dwordx2 %d" % (drained_loads(loop, "dword"), drained_loads(loop, "dwordx2")))


if __name__ == "__main__":
    main()
