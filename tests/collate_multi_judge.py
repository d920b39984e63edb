"""Multi-barcode `collate` restated in plain Python on bytes, from the reference's text (do_collate_multi_bc_fast, src/collate.rs:
1415-1920; the unmapped counts, :341-425; the plan's layout, src/correction_plan.rs): the judge of afq_collate_multi_rad and of
afq_collate_multi.  libradicl's collate_multi_barcode is not at hand; where collate.rs leaves a rule to it, DESIGN.md 3.4h's choice
is restated.

  cells      every (sample, barcode) of every sample's permit_freq.bin, by (plate index - the position in sample_info.json's samples -
             ascending, count descending, barcode ascending) (:1611); exactly one output chunk per cell, in that order.
  ordinals   the samples that have a cell, numbered 0, 1, ... in plate order (:1630-1638): the value written into b0.
  kept       a record is kept iff it is compatible with expected_ori (both: always; fw: some alignment word has bit 31 set; rc: some
             has it clear; na == 0 only under both), its b0 is an observed key of the plan's sample corrections whose target is a
             sample of sample_info.json (:1754-1761), and its b1 is an observed key of that sample's cell scope.
  written    na' (the number of fitting alignments), b0 = the sample's ordinal, b1 = the corrected cell barcode, the UMI unchanged,
             the fitting alignment words untouched, in input order.
  order      inside a chunk: input order - by input chunk, then by record.
  empty      a cell that receives no record is a header-only chunk: nbytes 8, nrec 0.
  manifest   one group per sample with cells, in plate order: (canonical barcode, name, chunk_start, its cells, the sum of its
             permit_freq.bin counts) (:1861-1882).

The input records are hopped here, byte by byte."""
import json
import os

BOTH, FW, RC = "both", "fw", "rc"
ORI = {"both": BOTH, "either": BOTH, "fw": FW, "rc": RC, 0: BOTH, 1: FW, 2: RC}
STAT_KEYS = ("n_records", "n_compatible", "n_unrouted", "n_uncorrected", "n_kept", "n_alignments_in", "n_alignments_kept", "n_long_records", "out_bytes")


def u(buf, at, width):
    return int.from_bytes(buf[at:at + width], "little")


def fits(word, ori):
    return ori == BOTH or (word >> 31 == 1) == (ori == FW)


def records(buf, chunk_off, b0_bytes, b1_bytes, umi_bytes, pos_bytes=0):
    """every record of every chunk, in input order: (chunk index, b0, b1, the UMI's bytes, [alignment bytes, ...])"""
    H, A = 4 + b0_bytes + b1_bytes + umi_bytes, 4 + pos_bytes
    for ci, off in enumerate(chunk_off):
        off = int(off)
        nbytes, nrec = u(buf, off, 4), u(buf, off + 4, 4)
        p, end = off + 8, off + nbytes
        for _ in range(nrec):
            na = u(buf, p, 4)
            assert p + H + A * na <= end, ("chunk", ci, "a record runs past the chunk")
            yield (ci, u(buf, p + 4, b0_bytes), u(buf, p + 4 + b0_bytes, b1_bytes), bytes(buf[p + 4 + b0_bytes + b1_bytes:p + H]),
                   [bytes(buf[p + H + A * j:p + H + A * (j + 1)]) for j in range(na)])
            p += H + A * na
        assert p == end, ("chunk", ci, "the records do not tile the chunk")


def collate_multi(buf, chunk_off, b0_bytes, b1_bytes, umi_bytes, expected_ori, sample_table, cell_table, cells, b0_out, pos_bytes=0, lane_alns=None):
    """sample_table: {observed b0: sample}; cell_table: {(sample, observed b1): corrected b1}; cells: [(sample, barcode)] in output order,
    distinct; b0_out: {sample: the value written into b0}.  -> {"bytes", "chunk_off" (n_cells + 1), "nrec" (per cell), "stats"}.
    lane_alns: afq_collate_multi_limits' long-record threshold, for stats["n_long_records"] only."""
    ori = ORI[expected_ori]
    index = {c: i for i, c in enumerate(cells)}
    assert len(index) == len(cells), "cells must be distinct"
    body = [bytearray() for _ in cells]
    nrec = [0] * len(cells)
    st = dict.fromkeys(STAT_KEYS, 0)
    for _, b0, b1, umi, alns in records(buf, chunk_off, b0_bytes, b1_bytes, umi_bytes, pos_bytes):
        st["n_records"] += 1
        st["n_alignments_in"] += len(alns)
        if lane_alns is not None and len(alns) > lane_alns:
            st["n_long_records"] += 1
        keep = [a for a in alns if fits(u(a, 0, 4), ori)]
        if not (ori == BOTH or keep):
            continue
        st["n_compatible"] += 1
        if b0 not in sample_table:
            st["n_unrouted"] += 1
            continue
        s = sample_table[b0]
        if (s, b1) not in cell_table:
            st["n_uncorrected"] += 1
            continue
        cell = index[(s, cell_table[(s, b1)])]
        st["n_kept"] += 1
        st["n_alignments_kept"] += len(keep)
        body[cell] += (len(keep).to_bytes(4, "little") + int(b0_out[s]).to_bytes(b0_bytes, "little") + int(cells[cell][1]).to_bytes(b1_bytes, "little") + umi +
                       b"".join(keep))
        nrec[cell] += 1
    out, offs = bytearray(), []
    for b, n in zip(body, nrec):
        offs.append(len(out))
        out += (len(b) + 8).to_bytes(4, "little") + n.to_bytes(4, "little") + b
    offs.append(len(out))
    st["out_bytes"] = len(out)
    return {"bytes": bytes(out), "chunk_off": offs, "nrec": nrec, "stats": st}


# ---- correction_plan.bin, sample-scoped (correction_plan.rs: magic, u16 version, bincode of CorrectionPlan { sample_barcode_len:
# Option<u8>, cell_barcode_len: u8, sample_spec: Option<CorrectionSpec>, sample_corrections: Vec<(u64, u64)>, cell_scopes: Vec<{
# sample_barcode: Option<u64>, spec, corrections }> }; bincode: u64 lengths, u32 variants, Option as a tag byte) ----
def _spec(buf, at):
    res = u(buf, at + 5, 4)
    assert u(buf, at + 1, 4) <= 1 and res <= 1, "correction plan: unknown neighbourhood or resolution"
    return at + 9 + (24 if res == 1 else 0)


def _pairs(buf, at):
    n = u(buf, at, 8)
    at += 8
    assert at + 16 * n <= len(buf), "correction plan: truncated"
    return [(u(buf, at + 16 * i, 8), u(buf, at + 16 * i + 8, 8)) for i in range(n)], at + 16 * n


def parse_plan(buf):
    """-> {"sample_len", "cell_len", "sample": [(observed, canonical)], "scopes": [(canonical sample barcode, [(observed, corrected)])]}
    in file order; a plan that is not sample-scoped, or does not tile, raises."""
    assert buf[:8] == b"AFCORR\0\0" and u(buf, 8, 2) == 1, "correction plan: bad magic or version"
    assert buf[10] == 1, "correction plan: not sample-scoped"
    sample_len, cell_len, at = buf[11], buf[12], 14
    if buf[13]:
        at = _spec(buf, at)
    sample, at = _pairs(buf, at)
    n_scopes = u(buf, at, 8)
    at += 8
    scopes = []
    for _ in range(n_scopes):
        has = buf[at]
        sb = u(buf, at + 1, 8) if has else None
        at = _spec(buf, at + 1 + (8 if has else 0))
        pp, at = _pairs(buf, at)
        if has:
            scopes.append((sb, pp))
    assert at == len(buf), "correction plan: trailing data"
    return {"sample_len": sample_len, "cell_len": cell_len, "sample": sample, "scopes": scopes}


def _freq(buf):
    n = u(buf, 16, 8)
    assert len(buf) == 24 + 16 * n
    return [(u(buf, 24 + 16 * i, 8), u(buf, 32 + 16 * i, 8)) for i in range(n)]


def _prelude(buf):
    """a RAD prelude as far as collate needs it: (offset of num_chunks, num_chunks, read-tag widths by name, file-tag values, first chunk)"""
    at = 1
    nref = u(buf, at, 8)
    at += 8
    for _ in range(nref):
        at += 2 + u(buf, at, 2)
    nc_at, num_chunks = at, u(buf, at, 8)
    at += 8
    width = {1: 1, 2: 2, 3: 4, 4: 8}
    sections = []
    for _ in range(3):
        n = u(buf, at, 2)
        at += 2
        tags = []
        for _ in range(n):
            ln = u(buf, at, 2)
            tags.append((bytes(buf[at + 2:at + 2 + ln]).decode(), buf[at + 2 + ln]))
            at += 3 + ln
        sections.append(tags)
    vals = {}
    for name, t in sections[0]:
        if t == 8:
            at += 2 + u(buf, at, 2)
        else:
            vals[name] = u(buf, at, width[t])
            at += width[t]
    return nc_at, num_chunks, {n: width[t] for n, t in sections[1]}, vals, at


def tables_from_directory(gpl_dir):
    """the inputs of collate_multi that a GPL output directory determines, and the manifest groups:
    -> {"expected_ori", "num_samples", "sample_table", "cell_table", "cells", "b0_out", "groups", "plan"}"""
    read = lambda *p: open(os.path.join(gpl_dir, *p), "rb").read()
    meta = json.loads(read("generate_permit_list.json"))
    assert meta["multi_barcode"] is True and not meta.get("velo_mode")
    info = json.loads(read("sample_info.json"))
    plate = [(e.get("name"), int(e.get("barcode", "0x0").replace("0x", "") or "0", 16)) for e in info["samples"]]
    plan = parse_plan(read("correction_plan.bin"))
    cells, b0_out, groups = [], {}, []
    for si, (name, bc) in enumerate(plate):
        name = name if name is not None else "%x" % bc
        path = os.path.join(gpl_dir, "sample_" + name, "permit_freq.bin")
        freq = _freq(open(path, "rb").read()) if os.path.exists(path) else []
        if not freq:
            continue
        b0_out[si] = len(groups)
        freq.sort(key=lambda bn: (-bn[1], bn[0]))
        groups.append((bc, name, len(cells), len(freq), sum(n for _, n in freq)))
        cells += [(si, b) for b, _ in freq]
    plate_of = {bc: si for si, (_, bc) in enumerate(plate)}
    sample_table = {o: plate_of[c] for o, c in plan["sample"] if c in plate_of}
    cell_table = {}
    scoped = set()
    for sb, pp in plan["scopes"]:
        if sb in plate_of:
            scoped.add(plate_of[sb])
            for o, c in pp:
                cell_table[(plate_of[sb], o)] = c
    for si in b0_out:
        assert si in scoped, "correction plan has no cell scope for canonical sample 0x%x" % plate[si][1]
    return {"expected_ori": meta["expected_ori"], "num_samples": info["num_samples"], "sample_table": sample_table, "cell_table": cell_table, "cells": cells,
            "b0_out": b0_out, "groups": groups, "plan": plan}


def from_directory(gpl_dir, rad_path, cmdline="", lane_alns=None):
    """what afq_collate_multi writes for a GPL output directory and a mapper's map.rad:
    -> {"rad": the bytes of map.collated.rad, "groups": the manifest's groups, "stats", "collate_json", "unmapped": the bytes of
    unmapped_bc_count_collated.bin, "nrec", "cells", "kept_per_group"}"""
    t = tables_from_directory(gpl_dir)
    buf = open(rad_path, "rb").read()
    nc_at, num_chunks, rw, vals, first = _prelude(buf)
    assert list(rw) == ["b0", "b1", "u"] and vals["num_barcodes"] == 2 and t["plan"]["cell_len"] == vals["b1len"]
    offs, p = [], first
    for _ in range(num_chunks):
        offs.append(p)
        p += u(buf, p, 4)
    out = collate_multi(buf, offs, rw["b0"], rw["b1"], rw["u"], t["expected_ori"], t["sample_table"], t["cell_table"], t["cells"], t["b0_out"], lane_alns=lane_alns)
    head = bytearray(buf[:first])
    head[nc_at:nc_at + 8] = len(t["cells"]).to_bytes(8, "little")
    kept = [sum(out["nrec"][g[2]:g[2] + g[3]]) for g in t["groups"]]
    return {"rad": bytes(head) + out["bytes"], "groups": t["groups"], "stats": out["stats"], "nrec": out["nrec"], "cells": t["cells"], "kept_per_group": kept,
            "collate_json": {"cmd": cmdline, "version_str": "0.18.0", "compressed_output": False, "multi_barcode": True, "num_samples": t["num_samples"],
                             "collation_mode": "optimized", "memory_budget_bytes": 0},
            "unmapped": bytes(8)}
