"""Two plain restatements of `convert` (bam2rad, src/convert.rs:167-594 of the reference), over the record dicts of tests/bam_cases.py.

literal(records, filter_best)  the reference's loop as it is written, line by line, its stale alignment list included: when a run
                               with two N is met the loop `continue`s without clearing tid_list and without updating old_qname.
stated(records, filter_best)   the semantics the project states: a dropped run is dropped, its neighbours are written
                               once each.
Both return the chunks as the reference would write them behind the prelude."""
import struct

MASK = 0x80000000
BUF_LIMIT = 10000
_CODE = {"A": 0, "N": 0, "C": 1, "G": 2, "T": 3}


class Refusal(Exception):
    def __init__(self, what, index):
        super().__init__(f"record {index}: {what}")
        self.what, self.index = what, index


def width_for(n):
    if 1 <= n <= 4:
        return 1
    if n <= 8:
        return 2
    if n <= 16:
        return 4
    if n <= 32:
        return 8
    raise Refusal("length", 0)


def code(s, index):
    """cb_string_to_u64 (convert.rs:75-89): base idx from the end at bit 2 idx; a release build's shift takes the amount mod 64"""
    v = 0
    for idx, ch in enumerate(reversed(s)):
        if ch not in _CODE:
            raise Refusal("unknown nucleotide", index)
        v |= (_CODE[ch] << ((2 * idx) & 63)) & 0xFFFFFFFFFFFFFFFF
    return v


def tag(r, name, index):
    for t, ty, val in r.get("aux", []):
        if t == name:
            if ty != "Z":
                raise Refusal("cannot convert non-string (Z) tag", index)
            return val
    raise Refusal(f"Input record missing {name} tag!", index)


def score_of(r, index):
    for t, ty, val in r.get("aux", []):
        if t == "AS":
            if ty not in "cCsSiI":
                raise Refusal("NO SCORE", index)
            return val - (1 << 32) if ty == "I" and val >= (1 << 31) else val   # `v as i32`
    raise Refusal("NO SCORE", index)


def widths(records):
    if not records:
        raise Refusal("bam file had no records!", 0)
    return width_for(len(tag(records[0], "CR", 0))), width_for(len(tag(records[0], "UR", 0)))


def _low(v, w):
    return (v & ((1 << (8 * w)) - 1)).to_bytes(w, "little")


def literal(records, filter_best):
    bw, uw = widths(records)
    chunks, data, local_nrec = [], bytearray(8), 0
    old_qname, bc, umi, tid_list, score_list = "", 0, 0, [], []

    def write_list():
        mx = max(score_list)
        fl = [t for t, s in zip(tid_list, score_list) if s >= mx]
        data.extend(struct.pack("<I", len(fl)) + _low(bc, bw) + _low(umi, uw) + b"".join(struct.pack("<I", t) for t in fl))

    def dump():
        data[0:8] = struct.pack("<II", len(data), local_nrec)
        chunks.append(bytes(data))

    for index, r in enumerate(records):
        flag = r.get("flag", 0)
        if flag & 0x4 or flag & 0x800:
            continue
        is_reverse = bool(flag & 0x10)
        qname = r["name"]
        tid = r.get("ref", 0)
        if tid < 0:
            raise Refusal("no reference id", index)
        if qname == old_qname:
            if not is_reverse:
                tid |= MASK
            tid_list.append(tid)
            score_list.append(score_of(r, index) if filter_best else 1)
            continue
        if tid_list:
            write_list()
        if local_nrec > BUF_LIMIT:
            dump()
            local_nrec, data = 0, bytearray(8)
        bc_string = tag(r, "CR", index).replace("N", "A", 1)
        umi_string = tag(r, "UR", index).replace("N", "A", 1)
        if "N" in bc_string:
            continue
        if "N" in umi_string:
            continue
        bc, umi = code(bc_string, index), code(umi_string, index)
        old_qname = qname
        tid_list, score_list = [], []
        if not is_reverse:
            tid |= MASK
        score = score_of(r, index) if filter_best else 1
        tid_list.append(tid)
        score_list.append(score)
        local_nrec += 1
    if local_nrec > 0:
        if tid_list:
            write_list()
        dump()
    return chunks


def records_held(chunk, bw, uw):
    """how many records the chunk's nbytes hold, walking na"""
    p, n = 8, 0
    while p < len(chunk):
        na = struct.unpack_from("<I", chunk, p)[0]
        p += 4 + bw + uw + 4 * na
        n += 1
    assert p == len(chunk)
    return n


def stated(records, filter_best, n_ref=1 << 31, lane_alns=16, bw=None, uw=None):
    """-> {"bytes", "chunk_off", "nrec", "stats"}; raises Refusal(what, record index)"""
    if bw is None:
        bw, uw = widths(records)
    kept = []
    for index, r in enumerate(records):
        if r.get("flag", 0) & 0x804:
            continue
        if not 0 <= r.get("ref", 0) < n_ref:
            raise Refusal("reference id out of range", index)
        kept.append((index, r))
    runs = []
    for index, r in kept:
        if runs and runs[-1][-1][1]["name"] == r["name"]:
            runs[-1].append((index, r))
        else:
            runs.append([(index, r)])
    st = dict(n_records=len(records), n_dropped_by_flag=len(records) - len(kept), n_runs=len(runs), n_runs_dropped_n=0, n_runs_written=0, n_alignments_in=0,
              n_alignments_written=0, n_long_runs=0, n_chunks=0, out_bytes=0)
    written = []
    for run in runs:
        hi, head = run[0]
        cr, ur = tag(head, "CR", hi), tag(head, "UR", hi)
        if cr.count("N") >= 2 or ur.count("N") >= 2:
            st["n_runs_dropped_n"] += 1
            continue
        bc, umi = code(cr, hi), code(ur, hi)
        words = [r.get("ref", 0) | (0 if r.get("flag", 0) & 0x10 else MASK) for _, r in run]
        if filter_best:
            scores = [score_of(r, i) for i, r in run]
            words = [w for w, s in zip(words, scores) if s == max(scores)]
        st["n_alignments_in"] += len(run)
        st["n_alignments_written"] += len(words)
        st["n_long_runs"] += len(run) > lane_alns
        written.append(struct.pack("<I", len(words)) + _low(bc, bw) + _low(umi, uw) + b"".join(struct.pack("<I", w) for w in words))
    out, off, nrec = bytearray(), [0], []
    for i in range(0, len(written), BUF_LIMIT + 1):
        body = b"".join(written[i:i + BUF_LIMIT + 1])
        n = len(written[i:i + BUF_LIMIT + 1])
        out += struct.pack("<II", 8 + len(body), n) + body
        off.append(len(out))
        nrec.append(n)
    st.update(n_runs_written=len(written), n_chunks=len(nrec), out_bytes=len(out))
    return {"bytes": bytes(out), "chunk_off": off, "nrec": nrec, "stats": st}
